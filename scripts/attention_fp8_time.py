"""Cost of the quantised attention launch (profiles/attention_fp8.md): dk_attention_fp8_bf16 (pre-pass + attention kernel, one figure: the two
launches of a call) against the default bf16 route on the same device, in alternating order, at FLUX's attention shapes (H = 24, D = 128), and the
worst per-row error of both against float64 on a sample of rows of head 0; then one 6-block FLUX-width model evaluation with the option off and on.

    python scripts/attention_fp8_time.py [--iters 20]
"""
import argparse
import math
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionkit_amd import ops  # noqa: E402


def batch_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(fns, iters, rounds=5):
    """median, min, max of ``rounds`` event-timed batches per function, the functions taking turns (warm: three calls each first)"""
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for r in range(rounds):
        for i in (range(len(fns)) if r % 2 == 0 else reversed(range(len(fns)))):
            t[i].append(batch_us(fns[i], iters))
    return [(sorted(x)[rounds // 2], min(x), max(x)) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rev = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown (no git)"
    print(f"commit {rev} (+ working tree), {torch.cuda.get_device_name(0)}")
    H, D = 24, 128
    for what, B, S in (("FLUX 1024^2", 1, 4608), ("FLUX 512^2", 1, 1280), ("FLUX 1024^2 B=4", 4, 4608)):
        gen = torch.Generator().manual_seed(1)
        qkv = (torch.randn(B, S, 3 * H * D, generator=gen) * 0.5).to("cuda", torch.bfloat16)
        ws = torch.empty(ops.attention_fp8_workspace_bytes(B, H, S), dtype=torch.uint8, device="cuda")
        out = torch.empty(B, S, H * D, dtype=torch.bfloat16, device="cuda")
        plain, fp8 = alternate([lambda: ops.attention(qkv, H, D), lambda: ops.attention_fp8(qkv, H, workspace=ws, out=out)], a.iters)
        flop = 4.0 * B * H * S * S * D
        print(f"{what} (B={B}, S={S}): bf16 default route {plain[0]:.1f} us (min {plain[1]:.1f}, max {plain[2]:.1f}; {flop / plain[0] / 1e6:.0f} TFLOP/s); "
              f"fp8 pre-pass + kernel {fp8[0]:.1f} us (min {fp8[1]:.1f}, max {fp8[2]:.1f}; {flop / fp8[0] / 1e6:.0f} TFLOP/s); ratio {fp8[0] / plain[0]:.2f}")
        x = qkv[0].float().cpu().double()
        q, k, v = x[:, :D], x[:, H * D:H * D + D], x[:, 2 * H * D:2 * H * D + D]
        rows = torch.tensor([0, 1, S // 3, S // 2 + 1, S - 2, S - 1])
        ref = torch.softmax(q[rows] @ k.t() / math.sqrt(D), dim=-1) @ v
        for name, y in (("bf16", ops.attention(qkv, H, D)), ("fp8", ops.attention_fp8(qkv, H, workspace=ws))):
            y = y[0, :, :D].float().cpu().double()[rows]
            print(f"  {name}: worst relative row error of {len(rows)} sampled rows of head 0 against float64 {float((torch.linalg.norm(y - ref, dim=-1) / torch.linalg.norm(ref, dim=-1)).max()):.2e}")
    model_evaluation(a.iters)


def model_evaluation(iters):
    """one forward of a FLUX-width model cut to 2 double + 4 single blocks (synthetic weights), S = 4096 + 512, with the option off and on"""
    from dataclasses import replace
    from diffusionkit_amd.config import FLUX_SCHNELL
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    cfg = replace(FLUX_SCHNELL, depth_multimodal=2, depth_unified=4)
    packed = pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1), "cuda")
    g = torch.Generator().manual_seed(2)
    pooled = torch.randn(1, cfg.pooled_text_embed_dim, generator=g).to("cuda", torch.bfloat16)
    lat = torch.randn(1, 128, 128, 16, generator=g).to("cuda")
    text = torch.randn(1, 512, cfg.token_level_text_embed_dim, generator=g).to("cuda", torch.bfloat16)
    fns = []
    for dtype in ("bfloat16", "fp8_e4m3"):
        eng = MMDiTEngine(replace(cfg, attention_dtype=dtype), packed)
        eng.prepare(1, (128, 128), 512, 1)
        eng.cache_modulation_params(pooled, [500.0])
        tok = eng.patchify(lat)
        fns.append(lambda eng=eng, tok=tok, out=torch.empty_like(tok): eng.forward_tokens(tok, text, 0, out))
    plain, fp8 = alternate(fns, max(1, iters // 4))
    print(f"model evaluation, 2 double + 4 single FLUX-width blocks, S = 4608: bf16 attention {plain[0] / 1e3:.2f} ms (min {plain[1] / 1e3:.2f}, max {plain[2] / 1e3:.2f}), "
          f"fp8 attention {fp8[0] / 1e3:.2f} ms (min {fp8[1] / 1e3:.2f}, max {fp8[2] / 1e3:.2f}): +{(fp8[0] - plain[0]) / 6:.0f} us per block")


if __name__ == "__main__":
    main()
