"""Per-launch time of the W4A6 GEMM (MX-fp4 weights x MX-fp6 activations, csrc/gemm256f4a6.hip) against W4A8 (csrc/gemm256f4.hip), the fp8 GEMM
(csrc/gemm256f8.hip) and the bf16 GEMM (ops.linear) on the LayerNorm-fed block Linears of FLUX (qkv, fc1 of the double blocks, linear1 of the
single blocks) at the 512^2 and 1024^2 token counts, of the two row quantisers, and of one 6-block FLUX-width model evaluation on the fp4 engine with
MX-fp8 and MX-fp6 activations, with the dB of both against the fp32 oracle on the same synthetic weights.
    python scripts/mxfp6_time.py > profiles/mxfp6_time.log
Warm weights: the same operands every launch; cold: a ring of weight copies larger than the last-level cache.  Device events around batches of
launches, the median of 7 batches after a warm-up batch; the four kernels take turns inside one process, W4A8 runs a second time at the end."""
import os
import sys
from dataclasses import replace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionkit_amd import ops  # noqa: E402
from diffusionkit_amd.weights import pack_mxfp4, quantize_weight_e4m3, quantize_weight_mxfp4  # noqa: E402

BF = torch.bfloat16
dev = torch.device("cuda")


def timed(fn, n=20, batches=7):
    fn()
    torch.cuda.synchronize()
    ts = []
    for b in range(batches + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        if b:
            ts.append(e0.elapsed_time(e1) * 1e3 / n)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def gemms():
    h = 3072
    print(f"device {torch.cuda.get_device_name(0)}; us per launch: median (min .. max) of 7 batches of 20")
    for name, M, N in (("qkv 512^2 image", 1024, 3 * h), ("fc1 512^2 image", 1024, 4 * h), ("linear1 512^2", 1024 + 512, 7 * h),
                       ("qkv 1024^2 image", 4096, 3 * h), ("fc1 1024^2 image", 4096, 4 * h), ("linear1 1024^2", 4096 + 512, 7 * h)):
        K = h
        x = torch.randn(M, K, device=dev, dtype=BF)
        a8, s8 = ops.quantize_mx8(x)
        a6, s6 = ops.quantize_rows_mx6(x)
        n_w = max(2, int(600e6 // (N * K // 2)))  # cold: > 512 MiB of MX-fp4 weights go round (so more of fp8 and bf16)
        ws = []
        for r in range(n_w):
            w = (torch.randn(N, K, device=dev) * 0.02).to(BF)
            code, e8, wsc = quantize_weight_mxfp4(w)
            q8, ws8 = quantize_weight_e4m3(w)
            ws.append((pack_mxfp4(code, e8) + (wsc,), (q8, ws8), w))
        bias = torch.zeros(N, device=dev, dtype=BF)
        out = torch.empty(M, N, device=dev, dtype=BF)
        for temp in ("warm", "cold"):
            pick = (lambda i=0: ws[0]) if temp == "warm" else (lambda i=0: ws[i % n_w])
            runs = (("W4A8", lambda i=0: ops.gemm_fp4(a8, s8, *pick(i)[0], bias=bias, M=M, k=K, out=out)),
                    ("W4A6", lambda i=0: ops.gemm_fp4(a6, s6, *pick(i)[0], bias=bias, M=M, k=K, out=out, activations="mxfp6")),
                    ("fp8", lambda i=0: ops.gemm_fp8(a8, s8, *pick(i)[1], bias=bias, M=M, k=K, out=out)),
                    ("bf16", lambda i=0: ops.linear(x, pick(i)[2], bias, out=out)),
                    ("W4A8 again", lambda i=0: ops.gemm_fp4(a8, s8, *pick(i)[0], bias=bias, M=M, k=K, out=out)))
            t = {k: timed(f) for k, f in runs}
            line = "  ".join(f"{k} {v[0]:7.1f} ({v[1]:.1f} .. {v[2]:.1f})" for k, v in t.items())
            print(f"{name:18s} M={M:5d} N={N:5d} K={K} {temp}: {line}  W4A6 / min W4A8 {t['W4A6'][0] / min(t['W4A8'][0], t['W4A8 again'][0]):.3f}", flush=True)
        q8 = timed(lambda i=0: ops.quantize_mx8(x, out=a8, scales=s8))
        q6 = timed(lambda i=0: ops.quantize_rows_mx6(x, out=a6, scales=s6))
        print(f"{'  row quantiser':18s} M={M:5d} h={K}: mx8 {q8[0]:6.1f} ({q8[1]:.1f} .. {q8[2]:.1f})  mx6 {q6[0]:6.1f} ({q6[1]:.1f} .. {q6[2]:.1f})", flush=True)
        del ws


def psnr(ref, got):
    ref, got = np.asarray(ref.double().cpu()).ravel(), np.asarray(got.double().cpu()).ravel()
    return float(20 * np.log10((np.abs(ref).max() + 1e-5) / (np.sqrt(np.mean((ref - got) ** 2)) + 1e-10)))


def model_evaluation():
    """a FLUX-width model cut to 2 double + 4 single blocks (synthetic weights) on the fp4 "speed" engine: one forward at S = 4096 + 512 with MX-fp8 and
    with MX-fp6 activations, taking turns; then at S = 1024 + 512 the dB of both against the fp32 oracle (CPU) on the same weights"""
    from diffusionkit_amd.config import FLUX_SCHNELL, fp4_config
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    from oracle.mmdit import OracleMMDiT, Prec
    base = replace(FLUX_SCHNELL, depth_multimodal=2, depth_unified=4)
    cfgs = {a: fp4_config(base, "speed", activations=a) for a in ("mxfp8", "mxfp6")}
    named = synth_mmdit_weights(cfgs["mxfp8"], seed=1)
    packed = pack_mmdit(cfgs["mxfp8"], named, "cuda")
    g = torch.Generator().manual_seed(2)
    pooled = torch.randn(1, base.pooled_text_embed_dim, generator=g)
    text = torch.randn(1, 512, base.token_level_text_embed_dim, generator=g)
    ts = [500.0]
    for side, what in ((128, "time"), (64, "dB")):
        lat = torch.randn(1, side, side, 16, generator=g)
        fns, outs = {}, {}
        for a, cfg in cfgs.items():
            eng = MMDiTEngine(cfg, packed)
            eng.prepare(1, (side, side), 512, 1)
            eng.cache_modulation_params(pooled.to("cuda", BF), ts)
            tok = eng.patchify(lat.to("cuda"))
            fns[a] = lambda i=0, eng=eng, tok=tok, out=torch.empty_like(tok): eng.forward_tokens(tok, text.to("cuda", BF), 0, out)
            outs[a] = fns[a]().float().cpu().clone()
        if what == "time":
            t = {}
            for k in ("mxfp8", "mxfp6", "mxfp8 again"):
                t[k] = timed(fns[k.split()[0]], n=5)
            print("model evaluation, 2 double + 4 single FLUX-width fp4 blocks, S = 4608, ms: " +
                  "  ".join(f"{k} {v[0] / 1e3:.3f} ({v[1] / 1e3:.3f} .. {v[2] / 1e3:.3f})" for k, v in t.items()), flush=True)
        else:
            m = OracleMMDiT(cfgs["mxfp8"], {k: v.float() for k, v in named.items()}, Prec())
            m.cache_modulation_params(pooled, torch.tensor(ts))
            taps = {}
            m(lat, text, ts[0], taps=taps)
            print(f"the same model at S = 1536 against the fp32 oracle: W4A8 {psnr(taps['final'], outs['mxfp8']):.2f} dB, W4A6 {psnr(taps['final'], outs['mxfp6']):.2f} dB; "
                  f"W4A6 against W4A8 {psnr(outs['mxfp8'], outs['mxfp6']):.2f} dB", flush=True)


if __name__ == "__main__":
    gemms()
    model_evaluation()
