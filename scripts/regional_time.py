"""Cost of the group-masked attention launch (regional prompts; profiles/regional_prompts.md): dk_attention_groups_bf16 against the plain launch at
FLUX's attention shape with a base prompt and two half-image regions (H = 24, B = 1, 512 text tokens per prompt) at 1024^2 and 512^2, the class
counts of that layout per (32-query wave, 64-key tile), and the worst per-row ratio against the float64 masked reference on a sample of rows.

    python scripts/regional_time.py [--iters 20]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionkit_amd import ops, regional  # noqa: E402


def tile_classes(words):
    """(skipped, full, mixed) per (wave of 32 queries, tile of 64 keys), and the (128-query block, tile) pairs whose K / V are loaded, of all pairs"""
    S = len(words)
    pad = lambda n: np.concatenate([words, np.zeros(-S % n, dtype=np.uint32)]).reshape(-1, n)
    k_or, k_and = np.bitwise_or.reduce(pad(64), axis=1), np.bitwise_and.reduce(pad(64), axis=1)
    qw = pad(32)
    q_or = np.bitwise_or.reduce(qw, axis=1)
    q_and = np.bitwise_and.reduce(np.where(qw == 0, np.uint32(0xFFFFFFFF), qw), axis=1)
    hit = (q_or[:, None] & k_or[None, :]) != 0
    full = hit & ((q_and[:, None] & k_and[None, :]) != 0)
    b_or = np.bitwise_or.reduce(pad(128), axis=1)
    loaded = (b_or[:, None] & k_or[None, :]) != 0
    return int((~hit).sum()), int(full.sum()), int((hit & ~full).sum()), int(loaded.sum()), loaded.size


def time_us(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(5):  # five batches of ``iters`` back-to-back launches between two events: the wrapper's host work hides behind the queue
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e3 / iters)
    t.sort()
    return t[2], t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    H, D, T = 24, 128, 512
    for side in (1024, 512):
        g = side // 16
        regions = [{"prompt": "l", "box": (0, 0, side // 2, side)}, {"prompt": "r", "box": (side // 2, 0, side, side)}]
        words = regional.region_words(regions, g, g, T)
        S = len(words)
        gen = torch.Generator().manual_seed(1)
        qkv = (torch.randn(1, S, 3 * H * D, generator=gen) * 0.5).to("cuda", torch.bfloat16)
        gw = ops.group_words(words, 1, S, qkv.device)
        plain = time_us(lambda: ops.attention(qkv, H, D), a.iters)
        grouped = time_us(lambda: ops.attention_groups(qkv, H, gw), a.iters)
        ones = ops.group_words(np.full(S, 0xFFFFFFFF, dtype=np.uint32), 1, S, qkv.device)
        allfull = time_us(lambda: ops.attention_groups(qkv, H, ones), a.iters)
        sk, fu, mi, ld, n = tile_classes(words)
        print(f"{side}^2 S={S}: plain {plain[0]:.1f} us (min {plain[1]:.1f}, max {plain[2]:.1f}); grouped {grouped[0]:.1f} us (min {grouped[1]:.1f}, max {grouped[2]:.1f}), "
              f"ratio {grouped[0] / plain[0]:.2f}; grouped with all-ones words (every tile full) {allfull[0]:.1f} us")
        print(f"  (wave, tile) pairs: skipped {sk}, full {fu}, mixed {mi}; (block, tile) pairs loaded {ld} of {n}")
        # accuracy on a sample of rows of head 0: text of each prompt, image rows at the box edge
        out = ops.attention_groups(qkv, H, gw).float().cpu()[0, :, :D].double()
        x = qkv.float().cpu()[0].double()
        q, k, v = x[:, :D], x[:, H * D:H * D + D], x[:, 2 * H * D:2 * H * D + D]
        rows = torch.tensor([0, T, 2 * T + 5, 3 * T, 3 * T + g // 2 - 1, 3 * T + g // 2, S - 1])
        w = torch.from_numpy(words.astype(np.int64))
        mask = (w[rows][:, None] & w[None, :]) != 0
        s = (q[rows] @ k.t() / math.sqrt(D)).masked_fill(~mask, float("-inf"))
        ref = torch.softmax(s, dim=-1) @ v
        err = (torch.linalg.norm(out[rows] - ref, dim=-1) / torch.linalg.norm(ref, dim=-1)).max()
        print(f"  worst relative row error of {len(rows)} sampled rows against float64: {float(err):.2e} (gate constant 7.8e-3)")
    model_evaluation(a.iters)


def model_evaluation(iters):
    """one forward of a FLUX-width model cut to 2 double + 4 single blocks (synthetic weights), S = 4096 + 1536, with and without the words"""
    from dataclasses import replace
    from diffusionkit_amd.config import FLUX_SCHNELL
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    cfg = replace(FLUX_SCHNELL, depth_multimodal=2, depth_unified=4)
    eng = MMDiTEngine(cfg, pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1), "cuda"))
    g = torch.Generator().manual_seed(2)
    eng.prepare(1, (128, 128), 1536, 1)
    eng.cache_modulation_params(torch.randn(1, cfg.pooled_text_embed_dim, generator=g).to("cuda", torch.bfloat16), [500.0])
    tok = eng.patchify(torch.randn(1, 128, 128, 16, generator=g).to("cuda"))
    text = torch.randn(1, 1536, cfg.token_level_text_embed_dim, generator=g).to("cuda", torch.bfloat16)
    out = torch.empty_like(tok)
    plain = time_us(lambda: eng.forward_tokens(tok, text, 0, out), iters)
    eng.set_attention_groups(regional.region_words([{"prompt": "l", "box": (0, 0, 512, 1024)}, {"prompt": "r", "box": (512, 0, 1024, 1024)}], 64, 64, 512))
    grouped = time_us(lambda: eng.forward_tokens(tok, text, 0, out), iters)
    print(f"model evaluation, 2 double + 4 single FLUX-width blocks, S = 5632: plain {plain[0] / 1e3:.2f} ms, with regions {grouped[0] / 1e3:.2f} ms "
          f"(+{(grouped[0] - plain[0]) / 6:.0f} us per block)")


if __name__ == "__main__":
    main()
