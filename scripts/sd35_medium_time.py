"""What Stable Diffusion 3.5 medium (MMDiT-X: 13 of 24 blocks with a second, image-only attention) costs per step next to SD3-medium, on
synthetic weights: model evaluations (dk_mmdit_forward with the context hoisted -- the whole of a step but its one update launch) at 512^2 and
1024^2, CFG batch 2, HIP events around back-to-back evaluations in one process, warm, several repeats, the two engines alternating.  The cost
of what a dual block adds -- the second output of the LayerNorm pass, the attn2 qkv GEMM (with its QKNorm), the image-only attention and
attn2.o_proj -- is taken as the difference between one dual and one plain block of the SD3.5-medium engine (dk_mmdit_run_blocks on block 0 and
on block 13: the same copies in and out), times 13, as a share of the evaluation.  The FLOP ratio the two presets predict stands beside it.

    python scripts/sd35_medium_time.py --commit HASH [--out profiles/sd35_medium.md]

One process, no retries: a failure ends the run."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S_T, WARM, EVALS, REPEATS = 154, 3, 5, 5
SIDES = (64, 128)  # latent cells: 512^2 and 1024^2 pixels
B = 2


def eval_flops(cfg, b, s_i, s_t):
    """multiply-adds x 2 of one evaluation's block Linears and attentions (embedders, adaLN and the final layer left out on both sides)"""
    h, r, n = cfg.hidden_size, cfg.mlp_ratio, cfg.depth_multimodal
    stream = (4 + 2 * r) * h * h
    lin = n * 2 * b * s_i * stream + (n - 1) * 2 * b * s_t * stream + 2 * b * s_t * 3 * h * h  # (the last text stream stops after q / k / v)
    lin += cfg.dual_attention_blocks * 2 * b * s_i * 4 * h * h
    att = n * 4 * b * (s_i + s_t) ** 2 * h + cfg.dual_attention_blocks * 4 * b * s_i ** 2 * h
    return lin + att


def measure(args):
    import torch
    from diffusionkit_amd.config import SD3_2b, SD3_5_MEDIUM
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    dev = torch.device("cuda", 0)
    presets = {"SD3_2b": SD3_2b, "SD3_5_MEDIUM": SD3_5_MEDIUM}
    engines = {n: MMDiTEngine(c, pack_mmdit(c, synth_mmdit_weights(c, seed=1234, device=dev), dev, consume=True)) for n, c in presets.items()}
    g = torch.Generator().manual_seed(1)
    text = torch.randn(B, S_T, SD3_2b.token_level_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    pooled = torch.randn(B, SD3_2b.pooled_text_embed_dim, generator=g).to(dev, torch.bfloat16)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    rows = []
    for side in SIDES:
        s_i = (side // 2) ** 2
        lat = torch.randn(B, side, side, 16, generator=g).to(dev)
        fns = {}
        for name, eng in engines.items():
            eng.prepare(B, (side, side), S_T, 1)
            eng.cache_modulation_params(pooled, [1000.0])
            eng.cache_context(text)
            tok = eng.patchify(lat)
            out = torch.empty_like(tok)
            fns[name] = (lambda eng=eng, tok=tok, out=out: eng.forward_tokens(tok, None, 0, tokens_out=out))
        m = engines["SD3_5_MEDIUM"]
        x = (torch.randn(B, S_T + s_i, SD3_5_MEDIUM.hidden_size, generator=g) * 0.5).to(dev, torch.bfloat16)
        n_dual = SD3_5_MEDIUM.dual_attention_blocks
        fns["dual block"] = lambda: m.run_blocks(x, 0, 0)
        fns["plain block"] = lambda: m.run_blocks(x, 0, n_dual)
        for fn in fns.values():
            timed(fn, WARM)
        t = {name: [] for name in fns}
        for _ in range(REPEATS):  # (alternating: drift of the box lands on every row alike)
            for name, fn in fns.items():
                t[name].append(timed(fn, EVALS))
        med = {name: float(np.median(v)) for name, v in t.items()}
        added = n_dual * (med["dual block"] - med["plain block"])
        rows.append((side * 8, med, {k: (min(v), max(v)) for k, v in t.items()}, added,
                     eval_flops(SD3_5_MEDIUM, B, s_i, S_T) / eval_flops(SD3_2b, B, s_i, S_T)))
    lines = ["# SD3.5-medium against SD3-medium: time of one model evaluation", "",
             f"Commit {args.commit}; {torch.cuda.get_device_name(0)}; synthetic weights, bf16, CFG batch {B}, text length {S_T}; medians of {REPEATS} repeats of",
             f"{EVALS} back-to-back evaluations, the rows alternating inside every repeat (`scripts/sd35_medium_time.py`).  An evaluation is",
             "`dk_mmdit_forward` with the context hoisted: a step without its one update launch.  *added launches*: 13 x (one dual block - one plain",
             "block of the SD3.5-medium engine through `dk_mmdit_run_blocks`) -- the LayerNorm pass's second output, the `attn2` qkv GEMM with its",
             "QKNorm, the image-only attention and `attn2.o_proj`.  No SD3.5-medium checkpoint has been run: the weights are random.", "",
             "| image | SD3_2b ms (min - max) | SD3_5_MEDIUM ms (min - max) | time ratio | FLOP ratio predicted | dual block ms | plain block ms | added launches ms | share of the evaluation |",
             "|---|---|---|---|---|---|---|---|---|"]
    for px, med, span, added, fr in rows:
        a, b_ = med["SD3_2b"], med["SD3_5_MEDIUM"]
        lines.append(f"| {px}^2 | {a:.2f} ({span['SD3_2b'][0]:.2f} - {span['SD3_2b'][1]:.2f}) | {b_:.2f} ({span['SD3_5_MEDIUM'][0]:.2f} - "
                     f"{span['SD3_5_MEDIUM'][1]:.2f}) | {b_ / a:.3f} | {fr:.3f} | {med['dual block']:.3f} | {med['plain block']:.3f} | {added:.2f} | "
                     f"{100 * added / b_:.1f} % |")
    text_out = "\n".join(lines) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text_out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sd35_medium.md"))
    ap.add_argument("--commit", default="unknown", help="stamp of the tree that runs (the caller knows it; a copy without .git does not)")
    measure(ap.parse_args())
