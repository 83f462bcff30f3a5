"""What perturbed-attention guidance costs (synthetic weights, times only), two tables in one process:

1. The identity-attention launch (``ops.attention_identity``, ident_from = 154) against the plain lean launch (``ops.attention`` under
   ``tune("attn", 4)``) on the same operands: SD3-medium's attention shape, H = 24, D = 64, S_t = 154, S_i = 1024 and 4096, B = 1 and 2.  The tile
   walk predicts the ratio: a block of 128 image queries walks ceil(154 / 64) + 2 = 5 key tiles instead of 19 (S_i = 1024) or 67 (S_i = 4096); the
   two blocks that hold a text query walk every tile.  The launches alternate inside every repeat.
2. One model evaluation of the SD3-medium preset (dk_mmdit_forward with the context hoisted) at 512^2 and 1024^2: on 2 rows (the CFG batch), on 1
   row (what a separate third call would evaluate) and on 3 rows with the last one forked in front of block 13 and perturbed there
   (``MMDiTEngine.set_perturbed_attention((13,), 1)``).  The fork row runs 24 - 13 = 11 of 24 blocks.

    python scripts/pag_time.py --commit HASH [--out profiles/perturbed_attention.md]

One process, no retries: a failure ends the run.  No checkpoint has been run: the weights and operands are random."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S_T, H, D = 154, 24, 64
WARM, EVALS, REPEATS = 3, 5, 5
SIDES = (64, 128)  # latent cells: 512^2 and 1024^2 pixels
LAYERS = (13,)


def tiles(S, F):
    """(key tiles the identity launch walks, key tiles the plain launch walks), summed over the 128-query blocks of one head"""
    nt, walked = (S + 63) // 64, 0
    for q0 in range(0, S, 128):
        walked += nt if q0 < F else (F + 63) // 64 + min(2, nt - q0 // 64)
    return walked, nt * ((S + 127) // 128)


def measure(args):
    import torch
    from diffusionkit_amd import ops
    from diffusionkit_amd.config import SD3_2b as cfg
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def rounds(fns, evals):
        for fn in fns.values():
            timed(fn, WARM)
        t = {name: [] for name in fns}
        for _ in range(REPEATS):  # (alternating: drift of the box lands on every row alike)
            for name, fn in fns.items():
                t[name].append(timed(fn, evals))
        return {k: float(np.median(v)) for k, v in t.items()}, {k: (min(v), max(v)) for k, v in t.items()}

    lines = ["# Perturbed-attention guidance: the identity launch and the forked evaluation", "",
             f"Commit {args.commit}; {torch.cuda.get_device_name(0)}; synthetic weights and operands, bf16, text length {S_T}; medians of {REPEATS} repeats,",
             "the rows of a table alternating inside every repeat, HIP events around back-to-back launches in one process (`scripts/pag_time.py`).",
             "No pass mark beyond the one-half line of the first table.  No checkpoint has been run.", "",
             "## The identity launch against the plain lean launch", "",
             f"H = {H}, D = {D}, ident_from = {S_T}; {20} launches per timing.  *tiles*: 64-key tiles walked per head, identity / plain, and their ratio -- the",
             "prediction.", "",
             "| S_i | B | plain us (min - max) | identity us (min - max) | identity / plain | tiles | predicted |", "|---|---|---|---|---|---|---|"]
    ops.tune("attn", 4)
    try:
        for S_i in (1024, 4096):
            for B in (1, 2):
                S = S_T + S_i
                qkv = torch.randn(B, S, 3 * H * D, generator=g).to(dev, torch.bfloat16)
                med, span = rounds({"plain": lambda: ops.attention(qkv, H, D), "identity": lambda: ops.attention_identity(qkv, H, D, S_T)}, 20)
                w, p = tiles(S, S_T)
                cell = lambda k: f"{1e3 * med[k]:.1f} ({1e3 * span[k][0]:.1f} - {1e3 * span[k][1]:.1f})"  # noqa: E731
                lines.append(f"| {S_i} | {B} | {cell('plain')} | {cell('identity')} | {med['identity'] / med['plain']:.3f} | {w} / {p} | {w / p:.3f} |")
    finally:
        ops.tune("attn", -1)

    packed = pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234, device=dev), dev, consume=True)
    rows_of = {"2 rows": 2, "1 row": 1, "3 rows, forked": 3}
    engines = {name: MMDiTEngine(cfg, packed) for name in rows_of}
    engines["3 rows, forked"].set_perturbed_attention(LAYERS, 1)
    text = torch.randn(2, S_T, cfg.token_level_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    pooled = torch.randn(2, cfg.pooled_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    group = lambda t, b: t[:b] if b < 3 else torch.cat([t, t[:1]], 0)  # noqa: E731  ([prompt | negative | prompt])
    depth, first = cfg.depth_multimodal, min(LAYERS)
    share = (depth - first) / depth
    lines += ["", "## One model evaluation, SD3-medium preset, block 13 perturbed", "",
              "An evaluation is `dk_mmdit_forward` with the context hoisted: a step without its one update launch.  *3 rows, forked*:",
              f"`set_perturbed_attention({LAYERS}, 1)`, the third row a copy of the first that joins in front of block {first} and runs its attention there as the",
              f"identity launch.  *extra*: forked minus the 2-row evaluation.  *predicted*: {depth - first}/{depth} of the 1-row time, from block counts alone;",
              "*separate call*: the 1-row time, what a third model call would add.", "",
              "| image | 2 rows ms (min - max) | 1 row ms (min - max) | 3 rows, forked ms (min - max) | extra ms | predicted ms | extra / predicted | separate call ms |",
              "|---|---|---|---|---|---|---|---|"]
    for side in SIDES:
        lat = torch.randn(1, side, side, 16, generator=g).to(dev)
        fns = {}
        for name, eng in engines.items():
            b = rows_of[name]
            eng.prepare(b, (side, side), S_T, 1)
            eng.cache_modulation_params(group(pooled, b).contiguous(), [1000.0])
            eng.cache_context(group(text, b).contiguous())
            tok = eng.patchify(lat, dup=b)
            out = torch.empty_like(tok)
            fns[name] = (lambda eng=eng, tok=tok, out=out: eng.forward_tokens(tok, None, 0, tokens_out=out))
        med, span = rounds(fns, EVALS)
        extra, pred = med["3 rows, forked"] - med["2 rows"], share * med["1 row"]
        cell = lambda k: f"{med[k]:.2f} ({span[k][0]:.2f} - {span[k][1]:.2f})"  # noqa: E731
        lines.append(f"| {side * 8}^2 | {cell('2 rows')} | {cell('1 row')} | {cell('3 rows, forked')} | {extra:.2f} | {pred:.2f} | {extra / pred:.2f} | "
                     f"{med['1 row']:.2f} |")
    text_out = "\n".join(lines) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text_out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "perturbed_attention.md"))
    ap.add_argument("--commit", default="unknown", help="stamp of the tree that runs (the caller knows it; a copy without .git does not)")
    measure(ap.parse_args())
