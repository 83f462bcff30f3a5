"""What the forked third row group of skip-layer guidance costs on Stable Diffusion 3.5 medium (synthetic weights): one model evaluation
(dk_mmdit_forward with the context hoisted -- a step without its update launch) at 512^2 and 1024^2 on 2 rows (the CFG batch of every step),
on 1 row (what a separate third call would evaluate) and on 3 rows with the last one forked in front of block 7 and sitting out blocks 7, 8, 9
(``MMDiTEngine.set_skip_layers((7, 8, 9), 1)``, the published recipe).  Three engines over one set of packed weights, HIP events around
back-to-back evaluations in one process, warm, several repeats, the rows alternating inside every repeat.

The prediction, from block counts alone: the fork row runs 24 - 7 - 3 = 14 of 24 blocks, so the extra time over the 2-row evaluation is about
14/24 of the 1-row time, against 21/24 for a separate third call that skips the three blocks.  It is reported beside the measured value.

    python scripts/slg_time.py --commit HASH [--out profiles/skip_layer_guidance.md]

One process, no retries: a failure ends the run.  No SD3.5-medium checkpoint has been run: the weights are random, the figures are times only."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S_T, WARM, EVALS, REPEATS = 154, 3, 5, 5
SIDES = (64, 128)  # latent cells: 512^2 and 1024^2 pixels
LAYERS = (7, 8, 9)


def measure(args):
    import torch
    from diffusionkit_amd.config import SD3_5_MEDIUM as cfg
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    dev = torch.device("cuda", 0)
    packed = pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234, device=dev), dev, consume=True)
    rows_of = {"2 rows": 2, "1 row": 1, "3 rows, forked": 3}
    engines = {name: MMDiTEngine(cfg, packed) for name in rows_of}
    engines["3 rows, forked"].set_skip_layers(LAYERS, 1)
    g = torch.Generator().manual_seed(1)
    text = torch.randn(2, S_T, cfg.token_level_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    pooled = torch.randn(2, cfg.pooled_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    group = lambda t, b: t[:b] if b < 3 else torch.cat([t, t[:1]], 0)  # noqa: E731  ([prompt | negative | prompt])

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    depth, first = cfg.depth_multimodal, min(LAYERS)
    share_fork, share_call = (depth - first - len(LAYERS)) / depth, (depth - len(LAYERS)) / depth
    out_rows = []
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
        for fn in fns.values():
            timed(fn, WARM)
        t = {name: [] for name in fns}
        for _ in range(REPEATS):  # (alternating: drift of the box lands on every row alike)
            for name, fn in fns.items():
                t[name].append(timed(fn, EVALS))
        out_rows.append((side * 8, {k: float(np.median(v)) for k, v in t.items()}, {k: (min(v), max(v)) for k, v in t.items()}))
    lines = ["# Skip-layer guidance: time of the forked third row group", "",
             f"Commit {args.commit}; {torch.cuda.get_device_name(0)}; SD3.5-medium, synthetic weights, bf16, text length {S_T}; medians of {REPEATS} repeats of",
             f"{EVALS} back-to-back evaluations, the rows alternating inside every repeat (`scripts/slg_time.py`).  An evaluation is `dk_mmdit_forward`",
             "with the context hoisted: a step without its one update launch.  *3 rows, forked*: `set_skip_layers((7, 8, 9), 1)`, the third row a copy of",
             "the first that joins in front of block 7 and sits out blocks 7, 8, 9.  *extra*: forked minus the 2-row evaluation.  *predicted*: 14/24 of the",
             "1-row time, from block counts alone (the fork row runs 14 of 24 blocks); *separate call*: 21/24 of the 1-row time, what a third model call",
             "that skips the three blocks would add.  No pass mark.  No SD3.5-medium checkpoint has been run: the weights are random.", "",
             "| image | 2 rows ms (min - max) | 1 row ms (min - max) | 3 rows, forked ms (min - max) | extra ms | predicted ms | extra / predicted | separate call ms |",
             "|---|---|---|---|---|---|---|---|"]
    for px, med, span in out_rows:
        extra, pred = med["3 rows, forked"] - med["2 rows"], share_fork * med["1 row"]
        cell = lambda k: f"{med[k]:.2f} ({span[k][0]:.2f} - {span[k][1]:.2f})"  # noqa: E731
        lines.append(f"| {px}^2 | {cell('2 rows')} | {cell('1 row')} | {cell('3 rows, forked')} | {extra:.2f} | {pred:.2f} | {extra / pred:.2f} | "
                     f"{share_call * med['1 row']:.2f} |")
    text_out = "\n".join(lines) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text_out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "skip_layer_guidance.md"))
    ap.add_argument("--commit", default="unknown", help="stamp of the tree that runs (the caller knows it; a copy without .git does not)")
    measure(ap.parse_args())
