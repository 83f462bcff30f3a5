"""What a reference image costs per denoising step: FLUX-width model evaluations (dk_mmdit_forward, the whole of a step but its one update launch)
at 1024^2 and 512^2, without a reference and with a reference of the image's own size, HIP events around back-to-back evaluations in one
process, warm, several repeats, the configurations alternating.

    python scripts/reference_image_time.py --out run.json [--commit HASH] [--no-reference]
    python scripts/reference_image_time.py --table parent=a.json this=b.json ... > profiles/reference_image.md

``--no-reference`` measures the no-reference rows only and touches nothing this option added, so the same file also runs in a checkout of the
parent commit: the yardstick for "off means off".  The model is FLUX.1-schnell's geometry with synthetic weights (FLUX.1 Kontext is FLUX.1-dev's:
the same blocks; its guidance embedding is outside the step)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S_T, WARM, EVALS, REPEATS = 256, 3, 6, 5
SIZES = {"1024": (128, 128), "512": (64, 64)}


def measure(args):
    import torch
    from diffusionkit_amd.config import FLUX_SCHNELL
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    dev = torch.device("cuda", 0)
    cfg = FLUX_SCHNELL
    eng = MMDiTEngine(cfg, pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234, device=dev), dev, consume=True))
    g = torch.Generator().manual_seed(1)
    text = torch.randn(1, S_T, cfg.token_level_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    pooled = torch.randn(1, cfg.pooled_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    rows = [(size, False) for size in SIZES] + ([] if args.no_reference else [(size, True) for size in SIZES])
    res = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "text_len": S_T, "evals_per_repeat": EVALS, "rows": {}}

    def run(size, ref):
        hl, wl = SIZES[size]
        if ref:
            eng.prepare(1, (hl, wl), S_T, 1, reference_size=(hl, wl))
        else:
            eng.prepare(1, (hl, wl), S_T, 1)
        eng.cache_modulation_params(pooled, [1000.0])
        eng.cache_context(text)
        if ref:
            eng.cache_reference(torch.randn(1, hl, wl, 16, generator=g).to(dev), per_image=False)
        tok = eng.patchify(torch.randn(1, hl, wl, 16, generator=g).to(dev))
        out = torch.empty_like(tok)
        for _ in range(WARM):
            eng.forward_tokens(tok, None, 0, tokens_out=out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(EVALS):
            eng.forward_tokens(tok, None, 0, tokens_out=out)
        e1.record()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.float()).all())
        return e0.elapsed_time(e1) / EVALS

    for size, ref in rows:
        run(size, ref)  # (first touch of every shape: not recorded)
    times = {r: [] for r in rows}
    for _ in range(REPEATS):  # (alternating: drift of the box lands on every row alike)
        for r in rows:
            times[r].append(round(run(*r), 3))
    for (size, ref), t in times.items():
        s_i = (SIZES[size][0] // 2) * (SIZES[size][1] // 2)
        res["rows"][f"{size}{'+ref' if ref else ''}"] = {"ms": t, "median_ms": round(float(np.median(t)), 3), "min_ms": min(t), "max_ms": max(t),
                                                        "S": S_T + s_i * (2 if ref else 1)}
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


def table(pairs):
    runs = [(p.split("=", 1)[0], json.load(open(p.split("=", 1)[1]))) for p in pairs]
    print("| run | commit | row | joint rows S | median ms | min - max ms |")
    print("|---|---|---|---|---|---|")
    for label, r in runs:
        for name, row in r["rows"].items():
            print(f"| {label} | {r['commit']} | {name} | {row['S']} | {row['median_ms']:.2f} | {row['min_ms']:.2f} - {row['max_ms']:.2f} |")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown", help="stamp of the tree that runs (the caller knows it; a copy without .git does not)")
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--table", nargs="+", metavar="LABEL=JSON", default=None)
    a = ap.parse_args()
    table(a.table) if a.table else measure(a)
