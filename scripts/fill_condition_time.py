"""What channel-concatenated conditioning (FLUX.1 Fill's width, 320 condition features) costs: FLUX-width model evaluations (dk_mmdit_forward,
the whole of a step but its one update launch) at 1024^2 without and with the condition, HIP events around back-to-back evaluations in one
process, warm, several repeats, the two engines alternating; and the once-per-call work -- masking the image out, the VAE encode, the token
build and dk_mmdit_cache_condition -- timed the same way.

    python scripts/fill_condition_time.py --out run.json [--commit HASH]
    python scripts/fill_condition_time.py --table a.json [b.json ...] > table.md

The model is FLUX.1-schnell's geometry with synthetic weights (FLUX.1 Fill is FLUX.1-dev's: the same blocks; its guidance embedding is outside
the step).  Both engines share every weight tensor but x_embedder's: the plain engine binds the first 64 columns of the wide one."""
import argparse
import json
import os
import sys
from dataclasses import replace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S_T, WARM, EVALS, REPEATS = 256, 3, 6, 5
HL = WL = 128  # 1024^2 pixels
WIDTH = 320


def measure(args):
    import torch
    from diffusionkit_amd import ops
    from diffusionkit_amd.config import FLUX_SCHNELL, VAEEncoderConfig
    from diffusionkit_amd.engine import MMDiTEngine, VAEEncoderEngine
    from diffusionkit_amd.weights import pack_mmdit, pack_vae, synth_mmdit_weights, synth_vae_encoder_weights
    dev = torch.device("cuda", 0)
    wide_cfg = replace(FLUX_SCHNELL, condition_features=WIDTH)
    wide = pack_mmdit(wide_cfg, synth_mmdit_weights(wide_cfg, seed=1234, device=dev), dev, consume=True)
    plain = dict(wide)
    plain["x_embedder.proj.weight"] = wide["x_embedder.proj.weight"][:, :FLUX_SCHNELL.patch_dim].contiguous()
    engines = {"plain": MMDiTEngine(FLUX_SCHNELL, plain), "fill": MMDiTEngine(wide_cfg, wide)}
    ecfg = VAEEncoderConfig()
    encoder = VAEEncoderEngine(ecfg, pack_vae(ecfg, synth_vae_encoder_weights(ecfg, seed=1236, device="cpu"), dev))
    g = torch.Generator().manual_seed(1)
    text = torch.randn(1, S_T, FLUX_SCHNELL.token_level_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    pooled = torch.randn(1, FLUX_SCHNELL.pooled_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    lat = torch.randn(1, HL, WL, 16, generator=g).to(dev)
    image = torch.randint(0, 256, (1, 8 * HL, 8 * WL, 3), generator=g, dtype=torch.uint8).to(dev)
    mask = torch.randint(0, 256, (1, 8 * HL, 8 * WL), generator=g, dtype=torch.uint8).to(dev)
    zeros = torch.zeros(1, HL, WL, ecfg.out_channels // 2, dtype=torch.float32, device=dev)
    res = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "text_len": S_T, "evals_per_repeat": EVALS, "width": WIDTH, "rows": {}}

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def condition_tokens():
        z = encoder.sample(encoder.encode(ops.image_mask_out(image, mask)), zeros)
        return ops.fill_condition_tokens(z, mask)

    state = {}
    for name, eng in engines.items():
        eng.prepare(1, (HL, WL), S_T, 1)
        eng.cache_modulation_params(pooled, [1000.0])
        eng.cache_context(text)
        if name == "fill":
            state["cond"] = condition_tokens()
            eng.cache_condition(state["cond"], per_image=False)
        tok = eng.patchify(lat)
        state[name] = (tok, torch.empty_like(tok))

    def step(name):
        tok, out = state[name]
        return lambda: engines[name].forward_tokens(tok, None, 0, tokens_out=out)

    once = {"mask-out + encode + tokens": condition_tokens,
            "token build alone": lambda: ops.fill_condition_tokens(zeros, mask),
            "cache_condition": lambda: engines["fill"].cache_condition(state["cond"], per_image=False)}
    for name in engines:
        timed(step(name), WARM)
    for fn in once.values():
        timed(fn, WARM)
    times = {name: [] for name in (*engines, *once)}
    for _ in range(REPEATS):  # (alternating: drift of the box lands on every row alike)
        for name in engines:
            times[name].append(round(timed(step(name), EVALS), 3))
        for name, fn in once.items():
            times[name].append(round(timed(fn, EVALS), 4))
    for name in engines:
        assert bool(torch.isfinite(state[name][1].float()).all())
    for name, t in times.items():
        res["rows"][name] = {"ms": t, "median_ms": round(float(np.median(t)), 4), "min_ms": min(t), "max_ms": max(t)}
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


def table(paths):
    print("| run | commit | row | median ms | min - max ms |")
    print("|---|---|---|---|---|")
    for i, p in enumerate(paths, 1):
        r = json.load(open(p))
        for name, row in r["rows"].items():
            print(f"| {i} | {r['commit']} | {name} | {row['median_ms']:.3f} | {row['min_ms']:.3f} - {row['max_ms']:.3f} |")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown", help="stamp of the tree that runs (the caller knows it; a copy without .git does not)")
    ap.add_argument("--table", nargs="+", metavar="JSON", default=None)
    a = ap.parse_args()
    table(a.table) if a.table else measure(a)
