#!/usr/bin/env python
"""Lab script: what the guidance modes cost per step and what a guidance interval saves (the figures of profiles/guidance.md).  bench.py is the
yardstick and stays as it is; this script measures the options only.

    python scripts/guidance_bench.py [--steps 50] [--repeats 3] [--settings cfg rescale apg interval40] [--out DIR]

Without --worker it starts one child process under a time limit and reports what it printed.  The child builds the SD3-medium pipeline from seeded
synthetic weights (bench.py's sd3-medium-1024 leg: 1024 x 1024, 589 text tokens, CFG 5, bf16), warms every setting once, and then alternates, in ONE
process,
    cfg         the default loop (``denoise_latents`` without a guidance keyword -- this setting also runs on a tree without the feature),
    rescale     guidance="rescale", 0.7: two moment launches and the guided step behind every evaluation,
    apg         guidance="apg", momentum -0.5, norm threshold 15: the same launches plus the momentum buffer,
    interval40  plain cfg inside an interval that leaves the last 40 % of the evaluations (the lowest sigmas) unguided: one transition,
`--repeats` times, timing ``denoise_latents`` with the host clock around a device synchronisation.  With more than the cfg setting it also times
the transition alone (``pipeline._set_rows``: re-prepare + modulation table + context + patchify, alternating between 2 n and n rows) and one
model evaluation at each batch.  Synthetic weights say nothing about image quality: no setting is evaluated here."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SETTINGS = ("cfg", "rescale", "apg", "interval40")


def worker(steps, repeats, settings):
    import torch
    from diffusionkit_amd.config import SD3_2b, tiny_vae
    from diffusionkit_amd.pipeline import DiffusionPipeline
    from diffusionkit_amd.weights import pack_mmdit, pack_vae, synth_mmdit_weights, synth_vae_weights
    dev = torch.device("cuda", 0)
    cfg, S_t, latent, cfg_weight = SD3_2b, 589, (128, 128), 5.0
    vcfg = tiny_vae()  # (nothing is decoded)
    weights = {"mmdit": pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234, device=dev), dev, consume=True),
               "vae_decoder": pack_vae(vcfg, synth_vae_weights(vcfg, seed=1235, device=dev), dev)}
    pipe = DiffusionPipeline(w16=True, a16=True, shift=3.0, model_version="argmaxinc/mlx-stable-diffusion-3-medium", mmdit_config=cfg, vae_config=vcfg,
                             device=dev, text_len=S_t, packed_weights=weights)
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(2, S_t, cfg.token_level_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    pooled = torch.randn(2, cfg.pooled_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    sigmas = pipe.get_sigmas(pipe.sampler, steps)
    n_guided = steps - (2 * steps) // 5
    keywords = {"cfg": {}, "rescale": dict(guidance="rescale", guidance_rescale=0.7),
                "apg": dict(guidance="apg", apg_momentum=-0.5, apg_norm_threshold=15.0),
                "interval40": dict(guidance_interval=(float(sigmas[n_guided - 1]), 2.0))}

    def image(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.denoise_latents(cond, pooled, num_steps=steps, cfg_weight=cfg_weight, latent_size=latent, seed=0, **keywords[name])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name in settings:  # every shape warmed: each setting once
        image(name)
    ms = {name: [] for name in settings}
    for _ in range(repeats):
        for name in settings:
            ms[name].append(image(name))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    res = {"steps": steps, "repeats": repeats, "image_ms": ms, "image_ms_mean": mean, "ms_per_step": {k: v / steps for k, v in mean.items()},
           "images_per_s": {k: 1e3 / v for k, v in mean.items()}, "spread_ms_per_image": {k: max(v) - min(v) for k, v in ms.items()}}
    if "interval40" in settings:
        res["interval40"] = dict(pipe.last_guidance)
    if len(settings) > 1:
        from diffusionkit_amd import pipeline as pl
        import numpy as np
        model = pl.CFGDenoiser(pipe)
        x0 = torch.randn(1, *latent, 16, generator=g).to(dev)
        lp = pl._loop_setup(model, x0, sigmas, {"conditioning": cond, "pooled_conditioning": pooled, "cfg_weight": cfg_weight})
        trans, evals = {"to_n": [], "to_2n": []}, {}
        for k in range(6):
            for guided in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tok, out = pl._set_rows(model, lp, guided)
                torch.cuda.synchronize()
                trans["to_2n" if guided else "to_n"].append((time.perf_counter() - t0) * 1e3)
                if k == 5:  # one model evaluation at this batch, after a warm one
                    lp.mm.forward_tokens(tok, None, 1, tokens_out=out)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(10):
                        lp.mm.forward_tokens(tok, None, 1, tokens_out=out)
                    torch.cuda.synchronize()
                    evals["2n" if guided else "n"] = (time.perf_counter() - t0) * 1e2
        res["transition_ms"] = {k: {"first": v[0], "median_of_rest": float(np.median(v[1:]))} for k, v in trans.items()}
        res["model_eval_ms"] = evals
        res["unguided_over_guided_eval"] = evals["n"] / evals["2n"]
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--settings", nargs="+", default=list(SETTINGS), choices=SETTINGS)
    ap.add_argument("--limit", type=int, default=420, help="time limit of the measuring process in seconds")
    ap.add_argument("--out", default=None, help="directory for guidance_bench.json")
    ap.add_argument("--worker", action="store_true", help="measure in this process (what a profiler is pointed at)")
    args = ap.parse_args()
    if args.worker:
        worker(args.steps, args.repeats, args.settings)
        return 0
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(args.steps), "--repeats",
           str(args.repeats), "--settings"] + list(args.settings)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        print(p.stdout[-4000:])
        print(f"[guidance_bench] exit status {p.returncode}")
        return p.returncode or 1
    res = json.loads(lines[-1][7:])
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "guidance_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
