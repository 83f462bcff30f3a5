#!/usr/bin/env python
"""Lab script: what the first-block cache costs and saves per step (the figures of profiles/block_cache.md).  bench.py is the yardstick and stays
as it is; this script measures the option only.

    python scripts/block_cache_bench.py [--workloads flux-dev-1024 sd3-medium-1024] [--steps 50] [--repeats 2] [--out DIR]

Without --worker it starts one child process per workload, each under its own time limit, one after the other, and stops at the first that
does not end cleanly.  A child builds the workload's pipeline from seeded synthetic weights (the shapes of bench.py's legs: FLUX.1-dev 1024 x 1024
with 512 text tokens in bf16; SD3-medium 1024 x 1024, CFG 5), warms every policy once, and then alternates, in ONE process,
    off       the loop without the option,
    on-0      block_cache = 0.0: head + compute tail in every step (what the option costs when nothing is skipped),
    half      FixedSchedule skipping every odd step (the first and the last step always compute),
`--repeats` times, timing ``denoise_latents`` with the host clock around a device synchronisation.  It also measures, in the same process: a
device-to-device copy (the HBM rate the counted bytes are divided by), ``run_blocks(first_block=0, n_blocks=1)``, the reuse tail (residual add +
final layer) and the residual add alone.  Synthetic weights say nothing about image quality: no threshold is evaluated here."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORKLOADS = ("flux-dev-1024", "sd3-medium-1024")
IMAGE_ROW_PASSES = {"computed": 11, "skipped": 9}  # counted from the launches of a step: X0 save 2, probe 4, then X1 save 2 + capture 3, or reuse 3


def events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def worker(workload, steps, repeats, only=None, micro=True):
    import torch
    from diffusionkit_amd import ops
    from diffusionkit_amd.config import FLUX_SCHNELL, SD3_2b, tiny_vae
    from diffusionkit_amd.pipeline import DiffusionPipeline, FluxPipeline
    from diffusionkit_amd.sampler import FixedSchedule
    from diffusionkit_amd.weights import pack_mmdit, pack_vae, synth_mmdit_weights, synth_vae_weights
    dev = torch.device("cuda", 0)
    if workload == "flux-dev-1024":  # (bench.py: FLUX.1-dev runs on the schnell preset unless --guidance-embed)
        cfg, cls, mv, cfg_weight, shift, S_t, rows = FLUX_SCHNELL, FluxPipeline, "argmaxinc/mlx-FLUX.1-dev", 0.0, 1.0, 512, 1
    else:
        cfg, cls, mv, cfg_weight, shift, S_t, rows = SD3_2b, DiffusionPipeline, "argmaxinc/mlx-stable-diffusion-3-medium", 5.0, 3.0, 589, 2
    latent = (128, 128)
    vcfg = tiny_vae()  # (nothing is decoded)
    weights = {"mmdit": pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234, device=dev), dev, consume=True),
               "vae_decoder": pack_vae(vcfg, synth_vae_weights(vcfg, seed=1235, device=dev), dev)}
    pipe = cls(w16=True, a16=True, shift=shift, model_version=mv, mmdit_config=cfg, vae_config=vcfg, device=dev, text_len=S_t,
               packed_weights=weights)
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(rows, S_t, cfg.token_level_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    pooled = torch.randn(rows, cfg.pooled_text_embed_dim, generator=g).to(dev, torch.bfloat16)
    policies = {"off": lambda: None, "on0": lambda: 0.0, "half": lambda: FixedSchedule(range(1, steps, 2))}
    if only:  # (a kernel trace of one policy: rocprofv3 --kernel-trace --stats -- python scripts/block_cache_bench.py --worker W --policies on0 --no-micro)
        policies = {k: v for k, v in policies.items() if k in only}

    def image(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.denoise_latents(cond, pooled, num_steps=steps, cfg_weight=cfg_weight, latent_size=latent, seed=0, block_cache=policies[name]())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, pipe.last_block_cache

    for name in policies:  # every shape warmed: each policy once
        image(name)
    ms = {name: [] for name in policies}
    record = None
    for _ in range(repeats):
        for name in policies:
            t, rec = image(name)
            ms[name].append(t)
            record = rec if name == "half" else record
    if not micro or len(policies) < 3:
        print("RESULT " + json.dumps({"workload": workload, "steps": steps, "image_ms": ms}))
        return
    n_skipped, n_computed = len(record["skipped"]), len(record["computed"])
    mean = {k: sum(v) / len(v) for k, v in ms.items()}

    # the HBM rate of this box, in this process: a device-to-device copy of 1 GiB (read + write)
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_ms = events_ms(lambda: dst.copy_(src), 10)
    hbm_gbs = 2 * src.numel() / copy_ms / 1e6
    del src, dst

    # condition 2's yardstick, on the engine the last run left prepared (cache on): block 0 alone, the reuse tail, the residual add alone
    mm = pipe.mmdit
    B, p, h = rows, cfg.patch_size, cfg.hidden_size
    S_i = (latent[0] // p) * (latent[1] // p)
    x = torch.randn(B, S_t + S_i, h, generator=g).to(dev, mm.dtype)
    tok = torch.randn(*mm.tokens_shape(), generator=g).to(dev, mm.dtype)
    block0_ms = events_ms(lambda: mm.run_blocks(x, 1, 0, 1), 10)
    out = torch.empty_like(tok)

    def head_reuse():
        mm.forward_head(tok, None, 1)
        mm.forward_tail(1, True, tokens_out=out)

    def head_only():
        mm.forward_head(tok, None, 1)

    skipped_engine_ms = events_ms(head_reuse, 10)   # a skipped step without the probe read-back and the Euler launch
    head_ms = events_ms(head_only, 10)
    r = torch.zeros(B, S_i, h, dtype=mm.dtype, device=dev)
    residual_ms = events_ms(lambda: ops.block_residual(x, S_t, r, True), 20)
    probe_ms = events_ms(lambda: ops.block_probe(x, S_t, r, None), 20)
    row_bytes = B * S_i * h * 2
    per_step = {k: v / steps for k, v in mean.items()}
    skipped_ms = (mean["half"] - n_computed * per_step["on0"]) / n_skipped
    spread_ms = abs(ms["off"][0] - ms["off"][-1]) if len(ms["off"]) > 1 else float("nan")
    res = {
        "workload": workload, "steps": steps, "repeats": repeats, "image_ms": ms, "image_ms_mean": mean,
        "ms_per_computed_step": {"off": per_step["off"], "on0": per_step["on0"]}, "ms_per_skipped_step": skipped_ms,
        "images_per_s": {k: 1e3 / v for k, v in mean.items()}, "off_spread_ms_per_image": spread_ms,
        "half": {"computed": n_computed, "skipped": n_skipped},
        "hbm_copy_gb_per_s": hbm_gbs, "image_row_bytes": row_bytes,
        "counted_mb": {"issue_budget_13_passes": 13 * row_bytes / 1e6, "computed_step_11_passes": IMAGE_ROW_PASSES["computed"] * row_bytes / 1e6,
                       "skipped_step_9_passes": IMAGE_ROW_PASSES["skipped"] * row_bytes / 1e6},
        "on0_cost_ms_per_step": per_step["on0"] - per_step["off"],
        "condition1_allowance_ms_per_step": spread_ms / steps + 13 * row_bytes / (hbm_gbs * 1e6),
        "block0_run_blocks_ms": block0_ms, "head_ms": head_ms, "head_plus_reuse_tail_ms": skipped_engine_ms,
        "reuse_tail_ms": skipped_engine_ms - head_ms, "residual_add_ms": residual_ms, "probe_ms": probe_ms,
        "final_layer_ms_estimate": skipped_engine_ms - head_ms - residual_ms,
    }
    res["condition1_holds"] = res["on0_cost_ms_per_step"] <= res["condition1_allowance_ms_per_step"]
    res["condition2_yardstick_ms"] = block0_ms + res["final_layer_ms_estimate"]
    res["condition2_holds"] = skipped_ms <= 2 * res["condition2_yardstick_ms"]
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=WORKLOADS)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--limit", type=int, default=420, help="time limit of one workload's process in seconds")
    ap.add_argument("--out", default=None, help="directory for block_cache_<workload>.json")
    ap.add_argument("--worker", default=None, choices=WORKLOADS, help="run this workload in this process (what a profiler is pointed at)")
    ap.add_argument("--policies", nargs="+", default=None, choices=("off", "on0", "half"), help="with --worker: only these policies, image times only")
    ap.add_argument("--no-micro", action="store_true", help="with --worker: image times only")
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.steps, args.repeats, args.policies, not args.no_micro)
        return 0
    for wl in args.workloads:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker", wl, "--steps", str(args.steps),
               "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:  # (nothing more is started on the GPU behind a process that did not end cleanly)
            print(p.stdout[-4000:])
            print(f"[block_cache_bench] {wl}: exit status {p.returncode}; stopping")
            return p.returncode or 1
        res = json.loads(lines[-1][7:])
        print(json.dumps(res, indent=1))
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, f"block_cache_{wl}.json"), "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
