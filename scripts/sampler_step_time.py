"""The coefficient-row step (dk_lms_cfg_step) against dk_euler_cfg_step at the 128 x 128 x 16 latent -- with and without CFG, plain and masked, HIP
events over back-to-back launches in one process -- and FLUX.1-schnell 1024^2 at 4 steps under each sampler from the pipeline's iter_time
(alternating, each after a warm-up run).  ``python scripts/sampler_step_time.py [out.json]``; profiles/samplers.md."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionkit_amd import ops  # noqa: E402
from diffusionkit_amd.config import FLUX_SCHNELL, VAEDecoderConfig  # noqa: E402
from diffusionkit_amd.pipeline import FluxPipeline  # noqa: E402
from diffusionkit_amd.sampler import SAMPLERS  # noqa: E402
from diffusionkit_amd.weights import pack_mmdit, pack_vae, synth_mmdit_weights, synth_vae_weights  # noqa: E402

dev = torch.device("cuda", 0)
res = {}

# ---- the step kernel alone ---------------------------------------------------------------------------------------------------------------------------
n_img, Hl, Wl, C, p = 1, 128, 128, 16, 2
x = torch.randn(n_img, Hl, Wl, C, device=dev)
hist, xo, no, mm = torch.randn_like(x), torch.randn_like(x), torch.randn_like(x), torch.rand(1, Hl, Wl, device=dev)
AB2 = (1.0, -0.375, 0.125, 0.0, 1.0)  # a later ab2 row at equal steps of -0.25: reads H, leaves H = d


def kernel_us(fn, n=400):
    for _ in range(20):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / n, 3)


res["step_kernel_us_back_to_back"] = {}
for cfg_on in (False, True):
    out = torch.randn(n_img * (2 if cfg_on else 1), (Hl // p) * (Wl // p), p * p * C, device=dev).to(torch.bfloat16)
    tok = torch.empty_like(out)
    w = 5.0 if cfg_on else 0.0
    head = (x, out, tok, n_img, cfg_on, p, 1, 0.75, 0.5, w)
    launches = {"euler": lambda: ops.euler_cfg_step(*head), "lms": lambda: ops.lms_cfg_step(*head, hist, AB2, True, True),
                "lms_first_order": lambda: ops.lms_cfg_step(*head, None, (1.0, -0.25, 0.0, 0.0, 0.0), False, False),
                "euler_masked": lambda: ops.euler_cfg_step_masked(*head, xo, no, mm),
                "lms_masked": lambda: ops.lms_cfg_step_masked(*head, hist, AB2, True, True, xo, no, mm)}
    times = {k: [] for k in launches}
    for _ in range(3):  # (alternating)
        for k, fn in launches.items():
            times[k].append(kernel_us(fn))
    res["step_kernel_us_back_to_back"]["cfg" if cfg_on else "no_cfg"] = times

# ---- FLUX.1-schnell 1024^2, 4 steps, per sampler ------------------------------------------------------------------------------------------------------
cfg, vcfg = FLUX_SCHNELL, VAEDecoderConfig()
t0 = time.time()
weights = {"mmdit": pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234, device=dev), dev, consume=True),
           "vae_decoder": pack_vae(vcfg, synth_vae_weights(vcfg, seed=1235, device=dev), dev)}
pipe = FluxPipeline(w16=True, a16=True, shift=1.0, mmdit_config=cfg, vae_config=vcfg, device=dev, text_len=256, packed_weights=weights)
print(f"pipeline built in {time.time() - t0:.1f} s", flush=True)
g = torch.Generator().manual_seed(1)
cond = torch.randn(1, 256, cfg.token_level_text_embed_dim, generator=g).to(dev, torch.bfloat16)
pooled = torch.randn(1, cfg.pooled_text_embed_dim, generator=g).to(dev, torch.bfloat16)


def run(sampler):
    lat, it = pipe.denoise_latents(cond, pooled, num_steps=4, cfg_weight=0.0, latent_size=(128, 128), seed=5, sampler=sampler)
    return it, pipe.last_sampler["model_evals"], bool(torch.isfinite(lat).all())


for s in SAMPLERS:
    run(s)  # warm-up
res["flux_1024_4_steps"] = {s: {"iter_time_s": [], "model_evals": None} for s in SAMPLERS}
for _ in range(5):
    for s in SAMPLERS:
        it, evals, finite = run(s)
        assert finite
        res["flux_1024_4_steps"][s]["iter_time_s"].append(it)
        res["flux_1024_4_steps"][s]["model_evals"] = evals
for s in SAMPLERS:
    a = np.asarray(res["flux_1024_4_steps"][s]["iter_time_s"])
    r = res["flux_1024_4_steps"][s]
    r["step_ms_mean_per_position"] = [round(float(v) * 1e3, 2) for v in a.mean(axis=0)]
    r["image_ms_mean"] = round(float(a.sum(axis=1).mean()) * 1e3, 2)
    r["ms_per_model_eval"] = round(r["image_ms_mean"] / r["model_evals"], 2)
print(json.dumps(res, indent=1))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
