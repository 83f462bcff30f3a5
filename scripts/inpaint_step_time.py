"""FLUX.1-schnell 1024^2, 4 steps: step time from iter_time with and without an inpainting mask (one process, alternating, each after a warm-up run),
and the step kernel alone (HIP events over back-to-back launches).  ``python scripts/inpaint_step_time.py [out.json]``; profiles/inpaint.md."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionkit_amd import ops  # noqa: E402
from diffusionkit_amd.config import FLUX_SCHNELL, VAEDecoderConfig, VAEEncoderConfig  # noqa: E402
from diffusionkit_amd.pipeline import FluxPipeline  # noqa: E402
from diffusionkit_amd.weights import pack_mmdit, pack_vae, synth_mmdit_weights, synth_vae_weights  # noqa: E402

dev = torch.device("cuda", 0)
cfg, vcfg = FLUX_SCHNELL, VAEDecoderConfig()
t0 = time.time()
weights = {"mmdit": pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234, device=dev), dev, consume=True),
           "vae_decoder": pack_vae(vcfg, synth_vae_weights(vcfg, seed=1235, device=dev), dev)}
pipe = FluxPipeline(w16=True, a16=True, shift=1.0, mmdit_config=cfg, vae_config=vcfg, vae_encoder_config=VAEEncoderConfig(), device=dev, text_len=256,
                    packed_weights=weights)
print(f"pipeline built in {time.time() - t0:.1f} s", flush=True)
g = torch.Generator().manual_seed(1)
cond = torch.randn(1, 256, cfg.token_level_text_embed_dim, generator=g).to(dev, torch.bfloat16)
pooled = torch.randn(1, cfg.pooled_text_embed_dim, generator=g).to(dev, torch.bfloat16)
H = W = 1024
rng = np.random.RandomState(0)
yy, xx = np.mgrid[0:H, 0:W]
rgb = np.clip(np.stack([(yy * 255 // H), (xx * 255 // W), ((yy + xx) * 255 // (H + W))], -1) + rng.randint(-20, 20, size=(H, W, 3)), 0, 255).astype(np.uint8)
mask = np.zeros((H, W), dtype=np.uint8)
mask[:, W // 2:] = 255


def run(m):
    kw = {} if m is None else {"mask_path": m}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    lat, it = pipe.denoise_latents(cond, pooled, num_steps=4, cfg_weight=0.0, latent_size=(128, 128), seed=5, image_path=rgb, denoise=1.0, **kw)
    e1.record()
    torch.cuda.synchronize()
    return lat, it, e0.elapsed_time(e1)


res = {"iter_time_s": {"plain": [], "masked": []}, "denoise_latents_ms": {"plain": [], "masked": []}}
run(None), run(mask)  # warm-up of both paths (encoder included)
for r in range(6):
    for name, m in (("plain", None), ("masked", mask)):
        lat, it, ms = run(m)
        res["iter_time_s"][name].append(it)
        res["denoise_latents_ms"][name].append(round(ms, 3))
for name in ("plain", "masked"):
    a = np.asarray(res["iter_time_s"][name])
    res[f"step_ms_mean_{name}"] = round(float(a.mean()) * 1e3, 3)
    res[f"step_ms_mean_{name}_per_run"] = [round(float(v) * 1e3, 2) for v in a.mean(axis=1)]
# kept half of the masked run == the encoded image
x_orig = pipe.latent_format.process_in(pipe.encode_image_to_latents(rgb, seed=5))
kept = pipe.latent_format.process_out(x_orig)
res["kept_half_bit_equal_1024"] = bool(torch.equal(lat[:, :, :64].view(torch.int32), kept[:, :, :64].view(torch.int32)))

# the step kernel alone at this shape
n_img, Hl, Wl, C, p = 1, 128, 128, 16, 2
x = torch.randn(n_img, Hl, Wl, C, device=dev)
out = torch.randn(n_img, 4096, 64, device=dev).to(torch.bfloat16)
tok = torch.empty_like(out)
xo, no, mm = torch.randn_like(x), torch.randn_like(x), torch.rand(1, Hl, Wl, device=dev)


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


plain = lambda: ops.euler_cfg_step(x, out, tok, n_img, False, p, 1, 0.75, 0.5, 0.0)  # noqa: E731
masked = lambda: ops.euler_cfg_step_masked(x, out, tok, n_img, False, p, 1, 0.75, 0.5, 0.0, xo, no, mm)  # noqa: E731
res["step_kernel_us_back_to_back"] = {"plain": [kernel_us(plain) for _ in range(3)], "masked": [kernel_us(masked) for _ in range(3)]}
u8 = torch.randint(0, 256, (1, H, W, 3), device=dev, dtype=torch.uint8)
orig_d, mask_d = torch.from_numpy(rgb).to(dev), torch.from_numpy(mask[None]).to(dev)
res["composite_us_1024"] = kernel_us(lambda: ops.image_composite(u8, orig_d, mask_d), 100)
res["mask_to_latent_us_1024"] = kernel_us(lambda: ops.mask_to_latent(mask_d, 8), 100)
print(json.dumps(res, indent=1))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
