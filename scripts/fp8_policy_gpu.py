"""fp8 precision policy, measured on the GPU at full depth: dB per step against ms per step for
``MMDiTConfig.fp8_bf16_double_blocks = n`` -- the first n double-stream blocks keep bf16 Linears, everything else runs e4m3 weights /
MX-fp8 activations.  Case = tests/golden/fullsize_flux_dev_full.npz (BASELINE configs[3] at full depth: 19 + 38 blocks, S_t = 512,
teacher-forced Euler steps 1 / 2 / 49 / 50 of the 50-step schedule against the fp32 oracle with the ORIGINAL weights).

    python scripts/fp8_policy_gpu.py [n ...]        (default n = 0 1 2 3 4 6 8 12 19; "bf16" = the bf16 model as the ceiling)
    python scripts/fp8_policy_gpu.py --local-ckpt flux1-dev.safetensors [n ...]

``--local-ckpt`` (round-6 review: the shipped policy was fitted on synthetic weights): the same sweep on a real FLUX checkpoint (.safetensors in BFL or
reference key layout, diffusionkit_amd/model_io.py).  No fp32-oracle fixture exists for a real checkpoint, so the yardstick is the bf16 engine on the
same weights and the same teacher-forced inputs: the table then reads "dB lost to fp8" instead of "dB from the fp32 oracle".
"""
import argparse
import gc
import os
import sys
import time
from dataclasses import replace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_fullsize_fixtures as fx  # noqa: E402
from diffusionkit_amd.pipeline import FluxPipeline  # noqa: E402
from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights  # noqa: E402
from tests import test_gpu_fullsize as tf  # noqa: E402
from tests._util import BF, psnr, rel_l2  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("n", nargs="*", help='bf16 double blocks to measure, or "bf16" (default: 0 1 2 3 4 6 8 12 19 bf16)')
    ap.add_argument("--local-ckpt", default=None, help="FLUX MMDiT checkpoint (.safetensors): measure the policy on real weights against the bf16 engine")
    args = ap.parse_args()
    ns = args.n or ["0", "1", "2", "3", "4", "6", "8", "12", "19", "bf16"]
    c = fx.FLUX_DEV_FULL
    t0 = time.time()
    ref_dirs = None
    if args.local_ckpt:
        from diffusionkit_amd.model_io import load_mmdit_checkpoint
        w = dict(load_mmdit_checkpoint(args.local_ckpt, c["cfg"]))
        print(f"checkpoint {args.local_ckpt} read in {time.time() - t0:.0f} s; yardstick: the bf16 engine on the same weights", flush=True)
        ns = ["bf16"] + [n for n in ns if n != "bf16"]  # (the yardstick first)
    else:
        f = np.load(os.path.join(ROOT, "tests", "golden", "fullsize_flux_dev_full.npz"))
        w = synth_mmdit_weights(c["cfg"], seed=c["seed_w"])
        print(f"weights drawn in {time.time() - t0:.0f} s", flush=True)
    text, pooled, _ = fx.forced_inputs(c)
    for n in ns:
        if n == "bf16":
            cfg = c["cfg"]
        else:
            cfg = replace(c["cfg"], weight_dtype="fp8_e4m3", fp8_bf16_double_blocks=int(n))
        pipe = FluxPipeline(w16=True, a16=True, shift=c["shift"], device=dev, text_len=c["S_t"], packed_weights={"mmdit": pack_mmdit(cfg, dict(w), dev)},
                            mmdit_config=cfg)
        got = tf.forced_steps(pipe, c, dev)
        ps, es = [], []
        if args.local_ckpt and ref_dirs is None:
            ref_dirs = {i: got[i].float().clone() for i in got}
        for i in sorted(got):
            ref = ref_dirs[i] if args.local_ckpt else torch.from_numpy(f[f"d{i}_fp32_f16"].astype(np.float32))
            ps.append(psnr(ref, got[i].float()))
            es.append(rel_l2(ref, got[i].float()))
        # time per step: 6 forwards of the prepared engine through the pipeline's own step loop
        lat, it = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=8, cfg_weight=0.0, latent_size=c["latent"], seed=0)
        torch.cuda.synchronize()
        t1 = time.time()
        lat, it = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=8, cfg_weight=0.0, latent_size=c["latent"], seed=0)
        torch.cuda.synchronize()
        ms = (time.time() - t1) / 8 * 1e3
        print(f"bf16 double blocks {n:>4}: Euler direction PSNR steps 1 / 2 / 49 / 50 = " + " / ".join(f"{p:.2f}" for p in ps) +
              f" dB (worst {min(ps):.2f}), rel-L2 worst {max(es):.3e}, {ms:.2f} ms per step (8-step loop incl. host)", flush=True)
        del pipe, got, lat
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
