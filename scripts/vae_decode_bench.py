"""VAE decode alone (lab): N decodes of a 128 x 128 latent -> 1024 x 1024 at the production channel plan, wall time per decode;
TUNE="key=value,..." sets dk_tune_set knobs (e.g. conv_halo=0 | 1 | 2), DTYPE=bfloat16 | float16 the decoder's element type
(config.float16_vae_config).  Under `rocprofv3 --kernel-trace --stats` it is the per-kernel breakdown of the decoder
(profiles/r03_vae_kernel_stats*.md).

LEGS=1: the three-leg comparison of profiles/f16_vae.md in ONE process -- (a) bf16 as shipped, (b) bf16 with conv_v4=0 (conv_halo.hip for
every fused conv: the kernel text the fp16 decoder runs), (c) fp16 -- legs alternated, a warm-up decode per leg and round, REPEATS (default 3)
rounds of N (default 10) decodes each, every timing bracketed by synchronisations."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffusionkit_amd import _lib
from diffusionkit_amd.config import VAEDecoderConfig, float16_vae_config
from diffusionkit_amd.engine import VAEDecoderEngine
from diffusionkit_amd.weights import pack_vae, synth_vae_weights

dev = torch.device("cuda", 0)
lib = _lib.load()


def tune(k, v):
    _lib.check(lib.dk_tune_set(k.encode(), int(v)), "tune")


for kv in filter(None, os.environ.get("TUNE", "").split(",")):
    tune(*kv.split("="))
B = int(os.environ.get("BATCH", "1"))
n = int(os.environ.get("N", "10"))
named = synth_vae_weights(VAEDecoderConfig(), seed=4321)
z = torch.randn(B, 128, 128, 16, generator=torch.Generator().manual_seed(3)).to(dev)


def engine(dtype):
    cfg = float16_vae_config(VAEDecoderConfig(), dtype)
    return VAEDecoderEngine(cfg, pack_vae(cfg, named, dev))


def timed(eng, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        eng.decode(z)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / count * 1e3


if os.environ.get("LEGS", "0") != "1":
    dtype = os.environ.get("DTYPE", "bfloat16")
    eng = engine(dtype)
    for _ in range(2):
        eng.decode(z)
    print(f"TUNE={os.environ.get('TUNE', '')} dtype {dtype} batch {B}: {timed(eng, n):.3f} ms per decode", flush=True)
else:
    legs = [("a: bf16 as shipped", engine("bfloat16"), 1), ("b: bf16, conv_v4=0", engine("bfloat16"), 0), ("c: fp16", engine("float16"), 1)]
    times = {name: [] for name, _, _ in legs}
    for r in range(int(os.environ.get("REPEATS", "3"))):
        for name, eng, v4 in legs:
            tune("conv_v4", v4)
            timed(eng, 1)  # warm-up of this leg
            times[name].append(timed(eng, n))
    tune("conv_v4", 1)
    for name, _, _ in legs:
        t = times[name]
        print(f"leg {name}, batch {B}: " + " / ".join(f"{x:.3f}" for x in t) + f" ms per decode (median {sorted(t)[len(t) // 2]:.3f}, spread {max(t) - min(t):.3f})",
              flush=True)
