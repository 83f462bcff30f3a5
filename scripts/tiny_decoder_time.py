"""Times of the tiny latent decoder on an MI355X, one process, the compared forms alternating (device events, warmed up).  A timed window is
CALLS back-to-back calls through the Python wrappers (allocation of the outputs, ctypes, launches) and the figures are milliseconds per CALL --
call time, not kernel time:

  * dk_tae_decode as the engine ships it (Blocks as chains), dk_tae_decode with dk_tune_set("tae_block", 1) (Blocks as fused launches) and
    dk_vae_decode, on synthetic weights, latents 64 x 64 and 128 x 128, batch 1 and 4;
  * the fused Block (ops.tae_block, one launch) against its chain of three single convs (ops.tae_conv) at 128 x 128 and 1024 x 1024 grids, with
    the MFMA floor's share of the call time: 3 convs x 2 x 9 x 64 x 64 FLOP per pixel, times the fused form's recompute factor 1.28, at 2.5 PFLOP/s.

Prints one JSON line per measurement; needs a GPU (no fallback).  Usage: python scripts/tiny_decoder_time.py [--reps N]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionkit_amd import ops  # noqa: E402
from diffusionkit_amd.config import VAEDecoderConfig  # noqa: E402
from diffusionkit_amd.engine import TinyDecoderEngine, VAEDecoderEngine  # noqa: E402
from diffusionkit_amd.weights import pack_tae, pack_vae, synth_tae_weights, synth_vae_weights  # noqa: E402

PEAK = 2.5e15  # bf16 MFMA, dense
CALLS = 10     # calls per timed window


def alternate(forms, reps, warmup=3):
    """forms: name -> callable; median milliseconds per call and form over ``reps`` rounds in which the forms take turns, CALLS calls a window"""
    for _ in range(warmup):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / CALLS)
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiny_decoder_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    tae = TinyDecoderEngine(pack_tae(synth_tae_weights(), dev))
    vcfg = VAEDecoderConfig()
    vae = VAEDecoderEngine(vcfg, pack_vae(vcfg, synth_vae_weights(vcfg), dev))
    for side in (64, 128):
        for batch in (1, 4):
            lat = torch.randn(batch, side, side, 16, generator=g).to(dev)

            def tae_fused():
                ops.tune("tae_block", 1)
                try:
                    return tae.decode(lat)
                finally:
                    ops.tune("tae_block", -1)
            med, span = alternate({"tae": lambda: tae.decode(lat), "tae_fused": tae_fused, "vae": lambda: vae.decode(lat)}, args.reps)
            print(json.dumps({"what": "decode", "latent": side, "batch": batch, **{k + "_ms": round(v, 3) for k, v in med.items()},
                              **{k + "_min_max": [round(v, 3) for v in span[k]] for k in span}}), flush=True)
        vae._ws = None
    ws = [(torch.randn(64, 576, generator=g) * (2.0 / 576) ** 0.5).to(torch.bfloat16).to(dev) for _ in range(3)]
    bs = [(torch.randn(64, generator=g) * 0.1).to(torch.bfloat16).to(dev) for _ in range(3)]
    for side in (128, 1024):
        x = torch.randn(1, side, side, 64, generator=g).to(torch.bfloat16).to(dev)

        def chain():
            h = ops.tae_conv(x, ws[0], bs[0])
            h = ops.tae_conv(h, ws[1], bs[1])
            return ops.tae_conv(h, ws[2], bs[2], skip=x)
        same = torch.equal(chain(), ops.tae_block(x, ws, bs))
        med, span = alternate({"fused": lambda: ops.tae_block(x, ws, bs), "chain": chain}, args.reps)
        flops = 3 * 2 * 9 * 64 * 64 * side * side
        print(json.dumps({"what": "block", "grid": side, "fused_ms": round(med["fused"], 4), "chain_ms": round(med["chain"], 4),
                          "fused_min_max": [round(v, 4) for v in span["fused"]], "chain_min_max": [round(v, 4) for v in span["chain"]],
                          "same_bits": same, "mfma_floor_share_of_fused_call": round(flops * 1.28 / PEAK * 1e3 / med["fused"], 3),
                          "mfma_floor_share_of_chain_call": round(flops / PEAK * 1e3 / med["chain"], 3)}), flush=True)


if __name__ == "__main__":
    main()
