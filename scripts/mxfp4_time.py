"""Per-launch times of the MX-fp4 GEMM (csrc/gemm256f4.hip) against the fp8 GEMM (csrc/gemm256f8.hip) on FLUX's block Linears, on one GPU:
    python scripts/mxfp4_time.py [--tokens 1536 4608] [--reps 30]
Both kernels run in alternation inside one process, timed with device events around `reps` launches after a warm-up.  "warm": the same weight every
launch (it stays in the Infinity Cache where it fits); "cold": a ring of weight copies larger than the cache, a new one every launch -- what a model
step sees, every block has its own weights.  Prints one line per shape; nothing is gated.  (Results: profiles/mxfp4.md.)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diffusionkit_amd import ops
from diffusionkit_amd.weights import pack_mxfp4, quantize_weight_e4m3, quantize_weight_mxfp4

H = 3072
SHAPES = (("qkv", 3 * H, H), ("o_proj", H, H), ("fc1", 4 * H, H), ("fc2", H, 4 * H), ("linear1", 7 * H, H), ("linear2", H, 5 * H))  # (name, N, K)
CACHE_BYTES = 512 << 20  # a ring of weights at least this large: beyond L2 + Infinity Cache


def timed(fn, n_weights, reps):
    for i in range(3):
        fn(i % n_weights)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i % n_weights)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[1024 + 512, 4096 + 512], help="rows M: image + text tokens at 512^2 and 1024^2")
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda")
    wsp = ops.gemm_workspace(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for M in args.tokens:
        rows = (M + 127) // 128 * 128
        for name, N, K in SHAPES:
            lda = int(ops._lib.load().dk_weight_pitch_fp8(K))
            a8 = torch.randint(0, 64, (rows, lda), dtype=torch.uint8, device=dev, generator=g)  # finite e4m3 codes
            sa = torch.full((ops.mx_scale_bytes(rows, lda),), 127, dtype=torch.uint8, device=dev)
            w = torch.randn(N, K, device=dev, generator=g) * 0.02
            q8, ws8 = quantize_weight_e4m3(w)
            w8 = torch.zeros(N, lda, dtype=torch.uint8, device=dev)
            w8[:, :K] = q8
            code, e8, ws4 = quantize_weight_mxfp4(w)
            w4, sw = pack_mxfp4(code, e8, ops.weight_pitch_fp4(K))
            n8, n4 = max(2, CACHE_BYTES // w8.numel() + 1), max(2, CACHE_BYTES // w4.numel() + 1)
            ring8, ring4 = [w8.clone() for _ in range(n8)], [w4.clone() for _ in range(n4)]
            out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)

            def f8(i):
                ops.gemm_fp8(a8, sa, ring8[i], ws8, M=M, k=K, workspace=wsp, out=out)

            def f4(i):
                ops.gemm_fp4(a8, sa, ring4[i], sw, ws4, M=M, k=K, workspace=wsp, out=out)
            t = {}
            for rnd in range(2):  # alternate the kernels; keep the second round
                for key, fn, n in (("fp8 warm", f8, 1), ("fp4 warm", f4, 1), ("fp8 cold", f8, n8), ("fp4 cold", f4, n4)):
                    t[key] = timed(fn, n, args.reps)
            tf = 2.0 * M * N * K * 1e-6
            print(f"M {M:5d} {name:8s} N {N:5d} K {K:5d} | warm fp8 {t['fp8 warm']:7.1f} us  fp4 {t['fp4 warm']:7.1f} us | cold fp8 {t['fp8 cold']:7.1f} us  "
                  f"fp4 {t['fp4 cold']:7.1f} us ({tf / t['fp4 cold']:.0f} TFLOP/s) | weight bytes fp8 {w8.numel() >> 10} KiB  fp4 {(w4.numel() + sw.numel()) >> 10} KiB",
                  flush=True)
            del ring8, ring4


if __name__ == "__main__":
    main()
