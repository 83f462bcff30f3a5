"""Operands for the MX-fp6 activation (W4A6) tests: the product quantiser (diffusionkit_amd/weights.py: quantize_activation_mxfp6) is the format's
definition and tests/test_fp6_host.py checks it; here it only builds what the GPU tests compare against."""
import torch

from diffusionkit_amd.weights import dequantize_activation_mxfp6, pack_activation_mxfp6, quantize_activation_mxfp6
from tests import _fp8 as f8
from tests._util import bf16r, randn


def hazard_rows(M, K, seed=3):
    """bf16 rows for the quantiser: N(0, 1) with, per row, one 64x outlier beside small values (the in-block range hazard of a 2-bit exponent), an
    all-zero block and a negative-only block"""
    x = randn(M, K, seed=seed, scale=1.0)
    r = torch.arange(M)
    x[r, (r * 7) % 32] *= 64.0
    x[:, 32:64] = 0.0
    x[:, 64:96] = -x[:, 64:96].abs() - 0.01
    return bf16r(x)


def activation_operands(a, rows=None):
    """fp32 activations [M, K] -> (fragment-ordered bytes, scale side array, dequantised fp32 values)"""
    code, e8 = quantize_activation_mxfp6(a)
    a6 = pack_activation_mxfp6(code)
    return a6, f8.scales_to_array(e8, a6.shape[0] if rows is None else rows), dequantize_activation_mxfp6(code, e8)


def plan_desc(M, N, K, workspace=True):
    """a dk_gemm_fp8_desc of the W4A6 GEMM for ops.gemm_fp4a6_plan: made-up aligned pointers, the operator's pitches"""
    from diffusionkit_amd import _lib
    d = dict(A=0x10000, A_scales=0x20000, W=0x30000, w_scale=0x40000, C=0x50000, M=M, N=N, K=K, lda=K // 128 * 96, ldw=K // 2, ldc=N,
             a_row0=0, a_rows=(M + 15) // 16 * 16, epilogue=_lib.DK_EPI_BIAS)
    if workspace:
        d.update(workspace=0x100000, workspace_bytes=int(_lib.load().dk_gemm_workspace_bytes()))
    return d


def smallest_split_shape(M=255):
    """the (M, N, K) with the fewest weight elements N * K, one ragged row tile, that the launch rules cut along K once the workspace is there
    (N up to 1024, K up to 128 K-tiles; ties: the smaller N)"""
    from diffusionkit_amd import ops
    for nk, N, K in sorted((N * K, N, K) for N in (256, 512, 768, 1024) for K in range(128, 128 * 129, 128)):
        if ops.gemm_fp4a6_plan(plan_desc(M, N, K)).k_pieces > 1:
            return M, N, K
    raise AssertionError("no shape of the sweep is cut along K")
