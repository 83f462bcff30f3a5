"""Shapes and texts of the address-range guards, shared by tests/test_address_range_cpu.py (planners) and tests/test_gpu_address_extents.py (device)."""
import torch

BF, F16 = torch.bfloat16, torch.float16

# (id, dtype, knobs, kernel the plan must name on the near side, tile rows or None)
GEMM_KERNELS = [("v3_mf8", BF, dict(gemm=9, gemm_mf=8), 3, 256), ("v3_mf7", BF, dict(gemm=9, gemm_mf=7), 3, 224), ("v4", BF, dict(gemm=10), 4, None),
                ("v3_f16", F16, dict(gemm=9), 3, None)]
FORCED_TEXT = "gemm256v3 forced but the shape does not allow it"
# (id, dtype, knobs, D, S, kernel)
ATTN_KERNELS = [("lean", BF, dict(attn=4), 128, 768, 4), ("alt", BF, dict(attn=9), 128, 768, 9), ("wave", BF, dict(attn=10), 128, 768, 10),
                ("wave_key_split", BF, dict(attn=10, attn_split=2), 128, 1536, 10), ("lean_f16_d64", F16, dict(), 64, 768, 4)]
ATTN_TEXT = "one batch row of QKV must span < 4 GiB"
F8_TEXT = "gemm256f8: shape / strides / scale layout not eligible"
HALO_TEXT = "conv_halo: shape / alignment not supported"


def a_rows(M, seg_len, seg_stride):
    """gemm256v3.hip: dk_gemm256v3_eligible's count of the A rows a problem spans"""
    return (M - 1) // seg_len * seg_stride + (M - 1) % seg_len + 1


def edge_rows(lda_bytes):
    """the largest row count whose span stays below 2^32 bytes"""
    return (2 ** 32 - 1) // lda_bytes


def attn_edge_ld(S):
    """the largest row pitch (a multiple of 8 elements) with S * ld * 2 < 2^32"""
    return (2 ** 32 - 1) // (2 * S) // 8 * 8
