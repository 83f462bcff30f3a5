"""Shapes of the text encoders' Linears, shared by tests/test_text_plan_cpu.py (what dk_gemm_plan launches for them) and
tests/test_gpu_text_ops.py (parity of one shape per planned route).  Plain data and arithmetic: no GPU, no library."""
from diffusionkit_amd.text import CLIP_G, CLIP_L, T5_XXL

KERNEL_128, KERNEL_V4 = 128, 4  # dk_gemm_plan_t.kernel: the 128-tile kernel, gemm256v4


def clip_linears(cfg):
    """name -> (N, K) of the GEMMs CLIPTextEngine launches on its B * 77 token rows"""
    d = cfg.model_dims
    return {"qkv": (3 * d, d), "out_proj": (d, d), "linear1": (4 * d, d), "linear2": (d, 4 * d)}


def t5_linears(cfg):
    """name -> (N, K) of the GEMMs T5EncoderEngine launches on its B * N token rows (wi: wi_0 and wi_1 have one shape)"""
    inner = cfg.num_heads * cfg.d_kv
    return {"qkv": (3 * inner, cfg.d_model), "out_proj": (cfg.d_model, inner), "wi": (cfg.d_ff, cfg.d_model), "wo": (cfg.d_model, cfg.d_ff)}


# Row counts the product reaches: a CLIP prompt is 77 tokens, alone (FLUX) or with its negative prompt (SD3: B = 2), and the pooled projection sees one
# row per prompt; T5 encodes 77 (SD3), 256 (FLUX.1-schnell) or 512 (FLUX.1-dev) tokens, for one or two prompts.  CLIP never sees 256 rows or more (at
# 1024 rows its widths would plan gemm256v3, which no text launch uses), and only the pooled projection sees fewer than 77.
CLIP_ROWS = (77, 154)
POOLED_ROWS = (1, 2)
T5_ROWS = (77, 154, 256, 512, 1024)


ALL_ROWS = (1, 2, 77, 154, 256, 512, 1024)


def text_linears(reachable=True):
    """[(what, M, N, K)]: every text Linear of CLIP-L, CLIP-G and T5-XXL at the row counts its engine reaches (above), or at every row count of
    ALL_ROWS whether the product gets there or not"""
    out = []
    for name, cfg in (("clip_l", CLIP_L), ("clip_g", CLIP_G)):
        for lin, (N, K) in clip_linears(cfg).items():
            out += [(f"{name}.{lin}", M, N, K) for M in (CLIP_ROWS if reachable else ALL_ROWS)]
        out += [(f"{name}.text_projection", M, cfg.projection_dim, cfg.model_dims) for M in (POOLED_ROWS if reachable else ALL_ROWS)]
    for lin, (N, K) in t5_linears(T5_XXL).items():
        out += [(f"t5_xxl.{lin}", M, N, K) for M in (T5_ROWS if reachable else ALL_ROWS)]
    return out


# One shape per planned route and edge, called as the engines call ops.linear: (M, N, K, tail, bias, kernel, tile_rows).  tail "bias" = DK_EPI_BIAS,
# "res" = DK_EPI_RES (CLIP's linear2), "gelu" = DK_EPI_BIAS_GELU (CLIP-G's linear1 with a bias, T5's wi_0 without one); bias False = bias=None.
# kernel / tile_rows: what dk_gemm_plan names for the shape without a workspace -- tests/test_text_plan_cpu.py holds the plan to it, and holds the set
# of kernels over text_linears() to the set named here.
GEMM_CASES = [
    (1, 768, 768, "bias", False, KERNEL_128, 128),       # CLIP-L pooled projection, one prompt
    (2, 1280, 1280, "bias", False, KERNEL_128, 128),     # CLIP-G pooled projection, prompt + negative prompt
    (77, 768, 3072, "res", True, KERNEL_128, 128),       # CLIP-L linear2: 48 K tiles
    (154, 5120, 1280, "gelu", True, KERNEL_128, 128),    # CLIP-G linear1, two row tiles
    (77, 4096, 10240, "bias", False, KERNEL_128, 128),   # T5 wo at 77 tokens: 160 K tiles
    (256, 10240, 4096, "gelu", False, KERNEL_128, 128),  # T5 wi_0 at 256 tokens: erf-GELU tail without a bias
    (1024, 4096, 10240, "bias", False, KERNEL_V4, 224),  # T5 wo for two 512-token prompts: 224-row tiles, 80 workgroups
]
