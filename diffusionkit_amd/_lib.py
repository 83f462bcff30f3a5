"""ctypes binding of libdk_hip.so (include/dk_hip.h).

The product path has no CPU fallback: if the HIP extension is missing or an entry point
fails, a ``DkHipError`` is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# DK_HIP_LIB: another build of the same library, for same-box A/B measurements (scripts/ab_lib.sh); the in-tree one otherwise
LIB_PATH = os.environ.get("DK_HIP_LIB") or os.path.join(_HERE, "libdk_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dk_hip.h")


class DkHipError(RuntimeError):
    pass


class dk_gemm_desc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("W", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p),
        ("gate", C.c_void_p), ("res", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("lda", C.c_int32), ("ldc", C.c_int32), ("ldr", C.c_int32),
        ("a_seg_len", C.c_int32), ("a_seg_stride", C.c_int32),
        ("c_seg_len", C.c_int32), ("c_seg_stride", C.c_int32),
        ("r_seg_len", C.c_int32), ("r_seg_stride", C.c_int32),
        ("gate_seg_len", C.c_int32), ("gate_stride", C.c_int32),
        ("alpha", C.c_float), ("epilogue", C.c_int32), ("ldw", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class dk_conv_desc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("y", C.c_void_p), ("bias", C.c_void_p),
        ("res", C.c_void_p), ("zeros", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("O", C.c_int32),
        ("ldy", C.c_int32), ("ldr", C.c_int32), ("upsample", C.c_int32), ("epilogue", C.c_int32),
    ]


class dk_conv_gn_desc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("y", C.c_void_p), ("res", C.c_void_p),
        ("gn_scale_shift", C.c_void_p), ("gn_silu", C.c_int32),
        ("x2", C.c_void_p), ("bias2", C.c_void_p), ("stats_partial", C.c_void_p),
        ("image_f32", C.c_void_p), ("image_u8", C.c_void_p), ("raw_bf16", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("O", C.c_int32), ("C2", C.c_int32),
        ("ldw", C.c_int32), ("ldy", C.c_int32), ("ldr", C.c_int32), ("upsample", C.c_int32), ("stats_groups", C.c_int32),
    ]


class dk_mmdit_config(C.Structure):
    _fields_ = [
        ("num_heads", C.c_int32), ("depth_multimodal", C.c_int32), ("depth_unified", C.c_int32),
        ("hidden_size", C.c_int32), ("mlp_ratio", C.c_int32),
        ("vae_latent_dim", C.c_int32), ("patch_size", C.c_int32), ("patchify_via_reshape", C.c_int32),
        ("use_qk_norm", C.c_int32), ("use_rope", C.c_int32), ("rope_axes_dim", C.c_int32 * 4),
        ("n_rope_axes", C.c_int32), ("rope_theta", C.c_int32),
        ("use_pos_embed", C.c_int32), ("max_latent_resolution", C.c_int32),
        ("pooled_text_embed_dim", C.c_int32), ("token_level_text_embed_dim", C.c_int32),
        ("frequency_embed_dim", C.c_int32), ("max_period", C.c_int32),
        ("embed_dtype", C.c_int32), ("layer_norm_eps", C.c_float),
        ("guidance_embed", C.c_int32), ("fp8_linears", C.c_int32), ("fp8_bf16_double_blocks", C.c_int32),
    ]


class dk_gemm_fp8_desc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("A_scales", C.c_void_p), ("W", C.c_void_p), ("w_scale", C.c_void_p), ("C", C.c_void_p),
        ("bias", C.c_void_p), ("gate", C.c_void_p), ("res", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("lda", C.c_int32), ("ldw", C.c_int32), ("ldc", C.c_int32), ("ldr", C.c_int32),
        ("a_seg_len", C.c_int32), ("a_seg_stride", C.c_int32), ("a_row0", C.c_int32), ("a_rows", C.c_int32),
        ("c_seg_len", C.c_int32), ("c_seg_stride", C.c_int32),
        ("r_seg_len", C.c_int32), ("r_seg_stride", C.c_int32),
        ("gate_seg_len", C.c_int32), ("gate_stride", C.c_int32),
        ("epilogue", C.c_int32), ("c_mx8", C.c_int32),
        ("C_scales", C.c_void_p), ("c_rows", C.c_int32), ("c_row0", C.c_int32), ("c_col0", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


_FUSED_TAIL = [
    ("kn_w", C.c_void_p), ("kn_rope", C.c_void_p),
    ("kn_col0", C.c_int32), ("kn_col1", C.c_int32), ("kn_D", C.c_int32), ("kn_pos_off", C.c_int32), ("kn_seg_len", C.c_int32),
    ("kn_eps", C.c_float), ("qn_w", C.c_void_p), ("qn_col0", C.c_int32), ("qn_col1", C.c_int32),
]


class dk_gemm_side(C.Structure):
    _fields_ = [("n_split", C.c_int32), ("C2", C.c_void_p), ("ldc2", C.c_int32), ("epi2", C.c_int32)] + _FUSED_TAIL


class dk_gemm_fp8_side(C.Structure):
    _fields_ = [("n_split", C.c_int32), ("C2", C.c_void_p), ("ldc2", C.c_int32), ("epi2", C.c_int32), ("c2_mx8", C.c_int32)] + _FUSED_TAIL


class dk_attention_desc(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("S", C.c_int32), ("D", C.c_int32), ("ld", C.c_int32), ("ldo", C.c_int32),
        ("scale", C.c_float), ("bias", C.c_void_p), ("bias_head_stride", C.c_int64), ("ldb", C.c_int32),
        ("qn_a", C.c_void_p), ("qn_b", C.c_void_p), ("qn_split", C.c_int32), ("qn_eps", C.c_float), ("q_rope", C.c_void_p),
        ("O8", C.c_void_p), ("O8_scales", C.c_void_p), ("o8_ld", C.c_int32), ("o8_rows", C.c_int64),
        ("score_bound", C.c_float),
    ]


class dk_vae_config(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("block_out_channels", C.c_int32 * 4),
        ("n_blocks", C.c_int32), ("layers_per_block", C.c_int32), ("resnet_groups", C.c_int32),
        ("group_norm_eps", C.c_float),
    ]


DK_EPI_BIAS, DK_EPI_BIAS_GELU, DK_EPI_GATE_RES, DK_EPI_RES, DK_EPI_BIAS_SILU = range(5)

_vp, _i32, _i64, _f32, _sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
_fp = C.POINTER(C.c_float)

# name -> (restype, argtypes); must list every symbol include/dk_hip.h declares
class dk_gemm_plan_t(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kernel", "tile_rows", "tiles", "workgroups", "split_tiles", "k_pieces", "ks", "n_cu", "launches")]


class dk_attention_plan_t(C.Structure):  # (o8_split is read by dk_attention_plan, the other fields are written)
    _fields_ = [(n, C.c_int32) for n in ("kernel", "qfuse", "blocks", "whole", "split", "jobs", "merge", "quantize", "launches", "n_cu", "o8_split", "untracked")]


# the step entries (dk_euler / dk_lms / dk_guided _cfg_step, their masked and _f16 forms), composed: x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl,
# C, p, reshape_order, sigma; then Euler's sigma_next, cfg_weight, or the row's cfg_weight, hist, five coefficients, sigma_next, reads_h, writes_h; then
# the mask operands x_orig, noise, mask, mask_per_image; then mode, phi, eta, r, beta, reads_m, writes_m, m, workspace, its bytes; then (dk_slg_cfg_step)
# slg_scale; then (dk_noisy_cfg_step) guided, slg, cn, seeds, draw; then the stream
_STEP_HEAD = [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32]
_STEP_EULER = _STEP_HEAD + [_f32, _f32]
_STEP_ROW = _STEP_HEAD + [_f32, _vp, _f32, _f32, _f32, _f32, _f32, _f32, _i32, _i32]
_STEP_MASK = [_vp, _vp, _vp, _i32]
_STEP_GUIDE = [_i32, _f32, _f32, _f32, _f32, _i32, _i32, _vp, _vp, _sz]
_STEP_ENTRIES = {"dk_euler_cfg_step": _STEP_EULER, "dk_euler_cfg_step_masked": _STEP_EULER + _STEP_MASK, "dk_lms_cfg_step": _STEP_ROW,
                 "dk_lms_cfg_step_masked": _STEP_ROW + _STEP_MASK, "dk_guided_cfg_step": _STEP_ROW + _STEP_MASK + _STEP_GUIDE,
                 "dk_slg_cfg_step": _STEP_ROW + _STEP_MASK + _STEP_GUIDE + [_f32],
                 "dk_noisy_cfg_step": _STEP_ROW + _STEP_MASK + _STEP_GUIDE + [_f32] + [_i32, _i32, _f32, _vp, _i32]}
SIGNATURES = {
    "dk_abi_version": (_i32, []),
    "dk_last_error": (C.c_char_p, []),
    "dk_gemm_bf16": (_i32, [C.POINTER(dk_gemm_desc), _vp]),
    "dk_gemm_plan": (_i32, [C.POINTER(dk_gemm_desc), C.POINTER(dk_gemm_desc), C.POINTER(dk_gemm_plan_t)]),
    "dk_gemm_fused_bf16": (_i32, [C.POINTER(dk_gemm_desc), C.POINTER(dk_gemm_side), C.POINTER(dk_gemm_desc), C.POINTER(dk_gemm_side), _vp]),
    "dk_gemm_fused_plan": (_i32, [C.POINTER(dk_gemm_desc), C.POINTER(dk_gemm_side), C.POINTER(dk_gemm_desc), C.POINTER(dk_gemm_side),
                                  C.POINTER(dk_gemm_plan_t)]),
    "dk_gemm_fp8_fused": (_i32, [C.POINTER(dk_gemm_fp8_desc), C.POINTER(dk_gemm_fp8_side), C.POINTER(dk_gemm_fp8_desc), C.POINTER(dk_gemm_fp8_side),
                                 _vp]),
    "dk_attention_desc_bf16": (_i32, [C.POINTER(dk_attention_desc), _vp]),
    "dk_attention_plan": (_i32, [C.POINTER(dk_attention_desc), _sz, C.POINTER(dk_attention_plan_t)]),
    # identity attention (perturbed-attention guidance): the descriptor, ident_from, then the stream -- or f16 and the plan
    "dk_attention_identity_bf16": (_i32, [C.POINTER(dk_attention_desc), _i32, _vp]),
    "dk_attention_identity_f16": (_i32, [C.POINTER(dk_attention_desc), _i32, _vp]),
    "dk_attention_identity_plan": (_i32, [C.POINTER(dk_attention_desc), _i32, _i32, C.POINTER(dk_attention_plan_t)]),
    "dk_gemm_workspace_bytes": (C.c_size_t, []),
    "dk_attention_workspace_bytes": (C.c_size_t, []),
    "dk_attention_set_workspace": (C.c_int, [C.c_void_p, C.c_size_t]),
    "dk_conv3x3_bf16": (_i32, [C.POINTER(dk_conv_desc), _vp]),
    "dk_conv3x3_gn_bf16": (_i32, [C.POINTER(dk_conv_gn_desc), _vp]),
    "dk_groupnorm_table_bf16": (_i32, [_vp, _i32, C.c_int64, _i32, _i32, _vp, _vp, C.c_float, _vp, _i32, _vp, _vp]),
    "dk_attention_bf16": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp]),
    "dk_attention_d512_tp": (_i32, [_i32]),
    "dk_attention_d512_bf16": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_float, _vp, _vp]),
    "dk_attention_bias_bf16": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _i64, _i32, _vp]),
    "dk_embedding_bf16": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp]),
    "dk_layernorm_bf16": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _f32, _vp]),
    "dk_t5_rmsnorm_bf16": (_i32, [_vp, _vp, _i32, _i32, _vp, _f32, _vp]),
    "dk_text_elementwise": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "dk_t5_bias_bf16": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "dk_gemm_fp8": (_i32, [C.POINTER(dk_gemm_fp8_desc), _vp]),
    "dk_mx_scale_bytes": (_sz, [_i64, _i32]),
    "dk_quantize_mx8": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _vp, _i64, _i32, _i32, _vp]),
    "dk_ln_modulate_mx8": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _f32, _vp, _i32, _vp, _i64, _i32, _vp]),
    "dk_weight_pitch_fp8": (_i32, [_i32]),
    "dk_mmdit_set_guidance": (_i32, [_vp, _f32]),
    # float16 element type (SD3 family): siblings of the bf16 operators, same descriptors
    "dk_gemm_f16": (_i32, [C.POINTER(dk_gemm_desc), _vp]),
    "dk_gemm_plan_f16": (_i32, [C.POINTER(dk_gemm_desc), C.POINTER(dk_gemm_desc), C.POINTER(dk_gemm_plan_t)]),
    "dk_gemm_fused_f16": (_i32, [C.POINTER(dk_gemm_desc), C.POINTER(dk_gemm_side), C.POINTER(dk_gemm_desc), C.POINTER(dk_gemm_side), _vp]),
    "dk_attention_desc_f16": (_i32, [C.POINTER(dk_attention_desc), _vp]),
    "dk_attention_plan_f16": (_i32, [C.POINTER(dk_attention_desc), _sz, C.POINTER(dk_attention_plan_t)]),
    "dk_ln_modulate_f16": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp]),
    "dk_qk_norm_rope_f16": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _f32, _vp, _i32, _i32, _i32, _vp]),
    "dk_timestep_embedding_f16": (_i32, [_vp, _i32, _i32, _f32, _i32, _vp, _vp]),
    "dk_latent_to_tokens_f16": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dk_mmdit_set_activation_dtype": (_i32, [_vp, _i32]),
    "dk_ln_modulate_bf16": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp]),
    "dk_qk_norm_rope_bf16": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _f32, _vp, _i32, _i32, _i32, _vp]),
    "dk_rope_table_f32": (_i32, [_vp, _i32, _i32, _i32, C.POINTER(_i32), _i32, _f32, _vp]),
    "dk_timestep_embedding_bf16": (_i32, [_vp, _i32, _i32, _f32, _i32, _vp, _vp]),
    "dk_latent_to_tokens": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    # the step tail: Euler, the coefficient row of the second-order samplers, the guidance modes (mask operands nullable); plain / masked, bf16 / fp16
    **{name + f16: (_i32, args + [_vp]) for name, args in _STEP_ENTRIES.items() for f16 in ("", "_f16")},
    "dk_guidance_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    # stochastic samplers: the generator as an operator (out, seeds u64 [n_img], n_img, n_per_img, draw, stream tag, quad_offset; the step entry is
    # dk_noisy_cfg_step above)
    "dk_philox_normal_f32": (_i32, [_vp, _vp, _i32, _i64, _i32, _i32, C.c_uint64, _vp]),
    # FlowEdit: z, x_src, model_out, ld_out, tokens, zs_out, zt_out, n_img, cfg_on, Hl, Wl, C, p, reshape_order, w_src, w_tar, c, sigma_in, seeds, draw,
    # prime, stream; and the engine's guidance strength per batch row
    **{"dk_flowedit_step" + f16: (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp] + [_i32] * 7 + [_f32] * 4 + [_vp, _i32, _i32, _vp]) for f16 in ("", "_f16")},
    "dk_mmdit_set_guidance_rows": (_i32, [_vp, _fp, _i32]),
    # inpainting: the mask's pixels -> latent cells, the paste-back of the kept pixels
    "dk_mask_to_latent_f32": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "dk_image_composite_u8": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dk_affine_f32": (_i32, [_vp, _vp, _i64, _f32, _f32, _vp]),
    "dk_groupnorm_scratch_floats": (_sz, [_i32, _i32]),
    "dk_groupnorm_bf16": (_i32, [_vp, _vp, _i32, _i64, _i32, _i32, _vp, _vp, _f32, _i32, _vp, _vp]),
    "dk_softmax_rows_bf16": (_i32, [_vp, _i32, _i32, _i32, _vp]),
    "dk_transpose_bf16": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "dk_mmdit_create": (_i32, [C.POINTER(dk_mmdit_config), C.POINTER(_vp)]),
    "dk_mmdit_destroy": (None, [_vp]),
    "dk_mmdit_bind": (_i32, [_vp, C.c_char_p, _vp]),
    "dk_mmdit_mod_rows": (_i32, [_vp]),
    "dk_mmdit_mod_offset": (_i32, [_vp, _i32, _i32]),
    "dk_mmdit_score_bound": (_f32, [_vp, _i32, _i32]),
    "dk_mmdit_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32, _i32, _i32]),
    "dk_mmdit_prepare": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "dk_mmdit_cache_modulation_params": (_i32, [_vp, _vp, _fp, _i32, _vp]),
    "dk_mmdit_forward": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp]),
    "dk_mmdit_cache_context": (_i32, [_vp, _vp, _vp]),
    "dk_mmdit_run_blocks": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "dk_mmdit_debug_buffer": (_vp, [_vp, _i32]),
    # first-block cache: the engine's head / tail entries and the two kernels stand-alone
    "dk_mmdit_set_block_cache": (_i32, [_vp, _i32]),
    "dk_mmdit_reset_block_cache": (_i32, [_vp]),
    "dk_mmdit_forward_head": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp]),
    "dk_mmdit_forward_tail": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "dk_block_probe_bf16": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "dk_block_probe_f16": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "dk_block_residual_bf16": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    "dk_block_residual_f16": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    # reference-image conditioning: the engine's grid / hoist entries and the RoPE table for several grids
    "dk_mmdit_set_reference_grid": (_i32, [_vp, _i32, _i32]),
    "dk_mmdit_cache_reference": (_i32, [_vp, _vp, _i32, _vp]),
    "dk_rope_table_segments_f32": (_i32, [_vp, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, _f32, _vp]),
    # channel-concatenated conditioning (FLUX.1 Fill / Canny / Depth): the engine's width / hoist entries and the two operators
    "dk_mmdit_set_condition_width": (_i32, [_vp, _i32]),
    "dk_mmdit_cache_condition": (_i32, [_vp, _vp, _i32, _vp]),
    # MMDiT-X dual-attention blocks (Stable Diffusion 3.5 medium): the engine's setter and the LayerNorm pass with two modulated outputs
    "dk_mmdit_set_dual_attention": (_i32, [_vp, _i32]),
    # skip-layer guidance: the engine's forked row group (the step entry is dk_slg_cfg_step above)
    "dk_mmdit_set_skip_layers": (_i32, [_vp, C.POINTER(_i32), _i32, _i32]),
    # perturbed-attention guidance: the same fork with identity attention in the blocks named
    "dk_mmdit_set_perturbed_attention": (_i32, [_vp, C.POINTER(_i32), _i32, _i32]),
    **{"dk_ln_modulate_dual_" + el: (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                                            _i32, _f32, _vp]) for el in ("bf16", "f16")},
    # SD3 ControlNet: the control-net engine's setter / hoist / forward, the main engine's taps, and the LayerNorm pass with a residual tap in front
    "dk_mmdit_set_control_net": (_i32, [_vp, _i32]),
    "dk_mmdit_cache_control_image": (_i32, [_vp, _vp, _i32, _vp]),
    "dk_mmdit_control_forward": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp]),
    "dk_mmdit_set_control_taps": (_i32, [_vp, _vp, _i32, _f32]),
    **{"dk_ln_modulate_add_" + el: (_i32, [_vp, _vp, _i32, _f32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                                           _i32, _f32, _vp]) for el in ("bf16", "f16")},
    # FLUX ControlNet: the control-net engine of FLUX geometry, the main engine's double- and single-block taps, the one-job joint LayerNorm pass
    "dk_mmdit_set_flux_control_net": (_i32, [_vp, _i32]),
    "dk_mmdit_set_flux_control_taps": (_i32, [_vp, _vp, _i32, _i32, _f32]),
    "dk_ln_modulate_add_joint_bf16": (_i32, [_vp, _i32, _vp, _i32, _f32, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp]),
    # FLUX IP-Adapter: the engine's setter / hoist / scale and the decoupled image-prompt attention kernel
    "dk_mmdit_set_ip_adapter": (_i32, [_vp, _i32, _i32]),
    "dk_mmdit_cache_ip_tokens": (_i32, [_vp, _vp, _i32, _vp]),
    "dk_mmdit_set_ip_scale": (_i32, [_vp, _f32]),
    "dk_ip_attention_bf16": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp]),
    "dk_image_mask_out_f32": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "dk_fill_condition_tokens": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dk_vae_create": (_i32, [C.POINTER(dk_vae_config), C.POINTER(_vp)]),
    "dk_vae_destroy": (None, [_vp]),
    "dk_vae_bind": (_i32, [_vp, C.c_char_p, _vp]),
    "dk_vae_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32]),
    "dk_vae_decode": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dk_vae_encoder_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32]),
    "dk_vae_encode": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _sz, _vp]),
    "dk_latent_sample_f32": (_i32, [_vp, _i32, _vp, _vp, _i64, _i32, _vp]),
    # float16 element type of the VAE halves and their operators
    "dk_vae_set_dtype": (_i32, [_vp, _i32]),
    "dk_latent_sample_f16": (_i32, [_vp, _i32, _vp, _vp, _i64, _i32, _vp]),
    "dk_conv3x3_f16": (_i32, [C.POINTER(dk_conv_desc), _vp]),
    "dk_conv3x3_plan": (_i32, [C.POINTER(dk_conv_desc), C.POINTER(dk_gemm_plan_t)]),
    "dk_conv3x3_plan_f16": (_i32, [C.POINTER(dk_conv_desc), C.POINTER(dk_gemm_plan_t)]),
    # ... with the K-split workspace of the engines' convs (additive in ABI 5)
    **{"dk_conv3x3_ws_" + el: (_i32, [C.POINTER(dk_conv_desc), _vp, _sz, _vp]) for el in ("bf16", "f16")},
    **{"dk_conv3x3_ws_plan" + sfx: (_i32, [C.POINTER(dk_conv_desc), _sz, C.POINTER(dk_gemm_plan_t)]) for sfx in ("", "_f16")},
    "dk_conv3x3_gn_f16": (_i32, [C.POINTER(dk_conv_gn_desc), _vp]),
    "dk_groupnorm_table_f16": (_i32, [_vp, _i32, C.c_int64, _i32, _i32, _vp, _vp, C.c_float, _vp, _i32, _vp, _vp]),
    "dk_groupnorm_f16": (_i32, [_vp, _vp, _i32, _i64, _i32, _i32, _vp, _vp, _f32, _i32, _vp, _vp]),
    "dk_attention_d512_f16": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_float, _vp, _vp]),
    "dk_softmax_rows_f16": (_i32, [_vp, _i32, _i32, _i32, _vp]),
    "dk_transpose_f16": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "dk_profile_enable": (_i32, [_i32]),
    "dk_profile_read": (_i32, [_i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "dk_tune_set": (_i32, [C.c_char_p, _i32]),
    "dk_weight_pitch": (_i32, [_i32]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libdk_hip.so, failing loudly if it has not been built
    (``python -c 'import __graft_entry__ as g; g.build()'`` or ``make -C diffusionkit_amd/csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DkHipError(
            f"{LIB_PATH} not found: the HIP extension is not built and there is no CPU fallback. "
            "Run `make -C diffusionkit_amd/csrc` (needs hipcc, cross-compiles for gfx950).")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise DkHipError(f"{LIB_PATH} does not export {name}")
        fn.restype = res
        fn.argtypes = args
    if lib.dk_abi_version() != 5:
        raise DkHipError("libdk_hip.so ABI version mismatch")
    _lib = lib
    return lib


# This host thread's side of dk_attention_set_workspace, with the lifetime of the native thread-local it mirrors: .device -- the device index
# whose buffer the library's pointer holds right now; .bufs -- {device index: buffer}, kept alive while the library may point at one.  A thread
# that exits takes both with it, so a recycled thread ident never passes for "installed" and its buffers are released.
_attn_tls = threading.local()


def ensure_attention_workspace(device) -> None:
    """Hand the library its attention workspace for the calling host thread (dk_attention_set_workspace: the partial results of the
    key-split workgroups of csrc/attention5.hip).  The library keeps ONE pointer per host thread, so the pointer is installed again whenever
    the thread moves to another device (cuda:0 -> cuda:1 -> cuda:0 must not leave device-1 memory behind device-0 launches).
    Engines carry their own region and never consult this one; it serves the stand-alone ops.
    Optional for correctness: without it no launch is split."""
    import torch
    dev = torch.device(device)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    if getattr(_attn_tls, "device", None) == index:
        return
    lib = load()
    n = int(lib.dk_attention_workspace_bytes())
    bufs = _attn_tls.__dict__.setdefault("bufs", {})
    if index not in bufs:
        bufs[index] = torch.empty(max(n, 256), dtype=torch.uint8, device=torch.device("cuda", index))
    check(lib.dk_attention_set_workspace(bufs[index].data_ptr(), n), "dk_attention_set_workspace")
    _attn_tls.device = index


def forget_attention_workspace() -> None:
    """The calling thread's pointer was overwritten from outside (ops.attention(workspace=...), lab): the next ensure_attention_workspace
    installs the regular buffer again.  Other threads' state stays -- their native thread-locals still point at their buffers."""
    _attn_tls.device = None


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().dk_last_error().decode("utf-8", "replace")
        raise DkHipError(f"{what or 'dk call'} failed (rc={rc}): {msg}")
