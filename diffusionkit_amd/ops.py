"""Operator-level Python wrappers over the C ABI (include/dk_hip.h).

Each function is a thin argument marshaller: tensors must already be on the GPU, bf16
(unless stated) and contiguous; the call is enqueued on the current stream.  They mirror one
MLX op of the reference hot path each and are what the parity tests drive.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib
from ._lib import (DK_EPI_BIAS, DK_EPI_BIAS_GELU, DK_EPI_BIAS_SILU, DK_EPI_GATE_RES, DK_EPI_RES)  # noqa: F401
from .engine import _ptr, _require_cuda, _stream

Tensor = torch.Tensor
BF = torch.bfloat16
F16 = torch.float16


def _elem(dtype, what: str) -> str:
    """suffix of the operator entry for an element type: the SD3-path operators exist as ``*_bf16`` and ``*_f16`` (include/dk_hip.h)"""
    if dtype == BF:
        return "bf16"
    if dtype == F16:
        return "f16"
    raise _lib.DkHipError(f"{what}: element type must be torch.bfloat16 or torch.float16, got {dtype}")


def _same_elem(dt, what: str, **tensors) -> None:
    """every optional tensor of an operator call is of the call's element type: mixed element types are refused"""
    for n, t in tensors.items():
        if t is not None and t.dtype != dt:
            raise _lib.DkHipError(f"{what}: {n} must be {dt} like x, got {t.dtype} (mixed element types)")


def tune(key: str, value: int) -> None:
    """dk_tune_set: kernel-variant knobs for A/B measurements and parity tests (-1 = automatic)."""
    _lib.check(_lib.load().dk_tune_set(key.encode(), int(value)), "dk_tune_set")


_gemm_ws = {}


def gemm_workspace(device) -> Tensor:
    """Zero-initialised scratch of the GEMM's remainder-wave K split (dk_gemm_workspace_bytes), one per device."""
    key = str(device)
    if key not in _gemm_ws:
        _gemm_ws[key] = torch.zeros(_lib.load().dk_gemm_workspace_bytes(), dtype=torch.uint8, device=device)
    return _gemm_ws[key]


def linear(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, epilogue: int = DK_EPI_BIAS,
           gate: Optional[Tensor] = None, res: Optional[Tensor] = None, gate_seg_len: int = 0,
           alpha: float = 1.0, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """nn.Linear (+ fused epilogue).  x: [M, K]; w: [N, K]; gate: [n_batch, N]; res: [M, N].  bf16 tensors, or all float16 (dk_gemm_f16)."""
    lib = _lib.load()
    el = _elem(x.dtype, "linear")
    for n, t in (("x", x), ("w", w)):
        _require_cuda(t, n, x.dtype)
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    d = _lib.dk_gemm_desc()
    d.A, d.W, d.C = x.data_ptr(), w.data_ptr(), out.data_ptr()
    d.bias, d.gate, d.res = _ptr(bias), _ptr(gate), _ptr(res)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldc, d.ldr = x.stride(0), out.stride(0), (res.stride(0) if res is not None else 0)
    d.gate_seg_len = gate_seg_len
    d.gate_stride = gate.stride(0) if gate is not None else 0
    d.alpha, d.epilogue = alpha, epilogue
    if workspace is not None:
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel()
    _lib.check(getattr(lib, "dk_gemm_" + el)(C.byref(d), _stream()), "dk_gemm_" + el)
    return out


def gemm_desc_call(dtype=BF, **kw) -> None:
    """Raw descriptor call (segment mappings etc.); keyword names = dk_gemm_desc fields,
    tensors are converted to pointers.  ``dtype``: element type of every tensor named (bf16 | float16)."""
    lib = _lib.load()
    el = _elem(dtype, "gemm_desc_call")
    d = _lib.dk_gemm_desc()
    for k, v in kw.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    _lib.check(getattr(lib, "dk_gemm_" + el)(C.byref(d), _stream()), "dk_gemm_" + el)


def gemm_plan(d: dict, d2: Optional[dict] = None, dtype=BF):
    """dk_gemm_plan / dk_gemm_plan_f16: what the call would launch (host only; pointers may be made-up, aligned integers)."""
    a, b = _fill(_lib.dk_gemm_desc, d), _fill(_lib.dk_gemm_desc, d2)
    plan = _lib.dk_gemm_plan_t()
    name = "dk_gemm_plan" if _elem(dtype, "gemm_plan") == "bf16" else "dk_gemm_plan_f16"
    _lib.check(getattr(_lib.load(), name)(_ref(a), _ref(b), C.byref(plan)), name)
    return plan


def _fill(struct, fields):
    """a ctypes struct from {field: value}; tensors become their device pointers, None a NULL struct pointer"""
    if fields is None:
        return None
    s = struct()
    for k, v in fields.items():
        setattr(s, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return s


def _ref(s):
    return C.byref(s) if s is not None else None


def gemm_fused_call(d: dict, side: Optional[dict] = None, d2: Optional[dict] = None, side2: Optional[dict] = None, dtype=BF) -> None:
    """dk_gemm_fused_bf16 (``dtype`` float16: dk_gemm_fused_f16): the launch forms of the engines -- column split, QKNorm + RoPE in the tile tail, an image + text pair.
    ``d`` / ``d2``: dk_gemm_desc fields, ``side`` / ``side2``: dk_gemm_side fields (tensors are converted to pointers)."""
    a, f, b, f2 = _fill(_lib.dk_gemm_desc, d), _fill(_lib.dk_gemm_side, side), _fill(_lib.dk_gemm_desc, d2), _fill(_lib.dk_gemm_side, side2)
    name = "dk_gemm_fused_" + _elem(dtype, "gemm_fused_call")
    _lib.check(getattr(_lib.load(), name)(_ref(a), _ref(f), _ref(b), _ref(f2), _stream()), name)


def gemm_fused_plan(d: dict, side: Optional[dict] = None, d2: Optional[dict] = None, side2: Optional[dict] = None):
    """dk_gemm_fused_plan: what ``gemm_fused_call`` with these arguments would launch (host only; pointers may be made-up, aligned integers)."""
    a, f, b, f2 = _fill(_lib.dk_gemm_desc, d), _fill(_lib.dk_gemm_side, side), _fill(_lib.dk_gemm_desc, d2), _fill(_lib.dk_gemm_side, side2)
    plan = _lib.dk_gemm_plan_t()
    _lib.check(_lib.load().dk_gemm_fused_plan(_ref(a), _ref(f), _ref(b), _ref(f2), C.byref(plan)), "dk_gemm_fused_plan")
    return plan


def gemm_fp8_fused_call(d: dict, side: Optional[dict] = None, d2: Optional[dict] = None, side2: Optional[dict] = None) -> None:
    """dk_gemm_fp8_fused: the same forms on the fp8 GEMM (dk_gemm_fp8_desc / dk_gemm_fp8_side fields)."""
    a, f = _fill(_lib.dk_gemm_fp8_desc, d), _fill(_lib.dk_gemm_fp8_side, side)
    b, f2 = _fill(_lib.dk_gemm_fp8_desc, d2), _fill(_lib.dk_gemm_fp8_side, side2)
    _lib.check(_lib.load().dk_gemm_fp8_fused(_ref(a), _ref(f), _ref(b), _ref(f2), _stream()), "dk_gemm_fp8_fused")


def attention_desc_call(dtype=BF, **kw) -> None:
    """dk_attention_desc_bf16 (``dtype`` float16: dk_attention_desc_f16, head_dim 64): attention with the query QKNorm + RoPE in the Q load and / or the MX-fp8 output copy; keyword names =
    dk_attention_desc fields."""
    _lib.ensure_attention_workspace(torch.cuda.current_device())
    d = _fill(_lib.dk_attention_desc, kw)
    name = "dk_attention_desc_" + _elem(dtype, "attention_desc_call")
    _lib.check(getattr(_lib.load(), name)(C.byref(d), _stream()), name)


def attention_plan(dtype=BF, workspace_bytes=0, o8_split=0, **kw):
    """dk_attention_plan / dk_attention_plan_f16: what ``attention_desc_call`` with these dk_attention_desc fields and a workspace of ``workspace_bytes``
    bytes would launch (host only; pointers may be made-up, aligned integers).  ``o8_split``: the engines' row order of the MX-fp8 copy."""
    d, plan = _fill(_lib.dk_attention_desc, kw), _lib.dk_attention_plan_t(o8_split=o8_split)
    name = "dk_attention_plan" if _elem(dtype, "attention_plan") == "bf16" else "dk_attention_plan_f16"
    _lib.check(getattr(_lib.load(), name)(C.byref(d), workspace_bytes, C.byref(plan)), name)
    return plan


_zero_pages = {}


def zero_page(device) -> Tensor:
    key = str(device)
    if key not in _zero_pages:
        _zero_pages[key] = torch.zeros(256, dtype=BF, device=device)
    return _zero_pages[key]


def conv3x3(x: Tensor, w: Tensor, bias: Optional[Tensor], upsample: bool = False, res: Optional[Tensor] = None,
            downsample: bool = False, workspace: Optional[Tensor] = None) -> Tensor:
    """nn.Conv2d k3 on NHWC; w: [O,3,3,C] (or flattened [O, 9C]); C multiple of 64.  Default: stride 1, pad 1
    (``upsample``: over the nearest-x2 view of x); ``downsample``: stride 2 over x padded by one zero row /
    column at the bottom / right (vae.py:141-143).  bf16 tensors, or all float16 (dk_conv3x3_f16).
    ``workspace``: the K-split scratch (``gemm_workspace``) the VAE engines attach to their convs (dk_conv3x3_ws_bf16 / _f16)."""
    assert not (upsample and downsample)
    lib = _lib.load()
    el = _elem(x.dtype, "conv3x3")
    _require_cuda(x, "x", x.dtype)
    _require_cuda(w, "w", x.dtype)
    _same_elem(x.dtype, "conv3x3", bias=bias, res=res)
    B, Hs, Ws, Cc = x.shape
    H, W_ = (Hs * 2, Ws * 2) if upsample else (Hs // 2, Ws // 2) if downsample else (Hs, Ws)
    if downsample:
        assert Hs % 2 == 0 and Ws % 2 == 0, "stride-2 conv needs even input sizes"
    O = w.shape[0]
    ldy = (O + 3) // 4 * 4
    y = torch.empty(B, H, W_, ldy, dtype=x.dtype, device=x.device)
    d = _lib.dk_conv_desc()
    d.x, d.w, d.y, d.bias, d.res = x.data_ptr(), w.data_ptr(), y.data_ptr(), _ptr(bias), _ptr(res)
    d.zeros = zero_page(x.device).data_ptr()
    d.B, d.H, d.W, d.C, d.O = B, H, W_, Cc, O
    d.ldy, d.ldr = ldy, (res.shape[-1] if res is not None else 0)
    d.upsample = 2 if downsample else int(upsample)
    d.epilogue = DK_EPI_RES if res is not None else DK_EPI_BIAS
    if workspace is not None:
        _lib.check(getattr(lib, "dk_conv3x3_ws_" + el)(C.byref(d), workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()),
                   "dk_conv3x3_ws_" + el)
    else:
        _lib.check(getattr(lib, "dk_conv3x3_" + el)(C.byref(d), _stream()), "dk_conv3x3_" + el)
    return y[..., :O]


def conv3x3_plan(B: int, H: int, W: int, C_in: int, O: int, upsample: int = 0, dtype=BF, res: bool = False, workspace: int = 0):
    """dk_conv3x3_ws_plan / dk_conv3x3_ws_plan_f16: the route a ``conv3x3`` call of this OUTPUT size would take with a K-split workspace of
    ``workspace`` bytes (0: none -- dk_conv3x3_plan's answer) (host only, nothing is launched; the pointers are made-up, aligned integers)."""
    d = _lib.dk_conv_desc()
    d.x, d.w, d.y, d.bias, d.zeros = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    d.res = 0x60000 if res else None
    d.B, d.H, d.W, d.C, d.O = B, H, W, C_in, O
    d.ldy, d.ldr = (O + 3) // 4 * 4, (O if res else 0)
    d.upsample = int(upsample)
    d.epilogue = DK_EPI_RES if res else DK_EPI_BIAS
    plan = _lib.dk_gemm_plan_t()
    name = "dk_conv3x3_ws_plan" if _elem(dtype, "conv3x3_plan") == "bf16" else "dk_conv3x3_ws_plan_f16"
    _lib.check(getattr(_lib.load(), name)(C.byref(d), int(workspace), C.byref(plan)), name)
    return plan


def attention_d512(q: Tensor, k: Tensor, v: Tensor, scale: Optional[float] = None) -> Tensor:
    """single-head attention over head_dim 512 (VAE mid block, vae.py:28-57), flash-style; q / k / v: [B, T, 512] bf16, or all float16."""
    lib = _lib.load()
    name = "dk_attention_d512_" + _elem(q.dtype, "attention_d512")
    for n, t in (("q", q), ("k", k), ("v", v)):
        _require_cuda(t, n, q.dtype)
    B, T, Cc = q.shape
    assert Cc == 512, f"attention_d512: head_dim {Cc}, the kernel is built for 512"
    for n, t in (("q", q), ("k", k), ("v", v)):
        assert t.shape == q.shape and t.is_contiguous(), f"attention_d512: {n} must be a dense [B, T, 512] tensor (row pitch 512)"
    out = torch.empty_like(q)
    vt = torch.empty(B * 512 * lib.dk_attention_d512_tp(T), dtype=q.dtype, device=q.device)
    scale = scale if scale is not None else 1.0 / math.sqrt(Cc)
    _lib.check(getattr(lib, name)(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, T, Cc, Cc, scale, vt.data_ptr(), _stream()), name)
    return out


def groupnorm_table(x: Optional[Tensor], gamma: Tensor, beta: Tensor, groups: int, eps: float, partials: Optional[Tensor] = None,
                    shape=None) -> Tensor:
    """(scale | shift) table [B, 2, C] fp32 of nn.GroupNorm over NHWC ``x`` -- or over the tensor whose output-statistics
    ``partials`` [B, n, G, 2] a ``conv3x3_gn`` launch produced (then ``shape`` = (B, H*W, C)).  The element type is ``gamma``'s
    (bf16 | float16); ``beta`` and ``x`` must match it."""
    lib = _lib.load()
    name = "dk_groupnorm_table_" + _elem(gamma.dtype, "groupnorm_table")
    _same_elem(gamma.dtype, "groupnorm_table", beta=beta, x=x)
    if x is not None:
        _require_cuda(x, "x", gamma.dtype)
        B, HW, Cc = x.shape[0], x.shape[1] * x.shape[2], x.shape[3]
        n_part = 0
        scratch = torch.empty(lib.dk_groupnorm_scratch_floats(B, groups), dtype=torch.float32, device=x.device)
    else:
        B, HW, Cc = shape
        n_part = partials.shape[1]
        scratch = torch.empty(B * max(1024, n_part) * 2 * groups + B * groups * 2, dtype=torch.float32, device=partials.device)
        scratch[:partials.numel()] = partials.reshape(-1)
    ss = torch.empty(B, 2, Cc, dtype=torch.float32, device=gamma.device)
    _lib.check(getattr(lib, name)(_ptr(x), B, HW, Cc, groups, gamma.data_ptr(), beta.data_ptr(), eps, scratch.data_ptr(),
                                  n_part, ss.data_ptr(), _stream()), name)
    return ss


def conv3x3_gn(x: Tensor, w: Tensor, bias: Tensor, gn_table: Optional[Tensor] = None, silu: bool = True, res: Optional[Tensor] = None,
               x2: Optional[Tensor] = None, bias2: Optional[Tensor] = None, stats_groups: int = 0, upsample: bool = False,
               image: bool = False):
    """norm -> silu -> conv3x3 as one launch (csrc/conv_halo.hip): ``x`` raw NHWC, ``gn_table`` from ``groupnorm_table``;
    ``w`` [O, 9 C (+ C2)] K-major.  Returns y, or (y, partials) with ``stats_groups``, or (image_f32, image_u8, raw) with ``image``.
    bf16 tensors, or all float16 (dk_conv3x3_gn_f16: always conv_halo.hip's kernel, whatever ``tune("conv_v4", v)`` says)."""
    lib = _lib.load()
    dt = x.dtype
    name = "dk_conv3x3_gn_" + _elem(dt, "conv3x3_gn")
    _require_cuda(x, "x", dt)
    _require_cuda(w, "w", dt)
    _same_elem(dt, "conv3x3_gn", bias=bias, res=res, x2=x2, bias2=bias2)
    B, Hs, Ws, Cc = x.shape
    H, W_ = (Hs * 2, Ws * 2) if upsample else (Hs, Ws)
    O = w.shape[0]
    w2 = w.reshape(O, -1)
    d = _lib.dk_conv_gn_desc()
    d.x, d.w, d.bias, d.res = x.data_ptr(), w2.data_ptr(), bias.data_ptr(), _ptr(res)
    d.gn_scale_shift, d.gn_silu = _ptr(gn_table), int(silu)
    d.x2, d.bias2 = _ptr(x2), _ptr(bias2)
    d.B, d.H, d.W, d.C, d.O, d.C2 = B, H, W_, Cc, O, (x2.shape[-1] if x2 is not None else 0)
    d.ldw, d.upsample = w2.shape[1], int(upsample)
    out = None
    if image:
        img = torch.empty(B, H, W_, 3, dtype=torch.float32, device=x.device)
        u8 = torch.empty(B, H, W_, 3, dtype=torch.uint8, device=x.device)
        raw = torch.empty(B, H, W_, 4, dtype=dt, device=x.device)
        d.image_f32, d.image_u8, d.raw_bf16 = img.data_ptr(), u8.data_ptr(), raw.data_ptr()
        out = (img, u8, raw)
    else:
        y = torch.empty(B, H, W_, O, dtype=dt, device=x.device)
        d.y, d.ldy, d.ldr = y.data_ptr(), O, (res.shape[-1] if res is not None else 0)
        out = y
        if stats_groups:
            part = torch.empty(B, (H // 16) * (W_ // 16), stats_groups, 2, dtype=torch.float32, device=x.device)
            d.stats_partial, d.stats_groups = part.data_ptr(), stats_groups
            out = (y, part)
    _lib.check(getattr(lib, name)(C.byref(d), _stream()), name)
    return out


def attention(qkv: Tensor, H: int, D: int, scale: Optional[float] = None, workspace: Optional[Tensor] = None,
              score_bound: Optional[float] = None, qn=None) -> Tensor:
    """SDPA over a token-major [B, S, 3*H*D] projection buffer -> [B, S, H*D].  ``workspace``: lab only (trace buffer of attention4.hip's
    DK4_TRACE builds, dk_attention_set_workspace for the duration of the call).
    ``score_bound``: the caller's PROMISE that |scale * q.k| <= score_bound for every query / key pair of the call (dk_attention_desc.score_bound: not
    checked; it lets the one-wave-per-SIMD kernel drop its running row maximum).  ``qn``: (qn_a, qn_b, qn_split[, q_rope]), the query QKNorm (+ RoPE)
    of the kernel's Q load as ``attention_desc_call`` names them (qn_a / qn_b may be None: RoPE only).  Either one sends the call through
    dk_attention_desc_bf16."""
    lib = _lib.load()
    _require_cuda(qkv, "qkv", BF)
    if score_bound is not None or qn is not None:
        assert workspace is None, "attention: the lab workspace goes with the plain call only"
        B, S, ld = qkv.shape
        h = H * D
        out = torch.empty(B, S, h, dtype=BF, device=qkv.device)
        kw = dict(q=qkv, k=qkv[:, :, h:], v=qkv[:, :, 2 * h:], out=out, B=B, H=H, S=S, D=D, ld=ld, ldo=h,
                  scale=scale if scale is not None else 1.0 / math.sqrt(D), score_bound=float(score_bound or 0.0))
        if qn is not None:
            kw.update(qn_a=qn[0], qn_b=qn[1], qn_split=int(qn[2]), qn_eps=1e-6, q_rope=qn[3] if len(qn) > 3 else None)
        attention_desc_call(BF, **kw)
        return out
    if workspace is None:
        _lib.ensure_attention_workspace(qkv.device)
    B, S, ld = qkv.shape
    h = H * D
    out = torch.empty(B, S, h, dtype=BF, device=qkv.device)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    base = qkv.data_ptr()
    if workspace is not None:
        _lib.check(lib.dk_attention_set_workspace(workspace.data_ptr(), workspace.numel()), "dk_attention_set_workspace")
    try:
        _lib.check(lib.dk_attention_bf16(base, base + 2 * h, base + 4 * h, out.data_ptr(), B, H, S, D, ld, h, scale, _stream()),
                   "dk_attention_bf16")
    finally:
        if workspace is not None:
            lib.dk_attention_set_workspace(None, 0)
            _lib.forget_attention_workspace()  # (this thread's next call hands the library its regular workspace again)
    return out


def attention_identity(qkv: Tensor, H: int, D: int, ident_from: int, scale: Optional[float] = None, qn=None) -> Tensor:
    """dk_attention_identity_bf16 / _f16 by the dtype of ``qkv``: ``attention`` over a token-major [B, S, 3*H*D] buffer in which a query
    s >= ``ident_from`` sees the keys [0, ident_from) and its own key only (perturbed-attention guidance; head_dim 64).  ``qn``: optionally
    (qn_a, qn_b, qn_split[, q_rope]), the query QKNorm (+ RoPE) of the kernel's Q load, as ``attention_desc_call`` names them."""
    el = _elem(qkv.dtype, "attention_identity")
    _require_cuda(qkv, "qkv", qkv.dtype)
    B, S, ld = qkv.shape
    h = H * D
    out = torch.empty(B, S, h, dtype=qkv.dtype, device=qkv.device)
    kw = dict(q=qkv, k=qkv[:, :, h:], v=qkv[:, :, 2 * h:], out=out, B=B, H=H, S=S, D=D, ld=ld, ldo=h,
              scale=scale if scale is not None else 1.0 / math.sqrt(D))
    if qn is not None:
        _same_elem(qkv.dtype, "attention_identity", qn_a=qn[0], qn_b=qn[1])
        kw.update(qn_a=qn[0], qn_b=qn[1], qn_split=int(qn[2]), qn_eps=1e-6, q_rope=qn[3] if len(qn) > 3 else None)
    d = _fill(_lib.dk_attention_desc, kw)
    name = "dk_attention_identity_" + el
    _lib.check(getattr(_lib.load(), name)(C.byref(d), int(ident_from), _stream()), name)
    return out


def attention_identity_plan(ident_from: int, dtype=BF, **kw):
    """dk_attention_identity_plan: what ``attention_identity`` with these dk_attention_desc fields would launch (host only; pointers may be
    made-up, aligned integers), and every refusal of the launch."""
    d, plan = _fill(_lib.dk_attention_desc, kw), _lib.dk_attention_plan_t()
    f16 = int(_elem(dtype, "attention_identity_plan") != "bf16")
    _lib.check(_lib.load().dk_attention_identity_plan(C.byref(d), int(ident_from), f16, C.byref(plan)), "dk_attention_identity_plan")
    return plan


def ln_modulate(x: Tensor, shift: Tensor, scale: Tensor, eps: float = 1e-6) -> Tensor:
    """x: [B, S, h]; shift/scale: [B, h] -> [B, S, h] (bf16, or all float16)."""
    lib = _lib.load()
    name = "dk_ln_modulate_" + _elem(x.dtype, "ln_modulate")
    _require_cuda(x, "x")
    for n, t in (("shift", shift), ("scale", scale)):
        if t.dtype != x.dtype:
            raise _lib.DkHipError(f"{n} must be {x.dtype}, got {t.dtype}")
    B, S, h = x.shape
    out = torch.empty_like(x)
    _lib.check(getattr(lib, name)(x.data_ptr(), h, out.data_ptr(), h, B * S, h, shift.data_ptr(), scale.data_ptr(),
                                  shift.stride(0), S, B * S, 0, eps, _stream()), name)
    return out


def ln_modulate_dual(x: Tensor, shift_a: Tensor, scale_a: Tensor, shift_b: Tensor, scale_b: Tensor, text=None, eps: float = 1e-6):
    """One LayerNorm pass, two modulated outputs (dk_ln_modulate_dual_*, the first launch of an MMDiT-X dual-attention block).
    x: [B, S, h]; shift_* / scale_*: [B, h] views of ONE modulation table (equal row strides) -> (out_a, out_b), each what ``ln_modulate`` gives
    for its pair.  ``text``: optionally (x1 [B, S1, h], shift1, scale1), a plain second row set in the same launch -> (out_a, out_b, out1)."""
    lib = _lib.load()
    name = "dk_ln_modulate_dual_" + _elem(x.dtype, "ln_modulate_dual")
    _require_cuda(x, "x")
    mods = [("shift_a", shift_a), ("scale_a", scale_a), ("shift_b", shift_b), ("scale_b", scale_b)]
    x1 = None
    if text is not None:
        x1, shift1, scale1 = text
        _require_cuda(x1, "text x")
        mods += [("text shift", shift1), ("text scale", scale1)]
    B, S, h = x.shape
    for n, t in mods:
        if t.dtype != x.dtype or t.stride(0) != shift_a.stride(0) or tuple(t.shape) != (B, h) or t.stride(1) != 1:
            raise _lib.DkHipError(f"{n} must be a [{B}, {h}] {x.dtype} view with the row stride of shift_a")
    out_a, out_b = torch.empty_like(x), torch.empty_like(x)
    if x1 is not None:
        if x1.dtype != x.dtype or x1.shape[0] != B or x1.shape[2] != h:
            raise _lib.DkHipError("text x must be [B, S1, h] in x's dtype")
        out1, S1 = torch.empty_like(x1), x1.shape[1]
        args1 = (x1.data_ptr(), out1.data_ptr(), B * S1, mods[4][1].data_ptr(), mods[5][1].data_ptr(), S1)
    else:
        args1 = (None, None, 0, None, None, 0)
    _lib.check(getattr(lib, name)(x.data_ptr(), out_a.data_ptr(), out_b.data_ptr(), B * S, shift_a.data_ptr(), scale_a.data_ptr(),
                                  shift_b.data_ptr(), scale_b.data_ptr(), S, *args1, h, h, h, shift_a.stride(0), S, args1[5], eps, _stream()), name)
    return (out_a, out_b) if x1 is None else (out_a, out_b, out1)


def ln_modulate_add(x: Tensor, tap: Tensor, s: float, shift: Tensor, scale: Tensor, text=None, eps: float = 1e-6):
    """The LayerNorm pass with a residual tap in front (dk_ln_modulate_add_*, the first launch of a main-model block behind a ControlNet tap):
    x <- round(fmaf(s, tap, x)) IN PLACE, fp32 with one rounding to x's dtype, and out = ``ln_modulate`` of the new rows -- one read of x.
    x: [B, S, h], contiguous or the row range of a joint buffer (a view ``joint[:, a:b]`` with unit inner stride); tap: [B, S, h] contiguous;
    shift / scale: [B, h] views of one modulation table.  ``text``: optionally (x1 [B, S1, h], shift1, scale1), a plain second row set of the same
    row pitch in the same launch, read only.  Returns (x, out) or (x, out, out1)."""
    lib = _lib.load()
    name = "dk_ln_modulate_add_" + _elem(x.dtype, "ln_modulate_add")
    if not x.is_cuda or x.dim() != 3:
        raise _lib.DkHipError("x must be a [B, S, h] tensor on the GPU; there is no CPU path")
    B, S, h = x.shape
    ldx = x.stride(1)
    if x.stride(2) != 1 or (B > 1 and x.stride(0) % ldx != 0):
        raise _lib.DkHipError("x must have unit inner stride and a batch stride that is a whole number of rows")
    _require_cuda(tap, "tap", x.dtype)
    if tuple(tap.shape) != (B, S, h):
        raise _lib.DkHipError(f"tap shape {tuple(tap.shape)} != {(B, S, h)}")
    mods = [("shift", shift), ("scale", scale)]
    x1 = None
    if text is not None:
        x1, shift1, scale1 = text
        mods += [("text shift", shift1), ("text scale", scale1)]
    for n, t in mods:
        if t.dtype != x.dtype or t.stride(0) != shift.stride(0) or tuple(t.shape) != (B, h) or t.stride(1) != 1:
            raise _lib.DkHipError(f"{n} must be a [{B}, {h}] {x.dtype} view with the row stride of shift")
    out = torch.empty(B, S, h, dtype=x.dtype, device=x.device)
    if x1 is not None:
        if not x1.is_cuda or x1.dtype != x.dtype or x1.dim() != 3 or x1.shape[0] != B or x1.shape[2] != h:
            raise _lib.DkHipError("text x must be [B, S1, h] in x's dtype on the GPU")
        if x1.stride(2) != 1 or x1.stride(1) != ldx or (B > 1 and x1.stride(0) % ldx != 0):
            raise _lib.DkHipError("text x must have x's row pitch, unit inner stride and a batch stride that is a whole number of rows")
        S1 = x1.shape[1]
        out1 = torch.empty(B, S1, h, dtype=x.dtype, device=x.device)
        args1 = (x1.data_ptr(), out1.data_ptr(), B * S1, mods[2][1].data_ptr(), mods[3][1].data_ptr(), S1)
        xss1 = x1.stride(0) // ldx if B > 1 else S1
    else:
        args1, xss1 = (None, None, 0, None, None, 0), 0
    xss = x.stride(0) // ldx if B > 1 else S
    _lib.check(getattr(lib, name)(x.data_ptr(), tap.data_ptr(), h, float(s), out.data_ptr(), B * S, shift.data_ptr(), scale.data_ptr(), S, *args1,
                                  ldx, h, h, shift.stride(0), xss, xss1, eps, _stream()), name)
    return (x, out) if x1 is None else (x, out, out1)


def ln_modulate_add_joint(x: Tensor, s_t: int, tap: Tensor, s: float, shift: Tensor, scale: Tensor, eps: float = 1e-6):
    """The LayerNorm pass of a joint stream with a residual tap in front of its image rows (dk_ln_modulate_add_joint_bf16: a single block's
    LayerNorm behind a FLUX ControlNet tap; the final layer's with ``s_t`` = 0).  x: [B, S, h] bf16 contiguous, the first ``s_t`` rows of every
    batch row text; tap: [B, S - s_t, h] contiguous -- there are no tap rows for the text rows.  Image rows: x <- round(fmaf(s, tap, x)) IN
    PLACE (fp32, one rounding); text rows: untouched.  out = ``ln_modulate`` of the rows as they then are.  shift / scale: [B, h] views of one
    modulation table.  Returns (x, out)."""
    lib = _lib.load()
    name = "dk_ln_modulate_add_joint_bf16"
    _require_cuda(x, "x", BF)
    if x.dim() != 3 or not x.is_contiguous():
        raise _lib.DkHipError("x must be a contiguous [B, S, h] tensor")
    B, S, h = x.shape
    s_t = int(s_t)
    if not 0 <= s_t < S:
        raise _lib.DkHipError(f"s_t = {s_t}: must lie in [0, S = {S})")
    _require_cuda(tap, "tap", BF)
    if tuple(tap.shape) != (B, S - s_t, h) or not tap.is_contiguous():
        raise _lib.DkHipError(f"tap must be a contiguous {(B, S - s_t, h)} tensor, got {tuple(tap.shape)}")
    for n, t in (("shift", shift), ("scale", scale)):
        if t.dtype != x.dtype or t.stride(0) != shift.stride(0) or tuple(t.shape) != (B, h) or t.stride(1) != 1:
            raise _lib.DkHipError(f"{n} must be a [{B}, {h}] {x.dtype} view with the row stride of shift")
    out = torch.empty(B, S, h, dtype=x.dtype, device=x.device)
    _lib.check(getattr(lib, name)(x.data_ptr(), h, tap.data_ptr(), h, float(s), S, s_t, out.data_ptr(), h, B * S, h, shift.data_ptr(), scale.data_ptr(),
                                  shift.stride(0), S, B * S, 0, eps, _stream()), name)
    return x, out


def ip_attention(qkv: Tensor, s_t: int, qn: Tensor, k: Tensor, v: Tensor, scale: Optional[float] = None, eps: float = 1e-6,
                 head_dim: int = 128) -> Tensor:
    """Decoupled image-prompt attention of the FLUX IP-Adapter (dk_ip_attention_bf16).  qkv: bf16 [B, S, 3h] contiguous, the q / k / v
    projection of a double block with the RAW queries in its first h columns and the first ``s_t`` rows of every batch row text (never
    read, like the k / v columns).  qn: [head_dim] QK-norm weight.  k, v: [B, N, h] views with unit inner stride and one row pitch (1 <= N
    <= 16), image b's keys / values.  Returns dense [B * (S - s_t), h]: softmax over the N keys of ``scale`` * q_n . k, times v, per head,
    q_n the QK-normed (not rotated) queries rounded to bf16."""
    lib = _lib.load()
    name = "dk_ip_attention_bf16"
    _require_cuda(qkv, "qkv", BF)
    if qkv.dim() != 3 or qkv.shape[2] % 3 != 0:
        raise _lib.DkHipError("qkv must be a contiguous [B, S, 3h] tensor")
    B, S, h3 = qkv.shape
    h, s_t = h3 // 3, int(s_t)
    if not 0 <= s_t < S:
        raise _lib.DkHipError(f"s_t = {s_t}: must lie in [0, S = {S})")
    _require_cuda(qn, "qn", BF)
    if tuple(qn.shape) != (head_dim,):
        raise _lib.DkHipError(f"qn must be a [{head_dim}] tensor, got {tuple(qn.shape)}")
    for n, t in (("k", k), ("v", v)):
        if not t.is_cuda or t.dtype != BF or t.dim() != 3 or tuple(t.shape) != (B, k.shape[1], h):
            raise _lib.DkHipError(f"{n} must be a bf16 [{B}, N, {h}] tensor on the GPU, got {tuple(t.shape)}")
        # (an empty N has no strides to speak of: the library refuses it by name below)
        if k.shape[1] > 0 and (t.stride(2) != 1 or t.stride(1) != k.stride(1) or (B > 1 and t.stride(0) != k.shape[1] * k.stride(1))):
            raise _lib.DkHipError(f"{n} must have unit inner stride, k's row pitch and batch rows of N consecutive rows")
    N = int(k.shape[1])
    out = torch.empty(B * (S - s_t), h, dtype=BF, device=qkv.device)
    _lib.check(getattr(lib, name)(qkv.data_ptr(), 3 * h, S - s_t, S, s_t, qn.data_ptr(), k.data_ptr(), v.data_ptr(), k.stride(1), B, N, h, int(head_dim),
                                  float(1.0 / math.sqrt(head_dim) if scale is None else scale), float(eps), out.data_ptr(), _stream()), name)
    return out


def block_probe(x: Tensor, s_t: int, d: Tensor, d_ref: Optional[Tensor] = None):
    """First-block-cache probe (dk_block_probe_*).  x: the joint stream [B, S, h] behind block 0 (text rows first, ``s_t`` of them per
    batch row; only the image rows are read); d: [B, S - s_t, h], X0's image rows on entry, D_cur = round(x - d) on return; d_ref: the
    same shape, or None (den = 0).  Returns (d, probe) with probe f32 [B, 2] = (sum |D_cur - D_ref|, sum |D_ref|) per batch row."""
    lib = _lib.load()
    name = "dk_block_probe_" + _elem(x.dtype, "block_probe")
    _require_cuda(x, "x")
    _require_cuda(d, "d", x.dtype)
    if d_ref is not None:
        _require_cuda(d_ref, "d_ref", x.dtype)
    B, S, h = x.shape
    s_i = S - s_t
    for n, t in (("d", d), ("d_ref", d_ref)):
        if t is not None and tuple(t.shape) != (B, s_i, h):
            raise _lib.DkHipError(f"{n} shape {tuple(t.shape)} != {(B, s_i, h)}")
    rows = torch.empty(B * s_i, 2, dtype=torch.float32, device=x.device)
    probe = torch.empty(B, 2, dtype=torch.float32, device=x.device)
    _lib.check(getattr(lib, name)(x.data_ptr() + s_t * h * x.element_size(), h, s_i, S, d.data_ptr(), _ptr(d_ref), rows.data_ptr(),
                                  probe.data_ptr(), B * s_i, h, s_i, _stream()), name)
    return d, probe


def block_residual(x: Tensor, s_t: int, r: Tensor, reuse: bool) -> Tensor:
    """dk_block_residual_* on the image rows of the joint stream x [B, S, h] and r [B, S - s_t, h].  reuse False: r = round(x - r) in place
    (r held X1's image rows), returns r; True: x's image rows = round(x + r) in place, returns x."""
    lib = _lib.load()
    name = "dk_block_residual_" + _elem(x.dtype, "block_residual")
    _require_cuda(x, "x")
    _require_cuda(r, "r", x.dtype)
    B, S, h = x.shape
    if tuple(r.shape) != (B, S - s_t, h):
        raise _lib.DkHipError(f"r shape {tuple(r.shape)} != {(B, S - s_t, h)}")
    _lib.check(getattr(lib, name)(x.data_ptr() + s_t * h * x.element_size(), h, S - s_t, S, r.data_ptr(), B * (S - s_t), h, int(bool(reuse)),
                                  _stream()), name)
    return x if reuse else r


def qk_norm_rope_(qkv: Tensor, H: int, D: int, qw: Optional[Tensor], kw: Optional[Tensor],
                  rope: Optional[Tensor], pos_off: int = 0, eps: float = 1e-6) -> Tensor:
    """In place on qkv [B, S, 3*H*D] (bf16, or float16 with float16 weights); rope: f32 [S_pos, D/2, 2]."""
    lib = _lib.load()
    name = "dk_qk_norm_rope_" + _elem(qkv.dtype, "qk_norm_rope_")
    _require_cuda(qkv, "qkv")
    for n, t in (("qw", qw), ("kw", kw)):
        if t is not None and t.dtype != qkv.dtype:
            raise _lib.DkHipError(f"{n} must be {qkv.dtype}, got {t.dtype}")
    B, S, ld = qkv.shape
    _lib.check(getattr(lib, name)(qkv.data_ptr(), ld, 0, H * D, B * S, H, D, _ptr(qw), _ptr(kw), eps, _ptr(rope),
                                  S, S, pos_off, _stream()), name)
    return qkv


def rope_table(S_txt: int, gh: int, gw: int, axes, theta: float, device) -> Tensor:
    lib = _lib.load()
    half = sum(a // 2 for a in axes)
    t = torch.empty(S_txt + gh * gw, half, 2, dtype=torch.float32, device=device)
    arr = (C.c_int32 * len(axes))(*axes)
    _lib.check(lib.dk_rope_table_f32(t.data_ptr(), S_txt, gh, gw, arr, len(axes), float(theta), _stream()), "dk_rope_table_f32")
    return t


def rope_table_segments(S_txt: int, segments, axes, theta: float, device) -> Tensor:
    """The table for several grids behind the text rows: ``segments`` = [(gh, gw, index), ...], rows at (index, row, col), rows and
    columns counted from 0 in every segment.  [(gh, gw, 0)] is ``rope_table`` bit for bit."""
    lib = _lib.load()
    segments = [tuple(int(v) for v in s) for s in segments]
    if not segments or any(len(s) != 3 or s[0] < 1 or s[1] < 1 for s in segments):
        raise _lib.DkHipError("segments: a non-empty list of (gh, gw, index) with positive sides")
    half = sum(a // 2 for a in axes)
    t = torch.empty(S_txt + sum(s[0] * s[1] for s in segments), half, 2, dtype=torch.float32, device=device)
    arr = (C.c_int32 * len(axes))(*axes)
    seg = (C.c_int32 * (3 * len(segments)))(*[v for s in segments for v in s])
    _lib.check(lib.dk_rope_table_segments_f32(t.data_ptr(), S_txt, len(segments), seg, arr, len(axes), float(theta), _stream()),
               "dk_rope_table_segments_f32")
    return t


def timestep_embedding(t: Tensor, dim: int, max_period: float, embed_dtype: int, dtype=BF) -> Tensor:
    """evaluated in ``embed_dtype`` (0 bf16, 1 fp16, 2 fp32), stored as ``dtype`` (bf16 | float16)"""
    lib = _lib.load()
    _require_cuda(t, "t", torch.float32)
    name = "dk_timestep_embedding_" + _elem(dtype, "timestep_embedding")
    out = torch.empty(t.numel(), dim, dtype=dtype, device=t.device)
    _lib.check(getattr(lib, name)(t.data_ptr(), t.numel(), dim, float(max_period), embed_dtype, out.data_ptr(), _stream()), name)
    return out


def _mask_per_image(n: int, per_image: int, n_img: int, what: str) -> int:
    """0: one mask of ``per_image`` elements for all images, 1: one per image"""
    if n == per_image:
        return 0
    if n == per_image * n_img:
        return 1
    raise ValueError(f"{what}: the mask holds {n} elements, expected {per_image} (shared) or {n_img} x {per_image} (per image)")


GUIDANCE_MODES = {"cfg": 0, "rescale": 1, "apg": 2}


def _step(what, x, model_out, tokens, n_img, cfg_on, p, reshape_order, sigma, sigma_next, cfg_weight, row=None, blend=None, blend_error=_lib.DkHipError,
          guide=None, slg_scale=None, noise_term=None) -> None:
    """The one call of a step entry, dk_<what> / _f16 by the dtype of ``model_out`` (the argument groups of ``_lib._STEP_ENTRIES``): the operands, then
    ``row`` = (hist, coef, reads_h, writes_h), ``blend`` = (x_orig, noise, mask) and ``guide`` = (mode, phi, eta, r, beta, reads_m, writes_m, m,
    workspace) and ``slg_scale`` where the entry has them, each validated here; ``noise_term`` = (guided, slg, cn, seeds, draw), dk_noisy_cfg_step's
    tail.  ``blend_error``: what a mask operand of the wrong shape raises -- the Euler wrapper
    says ValueError, in its own words, where the others say DkHipError."""
    name = "dk_" + what + ("" if _elem(model_out.dtype, what) == "bf16" else "_f16")
    if guide is not None and guide[0] not in GUIDANCE_MODES:
        raise ValueError(f"unknown guidance mode {guide[0]!r}: valid modes are {', '.join(GUIDANCE_MODES)}")
    _require_cuda(x, "x", torch.float32)
    _require_cuda(model_out, "model_out")
    _require_cuda(tokens, "tokens", model_out.dtype)
    _, hl, wl, c = x.shape
    if row is None:
        tail = (float(sigma_next), float(cfg_weight))
    else:
        hist, coef, reads_h, writes_h = row
        if hist is not None:
            _require_cuda(hist, "hist", torch.float32)
            if hist.shape != x.shape:
                raise _lib.DkHipError(f"hist {tuple(hist.shape)} must have the latent's shape {tuple(x.shape)}")
        cx, cd, ch, hx, hd = (float(v) for v in coef)
        tail = (float(cfg_weight), _ptr(hist), cx, cd, ch, hx, hd, float(sigma_next), int(bool(reads_h)), int(bool(writes_h)))
    if blend is not None:
        x_orig, noise, mask = blend
        for n, t in (("x_orig", x_orig), ("noise", noise), ("mask", mask)):
            if t is None and guide is not None:  # (the only entry whose mask operands may be left out)
                raise _lib.DkHipError(f"{what}: {n} is None while another mask operand is given")
            _require_cuda(t, n, torch.float32)
        if x_orig.shape != x.shape or noise.shape != x.shape:
            raise blend_error(f"x_orig {tuple(x_orig.shape)} and noise {tuple(noise.shape)} must have the latent's shape {tuple(x.shape)}")
        if blend_error is ValueError:  # (a mask of the wrong element count is ``_mask_per_image``'s ValueError)
            if tuple(mask.shape[-2:]) != (hl, wl):
                raise ValueError(f"mask {tuple(mask.shape)} does not end in the latent size {(hl, wl)}")
        elif tuple(mask.shape[-2:]) != (hl, wl) or mask.numel() not in (hl * wl, n_img * hl * wl):
            raise blend_error(f"{what}: mask {tuple(mask.shape)} is neither [{hl}, {wl}] (shared) nor [{n_img}, {hl}, {wl}] (per image)")
        tail += (x_orig.data_ptr(), noise.data_ptr(), mask.data_ptr(), _mask_per_image(mask.numel(), hl * wl, n_img, what))
    elif guide is not None:
        tail += (None, None, None, 0)
    if guide is not None:
        mode, phi, eta, r, beta, reads_m, writes_m, m, workspace = guide
        if m is not None:
            _require_cuda(m, "m", torch.float32)
            if m.shape != x.shape:
                raise _lib.DkHipError(f"m {tuple(m.shape)} must have the latent's shape {tuple(x.shape)}")
        ws_bytes = 0
        if workspace is not None:
            _require_cuda(workspace, "workspace")
            ws_bytes = workspace.numel() * workspace.element_size()
        tail += (GUIDANCE_MODES[mode], float(phi), float(eta), float(r), float(beta), int(bool(reads_m)), int(bool(writes_m)), _ptr(m),
                 _ptr(workspace), ws_bytes)
    if slg_scale is not None:
        tail += (float(slg_scale),)
    if noise_term is not None:
        guided, slg, cn, seeds, draw = noise_term
        if seeds is not None:
            _require_seeds(seeds, n_img, what)
        tail += (int(bool(guided)), int(bool(slg)), float(cn), _ptr(seeds), int(draw))
    _lib.check(getattr(_lib.load(), name)(x.data_ptr(), model_out.data_ptr(), model_out.shape[-1], tokens.data_ptr(), n_img, int(cfg_on), hl, wl, c, p,
                                          reshape_order, float(sigma), *tail, _stream()), name)


def euler_cfg_step(x: Tensor, model_out: Tensor, tokens: Tensor, n_img: int, cfg_on: bool, p: int, reshape_order: int, sigma: float,
                   sigma_next: float, cfg_weight: float) -> None:
    """dk_euler_cfg_step / _f16 by the dtype of ``model_out``: x f32 [n_img, Hl, Wl, C] updated in place, ``tokens`` (same dtype as
    ``model_out``) receives the next step's patchified input."""
    _step("euler_cfg_step", x, model_out, tokens, n_img, cfg_on, p, reshape_order, sigma, sigma_next, cfg_weight)


def euler_cfg_step_masked(x: Tensor, model_out: Tensor, tokens: Tensor, n_img: int, cfg_on: bool, p: int, reshape_order: int, sigma: float,
                          sigma_next: float, cfg_weight: float, x_orig: Tensor, noise: Tensor, mask: Tensor) -> None:
    """dk_euler_cfg_step_masked / _f16 by the dtype of ``model_out``: ``euler_cfg_step``, then x = m * x_new + (1 - m) * (sigma_next * noise +
    (1 - sigma_next) * x_orig) in the same launch.  ``x_orig``, ``noise``: f32 like x; ``mask``: f32 [Hl, Wl] (shared) or [n_img, Hl, Wl]."""
    _step("euler_cfg_step_masked", x, model_out, tokens, n_img, cfg_on, p, reshape_order, sigma, sigma_next, cfg_weight,
          blend=(x_orig, noise, mask), blend_error=ValueError)


def lms_cfg_step(x: Tensor, model_out: Tensor, tokens: Tensor, n_img: int, cfg_on: bool, p: int, reshape_order: int, sigma: float,
                 sigma_next: float, cfg_weight: float, hist: Optional[Tensor], coef, reads_h: bool, writes_h: bool) -> None:
    """dk_lms_cfg_step / _f16 by the dtype of ``model_out``: ``euler_cfg_step`` with the update as a coefficient row, ``coef`` = (cx, cd, ch, hx, hd):
    d = (x - den) / sigma, x = cx x + cd d + ch hist, hist = hx x + hd d.  ``hist``: f32 like x, read only under ``reads_h``, written only under
    ``writes_h`` (None when neither); the rows come from ``sampler.step_plan``."""
    _step("lms_cfg_step", x, model_out, tokens, n_img, cfg_on, p, reshape_order, sigma, sigma_next, cfg_weight, row=(hist, coef, reads_h, writes_h))


def lms_cfg_step_masked(x: Tensor, model_out: Tensor, tokens: Tensor, n_img: int, cfg_on: bool, p: int, reshape_order: int, sigma: float,
                        sigma_next: float, cfg_weight: float, hist: Optional[Tensor], coef, reads_h: bool, writes_h: bool, x_orig: Tensor,
                        noise: Tensor, mask: Tensor) -> None:
    """dk_lms_cfg_step_masked / _f16: ``lms_cfg_step``, then the blend of ``euler_cfg_step_masked`` with the known region re-noised to
    ``sigma_next``, in the same launch."""
    _step("lms_cfg_step_masked", x, model_out, tokens, n_img, cfg_on, p, reshape_order, sigma, sigma_next, cfg_weight,
          row=(hist, coef, reads_h, writes_h), blend=(x_orig, noise, mask))


def guidance_workspace_bytes(n_img: int, hl: int, wl: int, c: int) -> int:
    """dk_guidance_workspace_bytes: what ``guided_cfg_step`` needs as ``workspace`` for a latent [n_img, hl, wl, c]"""
    return int(_lib.load().dk_guidance_workspace_bytes(int(n_img), int(hl), int(wl), int(c)))


def guided_cfg_step(x: Tensor, model_out: Tensor, tokens: Tensor, n_img: int, cfg_on: bool, p: int, reshape_order: int, sigma: float,
                    sigma_next: float, cfg_weight: float, hist: Optional[Tensor], coef, reads_h: bool, writes_h: bool, *, mode: str,
                    workspace: Optional[Tensor], rescale: float = 0.0, eta: float = 0.0, norm_threshold: float = 0.0, momentum: float = 0.0,
                    reads_m: bool = False, writes_m: bool = False, m: Optional[Tensor] = None, x_orig: Optional[Tensor] = None,
                    noise: Optional[Tensor] = None, mask: Optional[Tensor] = None) -> None:
    """dk_guided_cfg_step / _f16 by the dtype of ``model_out``: ``lms_cfg_step`` (with ``x_orig``, ``noise`` and ``mask``: ``lms_cfg_step_masked``)
    with the two predictions combined by ``mode``: "cfg", "rescale" (``rescale`` = phi in [0, 1]) or "apg" (``eta``, ``norm_threshold`` r,
    ``momentum`` beta, and the momentum buffer ``m``, f32 like x, read only under ``reads_m`` and written only under ``writes_m``); the definitions
    are ``sampler.guide_reference``'s.  ``workspace``: a device tensor of at least ``guidance_workspace_bytes(...)`` bytes, 8-byte aligned, never
    initialised by the caller (None for "cfg", which launches nothing else)."""
    blend = None if x_orig is None and noise is None and mask is None else (x_orig, noise, mask)
    _step("guided_cfg_step", x, model_out, tokens, n_img, cfg_on, p, reshape_order, sigma, sigma_next, cfg_weight,
          row=(hist, coef, reads_h, writes_h), blend=blend, guide=(mode, rescale, eta, norm_threshold, momentum, reads_m, writes_m, m, workspace))


def slg_cfg_step(x: Tensor, model_out: Tensor, tokens: Tensor, n_img: int, cfg_on: bool, p: int, reshape_order: int, sigma: float,
                 sigma_next: float, cfg_weight: float, hist: Optional[Tensor], coef, reads_h: bool, writes_h: bool, *, slg_scale: float,
                 mode: str = "cfg", workspace: Optional[Tensor] = None, rescale: float = 0.0, eta: float = 0.0, norm_threshold: float = 0.0,
                 momentum: float = 0.0, reads_m: bool = False, writes_m: bool = False, m: Optional[Tensor] = None, x_orig: Optional[Tensor] = None,
                 noise: Optional[Tensor] = None, mask: Optional[Tensor] = None) -> None:
    """dk_slg_cfg_step / _f16 by the dtype of ``model_out``: ``guided_cfg_step`` with skip-layer guidance.  ``model_out`` holds three row groups,
    [3 * n_img, S_i, ld]: the prompt rows, the negative rows and the prompt rows evaluated with blocks skipped (``MMDiTEngine.set_skip_layers``);
    den = G(c, u) + ``slg_scale`` * (c - k), G the mode's combination and k the x0 prediction of the third group (``sampler.slg_reference``).
    ``tokens`` are written in their first 2 * n_img rows only.  ``slg_scale`` 0 gives ``guided_cfg_step``'s bits."""
    if model_out.dim() == 3 and model_out.shape[0] != 3 * n_img:
        raise _lib.DkHipError(f"slg_cfg_step: model_out holds {model_out.shape[0]} rows, expected 3 * n_img = {3 * n_img}")
    if tokens.dim() == 3 and tokens.shape[0] < 2 * n_img:
        raise _lib.DkHipError(f"slg_cfg_step: tokens hold {tokens.shape[0]} rows, expected at least 2 * n_img = {2 * n_img}")
    blend = None if x_orig is None and noise is None and mask is None else (x_orig, noise, mask)
    _step("slg_cfg_step", x, model_out, tokens, n_img, cfg_on, p, reshape_order, sigma, sigma_next, cfg_weight,
          row=(hist, coef, reads_h, writes_h), blend=blend, guide=(mode, rescale, eta, norm_threshold, momentum, reads_m, writes_m, m, workspace),
          slg_scale=slg_scale)


def seed_tensor(seeds, device) -> Tensor:
    """The per-image seeds of the stochastic samplers on the device: Python ints in [0, 2^64) -> int64 [n] holding their 64 bits (the library reads
    them as u64)"""
    seeds = [int(v) for v in seeds]
    if any(not 0 <= v < 1 << 64 for v in seeds):
        raise ValueError(f"seeds must lie in [0, 2^64), got {seeds}")
    import numpy as np
    return torch.from_numpy(np.asarray(seeds, dtype=np.uint64).view(np.int64).copy()).to(device)


def _require_seeds(seeds: Tensor, n_img: int, what: str) -> None:
    _require_cuda(seeds, "seeds")
    if seeds.dtype not in (torch.int64, torch.uint64) or seeds.numel() != n_img:
        raise _lib.DkHipError(f"{what}: seeds must hold one 64-bit integer per image ({n_img}; ``seed_tensor``), got {seeds.dtype} {tuple(seeds.shape)}")


def philox_normal(seeds: Tensor, n_per_img: int, draw: int, stream: int = 0, quad_offset: int = 0) -> Tensor:
    """dk_philox_normal_f32: f32 [n_img, n_per_img], row j = the standard normals of ``seeds[j]`` (``seed_tensor``) for draw ``draw`` of use
    ``stream``, from quad ``quad_offset`` on -- ``sampler.philox_normal_reference`` on the GPU, the noise the stochastic step forms in registers.
    ``n_per_img`` must be a multiple of 4."""
    n_img = int(seeds.numel())
    _require_seeds(seeds, n_img, "philox_normal")
    out = torch.empty(n_img, int(n_per_img), dtype=torch.float32, device=seeds.device)
    _lib.check(_lib.load().dk_philox_normal_f32(out.data_ptr(), seeds.data_ptr(), n_img, int(n_per_img), int(draw), int(stream), int(quad_offset),
                                                _stream()), "dk_philox_normal_f32")
    return out


def noisy_cfg_step(x: Tensor, model_out: Tensor, tokens: Tensor, n_img: int, cfg_on: bool, p: int, reshape_order: int, sigma: float,
                   sigma_next: float, cfg_weight: float, hist: Optional[Tensor], coef, reads_h: bool, writes_h: bool, *, cn: float,
                   seeds: Optional[Tensor], draw: int, guided: bool = False, slg_scale: Optional[float] = None, mode: str = "cfg",
                   workspace: Optional[Tensor] = None, rescale: float = 0.0, eta: float = 0.0, norm_threshold: float = 0.0, momentum: float = 0.0,
                   reads_m: bool = False, writes_m: bool = False, m: Optional[Tensor] = None, x_orig: Optional[Tensor] = None,
                   noise: Optional[Tensor] = None, mask: Optional[Tensor] = None) -> None:
    """dk_noisy_cfg_step / _f16 by the dtype of ``model_out``: the coefficient-row step of a stochastic sampler, x = cx x + cd d + ch hist +
    ``cn`` xi, xi the standard normals of draw ``draw`` of ``seeds[img]`` (``seed_tensor``; ``philox_normal``'s values), formed inside the launch in
    front of the blend.  ``guided``: the guidance group of ``guided_cfg_step`` is read (needs ``cfg_on``); ``slg_scale`` not None: ``slg_cfg_step``'s
    third row group.  Without either the call is ``lms_cfg_step`` (with the mask operands: ``lms_cfg_step_masked``) plus the term.  ``cn`` 0 gives
    the bits of those entries and reads neither ``seeds`` nor ``draw``.  The latent of one image must hold a multiple of 4 elements."""
    if slg_scale is not None:
        if model_out.dim() == 3 and model_out.shape[0] != 3 * n_img:
            raise _lib.DkHipError(f"noisy_cfg_step: model_out holds {model_out.shape[0]} rows, expected 3 * n_img = {3 * n_img}")
        if tokens.dim() == 3 and tokens.shape[0] < 2 * n_img:
            raise _lib.DkHipError(f"noisy_cfg_step: tokens hold {tokens.shape[0]} rows, expected at least 2 * n_img = {2 * n_img}")
    blend = None if x_orig is None and noise is None and mask is None else (x_orig, noise, mask)
    _step("noisy_cfg_step", x, model_out, tokens, n_img, cfg_on, p, reshape_order, sigma, sigma_next, cfg_weight,
          row=(hist, coef, reads_h, writes_h), blend=blend, guide=(mode, rescale, eta, norm_threshold, momentum, reads_m, writes_m, m, workspace),
          slg_scale=0.0 if slg_scale is None else slg_scale, noise_term=(guided, slg_scale is not None, cn, seeds, draw))


def flowedit_step(z: Tensor, x_src: Tensor, model_out: Optional[Tensor], tokens: Tensor, zt_out: Tensor, n_img: int, cfg_on: bool, p: int,
                  reshape_order: int, *, c: float, sigma_in: float, seeds: Tensor, draw: int, w_src: float = 1.0, w_tar: float = 1.0,
                  zs_out: Optional[Tensor] = None, prime: bool = False) -> None:
    """dk_flowedit_step / _f16 by the dtype of ``tokens``: the step of the FlowEdit loop (``sampler.flowedit_reference``).  ``z`` f32 [n_img, Hl, Wl,
    C] takes ``c`` (V_tar - V_src) in place, V the rows of ``model_out`` -- [src | tar], or under ``cfg_on`` [src+ | tar+ | src- | tar-] combined as
    neg + w (pos - neg) with ``w_src`` / ``w_tar`` -- then Zs = (1 - ``sigma_in``) ``x_src`` + ``sigma_in`` xi and Zt = Zs + (z - ``x_src``) are
    written to ``zs_out`` (optional) and ``zt_out`` (f32 like z) and, rounded and patchified, to the same rows of ``tokens``.  xi: the normals of
    ``seeds[img]`` (``seed_tensor``) for draw ``draw`` on stream 1, ``philox_normal(seeds, n, draw, stream=1)``'s values, formed in the launch.
    ``prime``: ``model_out`` is not read (may be None) and ``z`` stays; the launch that forms the first inputs."""
    what = "flowedit_step"
    name = "dk_" + what + ("" if _elem(tokens.dtype, what) == "bf16" else "_f16")
    rows = (4 if cfg_on else 2) * n_img
    _require_cuda(z, "z", torch.float32)
    _require_cuda(tokens, "tokens")
    if z.dim() != 4 or z.shape[0] != n_img:
        raise _lib.DkHipError(f"{what}: z {tuple(z.shape)} must be [n_img = {n_img}, Hl, Wl, C]")
    _, hl, wl, ch = z.shape
    for n, t in (("x_src", x_src), ("zt_out", zt_out), ("zs_out", zs_out)):
        if t is None and n == "zs_out":
            continue
        _require_cuda(t, n, torch.float32)
        if t.shape != z.shape:
            raise _lib.DkHipError(f"{what}: {n} {tuple(t.shape)} must have the latent's shape {tuple(z.shape)}")
    if hl % p or wl % p:
        raise _lib.DkHipError(f"{what}: latent size {(hl, wl)} must be divisible by the patch size {p}")
    s_i, f = (hl // p) * (wl // p), p * p * ch
    if tuple(tokens.shape) != (rows, s_i, f):
        raise _lib.DkHipError(f"{what}: tokens {tuple(tokens.shape)} must be [{rows}, {s_i}, {f}]: {'4' if cfg_on else '2'} * n_img batch rows")
    if model_out is None:
        if not prime:
            raise _lib.DkHipError(f"{what}: model_out is None while the launch reads it (prime = False)")
    else:
        _require_cuda(model_out, "model_out", tokens.dtype)
        if model_out.dim() != 3 or tuple(model_out.shape[:2]) != (rows, s_i) or model_out.shape[2] < f:
            raise _lib.DkHipError(f"{what}: model_out {tuple(model_out.shape)} must be [{rows}, {s_i}, >= {f}]")
    _require_seeds(seeds, n_img, what)
    _lib.check(getattr(_lib.load(), name)(z.data_ptr(), x_src.data_ptr(), _ptr(model_out), f if model_out is None else model_out.shape[-1],
                                          tokens.data_ptr(), _ptr(zs_out), zt_out.data_ptr(), n_img, int(bool(cfg_on)), hl, wl, ch, p, int(reshape_order),
                                          float(w_src), float(w_tar), float(c), float(sigma_in), seeds.data_ptr(), int(draw), int(bool(prime)), _stream()),
               name)


def mask_to_latent(mask: Tensor, factor: int = 8) -> Tensor:
    """dk_mask_to_latent_f32: uint8 [n_mask, H, W] (or [H, W]) -> f32 [n_mask, H / factor, W / factor], box sum / (factor^2 * 255)."""
    _require_cuda(mask, "mask", torch.uint8)
    if mask.dim() not in (2, 3):
        raise ValueError(f"mask must be [H, W] or [n_mask, H, W], got {tuple(mask.shape)}")
    H, W = mask.shape[-2:]
    n = mask.shape[0] if mask.dim() == 3 else 1
    out = torch.empty(n, H // factor, W // factor, dtype=torch.float32, device=mask.device)
    _lib.check(_lib.load().dk_mask_to_latent_f32(mask.data_ptr(), out.data_ptr(), n, H, W, int(factor), _stream()), "dk_mask_to_latent_f32")
    return out


def image_composite(dec: Tensor, orig: Tensor, mask: Tensor) -> Tensor:
    """dk_image_composite_u8: dec uint8 [B, H, W, 3], orig uint8 [H, W, 3] / [1 or B, H, W, 3], mask uint8 [H, W] / [1 or B, H, W] ->
    uint8 [B, H, W, 3]: the decoder's bytes where mask == 255, the original's where mask == 0."""
    for n, t in (("dec", dec), ("orig", orig), ("mask", mask)):
        _require_cuda(t, n, torch.uint8)
    if dec.dim() != 4 or dec.shape[-1] != 3:
        raise ValueError(f"dec must be [B, H, W, 3], got {tuple(dec.shape)}")
    B, H, W, _ = dec.shape
    if tuple(orig.shape[-3:]) != (H, W, 3) or tuple(mask.shape[-2:]) != (H, W):
        raise ValueError(f"orig {tuple(orig.shape)} / mask {tuple(mask.shape)} do not match the image {(H, W, 3)}")
    orig_pi = _mask_per_image(orig.numel(), H * W * 3, B, "image_composite (orig)")
    mask_pi = _mask_per_image(mask.numel(), H * W, B, "image_composite")
    out = torch.empty_like(dec)
    _lib.check(_lib.load().dk_image_composite_u8(dec.data_ptr(), orig.data_ptr(), mask.data_ptr(), out.data_ptr(), B, H, W, orig_pi, mask_pi,
                                                 _stream()), "dk_image_composite_u8")
    return out


def image_mask_out(image: Tensor, mask: Tensor) -> Tensor:
    """dk_image_mask_out_f32: image uint8 [n, H, W, 3], mask uint8 [H, W] / [1 or n, H, W] (255 = repaint) -> f32 [n, H, W, 3] =
    (image / 255 * 2 - 1) * (1 - mask / 255), the bits of that numpy float32 expression: the image FLUX.1 Fill's encoder may look at."""
    _require_cuda(image, "image", torch.uint8)
    _require_cuda(mask, "mask", torch.uint8)
    if image.dim() != 4 or image.shape[-1] != 3:
        raise ValueError(f"image must be [n, H, W, 3], got {tuple(image.shape)}")
    n, H, W, _ = image.shape
    if mask.dim() not in (2, 3) or tuple(mask.shape[-2:]) != (H, W) or (mask.dim() == 3 and mask.shape[0] not in (1, n)):
        raise ValueError(f"mask {tuple(mask.shape)} does not match the images {tuple(image.shape)}: [H, W] or [1 or n, H, W]")
    n_mask = mask.shape[0] if mask.dim() == 3 else 1
    out = torch.empty(n, H, W, 3, dtype=torch.float32, device=image.device)
    _lib.check(_lib.load().dk_image_mask_out_f32(image.data_ptr(), mask.data_ptr(), out.data_ptr(), n, n_mask, H, W, _stream()),
               "dk_image_mask_out_f32")
    return out


def fill_condition_tokens(z: Tensor, mask: Optional[Tensor] = None, patch: int = 2) -> Tensor:
    """dk_fill_condition_tokens: the condition latent z f32 [n, Hl, Wl, C] (+ mask uint8 [8 Hl, 8 Wl] / [1 or n, 8 Hl, 8 Wl]) -> bf16
    [n, S_i, patch^2 C (+ 64 patch^2)]: the latent's patch features in (c, ph, pw) order, then (FLUX.1 Fill) the mask / 255 in its 8 x 8
    pixel-unshuffled, patchified order (include/dk_hip.h).  No mask: FLUX.1 Canny / Depth's layout."""
    _require_cuda(z, "z", torch.float32)
    if z.dim() != 4 or z.shape[1] % patch or z.shape[2] % patch:
        raise ValueError(f"z must be [n, Hl, Wl, C] with sides divisible by the patch size {patch}, got {tuple(z.shape)}")
    n, Hl, Wl, Cc = z.shape
    n_mask = 0
    if mask is not None:
        _require_cuda(mask, "mask", torch.uint8)
        if mask.dim() not in (2, 3) or tuple(mask.shape[-2:]) != (8 * Hl, 8 * Wl) or (mask.dim() == 3 and mask.shape[0] not in (1, n)):
            raise ValueError(f"mask {tuple(mask.shape)} does not match the latent {tuple(z.shape)}: [8 Hl, 8 Wl] or [1 or n, 8 Hl, 8 Wl]")
        n_mask = mask.shape[0] if mask.dim() == 3 else 1
    width = patch * patch * Cc + (64 * patch * patch if mask is not None else 0)
    out = torch.empty(n, (Hl // patch) * (Wl // patch), width, dtype=BF, device=z.device)
    _lib.check(_lib.load().dk_fill_condition_tokens(z.data_ptr(), None if mask is None else mask.data_ptr(), out.data_ptr(), n, n_mask, Hl, Wl,
                                                    Cc, int(patch), _stream()), "dk_fill_condition_tokens")
    return out


def groupnorm(x: Tensor, gamma: Tensor, beta: Tensor, groups: int, eps: float, silu: bool) -> Tensor:
    """x: NHWC [B,H,W,C], bf16 or float16 (gamma / beta in the same type)."""
    lib = _lib.load()
    name = "dk_groupnorm_" + _elem(x.dtype, "groupnorm")
    _require_cuda(x, "x", x.dtype)
    _same_elem(x.dtype, "groupnorm", gamma=gamma, beta=beta)
    B, H, W_, Cc = x.shape
    y = torch.empty_like(x)
    scratch = torch.empty(lib.dk_groupnorm_scratch_floats(B, groups), dtype=torch.float32, device=x.device)
    _lib.check(getattr(lib, name)(x.data_ptr(), y.data_ptr(), B, H * W_, Cc, groups, gamma.data_ptr(), beta.data_ptr(), eps,
                                  int(silu), scratch.data_ptr(), _stream()), name)
    return y


def softmax_rows_(x: Tensor) -> Tensor:
    """In-place row softmax; ``x`` may be a column slice ``buf[:, :cols]`` of a wider row-major buffer, whose remaining
    columns are then written as zeros (row stride a multiple of 8)."""
    lib = _lib.load()
    if not (x.is_cuda and x.dtype in (BF, F16) and x.dim() == 2 and x.stride(1) == 1):
        raise _lib.DkHipError("softmax_rows_: bf16 / float16 GPU matrix with unit column stride expected")
    name = "dk_softmax_rows_" + _elem(x.dtype, "softmax_rows_")
    _lib.check(getattr(lib, name)(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), _stream()), name)
    return x


def transpose(x: Tensor) -> Tensor:
    lib = _lib.load()
    name = "dk_transpose_" + _elem(x.dtype, "transpose")
    _require_cuda(x, "x", x.dtype)
    y = torch.empty(x.shape[1], x.shape[0], dtype=x.dtype, device=x.device)
    _lib.check(getattr(lib, name)(x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], _stream()), name)
    return y


# ---- fp8 path (include/dk_hip.h: dk_gemm_fp8 / dk_quantize_mx8 / dk_ln_modulate_mx8) ----------------------------------
def mx_scale_bytes(rows: int, k: int) -> int:
    return int(_lib.load().dk_mx_scale_bytes(rows, k))


def quantize_mx8(x: Tensor, out: Optional[Tensor] = None, scales: Optional[Tensor] = None, out_row0: int = 0, out_col0: int = 0):
    """bf16 [M, h] -> MX-fp8: (e4m3 bytes uint8 [rows, ldo], scale side array uint8).  Fresh buffers hold exactly the M rows."""
    _require_cuda(x, "x", BF)
    M, h = x.shape
    if out is None:
        out = torch.zeros(M, h, dtype=torch.uint8, device=x.device)
    if scales is None:
        scales = torch.zeros(mx_scale_bytes(out.shape[0], out.shape[1]), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().dk_quantize_mx8(x.data_ptr(), x.stride(0), M, h, out.data_ptr(), out.stride(0), scales.data_ptr(),
                                           out.shape[0], out_row0, out_col0, _stream()), "dk_quantize_mx8")
    return out, scales


def ln_modulate_mx8(x: Tensor, shift: Tensor, scale: Tensor, mod_seg_len: int = 0, eps: float = 1e-6):
    """dk_ln_modulate_bf16 with an MX-fp8 output row: (e4m3 bytes [M, h], scale side array)."""
    for n, t in (("x", x), ("shift", shift), ("scale", scale)):
        _require_cuda(t, n, BF)
    M, h = x.shape
    out = torch.zeros(M, h, dtype=torch.uint8, device=x.device)
    scales = torch.zeros(mx_scale_bytes(M, h), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().dk_ln_modulate_mx8(x.data_ptr(), x.stride(0), M, h, shift.data_ptr(), scale.data_ptr(), shift.stride(0),
                                              mod_seg_len, eps, out.data_ptr(), h, scales.data_ptr(), M, 0, _stream()), "dk_ln_modulate_mx8")
    return out, scales


def gemm_fp8(a8: Tensor, a_scales: Tensor, w8: Tensor, w_scale: Tensor, bias: Optional[Tensor] = None, epilogue: int = DK_EPI_BIAS,
             gate: Optional[Tensor] = None, res: Optional[Tensor] = None, gate_seg_len: int = 0, M: Optional[int] = None,
             k: Optional[int] = None, out_mx8: bool = False, workspace: Optional[Tensor] = None, out: Optional[Tensor] = None,
             out_scales: Optional[Tensor] = None):
    """dk_gemm_fp8 over the first M rows / k columns of an MX-fp8 activation buffer a8 [rows, lda] and an e4m3 weight w8 [N, ldw]; any M >= 1 (the
    last 128-row scale block of a8 may be partial).  Returns bf16 [M, N], or with ``out_mx8`` (e4m3 bytes [M, N], scale side array).  ``workspace``
    (ops.gemm_workspace): lets a launch of at most half a round of tiles with a long reduction be cut along K, as the engines do.  ``out`` (and, with
    ``out_mx8``, ``out_scales`` = a side array of ops.mx_scale_bytes(out rows, out pitch)): an output buffer of at least M rows to write rows
    [0, M) of; the other rows are left alone."""
    lib = _lib.load()
    for n, t, dt in (("a8", a8, torch.uint8), ("a_scales", a_scales, torch.uint8), ("w8", w8, torch.uint8), ("w_scale", w_scale, torch.float32)):
        _require_cuda(t, n, dt)
    M = a8.shape[0] if M is None else M
    K = a8.shape[1] if k is None else k
    N = w8.shape[0]
    d = _lib.dk_gemm_fp8_desc()
    d.A, d.A_scales, d.W, d.w_scale = a8.data_ptr(), a_scales.data_ptr(), w8.data_ptr(), w_scale.data_ptr()
    d.bias, d.gate, d.res = _ptr(bias), _ptr(gate), _ptr(res)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldw = a8.stride(0), w8.stride(0)
    d.a_row0, d.a_rows = 0, a8.shape[0]
    d.ldr = res.stride(0) if res is not None else 0
    d.gate_seg_len = gate_seg_len
    d.gate_stride = gate.stride(0) if gate is not None else 0
    d.epilogue = epilogue
    if workspace is not None:
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel()
    if out is not None:
        _require_cuda(out, "out", torch.uint8 if out_mx8 else BF)
        if out.dim() != 2 or out.shape[0] < M or out.shape[1] < N or out.stride(1) != 1:
            raise ValueError(f"out must be a [>= {M}, >= {N}] matrix with contiguous rows")
    if out_mx8:
        if out is None:
            out = torch.zeros(M, N, dtype=torch.uint8, device=a8.device)
        sc = out_scales
        if sc is None:
            sc = torch.zeros(mx_scale_bytes(out.shape[0], out.stride(0)), dtype=torch.uint8, device=a8.device)
        _require_cuda(sc, "out_scales", torch.uint8)
        if sc.numel() < mx_scale_bytes(out.shape[0], out.stride(0)):
            raise ValueError("out_scales is smaller than ops.mx_scale_bytes(out rows, out pitch)")
        d.C, d.ldc, d.c_mx8, d.C_scales, d.c_rows, d.c_row0, d.c_col0 = out.data_ptr(), out.stride(0), 1, sc.data_ptr(), out.shape[0], 0, 0
        _lib.check(lib.dk_gemm_fp8(C.byref(d), _stream()), "dk_gemm_fp8")
        return out, sc
    if out is None:
        out = torch.empty(M, N, dtype=BF, device=a8.device)
    d.C, d.ldc = out.data_ptr(), out.stride(0)
    _lib.check(lib.dk_gemm_fp8(C.byref(d), _stream()), "dk_gemm_fp8")
    return out
