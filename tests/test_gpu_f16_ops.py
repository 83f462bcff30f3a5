"""Operator-level parity of the float16 element type (MI355X): every *_f16 operator against exact (fp64) arithmetic on the same fp16 operands.

Gates are derived, not tuned.  The project's TOL_SINGLE_OP = 3e-3 is 2.7 x the 1.1e-3 rel-L2 of one bf16 rounding; fp16 has three more mantissa
bits, so TOL_F16 = TOL_SINGLE_OP / 8 = 3.75e-4, and for attention the existing 6e-3 / 8 = 7.5e-4.  One bf16 rounding anywhere (1.1e-3) fails both.
Inputs are drawn with tests/_util.randn and rounded to fp16 once on the host, so both sides see identical values."""
import math

import pytest
import torch

from oracle import mmdit as om
from oracle.mmdit import Prec
from tests import _gates as gates
from tests._util import TOL_SINGLE_OP, max_abs, randn, rel_l2

pytestmark = pytest.mark.gpu


def gated(name, ratio):
    """a per-element / per-row gate of tests/_gates.py (proved on mutants in tests/test_gate_power_cpu.py): worst error / bound, printed, <= 1"""
    print(f"[gate] {name}: {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: worst error at {ratio:.3f} of the bound"

F16 = torch.float16
TOL_F16 = TOL_SINGLE_OP / 8
TOL_ATTN_F16 = 6e-3 / 8
P16 = Prec(F16)
PAD = 8  # sentinel rows behind the last row a launch may write


def f16r(x):
    """values representable in fp16, kept as fp32"""
    return x.to(F16).to(torch.float32)


def rnd(*shape, seed, scale=1.0):
    return f16r(randn(*shape, seed=seed, scale=scale))


def g(x, dev):
    return x.to(dev, F16).contiguous()


def exact_linear(x, w, b=None):
    """fp64 product (exact for fp16 operands up to the fp64 sum), rounded once to fp16: what every epilogue starts from"""
    y = x.double() @ w.double().t()
    if b is not None:
        y = y + b.double()
    return y


def epilogue_ref(ops, epi, y, res=None, gate=None):
    """the reference's op boundaries behind the Linear, on the exact product: (epilogue code, unrounded fp32 result)"""
    acc = f16r(y.float())
    if epi == "bias":
        return ops.DK_EPI_BIAS, y.float()
    if epi == "gelu":
        return ops.DK_EPI_BIAS_GELU, om.gelu_erf(acc, Prec())
    if epi == "silu":
        return ops.DK_EPI_BIAS_SILU, om.silu(acc, Prec())
    if epi == "res":
        return ops.DK_EPI_RES, res + acc
    return ops.DK_EPI_GATE_RES, res + f16r(gate * acc)


def phys_rows(M, seg_len, seg_stride):
    return ((M - 1) // seg_len) * seg_stride + (M - 1) % seg_len + 1


def seg_rows(M, seg_len, seg_stride):
    m = torch.arange(M)
    return (m // seg_len) * seg_stride + m % seg_len


def test_bf16_inputs_are_rejected_by_dtype(dev):
    from diffusionkit_amd import _lib, ops
    with pytest.raises(_lib.DkHipError):
        ops.linear(g(rnd(8, 64, seed=1), dev), rnd(8, 64, seed=2).to(dev, torch.bfloat16))


# ---- 128 x 128 kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", ["bias", "gelu", "silu", "gate_res"])
@pytest.mark.parametrize("M,N,K", [(154, 384, 256), (77, 256, 448)])
def test_gemm128_f16(dev, M, N, K, epi):
    from diffusionkit_amd import ops
    x, w, b = rnd(M, K, seed=10), rnd(N, K, seed=11, scale=0.08), rnd(N, seed=12, scale=0.1)
    res, gate = rnd(M, N, seed=13), rnd(1, N, seed=14)
    code, ref = epilogue_ref(ops, epi, exact_linear(x, w, b), res, gate)
    kw = dict(gate=g(gate, dev), res=g(res, dev), gate_seg_len=M) if epi == "gate_res" else {}
    p = ops.gemm_plan(dict(M=M, N=N, K=K, lda=K, ldc=N, ldr=N, alpha=1.0, epilogue=code, **kw), dtype=F16)
    assert (p.kernel, p.launches) == (128, 1)
    y = ops.linear(g(x, dev), g(w, dev), g(b, dev), epilogue=code, **kw)
    assert y.dtype == F16
    e = rel_l2(ref, y.float())
    print(f"gemm128_f16 {M}x{N}x{K} {epi}: rel_l2 {e:.3e}")
    assert e < TOL_F16
    gated(f"gemm128_f16 {M}x{N}x{K} {epi}", gates.gemm_gate(y.float().cpu(), x, w, b, F16, epi, res, gate))


# ---- gemm256v3: every epilogue, ragged row maps, the half column tile -------------------------------------------------------------------
@pytest.mark.parametrize("epi", ["bias", "gelu", "silu", "gate_res", "res"])
@pytest.mark.parametrize("N", [512, 384])
@pytest.mark.parametrize("M,seg,stride", [(1178, 589, 1613), (1024, 1024, 0)])
def test_gemm256v3_f16(dev, M, seg, stride, N, epi):
    """K = 448: seven K-tiles, a multiple of neither ring depth.  M = 1178: two row segments of 589 inside a stride-1613 stream (tiles straddle the
    segments of A, C, residual and gate: the per-lane row walk); N = 384: the half column tile.  Rows the maps do not reach stay untouched."""
    from diffusionkit_amd import ops
    K = 448
    rows = phys_rows(M, seg, stride) + PAD
    nb = (M + seg - 1) // seg
    A, X = rnd(rows, K, seed=20), rnd(rows, N, seed=21)
    w, b, gate = rnd(N, K, seed=22, scale=0.06), rnd(N, seed=23, scale=0.1), rnd(nb, N, seed=24)
    idx = seg_rows(M, seg, stride)
    code, ref = epilogue_ref(ops, epi, exact_linear(A[idx], w, b), X[idx], gate[torch.arange(M) // seg])
    Xd = g(X, dev)
    kw = dict(A=g(A, dev), W=g(w, dev), C=Xd, bias=g(b, dev), M=M, N=N, K=K, lda=K, ldc=N, a_seg_len=seg, a_seg_stride=stride,
              c_seg_len=seg, c_seg_stride=stride, alpha=1.0, epilogue=code)
    if epi in ("res", "gate_res"):
        kw.update(res=Xd, ldr=N, r_seg_len=seg, r_seg_stride=stride)
    if epi == "gate_res":
        kw.update(gate=g(gate, dev), gate_seg_len=seg, gate_stride=N)
    try:
        ops.tune("gemm", 9)
        p = ops.gemm_plan({k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}, dtype=F16)
        assert (p.kernel, p.launches) == (3, 1)
        ops.gemm_desc_call(dtype=F16, **kw)
    finally:
        ops.tune("gemm", -1)
    got = Xd.float().cpu()
    keep = torch.ones(rows, dtype=torch.bool)
    keep[idx] = False
    assert torch.equal(got[keep], X[keep])  # sentinel: rows >= M and the rows between the segments
    e = rel_l2(ref, got[idx])
    print(f"gemm256v3_f16 M={M} N={N} {epi}: rel_l2 {e:.3e}")
    assert e < TOL_F16
    gated(f"gemm256v3_f16 M={M} N={N} {epi}", gates.gemm_gate(got[idx], A[idx], w, b, F16, epi, X[idx], gate[torch.arange(M) // seg]))


@pytest.mark.parametrize("epi", ["bias", "gate_res"])
def test_gemm256v3_f16_grouped_image_and_text_pair(dev, epi):
    """the grouped two-problem launch: image rows M = 2048 in segments of 1024 and text rows M = 308 in segments of 154 of one joint buffer"""
    from diffusionkit_amd import ops
    B, S_t, S_i, N, K, GAP = 2, 154, 1024, 512, 448, 3
    S = S_t + S_i + GAP
    A, X = rnd(B * S, K, seed=30), rnd(B * S + PAD, N, seed=31)
    Xd, Ad = g(X, dev), g(A, dev)
    want = X.clone()
    calls = []
    gate_args = {}
    for sfx, row0, seg in (("img", S_t, S_i), ("txt", 0, S_t)):
        w, b, gate = rnd(N, K, seed=32 + row0, scale=0.06), rnd(N, seed=33 + row0, scale=0.1), rnd(B, N, seed=34 + row0)
        idx = row0 + seg_rows(B * seg, seg, S)
        code, ref = epilogue_ref(ops, epi, exact_linear(A[idx], w, b), X[idx], gate[torch.arange(B * seg) // seg])
        want[idx] = ref
        wd, bd, gd = g(w, dev), g(b, dev), g(gate, dev)
        d = dict(A=Ad.data_ptr() + 2 * row0 * K, W=wd, C=Xd.data_ptr() + 2 * row0 * N, bias=bd, M=B * seg, N=N, K=K, lda=K, ldc=N,
                 a_seg_len=seg, a_seg_stride=S, c_seg_len=seg, c_seg_stride=S, alpha=1.0, epilogue=code)
        if epi == "gate_res":
            d.update(res=d["C"], ldr=N, r_seg_len=seg, r_seg_stride=S, gate=gd, gate_seg_len=seg, gate_stride=N)
        calls.append((d, idx, (wd, bd, gd)))
        gate_args[sfx] = (idx, w, b, gate[torch.arange(B * seg) // seg])
    p = ops.gemm_plan({k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in calls[0][0].items()},
                      {k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in calls[1][0].items()}, dtype=F16)
    assert (p.kernel, p.launches) == (3, 1)  # one grouped launch
    ops.gemm_fused_call(calls[0][0], None, calls[1][0], None, dtype=F16)
    got = Xd.float().cpu()
    touched = torch.zeros(B * S + PAD, dtype=torch.bool)
    for _, idx, _ in calls:
        touched[idx] = True
        e = rel_l2(want[idx], got[idx])
        print(f"gemm256v3_f16 pair {epi} M={len(idx)}: rel_l2 {e:.3e}")
        assert e < TOL_F16
    for sfx, (idx, w, b, gate) in gate_args.items():
        gated(f"gemm256v3_f16 pair {epi} {sfx}", gates.gemm_gate(got[idx], A[idx], w, b, F16, epi, X[idx], gate))
    assert torch.equal(got[~touched], X[~touched])


def test_gemm256v3_f16_fused_key_qknorm_tail(dev):
    """QKNorm (+ RoPE) of the key columns inside the projection's tail at D = 64, against the plain projection followed by the separate
    dk_qk_norm_rope_f16 pass; query and value columns are the plain projection's bit for bit."""
    from diffusionkit_amd import ops
    B, S, H, D, K = 2, 589, 4, 64, 448
    h, M = H * D, 2 * 589
    x, w, b = rnd(M, K, seed=40), rnd(3 * h, K, seed=41, scale=0.06), rnd(3 * h, seed=42, scale=0.1)
    kw_ = f16r(1 + randn(D, seed=43, scale=0.1))
    tab = ops.rope_table(5, 8, 73, (16, 24, 24), 10000.0, dev)  # [589, 32, 2] fp32
    xd, wd, bd, kd = g(x, dev), g(w, dev), g(b, dev), g(kw_, dev)
    out = {}
    for fused in (True, False):
        C = torch.zeros(M + PAD, 3 * h, dtype=F16, device=dev)
        d = dict(A=xd, W=wd, C=C, bias=bd, M=M, N=3 * h, K=K, lda=K, ldc=3 * h, c_seg_len=S, c_seg_stride=S, alpha=1.0, epilogue=ops.DK_EPI_BIAS)
        side = dict(kn_w=kd, kn_rope=tab, kn_col0=h, kn_col1=2 * h, kn_D=D, kn_pos_off=0, kn_seg_len=S, kn_eps=1e-6) if fused else None
        ops.gemm_fused_call(d, side, dtype=F16)
        out[fused] = C
    plain = out[False].clone()
    sep = out[False][:M].reshape(B, S, 3 * h)
    ops.qk_norm_rope_(sep, H, D, None, kd, tab)  # (the pass rotates the queries too: only its key columns are compared)
    fused = out[True].float().cpu()
    assert torch.equal(fused[M:], torch.zeros(PAD, 3 * h))
    assert torch.equal(fused[:M, :h], plain[:M, :h].float().cpu()) and torch.equal(fused[:M, 2 * h:], plain[:M, 2 * h:].float().cpu())
    e = rel_l2(sep.reshape(M, 3 * h)[:, h:2 * h].float(), fused[:M, h:2 * h])
    k_ref = om.rope_apply(om.rms_norm(f16r(exact_linear(x, w, b).float())[:, h:2 * h].reshape(B, S, H, D).transpose(1, 2), kw_, 1e-6, P16),
                          tab.float().cpu(), Prec()).transpose(1, 2).reshape(M, h)
    e2 = rel_l2(k_ref, fused[:M, h:2 * h])
    print(f"fused key QKNorm f16: vs separate pass {e:.3e}, vs exact {e2:.3e}")
    assert e < TOL_F16 and e2 < TOL_F16
    assert not torch.equal(fused[:M, h:2 * h], plain[:M, h:2 * h].float().cpu())


def test_gemm256v3_f16_k_split(dev):
    """(1024, 512, 6144): eight tiles of 96 K-tiles -- with the split workspace every tile is cut along K (fp32 accumulator exchange), without it
    none is.  Both within TOL_F16 of the exact product; they differ in some bits (summation order); the flag region is zero afterwards."""
    from diffusionkit_amd import ops
    M, N, K = 1024, 512, 6144
    x, w, b = rnd(M, K, seed=50), rnd(N, K, seed=51, scale=0.02), rnd(N, seed=52, scale=0.1)
    ref = exact_linear(x, w, b)
    ws = ops.gemm_workspace(dev)
    d = dict(M=M, N=N, K=K, lda=K, ldc=N, ldr=N, alpha=1.0, epilogue=0)
    p_ws = ops.gemm_plan(dict(d, workspace=ws.data_ptr(), workspace_bytes=ws.numel()), dtype=F16)
    p_no = ops.gemm_plan(d, dtype=F16)
    assert p_ws.kernel == 3 and p_ws.split_tiles == p_ws.tiles and p_ws.k_pieces >= 2 and p_no.kernel == 3 and p_no.split_tiles == 0
    y_ws = ops.linear(g(x, dev), g(w, dev), g(b, dev), workspace=ws)
    y_no = ops.linear(g(x, dev), g(w, dev), g(b, dev))
    e_ws, e_no = rel_l2(ref, y_ws.float()), rel_l2(ref, y_no.float())
    ndiff = int((y_ws != y_no).sum())
    print(f"k split f16: split {e_ws:.3e}, whole {e_no:.3e}, {ndiff} of {M * N} elements differ")
    assert e_ws < TOL_F16 and e_no < TOL_F16
    gated("k split f16, split and whole", gates.gemm_gate([y_ws.float().cpu(), y_no.float().cpu()], x, w, b, F16, rows=gates.row_subset(M, N, K)))
    assert 0 < ndiff < 0.02 * M * N
    assert int(ws[-4096:].sum()) == 0


@pytest.mark.parametrize("mode", [-1, 9])
def test_gemm_f16_overflow_gives_inf(dev, mode):
    """an fp32 -> fp16 store that overflows gives +-inf exactly where the exact result rounds to it (the reference's cast); nothing is clamped"""
    from diffusionkit_amd import ops
    M, N, K = 64, 256, 256
    x, w = rnd(M, K, seed=60, scale=64.0), rnd(N, K, seed=61, scale=64.0)
    exact = exact_linear(x, w)
    want = exact.to(F16)
    assert 0.05 < float(want.isinf().float().mean()) < 0.95
    try:
        ops.tune("gemm", mode)
        y = ops.linear(g(x, dev), g(w, dev)).cpu()
    finally:
        ops.tune("gemm", -1)
    assert not bool(y.isnan().any())
    assert torch.equal(y.isinf(), want.isinf()) and torch.equal(torch.sign(y[y.isinf()]), torch.sign(want[want.isinf()]))
    fin = ~want.isinf()
    assert rel_l2(exact[fin], y.float()[fin]) < TOL_F16


@pytest.mark.parametrize("M,N,K,mode", [(154, 384, 256, -1), (1024, 512, 448, 9)])
def test_gemm_f16_subnormal_weights(dev, M, N, K, mode):
    """weights partly below 2^-14 (fp16 subnormals): finite, and within TOL_F16 of the exact product of the operands as stored.  Prints whether the
    MFMA kept or flushed the subnormal operands (distance to both exact variants)."""
    from diffusionkit_amd import ops
    x, w = rnd(M, K, seed=70, scale=64.0), rnd(N, K, seed=71, scale=2.0 ** -14)
    sub = w.abs() < 2.0 ** -14
    assert 0.3 < float(sub.float().mean()) < 0.9 and bool((w[sub] != 0).any())
    kept, flushed = exact_linear(x, w), exact_linear(x, torch.where(sub, torch.zeros_like(w), w))
    try:
        ops.tune("gemm", mode)
        y = ops.linear(g(x, dev), g(w, dev)).float()
    finally:
        ops.tune("gemm", -1)
    e_kept, e_flushed = rel_l2(kept, y), rel_l2(flushed, y)
    print(f"subnormal fp16 operands, kernel {'128^2 (32x32x16 MFMA)' if mode < 0 else 'gemm256v3 (16x16x32 MFMA)'}: "
          f"rel_l2 to kept {e_kept:.3e}, to flushed {e_flushed:.3e} -> {'kept' if e_kept < e_flushed else 'flushed'}")
    assert bool(torch.isfinite(y).all())
    assert e_kept < TOL_F16


# ---- attention, D = 64 --------------------------------------------------------------------------------------------------------------
def attn_f16(ops, qkv_dev, B, H, S, D, **kw):
    h = H * D
    out = torch.empty(B, S, h, dtype=F16, device=qkv_dev.device)
    base = qkv_dev.data_ptr()
    ops.attention_desc_call(dtype=F16, q=base, k=base + 2 * h, v=base + 4 * h, out=out, B=B, H=H, S=S, D=D, ld=3 * h, ldo=h,
                            scale=1.0 / math.sqrt(D), **kw)
    return out


def attn_ref(q, k, v, B, H, S, D):
    q, k, v = (t.double().reshape(B, S, H, D).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(q @ k.transpose(2, 3) / math.sqrt(D), dim=-1)
    return (p @ v).transpose(1, 2).reshape(B, S, H * D), p


def test_attention_f16_ragged(dev):
    from diffusionkit_amd import ops
    B, H, S, D = 2, 3, 333, 64  # ragged last query block and last key tile
    h = H * D
    qkv = rnd(B, S, 3 * h, seed=80)
    ref, _ = attn_ref(qkv[..., :h], qkv[..., h:2 * h], qkv[..., 2 * h:], B, H, S, D)
    try:
        ops.tune("attn", 9)  # (names a bf16-only kernel: no effect on an fp16 launch)
        y = attn_f16(ops, g(qkv, dev), B, H, S, D)
    finally:
        ops.tune("attn", -1)
    e = rel_l2(ref, y.float())
    print(f"attention_f16 (2, 3, 333): rel_l2 {e:.3e}")
    assert e < TOL_ATTN_F16
    gated("attention_f16 (2, 3, 333)", gates.attn_gate(y, qkv, H, D, F16))


def test_attention_f16_query_qknorm_in_the_q_load(dev):
    from diffusionkit_amd import ops
    B, H, S, D, split = 1, 6, 200, 64, 77
    h = H * D
    qkv = rnd(B, S, 3 * h, seed=81)
    wa, wb = f16r(1 + randn(D, seed=82, scale=0.1)), f16r(1 + randn(D, seed=83, scale=0.1))
    q = qkv[..., :h].reshape(B, S, H, D)
    qn = torch.cat([om.rms_norm(q[:, :split], wa, 1e-6, P16), om.rms_norm(q[:, split:], wb, 1e-6, P16)], dim=1).reshape(B, S, h)
    ref, _ = attn_ref(qn, qkv[..., h:2 * h], qkv[..., 2 * h:], B, H, S, D)
    y = attn_f16(ops, g(qkv, dev), B, H, S, D, qn_a=g(wa, dev), qn_b=g(wb, dev), qn_split=split, qn_eps=1e-6)
    e = rel_l2(ref, y.float())
    print(f"attention_f16 (1, 6, 200) fused query norm: rel_l2 {e:.3e}")
    assert e < TOL_ATTN_F16
    gated("attention_f16 (1, 6, 200) fused query norm", gates.attn_gate(y, torch.cat([qn, qkv[..., h:]], dim=-1), H, D, F16))


def test_attention_f16_spiked_key_forces_rescale(dev):
    """a key that dominates late in the sequence forces the deferred rescale (P up to e^4 before it: far inside fp16's range); fp64 softmax"""
    from diffusionkit_amd import ops
    B, H, S, D = 1, 2, 400, 64
    h = H * D
    qkv = rnd(B, S, 3 * h, seed=33, scale=0.5)
    qkv[0, 330, h:h + D] = f16r(qkv[0, 9, :D] * 8.0)  # head 0: key 330 aligned with query 9
    ref, p = attn_ref(qkv[..., :h], qkv[..., h:2 * h], qkv[..., 2 * h:], B, H, S, D)
    assert float(p[0, 0, 9, 330]) > 0.9
    y = attn_f16(ops, g(qkv, dev), B, H, S, D)
    e = rel_l2(ref, y.float())
    print(f"attention_f16 spiked key: rel_l2 {e:.3e}")
    assert e < TOL_ATTN_F16
    gated("attention_f16 spiked key", gates.attn_gate(y, qkv, H, D, F16))


# ---- elementwise ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1536, 2432])
def test_ln_modulate_f16(dev, h):
    from diffusionkit_amd import ops
    B, S = 2, 77
    x, shift, scale = rnd(B, S, h, seed=90, scale=3.0) + 0.5, rnd(B, h, seed=91), rnd(B, h, seed=92, scale=0.5)
    x = f16r(x)
    y = ops.ln_modulate(g(x, dev), g(shift, dev), g(scale, dev))
    ref = om.layer_norm(x.double(), 1e-6) * P16.r(1.0 + scale[:, None]).double() + shift[:, None].double()
    e = rel_l2(ref, y.float())
    print(f"ln_modulate_f16 h={h}: rel_l2 {e:.3e}")
    assert y.dtype == F16 and e < TOL_F16
    gated(f"ln_modulate_f16 h={h}", gates.ln_gate(y, x, shift, scale, F16))


def test_ln_modulate_f16_large_mean_rows(dev):
    """h = 2432 = 38 x 64 at mean / sigma 16 (tests/_gates.LN_CASES): rows on which a channel left out of the mean shows; the per-row gate alone"""
    from diffusionkit_amd import ops
    case = next(c for c in gates.LN_CASES if c[0] == F16 and len(c) > 5)
    x, shift, scale = gates.ln_operands(case)
    y = ops.ln_modulate(g(x, dev), g(shift, dev), g(scale, dev))
    gated(f"ln_modulate_f16 {case[1:4]} large mean", gates.ln_gate(y, x, shift, scale, F16))


def test_qk_norm_rope_f16(dev):
    from diffusionkit_amd import ops
    B, H, D, S_t, gh, gw = 2, 3, 64, 5, 4, 6
    S, h = S_t + gh * gw, H * D
    qkv = rnd(B, S, 3 * h, seed=93)
    qw, kw = f16r(1 + randn(D, seed=94, scale=0.1)), f16r(1 + randn(D, seed=95, scale=0.1))
    tab = ops.rope_table(S_t, gh, gw, (16, 24, 24), 10000.0, dev)
    d = g(qkv, dev)
    ops.qk_norm_rope_(d, H, D, g(qw, dev), g(kw, dev), tab)
    q, k = (qkv[..., i * h:(i + 1) * h].reshape(B, S, H, D).transpose(1, 2) for i in range(2))
    q, k = (om.rope_apply(om.rms_norm(t, w_, 1e-6, P16), tab.float().cpu(), Prec()) for t, w_ in ((q, qw), (k, kw)))
    ref = torch.cat([t.transpose(1, 2).reshape(B, S, h) for t in (q, k)], dim=-1)
    got = d.float().cpu()
    assert torch.equal(got[..., 2 * h:], qkv[..., 2 * h:])  # v untouched
    e = rel_l2(ref, got[..., :2 * h])
    print(f"qk_norm_rope_f16: rel_l2 {e:.3e}")
    assert e < TOL_F16
    gated("qk_norm_rope_f16", gates.qk_gate(got[..., :2 * h], qkv, qw, kw, tab, D, F16))


def test_timestep_embedding_f16_out(dev):
    """evaluated in fp16 (SD3's config.dtype) AND stored as fp16: the stored value is the evaluated one -- no second rounding"""
    from diffusionkit_amd import ops
    from diffusionkit_amd.config import SD3_2b
    t = torch.tensor([1000.0, 752.0, 500.0, 250.0, 8.9296875, 0.0])
    y = ops.timestep_embedding(t.to(dev), 256, 10000.0, 1, dtype=F16)
    ybf = ops.timestep_embedding(t.to(dev), 256, 10000.0, 1)
    ref = om.timestep_embedding(t, SD3_2b, P16)
    assert y.dtype == F16 and torch.equal(f16r(ref), ref)
    diff = (ref - y.float().cpu()).abs()
    # device and host libm may differ by 1 ulp of the fp16 output (<= 2^-10 at |v| <= 1) in a few entries
    assert float(diff.max()) <= 2.0 ** -10 + 1e-9
    assert float((diff > 0).float().mean()) < 0.05
    assert torch.equal(ybf.float(), y.float().to(torch.bfloat16).float())  # the bf16 entry stores the same evaluation, rounded once more
    assert float((ybf.float() != y.float()).float().mean()) > 0.5


def test_patchify_and_euler_step_f16(dev):
    """dk_latent_to_tokens_f16 + dk_euler_cfg_step_f16 at latent 8 x 12, B = 2, CFG 5: fp16 model output in, fp32 latent kept, fp16 tokens out"""
    from diffusionkit_amd import _lib, ops
    from diffusionkit_amd.config import tiny_sd3
    from diffusionkit_amd.engine import _stream
    from oracle.mmdit import OracleMMDiT
    cfg, lib = tiny_sd3(), _lib.load()
    n_img, Hl, Wl, C, p = 2, 8, 12, 16, 2
    x = torch.randn(n_img, Hl, Wl, C, generator=torch.Generator().manual_seed(80))
    S_i, F = (Hl // p) * (Wl // p), p * p * C
    xd = x.to(dev).contiguous()
    tok = torch.empty(n_img * 2, S_i, F, dtype=F16, device=dev)
    _lib.check(lib.dk_latent_to_tokens_f16(xd.data_ptr(), tok.data_ptr(), n_img, 2, Hl, Wl, C, p, 0, _stream()))
    orc = OracleMMDiT(cfg, {"x_embedder.proj.weight": torch.eye(F).reshape(F, p, p, C), "x_embedder.proj.bias": torch.zeros(F)}, Prec())
    assert torch.equal(tok.float().cpu()[:n_img], orc._patch_embed(f16r(x))) and torch.equal(tok[:n_img], tok[n_img:])
    assert not torch.equal(tok.float().cpu()[:n_img], orc._patch_embed(x.to(torch.bfloat16).float()))  # (not the bf16 rounding)
    out = rnd(n_img * 2, S_i, F, seed=81)
    sigma, sigma_next, w = 0.75, 0.5, 5.0
    ops.euler_cfg_step(xd, g(out, dev), tok, n_img, True, p, 0, sigma, sigma_next, w)
    xb = f16r(x)
    o = orc._unpatch(out, Hl, Wl)
    den, den_neg = xb - o[:n_img] * sigma, xb - o[n_img:] * sigma
    den = den_neg + w * (den - den_neg)
    ref = x + (x - den) / sigma * (sigma_next - sigma)
    assert max_abs(ref, xd) < 1e-5
    assert torch.equal(tok.float().cpu()[:n_img], orc._patch_embed(f16r(xd.cpu()))) and torch.equal(tok[:n_img], tok[n_img:])
