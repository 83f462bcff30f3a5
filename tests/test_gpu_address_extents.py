"""Extents past 2^31 and 2^32 bytes, and both sides of the address-range guards, on an MI355X ("Address-range guards").

The extents are built from strides, not from work: a few hundred rows are spread over more than 4 GiB of a NaN-filled arena (tests/_bigmem.py)
through leading dimensions and segment strides, only the addressed rows are written, and the arithmetic stays tiny.  Each guard's two edge shapes come
from the guard's own expression (tests/test_address_range_cpu.py sweeps the same edges through the planners):

  * accepted side: the plan names the guarded kernel; the result is right against fp64 at rows whose byte offsets lie in [0, 2^31), in
    [2^31, 2^32) and at the end of the span (tolerance: the parity test of the same kernel, named where it is used); it is BIT-identical to the same
    launch under the same forced kernel on a compact copy of the same rows; and with the addressed rows poisoned again the WHOLE arena holds NaN --
    nothing was written between the rows, beside them or 4 GiB below them;
  * other side: the plan names the kernel with 64-bit addressing and the result is equally right, or the call is refused with its documented text
    and the arena is untouched.

Needs 10.5 GiB of device memory (the arena), held by the module's fixture and freed at its teardown."""
import math

import pytest
import torch

from diffusionkit_amd import _lib
from tests import _bigmem as bm
from tests import _footprint as fp
from tests import _op_launches as L
from tests._util import TOL_SINGLE_OP, max_abs, rel_l2
from tests._address_cases import ATTN_KERNELS, ATTN_TEXT, F8_TEXT, FORCED_TEXT, GEMM_KERNELS, a_rows, attn_edge_ld, edge_rows

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
ARENA = 21 * 2 ** 29  # 10.5 GiB
POISON16 = 0x7FC0  # tests/_footprint.py's NaN as bfloat16: the arena's fill, two bytes at a time


@pytest.fixture(scope="module")
def arena(dev):
    from diffusionkit_amd import ops
    bm.need_free(dev, ARENA)
    ops.zero_page(dev), ops.gemm_workspace(dev), _lib.ensure_attention_workspace(dev)
    a = bm.Arena(dev, ARENA)
    yield a
    a.buf = a.words = a.pair = None
    del a
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def nothing_handed_out(arena):
    arena.live = []
    yield


def poison_again(arena, view):
    """the elements of a strided view of 2-byte elements hold the arena's fill again"""
    assert view.element_size() == 2
    lo = (view.data_ptr() - arena.base) // 2
    torch.as_strided(arena.buf.view(torch.int16), view.shape, view.stride(), lo).fill_(POISON16)


def whole_arena_is_poison(arena, what):
    arena.live = []
    arena.assert_poison(what)


def ranges(offsets, what):
    """the byte offsets reached lie below 2^31, between 2^31 and 2^32, and within 1 MiB of the end of the span"""
    o = torch.as_tensor(offsets, dtype=torch.int64)
    low, high, last = int((o < 2 ** 31).sum()), int(((o >= 2 ** 31) & (o < 2 ** 32)).sum()), int(o.max())
    print(f"[extent] {what}: {low} rows below 2^31, {high} rows in [2^31, 2^32), {int((o >= 2 ** 32).sum())} beyond; largest offset {last} = 2^32 {last - 2 ** 32:+d}")
    return low, high, last


# ---- GEMM: the A span (gemm256v3.hip:713), C and the residual on a wide pitch beyond 2^32 ----------------------------------------------------
M_SEG, N, K, LDA, LDC = 128, 256, 192, 3072, 3072
# A starts 2 GiB into the arena and C behind A's 4 GiB: an offset taken as signed, or one that lost bit 32, still lands inside the arena (a failed
# assertion, not a fault).  C's third segment starts 2 * 349600 * 6144 bytes = 2^32 + 917 504 in: its stores and residual loads go beyond 2^32.
A_LO, C_LO, C_STRIDE = 2 ** 31, 2 ** 31 + 2 ** 32 + 2 ** 20, 349600


def gemm_operands(dt, M):
    rnd = fp.rounder(dt)
    return dict(a=rnd(M, K, seed=901), w=rnd(N, K, seed=902, scale=0.08), b=rnd(N, seed=903, scale=0.1), res=rnd(M, N, seed=904),
                gate=rnd(3, N, seed=905))


def gemm_kw(v, M, a_seg, a_stride, c_seg, c_stride, lda, ldc, ldw=0):
    from diffusionkit_amd import ops
    return dict(A=v["A"], W=v["W"], C=v["C"], bias=v["b"], res=v["C"], gate=v["gate"], M=M, N=N, K=K, lda=lda, ldc=ldc, ldr=ldc, a_seg_len=a_seg,
                a_seg_stride=a_stride, c_seg_len=c_seg, c_seg_stride=c_stride, r_seg_len=c_seg, r_seg_stride=c_stride, gate_seg_len=M_SEG, gate_stride=N,
                alpha=1.0, epilogue=ops.DK_EPI_GATE_RES, ldw=ldw)


def gemm_reference(o):
    a, w, b, res, gate = (o[k].double() for k in ("a", "w", "b", "res", "gate"))
    return res + gate.repeat_interleave(M_SEG, 0)[:a.shape[0]] * (a @ w.t() + b)


def run_gemm_far_rows(dev, arena, dt, knobs, M, a_stride, want_kernel, what, compact_knobs=None):
    """the launch on rows spread by ``a_stride`` (A) and C_STRIDE (C = residual), and on a compact copy; returns nothing, asserts everything"""
    from diffusionkit_amd import ops
    o = gemm_operands(dt, M)
    idx_a, idx_c = fp.row_index(M, M_SEG, a_stride).to(dev), fp.row_index(M, M_SEG, C_STRIDE).to(dev)
    A = arena.strided(A_LO, (a_rows(M, M_SEG, a_stride), K), (LDA, 1), dt)
    C = arena.strided(C_LO, (a_rows(M, M_SEG, C_STRIDE), N), (LDC, 1), dt)
    A[idx_a] = o["a"].to(dev, dt)
    C[idx_c] = o["res"].to(dev, dt)
    small = {k: o[k].to(dev, dt).contiguous() for k in ("w", "b", "gate")}
    v = dict(A=A, C=C, W=small["w"], b=small["b"], gate=small["gate"])
    kw = gemm_kw(v, M, M_SEG, a_stride, M_SEG, C_STRIDE, LDA, LDC)
    with L.tuned(**knobs):
        plan = ops.gemm_plan(kw, dtype=dt)
        assert plan.kernel == want_kernel, f"{what}: planned kernel {plan.kernel}, expected {want_kernel}"
        ops.gemm_desc_call(dtype=dt, **kw)
    got = C[idx_c].clone()
    low, high, last = ranges(idx_a.cpu() * LDA * 2, what + " A rows")
    assert low >= 64 and high >= 64 and 2 ** 32 - 2 ** 20 < last + LDA * 2 <= 2 ** 32 + 4096
    assert ranges(idx_c.cpu() * LDC * 2, what + " C rows")[2] > 2 ** 32
    # the same rows, compact, under the same kernel
    vc = dict(A=o["a"].to(dev, dt).contiguous(), C=o["res"].to(dev, dt).contiguous(), W=small["w"], b=small["b"], gate=small["gate"])
    kc = gemm_kw(vc, M, M, 0, M, 0, K, N)
    with L.tuned(**(compact_knobs or knobs)):
        assert ops.gemm_plan(kc, dtype=dt).kernel == want_kernel
        ops.gemm_desc_call(dtype=dt, **kc)
    assert torch.equal(fp.bits(got), fp.bits(vc["C"])), f"{what}: the far-strided launch differs in its bits from the compact one"
    tol = TOL_SINGLE_OP if dt == BF else L.TOL_F16
    e = rel_l2(gemm_reference(o), got.float())
    print(f"[extent] {what}: kernel {plan.kernel}, tile rows {plan.tile_rows}; vs fp64 rel_l2 {e:.3e} (< {tol:.2e}: test_gemm_v3_ragged_and_straddling_segments)")
    assert e < tol
    torch.as_strided(arena.buf.view(torch.int16), A.shape, A.stride(), A_LO // 2)[idx_a] = POISON16
    torch.as_strided(arena.buf.view(torch.int16), C.shape, C.stride(), C_LO // 2)[idx_c] = POISON16
    whole_arena_is_poison(arena, what)


@pytest.mark.parametrize("kern", GEMM_KERNELS, ids=lambda k: k[0])
def test_gemm_rows_up_to_the_a_span_guard(dev, arena, kern):
    """a_rows * lda * 2 = 2^32 - 4096: three segments of 128 rows, the second one across 2^31 (its row tile is ragged on both sides of the bit), the
    third one ending 4096 bytes below 2^32; C = residual on a pitch of 3072 with its third segment beyond 2^32"""
    name, dt, knobs, kernel, _ = kern
    run_gemm_far_rows(dev, arena, dt, knobs, 384, 349461, kernel, f"gemm {name}, accepted edge")


@pytest.mark.parametrize("kern", GEMM_KERNELS, ids=lambda k: k[0])
def test_gemm_rows_beyond_the_a_span_guard(dev, arena, kern):
    """one row more (a_rows * lda * 2 = 2^32 + 2048): gemm256v4 forced hands over to the 128^2 kernel, which must be equally right with its last rows
    beyond 2^32; gemm256v3 forced is refused with its text and nothing in the arena changes"""
    from diffusionkit_amd import ops
    name, dt, knobs, kernel, _ = kern
    assert a_rows(383, M_SEG, 349462) * LDA * 2 == 2 ** 32 + 2048
    if kernel == 4:
        run_gemm_far_rows(dev, arena, dt, knobs, 383, 349462, 128, f"gemm {name}, beyond the edge", compact_knobs=dict(gemm=128))
        return
    o = gemm_operands(dt, 383)
    small = {k: o[k].to(dev, dt).contiguous() for k in ("w", "b", "gate")}
    v = dict(A=arena.buf[A_LO:], C=arena.buf[C_LO:], W=small["w"], b=small["b"], gate=small["gate"])
    with L.tuned(**knobs), pytest.raises(_lib.DkHipError, match=FORCED_TEXT):
        ops.gemm_desc_call(dtype=dt, **gemm_kw(v, 383, M_SEG, 349462, M_SEG, C_STRIDE, LDA, LDC))
    torch.cuda.synchronize()
    whole_arena_is_poison(arena, f"gemm {name}, refused")
    run_gemm_far_rows(dev, arena, dt, {}, 383, 349462, 128, f"gemm {name}, beyond the edge, automatic route", compact_knobs=dict(gemm=128))


@pytest.mark.parametrize("ldw,kernel", [(2 ** 22 - 8, 4), (2 ** 22, 128)], ids=["accepted", "beyond"])
def test_gemm_v4_weight_pitch_guard(dev, arena, ldw, kernel):
    """gemm256v4.hip:286: 256 rows of W below 2^31 bytes.  W [256, 192] on a pitch of 2^22 - 8 elements (its last row 2.139e9 bytes in) stays on
    gemm256v4; on 2^22 the forced kernel hands over to the 128^2 kernel.  (gemm256v3's and the fp8 GEMM's own W edges need a 64 GiB weight view:
    they are swept on the CPU only.)"""
    from diffusionkit_amd import ops
    M = 384
    o = gemm_operands(BF, M)
    W = arena.strided(A_LO, (N, K), (ldw, 1), BF)
    W.copy_(o["w"].to(dev, BF))
    ranges(torch.arange(N) * ldw * 2, f"gemm v4 W rows, ldw {ldw}")
    outs = {}
    for where, w, pitch in (("far", W, ldw), ("compact", o["w"].to(dev, BF).contiguous(), K)):
        v = dict(A=o["a"].to(dev, BF).contiguous(), C=o["res"].to(dev, BF).contiguous(), W=w, b=o["b"].to(dev, BF), gate=o["gate"].to(dev, BF).contiguous())
        kw = gemm_kw(v, M, M, 0, M, 0, K, N, ldw=pitch)
        with L.tuned(gemm=10 if where == "far" or kernel == 4 else 128):
            assert ops.gemm_plan(kw).kernel == kernel, (where, ops.gemm_plan(kw).kernel)
            ops.gemm_desc_call(**kw)
        outs[where] = v["C"]
    assert torch.equal(fp.bits(outs["far"]), fp.bits(outs["compact"]))
    e = rel_l2(gemm_reference(o), outs["far"].float())
    print(f"[extent] gemm v4 W pitch {ldw}: kernel {kernel}, vs fp64 rel_l2 {e:.3e} (< {TOL_SINGLE_OP}: test_gemm_v4_equals_v3)")
    assert e < TOL_SINGLE_OP
    poison_again(arena, W)
    whole_arena_is_poison(arena, f"gemm v4 W pitch {ldw}")


# ---- attention: one batch row of QKV below 4 GiB (attention.hip:70, attention5.hip:317) --------------------------------------------------------
def wide_ldo(S):
    """the output pitch: the two batch rows of the output fill the 2 GiB in front of Q (a pitch of about 1.4 MB at S = 768)"""
    return (2 ** 31 - 2 ** 20) // (2 * 2 * S) // 8 * 8


def attention_inputs(name, dt, S, D):
    if name == "wave_untracked":
        qkv, rope, bound = L._untracked_inputs(2, 1, S)
        return qkv, dict(rope=rope), bound
    return fp.rounder(dt)(2, S, 3 * D, seed=910), {}, None


ATTN_CASES = ATTN_KERNELS + [("wave_untracked", BF, dict(attn=10, attn_track=0), 128, 768, 10)]


@pytest.mark.parametrize("kern", ATTN_CASES, ids=lambda k: k[0])
def test_attention_batch_row_up_to_the_guard_and_refused_beyond(dev, arena, kern):
    """B = 2, H = 1, ld the largest multiple of 8 with S * ld * 2 < 2^32: the keys of the second half of a batch row lie at offsets with bit 31 set,
    the last key tile 4096 + 2 ld bytes below 2^32, batch row 1 beyond 2^32; the output on a pitch of about a megabyte.  ld + 8 is refused with its text"""
    from diffusionkit_amd import ops
    name, dt, knobs, D, S, kernel = kern
    ld, LDO = attn_edge_ld(S), wide_ldo(S)
    qkv_cpu, extra_cpu, bound = attention_inputs(name, dt, S, D)
    extra = {k: t.to(dev) for k, t in extra_cpu.items()}
    out_lo, q_lo = 0, 2 ** 31  # (Q 2 GiB into the arena, the output in front of it: a key offset taken as signed still lands inside the arena)
    O = arena.strided(out_lo, (2, S, D), (S * LDO, LDO, 1), dt)
    Q = arena.strided(q_lo, (2, S, 3 * D), (S * ld, ld, 1), dt)
    Q.copy_(qkv_cpu.to(dev, dt))
    low, high, last = ranges(torch.arange(S) * ld * 2, f"attention {name} key rows of a batch row")
    assert low > 64 and high > 64 and 2 ** 32 - 2 ** 23 < last < 2 ** 32 and S * ld * 2 > 2 ** 32 - 2 ** 20

    def desc(q, o, pitch, pitch_o):
        kw = dict(q=q.data_ptr(), k=q.data_ptr() + 2 * D, v=q.data_ptr() + 4 * D, out=o, B=2, H=1, S=S, D=D, ld=pitch, ldo=pitch_o, scale=1.0 / math.sqrt(D))
        if bound is not None:
            kw.update(q_rope=extra["rope"], score_bound=bound)
        return kw
    ws = int(_lib.load().dk_attention_workspace_bytes())
    with L.tuned(**knobs):
        plan = ops.attention_plan(dtype=dt, workspace_bytes=ws, **desc(Q, O, ld, LDO))
        assert plan.kernel == kernel and plan.untracked == int(bound is not None) and (plan.split == 2) == ("attn_split" in knobs)
        ops.attention_desc_call(dtype=dt, **desc(Q, O, ld, LDO))
        qc, oc = qkv_cpu.to(dev, dt).contiguous(), torch.empty(2, S, D, dtype=dt, device=dev)
        ops.attention_desc_call(dtype=dt, **desc(qc, oc, 3 * D, D))
    got = O.clone()
    assert torch.equal(fp.bits(got), fp.bits(oc)), f"attention {name}: the far-strided launch differs in its bits from the compact one"
    ref = fp.ref_attention(qkv_cpu.double(), 1, D)
    tol = 6e-3 if dt == BF else 6e-3 / 8
    e, m = rel_l2(ref, got.float()), max_abs(ref, got.float())
    print(f"[extent] attention {name}: kernel {plan.kernel} split {plan.split} untracked {plan.untracked}, ld {ld}; vs fp64 rel_l2 {e:.3e} (< {tol:.2e}), "
          f"max_abs {m:.3e} (< 0.03) [test_attention_kernel_variants]")
    assert e < tol and m < 0.03
    poison_again(arena, Q)
    poison_again(arena, O)
    whole_arena_is_poison(arena, f"attention {name}")
    with L.tuned(**knobs), pytest.raises(_lib.DkHipError, match=ATTN_TEXT):
        ops.attention_desc_call(dtype=dt, **desc(arena.buf[q_lo:], arena.buf[out_lo:], ld + 8, LDO))
    torch.cuda.synchronize()
    whole_arena_is_poison(arena, f"attention {name}, refused")


# ---- conv3x3: the pixel packing b:8 | y:12 | x:12 (gemm256v3.hip:703) --------------------------------------------------------------------------
def conv_windows(x, w, b, y, rows):
    """worst rel_l2 of output rows ``rows`` = [(image, first row, last row + 1)] against the fp64 convolution of the window cropped with its halo"""
    from oracle import vae as ov
    from oracle.mmdit import Prec
    worst = 0.0
    H = x.shape[1]
    for img, r0, r1 in rows:
        a, z = max(r0 - 1, 0), min(r1 + 1, H)
        ref = ov.conv2d_nhwc(x[img:img + 1, a:z].double(), w.double(), b.double(), Prec())[:, r0 - a:r0 - a + (r1 - r0)]
        worst = max(worst, rel_l2(ref, y[img:img + 1, r0:r1].float()))
    return worst


@pytest.mark.parametrize("near,far,rows", [
    ((256, 16, 16), (257, 16, 16), [(0, 0, 16), (127, 0, 16), (255, 0, 16)]),
    ((1, 4096, 16), (1, 4112, 16), [(0, 0, 3), (0, 2047, 2050), (0, 4093, 4096)]),
    ((1, 16, 4096), (1, 16, 4112), [(0, 0, 16)])], ids=["batch_256_257", "rows_4096_4112", "columns_4096_4112"])
def test_conv3x3_pixel_packing_limits(dev, near, far, rows):
    """C = 64, O = 256: B = 256 fills the b:8 field, H = 4096 the y:12 field, W = 4096 the x:12 field -- gemm256v3.hip's conv form; one step beyond
    (B = 257; 4112) the 128^2 kernel takes the launch.  Both against the fp64 convolution of windows (first, middle, last images / rows), at
    test_conv3x3_on_256_tile_kernel's TOL_SINGLE_OP; and the two kernels agree on the shared part as in that test (< 5 % of the elements differ)"""
    from diffusionkit_amd import ops
    C, O = 64, 256
    rnd = fp.rounder(BF)
    w, b = rnd(O, 3, 3, C, seed=921, scale=0.05), rnd(O, seed=922, scale=0.1)
    x = rnd(*far, C, seed=920, scale=1.5, shift=0.3)
    wd, bd = w.to(dev, BF), b.to(dev, BF)
    ys = {}
    for shape, kernel in ((near, 3), (far, 128)):
        B, H, W = shape
        assert ops.conv3x3_plan(B, H, W, C, O).kernel == kernel, shape
        xs = x[:B, :H, :W].contiguous()
        y = ops.conv3x3(xs.to(dev, BF), wd, bd).cpu()
        at = [r for r in rows] + ([(B - 1, 0, min(H, 3))] if B > 1 else [(0, H - 3, H)])
        e = conv_windows(xs, w, b, y, at)
        print(f"[extent] conv3x3 {shape}: kernel {kernel}, worst window vs fp64 rel_l2 {e:.3e} (< {TOL_SINGLE_OP}: test_conv3x3_on_256_tile_kernel)")
        assert e < TOL_SINGLE_OP and bool(torch.isfinite(y.float()).all())
        ys[kernel] = y
    B, H, W = near
    inner = (slice(0, B), slice(0, H - 1), slice(0, W - 1))  # (the last row / column of the smaller image sees its border, the larger one a neighbour)
    differ = float((ys[3][inner].float() != ys[128][inner].float()).float().mean())
    assert differ < 0.05, f"{differ:.3f} of the shared outputs differ between the two kernels"


# ---- row-strided elementwise operators: a row pitch that spreads 2050 rows over more than 2^32 bytes -------------------------------------------
ROWS, PITCH = 2050, 2 ** 20 + 8  # 2049 * (2^20 + 8) * 2 bytes = 2^32 + 2 129 936: the last row starts beyond 2^32, row 1024 beyond 2^31
X_LO = 2 ** 31                   # the far-strided operand starts 2 GiB into the arena, a second one behind it
Y_LO = X_LO + -(-(ROWS * PITCH * 2) // 512) * 512


def far_rows(arena, lo, h, values, dev, dt=BF):
    v = arena.strided(lo, (ROWS, h), (PITCH, 1), dt)
    v.copy_(values.to(dev, dt))
    return v


def stream():
    from diffusionkit_amd.engine import _stream
    return _stream()


def test_row_pitch_beyond_2_32_ln_modulate(dev, arena):
    """dk_ln_modulate_bf16 with ldx = ldo = 2^20 + 8: bit-identical to the compact launch, right against fp64 at test_ln_modulate's 2e-3 in the first
    rows, the rows behind 2^31 and the last rows (beyond 2^32), nothing written between the rows"""
    lib = _lib.load()
    h, rnd = 1536, fp.rounder(BF)
    x, shift, scale = rnd(ROWS, h, seed=960, scale=3.0, shift=0.5), rnd(1, h, seed=961), rnd(1, h, seed=962, scale=0.5)
    sd, cd = shift.to(dev, BF), scale.to(dev, BF)
    X, Y = far_rows(arena, X_LO, h, x, dev), arena.strided(Y_LO, (ROWS, h), (PITCH, 1), BF)
    assert ranges(torch.arange(ROWS) * PITCH * 2, "ln_modulate rows")[2] > 2 ** 32
    xc, yc = x.to(dev, BF).contiguous(), torch.empty(ROWS, h, dtype=BF, device=dev)
    for a, o, ld in ((X, Y, PITCH), (xc, yc, h)):
        _lib.check(lib.dk_ln_modulate_bf16(a.data_ptr(), ld, o.data_ptr(), ld, ROWS, h, sd.data_ptr(), cd.data_ptr(), h, ROWS, ROWS, 0, 1e-6, stream()))
    got = Y.clone()
    assert torch.equal(fp.bits(got), fp.bits(yc))
    ref = L._ref_ln(x.double()[None], shift.double(), scale.double(), BF)[0]
    for rows in (slice(0, 64), slice(1024, 1088), slice(ROWS - 64, ROWS)):
        e = rel_l2(ref[rows], got[rows].float())
        print(f"[extent] ln_modulate rows {rows.start}..{rows.stop}: vs fp64 rel_l2 {e:.3e} (< 2e-3: test_ln_modulate)")
        assert e < 2e-3
    poison_again(arena, X)
    poison_again(arena, Y)
    whole_arena_is_poison(arena, "ln_modulate far rows")


@pytest.mark.parametrize("D", [128, 64])
def test_row_pitch_beyond_2_32_qk_norm_rope(dev, arena, D):
    """dk_qk_norm_rope_bf16 in place on rows of pitch 2^20 + 8 (one sequence of 2050 positions): bit-identical to the compact launch, q and k against
    fp64 at test_qk_norm_rope's 2e-3"""
    lib = _lib.load()
    H, rnd = 2, fp.rounder(BF)
    h = H * D
    qkv, qw, kw = rnd(1, ROWS, 3 * h, seed=963), rnd(D, seed=964, scale=0.1, shift=1.0), rnd(D, seed=965, scale=0.1, shift=1.0)
    pos = torch.arange(ROWS, dtype=torch.float32)[:, None]
    ang = 0.37 * pos / (1.0 + 0.11 * torch.arange(D // 2, dtype=torch.float32)[None, :])
    tab = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).contiguous()
    qd, kd, td = qw.to(dev, BF), kw.to(dev, BF), tab.to(dev)
    X = far_rows(arena, X_LO, 3 * h, qkv[0], dev)
    xc = qkv[0].to(dev, BF).contiguous()
    for a, ld in ((X, PITCH), (xc, 3 * h)):
        _lib.check(lib.dk_qk_norm_rope_bf16(a.data_ptr(), ld, 0, h, ROWS, H, D, qd.data_ptr(), kd.data_ptr(), 1e-6, td.data_ptr(), ROWS, ROWS, 0, stream()))
    got = X.clone()
    assert torch.equal(fp.bits(got), fp.bits(xc))
    ref = fp.ref_qk_norm_rope(qkv.double(), H, D, qw.double(), kw.double(), tab.double())[0]
    for rows in (slice(0, 64), slice(1024, 1088), slice(ROWS - 64, ROWS)):
        e = rel_l2(ref[rows], got[rows].float())
        print(f"[extent] qk_norm_rope D {D} rows {rows.start}..{rows.stop}: vs fp64 rel_l2 {e:.3e} (< 2e-3: test_qk_norm_rope)")
        assert e < 2e-3
    poison_again(arena, X)
    whole_arena_is_poison(arena, "qk_norm_rope far rows")


def test_row_pitch_beyond_2_32_quantize_mx8(dev, arena):
    """dk_quantize_mx8 reading rows of pitch 2^20 + 8: bytes and scales bit-identical to the compact launch (test_quantize_mx8_bit_exact pins those
    against the oracle)"""
    from diffusionkit_amd import ops
    lib = _lib.load()
    h = 384
    x = fp.rounder(BF)(ROWS, h, seed=966, scale=2.0)
    X = far_rows(arena, X_LO, h, x, dev)
    outs = []
    for a, ld in ((X, PITCH), (x.to(dev, BF).contiguous(), h)):
        q = torch.zeros(ROWS, h, dtype=torch.uint8, device=dev)
        sc = torch.zeros(ops.mx_scale_bytes(ROWS, h), dtype=torch.uint8, device=dev)
        _lib.check(lib.dk_quantize_mx8(a.data_ptr(), ld, ROWS, h, q.data_ptr(), h, sc.data_ptr(), ROWS, 0, 0, stream()))
        outs.append((q, sc))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not bool(fp.nan_mask(outs[0][0]).any())
    poison_again(arena, X)
    whole_arena_is_poison(arena, "quantize_mx8 far rows")


@pytest.mark.parametrize("reuse", [0, 1], ids=["difference", "reuse"])
def test_row_pitch_beyond_2_32_block_residual_and_probe(dev, arena, reuse):
    """dk_block_residual_bf16 (r = x - r; reuse: x += r, in place on the far rows) and dk_block_probe_bf16 on x rows of pitch 2^20 + 8, two batch
    rows of 1025 rows: bit-identical to the compact launches; the difference / sum against fp64 within one bf16 rounding (TOL_SINGLE_OP)"""
    lib = _lib.load()
    h, seg = 1536, 1025
    rnd = fp.rounder(BF)
    x, r = rnd(ROWS, h, seed=967), rnd(ROWS, h, seed=968)
    X = far_rows(arena, X_LO, h, x, dev)
    xc = x.to(dev, BF).contiguous()
    res = []
    for a, ld in ((X, PITCH), (xc, h)):
        rd = r.to(dev, BF).contiguous()
        _lib.check(lib.dk_block_residual_bf16(a.data_ptr(), ld, seg, seg, rd.data_ptr(), ROWS, h, reuse, stream()))
        d = r.to(dev, BF).contiguous()
        rows_p, probe = torch.empty(ROWS, 2, device=dev), torch.empty(2, 2, device=dev)
        _lib.check(lib.dk_block_probe_bf16(a.data_ptr(), ld, seg, seg, d.data_ptr(), None, rows_p.data_ptr(), probe.data_ptr(), ROWS, h, seg, stream()))
        res.append((a.clone() if reuse else rd, d, probe))
    for got, want in zip(res[0], res[1]):
        assert torch.equal(fp.bits(got), fp.bits(want))
    ref = (x.double() + r.double()) if reuse else (x.double() - r.double())
    e = rel_l2(ref, res[0][0].float())
    print(f"[extent] block_residual reuse {reuse}: vs fp64 rel_l2 {e:.3e} (< {TOL_SINGLE_OP}: one bf16 rounding, tests/_util.py)")
    assert e < TOL_SINGLE_OP
    poison_again(arena, X)
    whole_arena_is_poison(arena, f"block_residual reuse {reuse} far rows")


# ---- fp8 GEMM: a_rows * lda < 2^32 with 1-byte elements (gemm256f8.hip:528) ---------------------------------------------------------------------
@pytest.mark.parametrize("stride,accepted", [(349440, True), (349568, False)], ids=["accepted", "beyond"])
def test_gemm_fp8_rows_up_to_the_a_span_guard(dev, arena, stride, accepted):
    """MX-fp8 activation bytes on a pitch of 6144 bytes, three segments of 128 rows (a map of several segments needs whole 128-row scale blocks per
    segment, so the segment stride moves in steps of 128 rows): stride 349 440 gives a_rows * lda = 2^32 - 262 144 -- the largest accepted at that
    alignment, its third segment in the LAST row block of the scale side array --, 349 568 gives 2^32 + 1 310 720 and is refused with the launcher's
    text (there is no other fp8 kernel), the arena untouched.  Accepted: bit-identical to the compact launch, test_gemm_fp8_bias's TOL_SINGLE_OP
    against the fp64 product of the decoded operands"""
    import ctypes as C
    from diffusionkit_amd import ops
    from diffusionkit_amd.weights import quantize_weight_e4m3
    from tests import _fp8 as f8
    lib = _lib.load()
    M, Kk, Nn, lda = 384, 384, 256, 6144
    rows = a_rows(M, M_SEG, stride)
    assert (rows * lda < 2 ** 32) == accepted and stride % 128 == 0
    x = fp.rounder(BF)(M, Kk, seed=970)
    x[:, :Kk // 2] *= 4.0
    q, s = ops.quantize_mx8(x.to(dev, BF))
    e = f8.array_to_scales(s, M, Kk)  # [M, K / 32] E8M0 bytes of the compact rows
    qw, wsc = quantize_weight_e4m3(fp.rounder(BF)(Nn, Kk, seed=971, scale=0.02).to(BF))
    w8, wsc = qw.to(dev), wsc.to(dev)
    bias = fp.rounder(BF)(Nn, seed=972, scale=0.5).to(dev, BF)
    idx = fp.row_index(M, M_SEG, stride)
    nblk = f8.n_blk128(rows)
    sa = torch.zeros(ops.mx_scale_bytes(rows, Kk), dtype=torch.uint8)
    r = idx[:, None].expand(M, Kk // 32)
    kb = torch.arange(Kk // 32)[None, :].expand(M, Kk // 32)
    sa[f8.scale_index(r, kb, nblk).reshape(-1)] = e.reshape(-1)
    assert int(idx[-1]) >> 7 == nblk - 2, "the last segment lies in the last row block the side array holds"
    sa = sa.to(dev)
    out = torch.full((M, Nn), fp.SENTINEL, dtype=BF, device=dev)
    d = _lib.dk_gemm_fp8_desc()
    d.A_scales, d.W, d.w_scale, d.C, d.bias = sa.data_ptr(), w8.data_ptr(), wsc.data_ptr(), out.data_ptr(), bias.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldw, d.ldc = M, Nn, Kk, lda, w8.stride(0), Nn
    d.a_seg_len, d.a_seg_stride, d.a_row0, d.a_rows, d.epilogue = M_SEG, stride, 0, rows, ops.DK_EPI_BIAS
    from diffusionkit_amd.engine import _stream
    if not accepted:
        d.A = arena.base + A_LO
        assert lib.dk_gemm_fp8(C.byref(d), _stream()) != 0 and F8_TEXT.encode() in lib.dk_last_error()
        torch.cuda.synchronize()
        assert bool((out == fp.SENTINEL).all())
        whole_arena_is_poison(arena, "gemm_fp8 refused")
        return
    A = arena.strided(A_LO, (rows, Kk), (lda, 1), torch.uint8)
    A[idx.to(dev)] = q
    d.A = A.data_ptr()
    low, high, last = ranges(idx * lda, "gemm_fp8 A rows")
    assert low >= 64 and high >= 64 and 2 ** 32 - 2 ** 20 < last + lda <= 2 ** 32
    _lib.check(lib.dk_gemm_fp8(C.byref(d), _stream()), "dk_gemm_fp8")
    compact = ops.gemm_fp8(q, s, w8, wsc, bias=bias, M=M, k=Kk)
    assert torch.equal(fp.bits(out), fp.bits(compact)), "the far-strided fp8 launch differs in its bits from the compact one"
    ref = f8.mx8_decode(q, e).double() @ (qw.view(torch.float8_e4m3fn).double() * wsc.cpu().double()[:, None]).t() + bias.double().cpu()
    err = rel_l2(ref, out.float())
    print(f"[extent] gemm_fp8 accepted edge: vs fp64 rel_l2 {err:.3e} (< {TOL_SINGLE_OP}: test_gemm_fp8_bias)")
    assert err < TOL_SINGLE_OP
    torch.as_strided(arena.buf.view(torch.int16), (rows, Kk // 2), (lda // 2, 1), A_LO // 2)[idx.to(dev)] = POISON16
    whole_arena_is_poison(arena, "gemm_fp8 far rows")


# ---- the same GEMM edge with REAL rows: every row tile of a 4 GiB A, across bit 31 and up to the edge -------------------------------------------
@pytest.mark.parametrize("kern", GEMM_KERNELS, ids=lambda k: k[0])
def test_gemm_every_row_up_to_the_a_span_guard(dev, arena, kern):
    """M = 699 050 rows of A on a pitch of 3072 (a_rows * lda * 2 = 2^32 - 4096: the largest accepted M), N 256, K 192, bias epilogue: every row tile
    of the launch, the ones across 2^31 and the last, ragged one included.  Bit-identical to the launch on a compact copy of A under the same kernel;
    the first rows, the rows around byte 2^31 and the last rows against fp64 at test_gemm_v3_ragged_and_straddling_segments' tolerance; nothing
    written into A's pitch gaps"""
    from diffusionkit_amd import ops
    name, dt, knobs, kernel, _ = kern
    M = edge_rows(LDA * 2)
    assert M == 699050 and M * LDA * 2 == 2 ** 32 - 4096
    g = torch.Generator(device=dev).manual_seed(980)
    a = torch.randn(M, K, device=dev, generator=g).to(dt)
    rnd = fp.rounder(dt)
    w, b = rnd(N, K, seed=981, scale=0.08).to(dev, dt), rnd(N, seed=982, scale=0.1).to(dev, dt)
    A = arena.strided(A_LO, (M, K), (LDA, 1), dt)
    A.copy_(a)
    outs = []
    for src, lda in ((A, LDA), (a, K)):
        c = torch.full((M, N), fp.SENTINEL, dtype=dt, device=dev)
        kw = dict(A=src, W=w, C=c, bias=b, M=M, N=N, K=K, lda=lda, ldc=N, a_seg_len=M, a_seg_stride=0, c_seg_len=M, c_seg_stride=0, alpha=1.0,
                  epilogue=ops.DK_EPI_BIAS)
        with L.tuned(**knobs):
            plan = ops.gemm_plan(kw, dtype=dt)
            assert plan.kernel == kernel, (plan.kernel, kernel)
            ops.gemm_desc_call(dtype=dt, **kw)
        outs.append(c)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"gemm {name}: the 4 GiB launch differs in its bits from the compact one"
    mid = 2 ** 31 // (LDA * 2)
    tol, worst = (TOL_SINGLE_OP if dt == BF else L.TOL_F16), 0.0
    for rows in (slice(0, 300), slice(mid - 300, mid + 300), slice(M - 300, M)):
        ref = a[rows].double().cpu() @ w.double().cpu().t() + b.double().cpu()
        worst = max(worst, rel_l2(ref, outs[0][rows].float()))
    print(f"[extent] gemm {name}, M {M} real rows: kernel {plan.kernel}, {plan.tiles} tiles of {plan.tile_rows} rows; rows 0.., {mid - 300}.. (byte 2^31), "
          f"{M - 300}..: vs fp64 rel_l2 {worst:.3e} (< {tol:.2e}: test_gemm_v3_ragged_and_straddling_segments)")
    assert worst < tol
    poison_again(arena, A)
    whole_arena_is_poison(arena, f"gemm {name}, every row")


# ---- attention_d512: the entry takes dense q / k / v only (ld == 512); the output pitch is free ----------------------------------------------------
D512_TEXT = "attention_d512: q / k / v rows of exactly 512 columns"


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_attention_d512_output_pitch_beyond_2_32_and_wide_ld_refused(dev, arena, dt):
    """dk_attention_d512_* states its limit on the input side itself: q / k / v rows of exactly 512 columns (its V transpose reads dense matrices), so
    an extent T * ld beyond 2^32 cannot be asked for -- ld = 520 and the ld that would put T * ld * 2 at 2^32 are refused with that text, nothing
    launched, the arena untouched.  The output pitch is free: B = 2, T = 100 on ldo = 2^24 + 8 puts batch row 0's last rows at offsets with bit 31
    set and batch row 1 across 2^32.  Bit-identical to the compact launch; against fp64 at test_attention_d512_flash's 6e-3 / 0.03 (fp16: 7.5e-4,
    test_gpu_vae_f16.py)"""
    from diffusionkit_amd import ops
    from diffusionkit_amd.engine import _stream
    lib = _lib.load()
    B, T, D, ldo = 2, 100, 512, 2 ** 24 + 8
    rnd = fp.rounder(dt)
    q, k, v = (rnd(B, T, D, seed=990 + i).to(dev, dt).contiguous() for i in range(3))
    vt = torch.empty(B * 512 * lib.dk_attention_d512_tp(T), dtype=dt, device=dev)
    fn = getattr(lib, "dk_attention_d512_" + ("bf16" if dt == BF else "f16"))
    for ld in (520, (2 ** 32 - 1) // (2 * T) // 8 * 8 + 8):
        assert fn(arena.base + X_LO, arena.base + X_LO + 1024, arena.base + X_LO + 2048, arena.base, B, T, ld, 512, 1.0 / math.sqrt(D), vt.data_ptr(), _stream()) != 0
        assert D512_TEXT.encode() in lib.dk_last_error(), lib.dk_last_error()
    torch.cuda.synchronize()
    whole_arena_is_poison(arena, "attention_d512 refused")
    O = arena.strided(X_LO, (B, T, D), (T * ldo, ldo, 1), dt)
    low, high, last = ranges(torch.arange(B * T) * ldo * 2, f"attention_d512 output rows, ldo {ldo}")
    assert low > 32 and high > 32 and last > 2 ** 32
    _lib.check(fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), O.data_ptr(), B, T, 512, ldo, 1.0 / math.sqrt(D), vt.data_ptr(), _stream()), "dk_attention_d512")
    got = O.clone()
    compact = ops.attention_d512(q, k, v)
    assert torch.equal(fp.bits(got), fp.bits(compact)), "attention_d512: the wide-pitch output differs in its bits from the compact one"
    ref = fp.ref_attention_d512(q.double().cpu(), k.double().cpu(), v.double().cpu())
    tol = 6e-3 if dt == BF else 6e-3 / 8
    e, m = rel_l2(ref, got.float()), max_abs(ref, got.float())
    print(f"[extent] attention_d512 {dt} ldo {ldo}: vs fp64 rel_l2 {e:.3e} (< {tol:.2e}), max_abs {m:.3e} (< 0.03)")
    assert e < tol and m < 0.03
    poison_again(arena, O)
    whole_arena_is_poison(arena, "attention_d512 wide output pitch")


def test_gemm_fp8_output_and_residual_beyond_2_32(dev, arena):
    """the fp8 GEMM with gate + residual, C = residual on a pitch of 3072 in three segments whose last one starts beyond 2^32 (A compact): bit-identical to
    the compact launch, test_gemm_fp8_gate_res's TOL_SINGLE_OP against the fp64 product of the decoded operands, nothing written between the rows"""
    import ctypes as C
    from diffusionkit_amd import ops
    from diffusionkit_amd.engine import _stream
    from diffusionkit_amd.weights import quantize_weight_e4m3
    from tests import _fp8 as f8
    lib = _lib.load()
    M, Kk = 384, 384
    x = fp.rounder(BF)(M, Kk, seed=973)
    q, s = ops.quantize_mx8(x.to(dev, BF))
    qw, wsc = quantize_weight_e4m3(fp.rounder(BF)(N, Kk, seed=974, scale=0.02).to(BF))
    w8, wsd = qw.to(dev), wsc.to(dev)
    rnd = fp.rounder(BF)
    bias, gate, res = rnd(N, seed=975, scale=0.5), rnd(3, N, seed=976), rnd(M, N, seed=977)
    bd, gd = bias.to(dev, BF), gate.to(dev, BF).contiguous()
    idx = fp.row_index(M, M_SEG, C_STRIDE).to(dev)
    Cv = arena.strided(C_LO, (a_rows(M, M_SEG, C_STRIDE), N), (LDC, 1), BF)
    Cv[idx] = res.to(dev, BF)
    assert ranges(idx.cpu() * LDC * 2, "gemm_fp8 C rows")[2] > 2 ** 32
    d = _lib.dk_gemm_fp8_desc()
    d.A, d.A_scales, d.W, d.w_scale, d.C, d.bias, d.gate, d.res = q.data_ptr(), s.data_ptr(), w8.data_ptr(), wsd.data_ptr(), Cv.data_ptr(), bd.data_ptr(), gd.data_ptr(), Cv.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldw, d.ldc, d.ldr = M, N, Kk, Kk, w8.stride(0), LDC, LDC
    d.a_row0, d.a_rows, d.c_seg_len, d.c_seg_stride, d.r_seg_len, d.r_seg_stride = 0, M, M_SEG, C_STRIDE, M_SEG, C_STRIDE
    d.gate_seg_len, d.gate_stride, d.epilogue = M_SEG, N, ops.DK_EPI_GATE_RES
    _lib.check(lib.dk_gemm_fp8(C.byref(d), _stream()), "dk_gemm_fp8")
    got = Cv[idx].clone()
    rc = res.to(dev, BF).contiguous()
    compact = ops.gemm_fp8(q, s, w8, wsd, bias=bd, epilogue=ops.DK_EPI_GATE_RES, gate=gd, res=rc, gate_seg_len=M_SEG, M=M, k=Kk)
    assert torch.equal(fp.bits(got), fp.bits(compact)), "gemm_fp8: the far-strided output differs in its bits from the compact one"
    acc = f8.mx8_decode(q, f8.array_to_scales(s, M, Kk)).double() @ (qw.view(torch.float8_e4m3fn).double() * wsc.double()[:, None]).t() + bias.double()
    r16 = lambda t: t.to(BF).double()  # (test_gemm_fp8_gate_res states the operator with the projection and the gated term rounded to bf16)
    ref = res.double() + r16(gate.double().repeat_interleave(M_SEG, 0) * r16(acc))
    e = rel_l2(ref, got.float())
    print(f"[extent] gemm_fp8 gate + residual, C beyond 2^32: vs fp64 rel_l2 {e:.3e} (< {TOL_SINGLE_OP}: test_gemm_fp8_gate_res)")
    assert e < TOL_SINGLE_OP
    torch.as_strided(arena.buf.view(torch.int16), Cv.shape, Cv.stride(), C_LO // 2)[idx] = POISON16
    whole_arena_is_poison(arena, "gemm_fp8 far C rows")


def test_gemm_fp8_mx8_output_in_the_last_block_of_its_scale_array(dev):
    """the fp8 GEMM writing an MX-fp8 output (c_mx8) through a row map of three 128-row segments 349 440 rows apart into a buffer of 699 008 rows: the
    third segment's scales land in the LAST row block (5460 of 5462) of the output's scale side array (sc_nblk).  Bytes and scales of the written rows
    equal the compact launch's; every other byte of the output and every other scale byte is untouched (zero)"""
    import ctypes as C
    from diffusionkit_amd import ops
    from diffusionkit_amd.engine import _stream
    from diffusionkit_amd.weights import quantize_weight_e4m3
    from tests import _fp8 as f8
    lib = _lib.load()
    M, Kk, stride = 384, 384, 349440
    rows = a_rows(M, M_SEG, stride)
    x = fp.rounder(BF)(M, Kk, seed=978)
    q, s = ops.quantize_mx8(x.to(dev, BF))
    qw, wsc = quantize_weight_e4m3(fp.rounder(BF)(N, Kk, seed=979, scale=0.02).to(BF))
    w8, wsd = qw.to(dev), wsc.to(dev)
    bd = fp.rounder(BF)(N, seed=983, scale=0.5).to(dev, BF)
    want_q, want_s = ops.gemm_fp8(q, s, w8, wsd, bias=bd, M=M, k=Kk, out_mx8=True)
    want_e = f8.array_to_scales(want_s, M, N)
    out = torch.zeros(rows, N, dtype=torch.uint8, device=dev)
    sc = torch.zeros(ops.mx_scale_bytes(rows, N), dtype=torch.uint8, device=dev)
    d = _lib.dk_gemm_fp8_desc()
    d.A, d.A_scales, d.W, d.w_scale, d.C, d.bias, d.C_scales = q.data_ptr(), s.data_ptr(), w8.data_ptr(), wsd.data_ptr(), out.data_ptr(), bd.data_ptr(), sc.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldw, d.ldc = M, N, Kk, Kk, w8.stride(0), N
    d.a_row0, d.a_rows, d.c_seg_len, d.c_seg_stride, d.c_mx8, d.c_rows, d.c_row0, d.c_col0, d.epilogue = 0, M, M_SEG, stride, 1, rows, 0, 0, ops.DK_EPI_BIAS
    _lib.check(lib.dk_gemm_fp8(C.byref(d), _stream()), "dk_gemm_fp8")
    idx = fp.row_index(M, M_SEG, stride)
    nblk = f8.n_blk128(rows)
    assert int(idx[-1]) >> 7 == nblk - 2
    assert torch.equal(out[idx.to(dev)], want_q), "the MX-fp8 bytes of the mapped rows differ from the compact launch"
    r = idx[:, None].expand(M, N // 32)
    kb = torch.arange(N // 32)[None, :].expand(M, N // 32)
    pos = f8.scale_index(r, kb, nblk).reshape(-1)
    scc = sc.cpu()
    assert torch.equal(scc[pos].reshape(M, N // 32), want_e), "the scales of the mapped rows differ from the compact launch"
    scc[pos] = 0
    assert int(scc.max()) == 0, "scale bytes of rows the launch does not own were written"
    out[idx.to(dev)] = 0
    assert int(out.max()) == 0, "output bytes of rows the launch does not own were written"


# ---- fused convs: the weight pitch (conv256v4.hip:293: ldw * 2 * 256 < 2^31; conv_halo.hip:525: O * ldw * 2 < 2^31) ------------------------------
def conv_gn_call(x, w, ldw, b, y, v4):
    """dk_conv3x3_gn_bf16 of a plain fused conv (no table, no residual) with the weight rows ``ldw`` elements apart (ops.conv3x3_gn takes dense weights)"""
    import ctypes as C
    from diffusionkit_amd.engine import _stream
    lib = _lib.load()
    B, H, W, Cc = x.shape
    d = _lib.dk_conv_gn_desc()
    d.x, d.w, d.bias, d.y = x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr()
    d.gn_silu, d.B, d.H, d.W, d.C, d.O, d.C2 = 0, B, H, W, Cc, y.shape[-1], 0
    d.ldw, d.ldy, d.ldr, d.upsample, d.stats_groups = ldw, y.shape[-1], 0, 0, 0
    with L.tuned(conv_v4=v4):
        _lib.check(lib.dk_conv3x3_gn_bf16(C.byref(d), _stream()), "dk_conv3x3_gn_bf16")


@pytest.mark.parametrize("O,ldw", [(256, 2 ** 22 - 8), (128, 2 ** 22)], ids=["O256_last_accepted_pitch", "O128_first_pitch_beyond_v4"])
def test_fused_conv_weight_pitch_guards(dev, arena, O, ldw):
    """test_conv256v4_equals_conv_halo's two-image 32 x 48 x 128 shape with the K-major weight rows on a wide pitch inside the arena.
    O = 256, ldw = 2^22 - 8: the last pitch conv256v4.hip:293 accepts (its weight offsets reach 2^31 - 4 352) and at the same time the last one
    conv_halo.hip:525 accepts (O * ldw * 2 = 2^31 - 4096): under conv_v4 = 2 (conv256v4 wherever eligible) and under conv_v4 = 0 (conv_halo) the
    launch is bit-identical to the launch of the same knob on the dense weight.  O = 128, ldw = 2^22: the first pitch beyond conv256v4's bound,
    still inside conv_halo's: conv_v4 = 2 hands the launch to conv_halo.hip.  The two kernels add in the same order and give the same bits
    (test_conv256v4_equals_conv_halo), so the hand-over does not show in the values -- tests/test_address_range_cpu.py:
    test_conv256v4_weight_pitch_guard_hands_over_to_conv_halo pins the route; here the values on both sides of the bound are right and equal under
    both knobs.
    Every output against the fp64 convolution at that test's TOL_SINGLE_OP; nothing written between the weight rows"""
    B, H, W, Cc = 2, 32, 48, 128
    rnd = fp.rounder(BF)
    x, w, b = rnd(B, H, W, Cc, seed=80, scale=1.5, shift=0.3), rnd(O, 3, 3, Cc, seed=83, scale=0.05), rnd(O, seed=84, scale=0.1)
    xd, bd, wc = x.to(dev, BF), b.to(dev, BF), w.reshape(O, -1).to(dev, BF).contiguous()
    Wv = arena.strided(A_LO, (O, 9 * Cc), (ldw, 1), BF)
    Wv.copy_(wc)
    last = ranges(torch.arange(O) * ldw * 2, f"fused conv W rows, O {O}, ldw {ldw}")[2]
    assert (ldw * 2 * 256 < 2 ** 31) == (O == 256) and O * ldw * 2 < 2 ** 31 and last + 9 * Cc * 2 < 2 ** 31
    ref = fp.ref_conv(x.double(), w.double(), b.double())
    out = {}
    for v4 in (2, 0):
        for where, wt, pitch in (("far", Wv, ldw), ("dense", wc, 9 * Cc)):
            y = torch.full((B, H, W, O), fp.SENTINEL, dtype=BF, device=dev)
            conv_gn_call(xd, wt, pitch, bd, y, v4)
            out[v4, where] = y
            e = rel_l2(ref, y.float())
            print(f"[extent] fused conv O {O} ldw {pitch} conv_v4={v4}: vs fp64 rel_l2 {e:.3e} (< {TOL_SINGLE_OP}: test_conv256v4_equals_conv_halo)")
            assert e < TOL_SINGLE_OP
        assert torch.equal(fp.bits(out[v4, "far"]), fp.bits(out[v4, "dense"])), f"conv_v4={v4}: the wide-pitch weight gives other bits than the dense one"
    assert torch.equal(fp.bits(out[2, "far"]), fp.bits(out[0, "far"])), "conv256v4.hip and conv_halo.hip differ in their bits on the wide-pitch weight"
    poison_again(arena, Wv)
    whole_arena_is_poison(arena, f"fused conv W pitch, O {O}")
