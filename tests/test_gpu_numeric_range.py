"""Numerical-range tests of the HIP kernels (MI355X): inputs chosen where kernels go wrong -- every finite 16-bit value through the pointwise
functions, rows with massive channels through LayerNorm and the GEMMs, long sums at a large mean through the GroupNorm statistics -- against
fp64 references, with the per-element gates of tests/_numeric_range.py (derived there, proved on the host by tests/test_numeric_range_cpu.py).
No bound here comes from the kernel under test.  Every test prints its worst error beside its bound."""
import pytest
import torch

from oracle import fp8 as o8
from tests import _fp8 as f8
from tests import _numeric_range as nr
from tests._util import TOL_SINGLE_OP

pytestmark = pytest.mark.gpu

BF, F16 = nr.BF, nr.F16
DT_IDS = {BF: "bf16", F16: "f16"}
PLAN_KERNEL = {128: 128, 9: 3, 10: 4}  # dk_tune_set("gemm", mode) -> dk_gemm_plan_t.kernel
GEMM_CASES = [(BF, 128), (BF, 9), (BF, 10), (F16, 128), (F16, 9)]
GEMM_IDS = [f"{DT_IDS[dt]}-gemm{m}" for dt, m in GEMM_CASES]


def g(x, dev, dt):
    return x.to(dev, dt).contiguous()


def _epi(ops, fn):
    return ops.DK_EPI_BIAS_GELU if fn == "gelu" else ops.DK_EPI_BIAS_SILU


def _forced_linear(ops, mode, dt, a, w, b, epilogue, dev, split=False):
    """ops.linear under dk_tune_set("gemm", mode), after dk_gemm_plan has confirmed that the named kernel takes the launch (a GELU / SiLU launch
    the planner routes elsewhere is skipped with that reason; a plain one fails)"""
    M, K = a.shape
    N = w.shape[0]
    ws = ops.gemm_workspace(dev) if split else None
    try:
        ops.tune("gemm", mode)
        if split:
            ops.tune("gemm_split", 1)
        d = dict(M=M, N=N, K=K, lda=K, ldc=N, ldr=N, alpha=1.0, epilogue=epilogue)
        if split:
            d.update(workspace=ws.data_ptr(), workspace_bytes=ws.numel())
        p = ops.gemm_plan(d, dtype=dt)
        if epilogue == ops.DK_EPI_BIAS:  # (a plain launch at a shape the kernel is named for: a planner that goes elsewhere is a failure)
            assert p.kernel == PLAN_KERNEL[mode], (mode, p.kernel)
        if p.kernel != PLAN_KERNEL[mode]:  # (host-side, before anything is launched: the kernel lacks the epilogue)
            pytest.skip(f"dk_tune_set('gemm', {mode}) does not put this launch (epilogue {epilogue}, {dt}) on kernel {PLAN_KERNEL[mode]}: the planner names {p.kernel}")
        if split:
            assert p.split_tiles > 0 and p.k_pieces >= 2, (p.split_tiles, p.k_pieces)
        return ops.linear(g(a, dev, dt), g(w, dev, dt), g(b, dev, dt), epilogue=epilogue, workspace=ws).cpu()
    finally:
        ops.tune("gemm", -1)
        ops.tune("gemm_split", -1)


# ---- A. pointwise functions over every finite 16-bit value --------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [0.0, nr.BIAS_ULP], ids=["bias0", "bias2^-7"])
@pytest.mark.parametrize("fn", ["gelu", "silu"])
@pytest.mark.parametrize("dt,mode", GEMM_CASES, ids=GEMM_IDS)
def test_gemm_tail_over_the_whole_domain(dev, dt, mode, fn, bias):
    """A = every finite value of the element type as a 256 x 256 matrix, W = I: each accumulator is exactly one input, so the only inexact step
    between input and output is the tail's function (and, in the second pass, the shared rounding of acc + 2^-7)"""
    from diffusionkit_amd import ops
    x = nr.domain(dt)
    y = _forced_linear(ops, mode, dt, x, torch.eye(256), torch.full((256,), bias), _epi(ops, fn), dev)
    bad, w = nr.pointwise_check(fn, nr.preact(x, dt, bias), y, dt)
    print(f"[range] {fn} tail, gemm {mode} {DT_IDS[dt]}, bias {bias}: worst error / bound {w:.3f} (bound sp(ref) + {nr.C_POINTWISE[fn]:.1e} |x| + {nr.FLOOR[dt]:g})")
    assert not bad, bad


@pytest.mark.parametrize("fn", ["gelu", "silu"])
def test_fp8_gemm_tail_over_the_e4m3_grid(dev, fn):
    """gemm256f8.hip: A = the e4m3 value grid under MX block scales 2^-9 .. 2^2 (pre-activations from 2^-18 to 1792, [-16, 16] at its finest),
    W = the e4m3 identity of scale 1: the accumulators are the grid values exactly"""
    from diffusionkit_amd import ops
    q, e, vals = nr.fp8_grid()
    w8 = torch.eye(256).to(torch.float8_e4m3fn).view(torch.uint8)
    y = ops.gemm_fp8(q.to(dev), f8.scales_to_array(e, 256).to(dev), w8.to(dev), torch.ones(256, device=dev), bias=torch.zeros(256, dtype=BF, device=dev),
                     epilogue=_epi(ops, fn))
    bad, w = nr.pointwise_check(fn, vals, y.cpu(), BF)
    print(f"[range] {fn} tail, fp8 gemm: worst error / bound {w:.3f}")
    assert not bad, bad


@pytest.mark.parametrize("kernel,mode,dt,C,O", [("conv_halo", 0, BF, 64, 128), ("conv_halo", 0, F16, 64, 128), ("conv256v4", 2, BF, 128, 256)],
                         ids=["halo-bf16", "halo-f16", "v4-bf16"])
def test_conv_load_path_silu_over_the_whole_domain(dev, kernel, mode, dt, C, O):
    """norm -> silu -> conv with a hand-built table (scale 1, shift 0) and the identity on the centre tap: the input passes the GroupNorm-apply
    unchanged, SiLU and its rounding happen on the way into LDS, and the conv copies channel o of the result to output o (zeros elsewhere)"""
    from diffusionkit_amd import ops
    d = nr.domain(dt).reshape(1, 32, 32, 64)
    x = torch.cat([d] * (C // 64), dim=-1)
    tab = torch.cat([torch.ones(1, 1, C), torch.zeros(1, 1, C)], dim=1)
    w = torch.zeros(O, 3, 3, C)
    w[torch.arange(C), 1, 1, torch.arange(C)] = 1.0
    try:
        ops.tune("conv_v4", mode)
        y = ops.conv3x3_gn(g(x, dev, dt), g(w, dev, dt).reshape(O, -1), torch.zeros(O, dtype=dt, device=dev), gn_table=tab.to(dev), silu=True).cpu()
    finally:
        ops.tune("conv_v4", 1)
    assert bool((y[..., C:] == 0).all())
    bad, wr = nr.pointwise_check("silu", x, y[..., :C], dt)
    print(f"[range] silu in the load path of {kernel} {DT_IDS[dt]}: worst error / bound {wr:.3f}")
    assert not bad, bad


# ---- B.1 LayerNorm + modulation on rows with massive channels --------------------------------------------------------------------------------------
LN_CASES = [(h, dt) for h in nr.LN_HS for dt in (BF, F16)]
LN_IDS = [f"{h}-{DT_IDS[dt]}" for h, dt in LN_CASES]


def _ln_check(got, x, shift, scale, dt, what):
    ref, unit = nr.ln_ref64(x, shift, scale, dt)
    got = got.float().cpu()
    assert bool(torch.isfinite(got).all()), what
    w = nr.worst((got.double() - ref).abs(), nr.ln_bound(ref, unit, dt))
    r = nr.row_rel_l2(ref, got)
    fams = nr.ln_families(dt)
    per_fam = ", ".join(f"({f}) {float(r[:, i * nr.LN_ROWS:(i + 1) * nr.LN_ROWS].max()):.2e}" for i, f in enumerate(fams))
    print(f"[range] {what}: worst error / bound {w:.3f} (bound sp(ref) + {nr.C_LN[dt]} 2^-23 max|x| rstd |w|); worst row rel-L2 by family {per_fam} (gate {TOL_SINGLE_OP:.0e})")
    assert w <= 1.0, what
    assert float(r.max()) < TOL_SINGLE_OP, what


def _mods(h, dt, dev, seeds=(0,)):
    """(host pairs, device views of ONE modulation table [B, 2 h len(seeds)])"""
    host = [nr.ln_mod(2, h, dt, s) for s in seeds]
    tab = g(torch.cat([t for pair in host for t in pair], dim=1), dev, dt)
    return host, [tab[:, i * h:(i + 1) * h] for i in range(2 * len(seeds))]


@pytest.mark.parametrize("h,dt", LN_CASES, ids=LN_IDS)
def test_ln_modulate_rows_with_massive_channels(dev, h, dt):
    from diffusionkit_amd import ops
    x = nr.ln_rows(h, dt)
    (pair,), (shift, scale) = _mods(h, dt, dev)
    _ln_check(ops.ln_modulate(g(x, dev, dt), shift, scale), x, *pair, dt, f"ln_modulate h={h} {DT_IDS[dt]}")


@pytest.mark.parametrize("h,dt", LN_CASES, ids=LN_IDS)
def test_ln_modulate_dual_rows_with_massive_channels(dev, h, dt):
    from diffusionkit_amd import ops
    x = nr.ln_rows(h, dt)
    (pa, pb), (sa, ca, sb, cb) = _mods(h, dt, dev, seeds=(0, 1))
    out_a, out_b = ops.ln_modulate_dual(g(x, dev, dt), sa, ca, sb, cb)
    _ln_check(out_a, x, *pa, dt, f"ln_modulate_dual (first pair) h={h} {DT_IDS[dt]}")
    _ln_check(out_b, x, *pb, dt, f"ln_modulate_dual (second pair) h={h} {DT_IDS[dt]}")


@pytest.mark.parametrize("tap_outlier", [True, False], ids=["outliers-in-tap", "outliers-in-rows"])
@pytest.mark.parametrize("h,dt", LN_CASES, ids=LN_IDS)
def test_ln_modulate_add_rows_with_massive_channels(dev, h, dt, tap_outlier):
    from diffusionkit_amd import ops
    x, tap, s, new = nr.ln_add_problem(h, dt, tap_outlier)
    (pair,), (shift, scale) = _mods(h, dt, dev)
    xd, out = ops.ln_modulate_add(g(x, dev, dt), g(tap, dev, dt), s, shift, scale)
    assert torch.equal(xd.float().cpu(), new)  # x <- round(fmaf(s, tap, x)): exact
    _ln_check(out, new, *pair, dt, f"ln_modulate_add ({'tap' if tap_outlier else 'rows'} carry the outliers) h={h} {DT_IDS[dt]}")


@pytest.mark.parametrize("h", nr.LN_HS)
def test_ln_modulate_mx8_rows_with_massive_channels(dev, h):
    """the MX-fp8 output row of the LayerNorm pass = oracle.fp8's quantiser applied to the bf16 result of the same pass (gated above), bit for bit:
    a block that holds an outlier shows its neighbours at the block's coarse scale exactly as the format says"""
    from diffusionkit_amd import ops
    x = nr.ln_rows(h, BF)
    B, S = x.shape[:2]
    (pair,), (shift, scale) = _mods(h, BF, dev)
    shift, scale = shift.contiguous(), scale.contiguous()
    xd = g(x, dev, BF)
    q, sc = ops.ln_modulate_mx8(xd.reshape(B * S, h), shift, scale, mod_seg_len=S)
    y = ops.ln_modulate(xd, shift, scale).float().cpu().reshape(B * S, h)
    q_ref, e_ref = o8.mx8_encode(y)
    n_q, n_e = int((q.cpu() != q_ref).sum()), int((f8.array_to_scales(sc, B * S, h) != e_ref).sum())
    print(f"[range] ln_modulate_mx8 h={h}: {n_q} bytes and {n_e} block scales differ from the quantiser on the bf16 result (gate 0)")
    assert n_q == 0 and n_e == 0


# ---- B.2 GEMM with outlier columns and rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (300, 512, 640)])
@pytest.mark.parametrize("dt,mode", GEMM_CASES, ids=GEMM_IDS)
def test_gemm_outlier_columns_and_rows(dev, dt, mode, M, N, K):
    from diffusionkit_amd import ops
    a, w, b, _ = nr.gemm_outlier_problem(M, N, K, dt)
    ref, bound, mag = nr.gemm_ref64(a, w, b, dt)
    y = _forced_linear(ops, mode, dt, a, w, b, ops.DK_EPI_BIAS, dev)
    bad, wr = nr.gemm_check(y, ref, bound, mag, K, dt)
    print(f"[range] gemm {mode} {DT_IDS[dt]} {M}x{N}x{K} with outlier columns / row: worst error / bound {wr:.3f} (bound sp(ref) + 2 K 2^-24 sum|a||w|)")
    assert not bad, bad


def test_gemm_v3_k_split_outlier_columns_and_rows(dev):
    """... and the K-split of gemm256v3 (fp32 slabs exchanged through the workspace), at test_gemm_v3_remainder_split's smallest shape"""
    from diffusionkit_amd import ops
    M, N, K = 1024, 768, 640
    a, w, b, _ = nr.gemm_outlier_problem(M, N, K, BF)
    ref, bound, mag = nr.gemm_ref64(a, w, b, BF)
    y = _forced_linear(ops, 9, BF, a, w, b, ops.DK_EPI_BIAS, dev, split=True)
    bad, wr = nr.gemm_check(y, ref, bound, mag, K, BF)
    print(f"[range] gemm 9 bf16 {M}x{N}x{K}, K split, with outlier columns / row: worst error / bound {wr:.3f}")
    assert not bad, bad
    assert int(ops.gemm_workspace(dev)[-4096:].sum()) == 0


# ---- C. GroupNorm statistics: long sums, large means --------------------------------------------------------------------------------------------------
def _table_check(tab, vals, gamma, beta, what):
    mean, var = nr.gn_stats64(vals)
    bad, e_scale, e_shift = nr.gn_table_check(tab, mean, var, gamma, beta)
    print(f"[range] {what}: relative rstd error {e_scale:.3e} (bound {nr.GN_RSTD_BOUND:.3e}), shift error / bound {e_shift:.3f}")
    return bad, mean, var


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("rho", nr.GN_RHOS)
@pytest.mark.parametrize("shape", nr.GN_PASS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_statistics_long_sums_large_mean(dev, shape, rho, dt):
    """the stand-alone statistics pass where gn_nchunk is capped at 1024 chunks, ``per`` is ragged and trailing chunks are empty, at mean / sigma
    up to 32: the table against an fp64 two-pass table, the normalised output per (image, group)"""
    from diffusionkit_amd import ops
    x = nr.gn_input(shape, rho, dt)
    gamma, beta = nr.gn_affine(shape[3], dt)
    xd = g(x, dev, dt)
    tab = ops.groupnorm_table(xd, g(gamma, dev, dt), g(beta, dev, dt), nr.GN_G, nr.EPS_GN)
    y = ops.groupnorm(xd, g(gamma, dev, dt), g(beta, dev, dt), nr.GN_G, nr.EPS_GN, False).cpu()
    what = f"groupnorm {shape} mean/sigma {rho} {DT_IDS[dt]}"
    bad, mean, var = _table_check(tab, x, gamma, beta, what)
    tol = TOL_SINGLE_OP if dt == BF else TOL_SINGLE_OP / 8
    cpg = shape[3] // nr.GN_G
    r = max(float(nr.row_rel_l2(nr.gn_out64(x, mean, var, gamma, beta, gi), y[..., gi * cpg:(gi + 1) * cpg].reshape(shape[0], -1)).max())
            for gi in range(nr.GN_G))
    print(f"[range] {what}: worst rel-L2 of the normalised output per (image, group) {r:.3e} (gate {tol:.3e})")
    assert not bad, bad
    assert r < tol


CONV_CASES = [(k, dt) for k in nr.GN_CONV_KERNELS for dt in k[4]]


@pytest.mark.parametrize("rho", nr.GN_RHOS)
@pytest.mark.parametrize("B,H,W", nr.GN_CONV_SHAPES)
@pytest.mark.parametrize("kernel,dt", CONV_CASES, ids=[f"{k[0]}-{DT_IDS[dt]}" for k, dt in CONV_CASES])
def test_conv_tail_statistics_large_mean(dev, kernel, dt, B, H, W, rho):
    """the output statistics of the conv tails (stats_out) with the offset carried by the bias: the table built from the partials against an fp64
    two-pass table over the STORED output"""
    from diffusionkit_amd import ops
    name, mode, C, O, _ = kernel
    x, w, b = nr.conv_stats_problem(B, H, W, C, O, rho, dt)
    try:
        ops.tune("conv_v4", mode)
        y, part = ops.conv3x3_gn(g(x, dev, dt), g(w, dev, dt).reshape(O, -1), g(b, dev, dt), gn_table=None, silu=True, stats_groups=nr.GN_G)
    finally:
        ops.tune("conv_v4", 1)
    gamma, beta = nr.gn_affine(O, dt)
    tab = ops.groupnorm_table(None, g(gamma, dev, dt), g(beta, dev, dt), nr.GN_G, nr.EPS_GN, partials=part, shape=(B, H * W, O))
    yc = y.float().cpu()
    assert abs(float(yc.mean()) - rho) < 0.2 and 0.6 < float(yc.var()) < 1.5
    bad, _, _ = _table_check(tab, yc, gamma, beta, f"conv tail {name} {DT_IDS[dt]} {(B, H, W, C, O)} mean/sigma {rho}")
    assert not bad, bad
