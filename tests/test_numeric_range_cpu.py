"""The gates of the numerical-range tests (tests/_numeric_range.py), proved on the host: for every case of tests/test_gpu_numeric_range.py the
fp32 restatement of the operation passes the gate at HALF the bound (the gate can be met), and a deliberately wrong restatement misses the
whole bound (the gate is not vacuous).  Each test prints the figures the constants were taken from."""
import pytest
import torch

from oracle import vae as ov
from oracle.mmdit import Prec
from tests import _numeric_range as nr
from tests._util import TOL_SINGLE_OP

BF, F16 = nr.BF, nr.F16
DTS = [BF, F16]


def test_domain_and_spacing():
    for dt in DTS:
        d = nr.domain(dt)
        assert d.shape == (256, 256) and bool(torch.isfinite(d).all())
        assert torch.equal(d, nr.rnd(d, dt)) and d.reshape(-1)[:nr.N_FINITE[dt]].unique().numel() == nr.N_FINITE[dt] - 1  # (+0 and -0 are one value)
    one = torch.tensor([1.0, 1.5, 2.0, 0.0, 1e-45, 300.0], dtype=torch.float64)
    assert nr.spacing(one, BF).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133, 2.0]
    assert nr.spacing(one, F16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 0.25]


@pytest.mark.parametrize("bias", [0.0, nr.BIAS_ULP])
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("fn", ["gelu", "silu"])
def test_pointwise_gate(fn, dt, bias):
    x = nr.preact(nr.domain(dt), dt, bias)
    e = nr.pointwise_unit_error(fn, dt, bias)
    print(f"[range cpu] {fn} {dt} bias {bias}: worst |fp32 restatement - ref| / |x| {e:.3e} (c_f {nr.C_POINTWISE[fn]:.2e})")
    assert 2.0 * e <= nr.C_POINTWISE[fn]
    for form in nr.POINTWISE[fn][1]:
        bad, w = nr.pointwise_check(fn, x, nr.rnd(form(x), dt), dt, frac=0.5)
        assert not bad, (form.__name__, bad)
        bad, w = nr.pointwise_check(fn, x, nr.rnd(form(x, wrong=True), dt), dt)
        assert bad and w > 1.0, form.__name__


def test_pointwise_gate_fp8_grid():
    q, e, vals = nr.fp8_grid()
    assert bool(torch.isfinite(vals).all()) and torch.equal(vals, nr.rnd(vals, BF))
    assert float(vals.abs().max()) == 1792.0 and int(((vals.abs() <= 16) & (vals != 0)).sum()) > 20000
    for fn in ("gelu", "silu"):
        for form in nr.POINTWISE[fn][1]:
            assert not nr.pointwise_check(fn, vals, nr.rnd(form(vals), BF), BF, frac=0.5)[0]
            assert nr.pointwise_check(fn, vals, nr.rnd(form(vals, wrong=True), BF), BF)[0]


def _ln_gate(x, shift, scale, dt, what):
    ref, unit = nr.ln_ref64(x, shift, scale, dt)
    got = nr.rnd(nr.ln_f32(x, shift, scale, dt), dt)
    w = nr.worst((got.double() - ref).abs(), 0.5 * nr.ln_bound(ref, unit, dt))
    r = float(nr.row_rel_l2(ref, got).max())
    bad = nr.rnd(nr.ln_f32(nr.ln_zero_outliers(x), shift, scale, dt), dt)
    w_bad = nr.worst((bad.double() - ref).abs(), nr.ln_bound(ref, unit, dt))
    print(f"[range cpu] {what}: error / half bound {w:.3f}, worst row rel-L2 {r:.3e}; outlier columns zeroed: error / bound {w_bad:.1f}")
    assert w <= 1.0 and r < TOL_SINGLE_OP  # (the rel-L2 gate is the project's fixed tolerance, shown met, not halved: one bf16 rounding of such a row is already 2.4e-3)
    assert w_bad > 1.0


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("h", nr.LN_HS)
def test_ln_gate(h, dt):
    e = nr.ln_unit_error(h, dt)
    print(f"[range cpu] ln h={h} {dt}: worst |fp32 restatement - ref| / unit {e:.3f} (c {nr.C_LN[dt]})")
    assert 2.0 * e <= nr.C_LN[dt]
    shift, scale = nr.ln_mod(2, h, dt, 0)
    _ln_gate(nr.ln_rows(h, dt), shift, scale, dt, f"ln_modulate h={h} {dt}")
    shift_b, scale_b = nr.ln_mod(2, h, dt, 1)
    _ln_gate(nr.ln_rows(h, dt), shift_b, scale_b, dt, f"ln_modulate_dual second pair h={h} {dt}")
    for tap_outlier in (True, False):
        _ln_gate(nr.ln_add_problem(h, dt, tap_outlier)[3], shift, scale, dt, f"ln_modulate_add (outliers in the {'tap' if tap_outlier else 'rows'}) h={h} {dt}")


GEMM_SHAPES = [(256, 256, 256), (300, 512, 640), (1024, 768, 640)]  # the last: the K-split case of gemm256v3


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_outlier_gate(M, N, K, dt):
    a, w, b, cols = nr.gemm_outlier_problem(M, N, K, dt)
    ref, bound, mag = nr.gemm_ref64(a, w, b, dt)
    # the large products cancel: the result is small against sum |a| |w|
    assert float(ref[1:].abs().median()) < 0.5 * float(mag[1:].median())
    bad, wr = nr.gemm_check(nr.gemm_f32(a, w, b).to(dt), ref, bound, mag, K, dt, frac=0.5)
    assert not bad, bad
    a0 = a.clone()
    a0[:, cols[1]] = 0.0
    bad, w_bad = nr.gemm_check(nr.gemm_f32(a0, w, b).to(dt), ref, bound, mag, K, dt)
    print(f"[range cpu] gemm {M}x{N}x{K} {dt}: fp32 restatement error / half bound {wr:.3f}; an outlier column zeroed: error / bound {w_bad:.1f}")
    assert bad and w_bad > 1.0


def _gn_gate(x, dt, rho, what, outputs=False):
    gamma, beta = nr.gn_affine(x.shape[-1], dt)
    mean, var = nr.gn_stats64(x)
    bad, e_scale, e_shift = nr.gn_table_check(nr.gn_table_f32(x, gamma, beta), mean, var, gamma, beta, frac=0.5)
    assert not bad, (what, bad)
    wrongs = ["tail"] + (["one_pass"] if rho else [])
    e_w = {}
    for wrong in wrongs:
        bad, e_w[wrong], _ = nr.gn_table_check(nr.gn_table_f32(x, gamma, beta, wrong=wrong), mean, var, gamma, beta)
        assert bad, (what, wrong)
    print(f"[range cpu] {what}: fp32 two-pass rstd error {e_scale:.2e} (half bound {0.5 * nr.GN_RSTD_BOUND:.2e}), shift error / half bound {e_shift:.3f}; "
          + ", ".join(f"{k}: {v:.2e}" for k, v in e_w.items()))
    if outputs:  # the normalised output, per (image, group): one rounding meets the (fixed) gate, a 1 % rstd error misses it
        tol = TOL_SINGLE_OP if dt == BF else TOL_SINGLE_OP / 8
        for gi in (0, nr.GN_G - 1):
            ref = nr.gn_out64(x, mean, var, gamma, beta, gi)
            assert float(nr.row_rel_l2(ref, nr.rnd(ref.to(torch.float32), dt)).max()) < tol
            off = nr.gn_out64(x, mean, var * 1.02, gamma, beta, gi)
            assert float(nr.row_rel_l2(ref, nr.rnd(off.to(torch.float32), dt)).max()) > tol


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("rho", nr.GN_RHOS)
@pytest.mark.parametrize("shape", nr.GN_PASS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_statistics_gate(shape, rho, dt):
    x = nr.gn_input(shape, rho, dt)
    _gn_gate(x, dt, rho, f"groupnorm {shape} mean/sigma {rho} {dt}", outputs=shape[1] == 200)


def test_the_oracles_groupnorm_is_no_yardstick_at_a_large_mean():
    """why GN_E32 is taken from a literal fp32 two-pass and not from oracle.vae.group_norm_nhwc: on the channels-last view F.group_norm forms
    E[x^2] - mean^2 in fp32 -- its own rstd error at mean / sigma 32 is far above anything the gate allows (reported; the oracle is left as it is)"""
    shape = (1, 64, 64, 128)
    e0, e32 = nr.gn_oracle_rstd_error(nr.gn_input(shape, 0, BF)), nr.gn_oracle_rstd_error(nr.gn_input(shape, 32, BF))
    print(f"[range cpu] oracle.vae.group_norm_nhwc, fp32: relative rstd error {e0:.2e} at mean / sigma 0, {e32:.2e} at 32 (gate {nr.GN_RSTD_BOUND:.2e})")
    assert e0 < 1e-5


@pytest.mark.parametrize("rho", nr.GN_RHOS)
@pytest.mark.parametrize("B,H,W", nr.GN_CONV_SHAPES)
@pytest.mark.parametrize("kernel", nr.GN_CONV_KERNELS, ids=lambda k: k[0])
def test_conv_tail_statistics_gate(kernel, B, H, W, rho):
    name, _, C, O, dts = kernel
    for dt in dts:
        x, w, b = nr.conv_stats_problem(B, H, W, C, O, rho, dt)
        y = nr.rnd(ov.conv2d_nhwc(x, w, b, Prec()), dt)  # the stored output: the statistics are those of these values
        mean, var = nr.gn_stats64(y)
        assert abs(float(mean.mean()) - rho) < 0.2 and 0.6 < float(var.mean()) < 1.5
        _gn_gate(y, dt, rho, f"conv tail {name} {(B, H, W, C, O)} mean/sigma {rho} {dt}")
