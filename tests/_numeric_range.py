"""Inputs, fp64 references and per-element bounds of the numerical-range tests (tests/test_numeric_range_cpu.py proves the gates on the host,
tests/test_gpu_numeric_range.py applies them to the HIP kernels).  Plain torch, no GPU.

Every gate has the form  |got - ref| <= sp(ref) + (a term derived from the arithmetic)  per element, ``sp`` the spacing of the element type at the
fp64 reference (one spacing = the final rounding plus one).  Where the derived term has a constant that cannot be derived, it is MEASURED on the
fp32 restatement of the operation (never on the kernel), on the inputs the GPU test uses, and doubled for the hardware's 1-ulp v_rcp / v_exp and
another summation order; the measured values stand beside the constants below and in DESIGN.md section 4."""
import math

import torch

BF, F16 = torch.bfloat16, torch.float16
FMT = {BF: (7, -126, 127), F16: (10, -14, 15)}  # explicit mantissa bits, exponent of the smallest normal, of the largest binade
FLOOR = {BF: 1e-30, F16: 0.0}  # absolute floor of the pointwise gates: __expf overflow below -88.7 and fp32 subnormal flushes (bf16 has fp32's range)
EPS_LN, EPS_GN = 1e-6, 1e-5


def rnd(x: torch.Tensor, dt) -> torch.Tensor:
    """fp32 values representable in ``dt``"""
    return x.to(torch.float32).to(dt).to(torch.float32)


def spacing(r: torch.Tensor, dt) -> torch.Tensor:
    """spacing of ``dt`` at r (fp64): 2^(floor(log2 |r|) - mantissa bits), the subnormal spacing below the normal range"""
    mant, emin, emax = FMT[dt]
    r = r.double().abs()
    _, e = torch.frexp(r)  # r = m 2^e, m in [0.5, 1)
    e = torch.where(r == 0, torch.full_like(e, emin), e - 1).clamp(emin, emax)
    return torch.ldexp(torch.ones_like(r), e - mant)


def worst(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max of err / bound: <= 1 passes the gate, <= 0.5 passes it at half the bound"""
    return float((err.double() / bound.double()).max())


# ---- A. pointwise functions over the whole finite 16-bit domain ----------------------------------------------------------------------------
N_FINITE = {BF: 65280, F16: 63488}


def domain(dt) -> torch.Tensor:
    """every finite bit pattern of ``dt``, padded with zeros to 65536 values, as a [256, 256] fp32 matrix"""
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dt).to(torch.float32)
    v = v[torch.isfinite(v)]
    assert v.numel() == N_FINITE[dt]
    return torch.cat([v, torch.zeros(65536 - v.numel())]).reshape(256, 256)


BIAS_ULP = 2.0 ** -7  # the second pass of the GEMM tails: pre-activation = round(x + 2^-7), the rounding of acc + bias the kernels and the oracle share


def preact(x: torch.Tensor, dt, bias: float) -> torch.Tensor:
    return rnd(x + torch.tensor(bias, dtype=torch.float32), dt) if bias else x


def gelu64(x):
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def silu64(x):
    x = x.double()
    return x * torch.sigmoid(x)


def _fma(a, b, c):
    """fp32 fused multiply-add (the product of two fp32 values is exact in fp64)"""
    f = lambda t: t.double() if isinstance(t, torch.Tensor) else float(torch.tensor(t, dtype=torch.float32))  # noqa: E731
    return (f(a) * f(b) + f(c)).to(torch.float32)


def gelu_f32(x, wrong=False):
    """dk_common.h gelu_erf_f restated in fp32 (A&S 7.1.26 on erfc).  ``wrong``: the polynomial with its last coefficient dropped"""
    x = x.to(torch.float32)
    z = x.abs() * 0.70710678118654752440
    t = 1.0 / _fma(0.3275911, z, 1.0)
    p = _fma(1.061405429, t, -1.453152027)
    p = _fma(p, t, 1.421413741)
    p = _fma(p, t, -0.284496736)
    p = _fma(p, t, 0.0 if wrong else 0.254829592)
    erfc_z = p * t * torch.exp2(-1.4426950408889634 * z * z)
    h = 0.5 * x * erfc_z
    return torch.where(x >= 0, x - h, h)


def gelu_f2_f32(x, wrong=False):
    """dk_common.h gelu_erf_f2 (the packed form of the 256 x 256 GEMM tails): coefficients times 1 / sqrt 2, max(x, 0) - w e"""
    x = x.to(torch.float32)
    z = x.abs() * 0.70710678118654752440
    t = 1.0 / _fma(z, 0.3275911, 1.0)
    p = _fma(t, 0.75052697643, -1.02753365239)
    p = _fma(p, t, 1.00509129513)
    p = _fma(p, t, -0.20116957125)
    p = _fma(p, t, 0.0 if wrong else 0.18019173255)
    e = torch.exp2(z * z * -1.4426950408889634)
    w = p * t * z
    return _fma(-w, e, x.clamp(min=0.0))


def silu_f32(x, wrong=False):
    """dk_common.h silu_f: x * rcp(1 + exp(-x)) in fp32.  ``wrong``: exp(-|x|), the positive branch's exponential on both sides"""
    x = x.to(torch.float32)
    e = torch.exp(-x.abs() if wrong else -x)
    return x * (1.0 / (1.0 + e))


POINTWISE = {"gelu": (gelu64, (gelu_f32, gelu_f2_f32)), "silu": (silu64, (silu_f32,))}
# c_f of the gate |got - ref| <= sp(ref) + c_f |x| + floor: twice the worst |restatement - ref| / |x| over both domains, both passes and
# (GELU) both forms.  Measured (tests/test_numeric_range_cpu.py::test_pointwise_gate prints them): GELU 2.26e-7 (bf16) / 2.71e-7 (float16), SiLU 1.22e-7.
C_POINTWISE = {"gelu": 5.5e-7, "silu": 2.5e-7}


def pointwise_unit_error(fn: str, dt, bias: float) -> float:
    """worst |fp32 restatement - fp64 reference| / |x| over the domain of ``dt`` (before the final rounding)"""
    ref_fn, forms = POINTWISE[fn]
    x = preact(domain(dt), dt, bias)
    nz = x != 0
    ref = ref_fn(x)
    return max(float(((f(x).double() - ref).abs()[nz] / x.double().abs()[nz]).max()) for f in forms)


def pointwise_bound(fn: str, x, ref, dt):
    return spacing(ref, dt) + C_POINTWISE[fn] * x.double().abs() + FLOOR[dt]


def pointwise_check(fn: str, x, got, dt, frac=1.0):
    """(problems, worst ratio) of ``got`` = fn(x) stored as ``dt``: the gate at ``frac`` of the bound, finite outputs, signs, and for GELU
    |gelu(x)| <= |x| and no decrease on x >= 1"""
    x, got = x.reshape(-1).to(torch.float32), got.reshape(-1).to(torch.float32)
    ref = POINTWISE[fn][0](x)
    bad = []
    if not bool(torch.isfinite(got).all()):
        return ["non-finite output for a finite input"], float("inf")
    w = worst((got.double() - ref).abs(), frac * pointwise_bound(fn, x, ref, dt))
    if w > 1.0:
        bad.append(f"gate missed: worst error / bound {w:.3f}")
    if bool(((got != 0) & (torch.sign(got).double() != torch.sign(ref))).any()):
        bad.append("wrong sign")
    if fn == "gelu":
        if bool((got.abs() > x.abs()).any()):
            bad.append("|gelu(x)| > |x|")
        o = torch.argsort(x)
        xs, gs = x[o], got[o]
        keep = xs >= 1
        if bool((gs[keep][1:] < gs[keep][:-1]).any()):
            bad.append("gelu decreases somewhere on x >= 1")
    return bad, w


def fp8_grid():
    """A of the fp8 GEMM tail test: the e4m3 codes (the two NaN codes replaced by zero) as the 256 columns of every row, row r under the block
    scale 2^((r % 12) - 9) in all its eight 32-column blocks: pre-activations q 2^k from +-2^-18 to +-1792, the grid of [-16, 16] at its finest.
    Returns (bytes uint8 [256, 256], E8M0 exponents uint8 [256, 8], the fp32 values)."""
    codes = torch.arange(256, dtype=torch.int32)
    codes = torch.where((codes & 0x7F) == 0x7F, torch.zeros_like(codes), codes).to(torch.uint8)
    q = codes[None, :].expand(256, 256).contiguous()
    e = (127 + (torch.arange(256) % 12) - 9).to(torch.uint8)[:, None].expand(256, 8).contiguous()
    vals = q.view(torch.float8_e4m3fn).to(torch.float32) * torch.ldexp(torch.ones(256, 1), e[:, :1].to(torch.int32) - 127)
    return q, e, vals


# ---- B.1 LayerNorm + modulation on rows with massive channels ----------------------------------------------------------------------------------
LN_HS = (1536, 2432, 3072)
LN_ROWS = 9
OUTLIER_COLS = (5, 700, 1501)  # the three massive channels of family (a)


def ln_families(dt):
    return ("a", "b", "c", "d", "e") if dt == F16 else ("a", "b", "c", "e")


def ln_rows(h: int, dt, seed: int = 0) -> torch.Tensor:
    """[2, 9 * families, h] fp32 values representable in ``dt``: (a) N(0, 1) with three channels at +-1000, (b) 300 + N(0, 1), (c) all entries
    equal (small dyadic values: every partial sum is exact, the variance is 0), (d) float16 only: +-(60000 + 100 N(0, 1)), (e) N(0, 1) with one
    outlier in the last, partial 64-lane chunk (column h - 3)"""
    g = torch.Generator().manual_seed(1000 + seed + h)
    out = []
    for fam in ln_families(dt):
        x = torch.randn(2, LN_ROWS, h, generator=g)
        if fam == "a":
            for i, c in enumerate(OUTLIER_COLS):
                x[..., c] = 1000.0 if i != 1 else -1000.0
        elif fam == "b":
            x = x + 300.0
        elif fam == "c":
            v = torch.tensor([3.0, -0.5, 300.0, 1000.0, -7.0, 0.25, 64.0, -1000.0, 0.0])
            x = v[None, :, None].expand(2, LN_ROWS, h).clone()
        elif fam == "d":
            x = torch.sign(x) * (60000.0 + 100.0 * torch.randn(2, LN_ROWS, h, generator=g))
        else:
            x[..., h - 3] = 1000.0
        out.append(x)
    return rnd(torch.cat(out, dim=1), dt)


def ln_zero_outliers(x: torch.Tensor) -> torch.Tensor:
    """the deliberately wrong input of the LN gates: the outlier columns zeroed"""
    x = x.clone()
    x[..., list(OUTLIER_COLS) + [x.shape[-1] - 3]] = 0.0
    return x


def ln_mod(B: int, h: int, dt, seed: int):
    """(shift, scale) [B, h]; scale >= -0.75, so that |1 + scale| >= 1/4: the gate's second term is proportional to it, and beside a weight
    of zero the plain fp32 roundings of w y + shift (2^-24 |shift|) would be the whole error of the restatement"""
    g = torch.Generator().manual_seed(2000 + seed + h)
    return rnd(torch.randn(B, h, generator=g), dt), rnd((0.5 * torch.randn(B, h, generator=g)).clamp(min=-0.75), dt)


def ln_weight(scale, dt):
    """round(1 + scale): the one rounding in front of the fp32 arithmetic that the kernel and the oracle share"""
    return rnd(torch.tensor(1.0, dtype=torch.float32) + scale, dt)


def ln_ref64(x, shift, scale, dt):
    """fp64 LayerNorm, then w y + shift -> (ref, unit) with unit = 2^-23 max|x_row| rstd |w_c|, the size of the fp32 error of v - mean"""
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + EPS_LN)
    w = ln_weight(scale, dt).double()[:, None]
    ref = (xd - mu) * rstd * w + shift.double()[:, None]
    unit = 2.0 ** -23 * xd.abs().amax(-1, keepdim=True) * rstd * w.abs()
    return ref, unit


def ln_f32(x, shift, scale, dt):
    """the oracle's fp32 restatement (oracle.mmdit.layer_norm, fused batch-1 form of affine_transform), before the output rounding"""
    from oracle import mmdit as om
    return om.layer_norm(x.to(torch.float32), EPS_LN) * ln_weight(scale, dt)[:, None] + shift[:, None]


# c of |got - ref| <= sp(ref) + c unit: twice the worst |fp32 restatement - ref| / unit over every h and family.  Measured: 1.34 (bf16), 5.79
# (float16: family (d), where max|x| rstd is 1 and the unit is as small as the fp32 roundings of w y + shift themselves)
C_LN = {BF: 2.7, F16: 11.6}


def ln_bound(ref, unit, dt):
    return spacing(ref, dt) + C_LN[dt] * unit


def ln_unit_error(h, dt, seed=0) -> float:
    x = ln_rows(h, dt, seed)
    shift, scale = ln_mod(2, h, dt, seed)
    ref, unit = ln_ref64(x, shift, scale, dt)
    err = (ln_f32(x, shift, scale, dt).double() - ref).abs()
    return float((err / unit.clamp(min=1e-300))[unit.expand_as(err) > 0].max())


def row_rel_l2(ref, got):
    """rel-L2 per row (last dimension)"""
    ref, got = ref.double(), got.double()
    return torch.linalg.norm(ref - got, dim=-1) / (torch.linalg.norm(ref, dim=-1) + 1e-30)


# ---- B.2 GEMM with outlier columns and rows -----------------------------------------------------------------------------------------------------
def gemm_outlier_problem(M, N, K, dt, seed=0):
    """A [M, K]: N(0, 1), four columns x 1000 (two of them equal), row 0 x 300 (float16: saturated at the largest finite value); W [N, K]:
    N(0, 0.05^2) with equal and opposite weights on the two equal columns, so their large products cancel; bias [N]"""
    g = torch.Generator().manual_seed(3000 + seed + M + N + K)
    a = torch.randn(M, K, generator=g)
    cols = [3, K // 3, K // 2 + 1, K - 2]
    a[:, cols] *= 1000.0
    a[:, cols[2]] = a[:, cols[0]]
    a[0] *= 300.0
    if dt == F16:
        a = a.clamp(-65504.0, 65504.0)
    w = 0.05 * torch.randn(N, K, generator=g)
    w[:, cols[2]] = -w[:, cols[0]]
    b = torch.randn(N, generator=g)
    return rnd(a, dt), rnd(w, dt), rnd(b, dt), cols


def gemm_ref64(a, w, b, dt):
    """(fp64 result, bound): sp(ref) + 2 K 2^-24 sum_k |a_k| |w_k| -- the running-error bound of K fp32 additions, doubled for a
    truncating accumulator; nothing in it is measured"""
    ref = a.double() @ w.double().t() + b.double()
    mag = a.double().abs() @ w.double().abs().t()
    return ref, spacing(ref, dt) + 2.0 * a.shape[1] * 2.0 ** -24 * mag, mag


def gemm_f32(a, w, b):
    return a.to(torch.float32) @ w.to(torch.float32).t() + b.to(torch.float32)


def gemm_check(got, ref, bound, mag, K, dt, frac=1.0):
    """(problems, worst ratio); float16: an overflowing store gives +-inf where the fp64 result rounds to it, and only there (results within the
    accumulation error of the rounding boundary 65520 may go either way)"""
    got = got.double()
    bad = []
    fin = torch.ones_like(ref, dtype=torch.bool)
    if dt == F16:
        acc = 2.0 * K * 2.0 ** -24 * mag
        want_inf = ref.abs() >= 65520.0
        sure = (ref.abs() - 65520.0).abs() > acc
        if bool((sure & (got.isinf() != want_inf)).any()) or bool((got.isinf() & (torch.sign(got) != torch.sign(ref))).any()):
            bad.append("+-inf exactly where the exact result overflows float16: violated")
        fin = ~want_inf & ~got.isinf()
    if bool(got.isnan().any()) or (dt == BF and not bool(torch.isfinite(got).all())):
        return bad + ["non-finite output"], float("inf")
    w = worst((got - ref).abs()[fin], frac * bound[fin])
    if w > 1.0:
        bad.append(f"gate missed: worst error / bound {w:.3f}")
    return bad, w


# ---- C. GroupNorm statistics: long sums, large means ------------------------------------------------------------------------------------------------
GN_G = 32
GN_RHOS = (0, 8, 32)  # mean / sigma; beyond 32 a bf16 tensor no longer represents its own sigma, nothing is claimed there
GN_PASS_SHAPES = ((1, 129, 255, 512),   # gn_nchunk = 1024, per = 33, 27 empty chunks, unrolled + remainder loop
                  (1, 256, 513, 128),   # 128 channels: 16 pixels per iteration, 1024 chunks of 129
                  (1, 200, 200, 512))   # the production mid-block
# relative rstd error of a literal fp32 two-pass GroupNorm (``gn_table_f32``) against fp64 over every input the gate is applied to.
# Measured: <= 1.63e-7 on the inputs of the stand-alone pass, <= 1.91e-7 on the stored conv outputs (conv256v4's 128-channel tiles, 2 x 32 x 48,
# mean / sigma 32)
GN_E32 = 1.92e-7
GN_RSTD_BOUND = 2.0 * GN_E32 + 1e-6


def gn_input(shape, rho, dt, seed=0):
    g = torch.Generator().manual_seed(4000 + seed + shape[1] * 7 + shape[3] + int(rho))
    return rnd(torch.randn(*shape, generator=g) + float(rho), dt)


def gn_affine(C, dt, seed=0):
    g = torch.Generator().manual_seed(5000 + seed + C)
    return rnd(1.0 + 0.1 * torch.randn(C, generator=g), dt), rnd(0.1 * torch.randn(C, generator=g), dt)


def gn_stats64(x, G=GN_G):
    """fp64 two-pass (mean, var) [B, G] of an NHWC tensor, group by group"""
    B, C = x.shape[0], x.shape[-1]
    cpg = C // G
    mean, var = torch.empty(B, G, dtype=torch.float64), torch.empty(B, G, dtype=torch.float64)
    for gi in range(G):
        v = x[..., gi * cpg:(gi + 1) * cpg].reshape(B, -1).double()
        mean[:, gi] = v.mean(1)
        var[:, gi] = ((v - mean[:, gi, None]) ** 2).mean(1)
    return mean, var


def gn_table64(mean, var, gamma, beta, G=GN_G):
    """(scale | shift) [B, 2, C] in fp64: scale = rstd gamma, shift = beta - mean scale"""
    cpg = gamma.numel() // G
    rstd = (1.0 / torch.sqrt(var + EPS_GN)).repeat_interleave(cpg, 1)
    scale = rstd * gamma.double()[None]
    return torch.stack([scale, beta.double()[None] - mean.repeat_interleave(cpg, 1) * scale], 1)


def gn_table_check(tab, mean, var, gamma, beta, G=GN_G, frac=1.0):
    """(problems, worst relative rstd error, worst shift ratio).  scale: |scale / scale64 - 1| <= GN_RSTD_BOUND (= the relative error of rstd;
    gamma is exact).  shift = beta - mean scale: the same relative error on mean scale, a mean that is off by that fraction of sigma (it moves
    the normalised output as much as the rstd error does), and fp32 roundings of the two terms"""
    ref = gn_table64(mean, var, gamma, beta, G)
    tab = tab.double().cpu()
    cpg = gamma.numel() // G
    e_scale = float((tab[:, 0] / ref[:, 0] - 1.0).abs().max())
    ms = (mean.repeat_interleave(cpg, 1) * ref[:, 0]).abs()
    sig = (torch.sqrt(var + EPS_GN).repeat_interleave(cpg, 1) * ref[:, 0]).abs()
    b_shift = frac * GN_RSTD_BOUND * (ms + sig) + 2.0 ** -22 * (ms + beta.double().abs()[None])
    e_shift = worst((tab[:, 1] - ref[:, 1]).abs(), b_shift)
    bad = []
    if e_scale > frac * GN_RSTD_BOUND:
        bad.append(f"rstd: relative error {e_scale:.3e} > {frac * GN_RSTD_BOUND:.3e}")
    if e_shift > 1.0:
        bad.append(f"shift: error / bound {e_shift:.3f}")
    return bad, e_scale, e_shift


def gn_table_f32(x, gamma, beta, G=GN_G, wrong=None):
    """the table of a literal fp32 two-pass GroupNorm: mean, then the mean of (x - mean)^2, both in fp32.  ``wrong``: "one_pass" = fp32
    E[x^2] - mean^2 over the whole group, "tail" = statistics that miss the last 1/1024 of the pixels (a ragged last chunk dropped)"""
    B, C = x.shape[0], x.shape[-1]
    cpg = C // G
    if wrong == "tail":
        xf = x.reshape(B, -1, C)
        mean, var = gn_stats64(xf[:, :xf.shape[1] - max(1, xf.shape[1] // 1024)][:, :, None], G)
        return gn_table64(mean, var, gamma, beta, G).to(torch.float32)
    mean, var = torch.empty(B, G, dtype=torch.float64), torch.empty(B, G, dtype=torch.float64)
    for gi in range(G):
        v = x[..., gi * cpg:(gi + 1) * cpg].reshape(B, -1).to(torch.float32)
        m = v.mean(1)
        q = ((v * v).mean(1) - m * m).clamp(min=0) if wrong == "one_pass" else ((v - m[:, None]) ** 2).mean(1)
        mean[:, gi], var[:, gi] = m.double(), q.double()
    return gn_table64(mean, var, gamma, beta, G).to(torch.float32)


def gn_oracle_rstd_error(x, G=GN_G) -> float:
    """relative rstd error of oracle.vae.group_norm_nhwc with Prec() against fp64: the slope of its normalised values (unit gamma, zero beta)
    over each whole group.  Reported, not used: F.group_norm on the channels-last view the oracle hands it is itself a one-pass fp32
    E[x^2] - mean^2, so at large mean / sigma it is no yardstick for the statistics (GN_E32 comes from ``gn_table_f32``)"""
    from oracle import vae as ov
    from oracle.mmdit import Prec
    B, C = x.shape[0], x.shape[-1]
    cpg = C // G
    mean64, var64 = gn_stats64(x, G)
    y = ov.group_norm_nhwc(x, torch.ones(C), torch.zeros(C), G, EPS_GN, Prec())
    worst_e = 0.0
    for gi in range(G):
        yv = y[..., gi * cpg:(gi + 1) * cpg].reshape(B, -1).double()
        d = x[..., gi * cpg:(gi + 1) * cpg].reshape(B, -1).double() - mean64[:, gi, None]
        r32 = torch.sqrt((yv * yv).sum(1) / (d * d).sum(1))
        worst_e = max(worst_e, float((r32 * torch.sqrt(var64[:, gi] + EPS_GN) - 1.0).abs().max()))
    return worst_e


def gn_out64(x, mean, var, gamma, beta, gi, G=GN_G):
    """fp64 normalised output of group ``gi``: [B, pixels * C / G]"""
    cpg = x.shape[-1] // G
    sl = slice(gi * cpg, (gi + 1) * cpg)
    v = x[..., sl].double()
    rstd = 1.0 / torch.sqrt(var[:, gi] + EPS_GN)
    y = (v - mean[:, gi, None, None, None]) * rstd[:, None, None, None] * gamma[sl].double() + beta[sl].double()
    return y.reshape(x.shape[0], -1)


# conv-tail statistics: (B, H, W, C, O)
GN_CONV_SHAPES = ((1, 16, 16), (2, 32, 48))


def conv_stats_problem(B, H, W, C, O, rho, dt, seed=0):
    """x N(0, 1), w N(0, 1 / 9C) (the conv output has sigma ~ 1), bias = rho: the offset is carried by the bias"""
    g = torch.Generator().manual_seed(6000 + seed + H + C + O + int(rho))
    x = rnd(torch.randn(B, H, W, C, generator=g), dt)
    w = rnd(torch.randn(O, 3, 3, C, generator=g) / math.sqrt(9.0 * C), dt)
    return x, w, rnd(torch.full((O,), float(rho)), dt)


# (C, O) of the conv-tail cases by kernel: conv_halo.hip (bf16, float16), conv256v4.hip's 256- and 128-channel tiles (bf16)
GN_CONV_KERNELS = (("halo", 0, 64, 128, (BF, F16)), ("v4_256", 2, 128, 256, (BF,)), ("v4_128", 2, 128, 128, (BF,)))


def ln_add_problem(h, dt, tap_has_outlier: bool, seed=0):
    """ln_modulate_add: (x, tap, s, the rows x <- round(fmaf(s, tap, x)) the LayerNorm then reads).  The outlier families arrive through the tap
    (x benign) or through x (tap benign); s = 0.5, so s tap is exact and the sum has one fp32 rounding and one to the element type"""
    g = torch.Generator().manual_seed(7000 + seed + h)
    fam = ln_rows(h, dt, seed + 1)
    plain = rnd(torch.randn(fam.shape, generator=g), dt)
    s = 0.5
    x, tap = (plain, rnd((2.0 * fam).clamp(-65504.0, 65504.0), dt) if dt == F16 else 2.0 * fam) if tap_has_outlier else (fam, plain)
    new = rnd((s * tap.double() + x.double()).to(torch.float32), dt)
    return x, tap, s, new
