"""Stochastic samplers (``sampler="euler_a"`` / ``"sde"``) without a GPU: Philox4x32-10 against its published known answers, the moments and
correlations of the normals built on it, the coefficient rows of the two plans, an analytic problem that shows what each method does to the marginal
at a finite number of steps, and the CLI flags.  tests/test_gpu_stochastic.py holds the HIP path against the same definitions.

The bounds on the sample statistics are five standard errors of the statistic for independent standard normals at the sample size used; nothing here
is a tolerance of the code under test."""
import math

import numpy as np
import pytest

from diffusionkit_amd import cli
from diffusionkit_amd.config import MMDIT_CKPT
from diffusionkit_amd.sampler import (ALL_SAMPLERS, SAMPLERS, STOCHASTIC_SAMPLERS, FluxSampler, ModelSamplingDiscreteFlow, check_sampler,
                                      check_sampler_eta, euler_a_coefficients, get_sigmas, philox4x32_10, philox_normal_reference, step_plan,
                                      stochastic_reference)
from tests._stochastic import MOMENT_SEEDS, N_MOMENTS, corr, moment_bounds, moments, variance_ratio

FLUX1, SD3_3 = FluxSampler(shift=1.0), ModelSamplingDiscreteFlow(shift=3.0)


# ---- 1. the generator -----------------------------------------------------------------------------------------------------------------------------------
KNOWN_ANSWERS = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    """Random123's published vectors of philox4x32_10, on Python ints and on arrays"""
    for counter, key, want in KNOWN_ANSWERS:
        assert tuple(philox4x32_10(counter, key)) == want
    cols = [np.asarray(v, dtype=np.uint64) for v in zip(*(c for c, _, _ in KNOWN_ANSWERS))]
    keys = [np.asarray(v, dtype=np.uint64) for v in zip(*(k for _, k, _ in KNOWN_ANSWERS))]
    got = philox4x32_10(cols, keys)
    assert [tuple(int(w[i]) for w in got) for i in range(3)] == [w for _, _, w in KNOWN_ANSWERS]


def test_normal_reference_layout():
    """element r is z[r % 4] of the block of quad quad_offset + r // 4, counter (q lo, q hi, draw, stream), key (seed lo, seed hi): restated on one
    element with Python integers and math"""
    seed, draw, stream, off = (1 << 40) + 7, 3, 0, (1 << 32) - 2
    z = philox_normal_reference(seed, draw, 16, stream, off)
    for r in (0, 1, 6, 7, 9, 15):  # (quads off + 0 .. off + 3: the last two have a non-zero second counter word)
        q = off + r // 4
        o = philox4x32_10((q & 0xffffffff, q >> 32, draw, stream), (seed & 0xffffffff, seed >> 32))
        a = 2 * ((r % 4) // 2)
        u, theta = ((o[a] >> 8) + 1) * 2.0 ** -24, 2.0 * math.pi * (o[a + 1] >> 8) * 2.0 ** -24
        want = math.sqrt(-2.0 * math.log(u)) * (math.sin(theta) if r % 2 else math.cos(theta))
        assert abs(z[r] - want) <= 1e-14 * max(1.0, abs(want)), r
    assert (off + 3) >> 32 == 1
    assert np.array_equal(philox_normal_reference(seed, draw, 8, stream, off + 2), z[8:])
    for bad in (lambda: philox_normal_reference(-1, 0, 4), lambda: philox_normal_reference(1 << 64, 0, 4), lambda: philox_normal_reference(0, 0, 6)):
        with pytest.raises(ValueError):
            bad()


def test_normal_moments_and_correlations():
    """N = 2^20 per (seed, draw): |mean|, |var - 1|, |E z^3|, |E z^4 - 3| and every correlation -- draws 0 and 1 of a seed, seeds 0 and 1, lags 1 and 4
    inside a row -- below five standard errors"""
    z = {(s, d): philox_normal_reference(s, d, N_MOMENTS) for s in MOMENT_SEEDS for d in (0, 1)}
    bounds = moment_bounds(N_MOMENTS)
    worst = [0.0] * 4
    for key, v in z.items():
        assert bool(np.isfinite(v).all())
        got = moments(v)
        worst = [max(a, b) for a, b in zip(worst, got)]
        assert all(g < b for g, b in zip(got, bounds)), (key, got, bounds)
    cors = {}
    for s in MOMENT_SEEDS:
        cors[f"seed {s}: draw 0 x draw 1"] = corr(z[s, 0], z[s, 1])
        for lag in (1, 4):
            cors[f"seed {s}: lag {lag}"] = corr(z[s, 0][:-lag], z[s, 0][lag:])
    cors["seed 0 x seed 1"] = corr(z[0, 0], z[1, 0])
    print("[stochastic] largest |mean| {:.2e}, |var - 1| {:.2e}, |E z^3| {:.2e}, |E z^4 - 3| {:.2e}; bounds {:.2e} {:.2e} {:.2e} {:.2e}; largest "
          "correlation {:.2e} (bound {:.2e}); largest |z| {:.3f}".format(*worst, *bounds, max(cors.values()), bounds[0],
                                                                        max(float(np.abs(v).max()) for v in z.values())))
    assert all(v < bounds[0] for v in cors.values()), cors


# ---- 2. the plans -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smp", [FLUX1, SD3_3], ids=["flux", "sd3"])
@pytest.mark.parametrize("n", [1, 2, 4, 9])
def test_plan_rows(smp, n):
    sigmas = get_sigmas(smp, n)
    s = [float(v) for v in sigmas]
    euler = step_plan("euler", sigmas)
    assert step_plan("euler_a", sigmas, 0.0) == euler and all(r.cn == 0.0 and r.cx == 1.0 and r.draw == -1 for r in euler)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    for name, eta in (("euler_a", None), ("euler_a", 0.35), ("sde", None)):
        rows = step_plan(name, sigmas, eta)
        assert len(rows) == n and all(r.ends_step and not r.reads_h and not r.writes_h and r.ch == 0.0 for r in rows)
        for i, r in enumerate(rows):
            assert (r.index, r.sigma, r.sigma_next) == (i, s[i], s[i + 1])
            assert all(math.isfinite(v) and f32(v) == v for v in (r.cx, r.cd, r.cn))
            if s[i + 1] == 0.0:  # a step that ends at sigma' = 0 is its Euler row
                assert r == euler[i] and r.cn == 0.0
                continue
            assert r.cn > 0.0 and r.draw == r.index
            if name == "sde":
                assert (r.cx, r.cd, r.cn) == (f32(1.0 - s[i + 1]), f32(-(1.0 - s[i + 1]) * s[i]), s[i + 1])
            else:
                e = 1.0 if eta is None else eta
                down, cx, cd, cn = euler_a_coefficients(s[i], s[i + 1], e)
                assert down == s[i + 1] * (1.0 + (s[i + 1] / s[i] - 1.0) * e) and cx == (1.0 - s[i + 1]) / (1.0 - down) and cd == cx * (down - s[i])
                assert abs(cn * cn + (cx * down) ** 2 - s[i + 1] ** 2) <= 1e-12  # (before rounding: the marginal's variance is kept)
                assert (r.cx, r.cd, r.cn) == (f32(cx), f32(cd), f32(cn))
    # the deterministic plans carry the defaults, and a row built without the new fields compares equal to one built with them
    for name in SAMPLERS:
        assert all(r.cn == 0.0 and r.draw == -1 for r in step_plan(name, sigmas))
    assert type(euler[0])(*euler[0][:11]) == euler[0]


def test_cut_schedule_keeps_its_draws():
    """img2img: denoise 0.5 of 8 steps keeps sigmas[4:]; with the number of entries cut passed on, its rows are the whole plan's rows 4.. -- the same
    coefficients and the same draws -- with the index counted from the cut"""
    for smp in (FLUX1, SD3_3):
        sigmas = get_sigmas(smp, 8)
        for name in STOCHASTIC_SAMPLERS:
            whole, cut = step_plan(name, sigmas), step_plan(name, sigmas[4:], first_draw=4)
            assert len(cut) == 4
            for k, (a, b) in enumerate(zip(whole[4:], cut)):
                assert b.index == k and a.index == k + 4 and b._replace(index=a.index) == a
            assert [r.draw for r in cut[:-1]] == [4, 5, 6] and cut[-1].draw == -1


def test_refusals():
    sigmas = get_sigmas(FLUX1, 4)
    for eta in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            step_plan("euler_a", sigmas, eta)
    for name in ("heun", "euler", "ab2", "sde"):
        with pytest.raises(ValueError, match="euler_a"):
            step_plan(name, sigmas, 0.5)
        with pytest.raises(ValueError, match="euler_a"):
            check_sampler_eta(name, 0.5)
        assert check_sampler_eta(name, None) == 1.0
    assert check_sampler_eta("euler_a", None) == 1.0 and check_sampler_eta("euler_a", 0.25) == 0.25
    for call in (lambda: check_sampler("dpm"), lambda: step_plan("euler_ancestral", sigmas)):
        with pytest.raises(ValueError, match="euler, heun, ab2, euler_a, sde"):
            call()
    assert all(check_sampler(s) == s for s in ALL_SAMPLERS) and ALL_SAMPLERS == SAMPLERS + STOCHASTIC_SAMPLERS
    with pytest.raises(ValueError, match="sigma_down = 1"):  # (sigma' = 1: the schedule does not leave pure noise)
        step_plan("euler_a", np.asarray([1.0, 1.0, 0.5, 0.0], dtype=np.float32))


def test_stochastic_reference():
    sigmas = get_sigmas(FLUX1, 4)
    g = np.random.default_rng(3)
    x, den, xi = g.standard_normal(64), g.standard_normal(64), g.standard_normal(64)
    r = step_plan("sde", sigmas)[1]
    assert np.allclose(stochastic_reference(x, den, r, xi), (1.0 - r.sigma_next) * den + r.sigma_next * xi, rtol=0, atol=1e-6)  # (the rows are fp32)
    r = step_plan("euler", sigmas)[1]
    assert np.array_equal(stochastic_reference(x, den, r, None), x + r.cd * (x - den) / r.sigma)


# ---- 3. the analytic problem ------------------------------------------------------------------------------------------------------------------------------
def test_analytic_marginals():
    """data N(0, 0.7^2), the exact denoiser, a linear schedule 1 -> 0, 65536 elements: var(x_final) / s^2 at 8 / 16 / 32 steps.  euler and euler_a(1)
    move monotonically towards 1; euler_a(0) is euler.  sde's line is printed, not asserted: re-drawing all of the noise at every step does not keep
    the marginal of a mean-predicting denoiser at a finite number of steps (profiles/stochastic_samplers.md)."""
    table = {steps: (variance_ratio("euler", steps), variance_ratio("euler_a", steps, 1.0), variance_ratio("sde", steps)) for steps in (8, 16, 32)}
    for steps, row in table.items():
        print(f"[stochastic] analytic, {steps} steps: var / s^2 euler {row[0]:.3f}, euler_a(1) {row[1]:.3f}, sde {row[2]:.3f}")
        assert variance_ratio("euler_a", steps, 0.0) == row[0]
    for k in (0, 1):
        v = [table[s][k] for s in (8, 16, 32)]
        assert v[0] < v[1] < v[2] < 1.0 and 1.0 - v[2] < 0.2, (k, v)


# ---- 4. the CLI ---------------------------------------------------------------------------------------------------------------------------------------------
def parse(argv):
    return cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(argv)


def test_cli_flags():
    base = cli.resolve(parse(["--prompt", "x"]))
    assert "sampler" not in base and "sampler_eta" not in base
    for name in STOCHASTIC_SAMPLERS:
        assert cli.resolve(parse(["--prompt", "x", "--sampler", name])) == dict(base, sampler=name)
    assert cli.resolve(parse(["--prompt", "x", "--sampler", "euler_a", "--sampler-eta", "0.5"])) == dict(base, sampler="euler_a", sampler_eta=0.5)
    assert cli.resolve(parse(["--prompt", "x", "--sampler", "sde", "--block-cache", "0.1"])) == dict(base, sampler="sde", block_cache=0.1)
    for argv in (["--sampler", "heun", "--sampler-eta", "0.5"], ["--sampler", "sde", "--sampler-eta", "0.5"], ["--sampler-eta", "0.5"]):
        with pytest.raises(ValueError, match="euler_a"):
            cli.resolve(parse(["--prompt", "x"] + argv))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        cli.resolve(parse(["--prompt", "x", "--sampler", "euler_a", "--sampler-eta", "1.5"]))
    with pytest.raises(SystemExit):
        parse(["--prompt", "x", "--sampler", "ancestral"])


def test_keywords_are_keyword_only():
    import inspect
    from diffusionkit_amd.pipeline import DiffusionPipeline
    for fn in (DiffusionPipeline.denoise_latents, DiffusionPipeline.generate_image):
        p = inspect.signature(fn).parameters["sampler_eta"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
