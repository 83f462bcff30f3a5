"""Second-order samplers (``sampler="heun"`` / ``"ab2"``) without a GPU: the coefficient rows of ``sampler.step_plan``, their convergence order on a
problem with a closed-form answer, the restated loops on the oracle that tests/test_gpu_samplers.py then holds the HIP path against, and the CLI flag.

The reference has one integrator (sample_euler), so the other two are restated here twice: ``plan_loop`` runs the rows the way dk_lms_cfg_step does
(d = (x - den) / sigma, x' = cx x + cd d + ch H, H' = hx x + hd d, then the inpainting blend at the row's sigma_next), and ``textbook_loop`` writes
Heun's trapezoid rule and variable-step Adams-Bashforth 2 out without the plan.  What the analytic problem shows is the order of the coefficient
tables; it says nothing about image quality on a trained checkpoint."""
import math

import numpy as np
import pytest
import torch

from diffusionkit_amd import cli
from diffusionkit_amd.config import MMDIT_CKPT
from diffusionkit_amd.sampler import SAMPLERS, FluxSampler, ModelSamplingDiscreteFlow, check_sampler, get_sigmas, step_plan
from diffusionkit_amd.weights import synth_mmdit_weights
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec
from tests._util import BF, rel_l2
from tests.test_inpaint_cpu import FAMILIES, family_inputs, half_mask, latent_mask, t_act_of

FLUX1, SD3_3 = FluxSampler(shift=1.0), ModelSamplingDiscreteFlow(shift=3.0)
EVALS = {"euler": lambda n: n, "heun": lambda n: 2 * n - 1, "ab2": lambda n: n}


# ---- 1. convergence order on the Gaussian problem ---------------------------------------------------------------------------------------------------
S2 = 0.25  # the data is N(0, S2)


def gauss_denoiser(x, sigma):
    return x * (1.0 - sigma) * S2 / ((1.0 - sigma) ** 2 * S2 + sigma ** 2)


def gauss_error(name, sigmas):
    """|final state - exact| in float64, from x = 1 at sigmas[0]: the exact flow keeps x proportional to sqrt((1 - sigma)^2 S2 + sigma^2)"""
    x, hist = 1.0, None
    for r in step_plan(name, sigmas):
        d = (x - gauss_denoiser(x, r.sigma)) / r.sigma
        x, hist = r.cx * x + r.cd * d + (r.ch * hist if r.reads_h else 0.0), (r.hx * x + r.hd * d if r.writes_h else hist)
    v = lambda s: math.sqrt((1.0 - s) ** 2 * S2 + s ** 2)  # noqa: E731
    return abs(x - v(float(sigmas[-1])) / v(float(sigmas[0])))


def test_convergence_order():
    """FLUX schedule, shift 1, at 8 / 16 / 32 / 64 steps: halving the step divides the error by about 2 (euler) and about 4 (heun, ab2); on the SD3
    schedule with shift 3, 16 second-order steps beat 64 Euler steps.  Conditions on the coefficient tables, not tolerances of the GPU path."""
    errs = {name: [gauss_error(name, get_sigmas(FLUX1, n)) for n in (8, 16, 32, 64)] for name in SAMPLERS}
    for name, e in errs.items():
        ratios = [a / b for a, b in zip(e, e[1:])]
        print(f"[samplers] FLUX shift 1, {name}: errors " + " ".join(f"{v:.2e}" for v in e) + "; ratios " + " ".join(f"{v:.2f}" for v in ratios))
        if name == "euler":
            assert all(1.7 <= v <= 2.3 for v in ratios), (name, ratios)
        else:
            assert all(v >= 3.5 for v in ratios), (name, ratios)
    euler64 = gauss_error("euler", get_sigmas(SD3_3, 64))
    for name in ("heun", "ab2"):
        e16 = gauss_error(name, get_sigmas(SD3_3, 16))
        print(f"[samplers] SD3 shift 3: {name} at 16 steps {e16:.2e}, euler at 64 steps {euler64:.2e}")
        assert e16 < euler64


# ---- 2. plan structure ----------------------------------------------------------------------------------------------------------------------------------
def is_euler_row(r, sigmas):
    h = np.float32(np.float32(sigmas[r.index + 1]) - np.float32(sigmas[r.index]))  # the fp32 difference dk_euler_cfg_step takes
    return r.cx == 1.0 and r.cd == float(h) and r.ch == 0.0 and not r.reads_h and r.sigma_next == float(sigmas[r.index + 1]) and r.ends_step


@pytest.mark.parametrize("smp", [FLUX1, SD3_3], ids=["flux", "sd3"])
@pytest.mark.parametrize("n", [1, 2, 4, 9])
def test_plan_structure(smp, n):
    sigmas = get_sigmas(smp, n)
    assert len(sigmas) == n + 1 and float(sigmas[-1]) == 0.0
    for name in SAMPLERS:
        rows = step_plan(name, sigmas)
        assert len(rows) == EVALS[name](n) and sum(r.ends_step for r in rows) == n, name
        written = False
        for k, r in enumerate(rows):
            assert r.sigma == float(sigmas[r.index]) and r.sigma != 0.0 and 0 <= r.index < n, (name, k)
            assert all(math.isfinite(v) and float(np.float32(v)) == v for v in (r.cx, r.cd, r.ch, r.hx, r.hd, r.sigma, r.sigma_next)), (name, k)
            assert written or not r.reads_h, f"{name}: row {k} reads H before any row has written it"
            if r.sigma_next == 0.0 or name == "euler" or (name == "ab2" and k == 0):
                assert is_euler_row(r, sigmas), (name, k, r)
            if r.writes_h:
                assert (r.hx, r.hd) == (0.0, 1.0) and k + 1 < len(rows) and rows[k + 1].reads_h, f"{name}: row {k} writes an H nobody reads"
            written = written or r.writes_h
        assert not rows[-1].writes_h and rows[-1].ends_step, name
        if name == "euler":
            assert not any(r.reads_h or r.writes_h for r in rows)
    # heun: predictor (1, h, 0 | H = d) at sigma_i, corrector (1, h/2, -h/2) at sigma_{i+1} on the predicted state
    rows = step_plan("heun", sigmas)
    for i in range(n - 1):
        pr, co = rows[2 * i], rows[2 * i + 1]
        h = float(sigmas[i + 1]) - float(sigmas[i])
        assert (pr.index, pr.sigma_next, pr.cd, pr.reads_h, pr.writes_h, pr.ends_step) == (i, float(sigmas[i + 1]), float(np.float32(h)), False, True, False)
        assert (co.index, co.sigma, co.sigma_next, co.cx, co.reads_h, co.writes_h, co.ends_step) == (i + 1, pr.sigma_next, pr.sigma_next, 1.0, True, False, True)
        assert co.cd == float(np.float32(h / 2)) and co.ch == float(np.float32(-h / 2))
    # ab2: (1, h (1 + w), -h w), w = h / (2 h_prev)
    rows = step_plan("ab2", sigmas)
    for i in range(1, n - 1):
        h, hp = float(sigmas[i + 1]) - float(sigmas[i]), float(sigmas[i]) - float(sigmas[i - 1])
        w = h / (2 * hp)
        assert rows[i].reads_h and rows[i].cd == float(np.float32(h * (1 + w))) and rows[i].ch == float(np.float32(-h * w)) and rows[i].index == i


def test_plan_of_a_cut_schedule_starts_first_order():
    """img2img: denoise 0.5 of 8 steps keeps sigmas[4:], and the first remaining step is an Euler row (heun: a predictor that reads no history)"""
    for smp in (FLUX1, SD3_3):
        sigmas = get_sigmas(smp, 8)[4:]
        for name in SAMPLERS:
            rows = step_plan(name, sigmas)
            assert len(rows) == EVALS[name](4)
            assert rows[0].index == 0 and rows[0].sigma == float(sigmas[0]) and not rows[0].reads_h and rows[0].cx == 1.0
            assert rows[0].cd == float(np.float32(np.float32(sigmas[1]) - np.float32(sigmas[0]))) and rows[0].ch == 0.0


def test_unknown_sampler_lists_the_valid_ones():
    assert check_sampler(None) == "euler" and all(check_sampler(s) == s for s in SAMPLERS)
    for call in (lambda: check_sampler("dpm"), lambda: step_plan("rk4", get_sigmas(FLUX1, 4))):
        with pytest.raises(ValueError, match="euler, heun, ab2"):
            call()


# ---- 3. the restated loops on the oracle ---------------------------------------------------------------------------------------------------------------
def blend(x, sigma_next, noise, x_orig, mm):
    known = sigma_next * noise + (1.0 - sigma_next) * x_orig
    return mm * x + (1.0 - mm) * known


def plan_loop(model, name, x, sigmas, conditioning, pooled, cfg_weight, act, t_act=None, inpaint=None):
    """the rows of step_plan(name, sigmas) on oracle.pipeline.cfg_denoise, as dk_lms_cfg_step applies them; ``inpaint`` = (noise, x_orig, m [h, w]):
    the blend behind every row, at the row's sigma_next"""
    timesteps = (t_act or act).r(sigmas * 1000.0)
    model.cache_modulation_params(pooled, timesteps)
    hist = None
    for r in step_plan(name, sigmas.numpy()):
        den = op.cfg_denoise(model, x, float(timesteps[r.index]), r.sigma, conditioning, cfg_weight, act)
        d = (x - den) / r.sigma
        x_new = r.cx * x + r.cd * d + r.ch * hist if r.reads_h else r.cx * x + r.cd * d
        hist = r.hx * x + r.hd * d if r.writes_h else hist
        x = x_new
        if inpaint is not None:
            noise, x_orig, m = inpaint
            x = blend(x, r.sigma_next, noise, x_orig, m.to(torch.float32)[None, :, :, None])
    return x


def textbook_loop(model, name, x, sigmas, conditioning, pooled, cfg_weight, act, t_act=None):
    """euler: oracle.pipeline.sample_euler's body; heun: x + (h / 2)(d1 + d2) with d2 on the Euler-predicted state (k-diffusion's sample_heun; the
    step that ends at sigma = 0 is an Euler step); ab2: x + h ((1 + w) d - w d_prev), w = h / (2 h_prev), the first step and the step that ends at
    sigma = 0 first-order.  Written without the plan."""
    timesteps = (t_act or act).r(sigmas * 1000.0)
    model.cache_modulation_params(pooled, timesteps)
    s = [float(v) for v in sigmas]
    d_prev = None
    for i in range(len(s) - 1):
        h = s[i + 1] - s[i]
        d = (x - op.cfg_denoise(model, x, float(timesteps[i]), s[i], conditioning, cfg_weight, act)) / s[i]
        if name == "euler" or s[i + 1] == 0.0 or (name == "ab2" and d_prev is None):
            x = x + d * h
        elif name == "heun":
            x_pred = x + d * h
            d2 = (x_pred - op.cfg_denoise(model, x_pred, float(timesteps[i + 1]), s[i + 1], conditioning, cfg_weight, act)) / s[i + 1]
            x = x + (h / 2) * (d + d2)
        else:
            w = h / (2 * (s[i] - s[i - 1]))
            x = x + h * ((1 + w) * d - w * d_prev)
        d_prev = d
    return x


def start_state(sigmas, seed, h, w, x_T=None):
    noise = op.get_noise(seed, h, w)
    x_T = op.get_empty_latent(h, w) if x_T is None else x_T
    return sigmas[0] * noise + (1.0 - sigmas[0]) * x_T, noise


@pytest.mark.parametrize("family", list(FAMILIES))
def test_restated_loops(family):
    """tiny FLUX and tiny SD3 + CFG 5, latent 8 x 16, 4 steps.
    Plain: the rows of each plan against the textbook loop.  Both are fp32 evaluations of the same real-valued recurrence on an fp32 oracle with no
    activation rounding (a bf16 rounding of the model input would turn a last-bit difference into a 2^-9 one), so they differ by round-off only:
    a handful of 2^-24 roundings per element and step, carried through three more model evaluations -- rel-L2 < 1e-5 leaves two orders of magnitude
    for that amplification and is four orders below what a wrong coefficient costs (h is about 0.25).  Euler's plan is sample_euler bit for bit.
    Masked: m = 0 returns x_orig bit for bit, m = 1 the plain result bit for bit."""
    cfg, shift, cfgw, text, pooled = family_inputs(family)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    model = OracleMMDiT(cfg, wf, Prec())
    sigmas = op.get_sigmas(shift, cfg.is_flux, 4)
    x0, noise = start_state(sigmas, 2, 8, 16)
    kw = dict(act=Prec(), t_act=t_act_of(cfg) or Prec(BF))
    finals = {}
    for name in SAMPLERS:
        by_rows = plan_loop(model, name, x0, sigmas, text, pooled, cfgw, **kw)
        book = textbook_loop(model, name, x0, sigmas, text, pooled, cfgw, **kw)
        e = rel_l2(book, by_rows)
        print(f"[samplers] {family} {name}: plan rows against the textbook loop, rel_l2 {e:.2e}")
        assert e < 1e-5 and bool(torch.isfinite(by_rows).all())
        finals[name] = by_rows
    assert torch.equal(finals["euler"], op.sample_euler(model, x0, sigmas, text, pooled, cfgw, Prec(), t_act=kw["t_act"]))
    assert rel_l2(finals["euler"], finals["heun"]) > 1e-3 and rel_l2(finals["euler"], finals["ab2"]) > 1e-3  # (three different integrators)
    # masked, from an img2img start state, with the production rounding of the model input
    kw = dict(act=Prec(BF), t_act=t_act_of(cfg))
    x_orig = torch.randn(1, 8, 16, 16, generator=torch.Generator().manual_seed(11)) * 1.5 + 0.3
    x0, noise = start_state(sigmas, 2, 8, 16, x_T=x_orig)
    for name in ("heun", "ab2"):
        plain = plan_loop(model, name, x0, sigmas, text, pooled, cfgw, **kw)
        ones = plan_loop(model, name, x0, sigmas, text, pooled, cfgw, inpaint=(noise, x_orig, torch.ones(8, 16)), **kw)
        zeros = plan_loop(model, name, x0, sigmas, text, pooled, cfgw, inpaint=(noise, x_orig, torch.zeros(8, 16)), **kw)
        assert torch.equal(ones, plain), f"{name}: m = 1 is not the unmasked loop"
        assert torch.equal(zeros, x_orig), f"{name}: m = 0 does not return the encoded image"
        m = latent_mask(half_mask(64, 128))
        half = plan_loop(model, name, x0, sigmas, text, pooled, cfgw, inpaint=(noise, x_orig, m), **kw)
        assert torch.equal(half[0][m == 0.0], x_orig[0][m == 0.0]) and not torch.equal(half[0][m == 1.0], plain[0][m == 1.0])


# ---- 4. CLI and the public signature -------------------------------------------------------------------------------------------------------------------
def parse(argv):
    return cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(argv)


def test_cli_sampler_flag():
    r = cli.resolve(parse(["--prompt", "a cat"]))
    assert r == {"cfg": 0.0, "shift": 1.0, "height": 512, "width": 512, "flux": True, "low_memory_mode": True}  # without the flag: what it was
    for name in SAMPLERS:
        assert cli.resolve(parse(["--prompt", "x", "--sampler", name]))["sampler"] == name
    with pytest.raises(SystemExit):
        parse(["--prompt", "x", "--sampler", "dpm"])
    assert cli.resolve(parse(["--prompt", "x", "--sampler", "ab2", "--block-cache", "0.1"])) == dict(r, sampler="ab2", block_cache=0.1)
    with pytest.raises(ValueError, match="block-cache"):
        cli.resolve(parse(["--prompt", "x", "--sampler", "heun", "--block-cache", "0.1"]))


def test_sampler_keyword_is_keyword_only():
    import inspect
    from diffusionkit_amd.pipeline import DiffusionPipeline
    for fn in (DiffusionPipeline.denoise_latents, DiffusionPipeline.generate_image):
        p = inspect.signature(fn).parameters["sampler"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
