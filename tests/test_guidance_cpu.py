"""Guidance modes (``guidance="rescale"`` / ``"apg"``, ``guidance_interval=``) without a GPU: the identities of ``sampler.guide_reference`` (the
float64 statement of the modes), the classification of a plan's rows under an interval, the guided loops restated on the oracle that
tests/test_gpu_guidance.py then holds the HIP path against, and the validation, CLI flags and signatures.

The reference has one way to combine the two predictions (CFGDenoiser: neg + w (text - neg)), so the others are restated here: ``guided_loop`` is
tests/test_samplers_cpu.py's ``plan_loop`` with ``guide_reference`` between the two predictions of a guided evaluation, and the evaluations an
interval leaves out run on the prompt row alone.  None of this says anything about image quality on a trained checkpoint."""
import inspect

import numpy as np
import pytest
import torch

from diffusionkit_amd import cli
from diffusionkit_amd.config import MMDIT_CKPT
from diffusionkit_amd.sampler import (GUIDANCE, ModelSamplingDiscreteFlow, check_guidance, check_interval, get_sigmas, guidance_rows, guide_reference,
                                      step_plan)
from diffusionkit_amd.weights import synth_mmdit_weights
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec
from tests._util import BF
from tests.test_inpaint_cpu import family_inputs, t_act_of
from tests.test_samplers_cpu import blend, plan_loop, start_state

SD3_3 = ModelSamplingDiscreteFlow(shift=3.0)
W = 5.0
APG = dict(eta=0.0, norm_threshold=0.0, momentum=-0.5)  # the pipeline cases' APG setting


def operands(seed, n_img=3, shape=(6, 10, 16)):
    """seeded float64 (c, u) with a per-image offset, so that mean and standard deviation differ between the images"""
    rng = np.random.RandomState(seed)
    c = rng.randn(n_img, *shape) + 0.3 * np.arange(n_img).reshape(-1, 1, 1, 1)
    u = c + 0.2 * rng.randn(n_img, *shape) + 0.05
    return c, u


def per_image(v):
    return v.reshape(v.shape[0], -1)


# ---- 1. identities of guide_reference -------------------------------------------------------------------------------------------------------------------
def test_rescale_identities():
    c, u = operands(1)
    cfg, _ = guide_reference(c, u, W)
    assert np.array_equal(cfg, u + W * (c - u))
    r0, _ = guide_reference(c, u, W, "rescale", rescale=0.0)
    assert np.array_equal(r0, cfg), "rescale at phi = 0 is not cfg"
    r1, _ = guide_reference(c, u, W, "rescale", rescale=1.0)
    err = np.abs(per_image(r1).std(axis=1) - per_image(c).std(axis=1)).max()
    print(f"[guidance] rescale phi = 1: |std(den) - std(c)| {err:.2e}")
    assert err < 1e-12
    r7, _ = guide_reference(c, u, W, "rescale", rescale=0.7)
    s = 0.7 * per_image(c).std(axis=1) / per_image(cfg).std(axis=1) + 0.3
    assert np.allclose(r7, cfg * s.reshape(-1, 1, 1, 1), rtol=0, atol=1e-12) and not np.array_equal(r7, cfg)
    assert np.all(s < 1.0)  # (guidance at w = 5 inflates the standard deviation: the rescale shrinks)


def test_apg_identities():
    c, u = operands(2)
    cfg, _ = guide_reference(c, u, W)
    e1, _ = guide_reference(c, u, W, "apg", eta=1.0)
    err = np.abs(e1 - cfg).max()
    print(f"[guidance] apg eta = 1 against cfg: max_abs {err:.2e}")
    assert err < 1e-12
    e0, _ = guide_reference(c, u, W, "apg", eta=0.0)
    dots = (per_image(e0 - c) * per_image(c)).sum(axis=1)
    scale = np.linalg.norm(per_image(e0 - c), axis=1) * np.linalg.norm(per_image(c), axis=1)
    print(f"[guidance] apg eta = 0: <den - c, c> / (|den - c| |c|) per image {dots / scale}")
    assert np.all(np.abs(dots) <= 1e-12 * scale) and not np.allclose(e0, cfg)
    # a threshold below |c - u|: the direction is clipped to norm r (eta = 1: den - c = (w - 1) a D)
    nd = np.linalg.norm(per_image(c - u), axis=1)
    r = 0.5 * float(nd.min())
    clipped, _ = guide_reference(c, u, W, "apg", eta=1.0, norm_threshold=r)
    got = np.linalg.norm(per_image(clipped - c), axis=1) / (W - 1.0)
    print(f"[guidance] apg r = {r:.3f} below |c - u| = {nd}: |a D| {got}")
    assert np.allclose(got, r, rtol=1e-12, atol=0)
    loose, _ = guide_reference(c, u, W, "apg", eta=1.0, norm_threshold=2.0 * float(nd.max()))
    assert np.array_equal(loose, e1)  # (a threshold above the norm: a = 1)


def test_apg_momentum_recurrence():
    """three calls: D_t = (c_t - u_t) + beta D_{t-1}; the first reads nothing, the last writes nothing"""
    beta, m, want = -0.5, None, None
    for t in range(3):
        c, u = operands(10 + t)
        den, m_new = guide_reference(c, u, W, "apg", eta=1.0, momentum=beta, m=m, reads_m=t > 0, writes_m=t < 2)
        want = (c - u) + (beta * want if t > 0 else 0.0)
        assert np.allclose(den, c + (W - 1.0) * want, rtol=0, atol=1e-12), t
        if t < 2:
            assert np.array_equal(m_new, want) and m_new is not m
        else:
            assert m_new is m
        m = m_new
    # reads_m off: a NaN-filled buffer is not read
    c, u = operands(3)
    den, _ = guide_reference(c, u, W, "apg", momentum=beta, m=np.full_like(c, np.nan), reads_m=False)
    assert np.isfinite(den).all()


def test_degenerate_cases_stay_finite():
    c, u = operands(4)
    const = np.ones_like(c)
    den, _ = guide_reference(const, const, W, "rescale", rescale=0.7)  # std(g) == 0: s = 1
    assert np.array_equal(den, const)
    den, _ = guide_reference(c, c, W, "apg", norm_threshold=1.0)  # |D| == 0: a = 1
    assert np.array_equal(den, c)
    den, _ = guide_reference(np.zeros_like(c), u, W, "apg", norm_threshold=1.0)  # c == 0: b = 0
    assert np.isfinite(den).all()
    for mode in GUIDANCE:
        den, _ = guide_reference(np.zeros_like(c), np.zeros_like(c), W, mode)
        assert np.array_equal(den, np.zeros_like(c)), mode
    # one degenerate image does not disturb the others
    c2 = c.copy()
    c2[1] = 0.0
    den, _ = guide_reference(c2, u, W, "apg", norm_threshold=1.0)
    ref, _ = guide_reference(c, u, W, "apg", norm_threshold=1.0)
    assert np.isfinite(den).all() and np.array_equal(den[0], ref[0]) and np.array_equal(den[2], ref[2])


# ---- 2. interval classification ------------------------------------------------------------------------------------------------------------------------
def test_interval_classification():
    sigmas = get_sigmas(SD3_3, 4)
    print(f"[guidance] tiny SD3 4-step schedule: {sigmas}")
    assert float(sigmas[0]) > 0.9 and 0.5 <= float(sigmas[1]) <= 0.9 and 0.5 <= float(sigmas[2]) <= 0.9 and float(sigmas[3]) < 0.5
    for name in ("euler", "heun", "ab2"):
        plan = step_plan(name, sigmas)
        rows = guidance_rows(plan, (0.5, 0.9))
        assert [g.guided for g in rows] == [0.5 <= r.sigma <= 0.9 for r in plan], name  # (heun's corrector: by its own sigma)
        assert [g.guided for g in guidance_rows(plan, None)] == [True] * len(plan)
        assert not any(g.guided for g in guidance_rows(plan, (2.0, 3.0)))
        for k, g in enumerate(rows):
            assert g.first == (g.guided and (k == 0 or not rows[k - 1].guided)) and g.feeds == (g.guided and k + 1 < len(rows) and rows[k + 1].guided)
    assert [g.guided for g in guidance_rows(step_plan("euler", sigmas), (0.5, 0.9))] == [False, True, True, False]
    assert [g.guided for g in guidance_rows(step_plan("ab2", sigmas), (0.5, 0.9))] == [False, True, True, False]
    # heun: predictor 0 (sigma 1.0), corrector at sigma 1 (guided), predictor 1, corrector at sigma 2, predictor 2, corrector at sigma 3, euler row 3
    heun = guidance_rows(step_plan("heun", sigmas), (0.5, 0.9))
    assert [g.guided for g in heun] == [False, True, True, True, True, False, False]
    assert [g.first for g in heun] == [False, True, False, False, False, False, False]
    # the ends are inclusive, compared in float32
    s1 = float(sigmas[1])
    assert guidance_rows(step_plan("euler", sigmas), (s1, s1))[1].guided
    assert check_interval(None) == (0.0, float("inf"))
    with pytest.raises(ValueError, match="lo <= hi"):
        check_interval((0.9, 0.5))
    with pytest.raises(ValueError, match="lo <= hi"):
        check_interval((float("nan"), 0.5))


# ---- 3. the guided loops restated on the oracle --------------------------------------------------------------------------------------------------------
def guided_loop(model, name, x, sigmas, conditioning, pooled, cfg_weight, act, t_act=None, mode="cfg", interval=None, inpaint=None, rescale=0.7,
                eta=0.0, norm_threshold=0.0, momentum=0.0):
    """tests/test_samplers_cpu.py's ``plan_loop`` with the guidance modes: a guided evaluation forms both predictions as oracle.pipeline.cfg_denoise
    does and combines them by ``guide_reference`` (float64, rounded to float32 once; "cfg" keeps cfg_denoise's own fp32 expression), an unguided one
    runs on row 0 of the conditioning alone with the modulation cached for row 0.  ``conditioning`` / ``pooled``: [prompt, negative]."""
    timesteps = (t_act or act).r(sigmas * 1000.0)
    plan = step_plan(name, sigmas.numpy())
    rows = guidance_rows(plan, interval)
    hist = m = None
    on = None
    for r, g in zip(plan, rows):
        if g.guided != on:
            on = g.guided
            model.cache_modulation_params(pooled if on else pooled[0:1], timesteps)
        t = float(timesteps[r.index])
        if not on:
            den = op.cfg_denoise(model, x, t, r.sigma, conditioning[0:1], 0.0, act)
        elif mode == "cfg":
            den = op.cfg_denoise(model, x, t, r.sigma, conditioning, cfg_weight, act)
        else:
            x_in = act.r(torch.cat([x] * 2, dim=0))
            both = x_in - model(x_in, conditioning, t) * r.sigma
            reads, writes = momentum != 0.0 and not g.first, momentum != 0.0 and g.feeds
            den64, m = guide_reference(both[0:1].numpy(), both[1:2].numpy(), cfg_weight, mode, rescale=rescale, eta=eta, norm_threshold=norm_threshold,
                                       momentum=momentum, m=m, reads_m=reads, writes_m=writes)
            den = torch.from_numpy(den64).to(torch.float32)
        d = (x - den) / r.sigma
        x_new = r.cx * x + r.cd * d + r.ch * hist if r.reads_h else r.cx * x + r.cd * d
        hist = r.hx * x + r.hd * d if r.writes_h else hist
        x = x_new
        if inpaint is not None:
            noise, x_orig, mm = inpaint
            x = blend(x, r.sigma_next, noise, x_orig, mm.to(torch.float32)[None, :, :, None])
    return x


@pytest.fixture(scope="module")
def sd3():
    cfg, shift, cfgw, text, pooled = family_inputs("sd3_cfg")
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    sigmas = op.get_sigmas(shift, False, 4)
    x0, _ = start_state(sigmas, 2, 8, 16)
    return OracleMMDiT(cfg, wf, Prec()), sigmas, x0, text, pooled, cfgw, dict(act=Prec(BF), t_act=t_act_of(cfg))


@pytest.mark.parametrize("name", ["euler", "heun", "ab2"])
def test_guided_loops(sd3, name):
    """tiny SD3 + CFG 5, latent 8 x 16, 4 steps: "cfg" with the default interval is plan_loop bit for bit; an interval that excludes every step is the
    cfg_weight = 0 loop on the prompt row bit for bit; the other settings run, stay finite and differ from cfg"""
    model, sigmas, x0, text, pooled, cfgw, kw = sd3
    plain = plan_loop(model, name, x0, sigmas, text, pooled, cfgw, **kw)
    assert torch.equal(guided_loop(model, name, x0, sigmas, text, pooled, cfgw, **kw), plain)
    prompt_only = plan_loop(model, name, x0, sigmas, text[0:1], pooled[0:1], 0.0, **kw)
    assert torch.equal(guided_loop(model, name, x0, sigmas, text, pooled, cfgw, interval=(2.0, 3.0), **kw), prompt_only)
    assert not torch.equal(prompt_only, plain)
    outs = {"rescale": guided_loop(model, name, x0, sigmas, text, pooled, cfgw, mode="rescale", **kw),
            "apg": guided_loop(model, name, x0, sigmas, text, pooled, cfgw, mode="apg", **APG, **kw),
            "interval": guided_loop(model, name, x0, sigmas, text, pooled, cfgw, interval=(0.5, 0.9), **kw)}
    for what, x in outs.items():
        assert bool(torch.isfinite(x).all()) and not torch.equal(x, plain) and not torch.equal(x, prompt_only), what
    # rescale at phi = 0 is cfg up to the float64 evaluation of the combine
    r0 = guided_loop(model, name, x0, sigmas, text, pooled, cfgw, mode="rescale", rescale=0.0, **dict(kw, act=Prec()))
    p0 = plan_loop(model, name, x0, sigmas, text, pooled, cfgw, **dict(kw, act=Prec()))
    err = float((r0 - p0).abs().max())
    print(f"[guidance] {name}: rescale phi = 0 (float64 combine) against plan_loop (fp32 combine), no activation rounding: max_abs {err:.2e}")
    assert err < 1e-3


# ---- 4. validation, CLI, signatures --------------------------------------------------------------------------------------------------------------------
def test_unknown_guidance_lists_the_valid_ones():
    assert GUIDANCE == ("cfg", "rescale", "apg")
    assert check_guidance(None) == "cfg" and all(check_guidance(g) == g for g in GUIDANCE)
    for call in (lambda: check_guidance("cads"), lambda: guide_reference(np.zeros((1, 2)), np.zeros((1, 2)), 5.0, "pag")):
        with pytest.raises(ValueError, match="cfg, rescale, apg"):
            call()


def test_pipeline_validation():
    from diffusionkit_amd.pipeline import _DEFAULT_GUIDANCE, _guidance_options
    d = _DEFAULT_GUIDANCE
    args = lambda **kw: _guidance_options(*(kw.get(k, v) for k, v in (("mode", None), ("guidance_rescale", d["guidance_rescale"]),  # noqa: E731
                                                                       ("apg_eta", d["apg_eta"]), ("apg_norm_threshold", d["apg_norm_threshold"]),
                                                                       ("apg_momentum", d["apg_momentum"]), ("interval", None))), kw.get("w", 5.0))
    assert args() is None and args(mode="cfg") is None and args(w=0.0) is None  # (defaults: the loops run as they always did, FLUX included)
    assert args(mode="apg")["mode"] == "apg" and args(interval=(0.5, 0.9))["interval"] == (0.5, float(np.float32(0.9)))
    for kw in (dict(mode="rescale"), dict(mode="apg"), dict(interval=(0.5, 0.9)), dict(apg_eta=0.5), dict(guidance_rescale=0.5)):
        with pytest.raises(ValueError, match="cfg_weight"):
            args(w=0.0, **kw)
    with pytest.raises(ValueError, match="cfg, rescale, apg"):
        args(mode="cads")
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            args(mode="rescale", guidance_rescale=bad)
    for k in ("apg_eta", "apg_norm_threshold", "apg_momentum"):
        with pytest.raises(ValueError, match=k):
            args(mode="apg", **{k: float("inf")})
    with pytest.raises(ValueError, match="lo <= hi"):
        args(interval=(0.9, 0.5))


def parse(argv):
    return cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(argv)


def test_cli_guidance_flags():
    r = cli.resolve(parse(["--prompt", "a cat"]))
    assert r == {"cfg": 0.0, "shift": 1.0, "height": 512, "width": 512, "flux": True, "low_memory_mode": True}  # without the flags: what it was
    sd3 = ["--prompt", "x", "--model-version", "argmaxinc/mlx-stable-diffusion-3-medium"]
    base = cli.resolve(parse(sd3))
    assert base == {"cfg": 5.0, "shift": 3.0, "height": 512, "width": 512, "flux": False, "low_memory_mode": True}
    for name in GUIDANCE:
        assert cli.resolve(parse(sd3 + ["--guidance", name])) == dict(base, guidance=name)
    got = cli.resolve(parse(sd3 + ["--guidance", "apg", "--apg-eta", "0.25", "--apg-norm-threshold", "12.5", "--apg-momentum", "-0.5",
                                   "--guidance-interval", "0.5", "0.9", "--guidance-rescale", "0.5"]))
    assert got == dict(base, guidance="apg", apg_eta=0.25, apg_norm_threshold=12.5, apg_momentum=-0.5, guidance_interval=(0.5, 0.9), guidance_rescale=0.5)
    with pytest.raises(SystemExit):
        parse(sd3 + ["--guidance", "cads"])
    with pytest.raises(ValueError, match="guidance-rescale"):
        cli.resolve(parse(sd3 + ["--guidance-rescale", "1.5"]))
    with pytest.raises(ValueError, match="LO <= HI"):
        cli.resolve(parse(sd3 + ["--guidance-interval", "0.9", "0.5"]))
    for flags in (["--guidance", "apg"], ["--guidance-interval", "0.5", "0.9"]):  # FLUX runs without CFG: nothing to guide
        with pytest.raises(ValueError, match="--cfg > 0"):
            cli.resolve(parse(["--prompt", "x"] + flags))


def test_guidance_keywords_are_keyword_only():
    from diffusionkit_amd.pipeline import DiffusionPipeline
    want = {"guidance": None, "guidance_rescale": 0.7, "apg_eta": 0.0, "apg_norm_threshold": 0.0, "apg_momentum": 0.0, "guidance_interval": None}
    for fn in (DiffusionPipeline.denoise_latents, DiffusionPipeline.generate_image):
        params = inspect.signature(fn).parameters
        for name, default in want.items():
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default, (fn.__name__, name)
