"""Skip-layer guidance without a GPU: the windows of ``sampler.slg_rows``, the option checks, the restated loop (tests/_slg.py) against
tests/test_guidance_cpu.py's ``guided_loop`` at scale 0, the discrimination of the boosted weights -- a skipped block must move the oracle's output by
several times the gate tests/test_gpu_slg.py then applies -- and the new symbols of the library.  Arithmetic only: nothing here says anything about
image quality, and no SD3.5-medium checkpoint has been run."""
import inspect

import pytest
import torch

from diffusionkit_amd import cli
from diffusionkit_amd.config import MMDIT_CKPT, SKIP_LAYER_GUIDANCE, SD3_5_MEDIUM, tiny_sd3
from diffusionkit_amd.sampler import check_skip_layer_guidance, guidance_rows, slg_reference, slg_rows, step_plan
from oracle import pipeline as op
from oracle.mmdit import Prec
from tests import _slg
from tests._util import BF, rel_l2
from tests.test_guidance_cpu import APG, guided_loop, operands
from tests.test_samplers_cpu import start_state

F16 = torch.float16
VERSION = "stabilityai/stable-diffusion-3.5-medium"


def sigmas_of(n, shift=3.0):
    return op.get_sigmas(shift, False, n)


def steps_with_term(name, n, window, interval=None):
    """the 0-based steps whose rows take the term, and whether the rows of every step agree"""
    plan = step_plan(name, sigmas_of(n).numpy())
    rows = slg_rows(plan, guidance_rows(plan, interval), *window)
    assert len(rows) == len(plan) and all(isinstance(v, bool) for v in rows)
    per_step, i = {}, 0
    for r, v in zip(plan, rows):
        per_step.setdefault(i, []).append(v)
        i += r.ends_step
    return [s for s, vs in per_step.items() if any(vs)], all(len(set(vs)) == 1 for vs in per_step.values())


# ---- 1. the windows ---------------------------------------------------------------------------------------------------------------------------------
def test_slg_rows_windows():
    assert steps_with_term("euler", 4, (0.0, 0.6)) == ([1, 2], True)  # 0 < i < 2.4
    assert steps_with_term("euler", 50, (0.01, 0.2)) == (list(range(1, 10)), True)  # 0.5 < i < 10: the published window
    assert steps_with_term("ab2", 50, (0.01, 0.2)) == (list(range(1, 10)), True)
    assert steps_with_term("euler", 4, (0.5, 0.5)) == ([], True)  # start == stop: none
    assert steps_with_term("euler", 4, (0.25, 0.75)) == ([2], True)  # strict on both sides: 1 < i < 3
    assert steps_with_term("euler", 4, (0.0, 1.0)) == ([1, 2, 3], True)  # never step 0


def test_slg_rows_heun_shares_the_steps_decision():
    steps, agree = steps_with_term("heun", 4, (0.0, 0.6))
    assert steps == [1, 2] and agree
    plan = step_plan("heun", sigmas_of(4).numpy())
    rows = slg_rows(plan, guidance_rows(plan), 0.0, 0.6)
    assert len(plan) == 7 and rows == [False, False, True, True, True, True, False]  # (predictor, corrector) x 3, then the last step's Euler row


def test_slg_rows_follow_the_guidance_interval():
    """a row that the guidance interval leaves unguided takes no term: with shift 3 and 4 steps the sigmas are 1, 0.9, 0.75, 0.5"""
    plan = step_plan("euler", sigmas_of(4).numpy())
    sig = [r.sigma for r in plan]
    lo = (sig[2] + sig[1]) / 2  # guides steps 0 and 1 only
    rows = slg_rows(plan, guidance_rows(plan, (lo, 2.0)), 0.0, 1.0)
    assert rows == [False, True, False, False]
    assert slg_rows(plan, guidance_rows(plan, (2.0, 3.0)), 0.0, 1.0) == [False] * 4


# ---- 2. the option checks ---------------------------------------------------------------------------------------------------------------------------
def test_check_skip_layer_guidance():
    assert check_skip_layer_guidance(2.5, (9, 7, 8), (0.01, 0.2), 24) == (2.5, (7, 8, 9), (0.01, 0.2))
    assert check_skip_layer_guidance(0, [3], None, 4) == (0.0, (3,), (0.0, 1.0))
    for bad, what in (((float("nan"), (1,), None, 4), "finite"), ((float("inf"), (1,), None, 4), "finite"), (("x", (1,), None, 4), "float"),
                      ((2.5, (), None, 4), "at least one"), ((2.5, None, None, 4), "at least one"), ((2.5, (1, 1), None, 4), "twice"),
                      ((2.5, (4,), None, 4), r"\[0, 4\)"), ((2.5, (-1,), None, 4), r"\[0, 4\)"), ((2.5, (1.5,), None, 4), "integers"),
                      ((2.5, (1,), (0.5, 0.2), 4), "start <= stop"), ((2.5, (1,), (-0.1, 0.2), 4), "start <= stop"),
                      ((2.5, (1,), (0.1, 1.2), 4), "start <= stop")):
        with pytest.raises(ValueError, match=what):
            check_skip_layer_guidance(*bad)


def test_pipeline_options_and_defaults():
    from diffusionkit_amd.pipeline import DiffusionPipeline, _skip_layer_options
    assert SKIP_LAYER_GUIDANCE[VERSION] == {"layers": (7, 8, 9), "scale": 2.5, "interval": (0.01, 0.2)}
    other = "argmaxinc/mlx-stable-diffusion-3-medium"
    opt = lambda *a, version=VERSION, cfg=SD3_5_MEDIUM, flux=False, w=5.0, bc=None: _skip_layer_options(*a, version, cfg, flux, w, bc)  # noqa: E731
    assert opt(None, None, None) is None
    assert opt(True, None, None) == {"scale": 2.5, "layers": (7, 8, 9), "interval": (0.01, 0.2)}
    assert opt(1.5, (3, 2), None) == {"scale": 1.5, "layers": (2, 3), "interval": (0.01, 0.2)}
    assert opt(1.5, (1,), None, version=other, cfg=tiny_sd3()) == {"scale": 1.5, "layers": (1,), "interval": (0.0, 1.0)}
    for args, kw, what in (((None, (1,), None), {}, "scale"), ((None, None, (0.0, 0.5)), {}, "scale"), ((2.5, None, None), dict(flux=True), "FLUX"),
                           ((2.5, None, None), dict(w=0.0), "cfg_weight"), ((2.5, None, None), dict(bc=0.1), "block_cache"),
                           ((2.5, None, None), dict(version=other), "name them"), ((True, (1,), None), dict(version=other), "name a scale"),
                           ((2.5, (24,), None), {}, r"\[0, 24\)"), ((2.5, (2,), None), dict(version=other, cfg=tiny_sd3()), r"\[0, 2\)")):
        with pytest.raises(ValueError, match=what):
            opt(*args, **kw)
    for fn in (DiffusionPipeline.denoise_latents, DiffusionPipeline.generate_image):
        params = inspect.signature(fn).parameters
        for k in ("skip_layer_guidance", "skip_layers", "skip_layer_interval"):
            assert params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default is None


def test_cli_flags():
    parse = lambda argv: cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(["--prompt", "x"] + argv)  # noqa: E731
    keys = ("skip_layer_guidance", "skip_layers", "skip_layer_interval")
    r = cli.resolve(parse(["--model-version", VERSION, "--cfg", "5"]))
    assert not any(k in r for k in keys)
    r = cli.resolve(parse(["--model-version", VERSION, "--cfg", "5", "--slg-scale"]))
    assert [r[k] for k in keys] == [2.5, (7, 8, 9), (0.01, 0.2)]
    r = cli.resolve(parse(["--model-version", VERSION, "--cfg", "5", "--slg-scale", "1.5", "--skip-layers", "7", "8", "9", "--slg-interval", "0", "0.6"]))
    assert [r[k] for k in keys] == [1.5, (7, 8, 9), (0.0, 0.6)]
    for argv, what in ((["--model-version", VERSION, "--cfg", "5", "--skip-layers", "7"], "scale"),
                       (["--model-version", VERSION, "--cfg", "0", "--slg-scale", "2.5"], "cfg_weight"),
                       (["--model-version", VERSION, "--cfg", "5", "--slg-scale", "2.5", "--block-cache", "0.1"], "block_cache"),
                       (["--model-version", VERSION, "--cfg", "5", "--slg-scale", "2.5", "--skip-layers", "24"], r"\[0, 24\)"),
                       (["--model-version", "argmaxinc/mlx-stable-diffusion-3-medium", "--cfg", "5", "--slg-scale", "2.5"], "name them"),
                       (["--model-version", "argmaxinc/mlx-FLUX.1-schnell", "--slg-scale", "2.5", "--skip-layers", "1"], "FLUX")):
        with pytest.raises(ValueError, match=what):
            cli.resolve(parse(argv))


# ---- 3. the reference expression and the restated loop ------------------------------------------------------------------------------------------------
def test_slg_reference():
    from diffusionkit_amd.sampler import guide_reference
    c, u = operands(11)
    k = c + 0.1 * operands(12)[1]
    for mode, kw in (("cfg", {}), ("rescale", dict(rescale=0.7)), ("apg", dict(eta=0.0, norm_threshold=3.0))):
        g, _ = guide_reference(c, u, 5.0, mode, **kw)
        den, _ = slg_reference(c, u, k, 5.0, 2.5, mode, **kw)
        assert (den == g + 2.5 * (c - k)).all() and (slg_reference(c, u, k, 5.0, 0.0, mode, **kw)[0] == g).all()
        assert (slg_reference(c, u, c, 5.0, 2.5, mode, **kw)[0] == g).all()  # a skip model that changes nothing adds nothing


@pytest.fixture(scope="module")
def loop_case():
    text, pooled = _slg.pipe_inputs()
    sigmas = sigmas_of(_slg.STEPS, _slg.SHIFT)
    x0, _ = start_state(sigmas, 2, _slg.HL, _slg.WL)
    return text, pooled, sigmas, x0, dict(act=Prec(BF), t_act=Prec(F16))


@pytest.mark.parametrize("mode,kw", [("cfg", {}), ("rescale", {}), ("apg", APG)], ids=["cfg", "rescale", "apg"])
def test_restated_loop_at_scale_zero_is_guided_loop(loop_case, mode, kw):
    text, pooled, sigmas, x0, pk = loop_case
    full, skip = _slg.pipe_oracles(Prec())
    want = guided_loop(full, "euler", x0, sigmas, text, pooled, _slg.CFGW, mode=mode, **kw, **pk)
    got = _slg.slg_loop(full, skip, "euler", x0, sigmas, text, pooled, _slg.CFGW, mode=mode, slg_scale=0.0, slg_interval=_slg.WINDOW, **kw, **pk)
    assert torch.equal(got, want)
    off = _slg.slg_loop(full, skip, "euler", x0, sigmas, text, pooled, _slg.CFGW, mode=mode, slg_scale=_slg.SCALE, slg_interval=(0.5, 0.5), **kw, **pk)
    assert torch.equal(off, want)  # an empty window: no evaluation takes the term


# ---- 4. discrimination: the conditions of the GPU tests, on the oracles alone -------------------------------------------------------------------------
def gate_of(res):
    """the project's yardstick (tests/test_gpu_model.py: yardstick_ok) as a number: 2 e_emu + 2e-3"""
    return 2.0 * rel_l2(res["fp32"], res["emu"]) + 2e-3


@pytest.mark.parametrize("skip", _slg.SKIP_SETS, ids=[str(s) for s in _slg.SKIP_SETS])
def test_discrimination_forward(skip):
    """fp32 skip model against fp32 full model on the prompt rows: at least 5 x the gate the fork rows are held to, for every skip set of the GPU test"""
    n = _slg.FORWARD["b3"][1]
    res = _slg.forward_refs("b3", skip)
    moved, gate = rel_l2(res["full"]["fp32"][:n], res["skip"]["fp32"]), gate_of(res["skip"])
    print(f"[slg] forward, skip {skip}, g = {_slg.G:g}: skipping moves the output by {moved:.3f}, gate {gate:.4f}, ratio {moved / gate:.1f}")
    assert moved >= 5.0 * gate


def test_discrimination_forward_heads6():
    n = _slg.FORWARD["heads6_35tok"][1]
    res = _slg.forward_refs("heads6_35tok", (1, 2))
    moved, gate = rel_l2(res["full"]["fp32"][:n], res["skip"]["fp32"]), gate_of(res["skip"])
    print(f"[slg] forward heads 6, skip (1, 2), g = {_slg.G:g}: skipping moves the output by {moved:.3f}, gate {gate:.4f}, ratio {moved / gate:.1f}")
    assert moved >= 5.0 * gate


def test_discrimination_loop(loop_case):
    """the four-step loop with the term on steps 1 and 2 against the loop without it: at least 2 x the gate of the loop with the term"""
    text, pooled, sigmas, x0, pk = loop_case
    res = {}
    for name, P in (("fp32", Prec()), ("emu", Prec(BF))):
        full, skip = _slg.pipe_oracles(P)
        res[name] = _slg.slg_loop(full, skip, "euler", x0, sigmas, text, pooled, _slg.CFGW, slg_scale=_slg.SCALE, slg_interval=_slg.WINDOW, **pk)
    full, skip = _slg.pipe_oracles(Prec())
    off = guided_loop(full, "euler", x0, sigmas, text, pooled, _slg.CFGW, **pk)
    moved, gate = rel_l2(res["fp32"], off), gate_of(res)
    print(f"[slg] loop, skip {_slg.PIPE_SKIP}, g = {_slg.G:g}, scale {_slg.SCALE}: term on against term off {moved:.3f}, gate {gate:.4f}, "
          f"ratio {moved / gate:.1f}")
    assert moved >= 2.0 * gate


# ---- 5. the library ---------------------------------------------------------------------------------------------------------------------------------
def test_library_symbols():
    from diffusionkit_amd import _lib
    lib = _lib.load()
    assert lib.dk_abi_version() == 5
    for name in ("dk_slg_cfg_step", "dk_slg_cfg_step_f16", "dk_mmdit_set_skip_layers"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert len(_lib.SIGNATURES["dk_slg_cfg_step"][1]) == len(_lib.SIGNATURES["dk_guided_cfg_step"][1]) + 1
    header = open(_lib.HEADER_PATH).read()
    assert "#define DK_ABI_VERSION 5" in header and "int dk_mmdit_set_skip_layers(" in header and "int dk_slg_cfg_step_f16(" in header
