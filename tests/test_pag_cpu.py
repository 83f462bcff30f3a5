"""Perturbed-attention guidance without a GPU: the masked attention reference against the plain one (the mask must move the image rows by many
times the gate tests/test_gpu_pag.py applies), ``tests/_pag.PagOracle`` against ``MMDiTXOracle`` (equal with no block perturbed, several gates apart
with one), the option checks of sampler, pipeline and CLI, the host-only route checks of dk_attention_identity_plan, and the new symbols.
Arithmetic only: nothing here says anything about image quality, and no checkpoint has been run."""
import inspect

import pytest
import torch

from diffusionkit_amd import cli
from diffusionkit_amd.config import MMDIT_CKPT, SD3_5_MEDIUM, fp8_config, tiny_flux, tiny_sd3
from diffusionkit_amd.sampler import check_perturbed_attention_guidance
from oracle import pipeline as op
from oracle.mmdit import Prec
from tests import _footprint as fp
from tests import _pag, _slg
from tests._mmditx import MMDiTXOracle
from tests._util import BF, TOL_SINGLE_OP, rel_l2
from tests.test_guidance_cpu import guided_loop
from tests.test_samplers_cpu import start_state
from tests.test_slg_cpu import gate_of

VERSION = "stabilityai/stable-diffusion-3.5-medium"
D = _pag.D
GPU_GATE = TOL_SINGLE_OP  # the larger of the two gates tests/test_gpu_pag.py applies to the operator (bf16; fp16: an eighth)
IDS = ["x".join(map(str, c)) for c in _pag.OP_CASES]


# ---- 1. the masked reference is not the plain one -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _pag.OP_CASES, ids=IDS)
def test_masked_reference_is_not_the_plain_one(case):
    B, H, S_t, S_i = case
    qkv = _pag.op_inputs(case, BF)
    masked, plain = _pag.ref_identity_attention(qkv, H, D, S_t), fp.ref_attention(qkv.double(), H, D)
    assert torch.equal(masked[:, :S_t], plain[:, :S_t]), "the mask touched a text row"  # (adding 0.0 to a score changes no bit)
    e = rel_l2(plain[:, S_t:], masked[:, S_t:])
    print(f"[pag] {case}: masked against plain reference on the image rows {e:.3f} (needs >= {10 * GPU_GATE})")
    if S_i == 1:
        # A single image row sees the text keys and itself: every key.  By the definition the masked result IS the plain one here, so no choice
        # of inputs can separate them; the case stays in the GPU test for the kernel edge it exercises (one image row, a tile walk of 2 tiles)
        assert e == 0.0
        return
    assert e >= 10 * GPU_GATE


@pytest.mark.parametrize("case", _pag.LOUD_CASES, ids=["x".join(map(str, c)) for c in _pag.LOUD_CASES])
def test_masked_reference_loud_keys(case):
    B, H, S_t, S_i = case
    qkv = _pag.op_inputs(case, BF, loud=True)
    e = rel_l2(fp.ref_attention(qkv.double(), H, D)[:, S_t:], _pag.ref_identity_attention(qkv, H, D, S_t)[:, S_t:])
    print(f"[pag] {case} loud keys: masked against plain reference on the image rows {e:.3f}")
    assert e >= 0.5


def test_masked_reference_by_hand():
    """three text and two image tokens, one head: image row 3 is the softmax over keys {0, 1, 2, 3}, row 4 over {0, 1, 2, 4}"""
    qkv = _pag.op_inputs((1, 1, 3, 2), torch.float32, seed=5)
    got = _pag.ref_identity_attention(qkv, 1, D, 3)[0]
    q, k, v = (qkv[0, :, i * D:(i + 1) * D].double() for i in range(3))
    for s, keys in ((3, [0, 1, 2, 3]), (4, [0, 1, 2, 4]), (1, [0, 1, 2, 3, 4])):
        p = torch.softmax(q[s] @ k[keys].t() / 8.0, -1)
        assert torch.allclose(got[s], p @ v[keys], rtol=0, atol=1e-12)
    assert _pag.identity_mask(5, 3).isinf().sum() == 2  # exactly (3, 4) and (4, 3)


# ---- 2. the model oracle ------------------------------------------------------------------------------------------------------------------------------
def test_oracle_with_no_block_perturbed_is_the_base_oracle():
    cfg, n, Hl, Wl, S_t = _pag.FORWARD["b3"]
    wf = {k: v.float() for k, v in _pag.boosted_weights(cfg, (1,)).items()}
    text, pooled, lat = _slg.forward_inputs(cfg, n, Hl, Wl, S_t)
    for P in (Prec(), Prec(BF)):
        assert torch.equal(_slg._final(_pag.PagOracle(cfg, wf, P, ()), pooled, lat, text), _slg._final(MMDiTXOracle(cfg, wf, P), pooled, lat, text))


@pytest.mark.parametrize("pag", _pag.PAG_SETS, ids=[str(s) for s in _pag.PAG_SETS])
@pytest.mark.parametrize("case", list(_pag.FORWARD))
def test_discrimination_forward(case, pag):
    """fp32 perturbed model against fp32 full model on the prompt rows: at least 4 x the gate the fork rows are held to, for every case and set of
    the GPU test.  The GPU test needs the fork rows to FAIL the gate against the full oracle while passing it against the perturbed one: a result
    within one gate of the perturbed oracle is then at least three gates from the full one."""
    n = _pag.FORWARD[case][1]
    res = _pag.forward_refs(case, pag)
    moved, gate = rel_l2(res["full"]["fp32"][:n], res["pag"]["fp32"]), gate_of(res["pag"])
    print(f"[pag] forward {case}, pag {pag}, gate x {_pag.G_GATE:g}, query norm x {_pag.G_QUERY:g}: perturbing moves the output by {moved:.3f}, gate {gate:.4f}, ratio {moved / gate:.1f}")
    assert moved >= 4.0 * gate


def test_discrimination_loop():
    """the four-step loop with the term on steps 1 and 2 against the loop without it: at least 2 x the gate of the loop with the term, as
    tests/test_slg_cpu.py asks of skip-layer guidance"""
    text, pooled = _slg.pipe_inputs()
    sigmas = op.get_sigmas(_slg.SHIFT, False, _slg.STEPS)
    x0, _ = start_state(sigmas, 2, _slg.HL, _slg.WL)
    pk = dict(act=Prec(BF), t_act=Prec(torch.float16))
    res = {}
    for name, P in (("fp32", Prec()), ("emu", Prec(BF))):
        full, pert = _pag.pipe_oracles(P)
        res[name] = _slg.slg_loop(full, pert, "euler", x0, sigmas, text, pooled, _slg.CFGW, slg_scale=_pag.SCALE, slg_interval=_slg.WINDOW, **pk)
    full, pert = _pag.pipe_oracles(Prec())
    off = guided_loop(full, "euler", x0, sigmas, text, pooled, _slg.CFGW, **pk)
    assert torch.equal(_slg.slg_loop(full, pert, "euler", x0, sigmas, text, pooled, _slg.CFGW, slg_scale=0.0, slg_interval=_slg.WINDOW, **pk), off)
    moved, gate = rel_l2(res["fp32"], off), gate_of(res)
    print(f"[pag] loop, pag {_pag.PIPE_PAG}, scale {_pag.SCALE}: term on against term off {moved:.3f}, gate {gate:.4f}, ratio {moved / gate:.1f}")
    assert moved >= 2.0 * gate


# ---- 3. checks and options ----------------------------------------------------------------------------------------------------------------------------
def test_check_perturbed_attention_guidance():
    assert check_perturbed_attention_guidance(3, (13, 2), (0.0, 0.5), 24) == (3.0, (2, 13), (0.0, 0.5))
    assert check_perturbed_attention_guidance(0, [3], None, 4) == (0.0, (3,), None)
    for bad, what in (((float("nan"), (1,), None, 4), "finite"), ((float("inf"), (1,), None, 4), "finite"), ((-0.5, (1,), None, 4), ">= 0"),
                      (("x", (1,), None, 4), "float"), ((2.5, (), None, 4), "at least one"), ((2.5, None, None, 4), "at least one"),
                      ((2.5, (1, 1), None, 4), "twice"), ((2.5, (4,), None, 4), r"\[0, 4\)"), ((2.5, (-1,), None, 4), r"\[0, 4\)"),
                      ((2.5, (1.5,), None, 4), "integers"), ((2.5, (1,), (0.5, 0.2), 4), "start <= stop"), ((2.5, (1,), (-0.1, 0.2), 4), "start <= stop"),
                      ((2.5, (1,), (0.1, 1.2), 4), "start <= stop"), ((2.5, (1,), 0.5, 4), "None or")):
        with pytest.raises(ValueError, match=what):
            check_perturbed_attention_guidance(*bad)


def test_pipeline_options():
    from diffusionkit_amd.pipeline import DiffusionPipeline, _perturbed_attention_options
    opt = lambda *a, cfg=SD3_5_MEDIUM, flux=False, w=5.0, bc=None, ref=None, cond=None, slg=None: _perturbed_attention_options(  # noqa: E731
        *a, cfg, flux, w, bc, ref, cond, slg)
    assert opt(None, None, None) is None
    assert opt(3.0, (13,), None) == {"scale": 3.0, "layers": (13,), "interval": None}
    assert opt(0, (3, 2), (0.0, 0.6)) == {"scale": 0.0, "layers": (2, 3), "interval": (0.0, 0.6)}
    flux8 = fp8_config(tiny_flux(), "speed")
    for args, kw, what in (((3.0, None, None), {}, "pag_layers"), ((None, (1,), None), {}, "pag_scale"), ((None, None, (0.0, 0.5)), {}, "pag_scale"),
                           ((3.0, (1,), None), dict(flux=True), "FLUX"), ((3.0, (1,), None), dict(w=0.0), "cfg_weight"),
                           ((3.0, (1,), None), dict(bc=0.1), "block_cache"), ((3.0, (1,), None), dict(cfg=flux8), "fp8"),
                           ((3.0, (1,), None), dict(ref="ref.png"), "reference image"), ((3.0, (1,), None), dict(cond="canny"), "condition"),
                           ((3.0, (1,), None), dict(slg={"scale": 2.5}), "skip-layer guidance"), ((3.0, (24,), None), {}, r"\[0, 24\)"),
                           ((3.0, (2,), None), dict(cfg=tiny_sd3()), r"\[0, 2\)"), ((-1.0, (1,), None), {}, ">= 0")):
        with pytest.raises(ValueError, match=what):
            opt(*args, **kw)
    for fn in (DiffusionPipeline.denoise_latents, DiffusionPipeline.generate_image):
        params = inspect.signature(fn).parameters
        for k in ("pag_scale", "pag_layers", "pag_interval"):
            assert params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default is None


def test_cli_flags():
    parse = lambda argv: cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(["--prompt", "x"] + argv)  # noqa: E731
    keys = ("pag_scale", "pag_layers", "pag_interval")
    base = ["--model-version", VERSION, "--cfg", "5"]
    assert not any(k in cli.resolve(parse(base)) for k in keys)
    r = cli.resolve(parse(base + ["--pag-scale", "3", "--pag-layers", "13"]))
    assert [r[k] for k in keys] == [3.0, (13,), None]
    r = cli.resolve(parse(base + ["--pag-scale", "1.5", "--pag-layers", "9", "7", "--pag-interval", "0", "0.6"]))
    assert [r[k] for k in keys] == [1.5, (7, 9), (0.0, 0.6)]
    for argv, what in ((base + ["--pag-layers", "7"], "pag_scale"), (base + ["--pag-scale", "3"], "pag_layers"),
                       (["--model-version", VERSION, "--cfg", "0", "--pag-scale", "3", "--pag-layers", "7"], "cfg_weight"),
                       (base + ["--pag-scale", "3", "--pag-layers", "7", "--block-cache", "0.1"], "block_cache"),
                       (base + ["--pag-scale", "3", "--pag-layers", "24"], r"\[0, 24\)"),
                       (base + ["--pag-scale", "3", "--pag-layers", "7", "--slg-scale"], "skip-layer guidance"),
                       (["--model-version", "argmaxinc/mlx-FLUX.1-schnell", "--pag-scale", "3", "--pag-layers", "1"], "FLUX")):
        with pytest.raises(ValueError, match=what):
            cli.resolve(parse(argv))


# ---- 4. the route, host only --------------------------------------------------------------------------------------------------------------------------
def plan(F, dtype=BF, **over):
    from diffusionkit_amd import ops
    B, H, S, Dh = over.pop("B", 2), over.pop("H", 24), over.pop("S", 154 + 1024), over.pop("D", 64)
    h = H * Dh
    kw = dict(q=0x10000, k=0x20000, v=0x30000, out=0x40000, B=B, H=H, S=S, D=Dh, ld=3 * h, ldo=h, scale=0.125)
    kw.update(over)
    return ops.attention_identity_plan(F, dtype=dtype, **kw)


def test_route_of_an_accepted_call():
    from diffusionkit_amd import ops
    for dt in (BF, torch.float16):
        p = plan(154, dt)
        assert (p.kernel, p.qfuse, p.launches, p.split, p.jobs, p.merge, p.quantize) == (4, 0, 1, 1, 0, 0, 0)
        p = plan(154, dt, qn_a=0x50000, qn_b=0x60000, qn_split=154, qn_eps=1e-6)
        assert (p.kernel, p.qfuse, p.launches) == (4, 1, 1)
    assert plan(1).kernel == 4 and plan(154 + 1023).kernel == 4  # the ends of [1, S)
    try:  # kernel 4 whatever the knob says
        for mode in (9, 10):
            ops.tune("attn", mode)
            assert plan(154).kernel == 4
    finally:
        ops.tune("attn", -1)


def test_route_refusals():
    from diffusionkit_amd._lib import DkHipError
    S = 154 + 1024
    for dt in (BF, torch.float16):
        for F, over, what in ((0, {}, "1 <= ident_from < S"), (S, {}, "1 <= ident_from < S"), (S + 5, {}, "1 <= ident_from < S"),
                              (-1, {}, "1 <= ident_from < S"), (154, dict(D=128), "head_dim must be 64"),
                              (154, dict(bias=0x70000, bias_head_stride=S * 1216, ldb=1216), "no score bias"),
                              (154, dict(O8=0x80000, O8_scales=0x90000, o8_ld=24 * 64, o8_rows=2 * S), "no MX-fp8 copy")):
            with pytest.raises(DkHipError, match=what):
                plan(F, dt, **over)


# ---- 5. the library -----------------------------------------------------------------------------------------------------------------------------------
def test_library_symbols():
    from diffusionkit_amd import _lib
    lib = _lib.load()
    assert lib.dk_abi_version() == 5
    header = open(_lib.HEADER_PATH).read()
    assert "#define DK_ABI_VERSION 5" in header
    for name in ("dk_attention_identity_bf16", "dk_attention_identity_f16", "dk_attention_identity_plan", "dk_mmdit_set_perturbed_attention"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and f"int {name}(" in header
    from diffusionkit_amd import ops
    from diffusionkit_amd.engine import MMDiTEngine
    assert callable(ops.attention_identity) and callable(MMDiTEngine.set_perturbed_attention)
