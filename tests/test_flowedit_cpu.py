"""FlowEdit without a GPU: the plan of the edit phase, the float64 reference on analytic velocity fields, the refusals of the public interface with
their texts, the CLI flags as data, the two new ABI entries' argument checks, and the closed loop on the oracle at the shapes of the GPU pipeline
tests -- that the bf16-emulating oracle meets the gates those tests apply, and that the edit moves the latent far enough for the gates to see it."""
import ctypes as C
import functools
import re
from dataclasses import replace

import numpy as np
import pytest

from diffusionkit_amd import _lib, cli, sampler
from diffusionkit_amd.config import tiny_flux, tiny_sd3
from diffusionkit_amd.sampler import FLOWEDIT_DEFAULTS, cfg_combine, check_flowedit, flowedit_plan, flowedit_reference, flowedit_row_reference
from diffusionkit_amd.weights import synth_mmdit_weights
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec
from tests import _flowedit as fe
from tests._util import BF, psnr, randn, rel_l2
from tests.test_abi_and_host import _mmdit_handle
from tests.test_inpaint_cpu import FAMILIES, family_inputs, t_act_of

PLAN_CASES = [(6, 4, 0, 1), (6, 6, 2, 1), (5, 3, 1, 3)]  # (T, n_max, n_min, n_avg)


def schedule(T, shift=3.0):
    return op.get_sigmas(shift, False, T).numpy()


# ---- 1. the plan ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n_max,n_min,n_avg", PLAN_CASES)
def test_plan(T, n_max, n_min, n_avg):
    """the prime row first, then n_avg rows per outer step; the c of a step sum to sigmas[i + 1] - sigmas[i] up to n_avg fp32 roundings; sigma_in stays
    at sigmas[i] for every draw but the last, which moves it to sigmas[i + 1]; the draw numbers are distinct and a function of the schedule alone"""
    s = schedule(T)
    assert s[-1] == 0.0 and len(s) == T + 1
    plan = flowedit_plan(s, n_max, n_min, n_avg)
    assert len(plan) == 1 + n_avg * (n_max - n_min)
    i0 = T - n_max
    assert plan[0].prime and plan[0].c == 0.0 and plan[0].index == i0 and plan[0].next_index == i0 and plan[0].sigma_in == float(s[i0])
    assert not any(r.prime for r in plan[1:])
    rows = plan[1:]
    for step, i in enumerate(range(i0, T - n_min)):
        mine = rows[step * n_avg:(step + 1) * n_avg]
        assert [r.index for r in mine] == [i] * n_avg
        h = float(s[i + 1]) - float(s[i])
        assert abs(sum(r.c for r in mine) - h) <= n_avg * 2.0 ** -24 * abs(h)
        assert all(r.c == float(np.float32(h / n_avg)) for r in mine)
        assert [r.sigma_in for r in mine] == [float(s[i])] * (n_avg - 1) + [float(s[i + 1])]
        assert [r.next_index for r in mine] == [i] * (n_avg - 1) + [i + 1]
        assert [r.ends_step for r in mine] == [False] * (n_avg - 1) + [True]
    assert plan[-1].sigma_in == float(s[T - n_min]) and (n_min > 0 or plan[-1].sigma_in == 0.0)
    draws = [r.draw for r in plan]
    assert len(set(draws)) == len(draws) and min(draws) >= 0
    assert draws == [i0 * n_avg + k for k in range(len(plan))]  # (evaluation (i, k) takes draw i * n_avg + k: nothing about the batch enters)
    assert all(isinstance(v, float) and v == float(np.float32(v)) for r in plan for v in (r.c, r.sigma_in))


def test_plan_refuses():
    s = schedule(6)
    for bad, text in (((4, 4, 1), "n_min < n_max"), ((3, 5, 1), "n_min < n_max"), ((7, 0, 1), "exceeds num_steps"), ((4, -1, 1), "0 <= n_min"),
                      ((4, 0, 0), "edit_n_avg")):
        with pytest.raises(ValueError, match=text):
            flowedit_plan(s, *bad)
    assert check_flowedit(6, 6, 0, 1) == (6, 0, 1)
    assert FLOWEDIT_DEFAULTS == {"sd3": (50, 33, 0, 3.5, 13.5), "flux": (28, 24, 0, 1.5, 5.5)}
    assert sampler.FLOWEDIT_STREAM == 1


# ---- 2. the float64 reference on analytic fields ------------------------------------------------------------------------------------------------------
SEEDS = (3, (1 << 63) + 5)


@pytest.mark.parametrize("T,n_max,n_min,n_avg", PLAN_CASES)
def test_reference_equal_fields_return_the_source(T, n_max, n_min, n_avg):
    """the same field on both sides: Zt == Zs in every row (Z == x_src), so V_tar - V_src == 0 and Z stays x_src exactly"""
    x_src = randn(2, 4, 6, 16, seed=1).double().numpy()
    seen = []

    def velocity(zs, zt, sigma, index):
        seen.append(index)
        assert np.array_equal(zs, zt)
        return fe.field(zs, sigma), fe.field(zt, sigma)
    z, zt = flowedit_reference(x_src, schedule(T), n_max, n_min, n_avg, velocity, SEEDS)
    assert np.array_equal(z, x_src) and len(seen) == n_avg * (n_max - n_min)
    if n_min == 0:
        assert np.array_equal(zt, x_src)  # (x_src + 0: exact)
    else:
        assert not np.array_equal(zt, x_src)  # (noised to sigmas[T - n_min])


@pytest.mark.parametrize("T,n_max,n_min,n_avg", PLAN_CASES)
def test_reference_constant_difference(T, n_max, n_min, n_avg):
    """V_tar = V_src + d: Z moves by d times the sum of the steps' sigma differences, -d (sigmas[T - n_max] - sigmas[T - n_min])"""
    x_src = randn(2, 4, 6, 16, seed=1).double().numpy()
    s, d = schedule(T), 0.37
    z, _ = flowedit_reference(x_src, s, n_max, n_min, n_avg, lambda zs, zt, sigma, index: (fe.field(zs, sigma), fe.field(zs, sigma) + d), SEEDS)
    want = x_src - d * (float(s[T - n_max]) - float(s[T - n_min]))
    assert np.abs(z - want).max() <= 4 * n_avg * (n_max - n_min) * 2.0 ** -24  # (c is rounded to fp32 once per row)


def test_row_reference_and_noise():
    """one row: the statement itself, the noise of stream 1 (not stream 0's, not the next draw's), image j from seeds[j]"""
    x_src, z = randn(2, 4, 6, 16, seed=1).double().numpy(), randn(2, 4, 6, 16, seed=2).double().numpy()
    vs, vt = randn(2, 4, 6, 16, seed=3).double().numpy(), randn(2, 4, 6, 16, seed=4).double().numpy()
    row = sampler.FlowEditRow(2, -0.125, 0.75, 5, False, 3, True)
    xi = fe.xi1_of(SEEDS, row.draw, x_src.shape[1:])
    z1, zs, zt = flowedit_row_reference(z, x_src, vs, vt, row, xi)
    assert np.array_equal(z1, z - 0.125 * (vt - vs)) and np.array_equal(zs, 0.25 * x_src + 0.75 * xi) and np.array_equal(zt, zs + (z1 - x_src))
    z0, _, _ = flowedit_row_reference(z, x_src, None, None, row._replace(prime=True), xi)
    assert np.array_equal(z0, z)
    n = xi[0].size
    assert np.array_equal(xi[1].ravel(), sampler.philox_normal_reference(SEEDS[1], 5, n, 1))
    assert not np.array_equal(xi[0].ravel(), sampler.philox_normal_reference(SEEDS[0], 5, n, 0))
    assert not np.array_equal(xi[0].ravel(), sampler.philox_normal_reference(SEEDS[0], 6, n, 1))
    assert np.array_equal(cfg_combine(vs, vt, 2.5), vt + 2.5 * (vs - vt))


# ---- 3. refusals of the public interface ----------------------------------------------------------------------------------------------------------------
def bare(cls_name):
    """a pipeline object without engines: the refusals come before any GPU work"""
    from diffusionkit_amd import pipeline
    return object.__new__(getattr(pipeline, cls_name))


REFUSED = [(dict(mask_path="m.png"), "mask_path"), (dict(block_cache=0.1), "block_cache"), (dict(guidance="apg"), "guidance mode"),
           (dict(guidance_interval=(0.2, 0.8)), "guidance_interval"), (dict(skip_layer_guidance=2.5), "skip-layer guidance"),
           (dict(pag_scale=1.0, pag_layers=[0]), "perturbed-attention guidance"), (dict(controlnet_image_path="c.png"), "a ControlNet"),
           (dict(ip_adapter_image_embeds=np.zeros(4)), "an IP-Adapter"), (dict(reference_image_path="r.png"), "a reference image"),
           (dict(condition_image_path="c.png"), "condition=")]


@pytest.mark.parametrize("kw,text", REFUSED, ids=[t for _, t in REFUSED])
def test_edit_refuses_by_name(kw, text):
    pipe = bare("DiffusionPipeline")
    with pytest.raises(ValueError, match=re.escape("an edit (edit_source_text) cannot run together with") + ".*" + re.escape(text)):
        pipe.denoise_latents(None, None, num_steps=6, cfg_weight=5.0, image_path="x.png", edit_source_text="a cat", **kw)


def test_edit_refuses_the_rest():
    pipe, flux = bare("DiffusionPipeline"), bare("FluxPipeline")
    edit = dict(num_steps=6, cfg_weight=5.0, edit_source_text="a cat")
    with pytest.raises(ValueError, match="cannot run together with denoise"):
        pipe.denoise_latents(None, None, image_path="x.png", denoise=0.5, **edit)
    with pytest.raises(ValueError, match="needs image_path"):
        pipe.denoise_latents(None, None, **edit)
    for steps, text in (((4, 4), "n_min < n_max"), ((2, 3), "n_min < n_max"), ((7, 0), "n_max = 7 exceeds num_steps = 6")):
        with pytest.raises(ValueError, match=text):
            pipe.denoise_latents(None, None, image_path="x.png", edit_steps=steps, **edit)
    with pytest.raises(ValueError, match="edit_n_avg must be at least 1"):
        pipe.denoise_latents(None, None, image_path="x.png", edit_n_avg=0, **edit)
    for kw in (dict(edit_steps=(4, 0)), dict(edit_n_avg=2), dict(edit_source_cfg=2.0)):
        with pytest.raises(ValueError, match="belong to an edit: give edit_source_text"):
            pipe.denoise_latents(None, None, num_steps=6, cfg_weight=5.0, **kw)
    # a pipeline that was built with one of the excluded parts
    pipe.controlnet = object()
    with pytest.raises(ValueError, match="a ControlNet"):
        pipe.denoise_latents(None, None, image_path="x.png", **edit)
    # the SD3 family edits under CFG on both sides; FLUX.1-schnell has no guidance embedding for a source value
    pipe = bare("DiffusionPipeline")
    pipe.mmdit_config = tiny_sd3()
    for kw in (dict(cfg_weight=0.0), dict(cfg_weight=5.0, edit_source_cfg=0.0)):
        with pytest.raises(ValueError, match="needs classifier-free guidance on both sides"):
            pipe.denoise_latents(None, None, num_steps=6, image_path="x.png", edit_source_text="a cat", **kw)
    flux.mmdit_config = tiny_flux()
    with pytest.raises(ValueError, match="no guidance embedding"):
        flux.denoise_latents(None, None, num_steps=6, cfg_weight=0.0, image_path="x.png", edit_source_text="a cat", edit_source_cfg=1.5)


def test_sharding_refuses_an_edit():
    from diffusionkit_amd.dist import generate_sharded
    with pytest.raises(ValueError, match="cannot run under multi-GPU sharding"):
        generate_sharded(object(), "a dog", [1, 2], 0, 2, image_path="x.png", edit_source_text="a cat")


def test_keywords_are_keyword_only_and_default_off():
    import inspect
    from diffusionkit_amd.pipeline import DiffusionPipeline
    for fn in (DiffusionPipeline.denoise_latents, DiffusionPipeline.generate_image):
        sig = inspect.signature(fn).parameters
        for name in ("edit_source_text", "edit_steps", "edit_n_avg", "edit_source_cfg"):
            assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is None


def test_cli_flags():
    parse = cli.build_parser(tuple(cli_versions())).parse_args
    sd3 = ["--prompt", "a dog", "--model-version", "argmaxinc/mlx-stable-diffusion-3-medium", "--cfg", "5", "--steps", "6"]
    base = cli.resolve(parse(sd3 + ["--image-path", "x.png"]))
    got = cli.resolve(parse(sd3 + ["--image-path", "x.png", "--edit-source-prompt", "a cat", "--edit-steps", "4", "1", "--edit-n-avg", "2",
                                   "--edit-source-cfg", "2.5"]))
    assert got == dict(base, edit_source_text="a cat", edit_steps=(4, 1), edit_n_avg=2, edit_source_cfg=2.5)
    assert cli.resolve(parse(sd3 + ["--image-path", "x.png", "--edit-source-prompt", "a cat"])) == dict(base, edit_source_text="a cat")
    assert set(cli.EDIT_KEYS) == {"edit_source_text", "edit_steps", "edit_n_avg", "edit_source_cfg"}
    for argv, text in ((["--edit-steps", "4", "0"], "need --edit-source-prompt"),
                       (["--edit-source-prompt", "a cat"], "needs --image-path"),
                       (["--image-path", "x.png", "--edit-source-prompt", "a cat", "--denoise", "0.5"], "--denoise"),
                       (["--image-path", "x.png", "--edit-source-prompt", "a cat", "--mask-path", "m.png"], "--mask-path"),
                       (["--image-path", "x.png", "--edit-source-prompt", "a cat", "--block-cache", "0.1"], "--block-cache"),
                       (["--image-path", "x.png", "--edit-source-prompt", "a cat", "--guidance", "apg"], "--guidance"),
                       (["--image-path", "x.png", "--edit-source-prompt", "a cat", "--edit-steps", "7", "0"], "exceeds num_steps"),
                       (["--image-path", "x.png", "--edit-source-prompt", "a cat", "--edit-steps", "3", "3"], "n_min < n_max"),
                       (["--image-path", "x.png", "--edit-source-prompt", "a cat", "--edit-n-avg", "0"], "at least 1")):
        with pytest.raises(ValueError, match=text):
            cli.resolve(parse(sd3 + argv))
    schnell = ["--prompt", "a dog", "--steps", "4", "--image-path", "x.png", "--edit-source-prompt", "a cat"]
    assert cli.resolve(parse(schnell))["edit_source_text"] == "a cat"
    with pytest.raises(ValueError, match="no guidance embedding"):
        cli.resolve(parse(schnell + ["--edit-source-cfg", "1.5"]))


def cli_versions():
    from diffusionkit_amd.config import MMDIT_CKPT
    return MMDIT_CKPT.keys()


# ---- 4. the ABI without a GPU -------------------------------------------------------------------------------------------------------------------------------
NEW_NAMES = ("dk_flowedit_step", "dk_flowedit_step_f16", "dk_mmdit_set_guidance_rows")


def test_new_names_in_header_export_table_and_ctypes_table():
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    declared = set(re.findall(r"\b(dk_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for name in NEW_NAMES:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.dk_abi_version() == 5  # (additive)


def test_flowedit_step_refuses_bad_arguments():
    """every guard answers before anything is launched: host buffers stand in for device memory (never dereferenced), aligned as the entry asks"""
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 63) & ~63
    z, x, out, tok, zs, zt, seeds = (base + 256 * k for k in range(7))
    good = dict(z=z, x_src=x, model_out=out, ld_out=64, tokens=tok, zs_out=zs, zt_out=zt, n_img=1, cfg_on=0, Hl=4, Wl=4, C=16, p=2, order=0, w_src=1.0,
                w_tar=1.0, c=-0.1, sigma_in=0.5, seeds=seeds, draw=3, prime=0)

    def call(fn=lib.dk_flowedit_step, **kw):
        a = dict(good, **kw)
        rc = fn(*(a[k] for k in good), None)
        return rc, lib.dk_last_error().decode()
    for kw, text in ((dict(z=None), "null argument"), (dict(x_src=None), "null argument"), (dict(tokens=None), "null argument"),
                     (dict(zt_out=None), "null argument"), (dict(seeds=None), "null argument"), (dict(model_out=None), "model_out is null"),
                     (dict(n_img=0), "must be positive"), (dict(Hl=0), "must be positive"), (dict(Hl=5), "divisible by the patch size"),
                     (dict(p=0), "divisible by the patch size"), (dict(C=6), "multiple of 4"), (dict(ld_out=60), "ld_out"), (dict(ld_out=66), "ld_out"),
                     (dict(z=z + 4), "16-byte aligned"), (dict(zs_out=zs + 8), "16-byte aligned"), (dict(tokens=tok + 2), "8-byte aligned"),
                     (dict(model_out=out + 4), "8-byte aligned"), (dict(c=float("nan")), "must be finite"), (dict(w_src=float("inf")), "must be finite"),
                     (dict(sigma_in=float("nan")), "must be finite"), (dict(draw=-1), "draw must not be negative")):
        for fn in (lib.dk_flowedit_step, lib.dk_flowedit_step_f16):
            rc, msg = call(fn, **kw)
            assert rc != 0 and text in msg, (kw, msg)


def test_guidance_rows_refuses_bad_arguments():
    lib = _lib.load()
    g = (C.c_float * 2)(1.5, 5.5)
    assert lib.dk_mmdit_set_guidance_rows(None, g, 2) != 0 and b"null handle" in lib.dk_last_error()
    h = _mmdit_handle(lib, tiny_flux())  # (no guidance embedding: FLUX.1-schnell's preset)
    try:
        assert lib.dk_mmdit_set_guidance_rows(h, g, 2) != 0 and b"no guidance embedding" in lib.dk_last_error()
        assert lib.dk_mmdit_set_guidance_rows(h, None, 0) != 0 and b"no guidance embedding" in lib.dk_last_error()
    finally:
        lib.dk_mmdit_destroy(h)
    h = _mmdit_handle(lib, replace(tiny_flux(), guidance_embed=True))
    try:
        assert lib.dk_mmdit_set_guidance_rows(h, None, 0) == 0 and lib.dk_mmdit_set_guidance_rows(h, g, 0) == 0  # (unset is always accepted)
        assert lib.dk_mmdit_set_guidance_rows(h, g, 2) != 0 and b"dk_mmdit_prepare must precede" in lib.dk_last_error()
    finally:
        lib.dk_mmdit_destroy(h)


def test_guidance_rows_leave_the_workspace_alone():
    """the rows' scratch is borrowed from the QKV buffer while the table is computed: a configuration with the embedding asks for the bytes it
    always did (tests/test_abi_and_host.py pins the numbers), whether or not rows were ever (un)set"""
    lib = _lib.load()
    shape = (2, 8, 12, 20, 3)
    cfg = replace(tiny_flux(), guidance_embed=True)
    h, fresh = _mmdit_handle(lib, cfg), _mmdit_handle(lib, cfg)
    try:
        assert lib.dk_mmdit_set_guidance_rows(h, None, 0) == 0
        assert lib.dk_mmdit_workspace_bytes(h, *shape) == lib.dk_mmdit_workspace_bytes(fresh, *shape)
    finally:
        lib.dk_mmdit_destroy(h)
        lib.dk_mmdit_destroy(fresh)


# ---- 5. the closed loop on the oracle, at the shapes of the GPU pipeline tests -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loop_references(family, case, x_key=None):
    """{"fp32", "emu"} -> (Z, final latent) of tests/_flowedit.py's loop, from a synthetic x_src (the GPU tests start from the pipeline's encoded image)"""
    cfg, shift, cfgw, text, pooled = family_inputs(family)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    T, n_max, n_min, n_avg = case
    sigmas = op.get_sigmas(shift, cfg.is_flux, T)
    x_src = randn(1, fe.HL, fe.WL, 16, seed=21)
    src = fe.source_inputs(family)
    return x_src, {pname: fe.oracle_edit_loop(OracleMMDiT(cfg, wf, P), x_src, sigmas, n_max, n_min, n_avg, src, (text, pooled), fe.W_SRC, cfgw, Prec(BF),
                                              [fe.SEED], t_act_of(cfg)) for pname, P in (("fp32", Prec()), ("emu", Prec(BF)))}


@pytest.mark.parametrize("case", fe.LOOP_CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_oracle_loop_meets_the_gates_and_moves(family, case):
    """what the GPU pipeline tests rely on: the emulating oracle reaches 37 dB against the fp32 oracle at these shapes (so their 35 dB gate applies),
    and the edit moves the latent from x_src by more than ten times the yardstick gate, 2 err(emu) + 2e-3 -- an edit that did nothing would fail it"""
    x_src, res = loop_references(family, case)
    e_e, p_e = rel_l2(res["fp32"][1], res["emu"][1]), psnr(res["fp32"][1], res["emu"][1])
    n_min = case[2]
    moved = rel_l2(res["fp32"][0], x_src)  # Z against x_src (with n_min > 0 the final latent has been re-noised and sampled: Z is what the edit did)
    print(f"[flowedit] {family} {case}: emu-vs-fp32 rel_l2 {e_e:.3e}, PSNR {p_e:.1f} dB; |Z - x_src| / |Z| {moved:.3e}; gate {2 * e_e + 2e-3:.3e}")
    assert p_e >= 37.0
    assert moved > 10.0 * (2.0 * e_e + 2e-3)
    if n_min == 0:
        assert res["fp32"][0] is res["fp32"][1]  # (the result is Z)
