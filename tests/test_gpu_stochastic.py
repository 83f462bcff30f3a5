"""Stochastic samplers on an MI355X: the generator operator (dk_philox_normal_f32) against the float64 definition, the noise term of the step launch
(dk_noisy_cfg_step / _f16) against the operator bit for bit and against a float64 restatement in every case of the row kernel, cn = 0 against the old
launches, batch invariance, and the pipeline (``sampler="euler_a"`` / ``"sde"``) against the loop restated on the oracle in tests/_stochastic.py under
the project's model-level gates.  Every figure is printed before it is asserted.

Operator shapes: tests/test_gpu_samplers.py's (latent 8 x 12 x 16, p 2, two images) and tests/test_gpu_guidance.py's 6 x 10 x 16 with three images (960
elements per image: several workgroups, a ragged last one, images that straddle workgroups); pipeline shapes: tests/test_gpu_inpaint.py's."""
import functools

import numpy as np
import pytest
import torch

from diffusionkit_amd.sampler import FixedSchedule, StepRow, philox_normal_reference, stochastic_reference
from diffusionkit_amd.weights import synth_mmdit_weights
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec, embed_dtype
from tests import _footprint as fp
from tests import test_gpu_guidance as gg
from tests import test_gpu_samplers as gs
from tests._stochastic import N_MOMENTS, reference_loop
from tests._util import BF, max_abs, psnr, rel_l2
from tests.test_gpu_inpaint import HALF, HL, RGB, SEED, STEPS, WL, encoded, pipe_for, same_bits, tokens_of
from tests.test_gpu_samplers import sampled
from tests.test_gpu_slg import ALL_MODES, SLG, Operands3, live_tokens_ok
from tests.test_inpaint_cpu import FAMILIES, family_inputs, t_act_of
from tests.test_samplers_cpu import start_state

pytestmark = pytest.mark.gpu

F16 = torch.float16
SEEDS3 = (0, 1, (1 << 40) + 7)
SEEDS2 = (5, (1 << 63) + 11)  # (the second one has its top bit set: the seeds travel as the bits of an int64)
DRAW = 3
CN = float(np.float32(0.6))
# The generator against the float64 definition.  Measured on the first GPU run at N = 2^20: GENERATOR_MEASURED, at z = 3.96, where an fp32 ulp is
# 2.4e-7 (profiles/stochastic_samplers.md); the bound is four times that, because other boxes and compiler versions may round logf / sqrtf / sinpif /
# cospif differently.  A deviation above 1e-5 would not be rounding.
GENERATOR_MEASURED = 5.76e-7
GENERATOR_BOUND = 4.0 * GENERATOR_MEASURED


def seeds_on(dev, seeds):
    from diffusionkit_amd import ops
    return ops.seed_tensor(seeds, dev)


# ---- 1. the generator ---------------------------------------------------------------------------------------------------------------------------------
def test_generator(dev):
    """3 rows of 4 * 65 = 260 normals (no multiple of the workgroup): within the measured bound of the float64 reference; row j is the single-row call
    with seeds[j] bit for bit; quad_offset = 2^32 - 2 with 16 normals per row crosses into the counter's second word; another draw, stream or seed
    changes every quad"""
    from diffusionkit_amd import ops
    n = 260
    sd = seeds_on(dev, SEEDS3)
    z = ops.philox_normal(sd, n, DRAW)
    assert z.shape == (3, n) and z.dtype == torch.float32 and bool(torch.isfinite(z).all())
    ref = np.stack([philox_normal_reference(s, DRAW, n) for s in SEEDS3])
    e = float(np.abs(z.double().cpu().numpy() - ref).max())
    print(f"[stochastic] generator 3 x {n}: max_abs against the float64 reference {e:.2e} (bound {GENERATOR_BOUND:.2e})")
    assert e <= GENERATOR_BOUND
    for j, s in enumerate(SEEDS3):
        assert same_bits(ops.philox_normal(seeds_on(dev, [s]), n, DRAW), z[j:j + 1]), f"row {j} is not the single-row call"
    off = (1 << 32) - 2
    zo = ops.philox_normal(sd, 16, DRAW, 0, off)
    refo = np.stack([philox_normal_reference(s, DRAW, 16, 0, off) for s in SEEDS3])
    eo = float(np.abs(zo.double().cpu().numpy() - refo).max())
    print(f"[stochastic] generator at quad_offset 2^32 - 2: max_abs {eo:.2e}")
    assert eo <= GENERATOR_BOUND
    assert not same_bits(zo[:, 8:], ops.philox_normal(sd, 8, DRAW, 0, 0))  # (quads 2^32 and 2^32 + 1 are not quads 0 and 1)
    quads = lambda t: fp.bits(t).reshape(3, -1, 4)  # noqa: E731
    for what, other in (("draw", ops.philox_normal(sd, n, DRAW + 1)), ("stream", ops.philox_normal(sd, n, DRAW, 1)),
                        ("seed", ops.philox_normal(seeds_on(dev, [s + 1 for s in SEEDS3]), n, DRAW))):
        assert bool((quads(other) != quads(z)).any(dim=2).all()), f"another {what} leaves a quad as it was"


def test_generator_deviation(dev):
    """N = 2^20 normals of one seed: the largest deviation from the float64 reference, printed and held to four times the value first measured"""
    from diffusionkit_amd import ops
    z = ops.philox_normal(seeds_on(dev, [SEEDS3[2]]), N_MOMENTS, 0)
    ref = philox_normal_reference(SEEDS3[2], 0, N_MOMENTS)
    err = np.abs(z.double().cpu().numpy()[0] - ref)
    k = int(err.argmax())
    print(f"[stochastic] generator deviation at N = 2^20: max_abs {err.max():.3e} at element {k} (z = {ref[k]:.4f}), largest |z| {np.abs(ref).max():.3f}, "
          f"bound {GENERATOR_BOUND:.2e}")
    assert float(err.max()) <= GENERATOR_BOUND
    assert GENERATOR_BOUND <= 1e-5  # (anything above is not rounding)


# ---- 2. the fused noise is the operator's noise -----------------------------------------------------------------------------------------------------------
def noisy_step(o, coef, reads_h, writes_h, cn, seeds, draw=DRAW, mask=None, sigma_next=gs.SIGMA_NEXT, hist="own"):
    """tests/test_gpu_samplers.py's ``Operands.step`` through dk_noisy_cfg_step without the guidance groups: (x, tokens, hist)"""
    from diffusionkit_amd import ops
    x = o.x.to(o.dev)
    tok = torch.full((gs.N_IMG * o.dup, gs.S_I, gs.F), 7.0, dtype=o.dt, device=o.dev)
    h = o.hist.to(o.dev) if isinstance(hist, str) else hist
    kw = {} if mask is None else dict(x_orig=o.x_orig_d, noise=o.noise_d, mask=mask.to(o.dev))
    ops.noisy_cfg_step(x, o.out_d, tok, gs.N_IMG, o.cfg_on, gs.P_, o.order, gs.SIGMA, sigma_next, o.cfgw, h, coef, reads_h, writes_h, cn=cn, seeds=seeds,
                       draw=draw, **kw)
    return x, tok, h


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("order", [0, 1], ids=["sd3", "flux"])
def test_fused_noise_is_the_operators(dev, order, dt):
    """(cx, cd, cn) = (0, 0, 1): x' is ops.philox_normal's output bit for bit, up to the sign of a zero"""
    from diffusionkit_amd import ops
    o = gs.Operands(dev, order, 5.0, dt)
    sd = seeds_on(dev, SEEDS2)
    x, tok, _ = noisy_step(o, (0.0, 0.0, 0.0, 0.0, 0.0), False, False, 1.0, sd)
    xi = ops.philox_normal(sd, gs.Hl * gs.Wl * gs.C, DRAW).reshape(x.shape)
    differ = fp.bits(x) != fp.bits(xi)  # (allowed only between +0 and -0)
    assert bool(torch.isfinite(x).all()) and bool((x.cpu()[differ] == 0.0).all()) and bool((xi.cpu()[differ] == 0.0).all()), \
        f"{int(differ.sum())} elements differ from the operator's, beyond the sign of a zero"
    assert same_bits(tok, tokens_of(x, dt, gs.N_IMG, 2, gs.Hl, gs.Wl, gs.C, gs.P_, order))


# ---- 3. the fused step against float64 -----------------------------------------------------------------------------------------------------------------------
ROW = StepRow(0, gs.SIGMA, gs.SIGMA_NEXT, gs.COEF[0], gs.COEF[1], 0.0, 0.0, 0.0, False, False, True, CN, DRAW)


@gs.step_cases
def test_noisy_step_operator(dev, order, cfgw, dt, ld_pad):
    """a first-order row with cx, cd and cn all non-trivial: x' within 1e-5 of ``stochastic_reference`` fed the operator's normals, at unit-scale inputs
    (the bound of test_lms_step_operator); tokens == dk_latent_to_tokens(x'), both copies; the term is there"""
    from diffusionkit_amd import ops
    o = gs.Operands(dev, order, cfgw, dt, ld_pad)
    sd = seeds_on(dev, SEEDS2)
    x, tok, _ = noisy_step(o, (ROW.cx, ROW.cd, 0.0, 0.0, 0.0), False, False, ROW.cn, sd)
    xi = ops.philox_normal(sd, gs.Hl * gs.Wl * gs.C, DRAW).reshape(x.shape).double().cpu().numpy()
    d = o.ref64((0.0, 1.0, 0.0, 0.0, 0.0), False)[0].numpy()  # (d itself: the row (0, 1))
    x64 = o.x.double().numpy()
    ref = stochastic_reference(x64, x64 - gs.SIGMA * d, ROW, xi)
    e = float(np.abs(ref - x.double().cpu().numpy()).max())
    print(f"[stochastic] noisy step order={order} cfg={cfgw:g} {dt} ld+{ld_pad}: max_abs x' {e:.2e}")
    assert e < 1e-5
    assert same_bits(tok, tokens_of(x, dt, gs.N_IMG, o.dup, gs.Hl, gs.Wl, gs.C, gs.P_, order)), "tokens are not the patchified updated latent"
    if o.cfg_on:
        assert same_bits(tok[:gs.N_IMG], tok[gs.N_IMG:])
    assert not same_bits(x, o.step((ROW.cx, ROW.cd, 0.0, 0.0, 0.0), False, False)[0])
    assert not same_bits(x, noisy_step(o, (ROW.cx, ROW.cd, 0.0, 0.0, 0.0), False, False, ROW.cn, sd, draw=DRAW + 1)[0])


def step3(o, cn, seeds, mask=None, slg_scale=SLG, draw=DRAW, **mode):
    """tests/test_gpu_slg.py's ``Operands3.step3`` through dk_noisy_cfg_step with every group on: (x, tokens, hist, m)"""
    from diffusionkit_amd import ops
    x, h, mm = o.x.to(o.dev), o.hist.to(o.dev), o.m.to(o.dev)
    tok = torch.full((3 * gg.N_IMG, o.s_i, o.f), 7.0, dtype=o.dt, device=o.dev)
    kw = {} if mask is None else dict(x_orig=o.x_orig_d, noise=o.noise_d, mask=mask.to(o.dev))
    ops.noisy_cfg_step(x, o.out3_d, tok, gg.N_IMG, True, gg.P_, o.order, gg.SIGMA, gg.SIGMA_NEXT, gg.CFGW, h, gg.COEF, True, True, cn=cn, seeds=seeds,
                       draw=draw, guided=True, slg_scale=slg_scale, workspace=o.workspace(), reads_m=True, writes_m=True, m=mm, **mode, **kw)
    return x, tok, h, mm


@pytest.mark.parametrize("order", [0, 1], ids=["sd3", "flux"])
def test_noisy_step_ragged_and_composed(dev, order):
    """latent 6 x 10 x 16, three images at their own scales, fp16, with every other case of the kernel on at once: the history read and written,
    rescale guidance 0.7, the third row group of skip-layer guidance (scale 2.5) and a random per-image mask.
    Unmasked: x' within tests/test_gpu_slg.py's max(1e-5, 4 e32) of ``slg_reference``'s float64 row plus cn xi (the operator's normals), each image at
    its own scale.  Masked: within tests/test_gpu_inpaint.py's 4 * 2^-23 * max(|x'|, |noise|, |x_orig|) of the float64 blend of the unmasked launch's
    x'.  Tokens are the patchified result in the two live copies; H' does not see the noise."""
    from diffusionkit_amd import ops
    hl, wl = 6, 10
    o = Operands3(dev, order, F16, hl, wl)
    mode = ALL_MODES["rescale"]
    sd = seeds_on(dev, SEEDS3)
    x, tok, h, _ = step3(o, CN, sd, **mode)
    xi = ops.philox_normal(sd, hl * wl * gg.C, DRAW).reshape(x.shape).cpu()
    flags = dict(reads_h=True, reads_m=True, writes_m=True)
    rx, rh, _ = o.evaluate3(np.float64, gg.COEF, **flags, **mode)
    fx, _, _ = o.evaluate3(np.float32, gg.COEF, **flags, **mode)
    rx, fx = rx + CN * xi.double().numpy(), fx + np.float32(CN) * xi.numpy()
    e32, e = gg.own_scale_err(rx, fx), gg.own_scale_err(rx, x)
    bound = max(1e-5, 4.0 * e32)
    print(f"[stochastic] composed row order={order} f16 {hl}x{wl} unmasked: max_abs at own scale {e:.2e}, e32 {e32:.2e}, bound {bound:.2e}")
    assert e <= bound
    assert live_tokens_ok(tok, x, F16, hl, wl, order)
    assert same_bits(h, o.step3(**mode)[2]) and not same_bits(x, o.step3(**mode)[0])
    m = torch.rand(gg.N_IMG, hl, wl, generator=gg.gen(5))
    xm, tokm, hm, _ = step3(o, CN, sd, mask=m, **mode)
    xn, no, xo, mm = (t.double().cpu() for t in (x, o.noise, o.x_orig, m[..., None]))
    ref = mm * xn + (1.0 - mm) * (gg.SIGMA_NEXT * no + (1.0 - gg.SIGMA_NEXT) * xo)
    bnd = 4.0 * 2.0 ** -23 * torch.maximum(torch.maximum(xn.abs(), no.abs()), xo.abs())
    err = (xm.double().cpu() - ref).abs()
    print(f"[stochastic] composed row order={order} masked: largest |x - ref| / bound {float((err / bnd).max()):.3f}")
    assert bool((err <= bnd).all()) and not same_bits(xm, x)
    assert live_tokens_ok(tokm, xm, F16, hl, wl, order) and same_bits(hm, h)


# ---- 4. cn == 0 is the old launch ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,cfgw,dt", [(0, 5.0, BF), (1, 0.0, F16)], ids=["sd3-cfg-bf16", "flux-f16"])
def test_cn_zero_is_the_old_launch(dev, order, cfgw, dt):
    """the noisy entry with cn = 0 gives lms_cfg_step's / lms_cfg_step_masked's bits (x, tokens, H'); seeds -- a poison pattern between sentinel
    margins -- is not written, and no value of it can show: draw = -1 is accepted too"""
    o = gs.Operands(dev, order, cfgw, dt)
    for mask in (None, torch.rand(gs.N_IMG, gs.Hl, gs.Wl, generator=gs.gen(5))):
        poison, guard = fp.guarded(torch.full((gs.N_IMG,), 0x7FF8DEADBEEF7FF8, dtype=torch.int64, device=dev), 8, 0x0123456789ABCDEF)
        before = fp.bits(poison).clone()
        want = o.step(gs.COEF, True, True, mask=mask)
        got = noisy_step(o, gs.COEF, True, True, 0.0, poison, draw=-1, mask=mask)
        for name, a, b in zip(("x", "tokens", "H"), got, want):
            assert same_bits(a, b), f"{'masked' if mask is not None else 'plain'}: {name} differs from dk_lms_cfg_step's"
        assert torch.equal(fp.bits(poison), before)
        guard.check("seeds")
        assert all(same_bits(a, b) for a, b in zip(noisy_step(o, gs.COEF, True, True, 0.0, None, mask=mask), want))  # (seeds may be null)


def test_cn_zero_is_the_skip_layer_launch(dev):
    """... and with the guidance group and the third row group: dk_slg_cfg_step's bits in every mode"""
    o = Operands3(dev, 0, BF, 6, 10)
    for name, mode in ALL_MODES.items():
        want = o.step3(**mode)
        got = step3(o, 0.0, None, **mode)
        for tname, a, b in zip(("x", "tokens", "H", "M"), got, want):
            assert same_bits(a, b), f"{name}: {tname} differs from dk_slg_cfg_step's"


# ---- 5. batch invariance ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_batch_invariance_of_the_operator(dev, dt):
    """three images with three seeds in one launch (6 x 10 x 16: the images straddle workgroups) equal the three single-image launches bit for bit"""
    from diffusionkit_amd import ops
    hl, wl, n = 6, 10, gg.N_IMG
    o = gg.Operands(dev, 0, dt, hl, wl)
    coef = (ROW.cx, ROW.cd, 0.0, 0.0, 0.0)

    def run(imgs):
        k = len(imgs)
        x = o.x[imgs].to(dev).contiguous()
        out = torch.cat([o.out[imgs], o.out[[n + j for j in imgs]]]).to(dev).contiguous()
        tok = torch.full((2 * k, o.s_i, o.f), 7.0, dtype=dt, device=dev)
        ops.noisy_cfg_step(x, out, tok, k, True, gg.P_, 0, gg.SIGMA, gg.SIGMA_NEXT, gg.CFGW, None, coef, False, False, cn=CN,
                           seeds=seeds_on(dev, [SEEDS3[j] for j in imgs]), draw=DRAW)
        return x, tok
    x3, tok3 = run([0, 1, 2])
    for j in range(n):
        x1, tok1 = run([j])
        assert same_bits(x3[j:j + 1], x1), f"image {j} of the batch differs from its single launch"
        assert same_bits(tok3[[j, n + j]], tok1), f"tokens of image {j}"


@pytest.mark.parametrize("family", list(FAMILIES))
def test_batch_invariance_of_the_pipeline(dev, family):
    """seed = [2, 3, 4] under euler_a: each image equals its single-seed run bit for bit"""
    pipe = pipe_for(family, dev)
    three = sampled(pipe, family, dev, "euler_a", seed=[2, 3, 4])
    for i, s in enumerate((2, 3, 4)):
        one = sampled(pipe, family, dev, "euler_a", seed=s)
        print(f"[stochastic] {family} seed list: image {i} (seed {s}) against its single-seed run: max_abs {max_abs(three[i:i + 1], one):.3e}")
        assert same_bits(three[i:i + 1], one), f"image {i} of the seed list differs from the single-seed run"
    assert not same_bits(three[0:1], three[1:2])


# ---- 6. pipeline parity -----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loop_references(family, sampler):
    """the stochastic loop on the fp32 and the bf16-emulating oracle, after process_out"""
    cfg, shift, cfgw, text, pooled = family_inputs(family)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    sigmas = op.get_sigmas(shift, cfg.is_flux, STEPS)
    x0, _ = start_state(sigmas, SEED, HL, WL)
    return {pname: op.process_out(reference_loop(OracleMMDiT(cfg, wf, P), sampler, x0, sigmas, text, pooled, cfgw, Prec(BF), [SEED], t_act_of(cfg)),
                                  "flux" if cfg.is_flux else "sd3") for pname, P in (("fp32", Prec()), ("emu", Prec(BF)))}


@pytest.mark.parametrize("sampler", ["euler_a", "sde"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_pipeline_parity(dev, family, sampler):
    """tiny FLUX and tiny SD3 + CFG 5 against the loop of tests/_stochastic.py on the fp32 oracle, its noise from ``philox_normal_reference``: the gates
    tests/test_gpu_samplers.py applies to ab2 -- err(hip) <= 2 err(bf16-emulating oracle) + 2e-3, and 35 dB where the emulating oracle reaches 37 dB"""
    from tests.test_gpu_model import yardstick_ok
    pipe = pipe_for(family, dev)
    lat = sampled(pipe, family, dev, sampler)
    assert pipe.last_sampler == {"sampler": sampler, "model_evals": STEPS, "eta": 1.0 if sampler == "euler_a" else None, "noise_draws": STEPS - 1}
    res = loop_references(family, sampler)
    p_h, p_e = psnr(res["fp32"], lat), psnr(res["fp32"], res["emu"])
    print(f"[stochastic] {family} {sampler}: rel_l2 hip {rel_l2(res['fp32'], lat):.3e} / emu {rel_l2(res['fp32'], res['emu']):.3e}, "
          f"PSNR hip {p_h:.1f} dB / emu {p_e:.1f} dB")
    yardstick_ok(lat, res["emu"], res["fp32"], f"{family} {sampler}")
    if p_e >= 37.0:
        assert p_h > 35.0, f"{family} {sampler}: PSNR {p_h:.1f} dB"
    assert not same_bits(lat, sampled(pipe, family, dev, "euler"))
    assert same_bits(lat, sampled(pipe, family, dev, sampler))  # (the same seed: the same bits)


def test_pipeline_parity_f16(dev):
    """activation_dtype = "float16", SD3 + CFG 5, euler_a: the gates of tests/test_gpu_f16_model.py's pipeline test"""
    from tests.test_gpu_f16_model import f16_weights, gate
    family = "sd3_cfg"
    pipe = pipe_for(family, dev, f16=True)
    assert pipe.mmdit.dtype == F16
    lat = sampled(pipe, family, dev, "euler_a")
    cfg, shift, cfgw, text, pooled = family_inputs(family)
    _, wf = f16_weights(cfg)
    sigmas = op.get_sigmas(shift, False, STEPS)
    x0, _ = start_state(sigmas, SEED, HL, WL)
    res = {}
    for oname, (m, act) in {"fp32": (OracleMMDiT(cfg, wf, Prec(), embed_prec=Prec(embed_dtype(cfg))), Prec(F16)),
                            "emu16": (OracleMMDiT(cfg, wf, Prec(F16)), Prec(F16)), "emubf": (OracleMMDiT(cfg, wf, Prec(BF)), Prec(BF))}.items():
        res[oname] = op.process_out(reference_loop(m, "euler_a", x0, sigmas, text, pooled, cfgw, act, [SEED], t_act=Prec(F16)), "sd3")
    gate(lat, res["emu16"], res["emubf"], res["fp32"], "euler_a f16")


# ---- 7. compositions ---------------------------------------------------------------------------------------------------------------------------------------------
def recorded(monkeypatch):
    """the noisy launches of the calls that follow: [(cfg_on, draw, cn)]"""
    from diffusionkit_amd import ops
    calls, real = [], ops.noisy_cfg_step

    def spy(*a, **k):
        calls.append((bool(a[4]), k["draw"], k["cn"]))
        return real(*a, **k)
    monkeypatch.setattr(ops, "noisy_cfg_step", spy)
    return calls


def test_half_mask_inpainting(dev):
    """right-half mask on tiny FLUX under euler_a: the kept half is the encoded image bit for bit (the blend re-noises the known region with the start
    draw, whatever the step drew), the repainted half moves; an all-0 mask returns the encoded image"""
    pipe = pipe_for("flux", dev)
    lat = sampled(pipe, "flux", dev, "euler_a", image_path=RGB, denoise=1.0, mask_path=HALF)
    _, kept = encoded(pipe)
    assert same_bits(lat[:, :, :WL // 2], kept[:, :, :WL // 2])
    assert not same_bits(lat[:, :, WL // 2:], kept[:, :, WL // 2:]) and bool(torch.isfinite(lat).all())
    assert not same_bits(lat[:, :, WL // 2:], sampled(pipe, "flux", dev, "euler", image_path=RGB, denoise=1.0, mask_path=HALF)[:, :, WL // 2:])
    assert same_bits(sampled(pipe, "flux", dev, "euler_a", image_path=RGB, denoise=1.0, mask_path=np.zeros_like(HALF)), kept)


def test_img2img_cut_schedule(dev, monkeypatch):
    """denoise 0.5 of 4 steps under sde: the two remaining steps, the first with the draw of the entry it keeps (2), the last -- to sigma = 0 -- an
    Euler row"""
    pipe = pipe_for("flux", dev)
    calls = recorded(monkeypatch)
    cfg, _, cfgw, text, pooled = family_inputs("flux")
    outs = {}
    for sampler in ("euler", "sde"):
        lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=STEPS, cfg_weight=cfgw, latent_size=(HL, WL), seed=SEED,
                                              image_path=RGB, denoise=0.5, sampler=sampler)
        assert len(iter_time) == 2 and bool(torch.isfinite(lat).all())
        outs[sampler] = lat
    assert pipe.last_sampler == {"sampler": "sde", "model_evals": 2, "eta": None, "noise_draws": 1}
    assert [(c[0], c[1]) for c in calls] == [(False, 2)] and not same_bits(outs["sde"], outs["euler"])


def test_block_cache(dev):
    """sde with FixedSchedule({1}) runs and records one skip; a policy that never skips gives the plain run's bits"""
    pipe = pipe_for("flux", dev)
    plain = sampled(pipe, "flux", dev, "sde")
    lat = sampled(pipe, "flux", dev, "sde", block_cache=FixedSchedule({1}))
    rec = pipe.last_block_cache
    print(f"[stochastic] sde + FixedSchedule({{1}}): {rec}")
    assert rec["skipped"] == [1] and rec["computed"] == [0, 2, 3] and bool(torch.isfinite(lat).all()) and not same_bits(lat, plain)
    assert same_bits(sampled(pipe, "flux", dev, "sde", block_cache=0.0), plain)


def test_guidance_interval(dev, monkeypatch):
    """SD3 + CFG 5 under euler_a with guidance on sigma in [0.3, 0.8]: the rows outside it run -- and draw -- on the prompt rows alone"""
    pipe = pipe_for("sd3_cfg", dev)
    calls = recorded(monkeypatch)
    lat = sampled(pipe, "sd3_cfg", dev, "euler_a", guidance_interval=(0.3, 0.8))
    g = pipe.last_guidance
    print(f"[stochastic] euler_a + guidance_interval (0.3, 0.8): {g}; noisy launches {calls}")
    assert bool(torch.isfinite(lat).all()) and g["guided_evals"] + g["unguided_evals"] == STEPS and g["guided_evals"] > 0 and g["unguided_evals"] > 0
    assert [c[1] for c in calls] == list(range(STEPS - 1)) and {c[0] for c in calls} == {True, False}
    assert not same_bits(lat, sampled(pipe, "sd3_cfg", dev, "euler_a"))


def test_generate_image_and_refusals(dev):
    """generate_image logs what ran; sampler_eta reaches the plan; sampler_eta with another sampler, or outside [0, 1], raises"""
    pipe = pipe_for("flux", dev)
    img, log = pipe.generate_image("a cat", num_steps=STEPS, latent_size=(HL, WL), seed=SEED, verbose=False, sampler="euler_a", sampler_eta=0.5)
    d = log["denoising"]
    assert (d["sampler"], d["model_evals"], d["eta"], d["noise_draws"]) == ("euler_a", STEPS, 0.5, STEPS - 1) and len(d["iter_time"]) == STEPS
    half, full = sampled(pipe, "flux", dev, "euler_a", sampler_eta=0.5), sampled(pipe, "flux", dev, "euler_a")
    assert not same_bits(half, full) and same_bits(full, sampled(pipe, "flux", dev, "euler_a", sampler_eta=1.0))
    for sampler in ("heun", "sde", None):
        with pytest.raises(ValueError, match="euler_a"):
            sampled(pipe, "flux", dev, sampler, sampler_eta=0.5)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        sampled(pipe, "flux", dev, "euler_a", sampler_eta=1.5)


# ---- 8. the default is untouched --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_default_is_untouched(dev, family, monkeypatch):
    """sampler=None, "euler" and the call without the keyword: bit-identical latents and no launch of the new entries; euler_a with eta = 0 is that
    run too, launch for launch"""
    from diffusionkit_amd import ops
    pipe = pipe_for(family, dev)
    calls = []
    for name in ("noisy_cfg_step", "philox_normal", "seed_tensor", "lms_cfg_step", "lms_cfg_step_masked"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    omitted = sampled(pipe, family, dev, "omit")
    assert same_bits(sampled(pipe, family, dev, None), omitted) and same_bits(sampled(pipe, family, dev, "euler"), omitted)
    assert pipe.last_sampler == {"sampler": "euler", "model_evals": STEPS}
    assert same_bits(sampled(pipe, family, dev, "euler_a", sampler_eta=0.0), omitted)
    assert pipe.last_sampler == {"sampler": "euler_a", "model_evals": STEPS, "eta": 0.0, "noise_draws": 0}
    masked = sampled(pipe, family, dev, "omit", image_path=RGB, denoise=1.0, mask_path=HALF)
    assert same_bits(sampled(pipe, family, dev, "euler_a", sampler_eta=0.0, image_path=RGB, denoise=1.0, mask_path=HALF), masked)
    assert calls == []


# ---- 9. refused arguments ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """a non-finite cn, cn != 0 without seeds or with a negative draw, a latent whose size is no multiple of 4, a mode without the guidance group, seeds
    of the wrong kind; the operator's n_per_img: dk_last_error's text, and nothing written"""
    from diffusionkit_amd import _lib, ops
    from diffusionkit_amd._lib import DkHipError
    o = gs.Operands(dev, 1, 0.0, BF)
    x, tok, hist = o.x.to(dev), torch.full((gs.N_IMG, gs.S_I, gs.F), 7.0, dtype=BF, device=dev), o.hist.to(dev)
    head = (x, o.out_d, tok, gs.N_IMG, False, gs.P_, 1, gs.SIGMA, gs.SIGMA_NEXT, 0.0, hist, gs.COEF, True, True)
    sd = seeds_on(dev, SEEDS2)
    for bad in (fp.NAN, float("inf")):
        with pytest.raises(DkHipError, match="cn must be finite"):
            ops.noisy_cfg_step(*head, cn=bad, seeds=sd, draw=0)
    with pytest.raises(DkHipError, match="seeds is null"):
        ops.noisy_cfg_step(*head, cn=0.5, seeds=None, draw=0)
    with pytest.raises(DkHipError, match="draw"):
        ops.noisy_cfg_step(*head, cn=0.5, seeds=sd, draw=-1)
    with pytest.raises(DkHipError, match="mode 0"):
        ops.noisy_cfg_step(*head, cn=0.5, seeds=sd, draw=0, mode="rescale")
    with pytest.raises(DkHipError, match="cfg_on"):
        ops.noisy_cfg_step(*head, cn=0.5, seeds=sd, draw=0, guided=True, mode="rescale")
    with pytest.raises(DkHipError, match="seeds"):
        ops.noisy_cfg_step(*head, cn=0.5, seeds=sd[:1], draw=0)
    with pytest.raises(DkHipError, match="seeds"):
        ops.noisy_cfg_step(*head, cn=0.5, seeds=sd.to(torch.float64), draw=0)
    xo = torch.zeros(1, 1, 2, 3, device=dev)  # 1 x 2 x 3 = 6 elements per image, p = 1
    with pytest.raises(DkHipError, match="multiple of 4"):
        ops.noisy_cfg_step(xo, torch.zeros(1, 2, 3, dtype=BF, device=dev), torch.zeros(1, 2, 3, dtype=BF, device=dev), 1, False, 1, 1, gs.SIGMA,
                           gs.SIGMA_NEXT, 0.0, None, gs.COEF, False, False, cn=0.5, seeds=sd[:1], draw=0)
    with pytest.raises(DkHipError, match="multiple of 4"):
        ops.philox_normal(sd, 6, 0)
    with pytest.raises(DkHipError, match="negative"):
        ops.philox_normal(sd, 8, -1)
    with pytest.raises(ValueError, match="2\\^64"):
        ops.seed_tensor([-1], dev)
    lib = _lib.load()
    rc = lib.dk_philox_normal_f32(x.data_ptr(), None, 1, 8, 0, 0, 0, None)
    assert rc != 0 and b"null" in lib.dk_last_error()
    torch.cuda.synchronize(dev)
    assert same_bits(x, o.x) and same_bits(hist, o.hist) and bool((tok == 7.0).all()) and bool((xo == 0.0).all()), "a refused call wrote something"
