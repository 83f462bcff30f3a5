"""Guidance modes on an MI355X: dk_guided_cfg_step (per-image moments, then the coefficient-row step) against ``sampler.guide_reference`` and against
dk_lms_cfg_step bit for bit, its run-to-run bits, momentum discipline, masked ends and refusals, and the pipeline (``guidance=``, ``guidance_interval=``)
against the guided loops restated on the oracle in tests/test_guidance_cpu.py, under the project's model-level gates.  Every figure is printed before
it is asserted.

Operator shapes: latent 8 x 12 x 16 (tests/test_gpu_samplers.py's: 1536 elements per image, two moment workgroups per image) and 6 x 10 x 16 (960
elements per image: no multiple of 256, a flat grid would straddle images), p 2, THREE images with image k scaled by 10^k and its negative prediction
at its own distance from the prompt's, so that s, a and b all differ between the images by far more than any tolerance.  Pipeline shapes:
tests/test_gpu_inpaint.py's (latent 8 x 16, 4 steps, seed 2).  The file name sorts behind tests/test_gpu_fullsize.py like tests/test_gpu_samplers.py."""
import functools

import numpy as np
import pytest
import torch

from diffusionkit_amd.config import tiny_sd3, tiny_flux, tiny_vae, tiny_vae_encoder
from diffusionkit_amd.sampler import FixedSchedule, guide_reference
from diffusionkit_amd.weights import synth_mmdit_weights, synth_vae_encoder_weights
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec, embed_dtype
from oracle.vae import OracleVAEEncoder
from tests import _footprint as fp
from tests._util import BF, max_abs, psnr, rel_l2
from tests.test_gpu_inpaint import (H_IMG, HALF, HL, RGB, SEED, STEPS, W_IMG, WL, encoded, half_mask_gates, pipe_for, same_bits, tokens_of)
from tests.test_guidance_cpu import APG, guided_loop
from tests.test_inpaint_cpu import FAMILIES, family_inputs, latent_mask, t_act_of
from tests.test_samplers_cpu import start_state

pytestmark = pytest.mark.gpu

F16 = torch.float16
N_IMG, C, P_ = 3, 16, 2
SHAPES = [(8, 12), (6, 10)]
SIGMA, SIGMA_NEXT, CFGW = float(np.float32(0.8)), float(np.float32(0.3)), 5.0
COEF = tuple(float(np.float32(v)) for v in (0.9, -0.3, 0.45, 0.25, 0.75))  # tests/test_gpu_samplers.py's arbitrary row
EULER = (1.0, float(np.float32(SIGMA_NEXT) - np.float32(SIGMA)), 0.0, 0.0, 0.0)
GAPS = (0.2, 0.6, 1.0)  # distance of the negative prediction from the prompt's, per image
SCALE = torch.tensor([1.0, 10.0, 100.0]).reshape(N_IMG, 1, 1, 1)
R_ON = 20.0  # |D| is about 6 / 190 / 3100 for the three images: a = 1 for image 0, clipped for the others
MODES = {"rescale": dict(mode="rescale", rescale=0.7),
         "apg": dict(mode="apg", eta=0.0, norm_threshold=0.0, momentum=-0.5),
         "apg-r": dict(mode="apg", eta=0.0, norm_threshold=R_ON, momentum=-0.5)}


def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def where_of(order, hl, wl):
    """[N_IMG, S_I, F] -> which latent element each token feature is, taken from the oracle's patchify on a tensor of element indices"""
    f = P_ * P_ * C
    orc = OracleMMDiT(tiny_flux() if order else tiny_sd3(),
                      {"x_embedder.proj.weight": torch.eye(f).reshape(f, *((1, 1, f) if order else (P_, P_, C))), "x_embedder.proj.bias": torch.zeros(f)}, Prec())
    index = torch.arange(N_IMG * hl * wl * C, dtype=torch.float32).reshape(N_IMG, hl, wl, C)
    where = orc._patch_embed(index).long()
    assert torch.equal(torch.sort(where.reshape(-1))[0], torch.arange(index.numel()))
    return where


class Operands:
    """seeded operands of one launch; ``step`` runs it on fresh copies and returns (x, tokens, hist, m)"""

    def __init__(self, dev, order, dt, hl=8, wl=12, ld_pad=0):
        self.dev, self.order, self.dt, self.hl, self.wl = dev, order, dt, hl, wl
        self.s_i, self.f = (hl // P_) * (wl // P_), P_ * P_ * C
        shape = (N_IMG, hl, wl, C)
        self.x = torch.randn(*shape, generator=gen(1)) * SCALE
        text = torch.randn(N_IMG, self.s_i, self.f + ld_pad, generator=gen(2))
        neg = text + torch.randn(N_IMG, self.s_i, self.f + ld_pad, generator=gen(7)) * torch.tensor(GAPS).reshape(N_IMG, 1, 1)
        self.out = (torch.cat([text, neg]) * torch.cat([SCALE, SCALE]).reshape(2 * N_IMG, 1, 1)).to(dt)
        self.hist = torch.randn(*shape, generator=gen(6)) * SCALE
        self.m = torch.randn(*shape, generator=gen(8)) * SCALE * 0.3
        self.x_orig = (torch.randn(*shape, generator=gen(3)) * 1.5 + 0.3) * SCALE
        self.noise = torch.randn(*shape, generator=gen(4)) * SCALE
        self.out_d, self.x_orig_d, self.noise_d = self.out.to(dev), self.x_orig.to(dev), self.noise.to(dev)

    def workspace(self, fill=None):
        from diffusionkit_amd import ops
        n = ops.guidance_workspace_bytes(N_IMG, self.hl, self.wl, C)
        assert n > 0 and n % 4 == 0
        return torch.empty(n // 4, dtype=torch.float32, device=self.dev) if fill is None else torch.full((n // 4,), fill, device=self.dev)

    def step(self, coef=COEF, reads_h=True, writes_h=True, mask=None, sigma_next=SIGMA_NEXT, reads_m=True, writes_m=True, m="own", ws=None,
             plain=False, **mode):
        from diffusionkit_amd import ops
        x, h = self.x.to(self.dev), self.hist.to(self.dev)
        tok = torch.full((2 * N_IMG, self.s_i, self.f), 7.0, dtype=self.dt, device=self.dev)
        mm = self.m.to(self.dev) if isinstance(m, str) else m
        head = (x, self.out_d, tok, N_IMG, True, P_, self.order, SIGMA, sigma_next, CFGW, h, coef, reads_h, writes_h)
        if plain:
            if mask is None:
                ops.lms_cfg_step(*head)
            else:
                ops.lms_cfg_step_masked(*head, self.x_orig_d, self.noise_d, mask.to(self.dev))
        else:
            kw = {} if mask is None else dict(x_orig=self.x_orig_d, noise=self.noise_d, mask=mask.to(self.dev))
            ops.guided_cfg_step(*head, workspace=self.workspace() if ws is None else ws, reads_m=reads_m, writes_m=writes_m, m=mm, **mode, **kw)
        return x, tok, h, mm

    def predictions(self, ft):
        """(x, c, u) as ``ft`` arrays: the latent and the two x0 predictions formed from the 16-bit model output and the rounded latent"""
        where = where_of(self.order, self.hl, self.wl)
        n = N_IMG * self.hl * self.wl * C
        o = torch.empty(2 * n, dtype=torch.float64)
        o[torch.cat([where, where + n]).reshape(-1)] = self.out[:, :, :self.f].double().reshape(-1)  # (unpatchify, per CFG copy)
        o = o.reshape(2 * N_IMG, self.hl, self.wl, C).numpy().astype(ft)
        x, xb = self.x.numpy().astype(ft), self.x.to(self.dt).float().numpy().astype(ft)
        sg = ft(SIGMA)
        return x, xb - o[:N_IMG] * sg, xb - o[N_IMG:] * sg

    def evaluate(self, ft, coef, reads_h, reads_m, writes_m, mode, rescale=0.0, eta=0.0, norm_threshold=0.0, momentum=0.0):
        """(x', H', M') in ``ft``: float64 through ``guide_reference``; float32 through the same formulas in numpy float32 with float64 sums"""
        x, c, u = self.predictions(ft)
        m = self.m.numpy().astype(ft)
        if ft is np.float64:
            den, m_new = guide_reference(c, u, CFGW, mode, rescale=rescale, eta=eta, norm_threshold=norm_threshold, momentum=momentum, m=m,
                                         reads_m=reads_m, writes_m=writes_m)
        else:
            den, m_new = guide_f32(c, u, CFGW, mode, rescale, eta, norm_threshold, momentum, m, reads_m, writes_m)
        cx, cd, ch, hx, hd = (ft(v) for v in coef)
        d = (x - den) / ft(SIGMA)
        xn = cx * x + cd * d + (ch * self.hist.numpy().astype(ft) if reads_h else ft(0.0))
        return xn, hx * x + hd * d, m_new


def guide_f32(c, u, w, mode, phi, eta, r, beta, m, reads_m, writes_m):
    """``guide_reference``'s formulas on float32 arrays: every elementwise operation in float32, every per-image sum (and the scalar it ends in) in
    float64, the scalar rounded to float32 once"""
    f, ax = np.float32, (1, 2, 3)
    per = lambda v: v.astype(f).reshape(-1, 1, 1, 1)  # noqa: E731
    if mode == "rescale":
        g = u + f(w) * (c - u)
        s = phi * c.astype(np.float64).std(axis=ax) / g.astype(np.float64).std(axis=ax) + (1.0 - phi)
        return g * per(s), m
    delta = (c - u) + f(beta) * m if reads_m else c - u
    d64, c64 = delta.astype(np.float64), c.astype(np.float64)
    nd = np.sqrt((d64 * d64).sum(axis=ax))
    a = np.minimum(1.0, r / nd) if r > 0 else np.ones_like(nd)
    b = (1.0 - eta) * a * (d64 * c64).sum(axis=ax) / (c64 * c64).sum(axis=ax)
    return c + f(w - 1.0) * (per(a) * delta - per(b) * c), (delta if writes_m else m)


def own_scale_err(ref, got):
    """largest |ref - got| over the images, each divided by its scale 10^k"""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else got.astype(np.float64)
    return float((np.abs(ref - got) / SCALE.numpy()).max())


CASES = [(order, dt, hl, wl, 0) for order in (0, 1) for dt in (BF, F16) for hl, wl in SHAPES] + [(1, BF, 8, 12, 8)]
cases = pytest.mark.parametrize("order,dt,hl,wl,ld_pad", CASES,
                                ids=[f"order{o}-{'bf16' if d == BF else 'f16'}-{h}x{w}-ld+{l}" for o, d, h, w, l in CASES])


# ---- 1. the operator against guide_reference ---------------------------------------------------------------------------------------------------------
@cases
def test_guided_step_operator(dev, order, dt, hl, wl, ld_pad):
    """rescale 0.7 and apg (eta 0, beta -0.5, threshold off and on), M read and written, on x', H' and M': within max(1e-5, 4 e32) of
    guide_reference's float64 result, each image at its own scale -- e32 = the error of the float32 numpy evaluation of the same formulas (float64
    sums) on the same operands, the factor 4 for the kernel's fp32 lane sums and FMA contraction.  Tokens == dk_latent_to_tokens(x'), both copies."""
    o = Operands(dev, order, dt, hl, wl, ld_pad)
    for name, mode in MODES.items():
        x, tok, h, m = o.step(**mode)
        flags = dict(reads_h=True, reads_m=True, writes_m=True)
        rx, rh, rm = o.evaluate(np.float64, COEF, **flags, **mode)
        fx, fh, fm = o.evaluate(np.float32, COEF, **flags, **mode)
        for what, ref, f32, got in (("x'", rx, fx, x), ("H'", rh, fh, h)) + ((("M'", rm, fm, m),) if mode["mode"] == "apg" else ()):
            e32, e = own_scale_err(ref, f32), own_scale_err(ref, got)
            bound = max(1e-5, 4.0 * e32)
            print(f"[guidance] {name} order={order} {dt} {hl}x{wl} ld+{ld_pad} {what}: max_abs at own scale {e:.2e}, e32 {e32:.2e}, bound {bound:.2e}")
            assert e <= bound, f"{name} {what}: {e:.3e} > {bound:.3e}"
        if mode["mode"] != "apg":
            assert same_bits(m, o.m), "rescale touched M"
        assert same_bits(tok, tokens_of(x, dt, N_IMG, 2, hl, wl, C, P_, order)), "tokens are not the patchified updated latent"
        assert same_bits(tok[:N_IMG], tok[N_IMG:])
    # the modes are not each other, nor cfg
    plain = o.step(plain=True)[0]
    xs = [o.step(**mode)[0] for mode in MODES.values()]
    assert not any(same_bits(a, plain) for a in xs) and not same_bits(xs[0], xs[1]) and not same_bits(xs[1], xs[2])


# ---- 2. rescale at phi = 0 is dk_lms_cfg_step, bit for bit -----------------------------------------------------------------------------------------------
@cases
def test_rescale_zero_is_the_cfg_step(dev, order, dt, hl, wl, ld_pad):
    """s == 1.0f: x, tokens and H' of ops.lms_cfg_step / _masked, for the arbitrary row and the Euler row"""
    o = Operands(dev, order, dt, hl, wl, ld_pad)
    for mask in (None, torch.rand(N_IMG, hl, wl, generator=gen(5))):
        for coef, reads_h, writes_h in ((COEF, True, True), (EULER, False, False)):
            want = o.step(coef, reads_h, writes_h, mask=mask, plain=True)
            got = o.step(coef, reads_h, writes_h, mask=mask, mode="rescale", rescale=0.0)
            what = f"{'masked' if mask is not None else 'plain'} {'euler' if coef is EULER else 'arbitrary'} row"
            for name, a, b in zip(("x", "tokens", "H"), got, want):
                assert same_bits(a, b), f"{what}: {name} differs from dk_lms_cfg_step's in {int((fp.bits(a) != fp.bits(b)).sum())} elements"
    x_mode0 = o.step(mode="cfg", ws=torch.empty(0, device=dev))  # (mode 0 is the cfg step itself: no workspace)
    assert all(same_bits(a, b) for a, b in zip(x_mode0[:3], o.step(plain=True)[:3]))


# ---- 3. the same bits on every run; nothing is read before it is written ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("hl,wl", SHAPES, ids=["8x12", "6x10"])
def test_same_bits_every_run(dev, name, hl, wl):
    """two runs, and a run whose exact-size workspace (between sentinel margins) and unread M were filled with NaN"""
    o = Operands(dev, 0, BF, hl, wl)
    mode = MODES[name]
    first, second = o.step(reads_m=False, **mode), o.step(reads_m=False, **mode)
    ws, guard = fp.guarded(o.workspace(fp.NAN), 1, fp.SENTINEL)
    m_nan, m_guard = fp.guarded(torch.full((N_IMG, hl, wl, C), fp.NAN, device=dev), 8, fp.SENTINEL)
    third = o.step(reads_m=False, ws=ws, m=m_nan, **mode)
    guard.check("workspace")
    m_guard.check("M")
    for what, run in (("second run", second), ("NaN-filled workspace and M", third)):
        for tname, a, b in zip(("x", "tokens", "H", "M"), run, first):
            if tname == "M" and mode["mode"] != "apg":
                continue  # (rescale leaves M alone: the NaN fill is still there)
            assert bool(torch.isfinite(a.float()).all()), f"{what}: {tname} holds non-finite values"
            assert same_bits(a, b), f"{what}: {tname} differs in {int((fp.bits(a) != fp.bits(b)).sum())} elements"


# ---- 4. momentum discipline -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1], ids=["sd3", "flux"])
def test_momentum_discipline(dev, order):
    o = Operands(dev, order, BF)
    mode = MODES["apg-r"]
    nan_m = lambda: torch.full((N_IMG, 8, 12, C), fp.NAN, device=dev)  # noqa: E731
    # reads_m off: a NaN-filled M is never read, and the row leaves a finite one
    x, tok, h, m = o.step(reads_m=False, writes_m=True, m=nan_m(), **mode)
    assert all(bool(torch.isfinite(t.float()).all()) for t in (x, tok, h, m))
    # ... and what it leaves is c - u: the next row's momentum
    _, c, u = o.predictions(np.float64)
    e = own_scale_err(c - u, m)
    print(f"[guidance] M' with reads_m off against c - u: max_abs at own scale {e:.2e}")
    assert e < 1e-5
    # writes_m off: M stays byte for byte, and with both off a null M is accepted
    x1, _, _, m = o.step(reads_m=True, writes_m=False, **mode)
    assert same_bits(m, o.m)
    x0, _, _, _ = o.step(reads_m=False, writes_m=False, m=None, **mode)
    assert bool(torch.isfinite(x0).all()) and not same_bits(x0, x1)  # (the momentum term is there)
    # one NaN in M under reads_m reaches every element of its image (through the moments) and none of the others
    poisoned = o.m.clone()
    poisoned[1, 5, 7, 9] = fp.NAN
    xp = o.step(reads_m=True, writes_m=False, m=poisoned.to(dev), **mode)[0]
    assert bool(torch.isnan(xp[1]).all()) and same_bits(xp[0], x1[0]) and same_bits(xp[2], x1[2])


# ---- 5. masked ends ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rescale", "apg-r"])
@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_masked_ends(dev, name, dt):
    """m = 1: the unmasked guided launch bit for bit (x, tokens, H', M'); m = 0 with sigma_next = 0: the known region, x_orig, bit for bit"""
    o = Operands(dev, 0, dt, 6, 10)
    mode = MODES[name]
    plain = o.step(**mode)
    ones = o.step(mask=torch.ones(1, 6, 10), **mode)
    for tname, a, b in zip(("x", "tokens", "H", "M"), ones, plain):
        assert same_bits(a, b), f"a mask of ones is not the unmasked launch: {tname}"
    x, tok, h, m = o.step(mask=torch.zeros(N_IMG, 6, 10), sigma_next=0.0, **mode)
    assert same_bits(x, o.x_orig), "m = 0 with sigma_next = 0 does not return x_orig"
    assert same_bits(tok, tokens_of(o.x_orig_d, dt, N_IMG, 2, 6, 10, C, P_, 0))
    assert same_bits(h, plain[2]) and same_bits(m, plain[3])  # (H' and M' do not see the mask)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """cfg_on == 0, phi outside [0, 1], non-finite parameters, a null M under a flag, a short workspace: dk_last_error, and nothing written"""
    from diffusionkit_amd import ops
    from diffusionkit_amd._lib import DkHipError
    o = Operands(dev, 1, BF)
    x, h, m = o.x.to(dev), o.hist.to(dev), o.m.to(dev)
    tok = torch.full((2 * N_IMG, o.s_i, o.f), 7.0, dtype=BF, device=dev)
    ws = o.workspace(0.0)
    head = lambda cfg_on=True: (x, o.out_d, tok, N_IMG, cfg_on, P_, 1, SIGMA, SIGMA_NEXT, CFGW, h, COEF, True, True)  # noqa: E731
    apg = dict(mode="apg", momentum=-0.5, m=m, reads_m=True, writes_m=True, workspace=ws)
    with pytest.raises(DkHipError, match="cfg_on"):
        ops.guided_cfg_step(*head(False), **apg)
    for phi in (-0.01, 1.01, fp.NAN):
        with pytest.raises(DkHipError, match=r"phi|finite"):
            ops.guided_cfg_step(*head(), mode="rescale", rescale=phi, workspace=ws)
    for key in ("eta", "norm_threshold", "momentum"):
        for bad in (fp.NAN, float("inf")):
            with pytest.raises(DkHipError, match="finite"):
                ops.guided_cfg_step(*head(), **dict(apg, **{key: bad}))
    for flags in (dict(reads_m=True, writes_m=False), dict(reads_m=False, writes_m=True)):
        with pytest.raises(DkHipError, match="momentum buffer"):
            ops.guided_cfg_step(*head(), **dict(apg, m=None, **flags))
    for short in (None, ws[:-1], torch.empty(0, device=dev)):
        for mode in (dict(mode="rescale", rescale=0.7, workspace=short), dict(apg, workspace=short)):
            with pytest.raises(DkHipError, match="workspace"):
                ops.guided_cfg_step(*head(), **mode)
    with pytest.raises(ValueError, match="cfg, rescale, apg"):
        ops.guided_cfg_step(*head(), mode="cads", workspace=ws)
    with pytest.raises(DkHipError, match="mask"):
        ops.guided_cfg_step(*head(), mode="rescale", workspace=ws, x_orig=o.x_orig_d, noise=o.noise_d)
    torch.cuda.synchronize(dev)
    assert same_bits(x, o.x) and same_bits(h, o.hist) and same_bits(m, o.m) and bool((tok == 7.0).all()) and bool((ws == 0.0).all()), \
        "a refused call wrote something"


# ---- 7. pipeline parity ---------------------------------------------------------------------------------------------------------------------------------
FAMILY = "sd3_cfg"
SETTINGS = {"rescale": dict(guidance="rescale"),
            "apg": dict(guidance="apg", apg_momentum=APG["momentum"]),
            "interval": dict(guidance_interval=(0.5, 0.9))}
LOOP_KW = {"rescale": dict(mode="rescale"), "apg": dict(mode="apg", **APG), "interval": dict(interval=(0.5, 0.9))}


def sampled(pipe, dev, seed=SEED, family=FAMILY, cfg_weight=None, rows=slice(None), **kw):
    """text-to-image through denoise_latents at latent 8 x 16, 4 steps"""
    cfg, _, cfgw, text, pooled = family_inputs(family)
    n = len(seed) if isinstance(seed, list) else 1
    lat, iter_time = pipe.denoise_latents(text[rows].to(dev, BF), pooled[rows].to(dev, BF), num_steps=STEPS, cfg_weight=cfgw if cfg_weight is None else cfg_weight,
                                          latent_size=(HL, WL), seed=seed, **kw)
    assert lat.shape == (n, HL, WL, 16) and lat.dtype == torch.float32 and len(iter_time) == STEPS
    return lat


@functools.lru_cache(maxsize=None)
def loop_references(setting, sampler="euler"):
    """the guided loop on the fp32 and the bf16-emulating oracle, after process_out"""
    cfg, shift, cfgw, text, pooled = family_inputs(FAMILY)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    sigmas = op.get_sigmas(shift, False, STEPS)
    x0, _ = start_state(sigmas, SEED, HL, WL)
    return {pname: op.process_out(guided_loop(OracleMMDiT(cfg, wf, P), sampler, x0, sigmas, text, pooled, cfgw, Prec(BF), t_act_of(cfg), **LOOP_KW[setting]),
                                  "sd3") for pname, P in (("fp32", Prec()), ("emu", Prec(BF)))}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_pipeline_parity(dev, setting):
    """tiny SD3 + CFG 5: rescale 0.7, apg with momentum -0.5, and cfg inside the interval (0.5, 0.9), against the guided loop on the fp32 oracle: the
    project's yardstick, err(hip) <= 2 err(bf16-emulating oracle) + 2e-3, and 35 dB where the bf16-emulating oracle alone reaches 37 dB (otherwise the
    figure is printed).  Each differs in bits from plain cfg."""
    from tests.test_gpu_model import yardstick_ok
    pipe = pipe_for(FAMILY, dev)
    lat = sampled(pipe, dev, **SETTINGS[setting])
    res = loop_references(setting)
    p_h, p_e = psnr(res["fp32"], lat), psnr(res["fp32"], res["emu"])
    print(f"[guidance] {setting}: rel_l2 hip {rel_l2(res['fp32'], lat):.3e} / emu {rel_l2(res['fp32'], res['emu']):.3e}, "
          f"PSNR hip {p_h:.1f} dB / emu {p_e:.1f} dB; last_guidance {pipe.last_guidance}")
    yardstick_ok(lat, res["emu"], res["fp32"], setting)
    if p_e >= 37.0:
        assert p_h > 35.0, f"{setting}: PSNR {p_h:.1f} dB"
    assert not same_bits(lat, sampled(pipe, dev))


# ---- 8. the interval run -----------------------------------------------------------------------------------------------------------------------------------
def test_interval_run(dev):
    from diffusionkit_amd.pipeline import DiffusionPipeline
    pipe = pipe_for(FAMILY, dev)
    sampled(pipe, dev, guidance_interval=(0.5, 0.9))
    g = pipe.last_guidance
    print(f"[guidance] interval (0.5, 0.9): {g}")
    assert g["mode"] == "cfg" and g["interval"] == (0.5, float(np.float32(0.9))) and (g["guided_evals"], g["unguided_evals"]) == (2, 2)
    # an interval that excludes every evaluation: the cfg_weight = 0 run on the prompt row, bit for bit
    none = sampled(pipe, dev, guidance_interval=(2.0, 3.0))
    assert (pipe.last_guidance["guided_evals"], pipe.last_guidance["unguided_evals"]) == (0, STEPS)
    assert same_bits(none, sampled(pipe, dev, cfg_weight=0.0, rows=slice(0, 1))), "the all-excluding interval is not the unguided run"
    # an interval that holds every evaluation: plain cfg, bit for bit (through the coefficient-row loop)
    assert same_bits(sampled(pipe, dev, guidance_interval=(0.0, 2.0)), sampled(pipe, dev))
    # the re-prepare leaves no state behind: defaults on this pipeline equal a fresh pipeline's bits
    sampled(pipe, dev, guidance_interval=(0.5, 0.9))
    cfg, shift, _ = FAMILIES[FAMILY]
    fresh = DiffusionPipeline(model_version="argmaxinc/mlx-stable-diffusion-3-medium", w16=True, a16=True, shift=shift, mmdit_config=cfg, vae_config=tiny_vae(),
                              vae_encoder_config=tiny_vae_encoder(), device=dev, text_len=16)
    assert same_bits(sampled(pipe, dev), sampled(fresh, dev)), "a default run after an interval run differs from a fresh pipeline's"


# ---- 9. compositions ---------------------------------------------------------------------------------------------------------------------------------------
def test_seed_list_under_apg(dev):
    """seed = [2, 3]: each image equals its single-seed run bit for bit, tests/test_gpu_inpaint.py's seed-list criterion (moments and momentum are per
    image)"""
    pipe = pipe_for(FAMILY, dev)
    both = sampled(pipe, dev, seed=[2, 3], **SETTINGS["apg"])
    for i, s in enumerate((2, 3)):
        one = sampled(pipe, dev, seed=s, **SETTINGS["apg"])
        print(f"[guidance] seed list under apg: image {i} (seed {s}) against its single-seed run: max_abs {max_abs(both[i:i + 1], one):.3e}")
        assert same_bits(both[i:i + 1], one), f"image {i} of the seed list differs from the single-seed run"


def test_ab2_interval_block_cache(dev):
    """ab2 + interval (0.5, 0.9) + FixedSchedule({1, 2}): evaluation 1 opens the guided stretch on a re-prepared engine, so it computes although the
    schedule names it; 2 is skipped; 0 and 3 (first and last, each the start of an unguided stretch) compute"""
    pipe = pipe_for(FAMILY, dev)
    lat = sampled(pipe, dev, sampler="ab2", guidance_interval=(0.5, 0.9), block_cache=FixedSchedule({1, 2}))
    rec = pipe.last_block_cache
    print(f"[guidance] ab2 + interval + FixedSchedule({{1, 2}}): {rec}; {pipe.last_guidance}")
    assert rec["computed"] == [0, 1, 3] and rec["skipped"] == [2] and len(rec["rel"]) == STEPS
    assert bool(torch.isfinite(lat).all()) and (pipe.last_guidance["guided_evals"], pipe.last_guidance["unguided_evals"]) == (2, 2)
    assert same_bits(sampled(pipe, dev, sampler="ab2", guidance_interval=(0.5, 0.9), block_cache=0.0),
                     sampled(pipe, dev, sampler="ab2", guidance_interval=(0.5, 0.9)))  # (a policy that never skips: the same launches)
    with pytest.raises(ValueError, match="two model evaluations"):
        sampled(pipe, dev, sampler="heun", guidance="rescale", block_cache=0.1)
    heun = sampled(pipe, dev, sampler="heun", guidance="apg", apg_momentum=-0.5, guidance_interval=(0.5, 0.9))
    assert bool(torch.isfinite(heun).all()) and (pipe.last_guidance["guided_evals"], pipe.last_guidance["unguided_evals"]) == (4, 3)


@functools.lru_cache(maxsize=None)
def masked_references():
    """the rescale loop with the blend behind each row, on the fp32 and the bf16-emulating oracle, each from its own OracleVAEEncoder posterior sample
    (as tests/test_gpu_inpaint.py's references)"""
    cfg, shift, cfgw, text, pooled = family_inputs(FAMILY)
    ecfg = tiny_vae_encoder()
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    ewf = {k: v.float() for k, v in synth_vae_encoder_weights(ecfg, seed=1234 + 2).items()}
    sigmas = op.get_sigmas(shift, False, STEPS)
    res = {}
    for pname, P in (("fp32", Prec()), ("emu", Prec(BF))):
        x_orig = op.process_in(op.encode_image_to_latents(OracleVAEEncoder(ecfg, ewf, P), op.read_image_array(RGB), seed=SEED), "sd3")
        x0, noise = start_state(sigmas, SEED, HL, WL, x_T=x_orig)
        x = guided_loop(OracleMMDiT(cfg, wf, P), "euler", x0, sigmas, text, pooled, cfgw, Prec(BF), t_act_of(cfg), mode="rescale",
                        inpaint=(noise, x_orig, latent_mask(HALF)))
        res[pname] = op.process_out(x, "sd3")
    return res


def test_half_mask_inpainting_under_rescale(dev):
    """the kept half is the encoded image bit for bit, the whole latent within tests/test_gpu_inpaint.py's gates of the masked rescale loop"""
    pipe = pipe_for(FAMILY, dev)
    lat = sampled(pipe, dev, guidance="rescale", image_path=RGB, denoise=1.0, mask_path=HALF)
    _, kept = encoded(pipe)
    assert same_bits(lat[:, :, :WL // 2], kept[:, :, :WL // 2]) and not same_bits(lat[:, :, WL // 2:], kept[:, :, WL // 2:])
    assert not same_bits(lat, sampled(pipe, dev, image_path=RGB, denoise=1.0, mask_path=HALF))
    half_mask_gates(lat, masked_references(), "sd3 rescale half mask")


def test_f16_under_apg(dev):
    """activation_dtype = "float16": the gates of tests/test_gpu_f16_model.py's pipeline test"""
    from tests.test_gpu_f16_model import f16_weights, gate
    pipe = pipe_for(FAMILY, dev, f16=True)
    assert pipe.mmdit.dtype == F16
    lat = sampled(pipe, dev, **SETTINGS["apg"])
    cfg, shift, cfgw, text, pooled = family_inputs(FAMILY)
    _, wf = f16_weights(cfg)
    sigmas = op.get_sigmas(shift, False, STEPS)
    x0, _ = start_state(sigmas, SEED, HL, WL)
    res = {}
    for oname, (m, act) in {"fp32": (OracleMMDiT(cfg, wf, Prec(), embed_prec=Prec(embed_dtype(cfg))), Prec(F16)),
                            "emu16": (OracleMMDiT(cfg, wf, Prec(F16)), Prec(F16)), "emubf": (OracleMMDiT(cfg, wf, Prec(BF)), Prec(BF))}.items():
        res[oname] = op.process_out(guided_loop(m, "euler", x0, sigmas, text, pooled, cfgw, act, t_act=Prec(F16), **LOOP_KW["apg"]), "sd3")
    gate(lat, res["emu16"], res["emubf"], res["fp32"], "apg f16")


# ---- 10. the default is untouched ---------------------------------------------------------------------------------------------------------------------
def test_default_is_untouched(dev, monkeypatch):
    """without the keywords, with guidance=None and with guidance="cfg": bit-identical latents, no launch of the guided entry, no re-prepare; the
    keywords at their default values change nothing either.  FLUX raises with any guidance option."""
    from diffusionkit_amd import ops, pipeline
    pipe = pipe_for(FAMILY, dev)
    calls = []
    monkeypatch.setattr(ops, "guided_cfg_step", lambda *a, **k: calls.append("guided_cfg_step"))
    monkeypatch.setattr(pipeline, "_set_rows", lambda *a, **k: calls.append("_set_rows"))
    omitted = sampled(pipe, dev)
    assert pipe.last_guidance["mode"] == "cfg" and (pipe.last_guidance["guided_evals"], pipe.last_guidance["unguided_evals"]) == (STEPS, 0)
    assert same_bits(sampled(pipe, dev, guidance=None), omitted) and same_bits(sampled(pipe, dev, guidance="cfg"), omitted)
    assert same_bits(sampled(pipe, dev, guidance="cfg", guidance_rescale=0.7, apg_eta=0.0, apg_norm_threshold=0.0, apg_momentum=0.0,
                             guidance_interval=None), omitted)
    for s in ("heun", "ab2"):
        assert same_bits(sampled(pipe, dev, sampler=s, guidance="cfg"), sampled(pipe, dev, sampler=s))
    assert calls == []
    flux = pipe_for("flux", dev)
    for kw in (dict(guidance="rescale"), dict(guidance="apg"), dict(guidance_interval=(0.5, 0.9)), dict(apg_momentum=-0.5)):
        with pytest.raises(ValueError, match="cfg_weight"):
            sampled(flux, dev, family="flux", **kw)
    with pytest.raises(ValueError, match="cfg, rescale, apg"):
        sampled(pipe, dev, guidance="cads")
    assert calls == []


# ---- 11. generate_image and the CLI ---------------------------------------------------------------------------------------------------------------------
def test_generate_image_and_cli(dev, tmp_path):
    from diffusionkit_amd import cli
    pipe = pipe_for(FAMILY, dev)
    img, log = pipe.generate_image("a cat", num_steps=STEPS, cfg_weight=5.0, latent_size=(HL, WL), seed=SEED, verbose=False)
    assert "guidance" not in log["denoising"]
    img, log = pipe.generate_image("a cat", num_steps=STEPS, cfg_weight=5.0, latent_size=(HL, WL), seed=SEED, verbose=False, guidance="apg",
                                   apg_momentum=-0.5, apg_norm_threshold=15.0, guidance_interval=(0.5, 0.9))
    g = log["denoising"]["guidance"]
    print(f"[guidance] generate_image: {g}")
    assert img.size == (W_IMG, H_IMG) and len(log["denoising"]["iter_time"]) == STEPS and g == pipe.last_guidance
    assert (g["mode"], g["apg_momentum"], g["apg_norm_threshold"], g["guided_evals"], g["unguided_evals"]) == ("apg", -0.5, 15.0, 2, 2)
    over = dict(mmdit_config=tiny_sd3(), vae_config=tiny_vae(), text_len=20)
    out = tmp_path / "out.png"
    argv = ["--prompt", "a cat", "--model-version", "argmaxinc/mlx-stable-diffusion-3-medium", "--steps", "4", "--seed", "7", "--height", "64", "--width",
            "64", "-o", str(out)]
    img, log = cli.main(argv + ["--guidance", "rescale", "--guidance-rescale", "0.5", "--guidance-interval", "0.5", "0.9"], pipeline_overrides=over)
    g = log["denoising"]["guidance"]
    assert out.exists() and img.size == (64, 64)
    assert (g["mode"], g["guidance_rescale"], g["guided_evals"], g["unguided_evals"]) == ("rescale", 0.5, 2, 2)
    _, log = cli.main(argv, pipeline_overrides=over)
    assert "guidance" not in log["denoising"]
