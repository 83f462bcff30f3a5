"""Second-order samplers on an MI355X: the coefficient-row step (dk_lms_cfg_step / _masked / _f16) against a float64 restatement and against
dk_euler_cfg_step bit for bit, its history discipline and exact masked ends, and the pipeline (``sampler="heun"`` / ``"ab2"``) against the loops
restated on the oracle in tests/test_samplers_cpu.py, under the project's model-level gates.  Every figure is printed before it is asserted.

Operator shapes: test_patchify_and_euler_step's (latent 8 x 12 x 16, p 2, two images: 3072 elements, twelve blocks of 256 threads); pipeline
shapes: tests/test_gpu_inpaint.py's (latent 8 x 16, 4 steps, seed 2).  The file name sorts behind tests/test_gpu_fullsize.py like that file's."""
import functools

import numpy as np
import pytest
import torch

from diffusionkit_amd.config import tiny_flux, tiny_sd3, tiny_vae, tiny_vae_encoder
from diffusionkit_amd.sampler import FixedSchedule
from diffusionkit_amd.weights import synth_mmdit_weights, synth_vae_encoder_weights
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec, embed_dtype
from oracle.vae import OracleVAEEncoder
from tests import _footprint as fp
from tests._util import BF, max_abs, psnr, rel_l2
from tests.test_gpu_inpaint import (H_IMG, HALF, HL, RGB, SEED, STEPS, W_IMG, WL, encoded, half_mask_gates, pipe_for, same_bits, tokens_of)
from tests.test_inpaint_cpu import FAMILIES, family_inputs, latent_mask, t_act_of
from tests.test_samplers_cpu import plan_loop, start_state, textbook_loop

pytestmark = pytest.mark.gpu

F16 = torch.float16
N_IMG, Hl, Wl, C, P_ = 2, 8, 12, 16, 2
S_I, F = (Hl // P_) * (Wl // P_), P_ * P_ * C
SIGMA, SIGMA_NEXT = float(np.float32(0.8)), float(np.float32(0.3))  # (1 - sigma_next is not exact in fp32)
# an arbitrary row: every coefficient non-trivial, magnitudes below 1 like the plans' own (d reaches 25 under CFG 5: its fp32 round-off, about 3e-6,
# scales with cd and hd)
COEF = tuple(float(np.float32(v)) for v in (0.9, -0.3, 0.45, 0.25, 0.75))
EULER = (1.0, float(np.float32(SIGMA_NEXT) - np.float32(SIGMA)), 0.0, 0.0, 0.0)  # cd: the fp32 difference dk_euler_cfg_step takes


def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def where_of(order):
    """[N_IMG, S_I, F] -> which latent element each token feature is, taken from the oracle's patchify on a tensor of element indices"""
    orc = OracleMMDiT(tiny_flux() if order else tiny_sd3(),
                      {"x_embedder.proj.weight": torch.eye(F).reshape(F, *((1, 1, F) if order else (P_, P_, C))), "x_embedder.proj.bias": torch.zeros(F)}, Prec())
    index = torch.arange(N_IMG * Hl * Wl * C, dtype=torch.float32).reshape(N_IMG, Hl, Wl, C)
    where = orc._patch_embed(index).long()
    assert torch.equal(torch.sort(where.reshape(-1))[0], torch.arange(index.numel()))
    return where


class Operands:
    """seeded operands of one launch on the device; ``step`` runs it on fresh copies and returns (x, tokens, hist)"""

    def __init__(self, dev, order, cfgw, dt, ld_pad=0):
        self.dev, self.order, self.cfgw, self.dt, self.cfg_on = dev, order, cfgw, dt, cfgw > 0
        self.dup = 2 if self.cfg_on else 1
        self.x = torch.randn(N_IMG, Hl, Wl, C, generator=gen(1))
        self.out = torch.randn(N_IMG * self.dup, S_I, F + ld_pad, generator=gen(2)).to(dt)
        self.hist = torch.randn(N_IMG, Hl, Wl, C, generator=gen(6))
        self.x_orig = torch.randn(N_IMG, Hl, Wl, C, generator=gen(3)) * 1.5 + 0.3
        self.noise = torch.randn(N_IMG, Hl, Wl, C, generator=gen(4))
        self.out_d, self.x_orig_d, self.noise_d = self.out.to(dev), self.x_orig.to(dev), self.noise.to(dev)

    def step(self, coef, reads_h, writes_h, hist="own", mask=None, sigma_next=SIGMA_NEXT, euler=False):
        from diffusionkit_amd import ops
        x = self.x.to(self.dev)
        tok = torch.full((N_IMG * self.dup, S_I, F), 7.0, dtype=self.dt, device=self.dev)
        h = self.hist.to(self.dev) if isinstance(hist, str) else hist
        head = (x, self.out_d, tok, N_IMG, self.cfg_on, P_, self.order, SIGMA, sigma_next, self.cfgw)
        tail = () if mask is None else (self.x_orig_d, self.noise_d, mask.to(self.dev))
        if euler:
            (ops.euler_cfg_step if mask is None else ops.euler_cfg_step_masked)(*head, *tail)
        else:
            (ops.lms_cfg_step if mask is None else ops.lms_cfg_step_masked)(*head, h, coef, reads_h, writes_h, *tail)
        return x, tok, h

    def ref64(self, coef, reads_h):
        """float64 evaluation on the fp32 operands: (x', H')"""
        cx, cd, ch, hx, hd = coef
        where = where_of(self.order)
        n = N_IMG * Hl * Wl * C
        u = torch.empty(self.dup * n, dtype=torch.float64)
        u[torch.cat([where + k * n for k in range(self.dup)]).reshape(-1)] = self.out[:, :, :F].double().reshape(-1)  # (unpatchify, per CFG copy)
        u = u.reshape(self.dup * N_IMG, Hl, Wl, C)
        x, xb = self.x.double(), self.x.to(self.dt).double()  # xb: the value the denoiser saw
        den = xb - u[:N_IMG] * SIGMA
        if self.cfg_on:
            den_neg = xb - u[N_IMG:] * SIGMA
            den = den_neg + self.cfgw * (den - den_neg)
        d = (x - den) / SIGMA
        return cx * x + cd * d + (ch * self.hist.double() if reads_h else 0.0), hx * x + hd * d


STEP_CASES = [(order, cfgw, dt, 0) for order in (0, 1) for cfgw in (0.0, 5.0) for dt in (BF, F16)] + [(1, 5.0, BF, 8)]
step_cases = pytest.mark.parametrize("order,cfgw,dt,ld_pad", STEP_CASES,
                                     ids=[f"order{o}-cfg{w:g}-{'bf16' if d == BF else 'f16'}-ld+{l}" for o, w, d, l in STEP_CASES])


# ---- 5. the operator against a float64 restatement ----------------------------------------------------------------------------------------------------
@step_cases
def test_lms_step_operator(dev, order, cfgw, dt, ld_pad):
    """an arbitrary row with every coefficient non-trivial (history read and written), and the same row without the history read: x' and H' within
    1e-5 of the float64 evaluation at unit-scale inputs (the bound of test_patchify_and_euler_step), tokens == dk_latent_to_tokens(x'), both copies"""
    o = Operands(dev, order, cfgw, dt, ld_pad)
    for reads_h in (True, False):
        x, tok, h = o.step(COEF, reads_h, True)
        rx, rh = o.ref64(COEF, reads_h)
        ex, eh = max_abs(rx, x), max_abs(rh, h)
        print(f"[samplers] lms step order={order} cfg={cfgw:g} {dt} ld+{ld_pad} reads_h={reads_h}: max_abs x' {ex:.2e}, H' {eh:.2e}")
        assert ex < 1e-5 and eh < 1e-5
        assert same_bits(tok, tokens_of(x, dt, N_IMG, o.dup, Hl, Wl, C, P_, order)), "tokens are not the patchified updated latent"
        if o.cfg_on:
            assert same_bits(tok[:N_IMG], tok[N_IMG:])
    assert not same_bits(o.step(COEF, True, True)[0], o.step(COEF, False, True)[0])  # (the history term is there)


# ---- 6. the Euler row is dk_euler_cfg_step, bit for bit --------------------------------------------------------------------------------------------
@step_cases
def test_euler_row_is_the_euler_step(dev, order, cfgw, dt, ld_pad):
    """(cx = 1, cd = sigma_next - sigma, no history) against ops.euler_cfg_step, and masked against masked with a random mask: the same x, the same
    tokens; hist -- NaN between sentinel margins -- is neither read (every output finite) nor written (its bits and the margins as they were)"""
    o = Operands(dev, order, cfgw, dt, ld_pad)
    for mask in (None, torch.rand(N_IMG, Hl, Wl, generator=gen(5))):
        hist, guard = fp.guarded(torch.full((N_IMG, Hl, Wl, C), fp.NAN, device=dev), 8, fp.SENTINEL)
        before = fp.bits(hist).clone()
        want_x, want_tok, _ = o.step(None, False, False, mask=mask, euler=True)
        x, tok, _ = o.step(EULER, False, False, hist=hist, mask=mask)
        what = "masked" if mask is not None else "plain"
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(tok.float()).all()), what
        assert same_bits(x, want_x), f"{what}: x differs from dk_euler_cfg_step's in {int((fp.bits(x) != fp.bits(want_x)).sum())} elements"
        assert same_bits(tok, want_tok), f"{what}: the tokens differ from dk_euler_cfg_step's"
        assert torch.equal(fp.bits(hist), before), f"{what}: hist was written"
        guard.check(f"{what}: hist")


# ---- 7. history discipline ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1], ids=["sd3", "flux"])
def test_history_discipline(dev, order):
    o = Operands(dev, order, 5.0, BF)
    nan_hist = lambda: torch.full((N_IMG, Hl, Wl, C), fp.NAN, device=dev)  # noqa: E731
    # reads_h off: a NaN-filled hist is never read, and the row leaves a finite one
    x, tok, h = o.step(COEF, False, True, hist=nan_hist())
    assert all(bool(torch.isfinite(t.float()).all()) for t in (x, tok, h))
    # writes_h off: hist stays byte for byte
    clean_x, clean_tok, h = o.step(COEF, True, False)
    assert same_bits(h, o.hist)
    # one NaN in hist under reads_h: exactly that latent element and its token feature in both CFG copies
    idx = (1, 5, 7, 9)
    poisoned = o.hist.clone()
    poisoned[idx] = fp.NAN
    x, tok, h = o.step(COEF, True, False, hist=poisoned.to(dev))
    hand_x = torch.zeros(N_IMG, Hl, Wl, C, dtype=torch.bool)
    hand_x[idx] = True
    flat = ((idx[0] * Hl + idx[1]) * Wl + idx[2]) * C + idx[3]
    hand_tok = where_of(order) == flat
    assert int(hand_tok.sum()) == 1
    fp.assert_footprint(clean_x, x, hand_x, "one NaN in hist [x]")
    fp.assert_footprint(clean_tok, tok, torch.cat([hand_tok, hand_tok]), "one NaN in hist [tok]")
    assert same_bits(h, poisoned)


# ---- 8. masked ends -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,cfgw,dt", [(0, 5.0, BF), (1, 0.0, BF), (0, 5.0, F16)], ids=["sd3-cfg-bf16", "flux-bf16", "sd3-cfg-f16"])
def test_masked_ends(dev, order, cfgw, dt):
    """m = 1: the plain launch bit for bit (x, tokens, H'); m = 0: known = sigma_next noise + (1 - sigma_next) x_orig -- within 2 * 2^-23 *
    max(|noise|, |x_orig|) of its float64 value: at most four half-ulp roundings (1 - sigma_next, two products, one sum) of values no larger than
    that maximum, whatever is fused; m = 0 with sigma_next = 0: x_orig bit for bit, on a predictor-type row (writes H) and a corrector-type row
    (reads H).  H' does not see the mask."""
    o = Operands(dev, order, cfgw, dt)
    ones, zeros = torch.ones(1, Hl, Wl), torch.zeros(N_IMG, Hl, Wl)
    for coef, reads_h, writes_h, kind in ((COEF, False, True, "predictor"), (COEF, True, False, "corrector"), (COEF, True, True, "both")):
        px, ptok, ph = o.step(coef, reads_h, writes_h)
        x, tok, h = o.step(coef, reads_h, writes_h, mask=ones)
        assert same_bits(x, px) and same_bits(tok, ptok) and same_bits(h, ph), f"{kind}: a mask of ones is not the plain launch"
        x, tok, h = o.step(coef, reads_h, writes_h, mask=zeros)
        known = SIGMA_NEXT * o.noise.double() + (1.0 - SIGMA_NEXT) * o.x_orig.double()
        bound = 2.0 * 2.0 ** -23 * torch.maximum(o.noise.abs(), o.x_orig.abs()).double()
        err = (x.double().cpu() - known).abs()
        print(f"[samplers] masked {kind} row, m = 0: largest |x - known| / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()) and same_bits(h, ph)
        assert same_bits(tok, tokens_of(x, dt, N_IMG, o.dup, Hl, Wl, C, P_, order))
        x, tok, h = o.step(coef, reads_h, writes_h, mask=zeros, sigma_next=0.0)
        assert same_bits(x, o.x_orig), f"{kind}: m = 0 with sigma_next = 0 does not return x_orig"
        assert same_bits(tok, tokens_of(o.x_orig_d, dt, N_IMG, o.dup, Hl, Wl, C, P_, order))


# ---- 9. refused arguments ---------------------------------------------------------------------------------------------------------------------------
def test_lms_step_refuses_bad_arguments(dev):
    from diffusionkit_amd import _lib, ops
    from diffusionkit_amd._lib import DkHipError
    o = Operands(dev, 1, 0.0, BF)
    x, tok, hist = o.x.to(dev), torch.full((N_IMG, S_I, F), 7.0, dtype=BF, device=dev), o.hist.to(dev)
    head = (x, o.out_d, tok, N_IMG, False, P_, 1, SIGMA, SIGMA_NEXT, 0.0)
    mask = torch.ones(1, Hl, Wl, device=dev)
    with pytest.raises(DkHipError, match="hist"):
        ops.lms_cfg_step(*head, None, COEF, True, False)
    with pytest.raises(DkHipError, match="hist"):
        ops.lms_cfg_step_masked(*head, None, COEF, False, True, o.x_orig_d, o.noise_d, mask)
    for k in range(5):
        bad = tuple(fp.NAN if j == k else v for j, v in enumerate(COEF))
        with pytest.raises(DkHipError, match="finite"):
            ops.lms_cfg_step(*head, hist, bad, True, True)
    with pytest.raises(DkHipError, match="finite"):
        ops.lms_cfg_step(*head, hist, (1.0, float("inf"), 0.0, 0.0, 1.0), False, True)
    with pytest.raises(DkHipError, match="sigma"):
        ops.lms_cfg_step(x, o.out_d, tok, N_IMG, False, P_, 1, 0.0, 0.0, 0.0, hist, COEF, True, True)
    with pytest.raises(DkHipError, match="mask"):
        ops.lms_cfg_step_masked(*head, hist, COEF, True, True, o.x_orig_d, o.noise_d, torch.ones(3, Hl, Wl, device=dev))
    with pytest.raises(DkHipError, match="mask"):
        ops.lms_cfg_step_masked(*head, hist, COEF, True, True, o.x_orig_d, o.noise_d, torch.ones(1, Hl, Wl + 2, device=dev))
    with pytest.raises(DkHipError, match="float32"):
        ops.lms_cfg_step_masked(*head, hist, COEF, True, True, o.x_orig_d, o.noise_d, mask.to(BF))
    # the library's own check of the mask operands (the wrapper never passes a null one)
    lib = _lib.load()
    rc = lib.dk_lms_cfg_step_masked(x.data_ptr(), o.out_d.data_ptr(), F, tok.data_ptr(), N_IMG, 0, Hl, Wl, C, P_, 1, SIGMA, 0.0, hist.data_ptr(), *COEF,
                                    SIGMA_NEXT, 1, 1, o.x_orig_d.data_ptr(), o.noise_d.data_ptr(), None, 0, None)
    assert rc != 0 and b"null" in lib.dk_last_error()
    torch.cuda.synchronize(dev)
    assert same_bits(x, o.x) and same_bits(hist, o.hist) and bool((tok == 7.0).all()), "a refused call wrote something"


# ---- 10. pipeline parity -------------------------------------------------------------------------------------------------------------------------------
def sampled(pipe, family, dev, sampler="omit", seed=SEED, **kw):
    """text-to-image through denoise_latents at latent 8 x 16, 4 steps; ``sampler="omit"``: the call without the keyword"""
    cfg, _, cfgw, text, pooled = family_inputs(family)
    n = len(seed) if isinstance(seed, list) else 1
    if n > 1 and cfgw == 0:
        text, pooled = text.repeat(n, 1, 1), pooled.repeat(n, 1)
    if sampler != "omit":
        kw["sampler"] = sampler
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=STEPS, cfg_weight=cfgw, latent_size=(HL, WL), seed=seed, **kw)
    assert lat.shape == (n, HL, WL, 16) and lat.dtype == torch.float32 and len(iter_time) == STEPS
    return lat


@functools.lru_cache(maxsize=None)
def loop_references(family, sampler):
    """the textbook loop on the fp32 and the bf16-emulating oracle, after process_out"""
    cfg, shift, cfgw, text, pooled = family_inputs(family)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    sigmas = op.get_sigmas(shift, cfg.is_flux, STEPS)
    x0, _ = start_state(sigmas, SEED, HL, WL)
    return {pname: op.process_out(textbook_loop(OracleMMDiT(cfg, wf, P), sampler, x0, sigmas, text, pooled, cfgw, Prec(BF), t_act_of(cfg)),
                                  "flux" if cfg.is_flux else "sd3") for pname, P in (("fp32", Prec()), ("emu", Prec(BF)))}


@pytest.mark.parametrize("sampler", ["heun", "ab2"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_pipeline_parity(dev, family, sampler):
    """tiny FLUX and tiny SD3 + CFG 5 against the textbook loop on the fp32 oracle: the project's yardstick, err(hip) <= 2 err(bf16-emulating oracle) +
    2e-3, and 35 dB where the bf16-emulating oracle alone reaches 37 dB on the case.  It does on all but SD3 + CFG 5 under heun (33 - 34 dB with these
    random weights, measured without a GPU: the corrector's second evaluation goes through the bf16 rounding of the model input once more under a
    guidance weight of 5); there the yardstick is the gate and the figure is printed."""
    from tests.test_gpu_model import yardstick_ok
    pipe = pipe_for(family, dev)
    lat = sampled(pipe, family, dev, sampler)
    assert pipe.last_sampler == {"sampler": sampler, "model_evals": 2 * STEPS - 1 if sampler == "heun" else STEPS}
    res = loop_references(family, sampler)
    p_h, p_e = psnr(res["fp32"], lat), psnr(res["fp32"], res["emu"])
    print(f"[samplers] {family} {sampler}: rel_l2 hip {rel_l2(res['fp32'], lat):.3e} / emu {rel_l2(res['fp32'], res['emu']):.3e}, "
          f"PSNR hip {p_h:.1f} dB / emu {p_e:.1f} dB")
    yardstick_ok(lat, res["emu"], res["fp32"], f"{family} {sampler}")
    if p_e >= 37.0:
        assert p_h > 35.0, f"{family} {sampler}: PSNR {p_h:.1f} dB"
    assert not same_bits(lat, sampled(pipe, family, dev, "euler"))


def test_pipeline_parity_f16(dev):
    """activation_dtype = "float16", SD3 + CFG 5, ab2: the gates of tests/test_gpu_f16_model.py's pipeline test"""
    from tests.test_gpu_f16_model import f16_weights, gate
    family = "sd3_cfg"
    pipe = pipe_for(family, dev, f16=True)
    assert pipe.mmdit.dtype == F16
    lat = sampled(pipe, family, dev, "ab2")
    cfg, shift, cfgw, text, pooled = family_inputs(family)
    _, wf = f16_weights(cfg)
    sigmas = op.get_sigmas(shift, False, STEPS)
    x0, _ = start_state(sigmas, SEED, HL, WL)
    res = {}
    for oname, (m, act) in {"fp32": (OracleMMDiT(cfg, wf, Prec(), embed_prec=Prec(embed_dtype(cfg))), Prec(F16)),
                            "emu16": (OracleMMDiT(cfg, wf, Prec(F16)), Prec(F16)), "emubf": (OracleMMDiT(cfg, wf, Prec(BF)), Prec(BF))}.items():
        res[oname] = op.process_out(textbook_loop(m, "ab2", x0, sigmas, text, pooled, cfgw, act, t_act=Prec(F16)), "sd3")
    gate(lat, res["emu16"], res["emubf"], res["fp32"], "ab2 f16")


# ---- 11. compositions ---------------------------------------------------------------------------------------------------------------------------------
def test_seed_list_under_ab2(dev):
    """seed = [2, 3, 4]: each image equals its single-seed run bit for bit, as tests/test_gpu_inpaint.py's seed list does (the history buffer is
    per element, like the latent)"""
    pipe = pipe_for("flux", dev)
    three = sampled(pipe, "flux", dev, "ab2", seed=[2, 3, 4])
    for i, s in enumerate((2, 3, 4)):
        one = sampled(pipe, "flux", dev, "ab2", seed=s)
        print(f"[samplers] seed list: image {i} (seed {s}) against its single-seed run: max_abs {max_abs(three[i:i + 1], one):.3e}")
        assert same_bits(three[i:i + 1], one), f"image {i} of the seed list differs from the single-seed run"


@functools.lru_cache(maxsize=None)
def masked_references(family, sampler):
    """the rows of the plan with the blend behind each, on the fp32 and the bf16-emulating oracle, each from its own OracleVAEEncoder posterior sample
    (as tests/test_gpu_inpaint.py's references)"""
    cfg, shift, cfgw, text, pooled = family_inputs(family)
    ecfg = tiny_vae_encoder()
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    ewf = {k: v.float() for k, v in synth_vae_encoder_weights(ecfg, seed=1234 + 2).items()}
    fmt = "flux" if cfg.is_flux else "sd3"
    sigmas = op.get_sigmas(shift, cfg.is_flux, STEPS)
    res = {}
    for pname, P in (("fp32", Prec()), ("emu", Prec(BF))):
        x_orig = op.process_in(op.encode_image_to_latents(OracleVAEEncoder(ecfg, ewf, P), op.read_image_array(RGB), seed=SEED), fmt)
        x0, noise = start_state(sigmas, SEED, HL, WL, x_T=x_orig)
        x = plan_loop(OracleMMDiT(cfg, wf, P), sampler, x0, sigmas, text, pooled, cfgw, Prec(BF), t_act_of(cfg), inpaint=(noise, x_orig, latent_mask(HALF)))
        res[pname] = op.process_out(x, fmt)
    return res


@pytest.mark.parametrize("sampler", ["heun", "ab2"])
def test_half_mask_inpainting(dev, sampler):
    """right-half mask on tiny FLUX: the kept half is the encoded image bit for bit, the repainted half within tests/test_gpu_inpaint.py's gates of the
    masked loop restated on the oracle"""
    pipe = pipe_for("flux", dev)
    lat = sampled(pipe, "flux", dev, sampler, image_path=RGB, denoise=1.0, mask_path=HALF)
    _, kept = encoded(pipe)
    assert same_bits(lat[:, :, :WL // 2], kept[:, :, :WL // 2])
    assert not same_bits(lat[:, :, WL // 2:], kept[:, :, WL // 2:])
    euler = sampled(pipe, "flux", dev, "euler", image_path=RGB, denoise=1.0, mask_path=HALF)
    assert not same_bits(lat[:, :, WL // 2:], euler[:, :, WL // 2:])
    half_mask_gates(lat, masked_references("flux", sampler), f"flux {sampler} half mask")
    # an all-0 mask returns the encoded image, an all-255 mask the img2img run, bit for bit
    assert same_bits(sampled(pipe, "flux", dev, sampler, image_path=RGB, denoise=1.0, mask_path=np.zeros_like(HALF)), kept)
    assert same_bits(sampled(pipe, "flux", dev, sampler, image_path=RGB, denoise=1.0, mask_path=np.full_like(HALF, 255)),
                     sampled(pipe, "flux", dev, sampler, image_path=RGB, denoise=1.0))


def test_block_cache_compositions(dev):
    """ab2 with FixedSchedule({1}) runs and records one skip; heun refuses a block cache, and says why"""
    pipe = pipe_for("flux", dev)
    plain = sampled(pipe, "flux", dev, "ab2")
    assert pipe.last_block_cache is None
    lat = sampled(pipe, "flux", dev, "ab2", block_cache=FixedSchedule({1}))
    rec = pipe.last_block_cache
    print(f"[samplers] ab2 + FixedSchedule({{1}}): {rec}")
    assert rec["skipped"] == [1] and rec["computed"] == [0, 2, 3] and len(rec["rel"]) == STEPS
    assert bool(torch.isfinite(lat).all()) and not same_bits(lat, plain)
    assert same_bits(sampled(pipe, "flux", dev, "ab2", block_cache=0.0), plain)  # (a policy that never skips: the same launches)
    assert same_bits(sampled(pipe, "flux", dev, "ab2"), plain) and not pipe.mmdit.block_cache  # (and the option leaves nothing behind)
    with pytest.raises(ValueError, match="two model evaluations"):
        sampled(pipe, "flux", dev, "heun", block_cache=0.1)
    with pytest.raises(ValueError, match="euler, heun, ab2"):
        sampled(pipe, "flux", dev, "dpm")


def test_img2img_cut_schedule(dev):
    """denoise 0.5 of 4 steps: the two remaining steps, first-order start -- 3 evaluations under heun, 2 under ab2; runs and differs from Euler"""
    pipe = pipe_for("flux", dev)
    cfg, _, cfgw, text, pooled = family_inputs("flux")
    outs = {}
    for sampler, evals in (("euler", 2), ("heun", 3), ("ab2", 2)):
        lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=STEPS, cfg_weight=cfgw, latent_size=(HL, WL), seed=SEED,
                                              image_path=RGB, denoise=0.5, sampler=sampler)
        assert len(iter_time) == 2 and pipe.last_sampler == {"sampler": sampler, "model_evals": evals} and bool(torch.isfinite(lat).all())
        outs[sampler] = lat
    assert not same_bits(outs["heun"], outs["euler"])
    assert same_bits(outs["ab2"], outs["euler"])  # (two steps that end at sigma = 0: the first row and the last row are both Euler rows)


def test_generate_image_and_cli(dev, tmp_path):
    """generate_image(sampler=) logs what ran, with one iter_time entry per step; --sampler reaches it"""
    from diffusionkit_amd import cli
    pipe = pipe_for("flux", dev)
    for sampler, evals in ((None, STEPS), ("heun", 2 * STEPS - 1), ("ab2", STEPS)):
        img, log = pipe.generate_image("a cat", num_steps=STEPS, latent_size=(HL, WL), seed=SEED, verbose=False, sampler=sampler)
        assert img.size == (W_IMG, H_IMG) and len(log["denoising"]["iter_time"]) == STEPS
        assert log["denoising"]["sampler"] == (sampler or "euler") and log["denoising"]["model_evals"] == evals
    over = dict(mmdit_config=tiny_flux(), vae_config=tiny_vae(), text_len=20)
    argv = ["--prompt", "a cat", "--steps", "4", "--seed", "7", "--height", "64", "--width", "64", "-o", str(tmp_path / "out.png")]
    _, log = cli.main(argv + ["--sampler", "heun"], pipeline_overrides=over)
    assert log["denoising"]["sampler"] == "heun" and log["denoising"]["model_evals"] == 7 and len(log["denoising"]["iter_time"]) == 4
    with pytest.raises(ValueError, match="block-cache"):
        cli.main(argv + ["--sampler", "heun", "--block-cache", "0.1"], pipeline_overrides=over)


# ---- 12. the default is untouched ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_default_is_untouched(dev, family, monkeypatch):
    """sampler=None, sampler="euler" and the call without the keyword: bit-identical latents, and no launch of the new entries"""
    from diffusionkit_amd import ops
    pipe = pipe_for(family, dev)
    calls = []
    for name in ("lms_cfg_step", "lms_cfg_step_masked"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    omitted = sampled(pipe, family, dev, "omit")
    assert same_bits(sampled(pipe, family, dev, None), omitted) and same_bits(sampled(pipe, family, dev, "euler"), omitted)
    masked = sampled(pipe, family, dev, "omit", image_path=RGB, denoise=1.0, mask_path=HALF)
    assert same_bits(sampled(pipe, family, dev, "euler", image_path=RGB, denoise=1.0, mask_path=HALF), masked)
    assert calls == [] and pipe.last_sampler == {"sampler": "euler", "model_evals": STEPS}
