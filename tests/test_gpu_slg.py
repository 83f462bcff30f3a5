"""Skip-layer guidance on an MI355X: the engine's forked row group (``MMDiTEngine.set_skip_layers``) against ``tests/_slg.SkipOracle``, the step
entry dk_slg_cfg_step against ``sampler.slg_reference`` and against dk_guided_cfg_step bit for bit at scale 0, and the pipeline keywords against the
loop restated in tests/_slg.py.

The gates are the project's own: tests/test_gpu_model.py's ``yardstick_ok`` and PSNR > 35 dB, tests/test_gpu_f16_model.py's ``gate`` in float16,
tests/test_gpu_guidance.py's operator bound max(1e-5, 4 e32), tests/test_gpu_inpaint.py's half-mask gates; nothing here sets a tolerance of its own.
The weights are boosted (tests/_slg.boost) so that a skipped block moves the output by several times those gates: tests/test_slg_cpu.py asserts
that on the oracles alone.  Every figure is printed before it is asserted.  Arithmetic parity on synthetic weights: no SD3.5-medium checkpoint has
been run."""
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

from diffusionkit_amd.config import SD3_5_MEDIUM, float16_config, tiny_flux, tiny_vae, tiny_vae_encoder
from diffusionkit_amd.sampler import slg_reference
from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights, synth_vae_encoder_weights
from oracle import pipeline as op
from oracle.mmdit import Prec
from oracle.vae import OracleVAEEncoder
from tests import _footprint as fp
from tests import _slg
from tests._util import BF, psnr, randn, rel_l2
from tests.test_gpu_f16_model import gate as gate_f16
from tests.test_gpu_guidance import (C, CFGW, COEF, EULER, MODES, N_IMG, P_, SCALE, SIGMA, SIGMA_NEXT, Operands, cases, gen, guide_f32,
                                     own_scale_err, where_of)
from tests.test_gpu_inpaint import HALF, HL as MASK_HL, RGB, WL as MASK_WL, half_mask_gates, same_bits, tokens_of
from tests.test_gpu_model import psnr_ok, yardstick_ok
from tests.test_inpaint_cpu import latent_mask
from tests.test_samplers_cpu import start_state

pytestmark = pytest.mark.gpu

F16 = torch.float16
VERSION = "stabilityai/stable-diffusion-3.5-medium"
TS = _slg.TS


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------------------
def engine_for(cfg, named, dev):
    from diffusionkit_amd.engine import MMDiTEngine
    return MMDiTEngine(cfg, pack_mmdit(cfg, named, dev))


def three_groups(t, n):
    """[prompt x n | negative x n] -> [prompt x n | negative x n | prompt x n]"""
    return torch.cat([t, t[:n]], 0)


def forked_forward(eng, cfg, n, Hl, Wl, S_t, skip, dev, dt=BF, poison=False, cached_context=False):
    """one forward of step 1 on B = 3 n rows with the last n forked; ``poison``: the fork rows of tokens_in and of text hold NaN"""
    text, pooled, lat = _slg.forward_inputs(cfg, n, Hl, Wl, S_t)
    eng.prepare(3 * n, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(three_groups(pooled, n).to(dev), TS)
    eng.set_skip_layers(skip, n)
    tok = eng.patchify(three_groups(lat, n).to(dev))
    text = three_groups(text, n).to(dev, dt).contiguous()
    if poison:
        tok[2 * n:] = fp.NAN
        text[2 * n:] = fp.NAN
    if cached_context:
        eng.cache_context(text)
        text = None
    return eng.forward_tokens(tok, text, 1)


FORWARD_CASES = [("b3", s) for s in _slg.SKIP_SETS] + [("heads6_35tok", (1, 2))]


@pytest.mark.parametrize("case,skip", FORWARD_CASES, ids=[f"{c}-skip{'_'.join(map(str, s))}" for c, s in FORWARD_CASES])
def test_forked_forward(dev, case, skip):
    """rows [0, 2 n) against the full oracle, the fork rows against the skip oracle -- and the fork rows must FAIL the gate against the full oracle:
    otherwise the skip was not honoured"""
    cfg, n, Hl, Wl, S_t = _slg.FORWARD[case]
    eng = engine_for(cfg, _slg.boosted_weights(cfg, skip), dev)
    out = forked_forward(eng, cfg, n, Hl, Wl, S_t, skip, dev).float().cpu()
    assert out.shape[0] == 3 * n and bool(torch.isfinite(out).all())
    res = _slg.forward_refs(case, skip)
    live, fork = out[:2 * n], out[2 * n:]
    e_fork_full = rel_l2(res["full"]["fp32"][:n], fork)
    print(f"[slg] forward {case} skip {skip}: live rows hip-vs-fp32 {rel_l2(res['full']['fp32'], live):.3e} (emulation "
          f"{rel_l2(res['full']['fp32'], res['full']['emu']):.3e}), PSNR {psnr(res['full']['fp32'], live):.1f} dB; fork rows hip-vs-skip-fp32 "
          f"{rel_l2(res['skip']['fp32'], fork):.3e} (emulation {rel_l2(res['skip']['fp32'], res['skip']['emu']):.3e}), PSNR "
          f"{psnr(res['skip']['fp32'], fork):.1f} dB; fork rows against the FULL oracle {e_fork_full:.3e}")
    yardstick_ok(live, res["full"]["emu"], res["full"]["fp32"], f"{case} live rows")
    yardstick_ok(fork, res["skip"]["emu"], res["skip"]["fp32"], f"{case} fork rows")
    assert psnr(res["full"]["fp32"], live) > 35.0 and psnr(res["skip"]["fp32"], fork) > 35.0
    with pytest.raises(AssertionError):
        yardstick_ok(fork, res["full"]["emu"][:n], res["full"]["fp32"][:n], "fork rows against the full oracle")


def test_fork_rows_are_never_read(dev):
    """NaN in the fork rows of tokens_in and of text, no cached context: finite everywhere, and the bits of the call with finite fork rows; the same with
    the context cached from a text whose fork rows hold NaN"""
    cfg, n, Hl, Wl, S_t = _slg.FORWARD["heads6_35tok"]
    skip = (1, 2)
    eng = engine_for(cfg, _slg.boosted_weights(cfg, skip), dev)
    clean = forked_forward(eng, cfg, n, Hl, Wl, S_t, skip, dev).clone()
    dirty = forked_forward(eng, cfg, n, Hl, Wl, S_t, skip, dev, poison=True).clone()
    assert bool(torch.isfinite(dirty.float()).all()), "a NaN of the fork rows reached the output"
    assert same_bits(dirty, clean)
    cached = forked_forward(eng, cfg, n, Hl, Wl, S_t, skip, dev, poison=True, cached_context=True)
    assert bool(torch.isfinite(cached.float()).all()) and same_bits(cached, clean)


def test_same_bits_on_two_runs_and_after_switching_off(dev):
    cfg, n, Hl, Wl, S_t = _slg.FORWARD["b3"]
    skip = (1, 2)
    named = _slg.boosted_weights(cfg, skip)
    eng = engine_for(cfg, named, dev)
    first = forked_forward(eng, cfg, n, Hl, Wl, S_t, skip, dev).clone()
    assert same_bits(forked_forward(eng, cfg, n, Hl, Wl, S_t, skip, dev), first)

    def plain(e):
        text, pooled, lat = _slg.forward_inputs(cfg, n, Hl, Wl, S_t)
        e.prepare(3 * n, (Hl, Wl), S_t, len(TS))
        e.cache_modulation_params(three_groups(pooled, n).to(dev), TS)
        return e.forward_tokens(e.patchify(three_groups(lat, n).to(dev)), three_groups(text, n).to(dev, BF).contiguous(), 1)

    eng.set_skip_layers(None, 0)
    assert eng.skip_layers == () and eng.fork_rows == 0
    off = plain(eng).clone()
    never = plain(engine_for(cfg, named, dev))
    assert same_bits(off, never), "an engine whose skip layers were switched off differs from one that never had them"
    assert same_bits(off[2 * n:], off[:n]) and not same_bits(off[2 * n:], first[2 * n:])  # (the third group is then the prompt rows' plain evaluation)
    assert same_bits(off[:2 * n], first[:2 * n])  # (the live rows of a forked forward: the launches of a batch of 2 n up to the fork, all rows behind it)


def width_cfg():
    """SD3.5-medium at WIDTH (h 1536, 24 heads of 64, QK-norm), depth 3 with two dual blocks; a small positional table keeps the weights quick to draw"""
    return replace(SD3_5_MEDIUM, depth_multimodal=3, hidden_size_override=1536, dual_attention_blocks=2, max_latent_resolution=32)


def test_production_width(dev):
    """h 1536, 24 heads, depth 3, dual 2, skip (1,), latent 16 x 16, B = 3: test_mmditx_production_width_cfg_batch's gates on both row groups"""
    cfg, n, Hl, Wl, S_t, skip = width_cfg(), 1, 16, 16, 20, (1,)
    assert cfg.hidden_size == 1536 and cfg.num_heads == 24 and cfg.head_dim == 64
    named = synth_mmdit_weights(cfg, seed=1234)
    out = forked_forward(engine_for(cfg, named, dev), cfg, n, Hl, Wl, S_t, skip, dev).float().cpu()
    wf = {k: v.float() for k, v in named.items()}
    text, pooled, lat = _slg.forward_inputs(cfg, n, Hl, Wl, S_t)
    for what, rows, sk, sl in (("live rows", out[:2 * n], (), slice(None)), ("fork rows", out[2 * n:], skip, slice(0, n))):
        ref = {name: _slg._final(_slg.SkipOracle(cfg, wf, P, sk), pooled[sl], lat[sl], text[sl]) for name, P in (("fp32", Prec()), ("emu", Prec(BF)))}
        e_h, e_e = rel_l2(ref["fp32"], rows), rel_l2(ref["fp32"], ref["emu"])
        print(f"[slg] width {what}: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR {psnr(ref['fp32'], rows):.1f} dB (emulation "
              f"{psnr(ref['fp32'], ref['emu']):.1f})")
        yardstick_ok(rows, ref["emu"], ref["fp32"], f"sd3.5-medium width {what}")
        psnr_ok(rows, ref["emu"], ref["fp32"], f"sd3.5-medium width {what}")


def test_forked_forward_f16(dev):
    """case b3 with skip (1, 2) on float16_config: tests/test_gpu_f16_model.py's gate on both row groups"""
    cfg, n, Hl, Wl, S_t = _slg.FORWARD["b3"]
    skip = (1, 2)
    c16 = float16_config(cfg)
    eng = engine_for(c16, _slg.boosted_weights(cfg, skip), dev)
    out = forked_forward(eng, cfg, n, Hl, Wl, S_t, skip, dev, dt=F16)
    assert out.dtype == F16
    out = out.float().cpu()
    res = _slg.forward_refs("b3", skip, f16=True)
    gate_f16(out[:2 * n], res["full"]["emu16"], res["full"]["emubf"], res["full"]["fp32"], "slg f16 live rows")
    gate_f16(out[2 * n:], res["skip"]["emu16"], res["skip"]["emubf"], res["skip"]["fp32"], "slg f16 fork rows")
    with pytest.raises(AssertionError):
        gate_f16(out[2 * n:], res["full"]["emu16"][:n], res["full"]["emubf"][:n], res["full"]["fp32"][:n], "slg f16 fork rows against the full oracle")


def test_engine_refusals(dev):
    """every rule of dk_mmdit_set_skip_layers and of the entries it bars: the error names the rule, no state changes, the engine still works"""
    from diffusionkit_amd._lib import DkHipError
    from diffusionkit_amd.config import fp8_config
    cfg, n, Hl, Wl, S_t = _slg.FORWARD["b3"]
    skip = (1, 2)
    eng = engine_for(cfg, _slg.boosted_weights(cfg, skip), dev)
    want = forked_forward(eng, cfg, n, Hl, Wl, S_t, skip, dev).clone()
    for blocks, fork, what in (((1,), 0, "both zero"), (None, 1, "both zero"), ((4,), 1, "depth_multimodal"), ((-1,), 1, "depth_multimodal"),
                               ((1, 1), 1, "twice"), ((1,), -1, "negative")):
        with pytest.raises(DkHipError, match=what):
            eng.set_skip_layers(blocks, fork)
        assert eng.skip_layers == skip and eng.fork_rows == n
    text, pooled, lat = _slg.forward_inputs(cfg, n, Hl, Wl, S_t)
    x = randn(3 * n, S_t + (Hl // 2) * (Wl // 2), cfg.hidden_size, seed=840).to(dev, BF)
    with pytest.raises(DkHipError, match="run_blocks cannot run while skip layers are set"):
        eng.run_blocks(x, 1, 0)
    tok = eng.patchify(three_groups(lat, n).to(dev))
    txt = three_groups(text, n).to(dev, BF).contiguous()
    eng.set_skip_layers(skip, 2 * n)  # (accepted at the setter: the batch is only known at the forward)
    with pytest.raises(DkHipError, match="fork_rows"):
        eng.forward_tokens(tok, txt, 1)
    eng.set_skip_layers(skip, n)
    assert same_bits(eng.forward_tokens(tok, txt, 1), want), "the engine no longer works after refused calls"
    # the first-block cache's entries
    eng.enable_block_cache(True)
    eng.prepare(3 * n, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(three_groups(pooled, n).to(dev), TS)
    with pytest.raises(DkHipError, match="forward_head cannot run while skip layers are set"):
        eng.forward_head(tok, txt, 1)
    eng.set_skip_layers(None, 0)
    eng.forward_head(tok, txt, 1)
    eng.set_skip_layers(skip, n)
    with pytest.raises(DkHipError, match="forward_tail cannot run while skip layers are set"):
        eng.forward_tail(1, False)
    eng.set_skip_layers(None, 0)
    eng.enable_block_cache(False)
    # configurations that cannot fork: single blocks (FLUX), fp8 Linears, a reference grid, a condition width
    flux = tiny_flux()
    e = engine_for(flux, synth_mmdit_weights(flux, seed=1234), dev)
    with pytest.raises(DkHipError, match="depth_unified"):
        e.set_skip_layers((0,), 1)
    only_double = replace(flux, depth_unified=0)
    e = engine_for(only_double, synth_mmdit_weights(only_double, seed=1234), dev)
    e.prepare(1, (8, 8), 16, 1, reference_size=(8, 8))
    with pytest.raises(DkHipError, match="reference grid or a condition width"):
        e.set_skip_layers((0,), 1)
    cond = replace(only_double, condition_features=64)
    e = engine_for(cond, synth_mmdit_weights(cond, seed=1234), dev)
    with pytest.raises(DkHipError, match="reference grid or a condition width"):
        e.set_skip_layers((0,), 1)
    f8 = fp8_config(replace(tiny_flux(), depth_unified=0), "speed")
    e = engine_for(f8, synth_mmdit_weights(f8, seed=1234), dev)
    with pytest.raises(DkHipError, match="fp8_linears"):
        e.set_skip_layers((0,), 1)


# ---- the step operator --------------------------------------------------------------------------------------------------------------------------------
KGAPS = (0.5, 0.15, 0.8)  # distance of the skip prediction from the prompt's, per image: its own, unlike GAPS
SLG = 2.5
ALL_MODES = dict({"cfg": dict(mode="cfg")}, **MODES)


class Operands3(Operands):
    """tests/test_gpu_guidance.py's operands with a third row group of ``model_out``, the skip evaluation; ``step3`` runs dk_slg_cfg_step on fresh
    copies and returns (x, tokens [3 N, ...] pre-filled with the marker 7.0, hist, m)"""

    def __init__(self, dev, order, dt, hl=8, wl=12, ld_pad=0):
        super().__init__(dev, order, dt, hl, wl, ld_pad)
        text = torch.randn(N_IMG, self.s_i, self.f + ld_pad, generator=gen(2))  # (the parent's draw of the prompt rows)
        skip = text + torch.randn(N_IMG, self.s_i, self.f + ld_pad, generator=gen(9)) * torch.tensor(KGAPS).reshape(N_IMG, 1, 1)
        self.out3 = torch.cat([self.out, (skip * SCALE.reshape(N_IMG, 1, 1)).to(dt)])
        assert torch.equal(self.out3[:N_IMG], (text * SCALE.reshape(N_IMG, 1, 1)).to(dt))
        self.out3_d = self.out3.to(dev)

    def step3(self, coef=COEF, reads_h=True, writes_h=True, mask=None, sigma_next=SIGMA_NEXT, reads_m=True, writes_m=True, m="own", ws=None,
              slg_scale=SLG, **mode):
        from diffusionkit_amd import ops
        x, h = self.x.to(self.dev), self.hist.to(self.dev)
        tok = torch.full((3 * N_IMG, self.s_i, self.f), 7.0, dtype=self.dt, device=self.dev)
        mm = self.m.to(self.dev) if isinstance(m, str) else m
        kw = {} if mask is None else dict(x_orig=self.x_orig_d, noise=self.noise_d, mask=mask.to(self.dev))
        ops.slg_cfg_step(x, self.out3_d, tok, N_IMG, True, P_, self.order, SIGMA, sigma_next, CFGW, h, coef, reads_h, writes_h, slg_scale=slg_scale,
                         workspace=self.workspace() if ws is None else ws, reads_m=reads_m, writes_m=writes_m, m=mm, **mode, **kw)
        return x, tok, h, mm

    def skip_prediction(self, ft):
        where = where_of(self.order, self.hl, self.wl)
        o = torch.empty(N_IMG * self.hl * self.wl * C, dtype=torch.float64)
        o[where.reshape(-1)] = self.out3[2 * N_IMG:, :, :self.f].double().reshape(-1)
        xb = self.x.to(self.dt).float().numpy().astype(ft)
        return xb - o.reshape(N_IMG, self.hl, self.wl, C).numpy().astype(ft) * ft(SIGMA)

    def evaluate3(self, ft, coef, reads_h, reads_m, writes_m, mode, rescale=0.0, eta=0.0, norm_threshold=0.0, momentum=0.0):
        """(x', H', M') in ``ft``: float64 through ``slg_reference``; float32 through the same formulas in numpy float32 with float64 sums"""
        x, c, u = self.predictions(ft)
        k = self.skip_prediction(ft)
        m = self.m.numpy().astype(ft)
        if ft is np.float64:
            den, m_new = slg_reference(c, u, k, CFGW, SLG, mode, rescale=rescale, eta=eta, norm_threshold=norm_threshold, momentum=momentum, m=m,
                                       reads_m=reads_m, writes_m=writes_m)
        else:
            g, m_new = (u + ft(CFGW) * (c - u), m) if mode == "cfg" else guide_f32(c, u, CFGW, mode, rescale, eta, norm_threshold, momentum, m, reads_m,
                                                                                   writes_m)
            den = g + ft(SLG) * (c - k)
        cx, cd, ch, hx, hd = (ft(v) for v in coef)
        d = (x - den) / ft(SIGMA)
        xn = cx * x + cd * d + (ch * self.hist.numpy().astype(ft) if reads_h else ft(0.0))
        return xn, hx * x + hd * d, m_new


def live_tokens_ok(tok, x, dt, hl, wl, order):
    """the two live copies are the patchified updated latent, the third group keeps its marker"""
    return same_bits(tok[:2 * N_IMG], tokens_of(x, dt, N_IMG, 2, hl, wl, C, P_, order)) and bool((tok[2 * N_IMG:] == 7.0).all())


@cases
def test_slg_step_operator(dev, order, dt, hl, wl, ld_pad):
    """cfg, rescale 0.7 and apg (threshold off and on), scale 2.5, on x', H' and M': within tests/test_gpu_guidance.py's max(1e-5, 4 e32) of
    slg_reference's float64 result, each image at its own scale.  Tokens == dk_latent_to_tokens(x') in both live copies; the third group untouched."""
    o = Operands3(dev, order, dt, hl, wl, ld_pad)
    for name, mode in ALL_MODES.items():
        x, tok, h, m = o.step3(**mode)
        flags = dict(reads_h=True, reads_m=True, writes_m=True)
        rx, rh, rm = o.evaluate3(np.float64, COEF, **flags, **mode)
        fx, fh, fm = o.evaluate3(np.float32, COEF, **flags, **mode)
        for what, ref, f32, got in (("x'", rx, fx, x), ("H'", rh, fh, h)) + ((("M'", rm, fm, m),) if mode["mode"] == "apg" else ()):
            e32, e = own_scale_err(ref, f32), own_scale_err(ref, got)
            bound = max(1e-5, 4.0 * e32)
            print(f"[slg] step {name} order={order} {dt} {hl}x{wl} ld+{ld_pad} {what}: max_abs at own scale {e:.2e}, e32 {e32:.2e}, bound {bound:.2e}")
            assert e <= bound, f"{name} {what}: {e:.3e} > {bound:.3e}"
        assert live_tokens_ok(tok, x, dt, hl, wl, order), f"{name}: tokens"
        # the term is there: the guided entry on the same operands gives other bits
        assert not same_bits(x, o.step(**mode)[0]), name


@cases
def test_scale_zero_is_the_guided_step(dev, order, dt, hl, wl, ld_pad):
    """slg_scale = 0: dk_guided_cfg_step's bits for x, tokens, H and M in every mode, plain and masked, for the arbitrary row and the Euler row"""
    o = Operands3(dev, order, dt, hl, wl, ld_pad)
    for name, mode in ALL_MODES.items():
        for mask in (None, torch.rand(N_IMG, hl, wl, generator=gen(5))):
            for coef, reads_h, writes_h in ((COEF, True, True), (EULER, False, False)):
                want = o.step(coef, reads_h, writes_h, mask=mask, **mode)
                got = o.step3(coef, reads_h, writes_h, mask=mask, slg_scale=0.0, **mode)
                what = f"{name} {'masked' if mask is not None else 'plain'} {'euler' if coef is EULER else 'arbitrary'} row"
                assert same_bits(got[1][:2 * N_IMG], want[1]) and bool((got[1][2 * N_IMG:] == 7.0).all()), f"{what}: tokens"
                for tname, a, b in (("x", got[0], want[0]), ("H", got[2], want[2]), ("M", got[3], want[3])):
                    assert same_bits(a, b), f"{what}: {tname} differs from dk_guided_cfg_step's in {int((fp.bits(a) != fp.bits(b)).sum())} elements"


@pytest.mark.parametrize("name", ["cfg", "rescale", "apg-r"])
@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_slg_masked_ends(dev, name, dt):
    """m = 1: the unmasked launch bit for bit (x, tokens, H', M'); m = 0 with sigma_next = 0: the known region, x_orig, bit for bit"""
    o = Operands3(dev, 0, dt, 6, 10)
    mode = ALL_MODES[name]
    plain = o.step3(**mode)
    ones = o.step3(mask=torch.ones(1, 6, 10), **mode)
    for tname, a, b in zip(("x", "tokens", "H", "M"), ones, plain):
        assert same_bits(a, b), f"a mask of ones is not the unmasked launch: {tname}"
    x, tok, h, m = o.step3(mask=torch.zeros(N_IMG, 6, 10), sigma_next=0.0, **mode)
    assert same_bits(x, o.x_orig), "m = 0 with sigma_next = 0 does not return x_orig"
    assert live_tokens_ok(tok, o.x_orig_d, dt, 6, 10, 0)
    assert same_bits(h, plain[2]) and same_bits(m, plain[3])  # (H' and M' do not see the mask)


def test_slg_step_refusals(dev):
    """cfg_on == 0, a non-finite scale, and dk_guided_cfg_step's own refusals: dk_last_error, and nothing written"""
    from diffusionkit_amd import ops
    from diffusionkit_amd._lib import DkHipError
    o = Operands3(dev, 1, BF)
    x, h, m = o.x.to(dev), o.hist.to(dev), o.m.to(dev)
    tok = torch.full((3 * N_IMG, o.s_i, o.f), 7.0, dtype=BF, device=dev)
    ws = o.workspace(0.0)
    head = lambda cfg_on=True: (x, o.out3_d, tok, N_IMG, cfg_on, P_, 1, SIGMA, SIGMA_NEXT, CFGW, h, COEF, True, True)  # noqa: E731
    apg = dict(mode="apg", momentum=-0.5, m=m, reads_m=True, writes_m=True, workspace=ws, slg_scale=SLG)
    with pytest.raises(DkHipError, match="cfg_on"):
        ops.slg_cfg_step(*head(False), **apg)
    for bad in (fp.NAN, float("inf"), -float("inf")):
        with pytest.raises(DkHipError, match="slg_scale must be finite"):
            ops.slg_cfg_step(*head(), **dict(apg, slg_scale=bad))
        with pytest.raises(DkHipError, match="slg_scale must be finite"):
            ops.slg_cfg_step(*head(), slg_scale=bad)
    for phi in (-0.01, 1.01, fp.NAN):
        with pytest.raises(DkHipError, match=r"phi|finite"):
            ops.slg_cfg_step(*head(), mode="rescale", rescale=phi, workspace=ws, slg_scale=SLG)
    with pytest.raises(DkHipError, match="finite"):
        ops.slg_cfg_step(*head(), **dict(apg, eta=fp.NAN))
    with pytest.raises(DkHipError, match="momentum buffer"):
        ops.slg_cfg_step(*head(), **dict(apg, m=None))
    for short in (None, ws[:-1]):
        with pytest.raises(DkHipError, match="workspace"):
            ops.slg_cfg_step(*head(), mode="rescale", rescale=0.7, workspace=short, slg_scale=SLG)
    with pytest.raises(ValueError, match="cfg, rescale, apg"):
        ops.slg_cfg_step(*head(), mode="cads", workspace=ws, slg_scale=SLG)
    with pytest.raises(DkHipError, match="mask"):
        ops.slg_cfg_step(*head(), workspace=ws, slg_scale=SLG, x_orig=o.x_orig_d, noise=o.noise_d)
    with pytest.raises(DkHipError, match="3 \\* n_img"):
        ops.slg_cfg_step(x, o.out_d, tok, N_IMG, True, P_, 1, SIGMA, SIGMA_NEXT, CFGW, h, COEF, True, True, slg_scale=SLG)
    torch.cuda.synchronize(dev)
    assert same_bits(x, o.x) and same_bits(h, o.hist) and same_bits(m, o.m) and bool((tok == 7.0).all()) and bool((ws == 0.0).all()), \
        "a refused call wrote something"


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------------------------
H_IMG, W_IMG, SEED = _slg.HL * 8, _slg.WL * 8, 2
_PIPES = {}


def pipe_for(dev):
    """one SD3.5-medium tiny pipeline on the boosted weights for the whole module"""
    from diffusionkit_amd.pipeline import DiffusionPipeline
    if "sd35m" not in _PIPES:
        _PIPES["sd35m"] = DiffusionPipeline(w16=True, a16=True, shift=_slg.SHIFT, model_version=VERSION,
                                            local_ckpt={"mmdit": _slg.boosted_weights(_slg.PIPE_CFG, _slg.PIPE_SKIP)}, mmdit_config=_slg.PIPE_CFG,
                                            vae_config=tiny_vae(), vae_encoder_config=tiny_vae_encoder(), device=dev, text_len=16)
    return _PIPES["sd35m"]


def sampled(pipe, dev, seed=SEED, hw=(_slg.HL, _slg.WL), **kw):
    text, pooled = _slg.pipe_inputs()
    n = len(seed) if isinstance(seed, list) else 1
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=_slg.STEPS, cfg_weight=_slg.CFGW, latent_size=hw, seed=seed, **kw)
    assert lat.shape == (n, *hw, 16) and lat.dtype == torch.float32 and len(iter_time) == _slg.STEPS
    return lat


@functools.lru_cache(maxsize=None)
def loop_references(sampler="euler", mode="cfg", seed=SEED, masked=False):
    """the restated loop with the term on the fp32 and the bf16-emulating oracle, after process_out; ``masked``: from each oracle's own
    OracleVAEEncoder posterior sample of tests/test_gpu_inpaint.py's image (latent 8 x 16), with its half-mask blend behind every row (as
    tests/test_gpu_guidance.py's masked references)"""
    text, pooled = _slg.pipe_inputs()
    sigmas = op.get_sigmas(_slg.SHIFT, False, _slg.STEPS)
    res = {}
    for pname, P in (("fp32", Prec()), ("emu", Prec(BF))):
        full, skip = _slg.pipe_oracles(P)
        inpaint = None
        if masked:
            ecfg = tiny_vae_encoder()
            ewf = {k: v.float() for k, v in synth_vae_encoder_weights(ecfg, seed=1234 + 2).items()}
            x_orig = op.process_in(op.encode_image_to_latents(OracleVAEEncoder(ecfg, ewf, P), op.read_image_array(RGB), seed=seed), "sd3")
            x0, noise = start_state(sigmas, seed, MASK_HL, MASK_WL, x_T=x_orig)
            inpaint = (noise, x_orig, latent_mask(HALF))
        else:
            x0, _ = start_state(sigmas, seed, _slg.HL, _slg.WL)
        x = _slg.slg_loop(full, skip, sampler, x0, sigmas, text, pooled, _slg.CFGW, Prec(BF), Prec(F16), mode=mode, inpaint=inpaint,
                          slg_scale=_slg.SCALE, slg_interval=_slg.WINDOW)
        res[pname] = op.process_out(x, "sd3")
    return res


def parity(lat, res, what):
    e_h, e_e = rel_l2(res["fp32"], lat), rel_l2(res["fp32"], res["emu"])
    p_h, p_e = psnr(res["fp32"], lat), psnr(res["fp32"], res["emu"])
    print(f"[slg] pipeline {what}: rel_l2 hip {e_h:.3e} / emu {e_e:.3e}, PSNR hip {p_h:.1f} dB / emu {p_e:.1f} dB")
    yardstick_ok(lat, res["emu"], res["fp32"], what)
    assert p_h > 35.0, f"{what}: PSNR {p_h:.1f} dB"


def test_pipeline_parity(dev):
    """4 steps, CFG 5, shift 3, scale 2.5, interval (0, 0.6): the row groups go 2 n -> 3 n -> 2 n; against the restated loop"""
    pipe = pipe_for(dev)
    lat = sampled(pipe, dev, **_slg.SLG_KW)
    rec = pipe.last_skip_layer_guidance
    print(f"[slg] record {rec}")
    assert rec == {"scale": _slg.SCALE, "layers": _slg.PIPE_SKIP, "interval": _slg.WINDOW, "evals": 2}
    assert pipe.mmdit.skip_layers == () and pipe.mmdit.fork_rows == 0  # (the engine is left without skip layers)
    parity(lat, loop_references(), "euler cfg")
    off = sampled(pipe, dev)
    assert pipe.last_skip_layer_guidance is None and not same_bits(lat, off)
    moved = rel_l2(lat, off)
    print(f"[slg] pipeline: term on against term off {moved:.3f}")
    with pytest.raises(AssertionError):  # (the run without the term fails the gate: the term was applied)
        yardstick_ok(off, loop_references()["emu"], loop_references()["fp32"], "term off against the loop with the term")
    assert same_bits(sampled(pipe, dev, **dict(_slg.SLG_KW, skip_layer_interval=(0.5, 0.5))), off)  # an empty window: the plain run's bits


def test_pipeline_parity_ab2_rescale(dev):
    pipe = pipe_for(dev)
    lat = sampled(pipe, dev, sampler="ab2", guidance="rescale", **_slg.SLG_KW)
    assert pipe.last_skip_layer_guidance["evals"] == 2 and pipe.last_guidance["mode"] == "rescale"
    parity(lat, loop_references("ab2", "rescale"), "ab2 rescale")
    heun = sampled(pipe, dev, sampler="heun", **_slg.SLG_KW)
    assert bool(torch.isfinite(heun).all()) and pipe.last_skip_layer_guidance["evals"] == 4  # both evaluations of steps 1 and 2


def test_pipeline_parity_seed_list(dev):
    """seed = [2, 3]: B goes 4 -> 6 -> 4 with fork_rows 2; each image against the restated loop of its seed"""
    pipe = pipe_for(dev)
    both = sampled(pipe, dev, seed=[2, 3], **_slg.SLG_KW)
    assert pipe.last_skip_layer_guidance["evals"] == 2
    for i, s in enumerate((2, 3)):
        parity(both[i:i + 1], loop_references(seed=s), f"seed list, image {i} (seed {s})")


def test_pipeline_parity_half_mask(dev):
    """inpainting under the term: the kept half is the encoded image bit for bit; tests/test_gpu_inpaint.py's ``half_mask_gates`` on the whole.
    This case runs at that file's latent 8 x 16 (its 64 x 128 image and half mask), not at 8 x 12: ``read_image`` cuts an input image down to
    multiples of 64 pixels, so no img2img run has a latent width of 12."""
    pipe = pipe_for(dev)
    hw = (MASK_HL, MASK_WL)
    lat = sampled(pipe, dev, hw=hw, image_path=RGB, denoise=1.0, mask_path=HALF, **_slg.SLG_KW)
    assert pipe.last_skip_layer_guidance["evals"] == 2
    kept = pipe.latent_format.process_out(pipe.latent_format.process_in(pipe.encode_image_to_latents(RGB, seed=SEED)))
    w2 = MASK_WL // 2
    assert same_bits(lat[:, :, :w2], kept[:, :, :w2]) and not same_bits(lat[:, :, w2:], kept[:, :, w2:])
    assert not same_bits(lat, sampled(pipe, dev, hw=hw, image_path=RGB, denoise=1.0, mask_path=HALF))
    half_mask_gates(lat, loop_references(masked=True), "slg half mask")


def test_pipeline_float16(dev):
    """activation_dtype = "float16": the gate of tests/test_gpu_f16_model.py's pipeline test, against the restated loop on fp16-rounded weights"""
    from diffusionkit_amd.pipeline import DiffusionPipeline
    from oracle.mmdit import embed_dtype
    pipe = DiffusionPipeline(w16=True, a16=True, shift=_slg.SHIFT, model_version=VERSION, activation_dtype="float16",
                             local_ckpt={"mmdit": _slg.boosted_weights(_slg.PIPE_CFG, _slg.PIPE_SKIP)}, mmdit_config=_slg.PIPE_CFG, vae_config=tiny_vae(),
                             device=dev, text_len=16)
    assert pipe.mmdit.dtype == F16
    lat = sampled(pipe, dev, **_slg.SLG_KW)
    assert pipe.last_skip_layer_guidance["evals"] == 2
    text, pooled = _slg.pipe_inputs()
    sigmas = op.get_sigmas(_slg.SHIFT, False, _slg.STEPS)
    x0, _ = start_state(sigmas, SEED, _slg.HL, _slg.WL)
    res = {}
    for oname, (P, act, kw) in {"fp32": (Prec(), Prec(F16), dict(embed_prec=Prec(embed_dtype(_slg.PIPE_CFG)))), "emu16": (Prec(F16), Prec(F16), {}),
                                "emubf": (Prec(BF), Prec(BF), {})}.items():
        full, skip = _slg.pipe_oracles(P, f16=True, **kw)
        res[oname] = op.process_out(_slg.slg_loop(full, skip, "euler", x0, sigmas, text, pooled, _slg.CFGW, act, Prec(F16), slg_scale=_slg.SCALE,
                                                  slg_interval=_slg.WINDOW), "sd3")
    gate_f16(lat, res["emu16"], res["emubf"], res["fp32"], "slg f16 pipeline")


def test_default_is_untouched(dev, monkeypatch):
    """without the keywords and with them at None: bit-identical latents, no launch of the new entry, the engine never told, no re-prepare"""
    from diffusionkit_amd import ops, pipeline
    from diffusionkit_amd.engine import MMDiTEngine
    pipe = pipe_for(dev)
    calls = []
    monkeypatch.setattr(ops, "slg_cfg_step", lambda *a, **k: calls.append("slg_cfg_step"))
    monkeypatch.setattr(MMDiTEngine, "set_skip_layers", lambda *a, **k: calls.append("set_skip_layers"))
    monkeypatch.setattr(pipeline, "_set_rows", lambda *a, **k: calls.append("_set_rows"))
    omitted = sampled(pipe, dev)
    assert pipe.last_skip_layer_guidance is None
    assert same_bits(sampled(pipe, dev, skip_layer_guidance=None, skip_layers=None, skip_layer_interval=None), omitted)
    for s in ("heun", "ab2"):
        assert same_bits(sampled(pipe, dev, sampler=s, skip_layer_guidance=None), sampled(pipe, dev, sampler=s))
    assert same_bits(sampled(pipe, dev, guidance="rescale", skip_layer_guidance=None), sampled(pipe, dev, guidance="rescale"))
    assert calls == []


def test_pipeline_refusals(dev):
    from diffusionkit_amd.pipeline import FluxPipeline
    pipe = pipe_for(dev)
    text, pooled = _slg.pipe_inputs()
    run = lambda p=pipe, w=_slg.CFGW, **kw: p.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=2, cfg_weight=w, latent_size=(8, 8),  # noqa: E731
                                                              seed=0, **kw)
    with pytest.raises(ValueError, match="cfg_weight"):
        run(w=0.0, **_slg.SLG_KW)
    with pytest.raises(ValueError, match="block_cache"):
        run(block_cache=0.1, **_slg.SLG_KW)
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        run(**dict(_slg.SLG_KW, skip_layers=(1, 4)))
    with pytest.raises(ValueError, match="scale"):
        run(skip_layers=(1,))
    fcfg = tiny_flux()
    flux = FluxPipeline(w16=True, a16=True, mmdit_config=fcfg, vae_config=tiny_vae(), device=dev, text_len=16)
    ftext, fpooled = randn(1, 16, fcfg.token_level_text_embed_dim, seed=7), randn(1, fcfg.pooled_text_embed_dim, seed=8)
    with pytest.raises(ValueError, match="FLUX"):
        flux.denoise_latents(ftext.to(dev, BF), fpooled.to(dev, BF), num_steps=2, cfg_weight=0.0, latent_size=(8, 8), seed=0, **_slg.SLG_KW)
    assert bool(torch.isfinite(run()[0]).all())  # (the pipeline still works)


def test_generate_image_and_cli(dev, tmp_path):
    from diffusionkit_amd import cli
    pipe = pipe_for(dev)
    size = dict(num_steps=_slg.STEPS, cfg_weight=_slg.CFGW, latent_size=(_slg.HL, _slg.WL), seed=SEED, verbose=False)
    img, log = pipe.generate_image("a cat", **size)
    assert "skip_layer_guidance" not in log["denoising"]
    img, log = pipe.generate_image("a cat", **size, **_slg.SLG_KW)
    rec = log["denoising"]["skip_layer_guidance"]
    print(f"[slg] generate_image: {rec}")
    assert img.size == (W_IMG, H_IMG) and len(log["denoising"]["iter_time"]) == _slg.STEPS and rec == pipe.last_skip_layer_guidance
    assert (rec["layers"], rec["scale"], rec["interval"], rec["evals"]) == (_slg.PIPE_SKIP, _slg.SCALE, _slg.WINDOW, 2)
    over = dict(mmdit_config=_slg.PIPE_CFG, vae_config=tiny_vae(), text_len=20)
    out = tmp_path / "out.png"
    argv = ["--prompt", "a cat", "--model-version", VERSION, "--steps", "10", "--seed", "7", "--cfg", "5", "--height", "64", "--width", "64", "-o",
            str(out)]
    img, log = cli.main(argv + ["--slg-scale", "--skip-layers", "1", "2"], pipeline_overrides=over)  # the published scale and window: 0.1 < i < 2
    rec = log["denoising"]["skip_layer_guidance"]
    assert out.exists() and img.size == (64, 64)
    assert (rec["layers"], rec["scale"], rec["interval"], rec["evals"]) == ((1, 2), 2.5, (0.01, 0.2), 1)
    _, log = cli.main(argv, pipeline_overrides=over)
    assert "skip_layer_guidance" not in log["denoising"]
