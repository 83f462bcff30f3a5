"""Perturbed-attention guidance on an MI355X: the identity-attention operator (``ops.attention_identity``) against ``tests/_pag.ref_identity_attention``,
the engine's forked row group with perturbed blocks (``MMDiTEngine.set_perturbed_attention``) against ``tests/_pag.PagOracle``, and the pipeline
keywords against tests/_slg.py's restated loop with the perturbed oracle as the third model.

No tolerance is set here.  Operator: TOL_SINGLE_OP and tests/test_gpu_ops.py::test_attention's max-abs bound in bf16, tests/test_gpu_f16_ops.py's
TOL_F16 in fp16 (the fused query norm: that file's TOL_ATTN_F16 and test_attention's 6e-3, the gates of the tests it mirrors).  Model: tests/test_gpu_model.py's
``yardstick_ok`` and PSNR > 35 dB, tests/test_gpu_f16_model.py's ``gate``.  tests/test_pag_cpu.py asserts on the references alone that the mask and
the perturbed blocks move the results by several times those gates.  Every figure is printed before it is asserted.  Arithmetic parity on
synthetic weights: no checkpoint has been run."""
import ctypes as C
import functools
import math
from dataclasses import replace

import pytest
import torch

from diffusionkit_amd.config import float16_config, tiny_flux, tiny_vae, tiny_vae_encoder
from diffusionkit_amd.weights import synth_mmdit_weights
from oracle import mmdit as om
from oracle import pipeline as op
from oracle.mmdit import Prec
from tests import _footprint as fp
from tests import _pag, _slg
from tests._util import BF, TOL_SINGLE_OP, max_abs, psnr, randn, rel_l2
from tests.test_gpu_f16_model import gate as gate_f16
from tests.test_gpu_f16_ops import TOL_ATTN_F16, TOL_F16
from tests.test_gpu_inpaint import same_bits
from tests.test_gpu_model import psnr_ok, yardstick_ok
from tests.test_gpu_slg import engine_for, three_groups, width_cfg
from tests.test_samplers_cpu import start_state

pytestmark = pytest.mark.gpu

F16 = torch.float16
D = _pag.D
VERSION = "stabilityai/stable-diffusion-3.5-medium"
TS = _pag.TS
DTYPES = pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
MAX_ABS_BF16 = 0.03  # tests/test_gpu_ops.py::test_attention


# ---- the operator -------------------------------------------------------------------------------------------------------------------------------------
def plain_attention(qkv_dev, H):
    from diffusionkit_amd import ops
    if qkv_dev.dtype == BF:
        return ops.attention(qkv_dev, H, D)
    B, S, ld = qkv_dev.shape
    h = H * D
    out = torch.empty(B, S, h, dtype=F16, device=qkv_dev.device)
    ops.attention_desc_call(dtype=F16, q=qkv_dev, k=qkv_dev[:, :, h:], v=qkv_dev[:, :, 2 * h:], out=out, B=B, H=H, S=S, D=D, ld=ld, ldo=h,
                            scale=1.0 / math.sqrt(D))
    return out


def op_gate(ref, y, dt, what):
    e, m = rel_l2(ref, y.float()), max_abs(ref.float(), y.float())
    tol = TOL_SINGLE_OP if dt == BF else TOL_F16
    print(f"[pag] {what} {dt}: rel_l2 {e:.3e} (< {tol:.3e}), max_abs {m:.3e}" + (f" (< {MAX_ABS_BF16})" if dt == BF else ""))
    assert bool(torch.isfinite(y.float()).all()), what
    assert e < tol, f"{what}: rel_l2 {e:.3e}"
    if dt == BF:
        assert m < MAX_ABS_BF16, f"{what}: max_abs {m:.3e}"


def check_operator(dev, case, qkv, dt, what):
    """the launch against the masked reference; the text rows of whole text waves against the plain launch bit for bit"""
    from diffusionkit_amd import ops
    B, H, S_t, S_i = case
    qd = qkv.to(dev, dt).contiguous()
    y = ops.attention_identity(qd, H, D, S_t)
    assert y.shape == (B, S_t + S_i, H * D) and y.dtype == dt
    ref = _pag.ref_identity_attention(qkv, H, D, S_t)
    op_gate(ref, y.cpu(), dt, what)
    op_gate(ref[:, S_t:], y[:, S_t:].cpu(), dt, what + ", image rows")
    # The same kernel, the same tiles in the same order, and the mask is a no-op on a text row.  Rows below the last multiple of 32 <= F sit in
    # waves that hold text queries only and must be the plain launch's bits; the up to 31 text rows above it share a wave -- and its rescale
    # vote -- with image rows whose maxima are not the plain launch's, so they are held to the gate above instead (attention2.hip's header)
    whole = S_t // 32 * 32
    if whole:
        assert same_bits(y[:, :whole].cpu(), plain_attention(qd, H)[:, :whole].cpu()), f"{what}: text rows [0, {whole}) differ from the plain launch"


@DTYPES
@pytest.mark.parametrize("case", _pag.OP_CASES, ids=["x".join(map(str, c)) for c in _pag.OP_CASES])
def test_identity_operator(dev, case, dt):
    check_operator(dev, case, _pag.op_inputs(case, dt), dt, f"identity attention {case}")


@DTYPES
@pytest.mark.parametrize("case", _pag.LOUD_CASES, ids=["x".join(map(str, c)) for c in _pag.LOUD_CASES])
def test_identity_operator_loud_keys(dev, case, dt):
    """the image K rows x 4: a kernel that lets a masked key through is far off"""
    check_operator(dev, case, _pag.op_inputs(case, dt, loud=True), dt, f"identity attention {case}, loud keys")


@DTYPES
def test_identity_operator_spiked_own_key(dev, dt):
    """q_s . k_s dominates for every image row: the deferred rescale fires in the own tile, the last tile visited"""
    case, qkv = _pag.spiked_inputs(dt)
    B, H, S_t, S_i = case
    q, k, _ = fp.split_heads(qkv.double(), H, D)
    own = (q[:, :, S_t:] * k[:, :, S_t:]).sum(-1) / math.sqrt(D)
    text = ((q[:, :, S_t:] @ k[:, :, :S_t].transpose(-1, -2)) / math.sqrt(D)).amax(-1)
    assert float((own - text).min()) > 4.0  # (the own score exceeds every earlier one by more than the rescale threshold, for every image row)
    check_operator(dev, case, qkv, dt, "identity attention, spiked own key")


@DTYPES
def test_identity_operator_fused_query_norm(dev, dt):
    """(1, 6, S = 200, split = 77) with two norm weights, as test_attention_f16_query_qknorm_in_the_q_load: the QFUSE load under the flag"""
    from diffusionkit_amd import ops
    B, H, S, split = 1, 6, 200, 77
    h = H * D
    P = Prec(dt)
    r = lambda x: x.to(dt).float()  # noqa: E731
    qkv = r(randn(B, S, 3 * h, seed=81))
    wa, wb = r(1 + randn(D, seed=82, scale=0.1)), r(1 + randn(D, seed=83, scale=0.1))
    q = qkv[..., :h].reshape(B, S, H, D)
    qn = torch.cat([om.rms_norm(q[:, :split], wa, 1e-6, P), om.rms_norm(q[:, split:], wb, 1e-6, P)], dim=1).reshape(B, S, h)
    ref = _pag.ref_identity_attention(torch.cat([qn, qkv[..., h:]], dim=-1), H, D, split)
    y = ops.attention_identity(qkv.to(dev, dt).contiguous(), H, D, split, qn=(wa.to(dev, dt), wb.to(dev, dt), split))
    e, m = rel_l2(ref, y.float().cpu()), max_abs(ref.float(), y.float().cpu())
    tol = 6e-3 if dt == BF else TOL_ATTN_F16
    print(f"[pag] identity attention (1, 6, 200) fused query norm {dt}: rel_l2 {e:.3e} (< {tol:.3e}), max_abs {m:.3e}")
    assert e < tol and (dt != BF or m < MAX_ABS_BF16)
    plan = ops.attention_identity_plan(split, dtype=dt, q=0x10000, k=0x20000, v=0x30000, out=0x40000, B=B, H=H, S=S, D=D, ld=3 * h, ldo=h,
                                       scale=0.125, qn_a=0x50000, qn_b=0x60000, qn_split=split, qn_eps=1e-6)
    assert (plan.kernel, plan.qfuse, plan.launches) == (4, 1, 1)


@DTYPES
def test_identity_operator_footprint(dev, dt):
    """the packed qkv inside NaN margins, batch row 1 poisoned: batch row 0 keeps the clean run's bits, nothing around the output is written.  The
    last batch row ends in a ragged own tile: a read at or beyond its row S would meet the margin's NaN (in the clean run: a NaN output)."""
    from diffusionkit_amd import ops
    B, H, S_t, S_i = 2, 2, 77, 150
    S, h = S_t + S_i, H * D
    qkv = _pag.op_inputs((B, H, S_t, S_i), dt, seed=32)

    def run(t):
        view, _ = fp.guarded(t.to(dev, dt), 64)
        y = ops.attention_identity(view, H, D, S_t)
        torch.cuda.synchronize(dev)
        return y.cpu()

    clean = run(qkv)
    dirty_in = qkv.clone()
    dirty_in[1] = fp.NAN
    expect = torch.zeros(B, S, h, dtype=torch.bool)
    expect[1] = True
    fp.assert_footprint(clean, run(dirty_in), expect, f"identity attention footprint {dt}")
    op_gate(_pag.ref_identity_attention(qkv, H, D, S_t), clean, dt, "identity attention inside NaN margins")


def test_identity_operator_refusals(dev):
    """every rule of the route, at the launch: dk_last_error names it and the output keeps its fill"""
    from diffusionkit_amd import _lib, ops
    lib = _lib.load()
    B, H, S = 1, 2, 100
    for dt, entry in ((BF, "dk_attention_identity_bf16"), (F16, "dk_attention_identity_f16")):
        for Dh, F, extra, what in ((128, 20, {}, "head_dim"), (64, 0, {}, "ident_from"), (64, S, {}, "ident_from"), (64, -3, {}, "ident_from"),
                                   (64, 20, "bias", "score bias"), (64, 20, "O8", "MX-fp8")):
            h = H * Dh
            qkv = torch.ones(B, S, 3 * h, dtype=dt, device=dev)
            out = torch.full((B, S, h), fp.SENTINEL, dtype=dt, device=dev)
            kw = dict(q=qkv, k=qkv[:, :, h:], v=qkv[:, :, 2 * h:], out=out, B=B, H=H, S=S, D=Dh, ld=3 * h, ldo=h, scale=0.125)
            if extra == "bias":
                kw.update(bias=torch.zeros(H, S, 128, dtype=dt, device=dev), bias_head_stride=S * 128, ldb=128)
            if extra == "O8":
                kw.update(O8=torch.zeros(B * S, h, dtype=torch.uint8, device=dev), O8_scales=torch.zeros(4096, dtype=torch.uint8, device=dev), o8_ld=h,
                          o8_rows=B * S)
            d = ops._fill(_lib.dk_attention_desc, kw)
            with pytest.raises(_lib.DkHipError, match=what):
                _lib.check(getattr(lib, entry)(C.byref(d), F, None), entry)
            torch.cuda.synchronize(dev)
            assert bool((out == fp.SENTINEL).all()), f"{entry} D {Dh} F {F} {extra}: a refused call wrote its output"


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------------------
def pag_forward(eng, cfg, n, Hl, Wl, S_t, pag, dev, dt=BF, poison=False, cached_context=False):
    """tests/test_gpu_slg.py's ``forked_forward`` with the fork rows perturbed in ``pag`` instead of sitting blocks out"""
    text, pooled, lat = _slg.forward_inputs(cfg, n, Hl, Wl, S_t)
    eng.prepare(3 * n, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(three_groups(pooled, n).to(dev), TS)
    eng.set_perturbed_attention(pag, n)
    tok = eng.patchify(three_groups(lat, n).to(dev))
    text = three_groups(text, n).to(dev, dt).contiguous()
    if poison:
        tok[2 * n:] = fp.NAN
        text[2 * n:] = fp.NAN
    if cached_context:
        eng.cache_context(text)
        text = None
    return eng.forward_tokens(tok, text, 1)


FORWARD_CASES = [(c, s) for c in ("b3", "heads6_35tok") for s in _pag.PAG_SETS]


@pytest.mark.parametrize("case,pag", FORWARD_CASES, ids=[f"{c}-pag{'_'.join(map(str, s))}" for c, s in FORWARD_CASES])
def test_forked_forward(dev, case, pag):
    """rows [0, 2 n) against the full oracle, the fork rows against the perturbed oracle -- and the fork rows must FAIL the gate against the full
    oracle: otherwise the perturbation was not applied"""
    cfg, n, Hl, Wl, S_t = _pag.FORWARD[case]
    eng = engine_for(cfg, _pag.boosted_weights(cfg, pag), dev)
    out = pag_forward(eng, cfg, n, Hl, Wl, S_t, pag, dev).float().cpu()
    assert out.shape[0] == 3 * n and bool(torch.isfinite(out).all())
    res = _pag.forward_refs(case, pag)
    live, fork = out[:2 * n], out[2 * n:]
    print(f"[pag] forward {case} pag {pag}: live rows hip-vs-fp32 {rel_l2(res['full']['fp32'], live):.3e} (emulation "
          f"{rel_l2(res['full']['fp32'], res['full']['emu']):.3e}), PSNR {psnr(res['full']['fp32'], live):.1f} dB; fork rows hip-vs-pag-fp32 "
          f"{rel_l2(res['pag']['fp32'], fork):.3e} (emulation {rel_l2(res['pag']['fp32'], res['pag']['emu']):.3e}), PSNR "
          f"{psnr(res['pag']['fp32'], fork):.1f} dB; fork rows against the FULL oracle {rel_l2(res['full']['fp32'][:n], fork):.3e}")
    yardstick_ok(live, res["full"]["emu"], res["full"]["fp32"], f"{case} live rows")
    yardstick_ok(fork, res["pag"]["emu"], res["pag"]["fp32"], f"{case} fork rows")
    assert psnr(res["full"]["fp32"], live) > 35.0 and psnr(res["pag"]["fp32"], fork) > 35.0
    with pytest.raises(AssertionError):
        yardstick_ok(fork, res["full"]["emu"][:n], res["full"]["fp32"][:n], "fork rows against the full oracle")


def test_fork_rows_are_never_read(dev):
    cfg, n, Hl, Wl, S_t = _pag.FORWARD["heads6_35tok"]
    pag = (1, 2)
    eng = engine_for(cfg, _pag.boosted_weights(cfg, pag), dev)
    clean = pag_forward(eng, cfg, n, Hl, Wl, S_t, pag, dev).clone()
    dirty = pag_forward(eng, cfg, n, Hl, Wl, S_t, pag, dev, poison=True).clone()
    assert bool(torch.isfinite(dirty.float()).all()), "a NaN of the fork rows reached the output"
    assert same_bits(dirty, clean)
    cached = pag_forward(eng, cfg, n, Hl, Wl, S_t, pag, dev, poison=True, cached_context=True)
    assert bool(torch.isfinite(cached.float()).all()) and same_bits(cached, clean)


def test_same_bits_on_two_runs_and_after_switching_off(dev):
    cfg, n, Hl, Wl, S_t = _pag.FORWARD["b3"]
    pag = (1, 2)
    named = _pag.boosted_weights(cfg, pag)
    eng = engine_for(cfg, named, dev)
    first = pag_forward(eng, cfg, n, Hl, Wl, S_t, pag, dev).clone()
    assert same_bits(pag_forward(eng, cfg, n, Hl, Wl, S_t, pag, dev), first)

    def plain(e):
        text, pooled, lat = _slg.forward_inputs(cfg, n, Hl, Wl, S_t)
        e.prepare(3 * n, (Hl, Wl), S_t, len(TS))
        e.cache_modulation_params(three_groups(pooled, n).to(dev), TS)
        return e.forward_tokens(e.patchify(three_groups(lat, n).to(dev)), three_groups(text, n).to(dev, BF).contiguous(), 1)

    eng.set_perturbed_attention(None, 0)
    assert eng.perturbed_attention == () and eng.fork_rows == 0
    off = plain(eng).clone()
    never = plain(engine_for(cfg, named, dev))
    assert same_bits(off, never), "an engine whose perturbed attention was switched off differs from one that never had it"
    assert same_bits(off[2 * n:], off[:n]) and not same_bits(off[2 * n:], first[2 * n:])
    assert same_bits(off[:2 * n], first[:2 * n])  # (the live rows of a forked forward: the launches of a batch of 2 n up to the fork, all rows behind it)


def test_forked_forward_f16(dev):
    cfg, n, Hl, Wl, S_t = _pag.FORWARD["b3"]
    pag = (1, 2)
    eng = engine_for(float16_config(cfg), _pag.boosted_weights(cfg, pag), dev)
    out = pag_forward(eng, cfg, n, Hl, Wl, S_t, pag, dev, dt=F16)
    assert out.dtype == F16
    out = out.float().cpu()
    res = _pag.forward_refs("b3", pag, f16=True)
    gate_f16(out[:2 * n], res["full"]["emu16"], res["full"]["emubf"], res["full"]["fp32"], "pag f16 live rows")
    gate_f16(out[2 * n:], res["pag"]["emu16"], res["pag"]["emubf"], res["pag"]["fp32"], "pag f16 fork rows")
    with pytest.raises(AssertionError):
        gate_f16(out[2 * n:], res["full"]["emu16"][:n], res["full"]["emubf"][:n], res["full"]["fp32"][:n], "pag f16 fork rows against the full oracle")


def test_production_width(dev):
    """SD3-medium's h = 1536 with 24 heads at depth 2, S_t = 154, a 32 x 32 latent (S = 154 + 256), B = 3, block 1 perturbed"""
    cfg, n, Hl, Wl, S_t, pag = replace(width_cfg(), depth_multimodal=2), 1, 32, 32, 154, (1,)
    assert cfg.hidden_size == 1536 and cfg.num_heads == 24 and cfg.head_dim == 64
    named = synth_mmdit_weights(cfg, seed=1234)
    out = pag_forward(engine_for(cfg, named, dev), cfg, n, Hl, Wl, S_t, pag, dev).float().cpu()
    wf = {k: v.float() for k, v in named.items()}
    text, pooled, lat = _slg.forward_inputs(cfg, n, Hl, Wl, S_t)
    for what, rows, pg, sl in (("live rows", out[:2 * n], (), slice(None)), ("fork rows", out[2 * n:], pag, slice(0, n))):
        ref = {name: _slg._final(_pag.PagOracle(cfg, wf, P, pg), pooled[sl], lat[sl], text[sl]) for name, P in (("fp32", Prec()), ("emu", Prec(BF)))}
        print(f"[pag] width {what}: hip-vs-fp32 {rel_l2(ref['fp32'], rows):.3e} (emulation {rel_l2(ref['fp32'], ref['emu']):.3e}), PSNR "
              f"{psnr(ref['fp32'], rows):.1f} dB (emulation {psnr(ref['fp32'], ref['emu']):.1f})")
        yardstick_ok(rows, ref["emu"], ref["fp32"], f"sd3-medium width {what}")
        psnr_ok(rows, ref["emu"], ref["fp32"], f"sd3-medium width {what}")


def test_engine_refusals(dev):
    """every rule of dk_mmdit_set_perturbed_attention and of the entries it bars: the error names the rule, no state changes, the engine still works"""
    from diffusionkit_amd._lib import DkHipError
    from diffusionkit_amd.config import fp8_config
    cfg, n, Hl, Wl, S_t = _pag.FORWARD["b3"]
    pag = (1, 2)
    eng = engine_for(cfg, _pag.boosted_weights(cfg, pag), dev)
    want = pag_forward(eng, cfg, n, Hl, Wl, S_t, pag, dev).clone()
    for blocks, fork, what in (((1,), 0, "both zero"), (None, 1, "both zero"), ((4,), 1, "depth_multimodal"), ((-1,), 1, "depth_multimodal"),
                               ((1, 1), 1, "twice"), ((1,), -1, "negative")):
        with pytest.raises(DkHipError, match=what):
            eng.set_perturbed_attention(blocks, fork)
        assert eng.perturbed_attention == pag and eng.fork_rows == n
    with pytest.raises(DkHipError, match="perturbed attention is set"):
        eng.set_skip_layers((1,), n)
    assert eng.skip_layers == ()
    text, pooled, lat = _slg.forward_inputs(cfg, n, Hl, Wl, S_t)
    x = randn(3 * n, S_t + (Hl // 2) * (Wl // 2), cfg.hidden_size, seed=840).to(dev, BF)
    with pytest.raises(DkHipError, match="run_blocks cannot run while perturbed attention is set"):
        eng.run_blocks(x, 1, 0)
    tok = eng.patchify(three_groups(lat, n).to(dev))
    txt = three_groups(text, n).to(dev, BF).contiguous()
    eng.set_perturbed_attention(pag, 2 * n)  # (accepted at the setter: the batch is only known at the forward)
    with pytest.raises(DkHipError, match="fork_rows"):
        eng.forward_tokens(tok, txt, 1)
    eng.set_perturbed_attention(pag, n)
    assert same_bits(eng.forward_tokens(tok, txt, 1), want), "the engine no longer works after refused calls"
    eng.enable_block_cache(True)
    eng.prepare(3 * n, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(three_groups(pooled, n).to(dev), TS)
    with pytest.raises(DkHipError, match="forward_head cannot run while perturbed attention is set"):
        eng.forward_head(tok, txt, 1)
    eng.set_perturbed_attention(None, 0)
    eng.forward_head(tok, txt, 1)
    eng.set_perturbed_attention(pag, n)
    with pytest.raises(DkHipError, match="forward_tail cannot run while perturbed attention is set"):
        eng.forward_tail(1, False)
    eng.set_perturbed_attention(None, 0)
    eng.enable_block_cache(False)
    eng.set_skip_layers((1,), n)
    with pytest.raises(DkHipError, match="skip layers are set"):
        eng.set_perturbed_attention(pag, n)
    assert eng.perturbed_attention == () and eng.fork_rows == n
    eng.set_skip_layers(None, 0)
    flux = tiny_flux()
    e = engine_for(flux, synth_mmdit_weights(flux, seed=1234), dev)
    with pytest.raises(DkHipError, match="depth_unified"):
        e.set_perturbed_attention((0,), 1)
    only_double = replace(flux, depth_unified=0)
    e = engine_for(only_double, synth_mmdit_weights(only_double, seed=1234), dev)
    e.prepare(1, (8, 8), 16, 1, reference_size=(8, 8))
    with pytest.raises(DkHipError, match="reference grid or a condition width"):
        e.set_perturbed_attention((0,), 1)
    cond = replace(only_double, condition_features=64)
    e = engine_for(cond, synth_mmdit_weights(cond, seed=1234), dev)
    with pytest.raises(DkHipError, match="reference grid or a condition width"):
        e.set_perturbed_attention((0,), 1)
    f8 = fp8_config(replace(tiny_flux(), depth_unified=0), "speed")
    e = engine_for(f8, synth_mmdit_weights(f8, seed=1234), dev)
    with pytest.raises(DkHipError, match="fp8_linears"):
        e.set_perturbed_attention((0,), 1)


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------------------------
H_IMG, W_IMG, SEED = _slg.HL * 8, _slg.WL * 8, 2
_PIPES = {}


def pipe_for(dev):
    from diffusionkit_amd.pipeline import DiffusionPipeline
    if "sd35m" not in _PIPES:
        _PIPES["sd35m"] = DiffusionPipeline(w16=True, a16=True, shift=_slg.SHIFT, model_version=VERSION,
                                            local_ckpt={"mmdit": _pag.boosted_weights(_pag.PIPE_CFG, _pag.PIPE_PAG)}, mmdit_config=_pag.PIPE_CFG,
                                            vae_config=tiny_vae(), vae_encoder_config=tiny_vae_encoder(), device=dev, text_len=16)
    return _PIPES["sd35m"]


def sampled(pipe, dev, seed=SEED, hw=(_slg.HL, _slg.WL), **kw):
    text, pooled = _slg.pipe_inputs()
    n = len(seed) if isinstance(seed, list) else 1
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=_slg.STEPS, cfg_weight=_slg.CFGW, latent_size=hw, seed=seed, **kw)
    assert lat.shape == (n, *hw, 16) and lat.dtype == torch.float32 and len(iter_time) == _slg.STEPS
    return lat


@functools.lru_cache(maxsize=None)
def loop_references(sampler="euler", mode="cfg", seed=SEED, scale=_pag.SCALE):
    """tests/_slg.slg_loop with the perturbed oracle as the third model, on the fp32 and the bf16-emulating oracle, after process_out"""
    text, pooled = _slg.pipe_inputs()
    sigmas = op.get_sigmas(_slg.SHIFT, False, _slg.STEPS)
    res = {}
    for pname, P in (("fp32", Prec()), ("emu", Prec(BF))):
        full, pert = _pag.pipe_oracles(P)
        x0, _ = start_state(sigmas, seed, _slg.HL, _slg.WL)
        x = _slg.slg_loop(full, pert, sampler, x0, sigmas, text, pooled, _slg.CFGW, Prec(BF), Prec(F16), mode=mode, slg_scale=scale,
                          slg_interval=_slg.WINDOW)
        res[pname] = op.process_out(x, "sd3")
    return res


def parity(lat, res, what):
    e_h, e_e = rel_l2(res["fp32"], lat), rel_l2(res["fp32"], res["emu"])
    p_h, p_e = psnr(res["fp32"], lat), psnr(res["fp32"], res["emu"])
    print(f"[pag] pipeline {what}: rel_l2 hip {e_h:.3e} / emu {e_e:.3e}, PSNR hip {p_h:.1f} dB / emu {p_e:.1f} dB")
    yardstick_ok(lat, res["emu"], res["fp32"], what)
    psnr_ok(lat, res["emu"], res["fp32"], what)  # (on these boosted weights the bf16-emulating loop itself ends near 34 dB: the rule's second arm)


def test_pipeline_parity(dev):
    """4 steps, CFG 5, shift 3, scale 2.5, interval (0, 0.6): the row groups go 2 n -> 3 n -> 2 n; against the restated loop"""
    pipe = pipe_for(dev)
    lat = sampled(pipe, dev, **_pag.PAG_KW)
    rec = pipe.last_perturbed_attention_guidance
    print(f"[pag] record {rec}")
    assert rec == {"scale": _pag.SCALE, "layers": _pag.PIPE_PAG, "interval": _slg.WINDOW, "evals": 2}
    assert pipe.mmdit.perturbed_attention == () and pipe.mmdit.fork_rows == 0  # (the engine is left without the setting)
    parity(lat, loop_references(), "euler cfg")
    off = sampled(pipe, dev)
    assert pipe.last_perturbed_attention_guidance is None and not same_bits(lat, off)
    print(f"[pag] pipeline: term on against term off {rel_l2(lat, off):.3f}")
    with pytest.raises(AssertionError):  # (the run without the term fails the gate: the term was applied)
        yardstick_ok(off, loop_references()["emu"], loop_references()["fp32"], "term off against the loop with the term")
    assert same_bits(sampled(pipe, dev, **dict(_pag.PAG_KW, pag_interval=(0.5, 0.5))), off)  # an empty window: the plain run's bits


def test_pipeline_scale_zero_is_the_guided_loop(dev):
    pipe = pipe_for(dev)
    zero = sampled(pipe, dev, **dict(_pag.PAG_KW, pag_scale=0.0))
    assert pipe.last_perturbed_attention_guidance["evals"] == 2
    assert same_bits(zero, sampled(pipe, dev))


def test_pipeline_parity_ab2_rescale(dev):
    pipe = pipe_for(dev)
    lat = sampled(pipe, dev, sampler="ab2", guidance="rescale", **_pag.PAG_KW)
    assert pipe.last_perturbed_attention_guidance["evals"] == 2 and pipe.last_guidance["mode"] == "rescale"
    parity(lat, loop_references("ab2", "rescale"), "ab2 rescale")


def test_pipeline_parity_seed_list(dev):
    pipe = pipe_for(dev)
    both = sampled(pipe, dev, seed=[2, 3], **_pag.PAG_KW)
    assert pipe.last_perturbed_attention_guidance["evals"] == 2
    for i, s in enumerate((2, 3)):
        parity(both[i:i + 1], loop_references(seed=s), f"seed list, image {i} (seed {s})")


def test_default_is_untouched(dev, monkeypatch):
    """without the keywords and with them at None: bit-identical latents, the engine never told"""
    from diffusionkit_amd import ops, pipeline
    from diffusionkit_amd.engine import MMDiTEngine
    pipe = pipe_for(dev)
    calls = []
    monkeypatch.setattr(ops, "slg_cfg_step", lambda *a, **k: calls.append("slg_cfg_step"))
    monkeypatch.setattr(MMDiTEngine, "set_perturbed_attention", lambda *a, **k: calls.append("set_perturbed_attention"))
    monkeypatch.setattr(pipeline, "_set_rows", lambda *a, **k: calls.append("_set_rows"))
    omitted = sampled(pipe, dev)
    assert pipe.last_perturbed_attention_guidance is None
    assert same_bits(sampled(pipe, dev, pag_scale=None, pag_layers=None, pag_interval=None), omitted)
    assert same_bits(sampled(pipe, dev, sampler="ab2", pag_scale=None), sampled(pipe, dev, sampler="ab2"))
    assert calls == []


def test_pipeline_refusals(dev):
    from diffusionkit_amd.pipeline import FluxPipeline
    pipe = pipe_for(dev)
    text, pooled = _slg.pipe_inputs()
    run = lambda p=pipe, w=_slg.CFGW, **kw: p.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=2, cfg_weight=w, latent_size=(8, 8),  # noqa: E731
                                                              seed=0, **kw)
    for kw, what in ((dict(w=0.0, **_pag.PAG_KW), "cfg_weight"), (dict(block_cache=0.1, **_pag.PAG_KW), "block_cache"),
                     (dict(_pag.PAG_KW, pag_layers=(1, 4)), r"\[0, 4\)"), (dict(pag_layers=(1,)), "pag_scale"), (dict(pag_scale=3.0), "pag_layers"),
                     (dict(_pag.PAG_KW, **_slg.SLG_KW), "skip-layer guidance"), (dict(_pag.PAG_KW, pag_scale=-1.0), ">= 0")):
        with pytest.raises(ValueError, match=what):
            run(**kw)
    fcfg = tiny_flux()
    flux = FluxPipeline(w16=True, a16=True, mmdit_config=fcfg, vae_config=tiny_vae(), device=dev, text_len=16)
    ftext, fpooled = randn(1, 16, fcfg.token_level_text_embed_dim, seed=7), randn(1, fcfg.pooled_text_embed_dim, seed=8)
    with pytest.raises(ValueError, match="FLUX"):
        flux.denoise_latents(ftext.to(dev, BF), fpooled.to(dev, BF), num_steps=2, cfg_weight=0.0, latent_size=(8, 8), seed=0, **_pag.PAG_KW)
    assert pipe.mmdit.perturbed_attention == () and bool(torch.isfinite(run()[0]).all())  # (the pipeline still works)


def test_pipeline_float16_and_every_guided_row(dev):
    """activation_dtype = "float16" against the restated loop on fp16-rounded weights (tests/test_gpu_f16_model.py's gate), with pag_interval None:
    every guided evaluation, the first step included, carries the term"""
    from diffusionkit_amd.pipeline import DiffusionPipeline
    from oracle.mmdit import embed_dtype
    pipe = DiffusionPipeline(w16=True, a16=True, shift=_slg.SHIFT, model_version=VERSION, activation_dtype="float16",
                             local_ckpt={"mmdit": _pag.boosted_weights(_pag.PIPE_CFG, _pag.PIPE_PAG)}, mmdit_config=_pag.PIPE_CFG, vae_config=tiny_vae(),
                             device=dev, text_len=16)
    assert pipe.mmdit.dtype == F16
    lat = sampled(pipe, dev, **dict(_pag.PAG_KW, pag_interval=None))
    assert pipe.last_perturbed_attention_guidance == {"scale": _pag.SCALE, "layers": _pag.PIPE_PAG, "interval": None, "evals": _slg.STEPS}
    text, pooled = _slg.pipe_inputs()
    sigmas = op.get_sigmas(_slg.SHIFT, False, _slg.STEPS)
    x0, _ = start_state(sigmas, SEED, _slg.HL, _slg.WL)
    res = {}
    for oname, (P, act, kw) in {"fp32": (Prec(), Prec(F16), dict(embed_prec=Prec(embed_dtype(_pag.PIPE_CFG)))), "emu16": (Prec(F16), Prec(F16), {}),
                                "emubf": (Prec(BF), Prec(BF), {})}.items():
        full, pert = _pag.pipe_oracles(P, f16=True, **kw)
        res[oname] = op.process_out(_slg.slg_loop(full, pert, "euler", x0, sigmas, text, pooled, _slg.CFGW, act, Prec(F16), slg_scale=_pag.SCALE,
                                                  slg_interval=(-1.0, 2.0)), "sd3")  # (a window that holds every step, the first included)
    gate_f16(lat, res["emu16"], res["emubf"], res["fp32"], "pag f16 pipeline, every guided row")


def test_generate_image_and_cli(dev, tmp_path):
    from diffusionkit_amd import cli
    pipe = pipe_for(dev)
    size = dict(num_steps=_slg.STEPS, cfg_weight=_slg.CFGW, latent_size=(_slg.HL, _slg.WL), seed=SEED, verbose=False)
    img, log = pipe.generate_image("a cat", **size)
    assert "perturbed_attention_guidance" not in log["denoising"]
    img, log = pipe.generate_image("a cat", **size, **_pag.PAG_KW)
    rec = log["denoising"]["perturbed_attention_guidance"]
    print(f"[pag] generate_image: {rec}")
    assert img.size == (W_IMG, H_IMG) and rec == pipe.last_perturbed_attention_guidance
    assert (rec["layers"], rec["scale"], rec["interval"], rec["evals"]) == (_pag.PIPE_PAG, _pag.SCALE, _slg.WINDOW, 2)
    over = dict(mmdit_config=_pag.PIPE_CFG, vae_config=tiny_vae(), text_len=20)
    out = tmp_path / "out.png"
    argv = ["--prompt", "a cat", "--model-version", VERSION, "--steps", "4", "--seed", "7", "--cfg", "5", "--height", "64", "--width", "64", "-o", str(out)]
    img, log = cli.main(argv + ["--pag-scale", "3", "--pag-layers", "1", "2", "--pag-interval", "0", "0.6"], pipeline_overrides=over)
    rec = log["denoising"]["perturbed_attention_guidance"]
    assert out.exists() and img.size == (64, 64)
    assert (rec["layers"], rec["scale"], rec["interval"], rec["evals"]) == ((1, 2), 3.0, (0.0, 0.6), 2)
    _, log = cli.main(argv, pipeline_overrides=over)
    assert "perturbed_attention_guidance" not in log["denoising"]
