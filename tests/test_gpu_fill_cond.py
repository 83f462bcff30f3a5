"""Channel-concatenated conditioning (FLUX.1 Fill / Canny / Depth) on the GPU: the two operators bit for bit against their statements, the
engine against the oracle of tests/_fillcond.py -- its output, the EFFECT of the condition (so that an engine that ignores or misorders it
fails), zeroed condition columns against a plain engine -- broadcast, hoist, "off means off", poisoned state, the first-block cache, fp8, and
the pipeline.

Arithmetic parity only: no Fill / Canny / Depth checkpoint exists where this suite runs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from diffusionkit_amd import _lib, ops
from diffusionkit_amd.config import fp8_config, tiny_flux, tiny_vae, tiny_vae_encoder
from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights, synth_vae_encoder_weights
from oracle import fp8 as o8
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec, affine_transform
from oracle.vae import OracleVAEEncoder, sample_latent
from tests import _engine_state as es
from tests import _fillcond as fc
from tests import _footprint as fp
from tests._util import BF, TOL_SINGLE_OP, psnr, randn, rel_l2

pytestmark = pytest.mark.gpu

bits = fp.bits
TS, STEP = fc.TIMESTEPS, fc.STEP
RUN_IDS = [f"{name}-{width}" for name, width in fc.RUNS]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def yardstick_ok(hip, emu, exact, what=""):
    """the project's model-level rule (tests/test_gpu_model.py): hip-vs-fp32 <= 2 * emu-vs-fp32 + 2e-3 (relative L2)"""
    e_h, e_e = rel_l2(exact, hip), rel_l2(exact, emu)
    print(f"[condition] {what}: rel_l2 hip-vs-fp32 {e_h:.3e}, emu-vs-fp32 {e_e:.3e}")
    assert e_h <= 2.0 * e_e + 2e-3, f"{what}: hip-vs-fp32 {e_h:.3e} > 2*emu-vs-fp32 {e_e:.3e} + 2e-3"
    return e_h, e_e


def psnr_ok(hip, emu, exact, what=""):
    """tests/test_gpu_model.py: >= 35 dB against the fp32 oracle, or within 1.5 dB of what the bf16-emulating oracle reaches"""
    p_h, p_e = psnr(exact, hip), psnr(exact, emu)
    print(f"[condition] {what}: PSNR hip {p_h:.1f} dB, bf16-emulating oracle {p_e:.1f} dB")
    assert p_h > min(35.0, p_e - 1.5), f"{what}: PSNR hip {p_h:.1f} dB, bf16-emulating oracle {p_e:.1f} dB"


# ---- 1. the token kernel ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain_engine(dev):
    from diffusionkit_amd.engine import MMDiTEngine
    cfg = tiny_flux()
    return MMDiTEngine(cfg, pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234), dev))


# (n, Hl, Wl, n_mask; n_mask None: the null-mask form): one token, several blocks of threads, one mask for two images, 768 tokens
@pytest.mark.parametrize("n,Hl,Wl,n_mask", [(1, 2, 2, 1), (2, 6, 10, 1), (2, 6, 10, 2), (1, 64, 48, 1), (2, 6, 10, None)])
def test_condition_tokens_bit_for_bit(dev, n, Hl, Wl, n_mask):
    z = torch.randn(n, Hl, Wl, 16, generator=torch.Generator().manual_seed(Hl * Wl + n)) * 3.0  # (fp32 values that bf16 must round)
    mask = None if n_mask is None else fc.make_mask(n_mask, 8 * Hl, 8 * Wl, seed=Hl)
    if mask is not None:
        vals = set(np.unique(mask.numpy()).tolist())
        assert {0, 255} <= vals and len(vals) > 2
    width = 64 + (0 if mask is None else 256)
    n_tok = n * (Hl // 2) * (Wl // 2) * width
    slab = torch.full((n_tok + 4096,), float("nan"), dtype=BF, device=dev)
    z_dev, mask_dev = z.to(dev), None if mask is None else mask.to(dev)
    got = ops.fill_condition_tokens(z_dev, mask_dev)
    assert got.shape == (n, (Hl // 2) * (Wl // 2), width) and got.dtype == BF
    assert same_bits(got.cpu(), fc.condition_tokens_reference(z, mask)), "tokens != the reshape statement"
    assert same_bits(got[..., :64].contiguous(), plain_engine(dev).patchify(z_dev)), "latent columns != dk_latent_to_tokens"
    if mask is not None:  # a 2-D mask is the one-mask form
        assert same_bits(ops.fill_condition_tokens(z.to(dev), mask[0].to(dev)).cpu(), fc.condition_tokens_reference(z, mask[:1]))
    # the launch writes its tokens and nothing behind them
    out = slab[:n_tok].view(got.shape)
    _lib.check(_lib.load().dk_fill_condition_tokens(z_dev.data_ptr(), None if mask is None else mask_dev.data_ptr(), out.data_ptr(), n,
                                                    0 if mask is None else mask.shape[0], Hl, Wl, 16, 2, None), "dk_fill_condition_tokens")
    torch.cuda.synchronize()
    assert same_bits(out, got) and bool(torch.isnan(slab[n_tok:].float()).all()), "the slack behind the tokens was written"


def test_condition_tokens_refuses(dev):
    z = torch.zeros(2, 4, 6, 16, device=dev)
    with pytest.raises(ValueError, match="mask"):
        ops.fill_condition_tokens(z, torch.zeros(3, 32, 48, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="mask"):
        ops.fill_condition_tokens(z, torch.zeros(32, 40, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="patch size"):
        ops.fill_condition_tokens(torch.zeros(1, 3, 4, 16, device=dev))


# ---- 2. the masked-out image -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_mask", [(1, 1), (3, 1), (3, 3)])
def test_image_mask_out(dev, n, n_mask):
    H, W = 24, 40
    rng = np.random.RandomState(n * 7 + n_mask)
    image = rng.randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
    image[0, 0, :6] = [[0, 0, 0], [255, 255, 255], [1, 127, 128], [254, 2, 3], [85, 170, 51], [17, 34, 68]]
    mask = fc.make_mask(n_mask, H, W, seed=n).numpy()
    a = (image.astype(np.float32) / np.float32(255)) * np.float32(2) - np.float32(1.0)
    m = mask.astype(np.float32) / np.float32(255)
    want = a * (np.float32(1) - m)[..., None]
    assert want.dtype == np.float32
    got = ops.image_mask_out(torch.from_numpy(image).to(dev), torch.from_numpy(mask).to(dev))
    assert got.shape == (n, H, W, 3) and got.dtype == torch.float32
    assert same_bits(got.cpu(), torch.from_numpy(want)), "dk_image_mask_out_f32 != the numpy float32 statement"
    if n_mask == 1:
        assert same_bits(ops.image_mask_out(torch.from_numpy(image).to(dev), torch.from_numpy(mask[0]).to(dev)).cpu(), torch.from_numpy(want))
    with pytest.raises(ValueError, match="mask"):
        ops.image_mask_out(torch.from_numpy(image).to(dev), torch.zeros(n + 1, H, W, dtype=torch.uint8, device=dev))


# ---- the engine on the cases of tests/_fillcond.py ----------------------------------------------------------------------------------------
def build(dev, width, cfg=None, named=None):
    from diffusionkit_amd.engine import MMDiTEngine
    cfg = cfg or tiny_flux(condition_features=width)
    named = named or fc.weights(width)
    return MMDiTEngine(cfg, pack_mmdit(cfg, named, dev)), named


def peek(eng, which, shape):
    """a copy of one of the engine's internal buffers (dk_mmdit_debug_buffer) on the host"""
    torch.cuda.synchronize()
    ptr = eng.lib.dk_mmdit_debug_buffer(eng._h, which)
    assert ptr, f"debug buffer {which} is NULL"
    t = torch.empty(shape, dtype=eng.dtype, device=eng._ws.device)
    hip = ctypes.CDLL("libamdhip64.so")  # (kind 3: device to device)
    assert hip.hipMemcpy(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(t.numel() * t.element_size()), 3) == 0
    return t.cpu()


def condition_of(cfg, name, width, dev):
    """the condition tokens of a case on the device, one per batch row, made by the kernel under test (test 1 holds it to the statement)"""
    _, _, _, z, mask = fc.case_inputs(cfg, name, width)
    return ops.fill_condition_tokens(z.to(dev), None if mask is None else mask.to(dev))


def start(eng, name, width, dev, per_image=True, block_cache=False, zero=False, cond=True):
    """prepare + cache for a case -> (tokens, text) on the device; ``zero``: an all-zero condition; ``cond`` False: no cache_condition at all"""
    B, (Hl, Wl), S_t = fc.CASES[name]
    text, pooled, lat, _, _ = fc.case_inputs(eng.config, name, width)
    eng.enable_block_cache(block_cache)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(pooled.to(dev), TS)
    if cond and eng.condition_features:
        c = condition_of(eng.config, name, width, dev)
        c = torch.zeros_like(c) if zero else c
        eng.cache_condition(c if per_image else c[:1].contiguous(), per_image=per_image)
    return eng.patchify(lat.to(dev)), text.to(dev, eng.dtype)


@functools.lru_cache(maxsize=None)
def engine_case(dev, name, width):
    """one engine per run, shared by the tests below (read-only): tokens_out with the condition, and with an all-zero condition"""
    eng, _ = build(dev, width)
    tok, text = start(eng, name, width, dev)
    out = eng.forward_tokens(tok, text, STEP).cpu()
    tok, text = start(eng, name, width, dev, zero=True)
    out0 = eng.forward_tokens(tok, text, STEP).cpu()
    return {"out": out, "out0": out0}


# ---- 3. output parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,width", fc.RUNS, ids=RUN_IDS)
def test_output_parity(dev, name, width):
    got, res = engine_case(dev, name, width), fc.oracle_case(name, width)
    f, e = res["fp32"][STEP], res["emu"][STEP]
    assert got["out"].shape == f["final"].shape and bool(torch.isfinite(got["out"].float()).all())
    yardstick_ok(got["out"].float(), e["final"], f["final"], f"{name}/{width}: tokens_out")
    psnr_ok(got["out"].float(), e["final"], f["final"], f"{name}/{width}: tokens_out")


# ---- 4. the condition matters, and matters correctly -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,width", fc.RUNS, ids=RUN_IDS)
def test_condition_effect(dev, name, width):
    """delta = out(condition) - out(all-zero condition) against the fp32 oracle's delta; the bound is twice the bf16-emulating oracle's own
    figure + 0.02 (0.035 - 0.039 here: the oracle's figure is 0.008 - 0.010, and delta is 0.78 - 0.94 of the output norm).  Measured on the CPU
    oracle with the plain synthetic weights, F_c = 320: an engine that reads the mask columns in (ph pw c) order scores 0.39 - 0.41, one that
    takes the mask half in front of the latent half 1.05 - 1.07, one that ignores the condition 1.0 -- ten times the bound and more, so the
    sharpened weights of tests/_refcond.py are not needed (tests/test_fill_cond_cpu.py::test_effect_inputs_discriminate keeps that true)."""
    got, res = engine_case(dev, name, width), fc.oracle_case(name, width)
    f, e = res["fp32"][STEP], res["emu"][STEP]
    d32, de = f["final"] - f["final0"], e["final"] - e["final0"]
    dh = got["out"].float() - got["out0"].float()
    share, e_e, e_h = float(d32.norm() / f["final"].norm()), rel_l2(d32, de), rel_l2(d32, dh)
    print(f"[condition] {name}/{width}: delta is {share:.3f} of the output norm; rel_l2(delta) hip-vs-fp32 {e_h:.4f}, emu-vs-fp32 {e_e:.4f}")
    assert share >= 0.05, "the inputs stopped discriminating"
    assert e_e <= 0.2, "the bf16-emulating oracle no longer reproduces the condition's effect: the bound below would say nothing"
    assert e_h <= 2.0 * e_e + 0.02, f"{name}/{width}: the condition's effect on the output: {e_h:.4f} > 2 * {e_e:.4f} + 0.02"


def test_condition_share_buffer(dev):
    """CONDE (debug buffer 6) = cond . W[:, F:]^T without the bias, one bf16 rounding"""
    name, width = "A2", 320
    eng, named = build(dev, width)
    start(eng, name, width, dev)
    B, (Hl, Wl), _ = fc.CASES[name]
    S_i, h = (Hl // 2) * (Wl // 2), eng.config.hidden_size
    got = peek(eng, 6, (B, S_i, h)).float()
    w = named["x_embedder.proj.weight"].float().reshape(h, -1)
    want = condition_of(eng.config, name, width, dev).cpu().float() @ w[:, 64:].t()
    e = rel_l2(want, got)
    print(f"[condition] CONDE: rel_l2 {e:.3e}")
    assert e <= TOL_SINGLE_OP


# ---- 5. zeroed condition columns ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A2", "B"])
def test_zeroed_condition_columns_equal_a_plain_engine(dev, name):
    """W[:, F:] = 0: the row stride and the slice of the [h, F + F_c] weight, and the epilogue's order (bias, rounding, then the residual)"""
    width = 320
    named = {k: v.clone() for k, v in fc.weights(width).items()}
    named["x_embedder.proj.weight"][..., 64:] = 0
    eng, _ = build(dev, width, named=named)
    tok, text = start(eng, name, width, dev)
    out = eng.forward_tokens(tok, text, STEP).cpu()
    narrow = dict(named)
    narrow["x_embedder.proj.weight"] = named["x_embedder.proj.weight"][..., :64].contiguous()
    plain, _ = build(dev, 0, cfg=tiny_flux(), named=narrow)
    tok0, text0 = start(plain, name, width, dev)
    assert same_bits(tok0, tok)
    assert torch.equal(out, plain.forward_tokens(tok0, text0, STEP).cpu()), "zeroed condition columns != an engine bound to W[:, :F]"


# ---- 6. state and composition ------------------------------------------------------------------------------------------------------------
def test_broadcast_equals_per_image(dev):
    name, width = "A2", 320
    eng, _ = build(dev, width)
    B = fc.CASES[name][0]
    c = condition_of(eng.config, name, width, dev)
    tok, text = start(eng, name, width, dev, per_image=False)  # (one condition, c[:1], for both batch rows)
    one = eng.forward_tokens(tok, text, STEP).cpu()
    eng.cache_condition(c[:1].repeat(B, 1, 1).contiguous(), per_image=True)
    rep = eng.forward_tokens(tok, text, STEP).cpu()
    assert same_bits(one, rep), "per_image = 0 != per_image = 1 with the condition repeated"
    eng.cache_condition(c, per_image=True)
    both = eng.forward_tokens(tok, text, STEP).cpu()
    assert not same_bits(both, one), "another condition for batch row 1 changed nothing"
    assert same_bits(both, engine_case(dev, name, width)["out"])


def test_hoisted_condition_serves_every_step(dev):
    name, width, steps = "A1", 320, (0, 2)
    eng, _ = build(dev, width)
    tok, text = start(eng, name, width, dev)
    res = fc.oracle_case(name, width, steps=steps)
    for s in steps:  # (one cache_condition in front of both)
        out = eng.forward_tokens(tok, text, s).float().cpu()
        yardstick_ok(out, res["emu"][s]["final"], res["fp32"][s]["final"], f"{name}: step {s}")
        psnr_ok(out, res["emu"][s]["final"], res["fp32"][s]["final"], f"{name}: step {s}")


def test_forward_without_cached_condition_is_refused(dev):
    name, width = "A1", 320
    eng, _ = build(dev, width)
    B, (Hl, Wl), S_t = fc.CASES[name]
    tok, text = start(eng, name, width, dev, cond=False)
    with pytest.raises(_lib.DkHipError, match="dk_mmdit_cache_condition"):
        eng.forward_tokens(tok, text, STEP)
    with pytest.raises(_lib.DkHipError, match="dk_mmdit_cache_condition"):
        eng.run_blocks(torch.zeros(B, S_t + tok.shape[1], eng.config.hidden_size, dtype=BF, device=dev), STEP, 0)
    c = condition_of(eng.config, name, width, dev)
    eng.cache_condition(c, per_image=True)
    eng.forward_tokens(tok, text, STEP)
    eng.prepare(B, (Hl, Wl), S_t, len(TS) + 1)  # (prepare invalidates it)
    eng.cache_modulation_params(fc.case_inputs(eng.config, name, width)[1].to(dev), TS)
    with pytest.raises(_lib.DkHipError, match="dk_mmdit_cache_condition"):
        eng.forward_tokens(tok, text, STEP)
    with pytest.raises(_lib.DkHipError, match="condition tokens shape"):  # (the control width on a Fill engine; two conditions, one batch row)
        eng.cache_condition(c[..., :64].contiguous(), per_image=True)
    with pytest.raises(_lib.DkHipError, match="condition tokens shape"):
        eng.cache_condition(torch.cat([c, c], 0), per_image=True)
    with pytest.raises(_lib.DkHipError, match="condition_features"):  # (an engine without a width has no cache_condition)
        plain_engine(dev).cache_condition(c, per_image=True)


def test_too_narrow_weight_is_refused_before_binding(dev):
    """dk_mmdit_bind sees bare pointers: a 64-column weight under a width of 320 would be read out of bounds"""
    from diffusionkit_amd.engine import MMDiTEngine
    packed = pack_mmdit(tiny_flux(), synth_mmdit_weights(tiny_flux(), seed=1234), dev)
    for width in (64, 320):
        with pytest.raises(_lib.DkHipError, match=f"needs {64 + width} columns"):
            MMDiTEngine(tiny_flux(condition_features=width), packed)
    wide = pack_mmdit(tiny_flux(condition_features=320), fc.weights(320), dev)
    with pytest.raises(_lib.DkHipError, match="needs 64 columns"):
        MMDiTEngine(tiny_flux(), wide)
    with pytest.raises(_lib.DkHipError, match="needs 128 columns"):
        MMDiTEngine(tiny_flux(condition_features=64), wide)


@pytest.mark.parametrize("name", ["A2", "B"])
def test_width_off_again_equals_never_on(dev, name):
    """a plain engine whose handle had a width set (and a workspace carved for it) and cleared again: the bits and the bytes of one that never
    had.  (Nothing is launched while the width is on: the bound weight has no condition columns.)"""
    from diffusionkit_amd.engine import MMDiTEngine
    cfg = tiny_flux()
    make = lambda: MMDiTEngine(cfg, pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234), dev))
    eng, fresh = make(), make()
    B, (Hl, Wl), S_t = fc.CASES[name]
    shape = (B, Hl, Wl, S_t, len(TS))
    base = fresh.lib.dk_mmdit_workspace_bytes(fresh._h, *shape)
    _lib.check(eng.lib.dk_mmdit_set_condition_width(eng._h, 320), "dk_mmdit_set_condition_width")
    assert eng.lib.dk_mmdit_workspace_bytes(eng._h, *shape) > base
    eng.prepare(*shape[:1], (Hl, Wl), S_t, len(TS))
    assert eng.lib.dk_mmdit_debug_buffer(eng._h, 6)
    _lib.check(eng.lib.dk_mmdit_set_condition_width(eng._h, 0), "dk_mmdit_set_condition_width")
    eng._shape = None  # (the handle was un-prepared behind the wrapper's back)
    assert eng.lib.dk_mmdit_workspace_bytes(eng._h, *shape) == base
    outs = {}
    for label, e in (("off again", eng), ("never on", fresh)):
        tok, text = start(e, name, 0, dev)
        assert not e.lib.dk_mmdit_debug_buffer(e._h, 6)
        outs[label] = e.forward_tokens(tok, text, STEP).cpu()
    es.assert_identical(outs, f"{name}: condition width off again")


FP8 = fp8_config(tiny_flux(condition_features=320), "speed")


@pytest.mark.parametrize("name,cfg", [("A2", None), ("B", None), ("B", FP8)], ids=["A2", "B", "B-fp8"])
def test_exact_size_poisoned_workspace(dev, name, cfg):
    """an exact-size workspace that is all NaN before prepare, and NaN slack behind tokens_out: finite outputs, the bits of a clean run"""
    width = 320
    B, (Hl, Wl), S_t = fc.CASES[name]
    outs = {}
    for label, fill in (("zeros", es.FILL_ZERO), ("nan", es.FILL_NAN)):
        eng, _ = build(dev, width, cfg)
        nbytes = eng.lib.dk_mmdit_workspace_bytes(eng._h, B, Hl, Wl, S_t, len(TS))
        ws = es.GuardedWorkspace(nbytes, dev)
        ws.fill(fill)
        es.lend(eng, ws, nbytes)
        tok, text = start(eng, name, width, dev)
        assert eng._ws.data_ptr() == ws.interior(nbytes).data_ptr(), "the engine did not keep the lent workspace"
        n = tok.numel()
        slab = torch.full((n + 4096,), float("nan"), dtype=eng.dtype, device=dev)
        out = eng.forward_tokens(tok, text, STEP, tokens_out=slab[:n].view(tok.shape))
        torch.cuda.synchronize()
        ws.check(nbytes, f"{name} ({label})", fill)
        assert bool(torch.isnan(slab[n:].float()).all()), "the slack behind tokens_out was written"
        outs[label] = out.clone().cpu()
    if cfg is None:
        outs["plain"] = engine_case(dev, name, width)["out"]
    es.assert_identical(outs, f"{name}: poisoned exact-size workspace")


def test_block_cache_reuse_tail_with_condition(dev):
    """the header's definition on an engine with a condition width: X1 + R on the image rows, the text rows as block 0 left them, then the
    final layer; head + compute tail = forward; and a new condition resets the cache"""
    name, width = "A2", 320
    eng, named = build(dev, width)
    B, (Hl, Wl), S_t = fc.CASES[name]
    S_i, h = (Hl // 2) * (Wl // 2), eng.config.hidden_size
    S = S_t + S_i
    tok, text = start(eng, name, width, dev, block_cache=True)
    pooled = fc.case_inputs(eng.config, name, width)[1]
    a, b = 0, 1
    probe = eng.forward_head(tok, text, a).cpu()
    assert probe.shape == (B, 2) and bool((probe[:, 1] == 0).all())
    eng.forward_tail(a, False)
    R = peek(eng, 3, (B, S_i, h))
    assert int(bits(R).ne(0).sum()) > 0 and bool(torch.isfinite(R.float()).all())
    eng.forward_head(tok, text, b)
    X1 = peek(eng, 0, (B, S, h))
    out = eng.forward_tail(b, True).cpu()
    X = peek(eng, 0, (B, S, h))
    assert same_bits(X[:, S_t:], (X1[:, S_t:].float() + R.float()).to(BF)), "image rows != round(X1 + R)"
    assert same_bits(X[:, :S_t], X1[:, :S_t]), "the reuse tail touched the text rows"
    wf = {k: v.float() for k, v in named.items()}
    res = {}
    for pname, P in (("fp32", Prec()), ("emu", Prec(BF))):
        m = fc.FillCondMMDiT(eng.config, wf, P)
        m.cache_modulation_params(pooled, torch.tensor(TS))
        mod = m._mod["final_layer"][TS[b]].chunk(2, dim=-1)
        res[pname] = m._lin(affine_transform(X[:, S_t:].float(), mod[0], mod[1], eng.config.layer_norm_eps, P), "final_layer.linear")
    yardstick_ok(out.float(), res["emu"], res["fp32"], "FinalLayer behind the reuse tail")
    # head + compute tail = forward
    eng.reset_block_cache()
    eng.forward_head(tok, text, STEP)
    assert same_bits(eng.forward_tail(STEP, False).cpu(), engine_case(dev, name, width)["out"]), "head + compute tail != dk_mmdit_forward"
    # R and D_ref belong to the condition they were computed under
    eng.cache_condition(condition_of(eng.config, name, width, dev), per_image=True)
    eng.forward_head(tok, text, STEP)
    with pytest.raises(_lib.DkHipError, match="valid cache"):
        eng.forward_tail(STEP, True)


def test_fp8_with_condition(dev):
    """case B on the all-fp8 engine, bounded the way tests/test_gpu_reference_cond.py::test_fp8_with_reference bounds it (the three bounds of
    tests/test_gpu_fp8.py's tiny model-forward test): against the fake-quantising oracle 2 * emu + 2e-3 and > 35 dB, and against the
    un-quantised model -- the bf16 ENGINE's output for the case -- what the bf16-emulating fake-quant oracle reaches less 3 dB"""
    name, width = "B", 320
    eng, named = build(dev, width, FP8)
    tok, text = start(eng, name, width, dev)
    out = eng.forward_tokens(tok, text, STEP).float().cpu()
    assert bool(torch.isfinite(out).all())
    t, pooled, lat, z, mask = fc.case_inputs(FP8, name, width)
    cond = fc.condition_tokens_reference(z, mask).float()
    fq, paq = o8.fake_quant_block_weights(FP8, named), o8.policy_act_quant(FP8)
    res = {}
    for pname, P in (("fq_emu", Prec(BF)), ("fq_fp32", Prec())):
        m = fc.FillCondMMDiT(FP8, fq, P, act_quant=paq)
        m.cache_modulation_params(pooled, torch.tensor(TS))
        taps = {}
        m(lat, t, TS[STEP], taps=taps, cond=cond)
        res[pname] = taps["final"]
    bf16 = engine_case(dev, name, width)["out"].float()
    e_h, e_e = rel_l2(res["fq_fp32"], out), rel_l2(res["fq_fp32"], res["fq_emu"])
    p_fq, p_h, p_e = psnr(res["fq_fp32"], out), psnr(bf16, out), psnr(bf16, res["fq_emu"])
    print(f"[condition] fp8 {name}: rel_l2 vs fake-quant fp32 oracle {e_h:.3e} (bf16-emulating: {e_e:.3e}), PSNR {p_fq:.1f} dB; against the "
          f"bf16 engine {p_h:.1f} dB (bf16-emulating fake-quant oracle: {p_e:.1f} dB)")
    assert e_h <= 2.0 * e_e + 2e-3, (e_h, e_e)
    assert p_fq > 35.0
    assert p_h > p_e - 3.0


# ---- 7. the pipeline -----------------------------------------------------------------------------------------------------------------------
class WithCondition:
    """a ``FillCondMMDiT`` with its condition bound, as a model ``oracle.pipeline`` can call"""

    def __init__(self, model, cond):
        self.model, self.cond = model, cond

    def cache_modulation_params(self, pooled, timesteps):
        self.model.cache_modulation_params(pooled, timesteps)

    def __call__(self, latent, text, timestep):
        return self.model(latent, text, timestep, cond=self.cond)


def tiny_pipe(dev, condition=None):
    from diffusionkit_amd.pipeline import FluxPipeline
    return FluxPipeline(w16=True, a16=True, mmdit_config=tiny_flux(), vae_config=tiny_vae(), vae_encoder_config=tiny_vae_encoder(), device=dev,
                        text_len=16, **({} if condition is None else {"condition": condition}))


def picture(H=64, W=96, seed=4):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(yy * 255 // H), (xx * 255 // W), ((yy + xx) * 255 // (H + W))], -1)
    return np.clip(base + rng.randint(-20, 20, size=(H, W, 3)), 0, 255).astype(np.uint8)


def test_pipeline_fill(dev, tmp_path):
    from PIL import Image
    ecfg = tiny_vae_encoder()
    pipe = tiny_pipe(dev, "fill")
    cfg = pipe.mmdit_config
    assert cfg == tiny_flux(condition_features=320) and pipe.mmdit.condition_features == 320
    Hl, Wl, steps = 8, 12, 3
    rgb, mask = picture(8 * Hl, 8 * Wl), fc.make_mask(1, 8 * Hl, 8 * Wl, seed=11)[0].numpy()
    path, mpath = str(tmp_path / "image.png"), str(tmp_path / "mask.png")
    Image.fromarray(rgb).save(path)
    Image.fromarray(mask).save(mpath)
    seeds = [0, 1]
    text = randn(1, 16, cfg.token_level_text_embed_dim, seed=7)
    pooled = randn(1, cfg.pooled_text_embed_dim, seed=8)
    run = lambda **kw: pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=steps, cfg_weight=0.0, latent_size=(Hl, Wl), seed=seeds,
                                            condition_image_path=path, condition_mask_path=mpath, **kw)
    lat, iter_time = run()
    assert lat.shape == (2, Hl, Wl, 16) and len(iter_time) == steps
    assert pipe.last_condition == {"kind": "fill", "features": 320}
    # the oracle's closed loop: prepare_fill with the posterior's mean, then the Euler loop on the model with condition columns
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    ewf = {k: v.float() for k, v in synth_vae_encoder_weights(ecfg, seed=1234 + 2).items()}
    m = mask.astype(np.float32) / np.float32(255)
    image = torch.from_numpy(((rgb.astype(np.float32) / 255) * 2 - 1.0) * (np.float32(1) - m)[..., None])[None]
    res = {}
    for pname, P in (("fp32", Prec()), ("emu", Prec(BF))):
        hidden = OracleVAEEncoder(ecfg, ewf, P)(image)
        mean = sample_latent(hidden, torch.zeros(1, Hl, Wl, hidden.shape[-1] // 2))
        cond = fc.condition_tokens_reference(op.process_in(mean, "flux"), torch.from_numpy(mask)[None]).float()
        model = WithCondition(fc.FillCondMMDiT(cfg, wf, P), cond)
        res[pname] = torch.cat([op.denoise_latents(model, text, pooled, steps, 0.0, (Hl, Wl), s, 1.0, True, Prec(BF)) for s in seeds], 0)
    p_h, p_e = psnr(res["fp32"], lat), psnr(res["fp32"], res["emu"])
    print(f"[condition] pipeline: final latent PSNR {p_h:.1f} dB against the closed-loop fp32 oracle (bf16-emulating oracle: {p_e:.1f} dB)")
    assert p_h > 35.0
    # a list with one image / mask per seed, the same twice: the same latents
    lat2, _ = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=steps, cfg_weight=0.0, latent_size=(Hl, Wl), seed=seeds,
                                   condition_image_path=[path, rgb], condition_mask_path=[mask, mpath])
    assert same_bits(lat2.cpu(), lat.cpu())
    # the first-block cache at threshold 0 computes every step: the same latents; another sampler completes
    lat3, _ = run(block_cache=0.0)
    assert same_bits(lat3.cpu(), lat.cpu()), "block_cache = 0 with a condition != no block cache"
    lat4, _ = run(sampler="ab2")
    assert lat4.shape == lat.shape and bool(torch.isfinite(lat4).all())
    # img2img with masked denoising on top, at another size: it completes with finite output
    init = picture(64, 128, seed=5)
    half = np.zeros((64, 128), dtype=np.uint8)
    half[:, 64:] = 255
    lat5, _ = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=2, cfg_weight=0.0, latent_size=(8, 16), seed=seeds,
                                   image_path=init, mask_path=half, condition_image_path=init, condition_mask_path=half)
    assert lat5.shape == (2, 8, 16, 16) and bool(torch.isfinite(lat5).all())
    # generate_image: the log, and composite keeps the kept pixels' bytes (two seeds: the images are stacked vertically)
    img, log = pipe.generate_image("a cat", num_steps=2, latent_size=(Hl, Wl), seed=seeds, verbose=False, condition_image_path=path,
                                   condition_mask_path=mpath)
    assert log["denoising"]["condition"] == {"kind": "fill", "features": 320} and img.size == (8 * Wl, 2 * 8 * Hl)
    px = np.array(img).reshape(2, 8 * Hl, 8 * Wl, 3)
    keep = mask == 0
    assert keep.sum() > 100 and all(np.array_equal(px[i][keep], rgb[keep]) for i in range(2)), "composite did not keep the kept pixels' bytes"
    raw, _ = pipe.generate_image("a cat", num_steps=2, latent_size=(Hl, Wl), seed=seeds, verbose=False, condition_image_path=path,
                                 condition_mask_path=mpath, composite=False)
    raw = np.array(raw).reshape(2, 8 * Hl, 8 * Wl, 3)
    assert not np.array_equal(raw[0][keep], rgb[keep]), "without composite the decoder's bytes stand"
    full = mask == 255
    assert np.array_equal(raw[0][full], px[0][full]), "composite touched the repainted pixels"
    # a call without the keywords is refused, and so is the same call on a plain pipeline
    with pytest.raises(ValueError, match="needs condition_image_path in every call"):
        pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=2, latent_size=(Hl, Wl), seed=seeds)
    with pytest.raises(ValueError, match="condition='fill' or condition='control'"):
        tiny_pipe(dev).generate_image("a cat", num_steps=2, latent_size=(Hl, Wl), seed=seeds, verbose=False, condition_image_path=path,
                                      condition_mask_path=mpath)


def test_pipeline_control(dev):
    pipe = tiny_pipe(dev, "control")
    assert pipe.mmdit_config == tiny_flux(condition_features=64)
    Hl, Wl = 8, 12
    edges = picture(8 * Hl, 8 * Wl, seed=6)
    img, log = pipe.generate_image("a cat", num_steps=2, latent_size=(Hl, Wl), seed=3, verbose=False, condition_image_path=edges)
    assert log["denoising"]["condition"] == {"kind": "control", "features": 64} and img.size == (8 * Wl, 8 * Hl)
    other, _ = pipe.generate_image("a cat", num_steps=2, latent_size=(Hl, Wl), seed=3, verbose=False, condition_image_path=255 - edges)
    assert img.tobytes() != other.tobytes(), "another control image changed nothing"
    again, _ = pipe.generate_image("a cat", num_steps=2, latent_size=(Hl, Wl), seed=3, verbose=False, condition_image_path=edges)
    assert img.tobytes() == again.tobytes()
