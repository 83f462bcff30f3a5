"""SD3 ControlNet on the MI355X: the LayerNorm pass with a residual tap in front bit for bit against the plain pass and the fp64 add, its
footprint, the ControlNet engine against ``tests/_controlnet.ControlNetOracle``, the main engine with taps against ``ControlledOracle``, the
chain of the two at the production width and in float16, and both engines on guarded, poisoned workspaces.

The gates are the project's own (tests/test_gpu_model.py: err(hip, fp32) <= 2 err(emu, fp32) + 2e-3 and PSNR > 35 dB; tests/test_gpu_f16_model.py's
``gate`` in float16); nothing here sets a tolerance of its own.  Arithmetic parity on synthetic weights: no ControlNet checkpoint has been run."""
from dataclasses import replace

import pytest
import torch

from diffusionkit_amd.config import SD3_2b, float16_config, tiny_flux, tiny_sd3, tiny_sd3_controlnet, tiny_sd35m
from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
from oracle.mmdit import Prec, embed_dtype
from tests._controlnet import ControlledOracle, ControlNetOracle, tap_index
from tests._engine_state import FILL_NAN, GuardedWorkspace, lend
from tests._footprint import NAN, SENTINEL, assert_footprint, bits, guarded
from tests._util import BF, psnr, randn, rel_l2
from tests.test_gpu_f16_model import gate as gate_f16
from tests.test_gpu_model import psnr_ok, yardstick_ok

pytestmark = pytest.mark.gpu

F16 = torch.float16
TS = [1000.0, 752.0, 500.0]
S_T = 3  # text rows per batch row of the kernel tests' joint buffer


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
def kernel_case(dev, h, M, dtype):
    """a joint [B, S_t + S_i, h] buffer (text rows first), a dense tap and one modulation table of four rows"""
    B = 2 if M % 2 == 0 else 1
    S_i = M // B
    g = torch.Generator().manual_seed(h + M)
    joint = (torch.randn(B, S_T + S_i, h, generator=g) * 2 + 0.5).to(dev, dtype)
    tap = torch.randn(B, S_i, h, generator=g).to(dev, dtype)
    tab = (torch.randn(B, 4 * h, generator=g) * 0.5).to(dev, dtype)
    return joint, tap, [tab[:, i * h:(i + 1) * h] for i in range(4)]


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("with_text", [True, False], ids=["text", "alone"])
@pytest.mark.parametrize("M", [5, 70])
@pytest.mark.parametrize("h", [256, 320, 640, 1536])
def test_ln_modulate_add_bit_for_bit(dev, h, M, with_text, dtype):
    """h 256 / 320: lanes past the row end in the only pass; 640: a half-live second pass; 1536: three full passes (the production width).
    M 5 / 70: a last workgroup with one / two of its four rows; 70: two batch rows of 35 with their own modulation and their own segment of
    the joint buffer."""
    from diffusionkit_amd import ops
    joint0, tap, (sh, sc, s1, c1) = kernel_case(dev, h, M, dtype)
    plain = ops.ln_modulate(joint0[:, S_T:].contiguous(), sh, sc)
    text_ref = ops.ln_modulate(joint0[:, :S_T].contiguous(), s1, c1)
    for s in (1.0, 0.7, 0.0):
        joint = joint0.clone()
        x, x1 = joint[:, S_T:], joint[:, :S_T]
        want = (joint0[:, S_T:].double() + torch.tensor(s, dtype=torch.float32).double() * tap.double()).float().to(dtype)
        got = ops.ln_modulate_add(x, tap, s, sh, sc, text=(x1, s1, c1) if with_text else None)
        assert len(got) == (3 if with_text else 2) and got[0] is x
        assert same_bits(x, want), f"s = {s}: the rows written back"
        assert same_bits(got[1], ops.ln_modulate(x.contiguous(), sh, sc)), f"s = {s}: the modulated rows"
        assert same_bits(x1, joint0[:, :S_T]), f"s = {s}: the text rows of the joint buffer"
        if with_text:
            assert same_bits(got[2], text_ref)
        assert (s == 0.0) == same_bits(got[1], plain)
    joint = joint0.clone()
    got = ops.ln_modulate_add(joint[:, S_T:], torch.zeros_like(tap), 0.7, sh, sc, text=(joint[:, :S_T], s1, c1) if with_text else None)
    assert same_bits(got[1], plain) and same_bits(joint, joint0)


def launch_add(x, x_seg_stride, tap, s, out, sh, sc, S_i, text=None):
    """dk_ln_modulate_add_* on caller-owned buffers (ops.ln_modulate_add allocates its outputs: no margins to check)"""
    from diffusionkit_amd import _lib
    from diffusionkit_amd.ops import _stream
    M, h = tap.shape[0] * tap.shape[1], tap.shape[2]
    fn = getattr(_lib.load(), "dk_ln_modulate_add_" + ("f16" if x.dtype == F16 else "bf16"))
    t = (None, None, 0, None, None, 0) if text is None else text
    _lib.check(fn(x.data_ptr(), tap.data_ptr(), h, float(s), out.data_ptr(), M, sh.data_ptr(), sc.data_ptr(), S_i, *t, h, h, h, sh.stride(0),
                  x_seg_stride, x_seg_stride, 1e-6, _stream()), "dk_ln_modulate_add")


@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "f16"])
def test_ln_modulate_add_footprint(dev, dtype):
    """h 320, two batch rows of 35 image rows: a NaN in one tap element reaches exactly that element of x' and that row of out; a NaN in a text
    row reaches that text output row and no image output; the margins around the joint buffer, the tap and both outputs stay what they were"""
    h, M = 320, 70
    joint0, tap0, (sh, sc, s1, c1) = kernel_case(dev, h, M, dtype)
    B, S = joint0.shape[0], joint0.shape[1]
    S_i = S - S_T
    runs = {}
    for name in ("clean", "tap", "text"):
        joint, gj = guarded(joint0, 2)
        tap, gt = guarded(tap0, 2)
        out, go = guarded(torch.full((B, S_i, h), SENTINEL, dtype=dtype, device=dev), 2, fill=SENTINEL)
        out1, g1 = guarded(torch.full((B, S_T, h), SENTINEL, dtype=dtype, device=dev), 2, fill=SENTINEL)
        if name == "tap":
            tap[1, 17, 123] = NAN
        if name == "text":
            joint[1, 1, 200] = NAN
        launch_add(joint[:, S_T:], S, tap, 0.7, out, sh, sc, S_i, text=(joint.data_ptr(), out1.data_ptr(), B * S_T, s1.data_ptr(), c1.data_ptr(), S_T))
        torch.cuda.synchronize()
        for g, what in ((gj, "joint buffer"), (gt, "tap"), (go, "out"), (g1, "text out")):
            g.check(f"{name}: {what}")
        runs[name] = (joint.clone(), out.clone(), out1.clone())
    clean = runs["clean"]
    none = lambda t: torch.zeros(t.shape, dtype=torch.bool)
    # the tap's NaN: one element of x', one row of out, nothing of the text
    e_joint, e_out = none(clean[0]), none(clean[1])
    e_joint[1, S_T + 17, 123] = True
    e_out[1, 17, :] = True
    assert_footprint(clean[0], runs["tap"][0], e_joint, "tap NaN: joint buffer")
    assert_footprint(clean[1], runs["tap"][1], e_out, "tap NaN: out")
    assert_footprint(clean[2], runs["tap"][2], none(clean[2]), "tap NaN: text out")
    # the text row's NaN: its own output row; the joint buffer holds the poison itself and nothing else
    e_joint, e_out1 = none(clean[0]), none(clean[2])
    e_joint[1, 1, 200] = True
    e_out1[1, 1, :] = True
    assert_footprint(clean[0], runs["text"][0], e_joint, "text NaN: joint buffer")
    assert_footprint(clean[1], runs["text"][1], none(clean[1]), "text NaN: out")
    assert_footprint(clean[2], runs["text"][2], e_out1, "text NaN: text out")


# ---- the ControlNet engine ----------------------------------------------------------------------------------------------------------
def build(cfg, dev, seed=1234):
    from diffusionkit_amd.engine import MMDiTEngine
    named = synth_mmdit_weights(cfg, seed=seed)
    return MMDiTEngine(cfg, pack_mmdit(cfg, named, dev)), named


def inputs(cfg, B, Hl, Wl, S_t):
    return (randn(B, S_t, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, Hl, Wl, 16, seed=5),
            randn(B, Hl, Wl, 16, seed=6))


def prepared(cfg, dev, B, Hl, Wl, S_t, dtype=BF):
    eng, _ = build(cfg, dev)
    text, pooled, lat, ctrl = inputs(cfg, B, Hl, Wl, S_t)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(pooled.to(dev), TS)
    return eng, text.to(dev, dtype), eng.patchify(lat.to(dev)), ctrl.to(dev)


_oracle_cache = {}


def cn_oracle(cfg, B, Hl, Wl, S_t, step=1):
    """fp32 and bf16-emulating ControlNetOracle on the seeded case: (model, taps [N_c, B, S_i, h], streams), computed once per case"""
    key = ("cn", cfg, B, Hl, Wl, S_t, step)
    if key not in _oracle_cache:
        wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
        text, pooled, lat, ctrl = inputs(cfg, B, Hl, Wl, S_t)
        res = {}
        for name, P in (("fp32", Prec()), ("emu", Prec(BF))):
            m = ControlNetOracle(cfg, wf, P)
            m.cache_modulation_params(pooled, torch.tensor(TS))
            streams = {}
            res[name] = (m, m(lat, text, TS[step], ctrl, taps=streams), streams)
        _oracle_cache[key] = res
    return _oracle_cache[key]


CN_TINY = {"b2": (tiny_sd3_controlnet(depth=2, heads=4), 2, 8, 12, 20), "heads6_35tok": (tiny_sd3_controlnet(depth=2, heads=6), 1, 10, 14, 20)}


@pytest.mark.parametrize("name", list(CN_TINY))
def test_controlnet_taps_tiny(dev, name):
    """two blocks, the second with the text stream stopping after attention; heads 6: h = 384; 35 image tokens: an odd count on every tile"""
    cfg, B, Hl, Wl, S_t = CN_TINY[name]
    eng, text, tok, ctrl = prepared(cfg, dev, B, Hl, Wl, S_t)
    eng.cache_control_image(ctrl, per_image=True)
    taps = eng.control_forward(tok, text, 1)
    assert tuple(taps.shape) == eng.taps_shape() == (cfg.depth_multimodal, B, (Hl // 2) * (Wl // 2), cfg.hidden_size)
    res = cn_oracle(cfg, B, Hl, Wl, S_t)
    for j in range(cfg.depth_multimodal):
        e_h, e_e = yardstick_ok(taps[j].float(), res["emu"][1][j], res["fp32"][1][j], f"{name} tap {j}")
        print(f"[controlnet] {name} tap {j}: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e})")
    assert rel_l2(res["fp32"][1][0], res["fp32"][1][1]) > 0.5  # (the taps are different tensors)


def test_controlnet_shared_image_and_recache(dev):
    """one control image for both batch rows gives the bits of a per-image copy of it; a second cache_control_image replaces the first"""
    cfg, B, Hl, Wl, S_t = CN_TINY["b2"]
    eng, text, tok, ctrl = prepared(cfg, dev, B, Hl, Wl, S_t)
    eng.cache_control_image(ctrl, per_image=True)
    first = eng.control_forward(tok, text, 1).clone()
    eng.cache_control_image(ctrl[:1].repeat(B, 1, 1, 1).contiguous(), per_image=True)
    copied = eng.control_forward(tok, text, 1).clone()
    eng.cache_control_image(ctrl[:1].contiguous(), per_image=False)
    shared = eng.control_forward(tok, text, 1).clone()
    assert same_bits(shared, copied) and not same_bits(shared, first)
    eng.cache_control_image(ctrl, per_image=True)
    assert same_bits(eng.control_forward(tok, text, 1), first)


def test_controlnet_last_block_teacher_forced(dev):
    """run_blocks stays available on a control-net engine: its last block from the fp32 oracle's stream in front of it"""
    cfg, B, Hl, Wl, S_t = CN_TINY["b2"]
    res = cn_oracle(cfg, B, Hl, Wl, S_t)
    last = cfg.depth_multimodal - 1
    streams = res["fp32"][2]
    img, txt = (streams[f"double{last - 1}_{n}"].to(BF).float() for n in ("img", "txt"))
    eng, _, _, ctrl = prepared(cfg, dev, B, Hl, Wl, S_t)
    y = eng.run_blocks(torch.cat([txt, img], dim=1).to(dev, BF).contiguous(), 1, last).float().cpu()
    outs = {n: res[n][0]._double_block(last, img, txt, TS[1], None) for n in ("fp32", "emu")}
    yardstick_ok(y[:, S_t:], outs["emu"][0], outs["fp32"][0], "last block image rows")
    assert outs["fp32"][1] is None and torch.equal(y[:, :S_t], txt)  # the text stream stops after attention: rows untouched


def test_controlnet_engine_refusals(dev):
    from diffusionkit_amd._lib import DkHipError
    cfg, B, Hl, Wl, S_t = CN_TINY["b2"]
    eng, text, tok, ctrl = prepared(cfg, dev, B, Hl, Wl, S_t)
    with pytest.raises(DkHipError, match="cache_control_image"):
        eng.control_forward(tok, text, 1)
    eng.cache_control_image(ctrl, per_image=True)
    with pytest.raises(DkHipError, match="dk_mmdit_control_forward"):
        eng.forward_tokens(tok, text, 1)
    with pytest.raises(DkHipError, match="control-net engine"):
        eng.set_control_taps(torch.zeros(1, B, tok.shape[1], cfg.hidden_size, dtype=BF, device=dev))
    with pytest.raises(DkHipError, match="control-net engine"):
        eng.set_skip_layers([0], 1)
    with pytest.raises(DkHipError, match="control-net engine"):
        eng.enable_block_cache(True)
    main, _ = build(tiny_sd3(depth=2, heads=4), dev)
    main.prepare(B, (Hl, Wl), S_t, len(TS))
    with pytest.raises(DkHipError, match="control_net"):
        main.control_forward(tok, text, 1)
    with pytest.raises(DkHipError, match="control_net"):
        main.cache_control_image(ctrl)
    with pytest.raises((DkHipError, ValueError), match="SD3 family"):
        build(replace(tiny_flux(), control_net=True), dev)


# ---- the main engine with taps ------------------------------------------------------------------------------------------------------
MAIN = {"depth4_taps2": (4, 2), "depth3_taps2": (3, 2), "depth2_taps2": (2, 2)}
TAP_SCALE = 0.7


def synthetic_taps(n, B, S_i, h):
    return randn(n, B, S_i, h, seed=11, scale=0.1)


def main_oracle(cfg, n_taps, B, Hl, Wl, S_t, step=1):
    """the final layer's output of the fp32 and the bf16-emulating ControlledOracle under the synthetic taps, and of the fp32 one without"""
    key = ("main", cfg, n_taps, B, Hl, Wl, S_t, step)
    if key not in _oracle_cache:
        wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
        text, pooled, lat, _ = inputs(cfg, B, Hl, Wl, S_t)
        taps = synthetic_taps(n_taps, B, (Hl // 2) * (Wl // 2), cfg.hidden_size)
        res = {}
        for name, P, control in (("fp32", Prec(), (taps, TAP_SCALE)), ("emu", Prec(BF), (taps, TAP_SCALE)), ("plain", Prec(), None)):
            m = ControlledOracle(cfg, wf, P)
            m.control = control
            m.cache_modulation_params(pooled, torch.tensor(TS))
            streams = {}
            m(lat, text, TS[step], taps=streams)
            res[name] = streams["final"]
        _oracle_cache[key] = res
    return _oracle_cache[key]


@pytest.mark.parametrize("name", list(MAIN))
def test_main_engine_with_taps(dev, name):
    """depth 4 with 2 taps: taps 0, 0, 1 behind blocks 0, 1, 2; depth 3 with 2: the interval 1.5 is not whole, taps 0, 0; depth 2 with 2: tap 0
    behind block 0 and nothing else"""
    depth, n = MAIN[name]
    assert [tap_index(g, n, depth) for g in range(depth - 1)] == {"depth4_taps2": [0, 0, 1], "depth3_taps2": [0, 0], "depth2_taps2": [0]}[name]
    cfg, B, Hl, Wl, S_t = tiny_sd3(depth=depth, heads=4), 2, 8, 12, 20
    eng, text, tok, _ = prepared(cfg, dev, B, Hl, Wl, S_t)
    taps = synthetic_taps(n, B, tok.shape[1], cfg.hidden_size).to(dev, BF)
    plain = eng.forward_tokens(tok, text, 1).clone()
    eng.set_control_taps(taps, TAP_SCALE)
    out = eng.forward_tokens(tok, text, 1).clone()
    res = main_oracle(cfg, n, B, Hl, Wl, S_t)
    moved = rel_l2(res["plain"], res["fp32"])
    assert moved > 0.05, f"the taps move the fp32 oracle's output by {moved:.3e} only: the case shows nothing"
    e_h, e_e = yardstick_ok(out.float(), res["emu"], res["fp32"], name)
    p = psnr(res["fp32"], out.float())
    print(f"[controlnet] main {name}: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR {p:.1f} dB; the taps move the output by {moved:.3e}")
    assert p > 35.0 and rel_l2(plain.float(), out.float()) > 0.05
    # taps of zeros, and taps set and cleared: the plain forward's bits
    eng.set_control_taps(torch.zeros_like(taps), TAP_SCALE)
    assert same_bits(eng.forward_tokens(tok, text, 1), plain)
    eng.set_control_taps(taps, TAP_SCALE)
    eng.set_control_taps(None)
    assert same_bits(eng.forward_tokens(tok, text, 1), plain)


def test_main_engine_tap_refusals(dev):
    from diffusionkit_amd._lib import DkHipError
    B, Hl, Wl, S_t = 2, 8, 12, 20
    cfg = tiny_sd3(depth=3, heads=4)
    eng, text, tok, _ = prepared(cfg, dev, B, Hl, Wl, S_t)
    S_i, h = tok.shape[1], cfg.hidden_size
    taps = lambda n: torch.zeros(n, B, S_i, h, dtype=BF, device=dev)
    with pytest.raises(DkHipError, match="n_taps"):
        eng.set_control_taps(taps(4))
    with pytest.raises(DkHipError, match="taps shape"):
        eng.set_control_taps(torch.zeros(2, B, S_i + 1, h, dtype=BF, device=dev))
    eng.set_skip_layers([1], 1)
    with pytest.raises(DkHipError, match="skip layers"):
        eng.set_control_taps(taps(2))
    eng.set_skip_layers(None, 0)
    eng.set_perturbed_attention([1], 1)
    with pytest.raises(DkHipError, match="perturbed attention"):
        eng.set_control_taps(taps(2))
    eng.set_perturbed_attention(None, 0)
    eng.set_control_taps(taps(2))
    for call in (lambda: eng.set_skip_layers([1], 1), lambda: eng.set_perturbed_attention([1], 1), lambda: eng.enable_block_cache(True)):
        with pytest.raises(DkHipError, match="control taps"):
            call()
    x = torch.zeros(B, S_t + S_i, h, dtype=BF, device=dev)
    with pytest.raises(DkHipError, match="dk_mmdit_set_control_taps"):
        eng.run_blocks(x, 1, 0)
    eng.set_control_taps(None)
    eng.run_blocks(x, 1, 0)
    # the block cache: its entries refuse while taps are set, and taps refuse while it is on
    eng.enable_block_cache(True)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    with pytest.raises(DkHipError, match="block cache"):
        eng.set_control_taps(taps(2))
    # other families
    flux, _ = build(tiny_flux(), dev)
    flux.prepare(1, (8, 8), 16, 1)
    with pytest.raises(DkHipError, match="SD3 family"):
        flux.set_control_taps(torch.zeros(1, 1, 16, tiny_flux().hidden_size, dtype=BF, device=dev))
    c35 = tiny_sd35m()
    dual, _ = build(c35, dev)
    dual.prepare(B, (Hl, Wl), S_t, len(TS))
    with pytest.raises(DkHipError, match="dual attention"):
        dual.set_control_taps(torch.zeros(1, B, S_i, c35.hidden_size, dtype=BF, device=dev))


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
def chain_oracles(main_cfg, cn_cfg, B, Hl, Wl, S_t, precs, step=1):
    """{name: final} of ControlNetOracle -> taps -> ControlledOracle, each side in the precision named; weights rounded to ``wdt``"""
    text, pooled, lat, ctrl = inputs(main_cfg, B, Hl, Wl, S_t)
    out = {}
    for name, (P, wdt, kw) in precs.items():
        wm = {k: v.to(wdt).float() for k, v in synth_mmdit_weights(main_cfg, seed=1234).items()}
        wc = {k: v.to(wdt).float() for k, v in synth_mmdit_weights(cn_cfg, seed=4321).items()}
        cn, main = ControlNetOracle(cn_cfg, wc, P, **kw), ControlledOracle(main_cfg, wm, P, **kw)
        for m in (cn, main):
            m.cache_modulation_params(pooled, torch.tensor(TS))
        main.control = (cn(lat, text, TS[step], ctrl), TAP_SCALE)
        streams = {}
        main(lat, text, TS[step], taps=streams)
        out[name] = streams["final"]
    return out


def chain_engines(main_cfg, cn_cfg, dev, B, Hl, Wl, S_t, dtype=BF, step=1):
    from diffusionkit_amd.engine import MMDiTEngine
    text, pooled, lat, ctrl = inputs(main_cfg, B, Hl, Wl, S_t)
    main = MMDiTEngine(main_cfg, pack_mmdit(main_cfg, synth_mmdit_weights(main_cfg, seed=1234), dev))
    cn = MMDiTEngine(cn_cfg, pack_mmdit(cn_cfg, synth_mmdit_weights(cn_cfg, seed=4321), dev))
    for e in (main, cn):
        e.prepare(B, (Hl, Wl), S_t, len(TS))
        e.cache_modulation_params(pooled.to(dev), TS)
    cn.cache_control_image(ctrl.to(dev), per_image=True)
    tok, text = main.patchify(lat.to(dev)), text.to(dev, dtype)
    taps = cn.control_forward(tok, text, step)
    main.set_control_taps(taps, TAP_SCALE)
    return main.forward_tokens(tok, text, step)


def test_chain_production_width(dev):
    """SD3-medium's width (h 1536, 24 heads of 64): main depth 2, ControlNet depth 1, CFG batch 2, latent 16 x 16, S_t 20"""
    main_cfg = replace(SD3_2b, depth_multimodal=2, hidden_size_override=1536, max_latent_resolution=32)
    cn_cfg = replace(main_cfg, depth_multimodal=1, control_net=True)
    assert main_cfg.hidden_size == cn_cfg.hidden_size == 1536 and main_cfg.head_dim == 64
    out = chain_engines(main_cfg, cn_cfg, dev, 2, 16, 16, 20)
    res = chain_oracles(main_cfg, cn_cfg, 2, 16, 16, 20, {"fp32": (Prec(), torch.float32, {}), "emu": (Prec(BF), torch.float32, {})})
    e_h, e_e = yardstick_ok(out.float(), res["emu"], res["fp32"], "chain at width")
    p_h, p_e = psnr_ok(out.float(), res["emu"], res["fp32"], "chain at width")
    print(f"[controlnet] chain at width: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR {p_h:.1f} dB (emulation {p_e:.1f})")


def test_chain_tiny_f16(dev):
    """float16 engines under the float16 MMDiT tests' rule (tests/test_gpu_f16_model.py: fp16 weights on every side, the timestep embedding in
    the configuration's dtype on the fp32 side)"""
    main_cfg, cn_cfg = tiny_sd3(depth=3, heads=4), tiny_sd3_controlnet(depth=2, heads=4)
    B, Hl, Wl, S_t = 2, 8, 12, 20
    out = chain_engines(float16_config(main_cfg), float16_config(cn_cfg), dev, B, Hl, Wl, S_t, dtype=F16)
    assert out.dtype == F16
    res = chain_oracles(main_cfg, cn_cfg, B, Hl, Wl, S_t, {"fp32": (Prec(), F16, {"embed_prec": Prec(embed_dtype(main_cfg))}),
                                                           "emu16": (Prec(F16), F16, {}), "emubf": (Prec(BF), F16, {})})
    gate_f16(out.float(), res["emu16"], res["emubf"], res["fp32"], "controlnet chain tiny f16")


# ---- workspaces -----------------------------------------------------------------------------------------------------------------------
def test_chain_on_guarded_poisoned_workspaces(dev):
    """both engines on NaN-filled interiors of exactly the declared size, the taps tensor between NaN margins: the bits of the plain run and
    nothing written outside; then a smaller problem in the same (stale) allocations"""
    from diffusionkit_amd.engine import MMDiTEngine
    main_cfg, cn_cfg = tiny_sd3(depth=3, heads=4), tiny_sd3_controlnet(depth=2, heads=4)
    main = MMDiTEngine(main_cfg, pack_mmdit(main_cfg, synth_mmdit_weights(main_cfg, seed=1234), dev))
    cn = MMDiTEngine(cn_cfg, pack_mmdit(cn_cfg, synth_mmdit_weights(cn_cfg, seed=4321), dev))
    shapes = [(2, 8, 12, 20), (1, 6, 8, 12)]
    nbytes = {e: [int(e.lib.dk_mmdit_workspace_bytes(e._h, B, Hl, Wl, S_t, len(TS))) for B, Hl, Wl, S_t in shapes] for e in (main, cn)}
    ws = {e: GuardedWorkspace(max(nbytes[e]), dev) for e in (main, cn)}
    for k, (B, Hl, Wl, S_t) in enumerate(shapes):
        ref = chain_engines(main_cfg, cn_cfg, dev, B, Hl, Wl, S_t)
        text, pooled, lat, ctrl = inputs(main_cfg, B, Hl, Wl, S_t)
        for e in (main, cn):
            if k == 0:
                ws[e].fill(FILL_NAN)
            assert nbytes[e][k] <= nbytes[e][0]
            lend(e, ws[e], nbytes[e][k])
            e._shape = None
            e.prepare(B, (Hl, Wl), S_t, len(TS))
            assert e._ws.numel() == nbytes[e][k]
            e.cache_modulation_params(pooled.to(dev), TS)
        cn.cache_control_image(ctrl.to(dev), per_image=True)
        tok, text = main.patchify(lat.to(dev)), text.to(dev, BF)
        taps, gt = guarded(torch.full(cn.taps_shape(), NAN, dtype=BF, device=dev), 4)
        cn.control_forward(tok, text, 1, taps_out=taps)
        main.set_control_taps(taps, TAP_SCALE)
        out = main.forward_tokens(tok, text, 1)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(taps.float()).all())
        assert same_bits(out, ref), f"shape {k}: the guarded run differs from the plain one"
        gt.check(f"shape {k}: taps")
        for e, what in ((main, "main engine"), (cn, "control-net engine")):
            ws[e].check(nbytes[e][k], f"shape {k}: {what}", fill=FILL_NAN if k == 0 else None)


# ---- step loop and pipeline -----------------------------------------------------------------------------------------------------------
STEPS, HL_P, WL_P, CFGW, SHIFT, SCALE_P = 3, 8, 16, 5.0, 3.0, 0.8
PIPE_MAIN, PIPE_CN = tiny_sd3(depth=3, heads=4), tiny_sd3_controlnet(depth=2, heads=4)
SD3_VERSION = "argmaxinc/mlx-stable-diffusion-3-medium"
_PIPES = {}


def control_image(seed):
    import numpy as np
    return (np.random.RandomState(seed).rand(HL_P * 8, WL_P * 8, 3) * 255).astype(np.uint8)


def pipe_for(dev, controlnet=True, ckpt=None):
    """one tiny SD3 pipeline with the ControlNet (from reference-named tensors, or from ``ckpt``) and one without, for the whole module"""
    from diffusionkit_amd.config import tiny_vae, tiny_vae_encoder
    from diffusionkit_amd.pipeline import DiffusionPipeline
    key = (controlnet, ckpt)
    if key not in _PIPES:
        kw = dict(controlnet_ckpt=ckpt or synth_mmdit_weights(PIPE_CN, seed=4321), controlnet_config=PIPE_CN) if controlnet else {}
        _PIPES[key] = DiffusionPipeline(model_version=SD3_VERSION, w16=True, a16=True, shift=SHIFT, mmdit_config=PIPE_MAIN, vae_config=tiny_vae(),
                                        vae_encoder_config=tiny_vae_encoder(), device=dev, text_len=16, **kw)
    return _PIPES[key]


def pipe_inputs():
    return randn(2, 16, PIPE_MAIN.token_level_text_embed_dim, seed=7), randn(2, PIPE_MAIN.pooled_text_embed_dim, seed=8)


def sampled(pipe, dev, seed=0, **kw):
    text, pooled = pipe_inputs()
    n = len(seed) if isinstance(seed, list) else 1
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=STEPS, cfg_weight=CFGW, latent_size=(HL_P, WL_P), seed=seed, **kw)
    assert lat.shape == (n, HL_P, WL_P, 16) and lat.dtype == torch.float32 and len(iter_time) == STEPS
    return lat


def loop_references(pipe, image, seed=0, sampler="euler", interval=None, guidance_interval=None):
    """the oracle chain as ONE model in the restated step loop (tests/test_guidance_cpu.py's ``guided_loop``: every sampler, a guidance interval), on the
    fp32 and the bf16-emulating oracle, after process_out.  The control latent is the pipeline's own (its VAE encoder is not under test here)."""
    import numpy as np
    from diffusionkit_amd.sampler import step_plan
    from oracle import pipeline as op
    from tests._controlnet import ChainOracle, evaluations_active
    from tests.test_guidance_cpu import guided_loop
    from tests.test_samplers_cpu import start_state
    text, pooled = pipe_inputs()
    ctrl = pipe.latent_format.process_in(pipe.encode_reference_to_latents(np.ascontiguousarray(image[None]))).float().cpu()
    wm = {k: v.float() for k, v in synth_mmdit_weights(PIPE_MAIN, seed=1234).items()}
    wc = {k: v.float() for k, v in synth_mmdit_weights(PIPE_CN, seed=4321).items()}
    sigmas = op.get_sigmas(SHIFT, False, STEPS)
    active = evaluations_active(step_plan(sampler, sigmas.numpy()), interval)
    res = {}
    for name, P in (("fp32", Prec()), ("emu", Prec(BF))):
        chain = ChainOracle(ControlledOracle(PIPE_MAIN, wm, P), ControlNetOracle(PIPE_CN, wc, P), ctrl, SCALE_P, active)
        x0, _ = start_state(sigmas, seed, HL_P, WL_P)
        res[name] = op.process_out(guided_loop(chain, sampler, x0, sigmas, text, pooled, CFGW, Prec(BF), Prec(F16), interval=guidance_interval), "sd3")
        assert chain.calls == len(active)
    return res


def parity(lat, res, what):
    e_h, e_e = yardstick_ok(lat, res["emu"], res["fp32"], what)
    p_h, p_e = psnr(res["fp32"], lat), psnr(res["fp32"], res["emu"])
    print(f"[controlnet] {what}: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR hip {p_h:.1f} dB / emu {p_e:.1f} dB")
    if p_e >= 37.0:
        assert p_h > 35.0, f"{what}: PSNR {p_h:.1f} dB"


def test_pipeline_from_a_diffusers_layout_file(dev, tmp_path):
    """3 steps, CFG 5, tiny VAE, the ControlNet loaded from a file in the diffusers layout: the final latent against the oracle loop, the bits of the
    same weights handed over by name, and -- with scale 0 -- the bits of a pipeline without a ControlNet"""
    import os
    from safetensors.torch import save_file
    from tests._controlnet import to_diffusers_sd3_controlnet
    path = os.path.join(tmp_path, "controlnet.safetensors")
    save_file(to_diffusers_sd3_controlnet(synth_mmdit_weights(PIPE_CN, seed=4321), PIPE_CN), path)
    pipe, image = pipe_for(dev, ckpt=path), control_image(1)
    assert pipe.controlnet.control_net and pipe.controlnet.mod_rows() == PIPE_CN.num_modulation_rows()
    lat = sampled(pipe, dev, controlnet_image_path=image, controlnet_scale=SCALE_P)
    assert pipe.last_controlnet == {"scale": SCALE_P, "interval": None, "evals": STEPS} and pipe.mmdit.control_taps is None
    parity(lat, loop_references(pipe, image), "pipeline")
    named = pipe_for(dev)
    assert same_bits(lat, sampled(named, dev, controlnet_image_path=image, controlnet_scale=SCALE_P))
    plain = sampled(pipe_for(dev, controlnet=False), dev)
    assert not same_bits(lat, plain) and rel_l2(plain, lat) > 0.05
    assert same_bits(sampled(named, dev, controlnet_image_path=image, controlnet_scale=0.0), plain)
    from PIL import Image
    img, log = named.generate_image("a photo of a cat", num_steps=2, cfg_weight=CFGW, latent_size=(HL_P, WL_P), seed=3, verbose=False,
                                    controlnet_image_path=Image.fromarray(image), controlnet_interval=(0, 0.5))
    assert img.size == (WL_P * 8, HL_P * 8) and log["denoising"]["controlnet"] == {"scale": 1.0, "interval": (0.0, 0.5), "evals": 1}


def test_pipeline_interval(dev):
    """controlnet_interval = (0, 0.67) on 3 steps: the last step runs uncontrolled; an interval that holds no step: the plain pipeline's bits"""
    pipe, image = pipe_for(dev), control_image(1)
    lat = sampled(pipe, dev, controlnet_image_path=image, controlnet_scale=SCALE_P, controlnet_interval=(0, 0.67))
    assert pipe.last_controlnet["evals"] == 2 and pipe.mmdit.control_taps is None
    parity(lat, loop_references(pipe, image, interval=(0, 0.67)), "interval (0, 0.67)")
    assert not same_bits(lat, sampled(pipe, dev, controlnet_image_path=image, controlnet_scale=SCALE_P))
    none = sampled(pipe, dev, controlnet_image_path=image, controlnet_scale=SCALE_P, controlnet_interval=(0.5, 0.5))
    assert pipe.last_controlnet["evals"] == 0 and same_bits(none, sampled(pipe_for(dev, controlnet=False), dev))


def test_pipeline_heun(dev):
    """--sampler heun: two evaluations per step, both controlled or neither (the last step is an Euler step: 5 evaluations, 3 of them in the interval)"""
    pipe, image = pipe_for(dev), control_image(1)
    lat = sampled(pipe, dev, sampler="heun", controlnet_image_path=image, controlnet_scale=SCALE_P, controlnet_interval=(0.3, 1))
    assert pipe.last_sampler["model_evals"] == 5 and pipe.last_controlnet["evals"] == 3
    parity(lat, loop_references(pipe, image, sampler="heun", interval=(0.3, 1)), "heun, interval (0.3, 1)")


def test_pipeline_guidance_interval_halves_the_batch(dev):
    """a guidance interval that leaves the last evaluation unguided: both engines are re-prepared for the prompt rows alone, mid-run"""
    pipe, image = pipe_for(dev), control_image(1)
    lat = sampled(pipe, dev, controlnet_image_path=image, controlnet_scale=SCALE_P, guidance_interval=(0.7, 2.0))
    assert (pipe.last_guidance["guided_evals"], pipe.last_guidance["unguided_evals"]) == (2, 1) and pipe.last_controlnet["evals"] == STEPS
    parity(lat, loop_references(pipe, image, guidance_interval=(0.7, 2.0)), "guidance interval (0.7, 2.0)")
    assert pipe.controlnet.batch == 1 and pipe.mmdit.batch == 1


def test_pipeline_two_seeds_two_control_images(dev):
    """seed = [2, 3] with one control image each: every image against its own oracle loop"""
    pipe, images = pipe_for(dev), [control_image(1), control_image(2)]
    both = sampled(pipe, dev, seed=[2, 3], controlnet_image_path=images, controlnet_scale=SCALE_P)
    for i, s in enumerate((2, 3)):
        parity(both[i:i + 1], loop_references(pipe, images[i], seed=s), f"seed {s} with its control image")
    swapped = sampled(pipe, dev, seed=[2, 3], controlnet_image_path=images[::-1], controlnet_scale=SCALE_P)
    assert not same_bits(both, swapped)


def test_pipeline_refusals_on_the_device(dev):
    pipe, image = pipe_for(dev), control_image(1)
    text, pooled = pipe_inputs()
    run = lambda p, **kw: p.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=2, cfg_weight=CFGW, latent_size=(HL_P, WL_P), seed=0, **kw)
    with pytest.raises(ValueError, match="needs controlnet_image_path in every call"):
        run(pipe)
    with pytest.raises(ValueError, match="need a pipeline built with a ControlNet"):
        run(pipe_for(dev, controlnet=False), controlnet_image_path=image)
    with pytest.raises(ValueError, match="block_cache"):
        run(pipe, controlnet_image_path=image, block_cache=0.1)
    with pytest.raises(ValueError, match="skip-layer or perturbed-attention"):
        run(pipe, controlnet_image_path=image, pag_scale=3.0, pag_layers=[1])
    with pytest.raises(ValueError, match="output's size"):
        run(pipe, controlnet_image_path=image[:, :64])


def test_pipeline_float16_img2img_inpainting(dev):
    """the compositions no oracle loop above covers, in one run: a float16 pipeline, img2img from an encoded image, a half mask.  Scale 0 gives the
    bits of the same call on a float16 pipeline without a ControlNet (x + 0 * tap = x: the whole controlled path ran and changed nothing), a
    nonzero scale moves the repainted half and leaves the kept half what the blend makes it"""
    from diffusionkit_amd.config import tiny_vae, tiny_vae_encoder
    from diffusionkit_amd.pipeline import DiffusionPipeline
    from tests.test_gpu_inpaint import HALF, RGB
    kw = dict(model_version=SD3_VERSION, w16=True, a16=True, shift=SHIFT, mmdit_config=PIPE_MAIN, vae_config=tiny_vae(), vae_encoder_config=tiny_vae_encoder(),
              device=dev, text_len=16, activation_dtype="float16")
    with_cn = DiffusionPipeline(controlnet_ckpt=synth_mmdit_weights(PIPE_CN, seed=4321), controlnet_config=PIPE_CN, **kw)
    without = DiffusionPipeline(**kw)
    assert with_cn.controlnet.dtype == F16 and with_cn.mmdit.dtype == F16
    text, pooled = pipe_inputs()
    call = lambda p, **c: p.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=4, cfg_weight=CFGW, latent_size=(HL_P, WL_P), seed=2,
                                            image_path=RGB, denoise=0.75, mask_path=HALF, sampler="ab2", **c)[0]
    image = control_image(1)
    plain = call(without)
    off = call(with_cn, controlnet_image_path=image, controlnet_scale=0.0)
    on = call(with_cn, controlnet_image_path=image, controlnet_scale=SCALE_P)
    assert with_cn.last_controlnet["evals"] == 3 and bool(torch.isfinite(on).all())
    assert same_bits(off, plain)
    assert same_bits(on[:, :, :WL_P // 2], plain[:, :, :WL_P // 2]), "the kept half of the latent"
    assert rel_l2(plain[:, :, WL_P // 2:], on[:, :, WL_P // 2:]) > 0.05, "the repainted half"
