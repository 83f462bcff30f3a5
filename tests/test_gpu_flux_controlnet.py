"""FLUX ControlNet on the MI355X: the one-job joint LayerNorm pass with a residual tap in front of its image rows bit for bit against the plain
pass and the fp64 add, its footprint, the ControlNet engine against ``tests/_flux_controlnet.FluxControlNetOracle``, the main engine with double-
and single-block taps against ``ControlledFluxOracle``, the chain of the two at the production width, both engines on guarded, poisoned
workspaces, the refusals, and the pipeline's step loop against the oracle loop.

The gates are the project's own (tests/test_gpu_model.py: err(hip, fp32) <= 2 err(emu, fp32) + 2e-3 and PSNR > 35 dB); nothing here sets a
tolerance of its own.  Arithmetic parity on synthetic weights: no ControlNet checkpoint has been run."""
from dataclasses import replace

import pytest
import torch

from diffusionkit_amd.config import FLUX_SCHNELL, fp8_config, tiny_flux, tiny_flux_controlnet, flux_controlnet_config
from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
from oracle.mmdit import Prec, embed_dtype
from tests._engine_state import FILL_NAN, GuardedWorkspace, lend
from tests._flux_controlnet import (TAP_SCALE, ControlledFluxOracle, FluxChainOracle, FluxControlNetOracle, evaluations_active, flux_tap_index,
                                    sd3_tap_index, synthetic_taps, to_diffusers_flux_controlnet)
from tests._footprint import NAN, SENTINEL, assert_footprint, bits, guarded
from tests._util import BF, psnr, randn, rel_l2
from tests.test_gpu_model import psnr_ok, yardstick_ok

pytestmark = pytest.mark.gpu

TS = [1000.0, 752.0, 500.0]


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
ROWS = [(1, 0, 5), (2, 3, 5), (2, 8, 70), (3, 5, 6)]  # (B, S_t, S_i)


def kernel_case(dev, h, B, S_t, S_i):
    """a joint [B, S_t + S_i, h] stream (text rows first), a dense tap of the image rows alone and one modulation table of two rows"""
    g = torch.Generator().manual_seed(h + 100 * B + 10 * S_t + S_i)
    joint = (torch.randn(B, S_t + S_i, h, generator=g) * 2 + 0.5).to(dev, BF)
    tap = torch.randn(B, S_i, h, generator=g).to(dev, BF)
    tab = (torch.randn(B, 2 * h, generator=g) * 0.5).to(dev, BF)
    return joint, tap, tab[:, :h], tab[:, h:]


@pytest.mark.parametrize("rows", ROWS, ids=[f"B{b}_St{t}_Si{i}" for b, t, i in ROWS])
@pytest.mark.parametrize("h", [256, 320, 3072])
def test_ln_modulate_add_joint_bit_for_bit(dev, h, rows):
    """h 256 / 320: lanes past the row end in the only pass (320: a partial last chunk); 3072: six full passes, the production width.
    (1, 0, 5): the image-only form, the final layer's, and a last workgroup with one row; (2, 3, 5): 16 rows, every workgroup straddles a text /
    image seam; (2, 8, 70): 156 rows, seams inside workgroups and a batch-row seam at row 78, not a multiple of 4; (3, 5, 6): 33 rows, three
    batch rows of 11 -- no seam on a workgroup boundary."""
    from diffusionkit_amd import ops
    B, S_t, S_i = rows
    joint0, tap, sh, sc = kernel_case(dev, h, B, S_t, S_i)
    plain = ops.ln_modulate(joint0.clone(), sh, sc)
    for s in (1.0, 0.7, 0.0):
        joint = joint0.clone()
        want = (joint0[:, S_t:].double() + torch.tensor(s, dtype=torch.float32).double() * tap.double()).float().to(BF)
        x, out = ops.ln_modulate_add_joint(joint, S_t, tap, s, sh, sc)
        assert x is joint
        assert same_bits(joint[:, :S_t], joint0[:, :S_t]), f"s = {s}: the text rows of x"
        assert same_bits(joint[:, S_t:], want), f"s = {s}: the image rows written back"
        assert same_bits(out, ops.ln_modulate(joint.clone(), sh, sc)), f"s = {s}: the modulated rows"
        assert (s == 0.0) == same_bits(out, plain)
        if s == 0.0:
            assert same_bits(joint, joint0)
    joint = joint0.clone()
    _, out = ops.ln_modulate_add_joint(joint, S_t, torch.zeros_like(tap), 0.7, sh, sc)
    assert same_bits(out, plain) and same_bits(joint, joint0)


def launch_joint(x, S, S_t, tap, s, out, sh, sc):
    """dk_ln_modulate_add_joint_bf16 on caller-owned buffers (ops.ln_modulate_add_joint allocates its output: no margins to check)"""
    from diffusionkit_amd import _lib
    from diffusionkit_amd.ops import _stream
    B, h = x.shape[0], x.shape[2]
    _lib.check(_lib.load().dk_ln_modulate_add_joint_bf16(x.data_ptr(), h, tap.data_ptr(), h, float(s), S, S_t, out.data_ptr(), h, B * S, h, sh.data_ptr(),
                                                         sc.data_ptr(), sh.stride(0), S, B * S, 0, 1e-6, _stream()), "dk_ln_modulate_add_joint_bf16")


@pytest.mark.parametrize("rows", [(2, 3, 5), (3, 5, 6)], ids=["B2_St3_Si5", "B3_St5_Si6"])
def test_ln_modulate_add_joint_footprint(dev, rows):
    """h 320.  The tap is EXACTLY [B S_i, h] between NaN margins: a tap row read for a text row -- or past either end -- would poison the clean
    run.  A NaN in one tap element reaches exactly that element of x' and that row of out; a NaN in a text row of x reaches that row of out and is
    not written back; the margins around x, the tap and out stay what they were."""
    h = 320
    B, S_t, S_i = rows
    S = S_t + S_i
    joint0, tap0, sh, sc = kernel_case(dev, h, B, S_t, S_i)
    b, ti, tt = B - 1, S_i - 2, S_t - 1
    runs = {}
    for name in ("clean", "tap", "text"):
        joint, gj = guarded(joint0, 2)
        tap, gt = guarded(tap0, 2)
        out, go = guarded(torch.full((B, S, h), SENTINEL, dtype=BF, device=dev), 2, fill=SENTINEL)
        if name == "tap":
            tap[b, ti, 123] = NAN
        if name == "text":
            joint[b, tt, 200] = NAN
        launch_joint(joint, S, S_t, tap, 0.7, out, sh, sc)
        torch.cuda.synchronize()
        for g, what in ((gj, "x"), (gt, "tap"), (go, "out")):
            g.check(f"{name}: {what}")
        runs[name] = (joint.clone(), out.clone())
    clean = runs["clean"]
    assert same_bits(clean[0][:, :S_t], joint0[:, :S_t]) and not same_bits(clean[0][:, S_t:], joint0[:, S_t:])
    none = lambda t: torch.zeros(t.shape, dtype=torch.bool)
    e_x, e_out = none(clean[0]), none(clean[1])
    e_x[b, S_t + ti, 123] = True
    e_out[b, S_t + ti, :] = True
    assert_footprint(clean[0], runs["tap"][0], e_x, "tap NaN: x")
    assert_footprint(clean[1], runs["tap"][1], e_out, "tap NaN: out")
    e_x, e_out = none(clean[0]), none(clean[1])
    e_x[b, tt, 200] = True
    e_out[b, tt, :] = True
    assert_footprint(clean[0], runs["text"][0], e_x, "text NaN: x")
    assert_footprint(clean[1], runs["text"][1], e_out, "text NaN: out")


# ---- the ControlNet engine ----------------------------------------------------------------------------------------------------------
def build(cfg, dev, seed=1234):
    from diffusionkit_amd.engine import MMDiTEngine
    return MMDiTEngine(cfg, pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=seed), dev))


def inputs(cfg, B, Hl, Wl, S_t):
    return (randn(B, S_t, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, Hl, Wl, 16, seed=5),
            randn(B, Hl, Wl, 16, seed=6))


def prepared(cfg, dev, B, Hl, Wl, S_t, seed=1234):
    eng = build(cfg, dev, seed)
    text, pooled, lat, ctrl = inputs(cfg, B, Hl, Wl, S_t)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(pooled.to(dev), TS)
    return eng, text.to(dev, BF), eng.patchify(lat.to(dev)), ctrl.to(dev)


_oracle_cache = {}


def cn_oracle(cfg, B, Hl, Wl, S_t, step=1):
    """fp32 and bf16-emulating FluxControlNetOracle on the seeded case: taps [n, B, S_i, h], computed once per case"""
    key = ("cn", cfg, B, Hl, Wl, S_t, step)
    if key not in _oracle_cache:
        wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
        text, pooled, lat, ctrl = inputs(cfg, B, Hl, Wl, S_t)
        res = {}
        for name, P in (("fp32", Prec()), ("emu", Prec(BF))):
            m = FluxControlNetOracle(cfg, wf, P)
            m.cache_modulation_params(pooled, torch.tensor(TS))
            res[name] = m(lat, text, TS[step], ctrl)
        _oracle_cache[key] = res
    return _oracle_cache[key]


CN_TINY = {"2+2": (tiny_flux_controlnet(2, 2), 2, 8, 12, 20), "3+0_35tok": (tiny_flux_controlnet(3, 0), 1, 10, 14, 20)}


@pytest.mark.parametrize("name", list(CN_TINY))
def test_controlnet_taps_tiny(dev, name):
    """(2, 2): taps behind double and behind single blocks, the latter read from the image rows of the joint stream; (3, 0): no single blocks, the
    last block's text stream stops after attention; 35 image tokens: an odd count on every tile"""
    cfg, B, Hl, Wl, S_t = CN_TINY[name]
    eng, text, tok, ctrl = prepared(cfg, dev, B, Hl, Wl, S_t)
    assert eng.control_net and eng.control_net_flux and eng.mod_rows() == cfg.num_modulation_rows()
    eng.cache_control_image(ctrl, per_image=True)
    taps = eng.control_forward(tok, text, 1)
    n = cfg.depth_multimodal + cfg.depth_unified
    assert tuple(taps.shape) == eng.taps_shape() == (n, B, (Hl // 2) * (Wl // 2), cfg.hidden_size)
    res = cn_oracle(cfg, B, Hl, Wl, S_t)
    for j in range(n):
        e_h, e_e = yardstick_ok(taps[j].float(), res["emu"][j], res["fp32"][j], f"{name} tap {j}")
        p_h, _ = psnr_ok(taps[j].float(), res["emu"][j], res["fp32"][j], f"{name} tap {j}")
        print(f"[flux controlnet] {name} tap {j}: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR {p_h:.1f} dB")
    assert all(rel_l2(res["fp32"][0], res["fp32"][j]) > 0.5 for j in range(1, n))  # (the taps are different tensors)


def test_controlnet_shared_image_and_recache(dev):
    """one control image for both batch rows gives the bits of a per-image copy of it; a second cache_control_image replaces the first"""
    cfg, B, Hl, Wl, S_t = CN_TINY["2+2"]
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


# ---- the main engine with taps ------------------------------------------------------------------------------------------------------
# name -> (double blocks, single blocks, double taps, single taps)
MAIN = {"4+3_taps3+2": (4, 3, 3, 2), "4+3_taps4+3": (4, 3, 4, 3), "4+3_taps4+0": (4, 3, 4, 0), "4+3_taps0+3": (4, 3, 0, 3), "3+0_taps3+0": (3, 0, 3, 0)}
SHAPE = (2, 8, 12, 20)  # B, Hl, Wl, S_t


def main_oracle(cfg, nd_taps, ns_taps, step=1):
    """the final layer's output of the fp32 and the bf16-emulating ControlledFluxOracle under the synthetic taps, and of the fp32 one without"""
    B, Hl, Wl, S_t = SHAPE
    key = ("main", cfg, nd_taps, ns_taps, step)
    if key not in _oracle_cache:
        wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
        text, pooled, lat, _ = inputs(cfg, B, Hl, Wl, S_t)
        control = (synthetic_taps(nd_taps + ns_taps, B, (Hl // 2) * (Wl // 2), cfg.hidden_size), nd_taps, TAP_SCALE)
        res = {}
        for name, P, c in (("fp32", Prec(), control), ("emu", Prec(BF), control), ("plain", Prec(), None)):
            m = ControlledFluxOracle(cfg, wf, P)
            m.control = c
            m.cache_modulation_params(pooled, torch.tensor(TS))
            streams = {}
            m(lat, text, TS[step], taps=streams)
            res[name] = streams["final"]
        _oracle_cache[key] = res
    return _oracle_cache[key]


@pytest.mark.parametrize("name", list(MAIN))
def test_main_engine_with_taps(dev, name):
    """(4, 3) blocks with (3, 2) taps: double taps 0, 0, 1, 1 where the SD3 rule reads 0, 0, 1, 2, single taps 0, 0, 1; with (4, 3): one tap per
    block -- every site counts (tests/test_flux_controlnet_cpu.py shows each moves the oracle by ten times the gate); (4, 0) / (0, 3): one kind
    alone, the tap behind the last double block still lands in single block 0 / none does; (3, 0) blocks: no single blocks, the tap behind the
    last double block lands in the final layer."""
    n_double, n_single, nd, ns = MAIN[name]
    if name == "4+3_taps3+2":
        assert [flux_tap_index(g, nd, n_double) for g in range(n_double)] == [0, 0, 1, 1] != [sd3_tap_index(g, nd, n_double) for g in range(n_double)]
        assert [flux_tap_index(g, ns, n_single) for g in range(n_single)] == [0, 0, 1]
    cfg = tiny_flux(n_double, n_single)
    B, Hl, Wl, S_t = SHAPE
    eng, text, tok, _ = prepared(cfg, dev, B, Hl, Wl, S_t)
    taps = synthetic_taps(nd + ns, B, tok.shape[1], cfg.hidden_size).to(dev, BF)
    plain = eng.forward_tokens(tok, text, 1).clone()
    eng.set_flux_control_taps(taps, nd, TAP_SCALE)
    out = eng.forward_tokens(tok, text, 1).clone()
    res = main_oracle(cfg, nd, ns)
    moved = rel_l2(res["plain"], res["fp32"])
    e_h, e_e = yardstick_ok(out.float(), res["emu"], res["fp32"], name)
    p_h, p_e = psnr_ok(out.float(), res["emu"], res["fp32"], name)
    print(f"[flux controlnet] main {name}: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR {p_h:.1f} dB (emulation {p_e:.1f}); the taps move "
          f"the output by {moved:.3e}")
    assert moved >= 10 * (2 * e_e + 2e-3), f"the taps move the fp32 oracle's output by {moved:.3e} only: a pass would show nothing"
    assert rel_l2(plain.float(), out.float()) >= 10 * (2 * e_e + 2e-3)
    # scale 0, and taps set and cleared: the plain forward's bits
    eng.set_flux_control_taps(taps, nd, 0.0)
    assert same_bits(eng.forward_tokens(tok, text, 1), plain)
    eng.set_flux_control_taps(taps, nd, TAP_SCALE)
    eng.set_flux_control_taps(None)
    assert eng.control_taps is None and same_bits(eng.forward_tokens(tok, text, 1), plain)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
def chain_oracles(main_cfg, cn_cfg, B, Hl, Wl, S_t, step=1, named=None):
    """{fp32, emu: final} of FluxControlNetOracle -> taps -> ControlledFluxOracle, each side in the precision named.  The fp32 side evaluates the
    timestep embedding in the configuration's dtype, as the reference does whatever the activation dtype is (oracle/mmdit.py, ``embed_prec``): at
    h = 3072 the modulation is of order one, and an exact embedding would put the fp32 side 20 % away from ANY implementation of the model
    (22.5 dB, the emulation included) -- a gate that passes everything"""
    text, pooled, lat, ctrl = inputs(main_cfg, B, Hl, Wl, S_t)
    named = named or (synth_mmdit_weights(main_cfg, seed=1234), synth_mmdit_weights(cn_cfg, seed=4321))
    wm, wc = ({k: v.float() for k, v in w.items()} for w in named)
    out = {}
    for name, P, kw in (("fp32", Prec(), dict(embed_prec=Prec(embed_dtype(main_cfg)))), ("emu", Prec(BF), {})):
        cn, main = FluxControlNetOracle(cn_cfg, wc, P, **kw), ControlledFluxOracle(main_cfg, wm, P, **kw)
        for m in (cn, main):
            m.cache_modulation_params(pooled, torch.tensor(TS))
        main.control = (cn(lat, text, TS[step], ctrl), cn_cfg.depth_multimodal, TAP_SCALE)
        streams = {}
        main(lat, text, TS[step], taps=streams)
        out[name] = streams["final"]
    return out


def chain_engines(main_cfg, cn_cfg, dev, B, Hl, Wl, S_t, step=1, engines=None):
    text, pooled, lat, ctrl = inputs(main_cfg, B, Hl, Wl, S_t)
    main, cn = engines or (build(main_cfg, dev, 1234), build(cn_cfg, dev, 4321))
    for e in (main, cn):
        e.prepare(B, (Hl, Wl), S_t, len(TS))
        e.cache_modulation_params(pooled.to(dev), TS)
    cn.cache_control_image(ctrl.to(dev), per_image=True)
    tok, text = main.patchify(lat.to(dev)), text.to(dev, BF)
    taps = cn.control_forward(tok, text, step)
    main.set_flux_control_taps(taps, cn_cfg.depth_multimodal, TAP_SCALE)
    return main.forward_tokens(tok, text, step)


def test_chain_production_width(dev):
    """FLUX.1's width (h 3072, 24 heads of 128, RoPE axes 16 + 56 + 56): main (1, 1), ControlNet (1, 1), batch 1, latent 4 x 8, S_t 8 -- the joint
    LayerNorm pass at NCH = 6 in single block 0 and in the final layer"""
    main_cfg = replace(FLUX_SCHNELL, depth_multimodal=1, depth_unified=1, token_level_text_embed_dim=256, pooled_text_embed_dim=64)
    cn_cfg = flux_controlnet_config(1, 1, main_cfg)
    assert main_cfg.hidden_size == cn_cfg.hidden_size == 3072 and main_cfg.head_dim == 128 and main_cfg.num_heads == 24
    from diffusionkit_amd.engine import MMDiTEngine
    named = (synth_mmdit_weights(main_cfg, seed=1234), synth_mmdit_weights(cn_cfg, seed=4321))  # (drawn once: half a billion values each)
    engines = tuple(MMDiTEngine(c, pack_mmdit(c, w, dev)) for c, w in zip((main_cfg, cn_cfg), named))
    out = chain_engines(main_cfg, cn_cfg, dev, 1, 4, 8, 8, engines=engines)
    res = chain_oracles(main_cfg, cn_cfg, 1, 4, 8, 8, named=named)
    e_h, e_e = yardstick_ok(out.float(), res["emu"], res["fp32"], "chain at width")
    p_h, p_e = psnr_ok(out.float(), res["emu"], res["fp32"], "chain at width")
    print(f"[flux controlnet] chain at width: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR {p_h:.1f} dB (emulation {p_e:.1f})")


# ---- workspaces -----------------------------------------------------------------------------------------------------------------------
def test_chain_on_guarded_poisoned_workspaces(dev):
    """both engines on NaN-filled interiors of exactly the declared size, the taps tensor between NaN margins: the bits of the plain run and
    nothing written outside; then a smaller problem in the same (stale) allocations, the engines reused"""
    main_cfg, cn_cfg = tiny_flux(3, 2), tiny_flux_controlnet(2, 1)
    main, cn = build(main_cfg, dev, 1234), build(cn_cfg, dev, 4321)
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
        main.set_flux_control_taps(taps, cn_cfg.depth_multimodal, TAP_SCALE)
        out = main.forward_tokens(tok, text, 1)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(taps.float()).all())
        assert same_bits(out, ref), f"shape {k}: the guarded run differs from the plain one"
        gt.check(f"shape {k}: taps")
        for e, what in ((main, "main engine"), (cn, "control-net engine")):
            ws[e].check(nbytes[e][k], f"shape {k}: {what}", fill=FILL_NAN if k == 0 else None)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_engine_refusals(dev):
    from diffusionkit_amd._lib import DkHipError
    B, Hl, Wl, S_t = SHAPE
    cfg = tiny_flux(2, 2)
    eng, text, tok, ctrl = prepared(cfg, dev, B, Hl, Wl, S_t)
    S_i, h = tok.shape[1], cfg.hidden_size
    taps = lambda n: torch.zeros(n, B, S_i, h, dtype=BF, device=dev)
    # the SD3 entries on FLUX geometry
    with pytest.raises(DkHipError, match="SD3 family"):
        eng.set_control_taps(taps(1))
    with pytest.raises((DkHipError, ValueError), match="SD3 family"):
        build(replace(tiny_flux(), control_net=True), dev)
    with pytest.raises(DkHipError, match="n_double_taps"):
        eng.set_flux_control_taps(taps(3), 3)
    with pytest.raises(DkHipError, match="n_single_taps"):
        eng.set_flux_control_taps(taps(3), 0)
    with pytest.raises(DkHipError, match="taps shape"):
        eng.set_flux_control_taps(torch.zeros(2, B, S_i + 1, h, dtype=BF, device=dev), 1)
    eng.set_flux_control_taps(taps(4), 2)
    x = torch.zeros(B, S_t + S_i, h, dtype=BF, device=dev)
    with pytest.raises(DkHipError, match="dk_mmdit_set_flux_control_taps"):
        eng.run_blocks(x, 1, 0)
    # (head and tail need the block cache, which cannot be on beside taps: they refuse on either ground, and never launch)
    with pytest.raises(DkHipError):
        eng.forward_head(tok, text, 1)
    with pytest.raises(DkHipError):
        eng.forward_tail(1, False)
    with pytest.raises(DkHipError, match="control taps"):
        eng.enable_block_cache(True)
    eng.set_flux_control_taps(None)
    eng.run_blocks(x, 1, 0)
    # the block cache: taps refuse while it is on
    eng.enable_block_cache(True)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    with pytest.raises(DkHipError, match="block cache"):
        eng.set_flux_control_taps(taps(4), 2)
    eng.enable_block_cache(False)
    # a reference grid
    eng.prepare(B, (Hl, Wl), S_t, len(TS), reference_size=(Hl, Wl))
    with pytest.raises(DkHipError, match="reference grid"):
        eng.set_flux_control_taps(taps(4), 2)
    # a condition width
    ccfg = tiny_flux(2, 2, condition_features=64)
    cond = build(ccfg, dev)
    cond.prepare(B, (Hl, Wl), S_t, len(TS))
    with pytest.raises(DkHipError, match="condition width"):
        cond.set_flux_control_taps(taps(4), 2)
    # fp8 Linears
    f8 = build(fp8_config(tiny_flux(2, 2), "speed"), dev)
    f8.prepare(1, (8, 16), 128, 1)
    with pytest.raises(DkHipError, match="fp8"):
        f8.set_flux_control_taps(torch.zeros(4, 1, 32, h, dtype=BF, device=dev), 2)
    # the control-net engine
    cn, ctext, ctok, cctrl = prepared(tiny_flux_controlnet(2, 2), dev, B, Hl, Wl, S_t)
    with pytest.raises(DkHipError, match="cache_control_image"):
        cn.control_forward(ctok, ctext, 1)
    cn.cache_control_image(cctrl, per_image=True)
    with pytest.raises(DkHipError, match="dk_mmdit_control_forward"):
        cn.forward_tokens(ctok, ctext, 1)
    with pytest.raises(DkHipError, match="control-net engine"):
        cn.set_flux_control_taps(taps(4), 2)
    with pytest.raises(DkHipError, match="control_net"):
        eng.control_forward(tok, text, 1)


# ---- step loop and pipeline -----------------------------------------------------------------------------------------------------------
STEPS, HL_P, WL_P, SCALE_P = 3, 8, 16, 0.8
PIPE_MAIN, PIPE_CN = tiny_flux(3, 2), tiny_flux_controlnet(2, 1)
_PIPES = {}


def control_image(seed):
    import numpy as np
    return (np.random.RandomState(seed).rand(HL_P * 8, WL_P * 8, 3) * 255).astype(np.uint8)


def pipe_for(dev, controlnet=True, ckpt=None):
    """one tiny FLUX pipeline with the ControlNet (from reference-named tensors, or from ``ckpt``) and one without, for the whole module"""
    from diffusionkit_amd.config import tiny_vae, tiny_vae_encoder
    from diffusionkit_amd.pipeline import FluxPipeline
    key = (controlnet, ckpt)
    if key not in _PIPES:
        kw = dict(controlnet_ckpt=ckpt or synth_mmdit_weights(PIPE_CN, seed=4321), controlnet_config=PIPE_CN) if controlnet else {}
        _PIPES[key] = FluxPipeline(w16=True, a16=True, mmdit_config=PIPE_MAIN, vae_config=tiny_vae(), vae_encoder_config=tiny_vae_encoder(), device=dev,
                                   text_len=16, **kw)
    return _PIPES[key]


def pipe_inputs():
    return randn(1, 16, PIPE_MAIN.token_level_text_embed_dim, seed=7), randn(1, PIPE_MAIN.pooled_text_embed_dim, seed=8)


def sampled(pipe, dev, seed=0, **kw):
    text, pooled = pipe_inputs()
    n = len(seed) if isinstance(seed, list) else 1
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=STEPS, cfg_weight=0.0, latent_size=(HL_P, WL_P), seed=seed, **kw)
    assert lat.shape == (n, HL_P, WL_P, 16) and lat.dtype == torch.float32
    return lat


def loop_references(pipe, image, seed=0, sampler="euler", interval=None):
    """the oracle chain as ONE model in the restated step loop (tests/test_samplers_cpu.py's ``plan_loop``), on the fp32 and the bf16-emulating
    oracle, after process_out.  The control latent is the pipeline's own (its VAE encoder is not under test here)."""
    import numpy as np
    from diffusionkit_amd.sampler import step_plan
    from oracle import pipeline as op
    from tests.test_samplers_cpu import plan_loop, start_state
    text, pooled = pipe_inputs()
    ctrl = pipe.latent_format.process_in(pipe.encode_reference_to_latents(np.ascontiguousarray(image[None]))).float().cpu()
    wm = {k: v.float() for k, v in synth_mmdit_weights(PIPE_MAIN, seed=1234).items()}
    wc = {k: v.float() for k, v in synth_mmdit_weights(PIPE_CN, seed=4321).items()}
    sigmas = op.get_sigmas(1.0, True, STEPS)
    active = evaluations_active(step_plan(sampler, sigmas.numpy()), interval)
    res = {}
    for name, P in (("fp32", Prec()), ("emu", Prec(BF))):
        chain = FluxChainOracle(ControlledFluxOracle(PIPE_MAIN, wm, P), FluxControlNetOracle(PIPE_CN, wc, P), ctrl, SCALE_P, active)
        x0, _ = start_state(sigmas, seed, HL_P, WL_P)
        res[name] = op.process_out(plan_loop(chain, sampler, x0, sigmas, text, pooled, 0.0, Prec(BF)), "flux")
        assert chain.calls == len(active)
    return res


def parity(lat, res, what):
    e_h, e_e = yardstick_ok(lat, res["emu"], res["fp32"], what)
    p_h, p_e = psnr(res["fp32"], lat), psnr(res["fp32"], res["emu"])
    print(f"[flux controlnet] {what}: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR hip {p_h:.1f} dB / emu {p_e:.1f} dB")
    assert p_h > 35.0, f"{what}: PSNR {p_h:.1f} dB"


def test_pipeline_from_a_diffusers_layout_file(dev, tmp_path):
    """3 Euler steps, tiny VAE, the ControlNet loaded from a file in the diffusers FluxControlNetModel layout: the final latent against the oracle
    loop, the bits of the same weights handed over by name, and -- with scale 0 -- the bits of a pipeline without a ControlNet"""
    import os
    from safetensors.torch import save_file
    path = os.path.join(tmp_path, "flux_controlnet.safetensors")
    save_file(to_diffusers_flux_controlnet(synth_mmdit_weights(PIPE_CN, seed=4321), PIPE_CN), path)
    pipe, image = pipe_for(dev, ckpt=path), control_image(1)
    assert pipe.controlnet.control_net_flux and pipe.controlnet.mod_rows() == PIPE_CN.num_modulation_rows()
    lat = sampled(pipe, dev, controlnet_image_path=image, controlnet_scale=SCALE_P)
    assert pipe.last_controlnet == {"scale": SCALE_P, "interval": None, "evals": STEPS} and pipe.mmdit.control_taps is None
    parity(lat, loop_references(pipe, image), "pipeline, euler")
    named = pipe_for(dev)
    assert same_bits(lat, sampled(named, dev, controlnet_image_path=image, controlnet_scale=SCALE_P))
    plain = sampled(pipe_for(dev, controlnet=False), dev)
    assert not same_bits(lat, plain) and rel_l2(plain, lat) > 0.05
    assert same_bits(sampled(named, dev, controlnet_image_path=image, controlnet_scale=0.0), plain)


def test_pipeline_heun_and_interval(dev):
    """--sampler heun with controlnet_interval = (0.3, 1): two evaluations per step, both controlled or neither (5 evaluations, 3 of them in the
    interval); euler with (0, 0.67): the last step runs uncontrolled; an interval that holds no step: the plain pipeline's bits"""
    pipe, image = pipe_for(dev), control_image(1)
    lat = sampled(pipe, dev, sampler="heun", controlnet_image_path=image, controlnet_scale=SCALE_P, controlnet_interval=(0.3, 1))
    assert pipe.last_sampler["model_evals"] == 5 and pipe.last_controlnet["evals"] == 3
    parity(lat, loop_references(pipe, image, sampler="heun", interval=(0.3, 1)), "heun, interval (0.3, 1)")
    lat = sampled(pipe, dev, controlnet_image_path=image, controlnet_scale=SCALE_P, controlnet_interval=(0, 0.67))
    assert pipe.last_controlnet["evals"] == 2 and pipe.mmdit.control_taps is None
    parity(lat, loop_references(pipe, image, interval=(0, 0.67)), "euler, interval (0, 0.67)")
    none = sampled(pipe, dev, controlnet_image_path=image, controlnet_scale=SCALE_P, controlnet_interval=(0.5, 0.5))
    assert pipe.last_controlnet["evals"] == 0 and same_bits(none, sampled(pipe_for(dev, controlnet=False), dev))


def test_pipeline_two_seeds_two_control_images(dev):
    """seed = [2, 3] with one control image each: every image against its own oracle loop"""
    pipe, images = pipe_for(dev), [control_image(1), control_image(2)]
    both = sampled(pipe, dev, seed=[2, 3], controlnet_image_path=images, controlnet_scale=SCALE_P)
    for i, s in enumerate((2, 3)):
        parity(both[i:i + 1], loop_references(pipe, images[i], seed=s), f"seed {s} with its control image")
    swapped = sampled(pipe, dev, seed=[2, 3], controlnet_image_path=images[::-1], controlnet_scale=SCALE_P)
    assert not same_bits(both, swapped)


def test_pipeline_img2img_inpainting(dev):
    """img2img from an encoded image with a half mask, sampler ab2 -- checked the way the SD3 ControlNet test checks them, without an oracle loop:
    scale 0 gives the bits of the same call on a pipeline without a ControlNet (x + 0 * tap = x: the whole controlled path ran and changed
    nothing), a nonzero scale moves the repainted half and leaves the kept half what the blend makes it"""
    from tests.test_gpu_inpaint import HALF, RGB
    with_cn, without = pipe_for(dev), pipe_for(dev, controlnet=False)
    text, pooled = pipe_inputs()
    call = lambda p, **c: p.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=4, cfg_weight=0.0, latent_size=(HL_P, WL_P), seed=2,
                                            image_path=RGB, denoise=0.75, mask_path=HALF, sampler="ab2", **c)[0]
    image = control_image(1)
    plain = call(without)
    off = call(with_cn, controlnet_image_path=image, controlnet_scale=0.0)
    on = call(with_cn, controlnet_image_path=image, controlnet_scale=SCALE_P)
    assert with_cn.last_controlnet["evals"] == 3 and bool(torch.isfinite(on).all())
    assert same_bits(off, plain)
    assert same_bits(on[:, :, :WL_P // 2], plain[:, :, :WL_P // 2]), "the kept half of the latent"
    assert rel_l2(plain[:, :, WL_P // 2:], on[:, :, WL_P // 2:]) > 0.05, "the repainted half"


def test_pipeline_refusals_on_the_device(dev):
    from diffusionkit_amd.config import tiny_vae
    from diffusionkit_amd.pipeline import FluxPipeline
    pipe, image = pipe_for(dev), control_image(1)
    text, pooled = pipe_inputs()
    run = lambda p, **kw: p.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=2, cfg_weight=0.0, latent_size=(HL_P, WL_P), seed=0, **kw)
    with pytest.raises(ValueError, match="needs controlnet_image_path in every call"):
        run(pipe)
    with pytest.raises(ValueError, match="need a pipeline built with a ControlNet"):
        run(pipe_for(dev, controlnet=False), controlnet_image_path=image)
    with pytest.raises(ValueError, match="block_cache"):
        run(pipe, controlnet_image_path=image, block_cache=0.1)
    with pytest.raises(ValueError, match="reference_image_path"):
        run(pipe, controlnet_image_path=image, reference_image_path=image)
    with pytest.raises(ValueError, match="output's size"):
        run(pipe, controlnet_image_path=image[:, :64])
    kw = dict(w16=True, a16=True, vae_config=tiny_vae(), device=dev, text_len=16, controlnet_ckpt=synth_mmdit_weights(PIPE_CN, seed=4321))
    with pytest.raises(ValueError, match="SD3 family"):
        FluxPipeline(mmdit_config=PIPE_MAIN, **kw)
    with pytest.raises(ValueError, match="fp8"):
        FluxPipeline(mmdit_config=fp8_config(PIPE_MAIN, "speed"), controlnet_config=PIPE_CN, **kw)
    with pytest.raises(ValueError, match="condition="):
        FluxPipeline(mmdit_config=PIPE_MAIN, condition="control", controlnet_config=PIPE_CN, **kw)
