"""Group-masked joint attention (regional prompts; csrc/attention_group.hip) on the GPU: the operator against the float64 masked softmax at the
shapes that reach each hazard of the kernel, its NaN footprint, the engine against a masked oracle with its refusals, and the pipeline."""
import functools
import math

import numpy as np
import pytest
import torch

from diffusionkit_amd import config as C
from diffusionkit_amd import ops, regional
from diffusionkit_amd._lib import DkHipError
from oracle import mmdit as om
from oracle.mmdit import Prec
from tests import _fused_cases as fc
from tests import _regional as R
from tests._footprint import assert_footprint
from tests._gates import BF, C_ROW, inputs, rnd, row_ratio, split_qkv
from tests._util import psnr, randn, rel_l2
from tests.test_gpu_model import build, psnr_ok, yardstick_ok

pytestmark = pytest.mark.gpu
H, D, DEV = 2, 128, "cuda"


@functools.lru_cache(maxsize=None)
def case(name, qfuse):
    """(qkv, qn, words, float64 reference [B, S, H D]) of a layout, computed once"""
    B, S, words = R.LAYOUTS[name]
    qkv = inputs(BF, B, S, 3 * H * D, seed=50 + len(name))
    q, k, v = split_qkv(qkv, H, D)
    qn = None
    if qfuse:  # the fused query load: QKNorm with two weights split inside the first wave, then RoPE (rounded where the kernel rounds)
        qa, qb, tab, split = rnd(inputs(BF, D, seed=3, scale=0.05) + 0.5, BF), rnd(inputs(BF, D, seed=4, scale=0.05) + 1.5, BF), fc.rope_table_for("angle", S, D), 21
        w = torch.where((torch.arange(S) < split)[:, None], qa[None, :], qb[None, :])
        q = rnd(om.rope_apply(rnd(om.rms_norm(q, w, fc.KN_EPS, Prec()), BF), tab, Prec()), BF)
        qn = (qa, qb, split, tab)
    mask = R.allowed(words).repeat_interleave(H, dim=0)
    ref = R.masked_ref64(q, k, v, 1.0 / math.sqrt(D), mask)
    return qkv, qn, words, ref.reshape(B, H, S, D).permute(0, 2, 1, 3).reshape(B, S, H * D)


def run(qkv, qn, words):
    qn = qn and (qn[0].to(DEV, BF), qn[1].to(DEV, BF), qn[2], qn[3].to(DEV))
    out = ops.attention_groups(qkv.to(DEV, BF), H, words, qn=qn)
    torch.cuda.synchronize()
    return out.float().cpu()


@pytest.mark.parametrize("qfuse", [False, True], ids=["plain_q", "fused_q"])
@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_operator_against_float64(name, qfuse):
    qkv, qn, words, ref = case(name, qfuse)
    got = run(qkv, qn, words)
    B, S, _ = got.shape
    rows = lambda t: t.reshape(B, S, H, D)  # the gate is per (row, head)
    assert row_ratio(rows(got), rows(ref), C_ROW[("attn", BF)], BF) <= 1.0
    if name.startswith("all_full") and not qfuse:  # every pair allowed: the unmasked float64 reference is the same yardstick
        q, k, v = split_qkv(qkv, H, D)
        plain = torch.softmax(q.double() @ k.double().transpose(1, 2) / math.sqrt(D), dim=-1) @ v.double()
        assert row_ratio(rows(got), plain.reshape(B, H, S, D).permute(0, 2, 1, 3), C_ROW[("attn", BF)], BF) <= 1.0


_E, _M, _R = (next(k for k in R.LAYOUTS if k.endswith(sfx)) for sfx in ("S133", "S300", "S70"))
# (layout, query row or None, keys poisoned when the row is None, fused query load)
FOOTPRINTS = [(_E, 97, None, False), (_E, 130, None, False), (_E, 5, None, False), (_M, 131, None, False), (_R, 66, None, False), (_M, None, (200,), False),
              (_E, None, (96,), False), (_M, 131, None, True)]


@pytest.mark.parametrize("name,row,keys,qfuse", FOOTPRINTS,
                         ids=[f"{n.rsplit('_', 1)[1]}-{'row%d' % r if r is not None else 'key%d' % k[0]}{'-fused_q' * q}" for n, r, k, q in FOOTPRINTS])
def test_footprint(name, row, keys, qfuse):
    """K and V of every key a query may not see (skipped tiles, masked keys of mixed tiles) are NaN: that query's output keeps its bits, and a
    NaN key reaches exactly the rows that may see it."""
    qkv, qn, words, _ = case(name, qfuse)
    allow = R.allowed(words)[0]
    poison = (~allow[row]).nonzero().flatten() if row is not None else torch.tensor(keys)
    bad = qkv.clone()
    bad[0, poison, H * D:] = float("nan")
    clean, got = run(qkv, qn, words), run(bad, qn, words)
    expect = torch.zeros_like(clean, dtype=torch.bool)
    expect[0] = allow[:, poison].any(dim=1)[:, None]
    assert row is None or not bool(expect[0, row].any())
    assert_footprint(clean, got, expect, f"{name} row {row} keys {keys}")


TS, REGIONS = [1000.0, 500.0], [{"prompt": "a", "box": (0, 0, 96, 128)}, {"prompt": "b", "box": (96, 0, 192, 128)}]


def engine(B=2, hw=(16, 24), t=45):
    """(engine, fp32 weights, tokens, text, pooled, latent): tiny FLUX, a base prompt and two regions of 15 text tokens, S = 45 + 96 = 141 (two query
    blocks, a ragged third key tile)"""
    eng, wf = build(C.tiny_flux(2, 2), DEV)
    text, pooled, lat = randn(B, t, eng.config.token_level_text_embed_dim, seed=3), randn(B, eng.config.pooled_text_embed_dim, seed=4), randn(B, *hw, 16, seed=5)
    eng.prepare(B, hw, t, len(TS))
    eng.cache_modulation_params(pooled.to(DEV), TS)
    return eng, wf, eng.patchify(lat.to(DEV)), text, pooled, lat


def test_engine_against_masked_oracle():
    eng, wf, tok, text, pooled, lat = engine()
    words = regional.region_words(REGIONS, 8, 12, 15)
    plain = eng.forward_tokens(tok, text.to(DEV, BF), 1).clone()
    eng.set_attention_groups(words)
    out = eng.forward_tokens(tok, text.to(DEV, BF), 1).float().cpu()
    eng.set_attention_groups(None)  # reset: the bits of the forward before the words were ever set
    assert torch.equal(eng.forward_tokens(tok, text.to(DEV, BF), 1), plain) and not torch.equal(out, plain.float().cpu())
    res = {"fp32": {}, "emu": {}}
    for name, P in (("fp32", Prec()), ("emu", Prec(BF))):
        m = R.RegionalOracle(eng.config, wf, P, np.broadcast_to(words, (2, len(words))))
        m.cache_modulation_params(pooled, torch.tensor(TS))
        m(lat, text, TS[1], taps=res[name])
    yardstick_ok(out, res["emu"]["final"], res["fp32"]["final"], "regional"), psnr_ok(out, res["emu"]["final"], res["fp32"]["final"], "regional")


def _taps(eng):
    eng.set_flux_control_taps(torch.zeros(2, 2, eng.tokens_shape()[1], eng.config.hidden_size, dtype=BF, device=DEV), 1)


# state -> the rule named (float16 activations, skip layers and perturbed attention need an engine without single blocks: the geometry rule comes first)
ENGINE_REFUSALS = {"sd3_geometry": "FLUX geometry", "fp8_linears": "fp8_linears", "control_net_engine": "control-net engine or while control taps",
                   "control_taps": "control-net engine or while control taps", "ip_adapter": "IP-Adapter", "reference_grid": "reference grid or a condition width",
                   "condition_width": "reference grid or a condition width", "block_cache": "block cache"}


@pytest.mark.parametrize("name", list(ENGINE_REFUSALS))
def test_engine_refuses(name):
    from tests.test_gpu_ip_adapter import build as build_with_adapter
    flux = C.tiny_flux(2, 2)
    cfg = {"sd3_geometry": C.tiny_sd3(), "fp8_linears": C.fp8_config(flux, "speed"), "control_net_engine": C.tiny_flux_controlnet(2, 1),
           "condition_width": C.tiny_flux(2, 2, condition_features=64)}.get(name, flux)
    eng = build_with_adapter(cfg, DEV) if name == "ip_adapter" else build(cfg, DEV)[0]
    if name == "block_cache":
        eng.enable_block_cache(True)
    eng.prepare(2, (8, 8), 128, 1, **({"reference_size": (8, 8)} if name == "reference_grid" else {}))
    if name == "control_taps":
        _taps(eng)
    with pytest.raises(DkHipError, match=ENGINE_REFUSALS[name]):
        eng.set_attention_groups(np.ones(128 + 16, dtype=np.uint32))


def test_engine_refuses_while_set():
    """the other entries while the words are set, and the rules asked again in front of a forward when another setter came after the words"""
    eng, _, tok, text, _, _ = engine()
    eng.set_attention_groups(regional.region_words(REGIONS, 8, 12, 15))
    with pytest.raises(DkHipError, match="dk_mmdit_run_blocks cannot run while attention groups are set"):
        eng.run_blocks(torch.zeros(2, 141, eng.config.hidden_size, dtype=BF, device=DEV), 1, 0)
    _taps(eng)
    with pytest.raises(DkHipError, match="control taps"):
        eng.forward_tokens(tok, text.to(DEV, BF), 1)


def test_pipeline_two_boxes():
    """generate_image / denoise_latents with two boxes and no base prompt against the same loop on the masked oracle (the gate of smoke()); swapping
    the two prompts changes the latent, swapping prompts and boxes does not, up to that gate"""
    from diffusionkit_amd.pipeline import FluxPipeline
    from diffusionkit_amd.weights import synth_mmdit_weights
    from oracle import pipeline as op
    cfg, T, hw = C.tiny_flux(), 16, (8, 12)
    pipe = FluxPipeline(w16=True, a16=True, mmdit_config=cfg, vae_config=C.tiny_vae(), device=DEV, text_len=T)
    boxes = [(0, 0, 48, 64), (48, 0, 96, 64)]
    (ca, pa), (cb, _) = (pipe.encode_text(t, 0.0) for t in ("a fox", "a lake"))

    def run_regions(order, box_order):
        regions = [{"prompt": "-", "box": boxes[b]} for b in box_order]
        lat, _ = pipe.denoise_latents(torch.cat([(ca, cb)[i] for i in order], 1), pa, num_steps=2, latent_size=hw, seed=0, regions=regions, region_base=False)
        return lat.float().cpu(), regions
    lat, regions = run_regions((0, 1), (0, 1))
    assert pipe.last_regions == {"regions": 2, "base": False, "isolate_image": False, "text_tokens": T, "image_tokens": [12, 12]}
    words = R.groups_for(4, 6, [T, T], boxes, base=False)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    ref = op.denoise_latents(R.RegionalOracle(cfg, wf, Prec(), words[None]), torch.cat([ca, cb], 1)[:1].float().cpu(), pa[:1].float().cpu(), 2, 0.0, hw, 0, 1.0,
                             True, Prec(BF))
    assert psnr(ref, lat) > 35.0
    both, prompts = run_regions((1, 0), (1, 0))[0], run_regions((1, 0), (0, 1))[0]
    assert psnr(lat, both) > 35.0 and rel_l2(lat, prompts) > max(1e-3, 2.0 * rel_l2(lat, both))  # (1e-3: far above a last-bit difference)
    # generate_image encodes and concatenates the same prompts in the documented order with the first region's pooled vector: the same image, bit for bit
    img, log = pipe.generate_image("unused", num_steps=2, latent_size=hw, seed=0, verbose=False, region_base=False,
                                   regions=[{"prompt": "a fox", "box": boxes[0]}, {"prompt": "a lake", "box": boxes[1]}])
    assert log["denoising"]["regions"]["regions"] == 2 and np.array_equal(np.asarray(img), pipe.decoder.decode(lat.to(DEV))[1][0].cpu().numpy())
    with pytest.raises(ValueError, match="block_cache"):
        pipe.denoise_latents(torch.cat([ca, cb], 1), pa, latent_size=hw, regions=regions, region_base=False, block_cache=0.1)
