"""Quantised attention (csrc/attention_f8.hip) on the GPU: the operator against float64 at the smallest shapes that hold each hazard, gated by the error of
the format's own emulation (tests/_attention_fp8.py); its footprint in a poisoned workspace; the engine against the oracle with that emulation; the pipeline."""
import functools
import math

from dataclasses import replace

import numpy as np
import pytest
import torch

from diffusionkit_amd import config as C
from diffusionkit_amd import ops
from diffusionkit_amd._lib import DkHipError
from diffusionkit_amd.weights import synth_mmdit_weights
from oracle import mmdit as om
from oracle.mmdit import Prec
from tests import _fused_cases as fc
from tests._attention_fp8 import emulate
from tests._footprint import guarded
from tests._gates import BF, attn_ref64, inputs, rnd, row_rel, split_qkv
from tests._util import psnr, randn, rel_l2

pytestmark = pytest.mark.gpu
D, DEV = 128, "cuda"
# name -> (B, H, S): the hazard each shape is the smallest for stands in the case's branch below
CASES = {"one_tile": (1, 1, 128), "one_key_in_tile_2": (1, 2, 129), "ragged_batch_heads": (2, 3, 200), "late_key_rescale": (1, 2, 640),
         "v_block_scales": (1, 2, 384), "fused_q": (1, 2, 320)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(qkv, qn, float64 reference, emulation), both [B H, S, D], computed once"""
    B, H, S = CASES[name]
    h = H * D
    qkv = inputs(BF, B, S, 3 * h, seed=70 + len(name))
    # The hazards are made large against the gate (ratios: profiles/attention_fp8.md).  Values carry a common offset of 2: a row then stands above the e4m3
    # roundings it sums and the gate is a few per cent, not N(0, 1)'s 10 % (not in fused_q: its hazard moves six rows' attention pattern, which an offset hides).
    if name != "fused_q":
        qkv[:, :, 2 * h:] = rnd(qkv[:, :, 2 * h:] + 2.0, BF)
    u = (torch.where(torch.arange(D) % 3 == 0, -1.0, 1.0) / math.sqrt(D)).repeat(H)
    if name in ("one_key_in_tile_2", "ragged_batch_heads"):  # queries lean 6 along u, keys 6 against it: every real score lies ~ 3 below the 0 of a
        qkv[:, :, :h] = rnd(qkv[:, :, :h] + 6.0 * u, BF)       # padded key, which would outweigh the row if it were kept
        qkv[:, :, h:2 * h] = rnd(qkv[:, :, h:2 * h] - 6.0 * u, BF)
    if name == "late_key_rescale":  # every query leans 4 along u, key 500 (the fourth tile) is 40 u: its score stands >= 8 above the rest of its row
        qkv[:, :, :h] = rnd(qkv[:, :, :h] + 4.0 * u, BF)
        qkv[:, 500, h:2 * h] = rnd(40.0 * u, BF)
    if name == "v_block_scales":
        # two channels x 64; the aligned 32-key run [160, 192) keeps its magnitude while every other key's values are 2^20 times larger -- under one
        # scale per d row the run would fall below e4m3's subnormals and vanish -- and every query attends to the run alone (its keys are 60 u, the
        # queries lean 10 along u: the other keys' probabilities are below 2^-40)
        qkv[:, :, 2 * h + 5] *= 64.0
        qkv[:, :, 2 * h + D + 77] *= 64.0
        qkv[:, :160, 2 * h:] *= 2.0 ** 20
        qkv[:, 192:, 2 * h:] *= 2.0 ** 20
        qkv[:, :, :h] = rnd(qkv[:, :, :h] + 10.0 * u, BF)
        qkv[:, 160:192, h:2 * h] = rnd(60.0 * u, BF)
    q, k, v = split_qkv(qkv, H, D)
    qn = None
    if name == "fused_q":  # QKNorm with two weights split at row 70 (inside the third wave's rows, no multiple of 32), then RoPE
        qa, qb, tab, split = rnd(inputs(BF, D, seed=3, scale=0.05) + 0.5, BF), rnd(inputs(BF, D, seed=4, scale=0.05) + 1.5, BF), fc.rope_table_for("angle", S, D), 70
        w = torch.where((torch.arange(S) < split)[:, None], qa[None, :], qb[None, :])
        q = om.rope_apply(rnd(om.rms_norm(q, w, fc.KN_EPS, Prec()), BF), tab, Prec())
        qn = (qa, qb, split, tab)
    scale = 1.0 / math.sqrt(D)
    return qkv, qn, attn_ref64(q, k, v, scale), emulate(q, k, v, scale)


def run(name, workspace=None, out=None):
    qkv, qn, _, _ = case(name)
    qn = qn and (qn[0].to(DEV, BF), qn[1].to(DEV, BF), qn[2], qn[3].to(DEV))
    got = ops.attention_fp8(qkv.to(DEV, BF), CASES[name][1], qn=qn, workspace=workspace, out=out)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_operator_against_float64(name):
    """per (query row, head): the kernel's relative error against float64 is at most twice the emulation's worst row -- the format's own error; the
    factor covers the row-to-row scatter of independent roundings, nothing else"""
    B, H, S = CASES[name]
    _, _, ref, emu = case(name)
    got = run(name).float().cpu().reshape(B, S, H, D).permute(0, 2, 1, 3).reshape(B * H, S, D)
    e_emu, e_got = row_rel(emu, ref), row_rel(got, ref)
    print(f"[attention_fp8] {name} B, H, S = {B}, {H}, {S}: emulation {e_emu:.3e}, kernel {e_got:.3e}, kernel against emulation {row_rel(got, emu):.3e}")
    assert bool(torch.isfinite(got).all()) and e_got <= 2.0 * e_emu


def test_footprint_in_a_poisoned_workspace():
    """an exact-size workspace of NaN bytes and an output of NaN: the bits of the clean run, finite; the guard rows around the output keep their poison"""
    name, (B, H, S) = "ragged_batch_heads", CASES["ragged_batch_heads"]
    clean = run(name).cpu()
    ws = torch.full((ops.attention_fp8_workspace_bytes(B, H, S),), 0xFF, dtype=torch.uint8, device=DEV)  # (0xFF: an e4m3 NaN, and 2^128 = NaN as an E8M0 scale)
    out, guard = guarded(torch.full((B, S, H * D), float("nan"), dtype=BF, device=DEV), 1)
    got = run(name, workspace=ws, out=out).cpu()
    assert bool(torch.isfinite(got.float()).all()) and torch.equal(got.view(torch.int16), clean.view(torch.int16))
    guard.check("attention_fp8 output")


# ---- engine and pipeline: MMDiTConfig(attention_dtype="fp8_e4m3") on the small FLUX geometry of tests/test_gpu_regional.py ------------------------
class Fp8AttentionOracle(om.OracleMMDiT):  # the FLUX oracle whose joint attention, in every double and single block, is the emulation
    def __call__(self, *args, **kw):
        plain = om.sdpa
        om.sdpa = lambda q, k, v, scale, P: P.r(emulate(*(t.reshape(-1, *t.shape[-2:]) for t in (q, k, v)), scale).float().reshape(q.shape))
        try:
            return super().__call__(*args, **kw)
        finally:
            om.sdpa = plain


TS = [1000.0, 500.0]


def engine(cfg, B=2, hw=(16, 24), t=45):
    """S = 45 + 96 = 141: two query blocks, a ragged second key tile"""
    from tests.test_gpu_model import build
    eng, wf = build(cfg, DEV)
    text, pooled, lat = randn(B, t, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, *hw, 16, seed=5)
    eng.prepare(B, hw, t, len(TS))
    eng.cache_modulation_params(pooled.to(DEV), TS)
    return eng, wf, eng.patchify(lat.to(DEV)), text, pooled, lat, int(eng.lib.dk_mmdit_workspace_bytes(eng._h, B, *hw, t, len(TS)))


def test_engine_against_emulating_oracle_and_plain_engine_unchanged():
    from tests.test_gpu_model import psnr_ok, yardstick_ok
    flux = C.tiny_flux(2, 2)
    before = engine(flux)
    plain = before[0].forward_tokens(before[2], before[3].to(DEV, BF), 1).clone()
    eng, wf, tok, text, pooled, lat, n_on = engine(replace(flux, attention_dtype="fp8_e4m3"))
    out = eng.forward_tokens(tok, text.to(DEV, BF), 1).float().cpu()
    res = {"fp32": {}, "emu": {}}
    for name, P in (("fp32", Prec()), ("emu", Prec(BF))):
        m = Fp8AttentionOracle(flux, wf, P)
        m.cache_modulation_params(pooled, torch.tensor(TS))
        m(lat, text, TS[1], taps=res[name])
    yardstick_ok(out, res["emu"]["final"], res["fp32"]["final"], "fp8 attention"), psnr_ok(out, res["emu"]["final"], res["fp32"]["final"], "fp8 attention")
    after = engine(flux)  # a plain engine built afterwards: the bits and the workspace of the one built before; the option adds exactly the K8 / V8T region
    assert not torch.equal(out, plain.float().cpu()) and torch.equal(after[0].forward_tokens(after[2], after[3].to(DEV, BF), 1), plain) and after[6] == before[6]
    assert n_on - before[6] == ops.attention_fp8_workspace_bytes(2, flux.num_heads, 141)
    with pytest.raises(DkHipError, match="only before the first dk_mmdit_prepare"):
        eng.set_attention_fp8(False)
    with pytest.raises(DkHipError, match="dk_mmdit_run_blocks cannot run while fp8 attention is set"):
        eng.run_blocks(torch.zeros(2, 141, flux.hidden_size, dtype=BF, device=DEV), 1, 0)
    eng.set_attention_groups(np.ones(141, dtype=np.uint32))  # (a setter that came later: the rule is asked again in front of the forward)
    with pytest.raises(DkHipError, match="fp8 attention cannot run with attention groups"):
        eng.forward_tokens(tok, text.to(DEV, BF), 1)


@pytest.mark.parametrize("hw", [(32, 32), (24, 32)], ids=["quantiser_pass", "split_row_quantiser_pass"])
def test_fp8_weight_engine(hw):
    """kernel 12 writes the bf16 buffer, the quantiser pass the MX-fp8 copy (192 image tokens: as two row ranges); test_mmdit_fp8_tiny's gates"""
    from oracle import fp8 as o8
    cfg = replace(C.fp8_config(C.tiny_flux(2, 2), "speed"), attention_dtype="fp8_e4m3")
    eng, _, tok, text, pooled, lat, _ = engine(cfg, 2, hw, 128)
    out = eng.forward_tokens(tok, text.to(DEV, BF), 1).float().cpu()
    fq, res = o8.fake_quant_block_weights(cfg, synth_mmdit_weights(cfg, seed=1234)), {}
    for name, P in (("fq_emu", Prec(BF)), ("fq_fp32", Prec())):
        m = Fp8AttentionOracle(cfg, fq, P, act_quant=o8.policy_act_quant(cfg))
        m.cache_modulation_params(pooled, torch.tensor(TS))
        m(lat, text, TS[1], taps=res.setdefault(name, {}))
    e_h, e_e = rel_l2(res["fq_fp32"]["final"], out), rel_l2(res["fq_fp32"]["final"], res["fq_emu"]["final"])
    print(f"[attention_fp8] fp8 weights {hw}: kernel {e_h:.3e}, emulating oracle {e_e:.3e}, PSNR {psnr(res['fq_fp32']['final'], out):.1f} dB")
    assert bool(torch.isfinite(out).all()) and e_h <= 2.0 * e_e + 2e-3 and psnr(res["fq_fp32"]["final"], out) > 35.0


@pytest.mark.parametrize("name,rule", [("sd3_geometry", "FLUX geometry"), ("ip_adapter", "IP-Adapter")])
def test_engine_refuses(name, rule):
    # (fp16 activations, perturbed attention and skip layers exist without single blocks alone, where the geometry rule comes first)
    from tests.test_gpu_ip_adapter import build as build_with_adapter
    from tests.test_gpu_model import build
    eng = build_with_adapter(C.tiny_flux(2, 2), DEV) if name == "ip_adapter" else build(C.tiny_sd3(), DEV)[0]
    with pytest.raises(DkHipError, match=rule):
        eng.set_attention_fp8(True)


def test_pipeline_runs_and_is_deterministic():
    from diffusionkit_amd.pipeline import FluxPipeline
    imgs = []
    for dtype in ("fp8_e4m3", "fp8_e4m3", "bfloat16"):
        pipe = FluxPipeline(w16=True, a16=True, mmdit_config=replace(C.tiny_flux(), attention_dtype=dtype), vae_config=C.tiny_vae(), device=DEV, text_len=16)
        imgs.append(np.asarray(pipe.generate_image("a fox", num_steps=2, latent_size=(32, 32), seed=0, verbose=False)[0]))
    assert imgs[0].shape[:2] == (256, 256) and np.array_equal(imgs[0], imgs[1]) and not np.array_equal(imgs[0], imgs[2])
