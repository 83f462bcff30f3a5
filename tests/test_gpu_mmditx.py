"""MMDiT-X (Stable Diffusion 3.5 medium) on the MI355X: the LayerNorm pass with two modulated outputs bit for bit against the single one,
and the dual-attention block form -- forward, single blocks, both QKNorm placements, the production width, float16, the step loop and the
pipeline from a Stability-layout checkpoint -- against ``tests/_mmditx.MMDiTXOracle``.

The gates are the project's own (tests/test_gpu_model.py: err(hip, fp32) <= 2 err(emu, fp32) + 2e-3 and PSNR > 35 dB; tests/test_gpu_f16_model.py's
``gate`` in float16); nothing here sets a tolerance of its own.  Arithmetic parity on synthetic weights: no SD3.5-medium checkpoint has been run."""
from dataclasses import replace

import pytest
import torch

from diffusionkit_amd.config import SD3_5_MEDIUM, float16_config, tiny_sd35m, tiny_vae
from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
from oracle import pipeline as op
from oracle.mmdit import Prec, embed_dtype
from tests._mmditx import MMDiTXOracle, to_stability_sd3
from tests._util import BF, bf16r, psnr, randn, rel_l2
from tests.test_gpu_f16_model import gate as gate_f16
from tests.test_gpu_model import psnr_ok, yardstick_ok

pytestmark = pytest.mark.gpu

F16 = torch.float16
VERSION = "stabilityai/stable-diffusion-3.5-medium"
TS = [1000.0, 752.0, 500.0]


# ---- the dual LayerNorm kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("with_text", [True, False], ids=["text", "alone"])
@pytest.mark.parametrize("M", [5, 70])
@pytest.mark.parametrize("h", [256, 320, 640, 1536])
def test_ln_modulate_dual_is_two_single_passes_bit_for_bit(dev, h, M, with_text, dtype):
    """h 256 / 320: lanes past the row end in the only pass; 640: a half-live second pass; 1536: three full passes (the production width).
    M 5 / 70: a last workgroup with one / two of its four rows; 70: two batch rows of 35 with their own modulation."""
    from diffusionkit_amd import ops
    B = 2 if M % 2 == 0 else 1
    S, S1 = M // B, 3
    g = torch.Generator().manual_seed(h + M)
    x = (torch.randn(B, S, h, generator=g) * 2 + 0.5).to(dev, dtype)
    x1 = torch.randn(B, S1, h, generator=g).to(dev, dtype)
    tab = (torch.randn(B, 6 * h, generator=g) * 0.5).to(dev, dtype)
    sa, ca, sb, cb, s1, c1 = (tab[:, i * h:(i + 1) * h] for i in range(6))
    got = ops.ln_modulate_dual(x, sa, ca, sb, cb, text=(x1, s1, c1) if with_text else None)
    assert len(got) == (3 if with_text else 2)
    ref_a, ref_b = ops.ln_modulate(x, sa, ca), ops.ln_modulate(x, sb, cb)
    assert torch.equal(got[0], ref_a) and torch.equal(got[1], ref_b)
    assert not torch.equal(ref_a, ref_b) and bool(torch.isfinite(ref_b.float()).all())
    if with_text:
        assert torch.equal(got[2], ops.ln_modulate(x1, s1, c1))


# ---- the block form -------------------------------------------------------------------------------------------------------------------
def build(cfg, dev, seed=1234):
    from diffusionkit_amd.engine import MMDiTEngine
    named = synth_mmdit_weights(cfg, seed=seed)
    return MMDiTEngine(cfg, pack_mmdit(cfg, named, dev)), named


def inputs(cfg, B, Hl, Wl, S_t):
    return randn(B, S_t, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, Hl, Wl, 16, seed=5)


_oracle_cache = {}


def oracle_taps(cfg, B, Hl, Wl, S_t, step=1):
    """fp32 and bf16-emulating MMDiTXOracle on the seeded case, computed once per case and left unchanged"""
    key = (cfg, B, Hl, Wl, S_t, step)
    if key not in _oracle_cache:
        wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
        text, pooled, lat = inputs(cfg, B, Hl, Wl, S_t)
        res = {}
        for name, P in (("fp32", Prec()), ("emu", Prec(BF))):
            m = MMDiTXOracle(cfg, wf, P)
            m.cache_modulation_params(pooled, torch.tensor(TS))
            taps = {}
            m(lat, text, TS[step], taps=taps)
            res[name] = (m, taps)
        _oracle_cache[key] = res
    return _oracle_cache[key]


def engine_forward(cfg, dev, B, Hl, Wl, S_t, step=1):
    eng, _ = build(cfg, dev)
    text, pooled, lat = inputs(cfg, B, Hl, Wl, S_t)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(pooled.to(dev), TS)
    return eng, eng.forward_tokens(eng.patchify(lat.to(dev)), text.to(dev, BF), step)


TINY = {"b2": (tiny_sd35m(depth=3, heads=4, dual=2), 2, 8, 12, 20), "heads6_35tok": (tiny_sd35m(depth=3, heads=6, dual=2), 1, 10, 14, 20)}


@pytest.mark.parametrize("name", list(TINY))
def test_mmditx_forward_tiny(dev, name):
    """two dual blocks, a plain block and the text-skipping last block behind them; heads 6: h = 384, no whole 256-column QKNorm tiles; 35 image
    tokens: an odd count on every attention and GEMM tile"""
    cfg, B, Hl, Wl, S_t = TINY[name]
    _, out = engine_forward(cfg, dev, B, Hl, Wl, S_t)
    res = oracle_taps(cfg, B, Hl, Wl, S_t)
    e_h, e_e = yardstick_ok(out.float(), res["emu"][1]["final"], res["fp32"][1]["final"], name)
    p = psnr(res["fp32"][1]["final"], out.float())
    print(f"[mmditx] forward {name}: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR {p:.1f} dB")
    assert p > 35.0


@pytest.mark.parametrize("block", [0, 2], ids=["dual", "plain_last"])
def test_mmditx_single_block_teacher_forced(dev, block):
    """run_blocks on one block from the fp32 oracle's tapped input (rounded to bf16: what all three sides read), against that block of the
    oracle: a failure names the block form"""
    cfg, B, Hl, Wl, S_t = TINY["b2"]
    res = oracle_taps(cfg, B, Hl, Wl, S_t)
    taps = res["fp32"][1]
    prev = "embed" if block == 0 else f"double{block - 1}"
    img, txt = bf16r(taps[prev + "_img"]), bf16r(taps[prev + "_txt"])
    eng, _ = build(cfg, dev)
    _, pooled, _ = inputs(cfg, B, Hl, Wl, S_t)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(pooled.to(dev), TS)
    y = eng.run_blocks(torch.cat([txt, img], dim=1).to(dev, BF).contiguous(), 1, block).float().cpu()
    outs = {n: res[n][0]._double_block(block, img, txt, TS[1], None) for n in ("fp32", "emu")}
    e_h, e_e = yardstick_ok(y[:, S_t:], outs["emu"][0], outs["fp32"][0], f"block {block} image rows")
    print(f"[mmditx] block {block} image rows: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e})")
    if outs["fp32"][1] is None:
        assert block == cfg.depth_multimodal - 1 and torch.equal(y[:, :S_t], txt)  # the last text stream stops after attention: rows untouched
    else:
        yardstick_ok(y[:, :S_t], outs["emu"][1], outs["fp32"][1], f"block {block} text rows")


def test_mmditx_block_cache_head_and_compute_tail_are_the_forward(dev):
    """the first-block cache's head (embedders + block 0, a dual block) and compute tail go through the same block driver: the bits of
    dk_mmdit_forward, with the three dual buffers carved behind the cache's"""
    cfg, B, Hl, Wl, S_t = TINY["b2"]
    eng, _ = build(cfg, dev)
    text, pooled, lat = inputs(cfg, B, Hl, Wl, S_t)
    text = text.to(dev, BF)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(pooled.to(dev), TS)
    tok = eng.patchify(lat.to(dev))
    ref = eng.forward_tokens(tok, text, 1).clone()
    eng.enable_block_cache(True)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(pooled.to(dev), TS)
    probe = eng.forward_head(tok, text, 1)
    out = eng.forward_tail(1, False)
    assert torch.equal(out, ref) and bool(torch.isfinite(probe).all()) and float(probe[:, 0].min()) > 0.0


def width_cfg():
    """SD3.5-medium at WIDTH (h 1536, 24 heads of 64, QK-norm), depth 2 with one dual block; a small positional table keeps the weights quick to draw"""
    return replace(SD3_5_MEDIUM, depth_multimodal=2, hidden_size_override=1536, dual_attention_blocks=1, max_latent_resolution=32)


def test_mmditx_production_width_cfg_batch(dev):
    """modelled on test_sd3_width_cfg_batch: CFG batch 2 (two pooled vectors: two modulation rows per module), latent 16 x 16, S_t 20"""
    cfg = width_cfg()
    assert cfg.hidden_size == 1536 and cfg.num_heads == 24 and cfg.head_dim == 64
    _, out = engine_forward(cfg, dev, 2, 16, 16, 20)
    res = oracle_taps(cfg, 2, 16, 16, 20)
    e_h, e_e = yardstick_ok(out.float(), res["emu"][1]["final"], res["fp32"][1]["final"], "sd3.5-medium width")
    p_h, p_e = psnr_ok(out.float(), res["emu"][1]["final"], res["fp32"][1]["final"], "sd3.5-medium width")
    print(f"[mmditx] width: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR {p_h:.1f} dB (emulation {p_e:.1f})")


@pytest.mark.parametrize("name", ["tiny", "width"])
def test_attn2_fused_norm_matches_separate_pass(dev, name):
    """attn2's key / query QKNorm in the projection's tail or the Q load against the stand-alone pass, switched as
    test_fused_key_norm_matches_separate_pass switches the main attention's, with that test's bounds.  width: 1024 image tokens x N = 4608, the
    256-column kernel whose tail holds the fused form (below 1024 rows the route takes the 128^2 kernel and the stand-alone pass under every
    setting: the tiny case then only shows that the switches are harmless there)"""
    from diffusionkit_amd import ops
    cfg, B, Hl, Wl, S_t = (width_cfg(), 1, 64, 64, 20) if name == "width" else TINY["b2"]
    eng, _ = build(cfg, dev)
    text, pooled, lat = inputs(cfg, B, Hl, Wl, S_t)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(pooled.to(dev), TS)
    S = S_t + (Hl // 2) * (Wl // 2)
    x = randn(B, S, cfg.hidden_size, seed=840).to(dev, BF)
    outs = {}
    try:
        for fuse in ((1, 1), (1, 0), (0, 1)):
            ops.tune("gemm_fuse_k", fuse[0])
            ops.tune("gemm_fuse_q", fuse[1])
            outs[fuse] = eng.run_blocks(x, 1, 0).float().cpu()  # block 0: the dual block alone
    finally:
        ops.tune("gemm_fuse_k", 1)
        ops.tune("gemm_fuse_q", -1)
    ref = outs[(0, 1)]
    assert torch.isfinite(ref).all() and torch.isfinite(outs[(1, 1)]).all()
    for key in ((1, 1), (1, 0)):
        d = (outs[key] - ref).abs()
        print(f"[mmditx] fused norm {name} {key}: rel-L2 {rel_l2(ref, outs[key]):.3e}, max {float(d.max()):.3e} of {float(ref.abs().max()):.3e}")
        assert rel_l2(ref, outs[key]) < 8e-3, (key, float(rel_l2(ref, outs[key])))
        assert float(d.max()) <= 0.05 * float(ref.abs().max()), key
    if name == "width":  # (the switch does select another path: the sums of squares differ in their order)
        assert not torch.equal(outs[(1, 0)], ref) and not torch.equal(outs[(1, 1)], outs[(1, 0)])


def f16_oracles(cfg, wf):
    return {"fp32": MMDiTXOracle(cfg, wf, Prec(), embed_prec=Prec(embed_dtype(cfg))), "emu16": MMDiTXOracle(cfg, wf, Prec(F16)),
            "emubf": MMDiTXOracle(cfg, wf, Prec(BF))}


def test_mmditx_forward_tiny_f16(dev):
    """float16_config(tiny_sd35m()) under the float16 MMDiT tests' rule (tests/test_gpu_f16_model.py: forward_case_f16 with this oracle)"""
    from diffusionkit_amd.engine import MMDiTEngine
    cfg, B, Hl, Wl, S_t = TINY["b2"]
    c16 = float16_config(cfg)
    named = synth_mmdit_weights(cfg, seed=1234)
    wf = {k: v.to(F16).float() for k, v in named.items()}
    eng = MMDiTEngine(c16, pack_mmdit(c16, named, dev))
    text, pooled, lat = inputs(cfg, B, Hl, Wl, S_t)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(pooled.to(dev), TS)
    out = eng.forward_tokens(eng.patchify(lat.to(dev)), text.to(dev, F16), 1)
    assert out.dtype == F16
    res = {}
    for n, m in f16_oracles(cfg, wf).items():
        m.cache_modulation_params(pooled, torch.tensor(TS))
        taps = {}
        m(lat, text, TS[1], taps=taps)
        res[n] = taps["final"]
    gate_f16(out.float(), res["emu16"], res["emubf"], res["fp32"], "mmditx tiny f16")


# ---- step loop and pipeline -----------------------------------------------------------------------------------------------------------
def test_mmditx_denoise_latents_tiny(dev):
    """the whole step loop as test_denoise_latents_tiny runs it for SD3: 3 steps, CFG 5, shift 3, seed 0"""
    from diffusionkit_amd.pipeline import DiffusionPipeline
    cfg = tiny_sd35m()
    pipe = DiffusionPipeline(w16=True, a16=True, shift=3.0, model_version=VERSION, mmdit_config=cfg, vae_config=tiny_vae(), device=dev, text_len=16)
    text, pooled = randn(2, 16, cfg.token_level_text_embed_dim, seed=7), randn(2, cfg.pooled_text_embed_dim, seed=8)
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=3, cfg_weight=5.0, latent_size=(8, 8), seed=0)
    assert len(iter_time) == 3 and lat.shape == (1, 8, 8, 16) and lat.dtype == torch.float32
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    res = {n: op.denoise_latents(MMDiTXOracle(cfg, wf, P), text, pooled, 3, 5.0, (8, 8), 0, 3.0, False, Prec(BF), t_act=Prec(F16))
           for n, P in (("fp32", Prec()), ("emu", Prec(BF)))}
    e_h, e_e = yardstick_ok(lat, res["emu"], res["fp32"], "sd3.5-medium tiny")
    p = psnr(res["fp32"], lat)
    print(f"[mmditx] denoise_latents: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR {p:.1f} dB")
    assert p > 35.0


def test_mmditx_pipeline_from_stability_checkpoint_file(dev, tmp_path):
    """model_version + local_ckpt: a safetensors file in the Stability key layout (attn2 tensors, 9h adaLN rows) generates an image, and gives
    the latent the same weights give when handed over as a reference-named dict"""
    import os
    from PIL import Image
    from safetensors.torch import save_file
    from diffusionkit_amd.pipeline import DiffusionPipeline
    cfg, vcfg = tiny_sd35m(), tiny_vae()
    w = synth_mmdit_weights(cfg, seed=21)
    path = os.path.join(tmp_path, "sd3.5_medium.safetensors")
    save_file(to_stability_sd3(w, cfg), path)
    text, pooled = randn(2, 16, cfg.token_level_text_embed_dim, seed=7).to(dev, BF), randn(2, cfg.pooled_text_embed_dim, seed=8).to(dev, BF)
    lats = []
    for ck in ({"mmdit": w}, {"mmdit": path}):
        pipe = DiffusionPipeline(w16=True, a16=True, shift=3.0, model_version=VERSION, local_ckpt=ck, mmdit_config=cfg, vae_config=vcfg, device=dev,
                                 text_len=16)
        assert pipe.mmdit.config.dual_attention_blocks == 2 and pipe.mmdit.mod_rows() == cfg.num_modulation_rows()
        lat, _ = pipe.denoise_latents(text, pooled, num_steps=2, cfg_weight=5.0, latent_size=(8, 8), seed=4)
        lats.append(lat.clone())
    assert torch.equal(lats[0], lats[1]) and bool(torch.isfinite(lats[0]).all())
    img, log = pipe.generate_image("a photo of a cat", num_steps=2, cfg_weight=5.0, latent_size=(8, 8), seed=3, verbose=False)
    assert isinstance(img, Image.Image) and img.size == (64, 64) and len(log["denoising"]["iter_time"]) == 2
