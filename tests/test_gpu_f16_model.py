"""Model- and pipeline-level parity of the float16 activation mode of the SD3 family (MI355X).

Gates are derived, not tuned.  Both errors are relative L2 against the function the reference computes with fp32 activations,
``OracleMMDiT(cfg, w, Prec(), embed_prec=Prec(embed_dtype(cfg)))``; emu16 = ``OracleMMDiT(cfg, w, Prec(torch.float16))`` restates the reference's
fp16 rounding points:
    err(hip) <= 2 * err(emu16) + 2.5e-4      (the project's model-level gate with its floor 2e-3 / 8: fp16 has three more mantissa bits than bf16)
    err(hip) <= 0.5 * err(emu-bf16)          (the reference alone holds it with room: emu16 / emu-bf16 = 0.12 - 0.13 on all five forward cases --
                                              tiny 6.6e-4 vs 5.4e-3 and 7.7e-4 vs 5.9e-3, SD3-medium at width 9.8e-4 vs 8.1e-3, SD3.5-large at
                                              width 1.2e-3 vs 1.0e-2; a bf16 rounding anywhere on the fp16 path fails it)
The full-depth gates read what the fp16-emulating oracle reached from the committed fixtures: measured - 2 dB of PSNR, x 1.5 in relative L2
(catches one rounding point per stored tensor)."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from diffusionkit_amd.config import SD3_2b, SD3_8b, float16_config, tiny_sd3, tiny_vae
from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec, embed_dtype
from tests._util import BF, psnr, randn, rel_l2

pytestmark = pytest.mark.gpu

F16 = torch.float16
FLOOR_F16 = 2e-3 / 8


def f16_weights(cfg, seed=1234):
    """(source tensors, the fp32 view of what an fp16 engine holds): both sides of every comparison see the same values"""
    named = synth_mmdit_weights(cfg, seed=seed)
    return named, {k: v.to(F16).float() for k, v in named.items()}


def gate(hip, emu16, emubf, exact, what):
    e_h, e_16, e_bf = rel_l2(exact, hip), rel_l2(exact, emu16), rel_l2(exact, emubf)
    print(f"[f16] {what}: hip {e_h:.3e}, fp16-emulating oracle {e_16:.3e}, bf16-emulating oracle {e_bf:.3e} (PSNR hip {psnr(exact, hip):.2f} dB)")
    assert e_h <= 2.0 * e_16 + FLOOR_F16, f"{what}: hip-vs-fp32 {e_h:.3e} > 2 * emu16-vs-fp32 {e_16:.3e} + {FLOOR_F16}"
    assert e_h <= 0.5 * e_bf, f"{what}: hip-vs-fp32 {e_h:.3e} > 0.5 * bf16-emulation-vs-fp32 {e_bf:.3e}"
    return e_h


def oracles(cfg, wf):
    return {"fp32": OracleMMDiT(cfg, wf, Prec(), embed_prec=Prec(embed_dtype(cfg))), "emu16": OracleMMDiT(cfg, wf, Prec(F16)),
            "emubf": OracleMMDiT(cfg, wf, Prec(BF))}


def forward_case_f16(cfg, dev, B, Hl, Wl, S_t, timesteps, step, what):
    """tests/test_gpu_model.py's forward_case (same seeds) on an fp16 engine"""
    from diffusionkit_amd.engine import MMDiTEngine
    c16 = float16_config(cfg)
    named, wf = f16_weights(cfg)
    eng = MMDiTEngine(c16, pack_mmdit(c16, named, dev))
    text = randn(B, S_t, cfg.token_level_text_embed_dim, seed=3)
    pooled = randn(B, cfg.pooled_text_embed_dim, seed=4)
    lat = randn(B, Hl, Wl, 16, seed=5)
    eng.prepare(B, (Hl, Wl), S_t, len(timesteps))
    eng.cache_modulation_params(pooled.to(dev), timesteps)
    tok = eng.patchify(lat.to(dev))
    out = eng.forward_tokens(tok, text.to(dev, F16), step)
    assert tok.dtype == F16 and out.dtype == F16
    res = {}
    for name, m in oracles(cfg, wf).items():
        m.cache_modulation_params(pooled, torch.tensor(timesteps))
        taps = {}
        m(lat, text, timesteps[step], taps=taps)
        res[name] = taps["final"]
    gate(out.float(), res["emu16"], res["emubf"], res["fp32"], what)
    return eng


@pytest.mark.parametrize("name,cfg,B,Hl,Wl,S_t", [("sd3", tiny_sd3(), 2, 8, 12, 20), ("sd3_24x20", tiny_sd3(), 2, 24, 20, 77),
                                                   ("sd35", replace(tiny_sd3(depth=3, heads=6), use_qk_norm=True), 2, 8, 12, 20)])
def test_mmdit_forward_tiny_f16(dev, name, cfg, B, Hl, Wl, S_t):
    forward_case_f16(cfg, dev, B, Hl, Wl, S_t, [1000.0, 752.0, 500.0], 1, name)


def test_sd3_width_cfg_batch_f16(dev):
    """SD3-medium at width as tests/test_gpu_model.py::test_sd3_width_cfg_batch: h 1536, depth 2, B 2, latent 64 x 64, S_t 154"""
    cfg = replace(SD3_2b, depth_multimodal=2, hidden_size_override=1536)
    forward_case_f16(cfg, dev, 2, 64, 64, 154, [1000.0, 857.5], 1, "sd3 width")


def test_sd35_large_width_cfg_batch_f16(dev):
    """SD3.5-large at width: h 2432 (the half column tile of gemm256v3.hip), QK-norm (the fused key tail + the Q-load norm)"""
    cfg = replace(SD3_8b, depth_multimodal=2, hidden_size_override=38 * 64)
    forward_case_f16(cfg, dev, 2, 64, 64, 154, [1000.0, 857.5], 1, "sd3.5-large width")


def test_bfloat16_field_changes_nothing(dev):
    """activation_dtype="bfloat16" spelled out is the default configuration: the same engine, the same bits (the committed bf16 goldens of
    tests/test_gpu_model.py pin those bits to the earlier builds'); an fp16 engine refuses bf16 tokens and bf16 weights"""
    from diffusionkit_amd import _lib
    from diffusionkit_amd.engine import MMDiTEngine
    cfg = tiny_sd3()
    named = synth_mmdit_weights(cfg, seed=1234)
    B, Hl, Wl, S_t, ts = 2, 8, 12, 20, [1000.0, 752.0]
    text, pooled, lat = randn(B, S_t, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, Hl, Wl, 16, seed=5)
    outs = []
    for c, explicit in ((cfg, False), (replace(cfg, activation_dtype="bfloat16"), True)):
        assert c == cfg
        eng = MMDiTEngine(c, pack_mmdit(c, named, dev))
        eng.prepare(B, (Hl, Wl), S_t, len(ts))
        eng.cache_modulation_params(pooled.to(dev), ts)
        outs.append(eng.forward_tokens(eng.patchify(lat.to(dev)), text.to(dev, BF), 1))
    assert outs[0].dtype == BF and torch.equal(outs[0], outs[1])
    c16 = float16_config(cfg)
    eng = MMDiTEngine(c16, pack_mmdit(c16, named, dev))
    eng.prepare(B, (Hl, Wl), S_t, len(ts))
    eng.cache_modulation_params(pooled.to(dev), ts)
    with pytest.raises(_lib.DkHipError, match="float16"):
        eng.forward_tokens(eng.patchify(lat.to(dev)).to(BF), text.to(dev, BF), 1)
    with pytest.raises(_lib.DkHipError, match="float16"):
        MMDiTEngine(c16, pack_mmdit(cfg, named, dev))  # bf16 tensors for an fp16 engine


def denoise_oracles(cfg, wf, text, pooled, steps, cfgw, latent, seed, shift):
    out = {}
    for name, (m, act) in {"fp32": (OracleMMDiT(cfg, wf, Prec(), embed_prec=Prec(embed_dtype(cfg))), Prec(F16)),
                           "emu16": (OracleMMDiT(cfg, wf, Prec(F16)), Prec(F16)), "emubf": (OracleMMDiT(cfg, wf, Prec(BF)), Prec(BF))}.items():
        # ``act``: the dtype the latent is rounded to on its way into the model (what the denoiser saw); timesteps: fp16 (quirk Q1)
        out[name] = op.denoise_latents(m, text, pooled, steps, cfgw, latent, seed, shift, False, act, t_act=Prec(F16))
    return out


def test_denoise_latents_tiny_f16(dev):
    """the whole step loop (sample_euler + CFGDenoiser + schedule + latent format) in fp16: CFG 5, shift 3, 3 steps, seed 0"""
    from diffusionkit_amd.pipeline import DiffusionPipeline
    cfg = tiny_sd3()
    pipe = DiffusionPipeline(w16=True, a16=True, shift=3.0, model_version="argmaxinc/mlx-stable-diffusion-3-medium", mmdit_config=cfg,
                             vae_config=tiny_vae(), device=dev, text_len=16, activation_dtype="float16")
    assert pipe.activation_dtype == pipe.dtype == pipe.float16_dtype == F16 and pipe.mmdit.dtype == F16
    assert pipe.mmdit_config == float16_config(cfg)
    text, pooled = randn(2, 16, cfg.token_level_text_embed_dim, seed=7), randn(2, cfg.pooled_text_embed_dim, seed=8)
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=3, cfg_weight=5.0, latent_size=(8, 8), seed=0)
    assert len(iter_time) == 3 and lat.shape == (1, 8, 8, 16) and lat.dtype == torch.float32
    _, wf = f16_weights(cfg)
    res = denoise_oracles(cfg, wf, text, pooled, 3, 5.0, (8, 8), 0, 3.0)
    gate(lat, res["emu16"], res["emubf"], res["fp32"], "denoise_latents tiny")


def test_generate_image_f16(dev):
    """DiffusionPipeline(activation_dtype="float16"): generate_image returns an image, and the latent it decoded is within the gate"""
    from PIL import Image
    from diffusionkit_amd.pipeline import DiffusionPipeline
    cfg = tiny_sd3()
    pipe = DiffusionPipeline(w16=True, a16=True, shift=3.0, mmdit_config=cfg, vae_config=tiny_vae(), device=dev, text_len=16,
                             activation_dtype="float16")
    img, log = pipe.generate_image("a photo of a cat", num_steps=2, cfg_weight=5.0, latent_size=(8, 8), seed=3, verbose=False)
    assert isinstance(img, Image.Image) and img.size == (64, 64) and len(log["denoising"]["iter_time"]) == 2
    text, pooled = pipe.encode_text("a photo of a cat", 5.0, "")  # (bf16: the encoders' side stays bf16; the hand-over casts to fp16, exact in range)
    assert text.dtype == BF
    lat, _ = pipe.denoise_latents(text, pooled, num_steps=2, cfg_weight=5.0, latent_size=(8, 8), seed=3)
    _, u8, _ = pipe.decoder.decode(lat)
    assert np.array_equal(np.asarray(img), u8.reshape(-1, u8.shape[2], 3).cpu().numpy())  # the latent generate_image decoded
    _, wf = f16_weights(cfg)
    res = denoise_oracles(cfg, wf, text.float().cpu(), pooled.float().cpu(), 2, 5.0, (8, 8), 3, 3.0)
    gate(lat, res["emu16"], res["emubf"], res["fp32"], "generate_image latent")


def test_cli_end_to_end_tiny_f16(dev, tmp_path):
    from diffusionkit_amd import cli
    over = dict(mmdit_config=tiny_sd3(), vae_config=tiny_vae(), text_len=20)
    argv = ["--prompt", "a cat", "--model-version", "argmaxinc/mlx-stable-diffusion-3-medium", "--steps", "2", "--seed", "1", "--height", "64",
            "--width", "64", "--negative_prompt", "blurry"]
    out = tmp_path / "f16.png"
    img, log = cli.main(argv + ["-o", str(out), "--activation-dtype", "float16"], pipeline_overrides=over)
    assert out.exists() and img.size == (64, 64) and len(log["denoising"]["iter_time"]) == 2


# ---- full depth (SD3-medium, 24 blocks): one seeded weight set, packed once as fp16 ---------------------------------------------
@pytest.fixture(scope="module")
def sd3_medium_f16(dev):
    from tests import test_gpu_fullsize as fs
    c = fs.fx.SD3_512
    assert fs.fx.SD3_FULL_LATE["cfg"] == c["cfg"] and fs.fx.SD3_FULL_LATE["seed_w"] == c["seed_w"]
    cfg = float16_config(c["cfg"])
    return {"mmdit": pack_mmdit(cfg, synth_mmdit_weights(c["cfg"], seed=c["seed_w"]), dev, consume=True)}


def test_sd3_medium_512_full_depth_closed_loop_f16(dev, sd3_medium_f16):
    """fullsize_sd3_512.npz: 24 blocks, 512 x 512, 4 Euler steps, closed loop -- the final latent against the fp32 oracle's, gated at what the
    fp16-emulating oracle reached - 2 dB / x 1.5 (52.46 dB: the bf16 path's 51.86 dB fails it)"""
    from diffusionkit_amd.pipeline import DiffusionPipeline
    from tests import test_gpu_fullsize as fs
    f, c = fs.load("sd3_512"), fs.fx.SD3_512
    pipe = DiffusionPipeline(w16=True, a16=True, shift=c["shift"], device=dev, text_len=c["S_t"], packed_weights=sd3_medium_f16,
                             vae_config=tiny_vae(), activation_dtype="float16")
    text, pooled = fs.fx.sd3_512_inputs()
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=c["steps"], cfg_weight=0.0, latent_size=c["latent"],
                                          seed=c["noise_seed"])
    ref = torch.from_numpy(f["latent_fp32"])
    p, e = psnr(ref, lat.cpu()), rel_l2(ref, lat.cpu())
    min_p, max_e = float(f["emu_fp16_psnr"]) - 2.0, 1.5 * float(f["emu_fp16_rel_l2"])
    print(f"[f16 fullsize] sd3_512 latent: PSNR {p:.2f} dB, rel-L2 {e:.4e}  (fp16-emulating oracle {float(f['emu_fp16_psnr']):.2f} dB / "
          f"{float(f['emu_fp16_rel_l2']):.3e}; bf16-emulating {float(f['emu_psnr']):.2f} dB; gate {min_p:.2f} dB / {max_e:.3e})")
    assert len(iter_time) == c["steps"] and p >= min_p and e <= max_e


def test_sd3_medium_1024_full_depth_cfg_late_steps_f16(dev, sd3_medium_f16):
    """fullsize_sd3_full_late.npz: 1024 x 1024, B 2, CFG 5, steps 1 / 25 / 49 / 50 of 50, teacher-forced -- every step's Euler direction against the
    fp32 oracle's, gated per step at the fixture's fp16-emulation figures - 2 dB / x 1.5"""
    from diffusionkit_amd.pipeline import DiffusionPipeline
    from tests import test_gpu_fullsize as fs
    f, c = fs.load("sd3_full_late"), fs.fx.SD3_FULL_LATE
    pipe = DiffusionPipeline(w16=True, a16=True, shift=c["shift"], device=dev, text_len=c["S_t"], packed_weights=sd3_medium_f16,
                             vae_config=tiny_vae(), activation_dtype="float16")
    got = fs.forced_steps(pipe, c, dev)
    bad = []
    for i in sorted(got):
        ref = torch.from_numpy(f[f"d{i}_fp32_f16"].astype(np.float32))
        p, e = psnr(ref, got[i].float()), rel_l2(ref, got[i].float())
        min_p, max_e = float(f[f"d{i}_emu_fp16_psnr"]) - 2.0, 1.5 * float(f[f"d{i}_emu_fp16_rel_l2"])
        print(f"[f16 fullsize] sd3_full_late step {i + 1} of 50: Euler direction PSNR {p:.2f} dB, rel-L2 {e:.4e}  (fp16-emulating oracle "
              f"{float(f[f'd{i}_emu_fp16_psnr']):.2f} dB / {float(f[f'd{i}_emu_fp16_rel_l2']):.3e}; bf16-emulating "
              f"{float(f[f'd{i}_emu_psnr']):.2f} dB; gate {min_p:.2f} dB / {max_e:.3e})")
        if p < min_p or e > max_e:
            bad.append((i, p, e))
    assert sorted(got) == [0, 24, 48, 49] and not bad, bad
