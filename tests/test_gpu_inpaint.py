"""Inpainting on an MI355X: the three kernels (dk_mask_to_latent_f32, dk_euler_cfg_step_masked / _f16, dk_image_composite_u8) and the pipeline
on top of them (``mask_path=``, ``composite=``, ``--mask-path``), against exact expectations where the arithmetic has them and against the masked
reference loop of tests/test_inpaint_cpu.py (the fp32 oracle with the blend behind every step) under the project's model-level gates elsewhere.

Exact expectations: a mask of ones is dk_euler_cfg_step bit for bit; a mask of zeros with sigma_next = 0 returns x_orig bit for bit, so the cells
a pipeline run keeps are the encoded image; kept pixels of a composited image are the input's bytes.  Every figure is printed before it is asserted.

The file name sorts behind tests/test_gpu_fullsize.py on purpose (see the head of tests/test_gpu_vae_f16.py)."""
import functools

import numpy as np
import pytest
import torch

from diffusionkit_amd.config import tiny_flux, tiny_sd3, tiny_vae, tiny_vae_encoder
from diffusionkit_amd.weights import synth_mmdit_weights, synth_vae_encoder_weights
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec, embed_dtype
from oracle.vae import OracleVAEEncoder
from tests import _footprint as fp
from tests._util import BF, max_abs, psnr, rel_l2
from tests.test_inpaint_cpu import (FAMILIES, STEP_SHAPE, family_inputs, half_mask, latent_mask, make_image, masked_denoise_latents,
                                    masked_sample_euler, masked_step_family, t_act_of)

pytestmark = pytest.mark.gpu

F16 = torch.float16
bits = fp.bits


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- 1. dk_mask_to_latent_f32 ---------------------------------------------------------------------------------------------------------------
def test_mask_to_latent(dev):
    """two 48 x 80 masks, f = 8: random bytes, an all-0 block, an all-255 block and a block with a single 255 pixel"""
    from diffusionkit_amd import ops
    mask = torch.randint(0, 256, (2, 48, 80), generator=gen(1), dtype=torch.int32).to(torch.uint8).numpy()
    mask[0, 8:16, 16:24] = 0
    mask[1, 40:48, 72:80] = 255  # the last block of the last mask
    mask[1, 0:8, 0:8] = 0
    mask[1, 3, 5] = 255
    got = ops.mask_to_latent(torch.from_numpy(mask).to(dev), 8)
    assert got.shape == (2, 6, 10) and got.dtype == torch.float32
    got = got.cpu().numpy()
    assert got[0, 1, 2] == np.float32(0.0) and got[1, 5, 9] == np.float32(1.0) and got[1, 0, 0] == np.float32(255) / np.float32(16320)
    want = mask.astype(np.int64).reshape(2, 6, 8, 10, 8).sum(axis=(2, 4)).astype(np.float32) / np.float32(16320)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    one = ops.mask_to_latent(torch.from_numpy(mask[1]).to(dev))  # [H, W]: one mask
    assert np.array_equal(one.cpu().numpy().view(np.uint32), want[1:2].view(np.uint32))
    from diffusionkit_amd._lib import DkHipError
    with pytest.raises(DkHipError, match="divisible"):
        ops.mask_to_latent(torch.zeros(1, 44, 80, dtype=torch.uint8, device=dev), 8)


# ---- 2. the masked step operator ---------------------------------------------------------------------------------------------------------------
def tokens_of(x, dt, n_img, dup, Hl, Wl, C, p, order):
    from diffusionkit_amd import _lib
    from diffusionkit_amd.engine import _stream
    tok = torch.full((n_img * dup, (Hl // p) * (Wl // p), p * p * C), 7.0, dtype=dt, device=x.device)
    fn = _lib.load().dk_latent_to_tokens_f16 if dt == F16 else _lib.load().dk_latent_to_tokens
    _lib.check(fn(x.data_ptr(), tok.data_ptr(), n_img, dup, Hl, Wl, C, p, order, _stream()), "dk_latent_to_tokens")
    return tok


STEP_CASES = [(order, cfgw, dt, 0) for order in (0, 1) for cfgw in (0.0, 5.0) for dt in (BF, F16)] + [(1, 5.0, BF, 8)]


@pytest.mark.parametrize("order,cfgw,dt,ld_pad", STEP_CASES,
                         ids=[f"order{o}-cfg{w:g}-{'bf16' if d == BF else 'f16'}-ld+{l}" for o, w, d, l in STEP_CASES])
def test_masked_step_operator(dev, order, cfgw, dt, ld_pad):
    """latent 6 x 10, two images (1920 elements: the last block of 256 threads is half empty), C 16, p 2.
    (a) m == 1: x and tokens are dk_euler_cfg_step's, bit for bit; (b) m == 0, sigma_next = 0: x is x_orig bit for bit;
    (c) random m, shared and per image: |x - ref| <= 4 * 2^-23 * max(|x_new|, |noise|, |x_orig|) against the float64 evaluation of the blend on the
    fp32 inputs (x_new = the unmasked operator's output) -- the sum of the at most eight half-ulp roundings of the expression, whatever is fused;
    (d) tokens == dk_latent_to_tokens(x after the step), both CFG copies"""
    from diffusionkit_amd import ops
    n_img, Hl, Wl, C, p = (STEP_SHAPE[k] for k in ("n_img", "Hl", "Wl", "C", "p"))
    S_i, F = (Hl // p) * (Wl // p), p * p * C
    cfg_on = cfgw > 0
    dup = 2 if cfg_on else 1
    x0 = torch.randn(n_img, Hl, Wl, C, generator=gen(1)).to(dev)
    out = torch.randn(n_img * dup, S_i, F + ld_pad, generator=gen(2)).to(dev, dt)
    x_orig = (torch.randn(n_img, Hl, Wl, C, generator=gen(3)) * 1.5 + 0.3).to(dev)
    noise = torch.randn(n_img, Hl, Wl, C, generator=gen(4)).to(dev)
    sigma, sn = float(np.float32(0.8)), float(np.float32(0.3))  # (1 - sigma_next is not exact in fp32)

    def unmasked(sigma_next):
        x, tok = x0.clone(), torch.full((n_img * dup, S_i, F), 7.0, dtype=dt, device=dev)
        ops.euler_cfg_step(x, out, tok, n_img, cfg_on, p, order, sigma, sigma_next, cfgw)
        return x, tok

    def masked(m, sigma_next):
        x, tok = x0.clone(), torch.full((n_img * dup, S_i, F), 7.0, dtype=dt, device=dev)
        ops.euler_cfg_step_masked(x, out, tok, n_img, cfg_on, p, order, sigma, sigma_next, cfgw, x_orig, noise, m.to(dev))
        assert same_bits(tok, tokens_of(x, dt, n_img, dup, Hl, Wl, C, p, order)), "(d) tokens are not the patchified blended latent"
        return x, tok

    x_new, tok_new = unmasked(sn)
    x, tok = masked(torch.ones(1, Hl, Wl), sn)
    assert same_bits(x, x_new) and same_bits(tok, tok_new), "(a) a mask of ones is not the unmasked step"
    x, tok = masked(torch.ones(n_img, Hl, Wl), sn)
    assert same_bits(x, x_new) and same_bits(tok, tok_new), "(a) a per-image mask of ones is not the unmasked step"
    x, _ = masked(torch.zeros(1, Hl, Wl), 0.0)
    assert same_bits(x, x_orig), "(b) a mask of zeros with sigma_next = 0 does not return x_orig"
    for per_image in (False, True):
        m = torch.rand(n_img if per_image else 1, Hl, Wl, generator=gen(5 + per_image))
        x, _ = masked(m, sn)
        xn, no, xo, mm = (t.double().cpu() for t in (x_new, noise, x_orig, m[..., None]))
        ref = mm * xn + (1.0 - mm) * (sn * no + (1.0 - sn) * xo)
        bound = 4.0 * 2.0 ** -23 * torch.maximum(torch.maximum(xn.abs(), no.abs()), xo.abs())
        err = (x.double().cpu() - ref).abs()
        print(f"[inpaint] masked step order={order} cfg={cfgw:g} {dt} per_image={per_image}: largest |x - ref| / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), f"(c) {int((err > bound).sum())} elements beyond 4 * 2^-23 * max(|x_new|, |noise|, |x_orig|)"
        assert not same_bits(x, x_new)


def test_masked_step_refuses_bad_arguments(dev):
    from diffusionkit_amd import ops
    from diffusionkit_amd._lib import DkHipError
    x = torch.zeros(1, 4, 4, 16, device=dev)
    out, tok = torch.zeros(1, 4, 64, dtype=BF, device=dev), torch.zeros(1, 4, 64, dtype=BF, device=dev)
    m = torch.ones(1, 4, 4, device=dev)
    with pytest.raises(DkHipError, match="sigma"):
        ops.euler_cfg_step_masked(x, out, tok, 1, False, 2, 1, 0.0, 0.0, 0.0, x.clone(), x.clone(), m)
    with pytest.raises(DkHipError, match="divisible"):
        ops.euler_cfg_step_masked(x, out, tok, 1, False, 3, 1, 0.5, 0.25, 0.0, x.clone(), x.clone(), m)
    with pytest.raises(DkHipError, match="float32"):
        ops.euler_cfg_step_masked(x, out, tok, 1, False, 2, 1, 0.5, 0.25, 0.0, x.clone(), x.clone(), m.to(BF))
    with pytest.raises(ValueError):
        ops.euler_cfg_step_masked(x, out, tok, 1, False, 2, 1, 0.5, 0.25, 0.0, x.clone(), x.clone(), torch.ones(3, 4, 4, device=dev))


# ---- 3. footprint -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flux", [True, False], ids=["flux", "sd3"])
@pytest.mark.parametrize("per_image", [False, True], ids=["shared", "per_image"])
def test_masked_step_footprints(dev, flux, per_image):
    """NaN in one element of noise or x_orig -> exactly that latent element and its token feature in both CFG copies; NaN in one mask cell -> exactly the
    16 channels of that cell (of every image that shares the mask); everything else, guard margins included, bit-identical to the clean run"""
    from diffusionkit_amd import ops
    from tests.test_gpu_op_footprints import run_family
    ops_cpu, ref, (sigma, sigma_next, w), cases = masked_step_family(flux, per_image, **STEP_SHAPE)
    n_img, p = STEP_SHAPE["n_img"], STEP_SHAPE["p"]
    tok, g1 = fp.guarded(torch.empty(ops_cpu["out"].shape, dtype=BF, device=dev), 8, fp.SENTINEL)

    def launch(v):
        ops.euler_cfg_step_masked(v["x"], v["out"], tok, n_img, True, p, int(flux), sigma, sigma_next, w, v["x_orig"], v["noise"], v["mask"])
        return dict(x=v["x"], tok=tok)
    f32 = torch.float32
    run_family(dev, BF, ops_cpu, ref, cases, launch, f"masked step flux={flux} per_image={per_image}", guards=[("tok", g1)],
               dtypes={"x": f32, "x_orig": f32, "noise": f32, "mask": f32})


# ---- 4. dk_image_composite_u8 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_image", [False, True], ids=["shared", "per_image"])
def test_image_composite(dev, per_image):
    """two 24 x 40 images, one original for both: the decoder's bytes where mask == 255, the original's where mask == 0, elsewhere the plain fp32
    evaluation of (uint8)(w * dec + (1 - w) * orig + 0.5f), w = mask / 255.0f"""
    from diffusionkit_amd import ops
    B, H, W = 2, 24, 40

    def u8(*shape, seed):
        return torch.randint(0, 256, shape, generator=gen(seed), dtype=torch.int32).to(torch.uint8).numpy()
    dec, orig, mask = u8(B, H, W, 3, seed=1), u8(H, W, 3, seed=2), u8(B if per_image else 1, H, W, seed=3)
    mask[:, :8] = 0
    mask[:, 8:16] = 255
    mask[-1, H - 1, W - 1] = 255
    got = ops.image_composite(torch.from_numpy(dec).to(dev), torch.from_numpy(orig).to(dev), torch.from_numpy(mask).to(dev)).cpu().numpy()
    mb = np.broadcast_to(mask, (B, H, W))
    ob = np.broadcast_to(orig, (B, H, W, 3))
    assert np.array_equal(got[mb == 255], dec[mb == 255]) and np.array_equal(got[mb == 0], ob[mb == 0])
    w = (mb.astype(np.float32) / np.float32(255))[..., None]
    want = (w * dec.astype(np.float32) + (np.float32(1) - w) * ob.astype(np.float32) + np.float32(0.5)).astype(np.uint8)
    assert want.dtype == np.uint8 and np.array_equal(got, want)
    # the [H, W] / [H, W, 3] forms and an original per image
    if not per_image:
        again = ops.image_composite(torch.from_numpy(dec).to(dev), torch.from_numpy(np.ascontiguousarray(ob)).to(dev), torch.from_numpy(mask[0]).to(dev))
        assert np.array_equal(again.cpu().numpy(), want)


# ---- 5. pipeline -----------------------------------------------------------------------------------------------------------------------------------
H_IMG, W_IMG, HL, WL, STEPS, SEED = 64, 128, 8, 16, 4, 2
RGB = make_image(H_IMG, W_IMG, seed=1)
HALF = half_mask(H_IMG, W_IMG)  # columns 64.. of the image = latent columns 8.. are repainted
_PIPES = {}


def pipe_for(name, dev, f16=False):
    """one pipeline per family (and element type) for the whole module"""
    from diffusionkit_amd.pipeline import DiffusionPipeline, FluxPipeline
    key = (name, f16)
    if key not in _PIPES:
        cfg, shift, _ = FAMILIES[name]
        kw = dict(w16=True, a16=True, shift=shift, mmdit_config=cfg, vae_config=tiny_vae(), vae_encoder_config=tiny_vae_encoder(), device=dev, text_len=16)
        if f16:
            kw["activation_dtype"] = "float16"
        _PIPES[key] = FluxPipeline(**kw) if cfg.is_flux else DiffusionPipeline(model_version="argmaxinc/mlx-stable-diffusion-3-medium", **kw)
    return _PIPES[key]


def run(pipe, name, dev, mask, denoise=1.0, seed=SEED):
    cfg, _, cfgw, text, pooled = family_inputs(name)
    n = len(seed) if isinstance(seed, list) else 1
    if n > 1 and cfgw == 0:
        text, pooled = text.repeat(n, 1, 1), pooled.repeat(n, 1)
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=STEPS, cfg_weight=cfgw, latent_size=(HL, WL), seed=seed,
                                          image_path=RGB, denoise=denoise, **({} if mask is None else {"mask_path": mask}))
    assert lat.shape == (n, HL, WL, 16) and lat.dtype == torch.float32 and len(iter_time) == STEPS - int(STEPS * (1 - denoise))
    return lat


def encoded(pipe, seed=SEED):
    """(x_orig, process_out(x_orig)): the pipeline's own encoded image"""
    x_orig = pipe.latent_format.process_in(pipe.encode_image_to_latents(RGB, seed=seed))
    return x_orig, pipe.latent_format.process_out(x_orig)


@functools.lru_cache(maxsize=None)
def references(name, denoise):
    """the masked reference loop on the fp32 and the bf16-emulating oracle, each from its own OracleVAEEncoder posterior sample (as
    test_img2img_pipeline_tiny): after process_out.  Computed once per (family, denoise)."""
    cfg, shift, cfgw, text, pooled = family_inputs(name)
    ecfg = tiny_vae_encoder()
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    ewf = {k: v.float() for k, v in synth_vae_encoder_weights(ecfg, seed=1234 + 2).items()}
    res = {}
    for pname, P in (("fp32", Prec()), ("emu", Prec(BF))):
        z0 = op.encode_image_to_latents(OracleVAEEncoder(ecfg, ewf, P), op.read_image_array(RGB), seed=SEED)
        lat, _ = masked_denoise_latents(OracleMMDiT(cfg, wf, P), text, pooled, STEPS, cfgw, SEED, shift, cfg.is_flux, Prec(BF), z0, latent_mask(HALF),
                                        denoise=denoise, t_act=t_act_of(cfg))
        res[pname] = op.process_out(lat, "flux" if cfg.is_flux else "sd3")
    return res


def region_psnr(exact, got, region):
    """tests/_util.psnr over the cells of ``region`` [h, w], peak taken from the whole reference latent"""
    e, g = exact.double().cpu()[0][region], got.double().cpu()[0][region]
    peak = float(exact.double().abs().max())
    return float(20 * np.log10((peak + 1e-5) / (float(torch.sqrt(torch.mean((e - g) ** 2))) + 1e-10)))


def half_mask_gates(lat, res, what):
    """the project's gates (tests/test_gpu_model.py): yardstick and 35 dB on the whole latent, psnr_ok's rule on the repainted cells alone"""
    from tests.test_gpu_model import yardstick_ok
    repaint = latent_mask(HALF) == 1.0
    e_h, e_e = rel_l2(res["fp32"], lat), rel_l2(res["fp32"], res["emu"])
    p_h, p_e = psnr(res["fp32"], lat), psnr(res["fp32"], res["emu"])
    r_h, r_e = region_psnr(res["fp32"], lat, repaint), region_psnr(res["fp32"], res["emu"], repaint)
    print(f"[inpaint] {what}: whole latent rel_l2 hip {e_h:.3e} / emu {e_e:.3e}, PSNR hip {p_h:.1f} dB / emu {p_e:.1f} dB; "
          f"repainted cells PSNR hip {r_h:.1f} dB / emu {r_e:.1f} dB")
    yardstick_ok(lat, res["emu"], res["fp32"], what)
    assert p_h > 35.0, f"{what}: PSNR {p_h:.1f} dB"
    assert r_h > min(35.0, r_e - 1.5), f"{what}: repainted cells PSNR hip {r_h:.1f} dB, bf16-emulating oracle {r_e:.1f} dB"


@pytest.mark.parametrize("name", list(FAMILIES))
def test_pipeline_full_and_empty_mask(dev, name):
    """all-255: the latents of the same call without a mask, bit for bit; all-0: the encoded image, bit for bit"""
    pipe = pipe_for(name, dev)
    plain = run(pipe, name, dev, None)
    assert same_bits(run(pipe, name, dev, np.full((H_IMG, W_IMG), 255, dtype=np.uint8)), plain)
    _, kept = encoded(pipe)
    got = run(pipe, name, dev, np.zeros((H_IMG, W_IMG), dtype=np.uint8))
    assert same_bits(got, kept)
    assert not same_bits(plain, kept)


@pytest.mark.parametrize("name,denoise", [("flux", 1.0), ("sd3_cfg", 1.0), ("flux", 0.5)])
def test_pipeline_half_mask(dev, name, denoise):
    """right-half mask, 4 steps (denoise 0.5: the last 2): the kept half is the encoded image bit for bit, the whole latent and the repainted cells
    are within the project's gates of the masked fp32 reference loop"""
    pipe = pipe_for(name, dev)
    lat = run(pipe, name, dev, HALF, denoise)
    _, kept = encoded(pipe)
    assert same_bits(lat[:, :, :WL // 2], kept[:, :, :WL // 2])
    assert not same_bits(lat[:, :, WL // 2:], kept[:, :, WL // 2:])
    half_mask_gates(lat, references(name, denoise), f"{name} denoise={denoise}")


def test_pipeline_seed_list(dev):
    """seed = [2, 3] with one shared mask: one posterior sample and one noise draw per seed; equal to the two single-seed runs bit for bit"""
    pipe = pipe_for("flux", dev)
    both = run(pipe, "flux", dev, HALF, seed=[2, 3])
    for i, s in enumerate((2, 3)):
        one = run(pipe, "flux", dev, HALF, seed=s)
        print(f"[inpaint] seed list: image {i} (seed {s}) against its single-seed run: max_abs {max_abs(both[i:i + 1], one):.3e}")
        _, kept = encoded(pipe, seed=s)
        assert same_bits(both[i:i + 1, :, :WL // 2], kept[:, :, :WL // 2])
    for i, s in enumerate((2, 3)):
        assert same_bits(both[i:i + 1], run(pipe, "flux", dev, HALF, seed=s)), f"image {i} of the seed list differs from the single-seed run"
    # a mask per image: the second image keeps everything
    per = run(pipe, "flux", dev, [HALF, np.zeros_like(HALF)], seed=[2, 3])
    assert same_bits(per[0:1], both[0:1]) and same_bits(per[1:2], encoded(pipe, seed=3)[1])


def test_pipeline_half_mask_f16(dev):
    """tiny_sd3 with activation_dtype = "float16", CFG 5: the kept half bit-exact, the whole latent under the gates of tests/test_gpu_f16_model.py's
    pipeline test.  Those gates measure the fp16 step loop (hip <= 2 * emu16 + 2e-3 / 8 and <= 0.5 * emu-bf16), and the VAE encoder of this pipeline is
    the bf16 one, whose error they have no room for: every oracle therefore starts from the pipeline's own x_orig, so that the encoder's error is in
    none of the three and the kept half is exact in all of them."""
    from tests.test_gpu_f16_model import f16_weights, gate
    name = "sd3_cfg"
    pipe = pipe_for(name, dev, f16=True)
    assert pipe.mmdit.dtype == F16
    lat = run(pipe, name, dev, HALF)
    x_orig, kept = encoded(pipe)
    assert same_bits(lat[:, :, :WL // 2], kept[:, :, :WL // 2])
    cfg, shift, cfgw, text, pooled = family_inputs(name)
    _, wf = f16_weights(cfg)
    sigmas = op.get_sigmas(shift, False, STEPS)
    res = {}
    for oname, (m, act) in {"fp32": (OracleMMDiT(cfg, wf, Prec(), embed_prec=Prec(embed_dtype(cfg))), Prec(F16)),
                            "emu16": (OracleMMDiT(cfg, wf, Prec(F16)), Prec(F16)), "emubf": (OracleMMDiT(cfg, wf, Prec(BF)), Prec(BF))}.items():
        x = masked_sample_euler(m, x_orig.cpu(), latent_mask(HALF), SEED, sigmas, text, pooled, cfgw, act, t_act=Prec(F16))
        res[oname] = op.process_out(x, "sd3")
    gate(lat, res["emu16"], res["emubf"], res["fp32"], "inpaint half mask f16")
    # ... and on the repainted cells alone, where all of the error is
    cut = lambda t: t[:, :, WL // 2:]  # noqa: E731
    gate(cut(lat), cut(res["emu16"]), cut(res["emubf"]), cut(res["fp32"]), "inpaint half mask f16, repainted cells")


def test_generate_image_with_mask(dev, tmp_path):
    """generate_image(mask_path=): kept pixels are the input image's bytes; without the paste-back they are not (the VAE round trip is lossy)"""
    from PIL import Image
    pipe = pipe_for("flux", dev)
    ipath, mpath = str(tmp_path / "init.png"), str(tmp_path / "mask.png")
    Image.fromarray(RGB).save(ipath)
    Image.fromarray(HALF).save(mpath)
    kw = dict(num_steps=STEPS, latent_size=(HL, WL), seed=SEED, image_path=ipath, denoise=1.0, verbose=False)
    img, log = pipe.generate_image("a cat", mask_path=mpath, **kw)
    arr = np.asarray(img)
    assert img.size == (W_IMG, H_IMG) and len(log["denoising"]["iter_time"]) == STEPS
    assert np.array_equal(arr[:, :W_IMG // 2], RGB[:, :W_IMG // 2])
    raw, _ = pipe.generate_image("a cat", mask_path=mpath, composite=False, **kw)
    raw = np.asarray(raw)
    assert np.array_equal(raw[:, W_IMG // 2:], arr[:, W_IMG // 2:])  # repainted pixels: the decoder's bytes either way
    assert not np.array_equal(raw[:, :W_IMG // 2], RGB[:, :W_IMG // 2])
    # decode_async users: the public paste-back on decoded bytes
    pasted = pipe.composite_image(torch.from_numpy(raw[None].copy()).to(dev), RGB, HALF)
    assert np.array_equal(pasted[0].cpu().numpy(), arr)
    with pytest.raises(ValueError, match="image_path"):
        pipe.generate_image("a cat", num_steps=2, latent_size=(HL, WL), seed=SEED, mask_path=mpath, verbose=False)
    text, pooled = pipe.encode_text("a cat")
    with pytest.raises(ValueError, match="image_path"):
        pipe.denoise_latents(text, pooled, num_steps=2, latent_size=(HL, WL), seed=SEED, mask_path=mpath)


def test_cli_with_mask(dev, tmp_path):
    """--image-path + --mask-path through cli.main on tiny configs: an image of the right size, kept pixels from the input; --no-composite: not"""
    from PIL import Image
    from diffusionkit_amd import cli
    over = dict(mmdit_config=tiny_flux(), vae_config=tiny_vae(), vae_encoder_config=tiny_vae_encoder(), text_len=20)
    ipath, mpath, out = str(tmp_path / "init.png"), str(tmp_path / "mask.png"), tmp_path / "out.png"
    Image.fromarray(RGB).save(ipath)
    Image.fromarray(np.stack([HALF, 255 - HALF, HALF], -1)).save(mpath)  # three channels: the first one counts
    argv = ["--prompt", "a cat", "--steps", "4", "--seed", "7", "--height", str(H_IMG), "--width", str(W_IMG), "-o", str(out), "--image-path", ipath,
            "--denoise", "1.0", "--mask-path", mpath]
    img, log = cli.main(argv, pipeline_overrides=over)
    assert out.exists() and img.size == (W_IMG, H_IMG) and len(log["denoising"]["iter_time"]) == 4
    assert np.array_equal(np.asarray(Image.open(out).convert("RGB"))[:, :W_IMG // 2], RGB[:, :W_IMG // 2])
    img2, _ = cli.main(argv + ["--no-composite"], pipeline_overrides=over)
    assert not np.array_equal(np.asarray(img2)[:, :W_IMG // 2], RGB[:, :W_IMG // 2])
    assert np.array_equal(np.asarray(img2)[:, W_IMG // 2:], np.asarray(img)[:, W_IMG // 2:])
