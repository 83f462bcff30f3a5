"""Inpainting (latent blending for flow matching) without a GPU: the mask reader, the CLI flags, and the masked reference loop.

The reference has no inpainting, so its loop is restated here: ``oracle.pipeline.cfg_denoise`` and the update of ``oracle.pipeline.sample_euler``,
with the blend behind every step,
    known = sigma_next * noise + (1 - sigma_next) * x_orig,    x = m * x_new + (1 - m) * known,
x_orig = process_in(the encoded image), noise = the get_noise(seed) draw of the start state, m in [0, 1] per latent cell (1 = repaint).  The tests
below show that this restatement has every property the GPU tests (tests/test_gpu_inpaint.py) then demand of the HIP path: m == 1 is img2img bit for
bit, m == 0 returns the encoded image bit for bit (the schedules end in sigma = 0), and a half mask keeps its kept cells bit-equal."""
import numpy as np
import pytest
import torch

from diffusionkit_amd import cli
from diffusionkit_amd.config import MMDIT_CKPT, tiny_flux, tiny_sd3
from diffusionkit_amd.weights import synth_mmdit_weights
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec
from tests._util import BF, randn

F16 = torch.float16


def make_image(H, W, seed=0):
    """tests/test_gpu_model.py's _test_image: a colour ramp with seeded noise, HWC uint8"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(yy * 255 // H), (xx * 255 // W), ((yy + xx) * 255 // (H + W))], -1)
    return np.clip(base + rng.randint(-20, 20, size=(H, W, 3)), 0, 255).astype(np.uint8)


def latent_mask(mask_u8: np.ndarray, f: int = 8) -> torch.Tensor:
    """uint8 [H, W] -> f32 [H / f, W / f]: (integer sum of the f x f block) / (f * f * 255) in float32 -- what dk_mask_to_latent_f32 computes"""
    H, W = mask_u8.shape
    s = mask_u8.astype(np.int64).reshape(H // f, f, W // f, f).sum(axis=(1, 3))
    return torch.from_numpy(s.astype(np.float32) / np.float32(f * f * 255))


def masked_sample_euler(model, x_orig, m, seed, sigmas, conditioning, pooled, cfg_weight, act, t_act=None):
    """oracle.pipeline.sample_euler from the img2img start state, with the blend behind every step.  x_orig: fp32 [1, h, w, 16] (after
    process_in); m: fp32 [h, w].  Returns the latent BEFORE process_out."""
    h, w = x_orig.shape[1:3]
    noise = op.get_noise(seed, h, w)
    mm = m.to(torch.float32)[None, :, :, None]
    x = sigmas[0] * noise + (1.0 - sigmas[0]) * x_orig  # sampler.py:41-42, as oracle.pipeline.denoise_latents
    timesteps = (t_act or act).r(sigmas * 1000.0)
    model.cache_modulation_params(pooled, timesteps)
    for i in range(len(sigmas) - 1):
        den = op.cfg_denoise(model, x, float(timesteps[i]), float(sigmas[i]), conditioning, cfg_weight, act)
        d = (x - den) / sigmas[i]
        x = x + d * (sigmas[i + 1] - sigmas[i])
        known = sigmas[i + 1] * noise + (1.0 - sigmas[i + 1]) * x_orig
        x = mm * x + (1.0 - mm) * known
    return x


def masked_denoise_latents(model, conditioning, pooled, num_steps, cfg_weight, seed, shift, flux, act, init_latent, m, denoise=1.0, t_act=None):
    """oracle.pipeline.denoise_latents(init_latent=...) with a latent mask: (latent before process_out, x_orig)"""
    fmt = "flux" if flux else "sd3"
    x_orig = op.process_in(init_latent, fmt)
    sigmas = op.get_sigmas(shift, flux, num_steps)
    sigmas = sigmas[int(num_steps * (1 - denoise)):]
    return masked_sample_euler(model, x_orig, m, seed, sigmas, conditioning, pooled, cfg_weight, act, t_act), x_orig


FAMILIES = {"flux": (tiny_flux(), 1.0, 0.0), "sd3_cfg": (tiny_sd3(), 3.0, 5.0)}  # name -> (config, shift, cfg weight)


def family_inputs(name):
    """(cfg, shift, cfg weight, text, pooled) with the conditioning rows the oracle takes: [prompt, negative] under CFG, else one row"""
    cfg, shift, cfgw = FAMILIES[name]
    rows = 2 if cfgw > 0 else 1
    return cfg, shift, cfgw, randn(rows, 16, cfg.token_level_text_embed_dim, seed=7), randn(rows, cfg.pooled_text_embed_dim, seed=8)


def t_act_of(cfg):
    return None if cfg.is_flux else Prec(F16)  # SD3 timesteps: fp16 (quirk Q1)


# ---- read_mask ---------------------------------------------------------------------------------------------------------------------------
def half_mask(H, W):
    m = np.zeros((H, W), dtype=np.uint8)
    m[:, W // 2:] = 255
    return m


def test_read_mask_inputs_and_channels(tmp_path):
    from PIL import Image
    from diffusionkit_amd.pipeline import read_mask
    m = half_mask(64, 128)
    m[3, 5] = 77  # a value between: passes through untouched
    path = str(tmp_path / "mask.png")
    Image.fromarray(m).save(path)
    for src in (path, Image.fromarray(m), m):
        got = read_mask(src, (64, 128))
        assert got.dtype == np.uint8 and got.shape == (64, 128) and got.flags["C_CONTIGUOUS"] and np.array_equal(got, m)
    # 3 and 4 channels: only the first one is taken
    other = np.full((64, 128), 9, dtype=np.uint8)
    rgb, rgba = np.stack([m, other, other], -1), np.stack([m, other, other, other], -1)
    for arr in (rgb, rgba):
        assert np.array_equal(read_mask(arr, (64, 128)), m)
        assert np.array_equal(read_mask(Image.fromarray(arr), (64, 128)), m)
    p3 = str(tmp_path / "mask_rgb.png")
    Image.fromarray(rgb).save(p3)
    assert np.array_equal(read_mask(p3, (64, 128)), m)
    assert np.array_equal(read_mask(m > 127, (64, 128)), np.where(m > 127, 255, 0))  # a bool array: True = repaint
    with pytest.raises(ValueError):
        read_mask(m.astype(np.float32), (64, 128))
    with pytest.raises(ValueError):
        read_mask(np.zeros((2, 2, 2, 2), dtype=np.uint8), (64, 128))


def test_read_mask_resizes_with_nearest():
    """a 100 x 150 mask against the 64 x 128 image read_image makes of a 100 x 150 input: NEAREST keeps the values in {0, 255}"""
    from PIL import Image
    from diffusionkit_amd.pipeline import read_image_u8, read_mask
    assert read_image_u8(make_image(100, 150, seed=2)).shape == (64, 128, 3)
    m = half_mask(100, 150)
    got = read_mask(m, (64, 128))
    assert got.shape == (64, 128) and set(np.unique(got).tolist()) == {0, 255}
    assert np.array_equal(got, np.array(Image.fromarray(m).resize((128, 64), Image.NEAREST)))
    assert not got[:, :60].any() and got[:, 68:].all()  # still the right half


def test_read_image_u8_is_what_read_image_normalises():
    """read_image = read_image_u8 / 255 * 2 - 1: the paste-back uses the very pixels the encoder saw"""
    from diffusionkit_amd.pipeline import read_image_u8
    rgb = make_image(64, 128, seed=1)
    assert np.array_equal(read_image_u8(rgb), rgb)
    assert np.array_equal(read_image_u8(rgb[:, :, 0]), np.repeat(rgb[:, :, :1], 3, axis=2))  # grey -> three equal channels
    assert np.array_equal(read_image_u8(np.concatenate([rgb, rgb[:, :, :1]], -1)), rgb)  # alpha dropped


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------
def parse(argv):
    return cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(argv)


def test_cli_mask_flags():
    with pytest.raises(ValueError, match="--image-path"):
        cli.resolve(parse(["--prompt", "x", "--mask-path", "m.png"]))
    r = cli.resolve(parse(["--prompt", "x", "--image-path", "a.png", "--mask-path", "m.png"]))
    assert r["mask_path"] == "m.png" and "composite" not in r
    r = cli.resolve(parse(["--prompt", "x", "--image-path", "a.png", "--mask-path", "m.png", "--no-composite"]))
    assert r["mask_path"] == "m.png" and r["composite"] is False
    # without the flags the dict is what it was
    r = cli.resolve(parse(["--prompt", "a cat"]))
    assert r == {"cfg": 0.0, "shift": 1.0, "height": 512, "width": 512, "flux": True, "low_memory_mode": True}
    r = cli.resolve(parse(["--prompt", "a cat", "--image-path", "a.png", "--denoise", "0.5"]))
    assert r == {"cfg": 0.0, "shift": 1.0, "height": 512, "width": 512, "flux": True, "low_memory_mode": True}


def test_pipeline_keywords_are_keyword_only():
    """the reference's positional signatures stay verbatim; the new arguments come behind them, keyword-only"""
    import inspect
    from diffusionkit_amd.pipeline import DiffusionPipeline
    d = inspect.signature(DiffusionPipeline.denoise_latents).parameters
    assert list(d)[:9] == ["self", "conditioning", "pooled_conditioning", "num_steps", "cfg_weight", "latent_size", "seed", "image_path", "denoise"]
    assert d["mask_path"].kind is inspect.Parameter.KEYWORD_ONLY and d["mask_path"].default is None
    g = inspect.signature(DiffusionPipeline.generate_image).parameters
    assert list(g)[:10] == ["self", "text", "num_steps", "cfg_weight", "negative_text", "latent_size", "seed", "verbose", "image_path", "denoise"]
    assert g["mask_path"].kind is inspect.Parameter.KEYWORD_ONLY and g["composite"].kind is inspect.Parameter.KEYWORD_ONLY
    assert g["mask_path"].default is None and g["composite"].default is True


# ---- the restated reference loop on the fp32 oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FAMILIES))
def test_masked_reference_loop_properties(name):
    """4 steps at latent 8 x 16, a random x_orig: all-255 == img2img, all-0 == x_orig, a half mask keeps its kept cells bit for bit"""
    cfg, shift, cfgw, text, pooled = family_inputs(name)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    model = OracleMMDiT(cfg, wf, Prec())
    z0 = torch.randn(1, 8, 16, 16, generator=torch.Generator().manual_seed(11))
    kw = dict(act=Prec(BF), t_act=t_act_of(cfg))

    def run(mask_u8):
        return masked_denoise_latents(model, text, pooled, 4, cfgw, 2, shift, cfg.is_flux, init_latent=z0, m=latent_mask(mask_u8), **kw)

    fmt = "flux" if cfg.is_flux else "sd3"
    ones, x_orig = run(np.full((64, 128), 255, dtype=np.uint8))
    ref = op.denoise_latents(model, text, pooled, 4, cfgw, (8, 16), 2, shift, cfg.is_flux, init_latent=z0, **kw)
    assert torch.equal(op.process_out(ones, fmt), ref)
    zeros, _ = run(np.zeros((64, 128), dtype=np.uint8))
    assert torch.equal(zeros, x_orig)
    mask = half_mask(64, 128)
    mask[8:32, 56:64] = np.where(np.arange(8)[None, :] % 2 == 0, 255, 0)  # three seam cells at m = 0.5 (rows 1..3, column 7)
    m = latent_mask(mask)
    assert float(m.min()) == 0.0 and float(m.max()) == 1.0 and int((m == 0.5).sum()) == 3
    half, _ = run(mask)
    kept, repaint = (m == 0.0), (m == 1.0)
    assert torch.equal(half[0][kept], x_orig[0][kept])
    diff = float((half[0][repaint] - ones[0][repaint]).abs().max())
    print(f"[inpaint] {name}: repainted cells of the half mask differ from the all-255 run by at most {diff:.3f}")
    assert diff > 0.0  # the repainted half attends to another left half
    assert bool(torch.isfinite(half).all())


# ---- NaN footprint of the masked step (the GPU test's case family, proven here against hand-written dependency sets) ---------------------------
STEP_SHAPE = dict(n_img=2, Hl=6, Wl=10, C=16, p=2)  # 1920 latent elements: the last block of 256 threads is half empty; Hl != Wl


def masked_step_family(flux, per_image, n_img=2, Hl=6, Wl=10, C=16, p=2):
    """dk_euler_cfg_step_masked with CFG on, in the manner of tests/_footprint.py's patchify_family (the patch order is taken from the oracle once,
    on a tensor of element indices).  Operands: x, out [2 n_img, S_i, F], x_orig, noise, mask [n_img or 1, Hl, Wl]; outputs: ``x`` (the blended
    latent) and ``tok`` (its patchified rounding, both CFG copies)."""
    from tests import _footprint as fp
    S_i, F = (Hl // p) * (Wl // p), p * p * C
    orc = OracleMMDiT(tiny_flux() if flux else tiny_sd3(),
                      {"x_embedder.proj.weight": torch.eye(F).reshape(F, *((1, 1, F) if flux else (p, p, C))), "x_embedder.proj.bias": torch.zeros(F)}, Prec())

    def g(seed):
        return torch.Generator().manual_seed(seed)
    ops = dict(x=torch.randn(n_img, Hl, Wl, C, generator=g(80)), out=fp.rounder(BF)(2 * n_img, S_i, F, seed=81),
               x_orig=torch.randn(n_img, Hl, Wl, C, generator=g(82)) * 1.5 + 0.3, noise=torch.randn(n_img, Hl, Wl, C, generator=g(83)),
               mask=torch.rand(n_img if per_image else 1, Hl, Wl, generator=g(84)))
    sigma, sigma_next, wgt = 0.75, 0.5, 5.0
    index = torch.arange(n_img * Hl * Wl * C, dtype=torch.float32).reshape(n_img, Hl, Wl, C)
    where = orc._patch_embed(index).long()  # [n_img, S_i, F]: which latent element each token feature is
    assert torch.equal(torch.sort(where.reshape(-1))[0], torch.arange(index.numel()))  # a permutation

    def patch(x):
        t = x.reshape(-1)[where]
        return torch.cat([t, t])

    def ref(o):
        u = torch.empty(2 * n_img * Hl * Wl * C)
        u[torch.cat([where, where + index.numel()]).reshape(-1)] = o["out"].reshape(-1)  # (unpatchify, per CFG copy)
        u = u.reshape(2 * n_img, Hl, Wl, C)
        den, den_neg = o["x"] - u[:n_img] * sigma, o["x"] - u[n_img:] * sigma
        den = den_neg + wgt * (den - den_neg)
        x_new = o["x"] + (o["x"] - den) / sigma * (sigma_next - sigma)
        known = sigma_next * o["noise"] + (1.0 - sigma_next) * o["x_orig"]
        m = o["mask"][:, :, :, None]
        xb = m * x_new + (1.0 - m) * known
        return dict(x=xb, tok=patch(xb))

    def hands(mx):
        mt = torch.isin(where, index[mx].long())
        assert int(mt.sum()) == int(mx.sum())
        return dict(x=mx, tok=torch.cat([mt, mt]))

    def elems(*idx):
        mx = torch.zeros(n_img, Hl, Wl, C, dtype=torch.bool)
        mx[idx] = True
        return mx
    cell = (1, 3, 6) if per_image else (0, 3, 6)
    cases = [fp.Case("one noise element", [("noise", (1, 4, 7, 9))], hands(elems(1, 4, 7, 9))),
             fp.Case("one x_orig element, last cell of image 0", [("x_orig", (0, Hl - 1, Wl - 1, C - 1))], hands(elems(0, Hl - 1, Wl - 1, C - 1))),
             fp.Case("one mask cell", [("mask", cell)], hands(elems(1, 3, 6) if per_image else elems(slice(None), 3, 6)))]
    return ops, ref, (sigma, sigma_next, wgt), cases


@pytest.mark.parametrize("flux", [True, False], ids=["flux", "sd3"])
@pytest.mark.parametrize("per_image", [False, True], ids=["shared", "per_image"])
def test_masked_step_reference_has_the_hand_written_footprints(flux, per_image):
    """the reference of the GPU footprint test: isnan(ref(poisoned)) is the hand-written dependency set (one element and its token feature in both CFG
    copies; a mask cell: its C channels, in every image that shares the mask), and everything outside is bit-equal to the reference's own clean run"""
    from tests import _footprint as fp
    ops, ref, _, cases = masked_step_family(flux, per_image, **STEP_SHAPE)
    clean = ref(ops)
    assert int(cases[0].hand["x"].sum()) == 1 and int(cases[0].hand["tok"].sum()) == 2
    assert int(cases[2].hand["x"].sum()) == 16 * (1 if per_image else 2) and int(cases[2].hand["tok"].sum()) == 2 * int(cases[2].hand["x"].sum())
    for case in cases:
        got = ref(fp.poisoned(ops, case))
        for key in ("x", "tok"):
            assert torch.equal(torch.isnan(got[key]), case.hand[key]), (case.label, key)
            fp.assert_footprint(clean[key], got[key], case.hand[key], f"{case.label} [{key}]")
