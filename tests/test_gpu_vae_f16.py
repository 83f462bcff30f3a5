"""Parity of the float16 VAE on an MI355X: the operators (conv forms of the GEMM kernels, GroupNorm, the fused norm -> silu -> conv with its image
tail, the D = 512 attention, softmax / transpose), the decoder and encoder engines and the pipeline switch ``vae_dtype``.

Gates are derived, not tuned.
  operators: relative L2 against the EXACT result on the fp16-rounded operands (fp32 oracle) <= TOL_SINGLE_OP / 8 = 3.75e-4 -- the bf16 gate
      divided by 2^3 for fp16's three more mantissa bits, as tests/test_gpu_f16_ops.py gates the fp16 GEMMs; attention 6e-3 / 8 = 7.5e-4.
  engines: both errors are relative L2 against the fp32 oracle on the fp16-rounded weights; emu16 = the oracle with Prec(torch.float16), emubf =
      the oracle with Prec(torch.bfloat16):
          err(hip) <= 2 * err(emu16) + 2.5e-4   and   err(hip) <= 0.5 * err(emubf)
      (tests/test_gpu_f16_model.py's gate: emu16 alone sits at 0.12 x emubf on these inputs, a bf16 rounding anywhere on the path fails the second)
  image: PSNR against the fp32 oracle's image >= what the emu16 image reaches - 2 dB (the margin of the project's fp16 full-size gates).
Every figure is printed before it is asserted.

The file name sorts behind tests/test_gpu_fullsize.py on purpose: that file's weight prefetch (start_synth_prefetch, started at collection) hands the
SD3-medium set out for 1 + 3 uses under one key, and its four consumers are served only if the first of them runs before the second draw replaces the
first -- a test file in front of it moves that first use later.  Nothing here belongs to that schedule."""
import functools
import math

import numpy as np
import pytest
import torch

from diffusionkit_amd.config import (VAEDecoderConfig, VAEEncoderConfig, float16_vae_config, tiny_flux, tiny_sd3, tiny_vae, tiny_vae_encoder)
from diffusionkit_amd.weights import pack_vae, synth_mmdit_weights, synth_vae_encoder_weights, synth_vae_weights
from oracle import mmdit as om
from oracle import pipeline as op
from oracle import vae as ov
from oracle.mmdit import OracleMMDiT, Prec
from oracle.vae import OracleVAEDecoder, OracleVAEEncoder
from tests._util import BF, TOL_SINGLE_OP, psnr, randn, rel_l2

pytestmark = pytest.mark.gpu

F16 = torch.float16
TOL_F16 = TOL_SINGLE_OP / 8   # 3.75e-4
TOL_ATTN_F16 = 6e-3 / 8       # 7.5e-4
FLOOR_F16 = 2e-3 / 8


def f16r(x):
    """values representable in fp16, kept as fp32 (what both sides see as input)"""
    return x.to(F16).float()


def rnd(*shape, seed, scale=1.0):
    return f16r(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale)


def g(x, dev):
    return x.to(dev, F16).contiguous()


def op_gate(exact, got, what, tol=TOL_F16):
    e = rel_l2(exact, got.float())
    print(f"[f16 vae op] {what}: rel-L2 {e:.3e} against the exact result (gate {tol:.3e})")
    assert e <= tol, f"{what}: {e:.3e} > {tol:.3e}"


# ---- conv3x3: the conv forms of the GEMM kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,O,ups,res,mode", [(1, 16, 16, 64, 128, False, False, -1),   # plain
                                                    (2, 6, 10, 64, 128, False, True, -1),     # residual; sides that are no multiples of 16
                                                    (1, 8, 12, 64, 64, True, False, -1),      # through the nearest-x2 view
                                                    (1, 16, 16, 128, 256, False, False, 9)])  # forced onto gemm256v3's conv form
def test_conv3x3_f16(dev, B, H, W, C, O, ups, res, mode):
    from diffusionkit_amd import ops
    x, w, b = rnd(B, H, W, C, seed=20), rnd(O, 3, 3, C, seed=21, scale=0.05), rnd(O, seed=22, scale=0.1)
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    r = rnd(B, Ho, Wo, O, seed=23) if res else None
    try:
        ops.tune("gemm", mode)
        y = ops.conv3x3(g(x, dev), g(w, dev), g(b, dev), upsample=ups, res=g(r, dev) if res else None)
    finally:
        ops.tune("gemm", -1)
    ref = ov.conv2d_nhwc(ov.upsample_nearest(x) if ups else x, w, b, Prec())
    if res:
        ref = ref + r
    assert y.dtype == F16 and y.shape == ref.shape
    op_gate(ref, y, f"conv3x3 {(B, H, W, C, O)} ups {ups} res {res} gemm {mode}")
    if mode == 9:
        assert ops.conv3x3_plan(B, Ho, Wo, C, O, dtype=F16).kernel == 128  # (without the knob this shape stays on the 128^2 tiles)


@pytest.mark.parametrize("B,H,W,C,O", [(1, 16, 16, 128, 128), (2, 8, 24, 128, 64)])
def test_conv3x3_stride2_f16(dev, B, H, W, C, O):
    """the encoder's downsample (vae.py:141-143): pad bottom / right by one, conv k3 s2 p0"""
    from diffusionkit_amd import ops
    x, w, b = rnd(B, H, W, C, seed=24), rnd(O, 3, 3, C, seed=25, scale=0.05), rnd(O, seed=26, scale=0.1)
    y = ops.conv3x3(g(x, dev), g(w, dev), g(b, dev), downsample=True)
    ref = ov.conv2d_s2_pad_br_nhwc(x, w, b, Prec())
    assert y.dtype == F16 and y.shape == ref.shape == (B, H // 2, W // 2, O)
    op_gate(ref, y, f"conv3x3 stride 2 {(B, H, W, C, O)}")


def test_mixed_element_types_are_refused(dev):
    from diffusionkit_amd import _lib, ops
    x, w, b = rnd(1, 16, 16, 64, seed=1), rnd(128, 3, 3, 64, seed=2, scale=0.05), rnd(128, seed=3, scale=0.1)
    with pytest.raises(_lib.DkHipError, match="float16"):
        ops.conv3x3(g(x, dev), w.to(dev, BF), g(b, dev))
    with pytest.raises(_lib.DkHipError, match="mixed element types"):
        ops.conv3x3(g(x, dev), g(w, dev), b.to(dev, BF))
    with pytest.raises(_lib.DkHipError, match="float16"):
        ops.conv3x3_gn(g(x, dev), w.reshape(128, -1).to(dev, BF), g(b, dev))
    with pytest.raises(_lib.DkHipError, match="mixed element types"):
        ops.conv3x3_gn(g(x, dev), g(w.reshape(128, -1), dev), g(b, dev), res=torch.zeros(1, 16, 16, 128, dtype=BF, device=dev))
    with pytest.raises(_lib.DkHipError, match="mixed element types"):
        ops.groupnorm(g(x, dev), torch.ones(64, dtype=BF, device=dev), torch.zeros(64, dtype=F16, device=dev), 32, 1e-5, True)
    with pytest.raises(_lib.DkHipError, match="mixed element types"):
        ops.groupnorm_table(x.to(dev, BF), torch.ones(64, dtype=F16, device=dev), torch.zeros(64, dtype=F16, device=dev), 32, 1e-5)
    q = g(rnd(1, 64, 512, seed=4), dev)
    with pytest.raises(_lib.DkHipError, match="float16"):
        ops.attention_d512(q, q.to(BF), q)
    with pytest.raises(_lib.DkHipError):
        ops.transpose(torch.zeros(8, 8, device=dev))  # fp32


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,G,HW,silu", [(64, 32, (8, 8), True), (512, 32, (8, 8), False)])
def test_groupnorm_f16(dev, C, G, HW, silu):
    from diffusionkit_amd import ops
    B = 2
    x = f16r(rnd(B, HW[0], HW[1], C, seed=60, scale=2.0) + 0.7)
    gamma, beta = f16r(1 + rnd(C, seed=61, scale=0.1)), rnd(C, seed=62, scale=0.1)
    y = ops.groupnorm(g(x, dev), g(gamma, dev), g(beta, dev), G, 1e-5, silu)
    P = Prec(F16)
    ref = ov.group_norm_nhwc(x, gamma, beta, G, 1e-5, P)
    if silu:
        ref = ov.silu(ref, P)
    assert y.dtype == F16
    op_gate(ref, y, f"groupnorm C {C} silu {silu} (against the fp16-emulating oracle)")


# ---- the fused norm -> silu -> conv --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,O,res,sc,gn,ups", [(1, 16, 16, 64, 128, False, 0, True, False),     # one tile: every border is padding
                                                     (2, 32, 48, 128, 128, True, 0, True, False),     # 12 tiles, two images, residual
                                                     (1, 48, 32, 256, 128, False, 256, True, False),  # 256-channel shortcut extension
                                                     (1, 32, 32, 64, 256, False, 0, False, False),    # no table, two column tiles
                                                     (2, 16, 24, 128, 256, False, 0, False, True)])   # through the nearest-x2 view
def test_conv3x3_gn_f16(dev, B, H, W, C, O, res, sc, gn, ups):
    """conv_halo.hip on IEEE half: against emu16's GroupNorm + SiLU followed by the exact conv; the output statistics against a statistics pass over
    the stored output; and bit-identical under conv_v4 = 0 and 2 -- an fp16 launch never reaches the bf16 asm kernel (conv256v4.hip)"""
    from diffusionkit_amd import ops
    G, eps = 32, 1e-5
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    x = f16r(rnd(B, H, W, C, seed=80, scale=1.5) + 0.3)
    gamma, beta = f16r(1 + rnd(C, seed=81, scale=0.1)), rnd(C, seed=82, scale=0.1)
    w, b = rnd(O, 3, 3, C, seed=83, scale=0.05), rnd(O, seed=84, scale=0.1)
    r = rnd(B, Ho, Wo, O, seed=85) if res else None
    x2 = rnd(B, Ho, Wo, sc, seed=86) if sc else None
    ws = rnd(O, sc, seed=87, scale=0.05) if sc else None
    bs = rnd(O, seed=88, scale=0.1) if sc else None
    P = Prec(F16)
    act = ov.silu(ov.group_norm_nhwc(x, gamma, beta, G, eps, P), P) if gn else x
    ref = ov.conv2d_nhwc(ov.upsample_nearest(act) if ups else act, w, b, Prec())
    if res:
        ref = ref + r
    if sc:
        ref = ref + (x2 @ ws.t() + bs)
    xd = g(x, dev)
    tab = ops.groupnorm_table(xd, g(gamma, dev), g(beta, dev), G, eps) if gn else None
    wk = w.reshape(O, -1)
    if sc:
        wk = torch.cat([wk, ws], dim=1)
    outs = {}
    try:
        for mode in (0, 2):
            ops.tune("conv_v4", mode)
            outs[mode] = ops.conv3x3_gn(xd, g(wk, dev), g(b, dev), gn_table=tab, silu=True, res=g(r, dev) if res else None,
                                        x2=g(x2, dev) if sc else None, bias2=g(bs, dev) if sc else None, stats_groups=G, upsample=ups)
    finally:
        ops.tune("conv_v4", 1)
    y, part = outs[0]
    assert y.dtype == F16 and y.shape == ref.shape
    op_gate(ref, y, f"conv3x3_gn {(B, H, W, C, O)} res {res} shortcut {sc} table {gn} ups {ups}")
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])
    g2, b2 = f16r(1 + rnd(O, seed=89, scale=0.1)), rnd(O, seed=90, scale=0.1)
    t_part = ops.groupnorm_table(None, g(g2, dev), g(b2, dev), G, eps, partials=part, shape=(B, Ho * Wo, O))
    t_pass = ops.groupnorm_table(y.contiguous(), g(g2, dev), g(b2, dev), G, eps)
    e = rel_l2(t_pass.cpu(), t_part.cpu())
    print(f"[f16 vae op] statistics table from the partials against a pass over the output: {e:.3e}")
    assert e < 1e-5


def test_conv_out_image_tail_f16(dev):
    """conv_norm_out -> silu -> conv_out -> clip / uint8 in one launch, every product of the tail in fp16 (the reference's rule for SD3:
    mlx/__init__.py:581-584, 525-526)"""
    from diffusionkit_amd import ops
    B, H, W, C, G, eps = 2, 32, 48, 128, 32, 1e-5
    x = f16r(rnd(B, H, W, C, seed=91, scale=1.5) + 0.3)
    gamma, beta = f16r(1 + rnd(C, seed=92, scale=0.1)), rnd(C, seed=93, scale=0.1)
    w, b = rnd(3, 3, 3, C, seed=94, scale=0.05), rnd(3, seed=95, scale=0.1)
    P = Prec(F16)
    act = ov.silu(ov.group_norm_nhwc(x, gamma, beta, G, eps, P), P)
    ref = ov.conv2d_nhwc(act, w, b, Prec())
    xd = g(x, dev)
    tab = ops.groupnorm_table(xd, g(gamma, dev), g(beta, dev), G, eps)
    img, u8, raw = ops.conv3x3_gn(xd, g(w, dev).reshape(3, -1), g(b, dev), gn_table=tab, image=True)
    assert raw.dtype == F16
    op_gate(ref, raw[..., :3], "image tail raw")
    assert torch.all(raw[..., 3].float() == 0)
    want = torch.clip((raw[..., :3].float() / 2 + 0.5).to(F16).float(), 0, 1)
    assert torch.equal(img, want)
    assert torch.equal(u8, (want.to(F16) * 255).to(F16).to(torch.uint8))


# ---- D = 512 attention, softmax, transpose -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(1, 64), (2, 96), (1, 100)])
def test_attention_d512_f16(dev, B, T):
    from diffusionkit_amd import ops
    D = 512
    q, k, v = (rnd(B, T, D, seed=s) for s in (34, 35, 36))
    y = ops.attention_d512(g(q, dev), g(k, dev), g(v, dev))
    ref = om.sdpa(q[:, None], k[:, None], v[:, None], 1.0 / math.sqrt(D), Prec())[:, 0]
    assert y.dtype == F16
    op_gate(ref, y, f"attention_d512 B {B} T {T}", TOL_ATTN_F16)


def test_attention_d512_spiked_key_f16(dev):
    """a key that dominates late forces the deferred rescale across the S -> PV hand-off; fp16-rounded inputs against fp64"""
    from diffusionkit_amd import ops
    T, D = 320, 512
    q, k, v = (rnd(1, T, D, seed=s, scale=0.5) for s in (37, 38, 39))
    k[0, 250] = f16r(q[0, 7] * 6.0)  # key 250 aligned with query 7
    p = torch.softmax(q[0].double() @ k[0].double().t() / math.sqrt(D), dim=-1)
    ref = (p @ v[0].double())[None]
    assert float(p[7, 250]) > 0.9
    y = ops.attention_d512(g(q, dev), g(k, dev), g(v, dev))
    assert torch.isfinite(y.float()).all()
    op_gate(ref, y, "attention_d512 spiked key", TOL_ATTN_F16)


def test_softmax_and_transpose_f16(dev):
    from diffusionkit_amd import ops
    x = rnd(64, 256, seed=70, scale=3.0)
    y = ops.softmax_rows_(g(x, dev).clone())
    assert y.dtype == F16
    op_gate(torch.softmax(x, -1), y, "softmax_rows")
    z = ops.transpose(g(x, dev))
    assert z.dtype == F16 and torch.equal(z.float().cpu(), x.t())
    zr = ops.transpose(g(x[:37, :50].contiguous(), dev))  # sides that are no multiples of the 32 x 32 tile
    assert torch.equal(zr.float().cpu(), x[:37, :50].t())
    # ragged row length inside a padded row: the padding is ignored on input (NaNs there must not leak) and comes out as zeros
    buf = g(x, dev).clone()
    buf[:, 100:] = float("nan")
    ops.softmax_rows_(buf[:, :100])
    full = buf.float().cpu()
    op_gate(torch.softmax(x[:, :100], -1), full[:, :100], "softmax_rows, padded row")
    assert torch.all(full[:, 100:] == 0)
    # rows longer than the register cache
    xl = rnd(2, 16384 + 4096, seed=71, scale=3.0)
    bl = g(xl, dev).clone()
    ops.softmax_rows_(bl[:, :20000])
    fl = bl.float().cpu()
    op_gate(torch.softmax(xl[:, :20000], -1), fl[:, :20000], "softmax_rows, long rows")
    assert torch.all(fl[:, 20000:] == 0)


# ---- engines ---------------------------------------------------------------------------------------------------------------------------------
def gate(hip, emu16, emubf, exact, what):
    e_h, e_16, e_bf = rel_l2(exact, hip), rel_l2(exact, emu16), rel_l2(exact, emubf)
    print(f"[f16 vae] {what}: hip {e_h:.3e}, fp16-emulating oracle {e_16:.3e}, bf16-emulating oracle {e_bf:.3e} (PSNR hip {psnr(exact, hip):.2f} dB)")
    assert e_h <= 2.0 * e_16 + FLOOR_F16, f"{what}: hip-vs-fp32 {e_h:.3e} > 2 * emu16-vs-fp32 {e_16:.3e} + {FLOOR_F16}"
    assert e_h <= 0.5 * e_bf, f"{what}: hip-vs-fp32 {e_h:.3e} > 0.5 * bf16-emulation-vs-fp32 {e_bf:.3e}"
    return e_h


PRECS = (("fp32", Prec()), ("emu16", Prec(F16)), ("emubf", Prec(BF)))


@functools.lru_cache(maxsize=None)
def decoder_weights(prod: bool):
    """(config, source tensors, the fp32 view of what an fp16 engine holds): both sides of every comparison see the same values"""
    vcfg = VAEDecoderConfig() if prod else tiny_vae()
    named = synth_vae_weights(vcfg, seed=4321)
    return vcfg, named, {k: v.to(F16).float() for k, v in named.items()}


@functools.lru_cache(maxsize=None)
def tiny_decoder(dev):
    vcfg, named, _ = decoder_weights(False)
    from diffusionkit_amd.engine import VAEDecoderEngine
    c16 = float16_vae_config(vcfg)
    return VAEDecoderEngine(c16, pack_vae(c16, named, dev))


def image16(raw):
    """the reference's SD3 rule: the image is an fp16 product"""
    return torch.clip((raw / 2 + 0.5).to(F16).float(), 0, 1)


def decode_case(dev, prod, z, what):
    from diffusionkit_amd.engine import VAEDecoderEngine
    vcfg, named, wf = decoder_weights(prod)
    if prod:
        c16 = float16_vae_config(vcfg)
        eng = VAEDecoderEngine(c16, pack_vae(c16, named, dev))
    else:
        eng = tiny_decoder(dev)
    assert eng.dtype == F16
    img, u8, raw = eng.decode(z.to(dev), want_raw=True)
    assert raw.dtype == F16 and img.dtype == torch.float32 and u8.dtype == torch.uint8
    res = {n: OracleVAEDecoder(vcfg, wf, P)(f16r(z)) for n, P in PRECS}
    gate(raw[..., :3].float(), res["emu16"], res["emubf"], res["fp32"], what + " raw")
    ref_img = torch.clip(res["fp32"] / 2 + 0.5, 0, 1)
    p_h, p_16, p_bf = psnr(ref_img, img), psnr(ref_img, image16(res["emu16"])), psnr(ref_img, torch.clip((res["emubf"] / 2 + 0.5).to(BF).float(), 0, 1))
    print(f"[f16 vae] {what} image: PSNR hip {p_h:.2f} dB, fp16-emulating oracle {p_16:.2f} dB, bf16-emulating oracle {p_bf:.2f} dB (gate {p_16 - 2.0:.2f} dB)")
    assert p_h >= p_16 - 2.0
    assert torch.equal(img, image16(raw[..., :3].float()))
    assert torch.equal(u8, (img.to(F16) * 255).to(F16).to(torch.uint8))  # truncation of the fp16 product (mlx/__init__.py:525-526)
    assert torch.all(raw[..., 3].float() == 0)
    return eng


@pytest.mark.parametrize("hw", [(8, 8), (6, 10), (16, 8)])
def test_vae_decode_tiny_f16(dev, hw):
    z = torch.randn(2, hw[0], hw[1], 16, generator=torch.Generator().manual_seed(11))
    decode_case(dev, False, z, f"decoder tiny latent {hw}")


def test_vae_production_channels_f16(dev):
    """production channel plan (128, 256, 512, 512; 3 resnets per level) on a 16 x 16 latent: the D = 512 attention at T = 256 and the halo
    kernel at 512 channels"""
    z = torch.randn(1, 16, 16, 16, generator=torch.Generator().manual_seed(12))
    decode_case(dev, True, z, "decoder production plan latent (16, 16)")


def _test_image(H, W, seed=0):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(yy * 255 // H), (xx * 255 // W), ((yy + xx) * 255 // (H + W))], -1)
    return np.clip(base + rng.randint(-20, 20, size=(H, W, 3)), 0, 255).astype(np.uint8)


def encode_case(dev, cfg, seed_w, img, what):
    from diffusionkit_amd.engine import VAEEncoderEngine
    named = synth_vae_encoder_weights(cfg, seed=seed_w)
    wf = {k: v.to(F16).float() for k, v in named.items()}
    c16 = float16_vae_config(cfg)
    eng = VAEEncoderEngine(c16, pack_vae(c16, named, dev))
    assert eng.dtype == F16
    mom = eng.encode(img.to(dev))
    hid = mom[..., :cfg.out_channels]
    assert mom.dtype == F16 and hid.shape == (img.shape[0], img.shape[1] // 8, img.shape[2] // 8, cfg.out_channels)
    res = {n: OracleVAEEncoder(cfg, wf, P)(img) for n, P in PRECS}
    gate(hid.float(), res["emu16"], res["emubf"], res["fp32"], what + " moments")
    # sample() takes the fp16 moments: against the oracle's posterior sample of the same moments
    noise = randn(*hid.shape[:3], 16, seed=28)
    got = eng.sample(mom, noise.to(dev))
    ref = ov.sample_latent(hid.float().cpu(), noise)
    assert got.dtype == torch.float32 and torch.allclose(got.cpu(), ref, rtol=1e-5, atol=1e-6)
    return eng


@pytest.mark.parametrize("hw", [(64, 64), (128, 64)])
def test_vae_encode_tiny_f16(dev, hw):
    img = op.read_image_array(_test_image(*hw))
    encode_case(dev, tiny_vae_encoder(), 8765, torch.cat([img, -img], 0), f"encoder tiny image {hw}")


def test_vae_encoder_production_channels_f16(dev):
    encode_case(dev, VAEEncoderConfig(), 99, op.read_image_array(_test_image(128, 128, seed=3)), "encoder production plan image (128, 128)")


def test_latent_sample_f16_clips_the_log_variance(dev):
    from diffusionkit_amd.engine import VAEEncoderEngine
    c16 = float16_vae_config(tiny_vae_encoder())
    enc = VAEEncoderEngine(c16, pack_vae(c16, synth_vae_encoder_weights(c16), dev))
    mom = rnd(2, 4, 6, 32, seed=27)
    mom[0, 0, 0, 16] = 1000.0   # logvar clipped to 20
    mom[0, 0, 1, 17] = -1000.0  # logvar clipped to -30
    noise = randn(2, 4, 6, 16, seed=28)
    got = enc.sample(g(mom, dev), noise.to(dev))
    assert torch.allclose(got.cpu(), ov.sample_latent(mom, noise), rtol=1e-5, atol=1e-6)
    from diffusionkit_amd import _lib
    with pytest.raises(_lib.DkHipError, match="float16"):
        enc.sample(mom.to(dev, BF), noise.to(dev))


def test_dtype_field_bfloat16_changes_nothing_and_f16_engines_refuse_bf16(dev):
    from dataclasses import replace
    from diffusionkit_amd import _lib
    from diffusionkit_amd.engine import VAEDecoderEngine, VAEEncoderEngine
    vcfg, named, _ = decoder_weights(False)
    z = torch.randn(2, 8, 8, 16, generator=torch.Generator().manual_seed(11)).to(dev)
    outs = []
    for c in (vcfg, replace(vcfg, dtype="bfloat16"), float16_vae_config(vcfg, "bfloat16")):
        assert c == vcfg
        eng = VAEDecoderEngine(c, pack_vae(c, named, dev))
        assert eng.dtype == BF
        outs.append(eng.decode(z, want_raw=True))
    for o in outs[1:]:
        assert o[2].dtype == BF and all(torch.equal(a, b) for a, b in zip(outs[0], o))
    c16 = float16_vae_config(vcfg)
    with pytest.raises(_lib.DkHipError, match="float16"):
        VAEDecoderEngine(c16, pack_vae(vcfg, named, dev))  # bf16 tensors for an fp16 engine
    with pytest.raises(_lib.DkHipError, match="bfloat16"):
        VAEDecoderEngine(vcfg, pack_vae(c16, named, dev))  # and the other way round
    ecfg = tiny_vae_encoder()
    with pytest.raises(_lib.DkHipError, match="float16"):
        VAEEncoderEngine(float16_vae_config(ecfg), pack_vae(ecfg, synth_vae_encoder_weights(ecfg), dev))


def test_batch_of_two_equals_two_single_decodes_f16(dev):
    eng = tiny_decoder(dev)
    z = torch.randn(2, 16, 8, 16, generator=torch.Generator().manual_seed(11)).to(dev)
    both = [t.clone() for t in eng.decode(z, want_raw=True)]
    for i in range(2):
        one = eng.decode(z[i:i + 1].contiguous(), want_raw=True)
        assert all(torch.equal(a[i:i + 1], b) for a, b in zip(both, one)), i


# ---- pipeline ----------------------------------------------------------------------------------------------------------------------------------
def test_generate_image_f16_vae(dev):
    """DiffusionPipeline(activation_dtype="float16", vae_dtype="float16"): the image of generate_image is the fp16 decode of the latent; decode_async
    equals the inline decode; vae_dtype=None leaves the bf16 decoder of before, bit for bit"""
    from PIL import Image
    from diffusionkit_amd.engine import VAEDecoderEngine
    from diffusionkit_amd.pipeline import DiffusionPipeline
    cfg, vcfg = tiny_sd3(), tiny_vae()
    kw = dict(w16=True, a16=True, shift=3.0, mmdit_config=cfg, vae_config=vcfg, device=dev, text_len=16, activation_dtype="float16")
    pipe = DiffusionPipeline(vae_dtype="float16", **kw)
    assert pipe.decoder.dtype == F16 and pipe.vae_config == float16_vae_config(vcfg) and pipe.vae_encoder_config.dtype == "float16"
    img, log = pipe.generate_image("a photo of a cat", num_steps=2, cfg_weight=5.0, latent_size=(8, 8), seed=3, verbose=False)
    assert isinstance(img, Image.Image) and img.size == (64, 64) and len(log["denoising"]["iter_time"]) == 2
    text, pooled = pipe.encode_text("a photo of a cat", 5.0, "")
    lat, _ = pipe.denoise_latents(text, pooled, num_steps=2, cfg_weight=5.0, latent_size=(8, 8), seed=3)
    im16, u8, raw = pipe.decoder.decode(lat, want_raw=True)
    assert raw.dtype == F16
    assert np.array_equal(np.asarray(img), u8.reshape(-1, u8.shape[2], 3).cpu().numpy())  # the latent generate_image decoded
    # the decode is the fp16 decoder's: against the oracle on the pipeline's decoder weights
    named = synth_vae_weights(vcfg, seed=pipe.weights_seed + 1, device="cpu")
    wf = {k: v.to(F16).float() for k, v in named.items()}
    res = {n: OracleVAEDecoder(vcfg, wf, P)(f16r(lat.cpu())) for n, P in PRECS}
    gate(raw[..., :3].float(), res["emu16"], res["emubf"], res["fp32"], "pipeline decode raw")
    # decode_async: same kernels, same bits
    a_img, a_u8 = pipe.decode_async(lat).result()
    assert pipe._async_decoder.dtype == F16 and torch.equal(a_img, im16) and torch.equal(a_u8, u8)
    pipe.release_async_decoder()
    # packed_weights["vae_decoder"] in fp16
    c16 = float16_vae_config(vcfg)
    pipe_p = DiffusionPipeline(vae_dtype="float16", packed_weights={"vae_decoder": pack_vae(c16, named, dev)}, **kw)
    assert pipe_p.decoder.dtype == F16 and torch.equal(pipe_p.decoder.decode(lat)[1], u8)
    # vae_dtype=None (and "bfloat16"): today's decoder, also beside activation_dtype="float16"
    want = VAEDecoderEngine(vcfg, pack_vae(vcfg, named, dev)).decode(lat, want_raw=True)
    for v in (None, "bfloat16"):
        p0 = DiffusionPipeline(vae_dtype=v, **kw)
        assert p0.decoder.dtype == BF and p0.vae_config == vcfg
        assert all(torch.equal(a, b) for a, b in zip(p0.decoder.decode(lat, want_raw=True), want)), v
    assert not torch.equal(want[0], im16)


def test_img2img_through_the_f16_encoder(dev, tmp_path):
    """tests/test_gpu_model.py::test_img2img_pipeline_tiny with vae_dtype="float16": the image goes through the fp16 encoder (built on first use), the
    MMDiT stays bf16 -- gated against the oracle restatement with those rounding points, the project's chained-operator yardstick"""
    from PIL import Image
    from diffusionkit_amd.pipeline import FluxPipeline
    from tests.test_gpu_model import yardstick_ok
    cfg, ecfg = tiny_flux(), tiny_vae_encoder()
    pipe = FluxPipeline(w16=True, a16=True, mmdit_config=cfg, vae_config=tiny_vae(), vae_encoder_config=ecfg, device=dev, text_len=16, vae_dtype="float16")
    assert not hasattr(pipe, "encoder") and pipe.decoder.dtype == F16
    rgb = _test_image(64, 128, seed=1)
    path = str(tmp_path / "init.png")
    Image.fromarray(rgb).save(path)
    text, pooled = randn(1, 16, cfg.token_level_text_embed_dim, seed=7), randn(1, cfg.pooled_text_embed_dim, seed=8)
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=4, cfg_weight=0.0, latent_size=(8, 16), seed=2,
                                          image_path=path, denoise=0.5)
    assert pipe.encoder.dtype == F16 and len(iter_time) == 2 and lat.shape == (1, 8, 16, 16)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    ewf = {k: v.to(F16).float() for k, v in synth_vae_encoder_weights(ecfg, seed=1234 + 2).items()}
    res = {}
    for pname, PE, PM in (("fp32", Prec(), Prec()), ("emu", Prec(F16), Prec(BF))):
        z0 = op.encode_image_to_latents(OracleVAEEncoder(ecfg, ewf, PE), op.read_image_array(rgb), seed=2)
        res[pname] = op.denoise_latents(OracleMMDiT(cfg, wf, PM), text, pooled, 4, 0.0, (8, 16), 2, 1.0, True, Prec(BF), init_latent=z0, denoise=0.5)
    e_h, e_e = yardstick_ok(lat, res["emu"], res["fp32"], "img2img latent, fp16 encoder")
    print(f"[f16 vae] img2img latent: hip {e_h:.3e}, emulating oracle {e_e:.3e}, PSNR {psnr(res['fp32'], lat):.2f} dB")
    assert psnr(res["fp32"], lat) > 35.0
    img, log = pipe.generate_image("x", num_steps=2, latent_size=(8, 16), seed=2, image_path=path, denoise=1.0, verbose=False)
    assert img.size == (128, 64) and len(log["denoising"]["iter_time"]) == 2


def test_cli_end_to_end_tiny_f16_vae(dev, tmp_path):
    from diffusionkit_amd import cli
    over = dict(mmdit_config=tiny_sd3(), vae_config=tiny_vae(), text_len=20)
    argv = ["--prompt", "a cat", "--model-version", "argmaxinc/mlx-stable-diffusion-3-medium", "--steps", "2", "--seed", "1", "--height", "64",
            "--width", "64", "--negative_prompt", "blurry"]
    for name, extra in (("vae", ["--vae-dtype", "float16"]), ("both", ["--vae-dtype", "float16", "--activation-dtype", "float16"])):
        out = tmp_path / f"{name}.png"
        img, log = cli.main(argv + ["-o", str(out)] + extra, pipeline_overrides=over)
        assert out.exists() and img.size == (64, 64) and len(log["denoising"]["iter_time"]) == 2


# ---- full size ---------------------------------------------------------------------------------------------------------------------------------
def test_vae_decode_1024_f16_vs_oracle(dev):
    """fullsize_vae_1024.npz: one decode of the 128 x 128 latent (-> 1024 x 1024) in fp16 against the fixture's fp32 oracle output, gated at half of
    what the bf16-emulating oracle reached (the fixture stores that reference as fp16: about 3e-4 of its own, far below the expected 2e-3)"""
    from diffusionkit_amd.engine import VAEDecoderEngine
    from tests import test_gpu_fullsize as fs
    f, c = fs.load("vae_1024"), fs.fx.VAE_1024
    c16 = float16_vae_config(c["cfg"])
    eng = VAEDecoderEngine(c16, pack_vae(c16, synth_vae_weights(c["cfg"], seed=c["seed_vae"]), dev))
    z = fs.fx.randn(1, c["latent"][0], c["latent"][1], 16, seed=c["z_seed"])
    img, u8, raw = eng.decode(z.to(dev), want_raw=True)
    ref_raw = torch.from_numpy(f["raw_fp32_f16"].astype(np.float32))
    e, e_bf = rel_l2(ref_raw, raw[..., :3].float().cpu()), float(f["emu_rel_l2"])
    p = psnr(torch.clip(ref_raw / 2 + 0.5, 0, 1), img.cpu())
    print(f"[f16 vae fullsize] vae_1024 raw: rel-L2 {e:.4e} (bf16-emulating oracle {e_bf:.4e}, gate {0.5 * e_bf:.4e}); image PSNR {p:.2f} dB "
          f"(bf16-emulating oracle {float(f['emu_psnr_image']):.2f} dB)")
    assert raw.dtype == F16 and img.shape == (1, 1024, 1024, 3)
    assert e <= 0.5 * e_bf
