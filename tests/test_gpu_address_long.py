"""Genuinely long operands on an MI355X: conv inputs on both sides of 2^31 bytes, a GroupNorm batch of more than 2^32 bytes, an engine batch whose
activation buffers pass 2^31 bytes ("Address-range guards").  A few seconds and at most ~11 GiB of device memory each; the inputs are drawn on the GPU in chunks (no float32 copy of a
whole operand exists), the fp64 references are computed on the CPU for windows cropped with their halo and for sampled groups."""
import pytest
import torch

from diffusionkit_amd import _lib
from tests import _bigmem as bm
from tests import _footprint as fp
from tests import _op_launches as L
from tests._util import TOL_SINGLE_OP, rel_l2

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HALO_TEXT = "conv_halo: shape / alignment not supported"


def draw(dev, shape, seed, scale=1.5, shift=0.3, rows=64):
    """bf16 N(shift, scale) of ``shape`` = (B, H, W, C) on the device, drawn 64 image rows at a time"""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.empty(shape, dtype=BF, device=dev)
    B, H, W, C = shape
    for b in range(B):
        for r in range(0, H, rows):
            n = min(rows, H - r)
            x[b, r:r + n] = (torch.randn(n, W, C, device=dev, generator=g) * scale + shift).to(BF)
    return x


def windows(H, W, row_bytes):
    """(r0, r1, c0, c1): the four corners, the pixel rows in which the byte offset of the input crosses 2^30 and reaches its end (2^31 for the larger
    shape: the last rows), and the last 16 x 16 tile"""
    ws = [(0, 4, 0, 4), (0, 4, W - 4, W), (H - 4, H, 0, 4), (H - 4, H, W - 4, W), (H - 16, H, W - 16, W)]
    for off in (2 ** 30, 2 ** 31 - 1):
        r = min(off // row_bytes, H - 1)
        ws.append((max(r - 1, 0), min(r + 2, H), W // 2 - 3, W // 2 + 3))
    return ws


def conv_window_error(x, w, b, y, img, ws, act=None, res=None):
    """worst rel_l2 of y[img] over the windows against the fp64 3 x 3 convolution of the input window cropped with its halo (``act``: the
    activation in front of the conv, per element; ``res``: the residual added behind it)"""
    from oracle import vae as ov
    from oracle.mmdit import Prec
    H, W = x.shape[1], x.shape[2]
    wd, bd, worst = w.double().cpu(), b.double().cpu(), 0.0
    for r0, r1, c0, c1 in ws:
        a, z, l, r = max(r0 - 1, 0), min(r1 + 1, H), max(c0 - 1, 0), min(c1 + 1, W)
        xin = x[img:img + 1, a:z, l:r].double().cpu()
        if act is not None:
            xin = act(xin)
        ref = ov.conv2d_nhwc(xin, wd, bd, Prec())[:, r0 - a:r0 - a + (r1 - r0), c0 - l:c0 - l + (c1 - c0)]
        if res is not None:
            ref = ref + res[img:img + 1, r0:r1, c0:c1].double().cpu()
        worst = max(worst, rel_l2(ref, y[img:img + 1, r0:r1, c0:c1].float()))
    return worst


@pytest.mark.parametrize("shape,kernel", [((1, 2048, 1008), 3), ((1, 2048, 1024), 128), ((2, 1024, 1008), 3), ((2, 1024, 1024), 128)],
                         ids=["one_image_below", "one_image_2_31", "batch_below", "batch_2_31"])
def test_conv3x3_input_on_both_sides_of_2_31_bytes(dev, shape, kernel):
    """gemm256v3.hip:704: C = 512, O = 256; 2048 x 1008 (2.11e9 bytes) stays on gemm256v3.hip's conv form, whose 31-bit offsets then reach the last
    rows; 2048 x 1024 is exactly 2^31 bytes and goes to the 128^2 kernel.  The same with two images of half the height: this guard counts the batch.
    Windows against fp64 at test_conv3x3_on_256_tile_kernel's TOL_SINGLE_OP"""
    from diffusionkit_amd import ops
    B, H, W = shape
    C, O = 512, 256
    bm.need_free(dev, 4 * 2 ** 30)
    assert ops.conv3x3_plan(B, H, W, C, O).kernel == kernel
    assert (B * H * W * C * 2 < 2 ** 31) == (kernel == 3)
    x = draw(dev, (B, H, W, C), seed=930)
    rnd = fp.rounder(BF)
    w, b = rnd(O, 3, 3, C, seed=931, scale=0.02).to(dev, BF), rnd(O, seed=932, scale=0.1).to(dev, BF)
    y = ops.conv3x3(x, w, b)
    torch.cuda.synchronize()
    for img in range(B):
        e = conv_window_error(x, w, b, y, img, windows(H, W, W * C * 2))
        print(f"[long] conv3x3 {shape} image {img}: kernel {kernel}, input {B * H * W * C * 2} bytes = 2^31 {B * H * W * C * 2 - 2 ** 31:+d}; "
              f"worst window vs fp64 rel_l2 {e:.3e} (< {TOL_SINGLE_OP})")
        assert e < TOL_SINGLE_OP
    print(f"[long] conv3x3 {shape}: peak device memory {torch.cuda.max_memory_allocated(dev) / 2 ** 30:.2f} GiB")


@pytest.mark.parametrize("v4", [0, 2], ids=["conv_halo", "conv256v4"])
def test_fused_conv_input_on_both_sides_of_2_31_bytes(dev, v4):
    """conv_halo.hip:525 / conv256v4.hip (through it): ONE image below 2^31 bytes, whatever the batch.  Two images of 2048 x 1008 x 512 (4.2e9 bytes:
    image 1 starts 33.5 MB below 2^31 and ends at 4 227 858 432, its last rows at offsets with bit 31 set) are accepted and image 1 is bit-identical to image 1 run alone; 2048 x 1024 is refused with the
    launcher's text (the VAE engine routes such a stage to the unfused convs instead: vae_engine.hip:160)"""
    from diffusionkit_amd import ops
    B, H, W, C, O, G = 2, 2048, 1008, 512, 256, 32
    bm.need_free(dev, 9 * 2 ** 30)
    torch.cuda.reset_peak_memory_stats(dev)
    x = draw(dev, (B, H, W, C), seed=940)
    rnd = fp.rounder(BF)
    w, b = rnd(O, 9 * C, seed=941, scale=0.02).to(dev, BF), rnd(O, seed=942, scale=0.1).to(dev, BF)
    tab = torch.stack([rnd(B, C, seed=943, scale=0.1, shift=1.0), rnd(B, C, seed=944, scale=0.1)], dim=1).to(dev)  # [B, 2, C] fp32 (scale | shift)

    def act(img):
        sc, sh = tab[img, 0].double().cpu(), tab[img, 1].double().cpu()

        def f(t):  # (rounded to bf16 behind the norm and behind the SiLU, as conv_halo.hip does and test_conv3x3_gn_halo's Prec(BF) oracle states)
            u = (t * sc + sh).to(BF).double()
            return (u * torch.sigmoid(u)).to(BF).double()
        return f
    with L.tuned(conv_v4=v4):
        y = ops.conv3x3_gn(x, w, b, gn_table=tab, silu=True)
        y1 = ops.conv3x3_gn(x[1:2], w, b, gn_table=tab[1:2], silu=True)
    torch.cuda.synchronize()
    assert torch.equal(y[1:2].view(torch.int16), y1.view(torch.int16)), "image 1 of the batch differs in its bits from image 1 run alone"
    w4 = w.reshape(O, 3, 3, C)
    for img in range(B):
        e = conv_window_error(x, w4, b, y, img, windows(H, W, W * C * 2), act=act(img))
        print(f"[long] conv3x3_gn conv_v4={v4} image {img} at byte {img * H * W * C * 2}: worst window vs fp64 rel_l2 {e:.3e} (< {TOL_SINGLE_OP}: "
              f"test_conv3x3_gn_halo / test_conv256v4_equals_conv_halo)")
        assert e < TOL_SINGLE_OP
    print(f"[long] conv3x3_gn conv_v4={v4}: peak device memory {torch.cuda.max_memory_allocated(dev) / 2 ** 30:.2f} GiB")
    del y, y1, x
    torch.cuda.empty_cache()
    big = torch.empty(1, 2048, 1024, C, dtype=BF, device=dev)  # (never read: the call is refused from its shape)
    with L.tuned(conv_v4=v4), pytest.raises(_lib.DkHipError, match=HALO_TEXT):
        ops.conv3x3_gn(big, w, b, gn_table=tab[:1], silu=True)


def test_groupnorm_batch_of_more_than_2_32_bytes(dev):
    """B = 5, 1024 x 1024, C = 512, G = 32: x spans 5 GiB, images 2 .. 4 start beyond 2^31 / 2^32.  ops.groupnorm, ops.groupnorm_table and
    ops.conv3x3_gn consuming the table (conv_halo.hip and conv256v4.hip): every image bit-identical to that image run alone; the image run alone
    against fp64 statistics of sampled groups at test_groupnorm's 3e-3 (the fused conv against fp64: the test above)"""
    from diffusionkit_amd import ops
    B, H, W, C, G = 5, 1024, 1024, 512, 32
    bm.need_free(dev, 11 * 2 ** 30)
    torch.cuda.reset_peak_memory_stats(dev)
    x = draw(dev, (B, H, W, C), seed=950, scale=2.0, shift=0.7)
    rnd = fp.rounder(BF)
    gamma, beta = rnd(C, seed=951, scale=0.1, shift=1.0).to(dev, BF), rnd(C, seed=952, scale=0.1).to(dev, BF)
    y = ops.groupnorm(x, gamma, beta, G, 1e-5, True)
    tab = ops.groupnorm_table(x, gamma, beta, G, 1e-5)
    cg = C // G
    for img in range(B):
        y1 = ops.groupnorm(x[img:img + 1], gamma, beta, G, 1e-5, True)
        t1 = ops.groupnorm_table(x[img:img + 1], gamma, beta, G, 1e-5)
        assert torch.equal(y[img:img + 1].view(torch.int16), y1.view(torch.int16)), f"groupnorm: image {img} of the batch differs from the image run alone"
        assert torch.equal(tab[img:img + 1].view(torch.int32), t1.view(torch.int32)), f"groupnorm_table: image {img} differs from the image run alone"
        worst = 0.0
        for g in (0, 13, G - 1):
            xg = x[img, :, :, g * cg:(g + 1) * cg].double()
            mu, var = xg.mean(), xg.var(unbiased=False)
            rows = slice(H - 8, H) if g else slice(0, 8)
            ga, be = gamma[g * cg:(g + 1) * cg].double(), beta[g * cg:(g + 1) * cg].double()
            u = (xg[rows] - mu) * torch.rsqrt(var + 1e-5) * ga + be
            worst = max(worst, rel_l2(u * torch.sigmoid(u), y1[0, rows, :, g * cg:(g + 1) * cg].float()))
            sc = torch.rsqrt(var + 1e-5) * ga
            worst = max(worst, rel_l2(torch.stack([sc, be - mu * sc]), t1[0, :, g * cg:(g + 1) * cg]))
        print(f"[long] groupnorm image {img} at byte {img * H * W * C * 2}: sampled groups vs fp64 rel_l2 {worst:.3e} (< 3e-3: test_groupnorm)")
        assert worst < 3e-3
        del y1, t1
    print(f"[long] groupnorm B=5: peak device memory {torch.cuda.max_memory_allocated(dev) / 2 ** 30:.2f} GiB")
    # conv3x3_gn consuming the batch's table: every image of the batch launch bit-identical to that image (and its table rows) run alone
    del y
    torch.cuda.empty_cache()
    O = 256
    w, b = rnd(O, 9 * C, seed=953, scale=0.02).to(dev, BF), rnd(O, seed=954, scale=0.1).to(dev, BF)
    for v4 in (0, 2):
        with L.tuned(conv_v4=v4):
            z = ops.conv3x3_gn(x, w, b, gn_table=tab, silu=True)
            for img in range(B):
                z1 = ops.conv3x3_gn(x[img:img + 1], w, b, gn_table=tab[img:img + 1], silu=True)
                assert torch.equal(z[img:img + 1].view(torch.int16), z1.view(torch.int16)), f"conv3x3_gn conv_v4={v4}: image {img} differs from the image run alone"
                assert bool(torch.isfinite(z1.float()).all())
        del z, z1
    print(f"[long] groupnorm + conv3x3_gn B=5: peak device memory {torch.cuda.max_memory_allocated(dev) / 2 ** 30:.2f} GiB")


def test_engine_batch_with_activation_buffers_beyond_2_31_bytes(dev):
    """FLUX width, 1 double + 1 single block, 512 x 512 images (64 x 64 latents: 1024 image + 256 text tokens, S = 1280), 2 Euler steps, as
    test_eight_seeds_one_step_loop_equal_single_runs -- with a batch sized from the block Linears' extents so that an activation buffer of each block
    kind passes 2^31 bytes: the double blocks' MLP hidden buffer of the image stream (B * 1024 rows x 12288 columns) and the single blocks'
    linear1 output / linear2 input (B * 1280 rows x 21504 / 15360 columns).  Distinct seeds per image; images 0, the middle one and the last two
    against single-image runs of the same seeds at that test's 4e-3"""
    from dataclasses import replace
    from diffusionkit_amd.pipeline import FluxPipeline
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    import os
    import sys
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if gold not in sys.path:
        sys.path.insert(0, gold)
    import make_fullsize_fixtures as fx  # (case definitions + seeded inputs, as tests/test_gpu_fullsize.py)
    cfg = replace(fx.FLUX_FULL["cfg"], depth_multimodal=1, depth_unified=1)
    h, S_i, S_t = cfg.hidden_size, 1024, 256
    assert h == 3072
    B = max(-(-(2 ** 31 + 1) // (S_i * 4 * h * 2)), -(-(2 ** 31 + 1) // ((S_i + S_t) * 5 * h * 2)))
    extents = {"double block, image fc1 output [B * 1024, 4 h]": B * S_i * 4 * h * 2, "single block, linear1 output [B * 1280, 7 h]": B * (S_i + S_t) * 7 * h * 2,
               "single block, linear2 input [B * 1280, 5 h]": B * (S_i + S_t) * 5 * h * 2, "joint q / k / v [B * 1280, 3 h]": B * (S_i + S_t) * 3 * h * 2}
    for what, n in extents.items():
        print(f"[long] engine batch {B}: {what}: {n} bytes = 2^31 {n - 2 ** 31:+d}")
    assert B == 86 and extents["double block, image fc1 output [B * 1024, 4 h]"] > 2 ** 31 and extents["single block, linear2 input [B * 1280, 5 h]"] > 2 ** 31
    bm.need_free(dev, 9 * 2 ** 30)  # (measured peak 8.62 GiB: weights, the batch's workspace, the latents)
    torch.cuda.reset_peak_memory_stats(dev)
    packed = {"mmdit": pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234), dev, consume=True)}
    pipe = FluxPipeline(w16=True, a16=True, device=dev, text_len=256, packed_weights=packed, mmdit_config=cfg)
    text, pooled = fx.flux_full_inputs()
    text, pooled = text.to(dev, BF), pooled.to(dev, BF)
    seeds = list(range(300, 300 + B))
    lat, _ = pipe.denoise_latents(text, pooled, num_steps=2, cfg_weight=0.0, latent_size=(64, 64), seed=seeds)
    assert lat.shape == (B, 64, 64, 16) and bool(torch.isfinite(lat).all())
    worst = 0.0
    for i in (0, B // 2, B - 2, B - 1):
        one, _ = pipe.denoise_latents(text, pooled, num_steps=2, cfg_weight=0.0, latent_size=(64, 64), seed=seeds[i])
        e = rel_l2(one[0].cpu(), lat[i].cpu())
        print(f"[long] engine batch {B}: image {i} against its single run: rel_l2 {e:.3e} (<= 4e-3: test_eight_seeds_one_step_loop_equal_single_runs)")
        worst = max(worst, e)
    print(f"[long] engine batch {B}: peak device memory {torch.cuda.max_memory_allocated(dev) / 2 ** 30:.2f} GiB")
    assert worst <= 4e-3
