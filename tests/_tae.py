"""The tiny latent decoder's float64 reference (plain torch conv2d), its fp32 restatement, units and case lists.  No GPU.

``rounded``: apply the kernels' bf16 rounding points (csrc/tae.hip) -- the clamped latent, every conv's ReLU(acc + bias), a Block's
ReLU(acc + bias + x), the image value, and image * 255 before the truncation to a byte."""
import torch
import torch.nn.functional as F

from diffusionkit_amd.config import TinyDecoderConfig
from tests._util import randn

BF = torch.bfloat16
TH = TW = 16  # the kernels' output tile (ops.TAE_TILE)
BLOCK_GRIDS = [(1, 1, 1), (1, 2, 3), (1, TH, TW), (2, TH + 1, TW - 1), (1, TH - 1, 2 * TW + 1), (1, 3 * TH, 5)]
CONV_GRIDS = [(1, 1, 1), (2, TH + 1, TW - 1), (1, 5, 2 * TW + 1)]
LATENTS = [(1, 2, 2), (2, 3, 5), (1, 16, 18)]
# C_BLOCK: twice the worst |fp32 restatement - ref64| / unit of a Block over BLOCK_GRIDS (both with the rounding points; the restatement accumulates in
# fp32 in torch's order).  Measured 1.93e-6 at (2, 17, 15) (test_tae_cpu.py::test_measured_constants prints it): an intermediate the two round to
# different neighbours moves a result by a bf16 spacing of the INTERMEDIATE times a weight; the unit, a product of three absolute convs, is ~2e4 times
# the result, so the gate is coarse -- the sharp statement about the fused kernel is its bit-identity with the chain of single convs.
C_BLOCK = 3.9e-6
# whole decoder: PSNR of the rounding-point reference against the exact one over LATENTS is >= 55.4 dB (55.47 at (1, 16, 18); the same test prints it); minus 3 dB
PSNR_MIN = 52.4


def latent(i):
    """the i-th latent of LATENTS: the input PSNR_MIN was measured on and the one the GPU test decodes"""
    return randn(*LATENTS[i], 16, seed=330 + i)


def rb(x, rounded=True):
    return x.to(BF).to(x.dtype) if rounded else x


def conv(x, w, b, dt=torch.float64, ups=False):
    """x [B, H, W, I], w [O, 3, 3, I], zero-padded by 1; accumulation in ``dt``"""
    if ups:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    y = F.conv2d(x.to(dt).permute(0, 3, 1, 2), w.to(dt).permute(0, 3, 1, 2), None if b is None else b.to(dt), padding=1)
    return y.permute(0, 2, 3, 1)


def block(x, ws, bs, rounded, dt=torch.float64, keep_out_of_image=False):
    """``keep_out_of_image``: the classic fault -- the intermediates are computed on a halo of 2 around the image from zero-padded input
    instead of being zero outside the image"""
    x = x.to(dt)
    if keep_out_of_image:
        xp = F.pad(x, (0, 0, 2, 2, 2, 2))
        h = rb(torch.relu(conv(xp, ws[0], bs[0], dt)), rounded)
        h = rb(torch.relu(conv(h, ws[1], bs[1], dt)), rounded)[:, 1:-1, 1:-1]
        return rb(torch.relu(conv(h, ws[2], bs[2], dt)[:, 1:-1, 1:-1] + x), rounded)
    h = rb(torch.relu(conv(x, ws[0], bs[0], dt)), rounded)
    h = rb(torch.relu(conv(h, ws[1], bs[1], dt)), rounded)
    return rb(torch.relu(conv(h, ws[2], bs[2], dt) + x), rounded)


def block_unit(x, ws, bs):
    """the same chain on absolute values, plus |x| for the skip"""
    u = x.double().abs()
    for w, b in zip(ws, bs):
        u = conv(u, w.abs(), b.abs())
    return u + x.double().abs()


def block_operands(grid, seed=0, positive=False):
    B, H, W = grid
    x = randn(B, H, W, 64, seed=300 + seed)
    ws = [randn(64, 3, 3, 64, seed=310 + seed + j, scale=(2.0 / 576) ** 0.5) for j in range(3)]
    bs = [randn(64, seed=320 + seed + j, scale=0.1) for j in range(3)]
    if positive:
        x, ws, bs = x.abs(), [w.abs() for w in ws], [b.abs() for b in bs]
    return x, ws, bs


def clamp_latent(lat, scale=1.0, shift=0.0, rounded=True):
    return rb(3.0 * torch.tanh((lat.double() - shift) * scale / 3.0), rounded)


def image_tail(pre, rounded=True):
    """(image f64, uint8) from the last conv's acc + bias"""
    img = rb(pre, rounded).clamp(0.0, 1.0)
    return img, rb(img * 255.0, rounded).to(torch.uint8)


def decode(lat, w, rounded, cfg=TinyDecoderConfig()):
    """w: reference-layout weights (weights.synth_tae_weights) -> (image f64 [B, 8h, 8w, 3], uint8)"""
    x, ups = clamp_latent(lat, rounded=rounded), False
    for i, kind in cfg.layers:
        if kind == "conv_in":
            x = rb(torch.relu(conv(x, w[f"{i}.weight"], w[f"{i}.bias"])), rounded)
        elif kind == "block":
            x = block(x, [w[f"{i}.conv.{j}.weight"] for j in (0, 2, 4)], [w[f"{i}.conv.{j}.bias"] for j in (0, 2, 4)], rounded)
        elif kind == "up":
            ups = True
        elif kind == "conv":
            x, ups = rb(conv(x, w[f"{i}.weight"], None, ups=ups), rounded), False
        else:
            return image_tail(conv(x, w[f"{i}.weight"], w[f"{i}.bias"]), rounded)
