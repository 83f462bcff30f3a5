"""The OCP MX-fp4 weight format on the host (diffusionkit_amd/weights.py): known answers of the quantiser, a float64 restatement, the packer's
round trip, and the path from the config to the packed names.  No GPU."""
import math
from dataclasses import replace

import pytest
import torch

from diffusionkit_amd.config import fp4_config, tiny_flux, tiny_sd3
from diffusionkit_amd.weights import (E2M1_GRID, dequantize_weight_mxfp4, pack_mmdit, pack_mxfp4, quantize_weight_mxfp4, synth_mmdit_weights,
                                      unpack_mxfp4)


def _row(values, k=128):
    """a one-row weight whose first block starts with `values` and whose row amax is exactly 6 (wscale = 1), in the SECOND block"""
    w = torch.zeros(1, k)
    w[0, :len(values)] = torch.tensor(values, dtype=torch.float32)
    w[0, 32] = 6.0
    return w


def _q(w):
    code, e8, ws = quantize_weight_mxfp4(w)
    return dequantize_weight_mxfp4(code, e8, ws), e8, ws


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_grid_points_and_ties(sign):
    grid = [sign * g for g in E2M1_GRID]
    dq, e8, ws = _q(_row(grid))
    assert float(ws[0]) == 1.0 and int(e8[0, 0]) == 127
    assert dq[0, :8].tolist() == [g + 0.0 for g in grid]  # every grid point survives
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    dq, e8, _ = _q(_row([sign * t for t in ties] + [6.0]))  # (the 6 pins the block scale at 2^0)
    assert int(e8[0, 0]) == 127
    assert dq[0, :7].tolist() == [sign * v + 0.0 for v in (0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0)]  # round to nearest EVEN code


@pytest.mark.parametrize("k", [-3, 0, 2])
def test_block_scale_boundaries(k):
    """block amax exactly 6 * 2^k takes the code of 2^k; the next fp32 above it the code of 2^(k + 1); the one below stays"""
    top = 6.0 * 2.0 ** k
    up, down = (float(torch.nextafter(torch.tensor(top), torch.tensor(s))) for s in (math.inf, 0.0))
    for amax, want in ((top, 127 + k), (up, 128 + k), (down, 127 + k)):
        w = _row([amax])
        w[0, 32] = 6.0 * 2.0 ** 3  # the row amax: wscale = 8, exact; the first block's amax / 8 is amax * 2^-3
        _, e8, ws = _q(w)
        assert float(ws[0]) == 8.0 and int(e8[0, 0]) == want - 3, (amax, int(e8[0, 0]))


def test_zero_blocks_and_rows():
    w = torch.zeros(3, 256)
    w[1, 40] = -0.3  # row 0 all zero, row 1 one value, row 2 all zero
    code, e8, ws = quantize_weight_mxfp4(w)
    assert ws.tolist() == [1.0, pytest.approx(0.05), 1.0]
    assert int(e8[0].max()) == 1 and int(e8[1, 0]) == 1 and int(code[0].max()) == 0  # zero blocks: the lowest code
    assert torch.equal(dequantize_weight_mxfp4(code, e8, ws) != 0, w != 0) and float(dequantize_weight_mxfp4(code, e8, ws)[1, 40]) == pytest.approx(-0.3)


def test_round_trip_equals_float64_restatement():
    torch.manual_seed(3)
    w = (torch.randn(64, 384) * 0.02 * torch.exp2(torch.randint(-6, 7, (64, 12)).float()).repeat_interleave(32, 1)).to(torch.bfloat16)
    got = dequantize_weight_mxfp4(*quantize_weight_mxfp4(w))
    # the format, restated in float64 with Python loops over blocks
    grid = torch.tensor(E2M1_GRID, dtype=torch.float64)
    want = torch.zeros(64, 384, dtype=torch.float64)
    wf = w.float()
    ws = (wf.abs().amax(1) / 6.0)  # fp32, as defined
    x = (wf / ws[:, None]).double()
    for n in range(64):
        for b in range(12):
            blk = x[n, 32 * b:32 * b + 32]
            e = -126
            while blk.abs().max() > 6.0 * 2.0 ** e:
                e += 1
            y = blk / 2.0 ** e
            d = (y.abs()[:, None] - grid[None, :]).abs()
            lo = d.argmin(1)
            tie = (lo < 7) & (d.gather(1, (lo + 1).clamp(max=7)[:, None])[:, 0] == d.gather(1, lo[:, None])[:, 0])
            idx = torch.where(tie & (lo % 2 == 1), lo + 1, lo)  # nearest; on a tie the even code
            want[n, 32 * b:32 * b + 32] = grid[idx] * y.sign() * 2.0 ** e * float(ws[n])
    assert torch.equal(got.double(), want.float().double())


def test_pack_unpack_is_the_identity():
    code = torch.randint(0, 16, (128, 384), dtype=torch.uint8)
    e8 = torch.randint(1, 255, (128, 12), dtype=torch.uint8)
    for pitch in (None, 192 + 64):
        w4, sw = pack_mxfp4(code, e8, pitch)
        assert w4.shape == (128, pitch or 192) and sw.numel() == 128 * 12
        c2, e2 = unpack_mxfp4(w4, sw, 384)
        assert torch.equal(c2, code) and torch.equal(e2, e8)
    # lane (r, q) of fragment f, K-tile t: 16 bytes at f * 16 * pitch + t * 1024 + (q * 16 + r) * 16, low nibble = the even K
    w4, sw = pack_mxfp4(code, e8)
    f, t, r, q = 3, 2, 5, 1
    lane = w4.reshape(-1)[f * 16 * 192 + t * 1024 + (q * 16 + r) * 16:][:16]
    ks = t * 128 + q * 32 + torch.arange(0, 32, 2)
    assert torch.equal(lane, code[16 * f + r, ks] | (code[16 * f + r, ks + 1] << 4))
    assert int(sw[((1 * 3 + t) * 64 + (q * 16 + r)) * 4 + 2]) == int(e8[64 + 32 + r, 4 * t + q])  # G = 1, nf = 2


def test_pack_mmdit_names_policy_and_refusals():
    cfg = replace(tiny_flux(depth_multimodal=2, depth_unified=1, heads=2), weight_dtype="mxfp4", fp8_bf16_double_blocks=1)
    w = synth_mmdit_weights(cfg, seed=1)
    p = pack_mmdit(cfg, w, "cpu")
    h, r = cfg.hidden_size, cfg.mlp_ratio
    b0, b1 = (f"multimodal_transformer_blocks.{i}.image_transformer_block.attn.qkv" for i in (0, 1))
    assert b0 + ".weight" in p and b0 + ".weight_fp4" not in p  # the policy keeps block 0 in bf16
    assert p[b1 + ".weight_fp4"].shape == (3 * h, h // 2) and p[b1 + ".wscale4"].numel() == 3 * h * h // 32 and p[b1 + ".wscale"].shape == (3 * h,)
    s0 = "unified_transformer_blocks.0.transformer_block"
    assert p[s0 + ".linear2.weight_fp4"].shape == (h, (1 + r) * h // 2)
    # linear2 is quantised as the concatenation [o_proj | fc2]: one wscale per row over both parts
    cat = torch.cat([w[s0 + ".attn.o_proj.weight"], w[s0 + ".mlp.fc2.weight"]], dim=1)
    code, e8, ws = quantize_weight_mxfp4(cat)
    assert torch.equal(p[s0 + ".linear2.wscale"], ws)
    assert all(torch.equal(a, b) for a, b in zip(unpack_mxfp4(p[s0 + ".linear2.weight_fp4"], p[s0 + ".linear2.wscale4"], (1 + r) * h), (code, e8)))
    assert fp4_config(tiny_flux(), "quality").weight_dtype == "mxfp4" and fp4_config(tiny_flux(), "speed").fp8_bf16_double_blocks == 0
    with pytest.raises(ValueError, match="head_dim 128"):
        fp4_config(tiny_sd3())  # head_dim 64
