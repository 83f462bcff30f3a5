"""fp8 path on ragged row counts: a last MX scale block of fewer than 128 rows (any image token count).

The fp8 GEMM reads the scales of a wave's 128 rows as one aligned block of the activation buffer, so every row range starts on a multiple of
128 physical rows -- but it may end anywhere: the DMA clamps to row M - 1 and the tail masks rows >= M.  What is checked here:
  * rows are independent: rows [0, M) of a launch over M rows are bit for bit those of the launch over the whole buffer (same tiles, same K order),
    rows >= M of the output are never written -- bf16 and MX-fp8 outputs, K split included;
  * the engine at image token counts of 120, 360 (two images: the second one's segment starts inside a block) and 195 against the oracle, at the
    gates of test_gpu_fp8.test_mmdit_fp8_tiny, through the lean attention kernel + quantiser pass and through attention4.hip's own MX-fp8 writer;
  * the MX-fp8 copy of the attention output at B * S = 2 * 488 rows.
Tolerances are those of tests/test_gpu_fp8.py.
"""
import math
from dataclasses import replace

import pytest
import torch

from diffusionkit_amd import ops
from diffusionkit_amd._lib import DK_EPI_BIAS, DK_EPI_BIAS_GELU, DK_EPI_GATE_RES
from diffusionkit_amd.config import tiny_flux, tiny_sd3
from diffusionkit_amd.weights import dequantize_weight_e4m3, quantize_weight_e4m3
from tests import _fp8 as f8
from tests._util import BF, TOL_SINGLE_OP, bf16r, psnr, randn, rel_l2

pytestmark = pytest.mark.gpu

ROWS, K = 384, 384
# 120: one partial block, the tile's second wave row owns nothing; 264: the second tile holds 8 rows; 360: the second tile's first block is
# partial; 376: not a multiple of 16
RAGGED_M = [120, 264, 360, 376]
SENTINEL = 7.0


@pytest.fixture(scope="module")
def act(dev):
    """x [384, K] quantised once: (e4m3 bytes, scale side array) on the device"""
    x = bf16r(randn(ROWS, K, seed=801, scale=1.0))
    x[:, :K // 2] *= 4.0
    return ops.quantize_mx8(x.to(dev, BF))


def _weight(N, Kw, seed, dev):
    qw, ws = quantize_weight_e4m3(randn(N, Kw, seed=seed, scale=0.02).to(BF))
    return qw.to(dev), ws.to(dev), dequantize_weight_e4m3(qw, ws)


@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("epi", ["bias", "gelu", "gate_res"])
def test_gemm_fp8_ragged_rows_are_independent_bf16(dev, act, N, epi):
    a8, sa = act
    w8, ws, _ = _weight(N, K, 802 + N, dev)
    bias = randn(N, seed=803, scale=0.5).to(dev, BF)
    res = randn(ROWS, N, seed=804).to(dev, BF)
    gate = randn(8, N, seed=805).to(dev, BF)  # (two segments of M / 2 rows inside [0, M); the whole-buffer run goes on through the next rows of the gate)
    for M in RAGGED_M:
        kw = dict(bias=bias, k=K)
        if epi == "gelu":
            kw.update(epilogue=DK_EPI_BIAS_GELU)
        elif epi == "gate_res":
            kw.update(epilogue=DK_EPI_GATE_RES, gate=gate, res=res, gate_seg_len=M // 2)
        else:
            kw.update(epilogue=DK_EPI_BIAS)
        whole = ops.gemm_fp8(a8, sa, w8, ws, M=ROWS, **kw)
        out = torch.full((ROWS + 8, N), SENTINEL, dtype=BF, device=dev)
        got = ops.gemm_fp8(a8, sa, w8, ws, M=M, out=out, **kw)
        assert got.data_ptr() == out.data_ptr()
        n_diff = int((out[:M].view(torch.int16) != whole[:M].view(torch.int16)).sum())
        print(f"[fp8 ragged bf16 {epi} N={N} M={M}] elements of rows [0, M) that differ from the M = {ROWS} launch: {n_diff}")
        assert n_diff == 0
        assert bool((out[M:] == SENTINEL).all()), "rows >= M were written"
        assert bool(torch.isfinite(whole.float()).all())


@pytest.mark.parametrize("N", [256, 512])
def test_gemm_fp8_ragged_mx8_output(dev, act, N):
    """fc1 + GELU -> MX-fp8 on M rows: bytes and scales of rows [0, M) are those of the whole-buffer launch, the data rows behind them keep their
    sentinel, and the result is the next GEMM's operand (gated as test_gemm_fp8_gelu_mx8_output_feeds_next_gemm)"""
    a8, sa = act
    w8, ws, _ = _weight(N, K, 812 + N, dev)
    bias = randn(N, seed=813, scale=0.5).to(dev, BF)
    w2_8, ws2, w2_dq = _weight(256, N, 814 + N, dev)
    kw = dict(bias=bias, epilogue=DK_EPI_BIAS_GELU, k=K, out_mx8=True)
    whole_q, whole_s = ops.gemm_fp8(a8, sa, w8, ws, M=ROWS, **kw)
    whole_e = f8.array_to_scales(whole_s, ROWS, N)
    for M in RAGGED_M:
        buf = torch.full((ROWS, N), 0xAB, dtype=torch.uint8, device=dev)
        sc = torch.zeros(ops.mx_scale_bytes(ROWS, N), dtype=torch.uint8, device=dev)
        ops.gemm_fp8(a8, sa, w8, ws, M=M, out=buf, out_scales=sc, **kw)
        got_e = f8.array_to_scales(sc, M, N, rows=ROWS)
        n_q, n_e = int((buf[:M] != whole_q[:M]).sum()), int((got_e != whole_e[:M]).sum())
        print(f"[fp8 ragged mx8 N={N} M={M}] bytes that differ from the M = {ROWS} launch: {n_q}, scales: {n_e}")
        assert n_q == 0 and n_e == 0
        assert bool((buf[M:] == 0xAB).all()), "data rows >= M were written"
        hid = f8.mx8_decode(buf[:M], got_e)
        assert bool(torch.isfinite(hid).all())
        out = ops.gemm_fp8(buf, sc, w2_8, ws2, M=M)
        r = rel_l2(hid @ w2_dq.t(), out.float().cpu())
        print(f"[fp8 ragged mx8 N={N} M={M}] next GEMM on the written rows: rel_l2 {r:.3e} (< {TOL_SINGLE_OP})")
        assert out.shape == (M, 256) and r < TOL_SINGLE_OP


def test_gemm_fp8_ragged_launch_is_split_along_k(dev):
    """(1208, 3072, 12288): 60 tiles, the last row of tiles holds 184 rows -- cut along K like FLUX's fc2 at 512 x 512 (gates of
    test_gemm_fp8_small_launch_is_split_automatically)"""
    from oracle import fp8 as o8
    M, N, Kb = 1208, 3072, 12288
    a = bf16r(randn(M, Kb, seed=821, scale=1.0))
    a[:, :Kb // 2] *= 4.0
    qa, ea = o8.mx8_encode(a)
    qw, ws = quantize_weight_e4m3(randn(N, Kb, seed=822, scale=0.02).to(BF))
    a_dq, w_dq = f8.mx8_decode(qa, ea), dequantize_weight_e4m3(qw, ws)
    wp = torch.zeros(N, Kb + 128, dtype=torch.uint8)
    wp[:, :Kb] = qw
    bias, gate, res = randn(N, seed=5, scale=0.5), randn(1, N, seed=6), randn(M, N, seed=7)
    rows = (M + 127) // 128 * 128
    a8 = torch.zeros(rows, Kb, dtype=torch.uint8)
    a8[:M] = qa
    wsp = ops.gemm_workspace(dev)
    args = (a8.to(dev), f8.scales_to_array(ea, rows).to(dev), wp.to(dev), ws.to(dev))
    kw = dict(bias=bias.to(dev, BF), epilogue=DK_EPI_GATE_RES, gate=gate.to(dev, BF), res=res.to(dev, BF), gate_seg_len=M, M=M, k=Kb)
    y = ops.gemm_fp8(*args, workspace=wsp, **kw)
    y0 = ops.gemm_fp8(*args, **kw)
    ref = res + bf16r(gate * bf16r(a_dq @ w_dq.t() + bias))
    r, r0 = rel_l2(ref, y.float()), rel_l2(ref, y0.float())
    print(f"[fp8 ragged K split] rel_l2 with the workspace {r:.3e}, without {r0:.3e} (< {TOL_SINGLE_OP})")
    assert r < TOL_SINGLE_OP and r0 < TOL_SINGLE_OP
    assert not torch.equal(y0, y), "the launch was expected to be cut along K (other summation order)"
    assert float((y0.float() != y.float()).float().mean()) < 0.05
    assert int(wsp[-4096:].sum()) == 0  # the flag region (and the error word) is left zero


def _engine_gates(dev, cfg, B, Hl, Wl, S_t, tag):
    from tests.test_gpu_fp8 import _fp8_forward_case
    out, res = _fp8_forward_case(cfg, dev, B, Hl, Wl, S_t, [1000.0, 752.0, 500.0], 1)
    e_h, e_e = rel_l2(res["fq_fp32"], out), rel_l2(res["fq_fp32"], res["fq_emu"])
    p_fq, p_un, p_emu = psnr(res["fq_fp32"], out), psnr(res["fp32"], out), psnr(res["fp32"], res["fq_emu"])
    print(f"[fp8 ragged engine {tag}] hip-vs-fq {e_h:.3e}, emu-vs-fq {e_e:.3e} (gate {2.0 * e_e + 2e-3:.3e}); PSNR vs fake-quant fp32 oracle {p_fq:.1f} dB "
          f"(> 35), vs un-quantised {p_un:.1f} dB (bf16-emulating fake-quant oracle {p_emu:.1f} dB)")
    assert bool(torch.isfinite(out).all())
    assert e_h <= 2.0 * e_e + 2e-3, (e_h, e_e)
    assert p_fq > 35.0
    assert p_un > p_emu - 3.0


# (B, latent h, latent w, text length): 120 image tokens -- less than one block; 2 x 360 -- the second image's rows start inside a block; 195 -- odd
ENGINE_CASES = [(1, 24, 20, 128), (2, 40, 36, 128), (1, 30, 26, 128)]


@pytest.mark.parametrize("B,Hl,Wl,S_t", ENGINE_CASES)
def test_mmdit_fp8_ragged_image_tokens(dev, B, Hl, Wl, S_t):
    cfg = replace(tiny_flux(depth_multimodal=2, depth_unified=2, heads=2), weight_dtype="fp8_e4m3")
    _engine_gates(dev, cfg, B, Hl, Wl, S_t, f"B={B} S_i={(Hl // 2) * (Wl // 2)}")


def test_mmdit_fp8_ragged_precision_policy(dev):
    """the first double block on the bf16 path, the second one and the single blocks in fp8, two images of 360 tokens"""
    cfg = replace(tiny_flux(depth_multimodal=2, depth_unified=2, heads=2), weight_dtype="fp8_e4m3", fp8_bf16_double_blocks=1)
    _engine_gates(dev, cfg, 2, 40, 36, 128, "B=2 S_i=360, first double block bf16")


def test_mmdit_fp8_ragged_long_sequence_route(dev):
    """attention4.hip (what long ragged sequences run) writes the MX-fp8 copy from its accumulators: forced at the small size"""
    cfg = replace(tiny_flux(depth_multimodal=2, depth_unified=2, heads=2), weight_dtype="fp8_e4m3")
    try:
        ops.tune("attn", 9)
        _engine_gates(dev, cfg, 2, 40, 36, 128, "B=2 S_i=360, attn mode 9")
    finally:
        ops.tune("attn", -1)


@pytest.mark.parametrize("mode", [4, 9])
def test_attention_mx8_copy_ragged_rows(dev, mode):
    """B * S = 2 * 488 rows (no multiple of 128; the second image starts inside a scale block): O8 is exactly ops.quantize_mx8 of the bf16 output --
    of the same launch for the lean kernel (mode 4), of a second launch without O8 for attention4.hip (mode 9: it writes O8 instead of O)"""
    B, H, S, D = 2, 2, 488, 128
    h, M = H * D, B * S
    qkv = randn(B, S, 3 * h, seed=830).to(dev, BF)
    base = qkv.data_ptr()
    kw = dict(q=base, k=base + 2 * h, v=base + 4 * h, B=B, H=H, S=S, D=D, ld=3 * h, ldo=h, scale=1.0 / math.sqrt(D))
    out = torch.full((B, S, h), SENTINEL, dtype=BF, device=dev)
    plain = torch.full((B, S, h), SENTINEL, dtype=BF, device=dev)
    rows8 = M + 5
    o8b = torch.full((rows8, h), 0xAB, dtype=torch.uint8, device=dev)
    sc = torch.zeros(ops.mx_scale_bytes(rows8, h), dtype=torch.uint8, device=dev)
    try:
        ops.tune("attn", mode)
        ops.attention_desc_call(out=out, O8=o8b, O8_scales=sc, o8_ld=h, o8_rows=rows8, **kw)
        if mode == 9:
            ops.attention_desc_call(out=plain, **kw)
    finally:
        ops.tune("attn", -1)
    y = (plain if mode == 9 else out).reshape(M, h)
    assert not bool((y == SENTINEL).all())
    want_q, want_s = ops.quantize_mx8(y)
    want_e, got_e = f8.array_to_scales(want_s, M, h), f8.array_to_scales(sc, M, h, rows=rows8)
    n_q, n_e = int((o8b[:M] != want_q).sum()), int((got_e != want_e).sum())
    print(f"[attn o8 ragged mode {mode}] bytes that differ from quantize_mx8 of the bf16 output: {n_q} of {want_q.numel()}, scales: {n_e} of {want_e.numel()}")
    assert n_q == 0 and n_e == 0
    assert bool((o8b[M:] == 0xAB).all()), "rows behind B * S were written"
    if mode == 9:
        assert bool((out == SENTINEL).all()), "O written although the kernel owns the MX-fp8 copy"


def _splits(n, nb):
    """chained splits of [0, n): in two at every interior boundary (the policy boundary nb among them) and into single blocks"""
    out = [[(0, k), (k, n - k)] for k in range(1, n)]
    out.append([(i, 1) for i in range(n)])
    assert nb == 0 or [(0, nb), (nb, n - nb)] in out
    return out


_T22 = tiny_flux(depth_multimodal=2, depth_unified=2, heads=2)
# (config, B, latent h, latent w, text length): fp8 with the first double block in bf16 at aligned and at ragged (2 x 360) image token counts, the
# bf16 path of FLUX, and SD3 (its last double block skips the text stream's post-attention half)
COMPOSE_CASES = [(replace(_T22, weight_dtype="fp8_e4m3", fp8_bf16_double_blocks=1), 1, 32, 32, 128),
                 (replace(_T22, weight_dtype="fp8_e4m3", fp8_bf16_double_blocks=1), 2, 40, 36, 128),
                 (_T22, 2, 8, 8, 16),
                 (tiny_sd3(), 2, 8, 8, 16)]


@pytest.mark.parametrize("cfg,B,Hl,Wl,S_t", COMPOSE_CASES, ids=["fp8-policy", "fp8-policy-ragged", "flux-bf16", "sd3-bf16"])
def test_block_ranges_compose(dev, cfg, B, Hl, Wl, S_t):
    """run_blocks over [0, n) is bit for bit every chain of run_blocks over the parts of a split of [0, n): a block's launches do not depend on
    the range it is issued in, on either side of the precision-policy boundary or across it"""
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    eng = MMDiTEngine(cfg, pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234), dev))
    eng.prepare(B, (Hl, Wl), S_t, 3)
    eng.cache_modulation_params(randn(B, cfg.pooled_text_embed_dim, seed=4).to(dev), [1000.0, 752.0, 500.0])
    n = cfg.depth_multimodal + cfg.depth_unified
    nb = cfg.fp8_bf16_double_blocks if cfg.weight_dtype == "fp8_e4m3" else 0
    S = S_t + (Hl // cfg.patch_size) * (Wl // cfg.patch_size)
    x = randn(B, S, cfg.hidden_size, seed=840).to(dev, BF)
    whole = eng.run_blocks(x, 1, 0, n)
    assert bool(torch.isfinite(whole.float()).all()) and not torch.equal(whole, x)
    for split in _splits(n, nb):
        y = x
        for first, count in split:
            y = eng.run_blocks(y, 1, first, count)
        assert torch.equal(y, whole), f"blocks [0, {n}) differ from the chain {split}"
