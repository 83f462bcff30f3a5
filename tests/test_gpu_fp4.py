"""MX-fp4 weights (W4A8): the block-scaled fp4 x fp8 GEMM (csrc/gemm256f4.hip) and the MMDiT engine on it.

Gates: a single GEMM against the float64 product of the dequantised operands differs from exact only by the final bf16 rounding (~1e-3):
rel-L2 < TOL_SINGLE_OP, the project's gate for every single GEMM.  The tail's other forms take the gates of the fp8 tests of the same form
(tests/test_gpu_fp8.py).  Beside every rel-L2 of a GEMM output stands the per-element gate of tests/_gates.py (G.qgemm_gate, G.mx8_gate), proved
on mutants in tests/test_gate_power_cpu.py::test_qgemm_gate.  Every bias-only shape is also launched with a gate row and a residual in the tail
on the same operands, where the gate holds on this kernel; on the bias-only, GELU and MX-fp8 outputs the kernel leaves the bound at a few
elements (tests/test_gpu_fp8.py says where and by how much) and those forms print their figure without asserting it (``missed``).
Engine: e_h <= 2 e_e + 2e-3 against the oracle on the same fake-quantised values; what fp4 costs against the un-quantised oracle is printed, not
gated (random weights say nothing about a checkpoint)."""
from dataclasses import replace

import pytest
import torch

from diffusionkit_amd import ops
from diffusionkit_amd._lib import DK_EPI_BIAS, DK_EPI_BIAS_GELU, DK_EPI_GATE_RES
from oracle import fp8 as o8
from oracle.mmdit import OracleMMDiT, Prec, gelu_erf
from tests import _fp8 as f8
from tests import _gates as G
from tests import _mxfp4 as f4
from tests._util import BF, TOL_SINGLE_OP, bf16r, psnr, randn, rel_l2

pytestmark = pytest.mark.gpu


# one tile and one K-tile (prologue only); two K-tiles (the ON2 = false iterations); three (first steady-state iteration, partial second row tile);
# five (the three-slot weight ring wraps; last 128-row scale block partial); a single row; a pitched weight (dk_weight_pitch_fp4(K) != K / 2);
# a single row over two column tiles and 257 rows over three: all four `wn` waves, both weight pieces `wave` and `wave + 8`, column tiles 1 and 2
@pytest.mark.parametrize("M,N,K,w_pitch", [(256, 256, 128, None), (512, 512, 256, None), (384, 256, 384, None), (130, 256, 640, None), (1, 256, 128, None),
                                           (200, 256, 512, 512 // 2 + 64), (1, 512, 128, None), (257, 768, 384, None)])
def test_gemm_fp4_bias(dev, M, N, K, w_pitch):
    p = f8.GemmProblem("fp4", dev, M, N, K, w_pitch)
    y = p.run()
    r = rel_l2(p.ref, y)
    print(f"[fp4 gemm {M}x{N}x{K}] rel_l2 {r:.3e}")
    assert r < TOL_SINGLE_OP, r
    p.gate_bias("", y, missed=M > 1)
    p.gate_res("", p.run_res())


def test_gemm_fp4_k_split(dev):
    """(300, 768, 3072): 6 tiles of 24 K-tiles -- the shared K-split rule (dk_plan_split) cuts every tile in four once the workspace is there.  (The
    rule's break-even for an all-remainder Linear is 32 saved K-tile steps and this launch saves 18, so the test lowers the `gemm_split_min` knob for
    its launch: the protocol under test is the kernel's, not the break-even.)  Split and unsplit are both inside the gate and differ only by the fp32
    summation order."""
    p = f8.GemmProblem("fp4", dev, 300, 768, 3072)
    y, y0 = p.k_split(p.run, 8, False)
    assert rel_l2(p.ref, y) < TOL_SINGLE_OP and rel_l2(p.ref, y0) < TOL_SINGLE_OP, (rel_l2(p.ref, y), rel_l2(p.ref, y0))
    p.gate_bias("cut and whole", [y, y0], missed=False)
    p.gate_res("cut and whole", list(p.k_split(p.run_res, 8, False)))


@pytest.mark.parametrize("M,N,K,w_pitch", [(300, 768, 1664, None), (200, 256, 1024, 1024 // 2 + 64)])
def test_gemm_fp4_k_split_short_reductions(dev, M, N, K, w_pitch):
    """13 K-tiles (finisher 4, producers 3 + 3 + 3), and 8 K-tiles (2 + 2 + 2 + 2) with a pitched weight: the K-tile offsets of the pieces (k0 * 1024
    into a fragment row, k0 * sa_step and k0 * 256 into the scale arrays) at ranges the long shapes do not produce.  The shared rule would leave
    launches this short whole (9 and 6 saved K-tile steps), so `gemm_split` is forced beside the lowered `gemm_split_min`.  The fp8 kernel's:
    tests/test_gpu_fp8.py::test_gemm_fp8_k_split_short_reduction."""
    p = f8.GemmProblem("fp4", dev, M, N, K, w_pitch)
    y, y0 = p.k_split(p.run, 0, True)
    print(f"[fp4 K split {M}x{N}x{K}] rel_l2 cut {rel_l2(p.ref, y):.3e}, whole {rel_l2(p.ref, y0):.3e}; elements that differ {int((y0 != y).sum())}")
    assert rel_l2(p.ref, y) < TOL_SINGLE_OP and rel_l2(p.ref, y0) < TOL_SINGLE_OP
    p.gate_bias("cut and whole", [y, y0], missed=w_pitch is not None)
    p.gate_res("cut and whole", list(p.k_split(p.run_res, 0, True)))


def _block_scale_pattern(dev, K):
    M, N = 256, 256
    w = randn(N, K, seed=77, scale=0.02)
    kb, n = torch.arange(K)[None, :] // 32, torch.arange(N)[:, None]
    w = (w * torch.exp2(((kb * 5 + n * 3) % 17 - 8).float())).to(BF)
    p = f8.GemmProblem("fp4", dev, M, N, K, w=w)
    y = p.run()
    assert rel_l2(p.ref, y) < TOL_SINGLE_OP
    p.gate_bias("block pattern", y, missed=True)
    p.gate_res("block pattern", p.run_res())


def test_gemm_fp4_block_scales_are_applied_per_block(dev):
    """K blocks that differ by 2^+-8 along one row and across the rows of one 16-channel fragment: a wrong opsel or scale layout fails here and passes
    on a unit-scale weight"""
    _block_scale_pattern(dev, 256)


def test_gemm_fp4_block_scales_when_the_ring_wraps(dev):
    """the same pattern over five K-tiles: the three-slot weight ring wraps and the scale loads of K-tiles 3 and 4 follow it"""
    _block_scale_pattern(dev, 640)


def _desc(dev, qa, ea, w4, sw, ws, bias, M, N, K, a_row0=0):
    keep = dict(a8=qa.to(dev), sa=f8.scales_to_array(ea).to(dev), w4=w4.to(dev), sw=sw.to(dev), ws=ws.to(dev), bias=bias.to(dev, BF))
    d = dict(A=keep["a8"].data_ptr() + a_row0 * K, A_scales=keep["sa"], W=keep["w4"], w_scale=keep["ws"], bias=keep["bias"], M=M, N=N, K=K,
             lda=K, ldw=w4.shape[1], a_row0=a_row0, a_rows=qa.shape[0], epilogue=DK_EPI_BIAS)
    return d, keep


# (B, S_t, S_i) of the grouped pair: the fp8 test's; text rows from activation row 384 (a multiple of 128, not of 256); a text stream of one row
PAIRS = {"grouped_pair": (2, 128, 384), "grouped_pair_a_row0_384": (2, 128, 192), "grouped_pair_text_m1": (1, 1, 384)}


@pytest.mark.parametrize("form", ["gate_res", "gelu_mx8_chain", "column_split"] + list(PAIRS))
def test_gemm_fp4_tail_forms(dev, form):
    """the shared tail's other forms through this kernel, each against the reference and at the gate of the fp8 test of the same form"""
    if form == "gate_res":
        M, N, K, S = 512, 256, 256, 256
        qa, ea, w4, sw, ws, w_dq, a_dq = f4.fp4_problem(M, N, K, seed=21)
        bias, gate, res = randn(N, seed=5, scale=0.5), randn(M // S, N, seed=6), randn(M, N, seed=7)
        out = ops.gemm_fp4(qa.to(dev), f8.scales_to_array(ea).to(dev), w4.to(dev), sw.to(dev), ws.to(dev), bias=bias.to(dev, BF),
                           epilogue=DK_EPI_GATE_RES, gate=gate.to(dev, BF), res=res.to(dev, BF), gate_seg_len=S)
        ref = res + bf16r(gate.repeat_interleave(S, 0) * bf16r(a_dq @ w_dq.t() + bias))
        assert rel_l2(ref, out.float().cpu()) < TOL_SINGLE_OP
        G.assert_gate("fp4 gate_res", G.qgemm_gate(out, a_dq, w_dq, bias, "gate_res", res, gate.repeat_interleave(S, 0)))
    elif form == "gelu_mx8_chain":  # fc1 -> GELU -> MX-fp8 (written by the tail) -> fc2
        M, h, r = 512, 256, 4
        qa, ea, w4, sw, ws, w1_dq, a_dq = f4.fp4_problem(M, r * h, h, seed=31)
        b1 = randn(r * h, seed=8, scale=0.5)
        hq, hs = ops.gemm_fp4(qa.to(dev), f8.scales_to_array(ea).to(dev), w4.to(dev), sw.to(dev), ws.to(dev), bias=b1.to(dev, BF),
                              epilogue=DK_EPI_BIAS_GELU, out_mx8=True)
        want_q, want_e = o8.mx8_encode(gelu_erf(bf16r(a_dq @ w1_dq.t() + b1), Prec(BF)))
        got = f8.mx8_decode(hq.cpu(), f8.array_to_scales(hs.cpu(), M, r * h))
        assert rel_l2(f8.mx8_decode(want_q, want_e), got) < 6e-3
        G.assert_gate("fp4 gelu -> MX-fp8", G.mx8_gate(got, a_dq, w1_dq, b1))
        w24, sw2, ws2, w2_dq = f4.weight_operands(randn(h, r * h, seed=33, scale=0.02).to(BF))
        out = ops.gemm_fp4(hq, hs, w24.to(dev), sw2.to(dev), ws2.to(dev))
        assert rel_l2(got @ w2_dq.t(), out.float().cpu()) < TOL_SINGLE_OP  # on the hidden values the kernel itself produced
        G.assert_gate("fp4 fc2 on the MX-fp8 hidden values", G.qgemm_gate(out, got, w2_dq, None), missed=True)
    elif form == "column_split":  # [q | k | v] + bias -> bf16, gelu(fc1 + bias) -> MX-fp8 into a column window of a wider buffer
        M, K, n1, n2, col0, ld8 = 512, 256, 768, 1024, 128, 128 + 1024 + 64
        qa, ea, w4, sw, ws, w_dq, a_dq = f4.fp4_problem(M, n1 + n2, K, seed=41)
        bias = randn(n1 + n2, seed=42, scale=0.5)
        d, keep = _desc(dev, qa, ea, w4, sw, ws, bias, M, n1 + n2, K)
        out = torch.full((M + 8, n1), 7.0, dtype=BF, device=dev)
        buf8 = torch.full((M, ld8), 0xAB, dtype=torch.uint8, device=dev)
        sc = torch.zeros(ops.mx_scale_bytes(M, ld8), dtype=torch.uint8, device=dev)
        d.update(C=out, ldc=n1, C_scales=sc, c_rows=M, c_row0=0, c_col0=col0)
        ops.gemm_fp4_fused_call(d, dict(n_split=n1, C2=buf8.data_ptr() + col0, ldc2=ld8, epi2=DK_EPI_BIAS_GELU, c2_mx8=1), keep["sw"])
        acc = a_dq @ w_dq.t() + bias
        assert rel_l2(acc[:, :n1], out[:M].float().cpu()) < TOL_SINGLE_OP and bool((out[M:] == 7.0).all())
        G.assert_gate("fp4 column split, bf16 half", G.qgemm_gate(out[:M], a_dq, w_dq[:n1], bias[:n1]), missed=True)
        want_q, want_e = o8.mx8_encode(gelu_erf(bf16r(acc[:, n1:]), Prec(BF)))
        got = f8.mx8_decode(buf8[:, col0:col0 + n2].cpu(), f8.array_to_scales(sc.cpu(), M, n2, rows=M, col0=col0))
        assert rel_l2(f8.mx8_decode(want_q, want_e), got) < 6e-3
        G.assert_gate("fp4 column split, MX-fp8 half", G.mx8_gate(got, a_dq, w_dq[n1:], bias[n1:]))
        assert bool((buf8[:, :col0] == 0xAB).all()) and bool((buf8[:, col0 + n2:] == 0xAB).all())
    else:  # image rows and text rows of one activation buffer in one launch, gate + residual in place in a joint [B, S_t + S_i, N] buffer
        (B, S_t, S_i), N, K = PAIRS[form], 512, 256
        Mi, Mt, S = B * S_i, B * S_t, S_t + S_i
        qa, ea, _, _, _, _, a_dq = f4.fp4_problem(Mi + Mt, N, K, seed=51)
        X = randn(B * S + 8, N, seed=60)
        Xd = X.to(dev, BF)
        probs, descs, keeps = [], [], []
        for seed, row0, M, c_row0, seg in ((52, 0, Mi, S_t, S_i), (54, Mi, Mt, 0, S_t)):
            w4, sw, ws, w_dq = f4.weight_operands(randn(N, K, seed=seed, scale=0.03).to(BF))
            bias, gate = randn(N, seed=seed + 1, scale=0.5), randn(B, N, seed=seed + 10)
            d, keep = _desc(dev, qa, ea, w4, sw, ws, bias, M, N, K, a_row0=row0)
            keep["gate"] = gate.to(dev, BF)
            d.update(C=Xd.data_ptr() + c_row0 * N * 2, ldc=N, c_seg_len=seg, c_seg_stride=S, epilogue=DK_EPI_GATE_RES, ldr=N, r_seg_len=seg,
                     r_seg_stride=S, gate=keep["gate"], gate_seg_len=seg, gate_stride=N)
            d["res"] = d["C"]
            probs.append((w_dq, bias, gate, row0, M, c_row0, seg))
            descs.append(d)
            keeps.append(keep)
        ops.gemm_fp4_fused_call(descs[0], None, keeps[0]["sw"], descs[1], None, keeps[1]["sw"])
        got = Xd.float().cpu()
        for w_dq, bias, gate, row0, M, c_row0, seg in probs:
            m = torch.arange(M)
            rows = c_row0 + (m // seg) * S + m % seg
            ref = X[rows] + bf16r(gate.repeat_interleave(seg, 0) * bf16r(a_dq[row0:row0 + M] @ w_dq.t() + bias))
            assert rel_l2(ref, got[rows]) < TOL_SINGLE_OP
            G.assert_gate(f"fp4 {form}, activation row {row0}", G.qgemm_gate(got[rows], a_dq[row0:row0 + M], w_dq, bias, "gate_res", X[rows],
                                                                           gate.repeat_interleave(seg, 0)))
        assert torch.equal(got[B * S:], bf16r(X[B * S:]))


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------------
def _fp4_forward_case(cfg, dev, B):
    """tests/test_gpu_fp8.py::_fp8_forward_case on the MX-fp4 engine: one forward step against OracleMMDiT on the fp4-dequantised block weights
    with MX-fp8 activation fake-quantisation (the precision policy's bf16 blocks see neither)"""
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    Hl, Wl, S_t, ts, step = 32, 32, 128, [1000.0, 752.0, 500.0], 1
    named = synth_mmdit_weights(cfg, seed=1234)
    packed = pack_mmdit(cfg, named, dev)
    eng = MMDiTEngine(cfg, packed)
    text, pooled, lat = randn(B, S_t, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, Hl, Wl, 16, seed=5)
    eng.prepare(B, (Hl, Wl), S_t, len(ts))
    eng.cache_modulation_params(pooled.to(dev), ts)
    out = eng.forward_tokens(eng.patchify(lat.to(dev)), text.to(dev, BF), step).float().cpu()
    res = {}
    fq, plain, paq = f4.fake_quant_block_weights(cfg, named), {k: v.float() for k, v in named.items()}, o8.policy_act_quant(cfg)
    for name, w, P, aq in (("fq_emu", fq, Prec(BF), paq), ("fq_fp32", fq, Prec(), paq), ("fp32", plain, Prec(), None)):
        m = OracleMMDiT(cfg, w, P, act_quant=aq)
        m.cache_modulation_params(pooled, torch.tensor(ts))
        taps = {}
        m(lat, text, ts[step], taps=taps)
        res[name] = taps["final"]
    return out, res, packed


@pytest.mark.parametrize("B,n_bf16", [(1, 0), (2, 0), (1, 1)])
def test_mmdit_fp4_tiny(dev, B, n_bf16):
    from diffusionkit_amd.config import tiny_flux
    cfg = replace(tiny_flux(depth_multimodal=2, depth_unified=2, heads=2), weight_dtype="mxfp4", fp8_bf16_double_blocks=n_bf16)
    out, res, packed = _fp4_forward_case(cfg, dev, B)
    b0 = "multimodal_transformer_blocks.0.image_transformer_block.attn.qkv"
    assert (b0 + ".weight" in packed) == (n_bf16 == 1) and (b0 + ".weight_fp4" in packed) == (n_bf16 == 0)
    e_h, e_e = rel_l2(res["fq_fp32"], out), rel_l2(res["fq_fp32"], res["fq_emu"])
    print(f"fp4 tiny B={B}, bf16 double blocks {n_bf16}: e_h {e_h:.3e}, e_e {e_e:.3e}; PSNR vs the un-quantised fp32 oracle {psnr(res['fp32'], out):.1f} dB "
          f"(fake-quant oracle in fp32 arithmetic {psnr(res['fp32'], res['fq_fp32']):.1f} dB) -- reported, not gated")
    assert e_h <= 2.0 * e_e + 2e-3, (e_h, e_e)


def test_pipeline_fp4_generates(dev):
    """generate_image through FluxPipeline(mmdit_config=fp4_config(...)) on synthetic weights: runs, is deterministic, and is not the fp8 engine's image"""
    import numpy as np
    from diffusionkit_amd.config import fp4_config, fp8_config, tiny_flux, tiny_vae, tiny_vae_encoder
    from diffusionkit_amd.pipeline import FluxPipeline
    imgs = []
    for cfg in (fp4_config(tiny_flux(), "speed"), fp8_config(tiny_flux(), "speed")):
        pipe = FluxPipeline(w16=True, a16=True, mmdit_config=cfg, vae_config=tiny_vae(), vae_encoder_config=tiny_vae_encoder(), device=dev, text_len=128)
        runs = [np.asarray(pipe.generate_image("a cat", num_steps=2, latent_size=(8, 8), seed=0, verbose=False)[0]) for _ in range(2)]
        assert runs[0].shape == (64, 64, 3) and np.array_equal(runs[0], runs[1])
        imgs.append(runs[0])
    assert not np.array_equal(imgs[0], imgs[1])
