"""MX-fp6 activations (W4A6): the row quantiser (csrc/fp6_ops.hip) bit for bit against the host format, and the fp4 x fp6 GEMM
(csrc/gemm256f4a6.hip) against the float64 product of the dequantised operands at the gates of tests/test_gpu_fp4.py.

Shapes: M in {1, 255, 256, 257} x N in {256, 512} x K in {128, 256, 384, 640}, every combination, for the bias and the GELU -> MX-fp8 tails; the
key tail needs N = 3 h + n2 with h and n2 multiples of 256, so it runs every (M, K) at N = 1024.  The grouped two-problem launch (image + text
rows of one buffer) and the engine follow."""
import pytest
import torch

from diffusionkit_amd import ops
from diffusionkit_amd._lib import DK_EPI_BIAS, DK_EPI_BIAS_GELU
from diffusionkit_amd.weights import pack_activation_mxfp6, quantize_activation_mxfp6
from oracle import fp8 as o8
from oracle.mmdit import Prec, gelu_erf
from tests import _fp8 as f8
from tests import _gates as G
from tests import _mxfp4 as f4
from tests import _mxfp6 as f6
from tests._util import BF, TOL_SINGLE_OP, bf16r, randn, rel_l2

pytestmark = pytest.mark.gpu


def _same_as_host(y, a6, sc, M, K):
    """bytes (pad rows of the last group zero) and scale bytes of the kernel == the host format of the bf16 rows ``y``"""
    code, e8 = quantize_activation_mxfp6(y)
    assert torch.equal(a6.cpu(), pack_activation_mxfp6(code))
    assert torch.equal(f8.array_to_scales(sc, M, K, rows=a6.shape[0]), e8)


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 257])
def test_quantize_rows_mx6(dev, M, K):
    x = f6.hazard_rows(M, K)
    rows = (M + 15) // 16 * 16
    out = torch.full((rows, K // 128 * 96), 0xAA, dtype=torch.uint8, device=dev)  # (the pad rows must be WRITTEN as zeros)
    a6, sc = ops.quantize_rows_mx6(x.to(dev, BF), out=out)
    _same_as_host(x, a6, sc, M, K)


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 257])
def test_ln_modulate_rows_mx6(dev, M, K):
    """against the host format of (a) the oracle's LayerNorm-modulate in bf16 emulation, the reference of test_gpu_fp8.py::test_ln_modulate_mx8, and
    (b) the rows dk_ln_modulate_bf16 stores, whose arithmetic the kernel repeats"""
    from oracle.mmdit import affine_transform
    x, shift, scale = f6.hazard_rows(M, K, seed=1), randn(1, K, seed=2, scale=0.3), randn(1, K, seed=3, scale=0.3)
    xd, sd, cd = x.to(dev, BF), shift.to(dev, BF), scale.to(dev, BF)
    a6, sc = ops.quantize_rows_mx6(xd, sd, cd, mod_seg_len=M)
    _same_as_host(ops.ln_modulate(xd[None], sd, cd)[0].float().cpu(), a6, sc, M, K)
    _same_as_host(affine_transform(x[None], bf16r(shift)[None], bf16r(scale)[None], 1e-6, Prec(BF))[0], a6, sc, M, K)


MS, NS, KS = [1, 255, 256, 257], [256, 512], [128, 256, 384, 640]


def _problem(dev, M, N, K, w=None, a=None, seed=None):
    seed = M + N + K if seed is None else seed
    a = f8.fp8_activation(M, K, seed) if a is None else a
    w = randn(N, K, seed=seed + 1, scale=0.02).to(BF) if w is None else w
    a6, sa, a_dq = f6.activation_operands(a)
    w4, sw, ws, w_dq = f4.weight_operands(w)
    return (a6.to(dev), sa.to(dev), w4.to(dev), sw.to(dev), ws.to(dev)), a_dq, w_dq


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("tail", ["bias", "gelu_mx8"])
def test_gemm_fp4a6(dev, M, N, K, tail):
    args, a_dq, w_dq = _problem(dev, M, N, K)
    bias = randn(N, seed=5, scale=0.5)
    acc = (a_dq.double() @ w_dq.double().t() + bias.double()).float()
    if tail == "bias":
        y = ops.gemm_fp4(*args, bias=bias.to(dev, BF), activations="mxfp6", M=M, k=K).float().cpu()
        r = rel_l2(acc, y)
        print(f"[fp4a6 gemm {M}x{N}x{K}] rel_l2 {r:.3e}")
        assert r < TOL_SINGLE_OP, r
        G.assert_gate(f"fp4a6 bias {M}x{N}x{K}", G.qgemm_gate(y, a_dq, w_dq, bias), missed=M > 1)
    else:  # fc1: GELU, MX-fp8 out (the input of a W4A8 fc2)
        hq, hs = ops.gemm_fp4(*args, bias=bias.to(dev, BF), activations="mxfp6", M=M, k=K, epilogue=DK_EPI_BIAS_GELU, out_mx8=True)
        want_q, want_e = o8.mx8_encode(gelu_erf(bf16r(acc), Prec(BF)))
        got = f8.mx8_decode(hq.cpu(), f8.array_to_scales(hs.cpu(), M, N))
        assert rel_l2(f8.mx8_decode(want_q, want_e), got) < 6e-3
        G.assert_gate(f"fp4a6 gelu -> MX-fp8 {M}x{N}x{K}", G.mx8_gate(got, a_dq, w_dq, bias))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_gemm_fp4a6_key_tail_with_column_split(dev, M, K):
    """linear1's launch: [q | k | v] with QKNorm + RoPE of q and k in the tail, bf16; the columns behind 3 h leave through GELU as MX-fp8"""
    from tests import _fused_cases as fc
    h, D, n2 = 256, 128, 256
    case = dict(h=h, D=D, n_seq=1, seg_len=M, pos_off=0, K=K, table="real", qn=True, n2=n2)
    t = fc.knorm_inputs(case)
    args, a_dq, w_dq = _problem(dev, M, 3 * h + n2, K, w=t["W"].to(BF), a=bf16r(t["A"]))
    keep = dict(bias=t["bias"][0].to(dev, BF), kn=t["kn_w"].to(dev, BF), qn=t["qn_w"].to(dev, BF), rope=t["rope"].to(dev))
    out = torch.full((M + 8, 3 * h), 7.0, dtype=BF, device=dev)
    buf8 = torch.zeros(M, n2, dtype=torch.uint8, device=dev)
    sc = torch.zeros(ops.mx_scale_bytes(M, n2), dtype=torch.uint8, device=dev)
    d = dict(A=args[0], A_scales=args[1], W=args[2], w_scale=args[4], bias=keep["bias"], M=M, N=3 * h + n2, K=K, lda=args[0].shape[1],
             ldw=args[2].shape[1], a_row0=0, a_rows=args[0].shape[0], epilogue=DK_EPI_BIAS, C=out, ldc=3 * h, C_scales=sc, c_rows=M, c_row0=0, c_col0=0)
    side = dict(n_split=3 * h, C2=buf8, ldc2=n2, epi2=DK_EPI_BIAS_GELU, c2_mx8=1, kn_w=keep["kn"], kn_rope=keep["rope"], kn_col0=h, kn_col1=2 * h,
                kn_D=D, kn_pos_off=0, kn_seg_len=M, kn_eps=fc.KN_EPS, qn_w=keep["qn"], qn_col0=0, qn_col1=h)
    ops.gemm_fp4a6_fused_call(d, side, args[3])
    proj = fc.projection(a_dq, w_dq, t["bias"])
    got = out.float().cpu()
    fc.norm_columns_ok(fc.knorm_oracle(case, t, proj, Prec(BF)), got[:M], h, D, f"fp4a6 knorm {M}x{K}")
    assert rel_l2(proj[:, 2 * h:3 * h], got[:M, 2 * h:]) < TOL_SINGLE_OP and bool((got[M:] == 7.0).all())
    want_q, want_e = o8.mx8_encode(gelu_erf(proj[:, 3 * h:], Prec(BF)))
    got8 = f8.mx8_decode(buf8.cpu(), f8.array_to_scales(sc.cpu(), M, n2))
    assert rel_l2(f8.mx8_decode(want_q, want_e), got8) < 6e-3
    G.assert_gate(f"fp4a6 column split, MX-fp8 half {M}x{K}", G.mx8_gate(got8, a_dq, w_dq[3 * h:], t["bias"][0, 3 * h:]))


def test_gemm_fp4a6_k_split(dev):
    """the smallest shape the launch rules cut along K (tests/_mxfp6.py: smallest_split_shape, swept over dk_gemm_fp4a6_plan), at the rules' own
    knobs: the plan says cut once the workspace is there, the producers' slabs witness it, cut and whole are both inside the gate"""
    M, N, K = f6.smallest_split_shape()
    plan = ops.gemm_fp4a6_plan(f6.plan_desc(M, N, K))
    print(f"[fp4a6 K split] {M} x {N} x {K}: {plan.k_pieces} pieces of {plan.tiles} tiles, finisher {plan.ks} K-tiles, {plan.n_cu} CUs")
    assert plan.k_pieces > 1 and ops.gemm_fp4a6_plan(f6.plan_desc(M, N, K, workspace=False)).k_pieces == 1
    args, a_dq, w_dq = _problem(dev, M, N, K)
    bias = randn(N, seed=5, scale=0.5)
    ref = (a_dq.double() @ w_dq.double().t() + bias.double()).float()
    run = lambda **kw: ops.gemm_fp4(*args, bias=bias.to(dev, BF), activations="mxfp6", M=M, k=K, **kw).float().cpu()
    wsp = ops.gemm_workspace(dev)
    y0 = run()
    wsp[:-4096].zero_()
    y = run(workspace=wsp)
    assert bool(wsp[:-4096].any()) and int(wsp[-4096:].sum()) == 0
    assert rel_l2(ref, y) < TOL_SINGLE_OP and rel_l2(ref, y0) < TOL_SINGLE_OP, (rel_l2(ref, y), rel_l2(ref, y0))
    G.assert_gate("fp4a6 bias, cut and whole", G.qgemm_gate([y, y0], a_dq, w_dq, bias), missed=False)


def test_gemm_fp4a6_poisoned_footprint(dev):
    """M = 257: the 15 pad rows of the last 16-row group, the scale bytes of the rows behind M and everything behind the buffer (it ends a larger
    allocation's front part) hold 0xFF -- NaN scales, -7.5 elements; the output is bit-identical to the clean launch"""
    M, N, K = 257, 256, 384
    args, _, _ = _problem(dev, M, N, K)
    a6, sa = args[0], args[1]
    big = torch.full((a6.numel() + 65536,), 0xFF, dtype=torch.uint8, device=dev)
    dirty = big[:a6.numel()].view(a6.shape)
    code = torch.full((a6.shape[0], K), 63, dtype=torch.uint8)  # (fragment order: the pad rows are poisoned before packing)
    code[:M] = quantize_activation_mxfp6(f8.fp8_activation(M, K, M + N + K))[0]
    dirty.copy_(pack_activation_mxfp6(code))
    idx = f8.scale_index(torch.arange(M)[:, None], torch.arange(K // 32)[None, :], f8.n_blk128(a6.shape[0])).reshape(-1).to(dev)
    sa_dirty = torch.full_like(sa, 0xFF)
    sa_dirty[idx] = sa[idx]
    bias = randn(N, seed=5, scale=0.5).to(dev, BF)
    clean = ops.gemm_fp4(*args, bias=bias, activations="mxfp6", M=M, k=K)
    got = ops.gemm_fp4(dirty, sa_dirty, *args[2:], bias=bias, activations="mxfp6", M=M, k=K)
    assert torch.equal(clean.view(torch.int16), got.view(torch.int16)) and not bool(got.isnan().any())


def test_gemm_fp4a6_grouped_pair(dev):
    """the double blocks' launch: image rows [0, 300) and text rows [384, 512) of ONE activation buffer against two weights in one grouped launch"""
    Mi, T0, Mt, N, K = 300, 384, 128, 512, 384
    a = f8.fp8_activation(T0 + Mt, K, 91)
    a6, sa, a_dq = f6.activation_operands(a)
    a6d, sad = a6.to(dev), sa.to(dev)
    descs, keeps, refs = [], [], []
    for seed, row0, M in ((92, 0, Mi), (94, T0, Mt)):
        w4, sw, ws, w_dq = f4.weight_operands(randn(N, K, seed=seed, scale=0.02).to(BF))
        bias = randn(N, seed=seed + 1, scale=0.5)
        keep = dict(w4=w4.to(dev), sw=sw.to(dev), ws=ws.to(dev), bias=bias.to(dev, BF), out=torch.full((M + 8, N), 7.0, dtype=BF, device=dev))
        descs.append(dict(A=a6d.data_ptr() + row0 * a6.shape[1], A_scales=sad, W=keep["w4"], w_scale=keep["ws"], bias=keep["bias"], M=M, N=N, K=K,
                          lda=a6.shape[1], ldw=w4.shape[1], a_row0=row0, a_rows=a6.shape[0], epilogue=DK_EPI_BIAS, C=keep["out"], ldc=N))
        keeps.append(keep)
        refs.append((a_dq[row0:row0 + M], w_dq, bias, M))
    ops.gemm_fp4a6_fused_call(descs[0], None, keeps[0]["sw"], descs[1], None, keeps[1]["sw"])
    for keep, (x, w_dq, bias, M) in zip(keeps, refs):
        y = keep["out"].float().cpu()
        assert rel_l2((x.double() @ w_dq.double().t() + bias.double()).float(), y[:M]) < TOL_SINGLE_OP and bool((y[M:] == 7.0).all())
        G.assert_gate(f"fp4a6 grouped pair, M = {M}", G.qgemm_gate(y[:M], x, w_dq, bias), missed=True)


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------------
def _mx6_fake_quant(x):
    from diffusionkit_amd.weights import dequantize_activation_mxfp6
    x2 = x.to(torch.float32).reshape(-1, x.shape[-1])
    return dequantize_activation_mxfp6(*quantize_activation_mxfp6(x2)).reshape(x.shape)


def _w4a6_act_quant(cfg):
    """oracle/fp8.py: policy_act_quant wrapped: MX-fp6 in front of qkv / fc1 (and so linear1), MX-fp8 in front of o_proj / fc2; the bf16 blocks see neither"""
    keep = tuple(f"multimodal_transformer_blocks.{i}." for i in range(min(int(cfg.fp8_bf16_double_blocks), cfg.depth_multimodal)))

    def aq(x, site=None):
        if site is not None and keep and site[0].startswith(keep):
            return x
        return _mx6_fake_quant(x) if site is not None and site[1] in ("qkv", "fc1") else o8.mx8_fake_quant(x)
    aq.takes_site = True
    return aq


@pytest.mark.parametrize("B,n_bf16", [(1, 0), (2, 0), (1, 1)])
def test_mmdit_fp4a6_tiny(dev, B, n_bf16):
    """tests/test_gpu_fp4.py::test_mmdit_fp4_tiny with activations="mxfp6": one forward step against OracleMMDiT on the same fake-quantised values at
    that test's gate; and with the option off the engine's output is the plain fp4 engine's, bit for bit (a second engine built without it)"""
    from dataclasses import replace
    from diffusionkit_amd.config import fp4_config, tiny_flux
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    from oracle.mmdit import OracleMMDiT
    from tests._util import psnr
    cfg = replace(fp4_config(tiny_flux(depth_multimodal=2, depth_unified=2, heads=2), "speed", activations="mxfp6"), fp8_bf16_double_blocks=n_bf16)
    Hl, Wl, S_t, ts, step = 32, 32, 128, [1000.0, 752.0, 500.0], 1
    named = synth_mmdit_weights(cfg, seed=1234)
    packed = pack_mmdit(cfg, named, dev)
    text, pooled, lat = randn(B, S_t, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, Hl, Wl, 16, seed=5)
    outs = {}
    for name, c in (("a6", cfg), ("a8", replace(cfg, activation_quant="mxfp8")), ("off", cfg)):
        eng = MMDiTEngine(replace(c, activation_quant="mxfp8") if name == "off" else c, packed)
        assert eng.activation_fp6 == (name == "a6")
        if name == "off":
            eng.set_activation_fp6(True)
            eng.set_activation_fp6(False)  # (switched on and off again before prepare: the plain engine)
        eng.prepare(B, (Hl, Wl), S_t, len(ts))
        if name == "a6":
            with pytest.raises(Exception, match="before the first dk_mmdit_prepare"):
                eng.set_activation_fp6(False)
        eng.cache_modulation_params(pooled.to(dev), ts)
        outs[name] = eng.forward_tokens(eng.patchify(lat.to(dev)), text.to(dev, BF), step).float().cpu()
    assert torch.equal(outs["a8"], outs["off"]) and not torch.equal(outs["a8"], outs["a6"])
    fq, res = f4.fake_quant_block_weights(cfg, named), {}
    for name, w, P, aq in (("fq_emu", fq, Prec(BF), _w4a6_act_quant(cfg)), ("fq_fp32", fq, Prec(), _w4a6_act_quant(cfg)),
                           ("fp32", {k: v.float() for k, v in named.items()}, Prec(), None)):
        m = OracleMMDiT(cfg, w, P, act_quant=aq)
        m.cache_modulation_params(pooled, torch.tensor(ts))
        taps = {}
        m(lat, text, ts[step], taps=taps)
        res[name] = taps["final"]
    e_h, e_e = rel_l2(res["fq_fp32"], outs["a6"]), rel_l2(res["fq_fp32"], res["fq_emu"])
    print(f"fp4a6 tiny B={B}, bf16 double blocks {n_bf16}: e_h {e_h:.3e}, e_e {e_e:.3e}; PSNR vs the un-quantised fp32 oracle: W4A6 {psnr(res['fp32'], outs['a6']):.1f} dB, "
          f"W4A8 {psnr(res['fp32'], outs['a8']):.1f} dB -- reported, not gated")
    assert e_h <= 2.0 * e_e + 2e-3, (e_h, e_e)
