"""The text encoders on the MI355X at production widths and kernel edges: the five kernels of csrc/text_ops.hip against fp64 and as NaN footprints, the
score-bias attention at the encoders' head counts, the GEMM routes of the text Linears (tests/_textcases.py, planned on the CPU in
tests/test_text_plan_cpu.py), CLIP-L / CLIP-G / T5-XXL engines at full width with one or two layers, and properties that need no tolerance.

References: oracle/text.py and plain fp64 torch on the CPU.  tests/test_gpu_text.py keeps the toy-size engine and pipeline tests."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from diffusionkit_amd import _lib, ops
from diffusionkit_amd import text as tx
from diffusionkit_amd.text import (CLIP_G, CLIP_L, T5_XXL, CLIPTextEngine, T5EncoderEngine, attention_bias, synth_clip_weights, synth_t5_weights,
                                   tiny_clip, tiny_t5)
from oracle import text as ot
from oracle.mmdit import Prec, gelu_erf, linear
from tests import _footprint as fp
from tests import _textcases as tc
from tests._util import BF, TOL_SINGLE_OP, bf16r, randn, rel_l2
from tests.test_dispatch_plan import plan
from tests.test_gpu_text import yardstick

pytestmark = pytest.mark.gpu

NAN, SENTINEL = fp.NAN, fp.SENTINEL
F64 = torch.float64


def g(t, dev):
    return t.to(dev, BF).contiguous()


def gauss(*shape, seed, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def stream():
    return tx._stream()


# =====================================================================================================================================
# 1. the kernels of text_ops.hip against fp64
# =====================================================================================================================================
LN_SHAPES = [(1, 768), (77, 768), (154, 1280), (5, 200), (3, 8)]  # M not a multiple of 4, one row, h not a multiple of 64 (200, 8)
LN_CONSTANTS = (30.25, -1.703125, 0.0, 1000.0, 0.00390625)  # (bf16 values; h * c is exact in fp32 for every h here, so the mean is c)


def ln64(x, w, b, eps=1e-5):
    x, w, b = x.to(F64), w.to(F64), b.to(F64)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


@pytest.mark.parametrize("kind", ["wide", "offset", "constant"])
@pytest.mark.parametrize("M,h", LN_SHAPES)
def test_layernorm_against_fp64(dev, M, h, kind):
    """nn.LayerNorm rows of N(0.3, 2^2); of mean 30 and deviation 0.05 (bf16 spacing at 30 is 0.125: a one-pass E[x^2] - mean^2 in fp32 loses the
    variance there, the two-pass form does not); and constant rows, whose output is the bias exactly"""
    w, b = randn(h, seed=63, scale=0.2) + 1.0, randn(h, seed=64, scale=0.1)
    w, b = bf16r(w), bf16r(b)
    if kind == "wide":
        x = bf16r(gauss(M, h, seed=62, scale=2.0, shift=0.3))
    elif kind == "offset":
        x = bf16r(gauss(M, h, seed=65, scale=0.05, shift=30.0))
    else:
        x = bf16r(torch.tensor([LN_CONSTANTS[m % len(LN_CONSTANTS)] for m in range(M)])[:, None].expand(M, h).contiguous())
    y = tx._layernorm(g(x, dev), g(w, dev), g(b, dev)).float().cpu()
    assert bool(torch.isfinite(y).all())
    if kind == "constant":
        assert torch.equal(y, b[None].expand(M, h)), "a constant row must give the bias, bit for bit"
        return
    err = rel_l2(ln64(x, w, b), y)
    print(f"[layernorm {M}x{h} {kind}] rel_l2 vs fp64 {err:.3e}")
    assert err < TOL_SINGLE_OP


@pytest.mark.parametrize("kind", [1e-3, 1.0, 3e4, "spike", "zero"])
@pytest.mark.parametrize("M,h", [(1, 4096), (256, 4096), (21, 200)])
def test_t5_rmsnorm_against_fp64(dev, M, h, kind):
    """the T5 RMSNorm of the fp32 residual stream at row magnitudes 1e-3 (mean square = eps), 1 and 3e4, with one channel at 1e5 among N(0, 1) in
    every row, and on all-zero rows (zeros, not NaN)"""
    eps = 1e-6
    w = bf16r(gauss(h, seed=66, scale=0.2, shift=1.0))
    if kind == "zero":
        x = torch.zeros(M, h)
    elif kind == "spike":
        x = gauss(M, h, seed=67)
        x[torch.arange(M), (torch.arange(M) * 37 + h - 1) % h] = 1e5  # (row 0: the last channel, in the ragged chunk of h = 200)
    else:
        x = gauss(M, h, seed=68, scale=kind)
    y = tx._t5_rmsnorm(x.to(dev), g(w, dev), eps).float().cpu()
    assert bool(torch.isfinite(y).all())
    if kind == "zero":
        assert torch.equal(y, torch.zeros(M, h))
        return
    ref = ot.t5_rms_norm(x.to(F64), w.to(F64), eps, Prec())
    err = rel_l2(ref, y)
    print(f"[t5 rmsnorm {M}x{h} {kind}] rel_l2 vs fp64 {err:.3e}")
    assert err < TOL_SINGLE_OP
    if kind == "spike":  # the spike carries the whole-tensor norm: the other channels on their own as well
        rest = x != 1e5
        err = rel_l2(ref[rest], y[rest])
        print(f"[t5 rmsnorm {M}x{h} {kind}] rel_l2 of the channels beside the spike {err:.3e}")
        assert err < TOL_SINGLE_OP


@pytest.mark.parametrize("dim", [8, 768, 4096])
def test_embedding_bit_for_bit(dev, dim):
    """nn.Embedding (+ position rows): n = 154 ids over 77 position rows (the wrap of B = 2), ids 0, vocab - 1 and repeats; the T5 form (no positions,
    fp32 out); both outputs at once; ids outside [0, vocab) are clamped to the nearest row, as the kernel documents"""
    vocab, n, P = 100, 154, 77
    table, pos = randn(vocab, dim, seed=70), randn(P, dim, seed=71)
    ids = torch.randint(0, vocab, (n,), generator=torch.Generator().manual_seed(72))
    ids[:6] = torch.tensor([0, vocab - 1, 7, 7, vocab - 1, 0])
    ids[76:79] = torch.tensor([vocab - 1, 0, 7])  # around the wrap of the position rows
    td, pd = g(table, dev), g(pos, dev)
    ref = bf16r(table[ids] + pos[torch.arange(n) % P])
    e, ef = tx._embedding(td, ids.to(dev), pd, want_f32=True)  # both outputs
    assert e.dtype == BF and ef.dtype == torch.float32
    assert torch.equal(e.float().cpu(), ref) and torch.equal(ef.cpu(), ref)
    e, ef = tx._embedding(td, ids.to(dev), pd)  # CLIP's call
    assert ef is None and torch.equal(e.float().cpu(), ref)
    e, ef = tx._embedding(td, ids.to(dev), None, want_f32=True)  # T5's call
    assert torch.equal(ef.cpu(), table[ids]) and torch.equal(e.float().cpu(), table[ids])
    wild = ids.clone()
    wild[3], wild[80], wild[153], wild[0] = -1, vocab, vocab + 10 ** 6, -(2 ** 31)
    e, ef = tx._embedding(td, wild.to(dev), pd, want_f32=True)
    refc = bf16r(table[wild.clamp(0, vocab - 1)] + pos[torch.arange(n) % P])
    assert torch.equal(e.float().cpu(), refc) and torch.equal(ef.cpu(), refc)


EW_N = [1, 255, 256, 257, 77 * 3072]
QG_FIXED = [-20.0, 0.0, -0.0, 20.0, 50.0, -50.0, 88.0, -88.0, 1e4, -1e4]  # (n = 1 runs the first alone)


@pytest.mark.parametrize("n", EW_N)
def test_quick_gelu_within_one_bf16_ulp(dev, n):
    """op 0, x * sigmoid(1.702 x), on N(0, 3^2) and on the points where exp(-1.702 x) leaves the fp32 range: every result of magnitude >= 1e-30 within
    one bf16 ulp (relative 2^-8) of fp64, smaller ones at most 1e-30 in magnitude, no NaN"""
    a = bf16r(torch.cat([torch.tensor(QG_FIXED), gauss(n, seed=73, scale=3.0)])[:n])
    if n > 1:
        a = torch.cat([a[1:], a[:1]])  # (n = 255 ... 257: a fixed point in the last lane too)
    y = tx._elementwise(0, g(a, dev)).float().cpu().to(F64)
    assert not bool(torch.isnan(y).any())
    a64 = a.to(F64)
    ref = a64 * torch.sigmoid(1.702 * a64)
    big = ref.abs() >= 1e-30
    rel = ((y - ref).abs()[big] / ref.abs()[big])
    worst = float(rel.max()) if rel.numel() else 0.0
    print(f"[quick_gelu n={n}] worst relative error {worst:.3e} (bound {2.0 ** -8:.3e}); {int((~big).sum())} results below 1e-30")
    assert worst <= 2.0 ** -8
    assert bool((y[~big].abs() <= 1e-30).all())


@pytest.mark.parametrize("n", EW_N)
def test_product_and_fp32_residual_add_bit_for_bit(dev, n):
    """op 1 = bf16(a * b); op 2 = fp32 r + bf16 a at stream magnitudes 1 and 1e5 (torch's own fp32 sum)"""
    a, b = bf16r(gauss(n, seed=74, scale=3.0)), bf16r(gauss(n, seed=75))
    y = tx._elementwise(1, g(a, dev), g(b, dev))
    assert torch.equal(y.float().cpu(), bf16r(a * b))
    for mag in (1.0, 1e5):
        r0 = gauss(n, seed=76, scale=mag)
        r = r0.clone().to(dev)
        assert tx._elementwise(2, g(a, dev), r=r) is None
        assert torch.equal(r.cpu(), r0 + a), f"r += y at magnitude {mag}"


def _bias_engine(H, dev, cache={}):
    if H not in cache:
        cfg = dataclasses.replace(tiny_t5(), num_heads=H, d_kv=8, num_layers=1)
        named = synth_t5_weights(cfg, seed=12)
        cache[H] = (cfg, {k: v.float() for k, v in named.items()}, T5EncoderEngine(cfg, named, dev))
    return cache[H]


@pytest.mark.parametrize("H", [4, 64])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 77, 256, 512])
def test_t5_bias_table(dev, S, H):
    """the [H, S, pad64(S)] table the kernel gathers from the host-side buckets == the oracle's bias in columns < S, exactly zero in the pad columns"""
    cfg, wf, eng = _bias_engine(H, dev)
    tab = eng._position_bias(S)
    assert tuple(tab.shape) == (H, S, (S + 63) // 64 * 64) and tab.dtype == BF
    tab = tab.float().cpu()
    assert torch.equal(tab[:, :, :S], bf16r(ot.OracleT5Encoder(cfg, wf).bias(S)))
    assert bool((tab[:, :, S:] == 0).all())


# =====================================================================================================================================
# 2. footprints of the same kernels: operands inside NaN margins, outputs inside sentinel margins, the same launch clean and poisoned
# =====================================================================================================================================
PAD = 4


def sentinel_out(shape, dtype, dev):
    return fp.guarded(torch.full(shape, SENTINEL, dtype=dtype, device=dev), PAD, fill=SENTINEL)


def run_cases(views, clean_cpu, launch, cases, guards, what):
    """``views``: name -> device view; ``clean_cpu``: name -> the clean contents; ``launch()`` -> output (or dict of outputs) read back;
    ``cases``: [(label, [(name, index, value)], expected NaN mask or dict of masks)].  Clean launch first, then every case on restored buffers."""
    def restore():
        for k, v in views.items():
            v.copy_(clean_cpu[k])
    restore()
    clean = launch()
    for label, poison, hand in cases:
        restore()
        for name, idx, val in poison:
            views[name][idx] = val
        got = launch()
        for key in (hand if isinstance(hand, dict) else [None]):
            c, g_, h = (clean, got, hand) if key is None else (clean[key], got[key], hand[key])
            fp.assert_footprint(c, g_, h, f"{what}: {label}" + (f" [{key}]" if key else ""))
    for name, guard in guards.items():
        guard.check(f"{what}: margins of {name}")
    return clean


def mask(shape, *idx):
    m = torch.zeros(shape, dtype=torch.bool)
    if idx:
        m[idx] = True
    return m


@pytest.mark.parametrize("mode", ["layernorm", "t5_rmsnorm"])
def test_rownorm_footprint(dev, mode):
    """(5, 200): rows behind M hold NaN and are not read; one x element poisons its row, one weight / bias element its column; M * h outputs written"""
    lib = _lib.load()
    M, h, rows = 5, 200, 8
    ln = mode == "layernorm"
    cpu = dict(x=gauss(rows, h, seed=80, scale=2.0, shift=0.3), w=bf16r(gauss(h, seed=81, scale=0.2, shift=1.0)), b=bf16r(gauss(h, seed=82, scale=0.1)))
    if ln:
        cpu["x"] = bf16r(cpu["x"])
    bufs = {k: fp.guarded(v.to(dev, BF if (ln or k != "x") else torch.float32), PAD) for k, v in cpu.items()}
    views = {k: v for k, (v, _) in bufs.items()}
    out, og = sentinel_out((M, h), BF, dev)

    def launch():
        out.fill_(SENTINEL)
        if ln:
            _lib.check(lib.dk_layernorm_bf16(views["x"].data_ptr(), out.data_ptr(), M, h, views["w"].data_ptr(), views["b"].data_ptr(), 1e-5, stream()), mode)
        else:
            _lib.check(lib.dk_t5_rmsnorm_bf16(views["x"].data_ptr(), out.data_ptr(), M, h, views["w"].data_ptr(), 1e-6, stream()), mode)
        return out.float().cpu()
    cases = [("rows behind M", [("x", slice(M, None), NAN)], mask((M, h))),
             ("the last x element", [("x", (M - 1, h - 1), NAN)], mask((M, h), M - 1)),
             ("one x element of row 0", [("x", (0, 64), NAN)], mask((M, h), 0)),
             ("one weight element of the ragged chunk", [("w", h - 1, NAN)], mask((M, h), fp.ALL, h - 1))]
    if ln:
        cases.append(("one bias element", [("b", 0, NAN)], mask((M, h), fp.ALL, 0)))
    clean = run_cases(views, cpu, launch, cases, dict({k: gd for k, (_, gd) in bufs.items()}, out=og), mode)
    ref = ln64(cpu["x"][:M], cpu["w"], cpu["b"]) if ln else ot.t5_rms_norm(cpu["x"][:M].to(F64), cpu["w"].to(F64), 1e-6, Prec())
    assert rel_l2(ref, clean) < TOL_SINGLE_OP


def test_embedding_footprint(dev):
    """n = 12, dim 8: table rows no id names, position rows behind pos_rows and ids behind n are not read (the spare ids name a NaN row); one table /
    position element poisons the outputs that gather it; exactly n * dim elements of both outputs are written"""
    lib = _lib.load()
    vocab, dim, n, P = 50, 8, 12, 10
    ids = torch.tensor([3, 49, 0, 7, 7, 12, 1, 2, 3, 4, 5, 6, 0, 0, 0, 0], dtype=torch.int32)  # 12 ids + 4 spare
    named = torch.zeros(vocab, dtype=torch.bool)
    named[ids[:n].long()] = True
    hole = 20  # a row no id names: NaN in every poisoned launch, and what the ids' margins point at
    assert not bool(named[hole])
    cpu = dict(table=bf16r(gauss(vocab, dim, seed=83)), pos=bf16r(gauss(P + 3, dim, seed=84)), ids=ids)
    bufs = dict(table=fp.guarded(cpu["table"].to(dev, BF), PAD), pos=fp.guarded(cpu["pos"].to(dev, BF), PAD),
                ids=fp.guarded(ids.to(dev), PAD, fill=hole))
    views = {k: v for k, (v, _) in bufs.items()}
    (ob, gb), (of, gf) = sentinel_out((n, dim), BF, dev), sentinel_out((n, dim), torch.float32, dev)

    def launch():
        ob.fill_(SENTINEL), of.fill_(SENTINEL)
        _lib.check(lib.dk_embedding_bf16(views["table"].data_ptr(), views["ids"].data_ptr(), views["pos"].data_ptr(), P, ob.data_ptr(), of.data_ptr(),
                                         n, dim, vocab, stream()), "dk_embedding_bf16")
        return dict(bf16=ob.float().cpu(), f32=of.cpu())
    both = lambda m: dict(bf16=m, f32=m)
    unread = [("table", ~named, NAN), ("pos", slice(P, None), NAN), ("ids", slice(n, None), hole)]
    m_tab = mask((n, dim))
    m_tab[3, 5] = m_tab[4, 5] = True  # id 7 twice
    m_pos = mask((n, dim))
    m_pos[1, 2] = m_pos[11, 2] = True  # rows 1 and 11 take position row 1
    cases = [("everything the launch must not read", unread, both(mask((n, dim)))),
             ("one element of a table row named twice", unread + [("table", (7, 5), NAN)], both(m_tab)),
             ("one element of a position row used twice", unread + [("pos", (1, 2), NAN)], both(m_pos))]
    clean = run_cases(views, cpu, launch, cases, dict({k: gd for k, (_, gd) in bufs.items()}, out_bf16=gb, out_f32=gf), "embedding")
    ref = bf16r(cpu["table"][ids[:n].long()] + cpu["pos"][torch.arange(n) % P])
    assert torch.equal(clean["bf16"], ref) and torch.equal(clean["f32"], ref)


@pytest.mark.parametrize("op", [0, 1, 2])
def test_elementwise_footprint(dev, op):
    """n = 257 (two blocks, one live lane in the second): elements behind n are not read, one element poisons one output, n outputs written"""
    lib = _lib.load()
    n, room = 257, 300
    cpu = dict(a=bf16r(gauss(room, seed=85, scale=3.0)), b=bf16r(gauss(room, seed=86)))
    bufs = {k: fp.guarded(v.to(dev, BF), PAD) for k, v in cpu.items()}
    views = {k: v for k, (v, _) in bufs.items()}
    r0 = gauss(n, seed=87)
    (y, gy), (r, gr) = sentinel_out((n,), BF, dev), fp.guarded(r0.to(dev), PAD, fill=SENTINEL)

    def launch():
        y.fill_(SENTINEL), r.copy_(r0)
        _lib.check(lib.dk_text_elementwise(views["a"].data_ptr(), views["b"].data_ptr() if op == 1 else None, y.data_ptr() if op != 2 else None,
                                           r.data_ptr() if op == 2 else None, n, op, stream()), "dk_text_elementwise")
        return (r if op == 2 else y).float().cpu()
    cases = [("elements behind n", [("a", slice(n, None), NAN), ("b", slice(n, None), NAN)], mask((n,))),
             ("the last element of a", [("a", n - 1, NAN)], mask((n,), n - 1)),
             ("the last element of the first block", [("a", 255, NAN)], mask((n,), 255))]
    if op == 1:
        cases.append(("one element of b", [("b", 0, NAN)], mask((n,), 0)))
    run_cases(views, cpu, launch, cases, dict({k: gd for k, (_, gd) in bufs.items()}, y=gy, r=gr), f"elementwise op {op}")
    if op == 2:
        assert bool((y == SENTINEL).all())
    else:
        assert torch.equal(r.cpu(), r0)


def test_t5_bias_footprint(dev):
    """H = 4, S = 65 (ld 128): bucket entries outside [0, 2 S - 2] name a NaN embedding row and are not read, nor are the embedding rows no bucket names;
    one embedding element poisons one diagonal of one head; H * S * ld elements are written and the pad columns stay zero"""
    lib = _lib.load()
    H, S, nb = 4, 65, 32
    ld = (S + 63) // 64 * 64
    bucket = torch.from_numpy(tx.t5_relative_position_bucket(np.arange(-(S - 1), S), nb, 128).astype(np.int32))
    assert bucket.numel() == 2 * S - 1 and int(bucket.min()) >= 0 and int(bucket.max()) < nb
    named = torch.zeros(nb + 1, dtype=torch.bool)
    named[bucket.long()] = True
    hole = nb  # one row behind the table proper: NaN in every poisoned launch, what the spare bucket entries and the margins name
    spare = 16
    cpu = dict(emb=bf16r(gauss(nb + 1, H, seed=88, scale=0.5)), bucket=torch.cat([bucket, torch.zeros(spare, dtype=torch.int32)]))
    bufs = dict(emb=fp.guarded(cpu["emb"].to(dev, BF), PAD), bucket=fp.guarded(cpu["bucket"].to(dev), PAD, fill=hole))
    views = {k: v for k, (v, _) in bufs.items()}
    out, og = sentinel_out((H, S, ld), BF, dev)

    def launch():
        out.fill_(SENTINEL)
        _lib.check(lib.dk_t5_bias_bf16(views["emb"].data_ptr(), views["bucket"].data_ptr(), H, S, ld, out.data_ptr(), stream()), "dk_t5_bias_bf16")
        return out.float().cpu()
    unread = [("emb", ~named, NAN), ("bucket", slice(2 * S - 1, None), hole)]
    b0, hd = int(bucket[S - 1]), H - 1  # the bucket of relative position 0
    m = mask((H, S, ld))
    q, k = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    m[hd, :, :S] = bucket[(k - q + S - 1)] == b0
    assert int(m.sum()) == S, "relative position 0 has a bucket of its own"
    cases = [("everything the launch must not read", unread, mask((H, S, ld))),
             ("the embedding of relative position 0, last head", unread + [("emb", (b0, hd), NAN)], m)]
    clean = run_cases(views, cpu, launch, cases, dict({k_: gd for k_, (_, gd) in bufs.items()}, out=og), "t5 bias")
    assert torch.equal(clean[:, :, :S], cpu["emb"][bucket[(k - q + S - 1)].long()].permute(2, 0, 1)) and bool((clean[:, :, S:] == 0).all())


# =====================================================================================================================================
# 3. score-bias attention at the encoders' head counts
# =====================================================================================================================================
@pytest.mark.parametrize("B,H,S,D,per_head", [(1, 64, 512, 64, True), (2, 64, 256, 64, True), (2, 12, 77, 64, False), (2, 20, 77, 64, False)])
def test_attention_with_score_bias_at_encoder_shapes(dev, B, H, S, D, per_head):
    """test_attention_with_score_bias (tests/test_gpu_text.py), its reference and its bound, at T5-XXL's 64 heads x 512 / 256 tokens (per-head bias,
    bias_head_stride = S * ldb, scale 1) and at CLIP-L's 12 / CLIP-G's 20 heads under the shared causal mask; the reference runs head by head"""
    h = H * D
    qkv = randn(B, S, 3 * h, seed=60)
    ldb = (S + 63) // 64 * 64
    nb = H if per_head else 1
    if per_head:
        bias, scale = bf16r(randn(H, S, S, seed=61, scale=2.0)), 1.0
    else:
        bias, scale = bf16r(ot.clip_causal_mask(S, True))[None], 1.0 / math.sqrt(D)
    bd = torch.zeros(nb, S, ldb)
    bd[..., :S] = bias
    y = attention_bias(g(qkv, dev), H, D, scale, g(bd, dev) if per_head else g(bd[0], dev), per_head).float().cpu()
    ref = torch.empty(B, S, h)
    for hd in range(H):
        q, k, v = (qkv[..., i * h + hd * D:i * h + (hd + 1) * D] for i in range(3))
        s = (q * scale) @ k.transpose(-1, -2) + bias[hd if per_head else 0][None]
        ref[..., hd * D:(hd + 1) * D] = torch.softmax(s, dim=-1) @ v
    err = rel_l2(ref, y)
    worst_head = max(rel_l2(ref[..., hd * D:(hd + 1) * D], y[..., hd * D:(hd + 1) * D]) for hd in range(H))
    print(f"[attention_bias {(B, H, S, D)}] rel_l2 {err:.3e}, worst head {worst_head:.3e}")
    assert err < 2 * TOL_SINGLE_OP
    assert worst_head < 2 * TOL_SINGLE_OP, "one head off (a wrong bias_head_stride hides in the whole-tensor norm of 64 heads)"


# =====================================================================================================================================
# 4. GEMM routes of the text Linears
# =====================================================================================================================================
@pytest.mark.parametrize("M,N,K,tail,bias,kernel,tile_rows", tc.GEMM_CASES, ids=lambda v: str(v))
def test_text_linear_routes(dev, M, N, K, tail, bias, kernel, tile_rows):
    """ops.linear as the engines call it (no workspace), one shape per planned route and edge, against an fp64 matmul of the bf16 operands"""
    p = plan(M, N, K, ws=False)
    assert (p.kernel, p.tile_rows, p.split_tiles) == (kernel, tile_rows, 0)
    x, w = randn(M, K, seed=90), randn(N, K, seed=91, scale=1.0 / math.sqrt(K))  # outputs O(1) at every K
    b = randn(N, seed=92, scale=0.3) if bias else None
    res = randn(M, N, seed=93) if tail == "res" else None
    epi = {"bias": ops.DK_EPI_BIAS, "res": ops.DK_EPI_RES, "gelu": ops.DK_EPI_BIAS_GELU}[tail]
    y = ops.linear(g(x, dev), g(w, dev), g(b, dev) if bias else None, epilogue=epi, res=g(res, dev) if res is not None else None).float().cpu()
    ref = x.to(F64) @ w.to(F64).t()
    if bias:
        ref = ref + b.to(F64)
    if tail == "gelu":
        ref = 0.5 * ref * (1.0 + torch.erf(ref / math.sqrt(2.0)))
    if tail == "res":
        ref = ref + res.to(F64)
    err = rel_l2(ref, y)
    worst_row = float(((ref - y.to(F64)).norm(dim=1) / ref.norm(dim=1)).max())
    print(f"[text linear {(M, N, K)} {tail}] kernel {p.kernel} x {p.tile_rows}: rel_l2 {err:.3e}, worst row {worst_row:.3e}")
    assert bool(torch.isfinite(y).all()) and err < TOL_SINGLE_OP


# =====================================================================================================================================
# 5. engines at production width, one or two layers
# =====================================================================================================================================
def report(hip, emu, exact, what):
    print(f"[{what}] hip-vs-fp32 {rel_l2(exact, hip):.3e}, emu-vs-fp32 {rel_l2(exact, emu):.3e}")
    yardstick(hip, emu, exact, what)


@pytest.mark.parametrize("name", ["clip_l", "clip_g"])
def test_clip_engine_at_production_width(dev, name):
    """CLIP-L (768 / 12 heads, quick-GELU) and CLIP-G (1280 / 20 heads, erf-GELU), two layers, vocabulary 1024.  Row 0 is [bos, eos, pad ...]: its EOS
    sits at position 1 and, for CLIP-L, the pads are EOS ids as well (argmax: the first maximum wins); row 1 has its EOS at position 76"""
    cfg = dataclasses.replace(CLIP_L if name == "clip_l" else CLIP_G, num_layers=2, vocab_size=1024)
    eos, bos = cfg.vocab_size - 1, cfg.vocab_size - 2
    pad = eos if name == "clip_l" else 0
    tokens = torch.randint(1, bos, (2, 77), generator=torch.Generator().manual_seed(5))
    tokens[:, 0] = bos
    tokens[0, 1], tokens[0, 2:] = eos, pad
    tokens[1, 76] = eos
    named = synth_clip_weights(cfg, seed=13)
    out = CLIPTextEngine(cfg, named, dev)(tokens)
    wf = {k: v.float() for k, v in named.items()}
    res = {n: ot.OracleCLIPText(cfg, wf, P)(tokens) for n, P in (("fp32", Prec()), ("emu", Prec(BF)))}
    assert len(out.hidden_states) == 2 and tuple(out.pooled_output.shape) == (2, cfg.projection_dim)
    report(out.hidden_states[-2].float(), res["emu"][2][-2], res["fp32"][2][-2], f"{name} hidden[-2]")
    report(out.last_hidden_state.float(), res["emu"][1], res["fp32"][1], f"{name} last")
    report(out.pooled_output.float(), res["emu"][0], res["fp32"][0], f"{name} pooled")
    # the pooled row of prompt 0 is the EOS at position 1, not a pad: the projection of that row of last_hidden_state
    assert rel_l2(res["fp32"][1][0, 1] @ wf["text_projection.weight"].t(), res["fp32"][0][0]) < 1e-6


@pytest.fixture(scope="module")
def t5_wide(dev):
    """one layer at T5-XXL width (vocabulary 512): engine and fp32 weights, shared by the two token shapes"""
    cfg = dataclasses.replace(T5_XXL, num_layers=1, vocab_size=512)
    named = synth_t5_weights(cfg, seed=14)
    eng = T5EncoderEngine(cfg, named, dev)
    wf = {k: v.float() for k, v in named.items()}
    del named
    yield cfg, eng, wf
    del eng, wf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B,N", [(1, 256), (2, 77)])
def test_t5_engine_at_production_width(t5_wide, B, N):
    """one T5-XXL layer (4096 / 64 heads / d_ff 10240): K = 10240 on the 128-tile kernel, 64 per-head bias tables, h = 4096 row norms"""
    cfg, eng, wf = t5_wide
    tokens = torch.randint(0, cfg.vocab_size, (B, N), generator=torch.Generator().manual_seed(6))
    out = eng(tokens)
    assert tuple(out.shape) == (B, N, cfg.d_model) and out.dtype == BF
    res = {n: ot.OracleT5Encoder(cfg, wf, P)(tokens) for n, P in (("fp32", Prec()), ("emu", Prec(BF)))}
    report(out.float(), res["emu"], res["fp32"], f"t5-xxl width {(B, N)}")


def t5_with_bf16_stream(cfg, w, tokens):
    """OracleT5Encoder in its bf16-emulating mode with the one change the deep test is after: the residual stream rounded to bf16 after every addition"""
    P = Prec(BF)
    B, N = tokens.shape
    H, D = cfg.num_heads, cfg.d_kv
    x = w["wte.weight"][tokens].to(torch.float32)
    bias = ot.OracleT5Encoder(cfg, w).bias(N)
    for i in range(cfg.num_layers):
        p = f"encoder.layers.{i}"
        y = P.r(ot.t5_rms_norm(x, w[p + ".ln1.weight"], cfg.layer_norm_epsilon, P))
        q, k, v = (linear(y, w[p + f".attention.{n}_proj.weight"], None, P).reshape(B, N, H, D).transpose(1, 2) for n in ("query", "key", "value"))
        a = P.r(torch.softmax(P.r(P.r(q @ k.transpose(-1, -2)) + P.r(bias)), dim=-1))
        x = P.r(x + linear(P.r(a @ v).transpose(1, 2).reshape(B, N, H * D), w[p + ".attention.out_proj.weight"], None, P))
        y = ot.t5_rms_norm(x, w[p + ".ln2.weight"], cfg.layer_norm_epsilon, P)
        x = P.r(x + (gelu_erf(y @ w[p + ".dense.wi_0.weight"].t(), Prec()) * (y @ w[p + ".dense.wi_1.weight"].t())) @ w[p + ".dense.wo.weight"].t())
    return P.r(ot.t5_rms_norm(x, w["encoder.ln.weight"], cfg.layer_norm_epsilon, P))


@pytest.mark.parametrize("scale", [1e4, 64.0])
def test_t5_deep_narrow_with_a_large_residual_stream(dev, monkeypatch, scale):
    """twelve tiny_t5 layers on an embedding scaled so that the fp32 residual stream is ~1e4 by the last layer (asserted on the oracle): what the fp32
    stream and r += y exist for.  At 1e4 the layers' additions (~1 each) are 1e-4 of the output, below the output's own bf16 rounding, so the
    yardstick sees an engine that breaks down there but not a stream merely kept in bf16 (the oracle with such a stream: 1.7e-3 against a bound of
    5.3e-3).  The second scale, 64, is where it does: a bf16 stream (spacing 0.5 at 64) loses part of every addition and the oracle with such a
    stream misses the bound (8e-3 against 5.3e-3) -- asserted below, so the case is known to see what it is for."""
    cfg = dataclasses.replace(tiny_t5(), num_layers=12)
    named = synth_t5_weights(cfg, seed=15)
    named["wte.weight"] = (named["wte.weight"].float() * scale).to(BF)
    tokens = torch.randint(0, cfg.vocab_size, (2, 150), generator=torch.Generator().manual_seed(7))
    out = T5EncoderEngine(cfg, named, dev)(tokens)
    wf = {k: v.float() for k, v in named.items()}
    seen = []
    real = ot.t5_rms_norm
    monkeypatch.setattr(ot, "t5_rms_norm", lambda x, *a: (seen.append(float(x.pow(2).mean().sqrt())), real(x, *a))[1])
    exact = ot.OracleT5Encoder(cfg, wf, Prec())(tokens)
    monkeypatch.undo()
    assert len(seen) == 2 * cfg.num_layers + 1
    print(f"[deep t5 x{scale:g}] rms of the fp32 stream entering the final norm {seen[-1]:.3e}")
    assert 0.5 * scale < seen[-1] < 2.0 * scale
    emu = ot.OracleT5Encoder(cfg, wf, Prec(BF))(tokens)
    if scale == 64.0:
        e_n, e_e = rel_l2(exact, t5_with_bf16_stream(cfg, wf, tokens)), rel_l2(exact, emu)
        print(f"[deep t5 x{scale:g}] the oracle with a bf16 stream: {e_n:.3e} against the bound {2 * e_e + 2e-3:.3e}")
        assert e_n > 2 * e_e + 2e-3, "this case no longer tells an fp32 stream from a bf16 one"
    report(out.float(), emu, exact, f"deep narrow t5 x{scale:g}")


# =====================================================================================================================================
# 6. properties that need no tolerance
# =====================================================================================================================================
def clip_tokens(cfg, B=2, N=77, seed=8):
    t = torch.randint(1, cfg.vocab_size - 1, (B, N), generator=torch.Generator().manual_seed(seed))
    t[:, N - 1] = cfg.vocab_size - 1
    return t


@pytest.mark.parametrize("p", [0, 9, 63, 64])
def test_clip_is_causal_bit_for_bit(dev, p):
    """other tokens behind position p: every hidden state up to and including p keeps its bits (the -6e4 mask makes those probabilities exactly zero);
    p = 63 / 64: the last key of the first 64-key tile and the first of the second"""
    cfg = tiny_clip()
    eng = CLIPTextEngine(cfg, synth_clip_weights(cfg, seed=11), dev)
    a = clip_tokens(cfg)
    b = a.clone()
    b[:, p + 1:] = torch.randint(1, cfg.vocab_size - 1, (2, 77 - p - 1), generator=torch.Generator().manual_seed(9))
    assert not torch.equal(a[:, p + 1:], b[:, p + 1:])
    ya, yb = eng(a), eng(b)
    assert torch.equal(ya.last_hidden_state[:, :p + 1], yb.last_hidden_state[:, :p + 1])
    for i, (ha, hb) in enumerate(zip(ya.hidden_states, yb.hidden_states)):
        assert torch.equal(ha[:, :p + 1], hb[:, :p + 1]), f"hidden state {i}"
    assert not torch.equal(ya.last_hidden_state[:, p + 1:], yb.last_hidden_state[:, p + 1:])


def same_route(linears, rows_a, rows_b):
    """both row counts name one GEMM kernel and tile height for every (N, K)"""
    return all((plan(rows_a, N, K, ws=False).kernel, plan(rows_a, N, K, ws=False).tile_rows) ==
               (plan(rows_b, N, K, ws=False).kernel, plan(rows_b, N, K, ws=False).tile_rows) for N, K in linears)


def test_clip_rows_of_a_batch_are_independent(dev):
    """each prompt of a B = 2 call == its own B = 1 call, bit for bit (77 and 154 rows take the same GEMM kernel at this width: checked first; were
    they not, the comparison would be the yardstick against the oracle instead)"""
    cfg = tiny_clip()
    named = synth_clip_weights(cfg, seed=11)
    eng = CLIPTextEngine(cfg, named, dev)
    tokens = clip_tokens(cfg)
    tokens[0, 9:] = cfg.vocab_size - 1
    both = eng(tokens)
    exact = same_route(tc.clip_linears(cfg).values(), 77, 154) and same_route([(cfg.projection_dim, cfg.model_dims)], 1, 2)
    for r in range(2):
        one = eng(tokens[r:r + 1])
        pairs = [(both.last_hidden_state[r], one.last_hidden_state[0], 1), (both.pooled_output[r], one.pooled_output[0], 0)]
        pairs += [(hb[r], ho[0], None) for hb, ho in zip(both.hidden_states, one.hidden_states)]
        if exact:
            for x, y, _ in pairs:
                assert torch.equal(x, y), f"prompt {r}"
        else:
            wf = {k: v.float() for k, v in named.items()}
            res = {n: ot.OracleCLIPText(cfg, wf, P)(tokens[r:r + 1]) for n, P in (("fp32", Prec()), ("emu", Prec(BF)))}
            for x, _, which in pairs[:2]:
                yardstick(x.float(), res["emu"][which][0], res["fp32"][which][0], f"prompt {r} of the batch")


@pytest.mark.parametrize("N", [77, 150])
def test_t5_rows_of_a_batch_are_independent(dev, N):
    cfg = tiny_t5()
    named = synth_t5_weights(cfg, seed=12)
    eng = T5EncoderEngine(cfg, named, dev)
    tokens = torch.randint(0, cfg.vocab_size, (2, N), generator=torch.Generator().manual_seed(10))
    both = eng(tokens)
    exact = same_route(tc.t5_linears(cfg).values(), N, 2 * N)
    for r in range(2):
        if exact:
            assert torch.equal(both[r], eng(tokens[r:r + 1])[0]), f"prompt {r}"
        else:
            wf = {k: v.float() for k, v in named.items()}
            res = {n: ot.OracleT5Encoder(cfg, wf, P)(tokens[r:r + 1]) for n, P in (("fp32", Prec()), ("emu", Prec(BF)))}
            yardstick(both[r:r + 1].float(), res["emu"], res["fp32"], f"prompt {r} of the batch")


def test_cached_tables_survive_other_lengths(dev):
    """N = 77, then 20, then 77 on one engine: the first result again, and the N = 20 result of a fresh engine (CLIP's _mask, T5's _position_bias)"""
    ccfg, tcfg = tiny_clip(), tiny_t5()
    cw, tw = synth_clip_weights(ccfg, seed=11), synth_t5_weights(tcfg, seed=12)
    clip, t5 = CLIPTextEngine(ccfg, cw, dev), T5EncoderEngine(tcfg, tw, dev)
    ct, tt = clip_tokens(ccfg), torch.randint(0, tcfg.vocab_size, (2, 77), generator=torch.Generator().manual_seed(10))
    ct20 = ct[:, :20].clone()
    ct20[:, 19] = ccfg.vocab_size - 1
    c1, t1 = clip(ct), t5(tt).clone()
    c20, t20 = clip(ct20), t5(tt[:, :20]).clone()
    c2, t2 = clip(ct), t5(tt)
    assert torch.equal(c1.last_hidden_state, c2.last_hidden_state) and torch.equal(c1.pooled_output, c2.pooled_output)
    assert torch.equal(t1, t2)
    f20, ft20 = CLIPTextEngine(ccfg, cw, dev)(ct20), T5EncoderEngine(tcfg, tw, dev)(tt[:, :20])
    assert torch.equal(c20.last_hidden_state, f20.last_hidden_state) and torch.equal(c20.pooled_output, f20.pooled_output)
    assert torch.equal(t20, ft20)
    assert sorted(clip._masks) == [20, 77] and sorted(t5._bias) == [20, 77]
