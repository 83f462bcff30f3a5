"""NaN-footprint comparator (plain torch, no GPU needed).

One element (or one region) of an operand is poisoned with NaN; the set of NaN outputs must then be exactly the operation's data-dependency
footprint, and every output outside it must be BIT-identical to the clean run of the same launch.  No tolerance is involved: the technique
pins addressing, segment maps, halo geometry, masking and batch / head / group independence exactly, and it turns "reads data it must not
depend on, but multiplies it by zero" into a failure (0 * NaN = NaN).

The expected footprint of a case is ``isnan(reference(poisoned operands))`` with the references below -- the fp32 oracle's restatement of each
launch form.  tests/test_footprint_cpu.py proves on the CPU that these references have exactly the hand-written dependency sets the GPU tests
rely on, with everything outside bit-equal to their own clean run.
"""
import math

import torch

from oracle import mmdit as om
from oracle import vae as ov
from oracle.mmdit import Prec

NAN = float("nan")
SENTINEL = 7.0  # (finite output sentinel, as tests/test_gpu_fused_ops.py)
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t: torch.Tensor) -> torch.Tensor:
    """the raw bit patterns of ``t`` as integers of its element size (8, 16, 32 or 64 bits)"""
    t = t.detach().cpu().contiguous()
    return t if t.dtype == torch.uint8 else t.view(_INT[t.element_size()])


def nan_mask(t: torch.Tensor) -> torch.Tensor:
    """where ``t`` holds a NaN; for uint8 tensors, where the byte is an e4m3 NaN (0x7F / 0xFF: float8_e4m3fn has no other)"""
    t = t.detach().cpu()
    if t.dtype == torch.uint8:
        return (t & 0x7F) == 0x7F
    return torch.isnan(t)


class Guard:
    """the margins around a ``guarded`` view: ``intact()`` is False once any margin element no longer holds the fill pattern"""

    def __init__(self, whole, lo, hi, fill):
        self.whole, self.lo, self.hi = whole, lo, hi
        self._fill = bits(torch.full((1,), fill, dtype=whole.dtype))[0]

    def written(self) -> int:
        b = bits(self.whole)
        return int((b[:self.lo] != self._fill).sum()) + int((b[self.hi:] != self._fill).sum())

    def intact(self) -> bool:
        return self.written() == 0

    def check(self, what: str) -> None:
        n = self.written()
        assert n == 0, f"{what}: {n} margin elements around the tensor were written"


def guarded(t: torch.Tensor, pad_rows: int, fill=NAN):
    """(view, guard): ``view`` has ``t``'s shape, dtype, strides, device and values, and sits inside a larger allocation whose margins of
    ``pad_rows`` rows (a row = ``t.shape[-1]`` elements; rounded up to a multiple of 128 elements, so the view keeps a 128-byte alignment) in
    front of and behind it hold ``fill`` -- NaN for operands, a finite sentinel for outputs; ``guard.check()`` verifies the margins afterwards."""
    row = t.shape[-1] if t.dim() else 1
    pad = (max(1, pad_rows) * row + 127) // 128 * 128
    span = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride())) if t.numel() else 0
    whole = torch.full((pad + span + pad,), fill, dtype=t.dtype, device=t.device)
    view = torch.as_strided(whole, t.shape, t.stride(), pad)
    view.copy_(t)
    return view, Guard(whole, pad, pad + span, fill)


def _first(mask: torch.Tensor):
    return tuple(int(i) for i in torch.nonzero(mask)[0])


def assert_footprint(clean, poisoned, expect_nan, what, soft=None, soft_ref=None, soft_rel_l2=None, soft_max_abs=None):
    """(a) isnan(poisoned) == expect_nan element for element (a missing NaN: the poison was never read, the case is vacuous; an extra one: a leak);
    (b) outside expect_nan the raw bit patterns of ``poisoned`` and ``clean`` are equal; (c) ``clean`` holds no NaN / Inf.
    ``soft``: boolean mask of outputs where (b) is replaced by "finite, and within the oracle gate of the test the case mirrors" -- relative L2
    ``soft_rel_l2`` and largest difference ``soft_max_abs`` against ``soft_ref`` over the soft elements."""
    clean, poisoned = clean.detach().cpu(), poisoned.detach().cpu()
    expect_nan = expect_nan.detach().cpu().to(torch.bool)
    assert clean.shape == poisoned.shape == expect_nan.shape, f"{what}: shapes {tuple(clean.shape)} {tuple(poisoned.shape)} {tuple(expect_nan.shape)}"
    bad_clean = nan_mask(clean) if clean.dtype == torch.uint8 else ~torch.isfinite(clean)
    assert not bool(bad_clean.any()), f"{what}: the clean run holds {int(bad_clean.sum())} non-finite outputs, first at {_first(bad_clean)}"
    got = nan_mask(poisoned)
    missing, extra = expect_nan & ~got, got & ~expect_nan
    assert not bool(missing.any()), (f"{what}: {int(missing.sum())} of {int(expect_nan.sum())} footprint elements stayed finite "
                                     f"(the poison was not read), first at {_first(missing)}")
    assert not bool(extra.any()), (f"{what}: {int(extra.sum())} NaN outputs outside the footprint of {int(expect_nan.sum())} (a leak), "
                                   f"first at {_first(extra)}")
    outside = ~expect_nan
    if soft is not None:
        soft = soft.detach().cpu().to(torch.bool) & outside
        outside = outside & ~soft
        if bool(soft.any()):
            sv = poisoned[soft].double()
            assert bool(torch.isfinite(sv).all()), f"{what}: non-finite output in the soft region"
            rv = soft_ref.detach().cpu()[soft].double()
            rel = float(torch.linalg.norm(sv - rv) / (torch.linalg.norm(rv) + 1e-30))
            worst = float((sv - rv).abs().max())
            assert rel < soft_rel_l2 and worst < soft_max_abs, (f"{what}: soft region ({int(soft.sum())} elements) rel_l2 {rel:.3e} "
                                                                f"(< {soft_rel_l2}), max_abs {worst:.3e} (< {soft_max_abs})")
    diff = (bits(poisoned) != bits(clean)) & outside
    assert not bool(diff.any()), (f"{what}: {int(diff.sum())} outputs outside the footprint differ in their bits from the clean run, "
                                  f"first at {_first(diff)}: {poisoned[_first(diff)]!r} against {clean[_first(diff)]!r}")


# ---- references: the fp32 oracle's restatement of each launch form ---------------------------------------------------------------------
def ref_gemm_joint(att, X, w, b, gate, S_t, epi):
    """the text stream of a joint [B, S_t + S_i] buffer (tests/test_gpu_ops.py: test_gemm_v3_ragged_and_straddling_segments): A = att[:, :S_t],
    C (and the residual) = X[:, :S_t]; the gate is the second half of a [B, 2 N] table; the image rows of X are not touched"""
    N = w.shape[0]
    o = att[:, :S_t] @ w.t() + b
    out = X.clone()
    if epi == "bias":
        out[:, :S_t] = o
    else:
        out[:, :S_t] = X[:, :S_t] + gate[:, None, N:] * o
    return out


def ref_linear(x, w, b=None, gate=None, res=None):
    y = x @ w.t()
    if b is not None:
        y = y + b
    if gate is not None:
        y = res + gate * y
    return y


def split_heads(qkv, H, D):
    B, S, _ = qkv.shape
    h = H * D
    return tuple(qkv[..., i * h:(i + 1) * h].reshape(B, S, H, D).transpose(1, 2) for i in range(3))


def ref_attention(qkv, H, D, scale=None, bias=None):
    """oracle.mmdit.sdpa over a packed [B, S, 3 H D] buffer -> [B, S, H D]; ``bias`` [H or 1, S, S] is added to the scores"""
    B, S, _ = qkv.shape
    q, k, v = split_heads(qkv, H, D)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if bias is None:
        y = om.sdpa(q, k, v, scale, Prec())
    else:
        y = torch.softmax((q * scale) @ k.transpose(-1, -2) + bias[None], dim=-1) @ v
    return y.transpose(1, 2).reshape(B, S, H * D)


def ref_attention_d512(q, k, v):
    return om.sdpa(q[:, None], k[:, None], v[:, None], 1.0 / math.sqrt(q.shape[-1]), Prec())[:, 0]


def ref_ln_modulate(x, shift, scale, eps=1e-6):
    return om.layer_norm(x, eps) * (1.0 + scale[:, None]) + shift[:, None]


def ref_qk_norm_rope(qkv, H, D, qw, kw, tab, eps=1e-6):
    """RMS norm over each head of q and k, then the rotation of adjacent pairs by the table row of the token; v passes through"""
    B, S, _ = qkv.shape
    h = H * D
    q, k, v = split_heads(qkv, H, D)
    q, k = om.rms_norm(q, qw, eps, Prec()), om.rms_norm(k, kw, eps, Prec())
    if tab is not None:
        q, k = om.rope_apply(q, tab, Prec()), om.rope_apply(k, tab, Prec())
    return torch.cat([t.transpose(1, 2).reshape(B, S, h) for t in (q, k, v)], dim=-1)


def ref_groupnorm(x, gamma, beta, G, eps=1e-5, silu=False):
    y = ov.group_norm_nhwc(x, gamma, beta, G, eps, Prec())
    return ov.silu(y, Prec()) if silu else y


def ref_groupnorm_table(x, gamma, beta, G, eps=1e-5):
    """[B, 2, C]: (scale | shift) with y = x * scale + shift, as ops.groupnorm_table"""
    B, C = x.shape[0], x.shape[-1]
    xg = x.reshape(B, -1, G, C // G)
    mu = xg.mean(dim=(1, 3))
    var = ((xg - mu[:, None, :, None]) ** 2).mean(dim=(1, 3))
    rstd = torch.rsqrt(var + eps).repeat_interleave(C // G, dim=1)
    mu = mu.repeat_interleave(C // G, dim=1)
    sc = rstd * gamma
    return torch.stack([sc, beta - mu * sc], dim=1)


def ref_conv(x, w, b, form="plain", res=None, act=None, x2=None, ws=None, bs=None):
    """3 x 3 convolution over NHWC ``x`` (``act``: the activation in front of it, a function of x, for the fused norm -> silu -> conv form);
    form "plain": stride 1 pad 1, "up": over the nearest-x2 view, "s2": stride 2 over x padded bottom / right; + residual, + 1 x 1 shortcut"""
    a = act(x) if act is not None else x
    if form == "up":
        y = ov.conv2d_nhwc(ov.upsample_nearest(a), w, b, Prec())
    elif form == "s2":
        y = ov.conv2d_s2_pad_br_nhwc(a, w, b, Prec())
    else:
        y = ov.conv2d_nhwc(a, w, b, Prec())
    if res is not None:
        y = y + res
    if x2 is not None:
        y = y + (x2 @ ws.t() + bs)
    return y


def conv_footprint(shape_in, form, b, y, x):
    """hand-written footprint [B, Ho, Wo] of input pixel (b, y, x): the 3 x 3 neighbourhood clipped to its own image; for "up" the 2 x 2 block
    dilated by one; for "s2" the outputs whose window (rows 2 i .. 2 i + 2) holds the pixel"""
    B, H, W = shape_in
    if form == "up":
        Ho, Wo, ys, xs = 2 * H, 2 * W, range(2 * y - 1, 2 * y + 3), range(2 * x - 1, 2 * x + 3)
    elif form == "s2":
        Ho, Wo = H // 2, W // 2
        ys, xs = [i for i in range(Ho) if 2 * i <= y <= 2 * i + 2], [j for j in range(Wo) if 2 * j <= x <= 2 * j + 2]
    else:
        Ho, Wo, ys, xs = H, W, range(y - 1, y + 2), range(x - 1, x + 2)
    m = torch.zeros(B, Ho, Wo, dtype=torch.bool)
    for i in ys:
        for j in xs:
            if 0 <= i < Ho and 0 <= j < Wo:
                m[b, i, j] = True
    return m


# ---- case families: shared by the CPU proof (hand-written footprints) and the GPU tests (footprint = isnan(reference(poisoned))) --------------
# A family is (operands, reference, cases): ``operands`` name -> fp32 CPU tensor of values representable in the launch's element type,
# ``reference(operands)`` the output (or a dict of outputs), ``cases`` a list of Case.
class Case:
    """``poison``: [(operand name, index)] -- operand[index] = NaN; ``hand``: the hand-written footprint (bool mask of the output's shape, or a dict
    of masks); ``soft``: the mask of outputs exempt from bit-equality (attention Q rule only), None elsewhere"""

    def __init__(self, label, poison, hand, soft=None):
        self.label, self.poison, self.hand, self.soft = label, poison, hand, soft


def poisoned(operands, case):
    out = {k: v.clone() for k, v in operands.items()}
    for name, idx in case.poison:
        out[name][idx] = NAN
    return out


def rounder(dtype):
    def rnd(*shape, seed, scale=1.0, shift=0.0):
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift
        return x.to(dtype).to(torch.float32)
    return rnd


ALL = slice(None)
GEMM_JOINT_SHAPES = [(3, 77, 11), (2, 589, 64)]  # (B, S_t, S_i); h 192, N 512


def gemm_joint_family(B, S_t, S_i, epi, dtype, h=192, N=512):
    rnd = rounder(dtype)
    S = S_t + S_i
    ops = dict(att=rnd(B, S, h, seed=40), X=rnd(B, S, N, seed=41), w=rnd(N, h, seed=42, scale=0.08), b=rnd(N, seed=43, scale=0.1),
               gate=rnd(B, 2 * N, seed=44))

    def ref(o):
        return ref_gemm_joint(o["att"], o["X"], o["w"], o["b"], o["gate"], S_t, epi)

    def mask(*idx):
        m = torch.zeros(B, S, N, dtype=torch.bool)
        if idx:
            m[idx] = True
        return m
    b1 = B - 1  # first row of the last segment: a tile that straddles two segments of every map
    cases = [Case("other stream's rows of A and C", [("att", (ALL, slice(S_t, None))), ("X", (ALL, slice(S_t, None)))], mask(ALL, slice(S_t, None))),
             Case("one A element in the last K-tile", [("att", (b1, 0, h - 1))], mask(b1, 0)),
             Case("one A element of the last text row", [("att", (b1, S_t - 1, h - 3))], mask(b1, S_t - 1)),
             Case("one W element", [("w", (300, 5))], mask(ALL, slice(0, S_t), 300)),
             Case("one bias element", [("b", (511,))], mask(ALL, slice(0, S_t), 511))]
    if epi == "gate_res":
        cases.append(Case("one gate element", [("gate", (b1, N + 257))], mask(b1, slice(0, S_t), 257)))
        cases.append(Case("one residual element", [("X", (0, S_t - 1, 130))], mask(0, S_t - 1, 130)))
    return ops, ref, cases


def gemm_ksplit_family(dtype, M=1024, N=768, K=640):
    """test_gemm_v3_remainder_split's smallest shape, gate + residual: a NaN in the LAST K range must reach its output row (the finisher adds the
    producers' slabs) and nothing else"""
    rnd = rounder(dtype)
    ops = dict(x=rnd(M, K, seed=50), w=rnd(N, K, seed=51, scale=0.05), b=rnd(N, seed=52, scale=0.1), res=rnd(M, N, seed=53), gate=rnd(1, N, seed=54))

    def ref(o):
        return ref_linear(o["x"], o["w"], o["b"], o["gate"], o["res"])

    def mask(*idx):
        m = torch.zeros(M, N, dtype=torch.bool)
        if idx:
            m[idx] = True
        return m
    return ops, ref, [Case("one A element in the last K range", [("x", (M - 3, K - 1))], mask(M - 3)),
                      Case("one W element in the last K range", [("w", (N - 2, K - 2))], mask(ALL, N - 2))]


def attention_family(B, H, S, D, QB, dtype, scale_in=1.0, last_range_key=False):
    """packed qkv [B, S, 3 H D].  QB: the kernel's query block (rows that share a workgroup): the soft region of the Q case is the other rows of the
    poisoned row's block and head"""
    rnd = rounder(dtype)
    h = H * D
    ops = dict(qkv=rnd(B, S, 3 * h, seed=32, scale=scale_in))

    def ref(o):
        return ref_attention(o["qkv"], H, D)

    def mask(*idx):
        m = torch.zeros(B, S, h, dtype=torch.bool)
        if idx:
            m[idx] = True
        return m
    b0, hh = B - 1, H - 1
    head = slice(hh * D, (hh + 1) * D)
    cases = []
    if B == 2:
        cases.append(Case("image 1 poisoned", [("qkv", (1,))], mask(1)))
    else:
        cases.append(Case("margins only", [], mask()))
    j = S - 2  # in the ragged last key tile (or the last key range)
    cases.append(Case("one K element", [("qkv", (b0, j, h + hh * D + 3))], mask(b0, ALL, head)))
    cases.append(Case("one V element", [("qkv", (b0, j, 2 * h + hh * D + 5))], mask(b0, ALL, hh * D + 5)))
    i = S // 2 + 1
    blk = slice(i // QB * QB, min(S, i // QB * QB + QB))
    soft = mask(b0, blk, head)
    soft[b0, i] = False
    cases.append(Case("one Q element", [("qkv", (b0, i, hh * D + 7))], mask(b0, i, head), soft=soft))
    return ops, ref, cases


def attention_bias_family(B, H, S, D, per_head, dtype=torch.bfloat16):
    """tests/test_gpu_text.py: test_attention_with_score_bias; the bias table [H or 1, S, ldb] with ldb = S rounded up to 64 (pad columns S..ldb)"""
    rnd = rounder(dtype)
    h, nb, ldb = H * D, (H if per_head else 1), (S + 63) // 64 * 64
    bias = torch.zeros(nb, S, ldb)
    bias[..., :S] = rnd(nb, S, S, seed=61, scale=2.0)
    scale = 1.0 if per_head else 1.0 / math.sqrt(D)
    ops = dict(qkv=rnd(B, S, 3 * h, seed=60), bias=bias)

    def ref(o):
        return ref_attention(o["qkv"], H, D, scale, o["bias"][..., :S].expand(H, S, S))

    def mask(*idx):
        m = torch.zeros(B, S, h, dtype=torch.bool)
        if idx:
            m[idx] = True
        return m
    hb, i, j = nb - 1, S // 2, S - 1
    cols = slice(hb * D, (hb + 1) * D) if per_head else ALL
    return ops, ref, scale, [Case("pad columns of every bias row", [("bias", (ALL, ALL, slice(S, None)))], mask()),
                             Case("one bias element", [("bias", (hb, i, j))], mask(ALL, i, cols))]


def attention_d512_family(B, T, dtype):
    rnd = rounder(dtype)
    D = 512
    ops = dict(q=rnd(B, T, D, seed=34), k=rnd(B, T, D, seed=35), v=rnd(B, T, D, seed=36))

    def ref(o):
        return ref_attention_d512(o["q"], o["k"], o["v"])

    def mask(*idx):
        m = torch.zeros(B, T, D, dtype=torch.bool)
        if idx:
            m[idx] = True
        return m
    b0, i = B - 1, T // 2 + 1
    soft = mask(b0, slice(i // 64 * 64, min(T, i // 64 * 64 + 64)))
    soft[b0, i] = False
    return ops, ref, [Case("image 1 poisoned", [("q", (1,)), ("k", (1,)), ("v", (1,))], mask(1)),
                      Case("one K element", [("k", (b0, T - 2, 3))], mask(b0)),
                      Case("one V element", [("v", (b0, T - 2, 509))], mask(b0, ALL, 509)),
                      Case("one Q element", [("q", (b0, i, 7))], mask(b0, i), soft=soft)]


def ln_modulate_family(B, S, h, dtype):
    rnd = rounder(dtype)
    ops = dict(x=rnd(B, S, h, seed=40, scale=3.0, shift=0.5), shift=rnd(B, h, seed=41), scale=rnd(B, h, seed=42, scale=0.5))

    def ref(o):
        return ref_ln_modulate(o["x"], o["shift"], o["scale"])

    def mask(*idx):
        m = torch.zeros(B, S, h, dtype=torch.bool)
        if idx:
            m[idx] = True
        return m
    c = h - 2  # in the last (for h = 2432: partial) 64-lane chunk
    return ops, ref, [Case("margins only", [], mask()),
                      Case("one x element", [("x", (1, 5, c))], mask(1, 5)),
                      Case("one x element of the last row", [("x", (B - 1, S - 1, 0))], mask(B - 1, S - 1)),
                      Case("one shift element of image 1", [("shift", (1, c))], mask(1, ALL, c)),
                      Case("one scale element of image 0", [("scale", (0, c))], mask(0, ALL, c))]


def qk_norm_rope_family(D, dtype, B=2, H=3, S_t=5, gh=4, gw=6):
    """test_qk_norm_rope's shape: S = 5 + 24 tokens, row s of an image rotates by table row s"""
    rnd = rounder(dtype)
    S, h = S_t + gh * gw, H * D
    s = torch.arange(S, dtype=torch.float32)[:, None]
    i = torch.arange(D // 2, dtype=torch.float32)[None, :]
    ang = 0.37 * s / (1.0 + 0.11 * i) + 0.05 * i
    ops = dict(qkv=rnd(B, S, 3 * h, seed=50), qw=rnd(D, seed=51, scale=0.1, shift=1.0), kw=rnd(D, seed=52, scale=0.1, shift=1.0),
               tab=torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).contiguous())

    def ref(o):
        return ref_qk_norm_rope(o["qkv"], H, D, o["qw"], o["kw"], o["tab"])

    def mask(*idx):
        m = torch.zeros(B, S, 3 * h, dtype=torch.bool)
        if idx:
            m[idx] = True
        return m
    p, pair = 11, D // 2 - 2
    pair_cols = torch.tensor([part * h + hh * D + 2 * pair + e for part in (0, 1) for hh in range(H) for e in (0, 1)])
    kcols = torch.tensor([h + hh * D + 2 * 3 + e for hh in range(H) for e in (0, 1)])
    m_tab = mask()
    m_tab[:, p, pair_cols] = True
    m_kw = mask()
    m_kw[:, :, kcols] = True
    return ops, ref, [Case("one q element", [("qkv", (1, 7, 1 * D + 9))], mask(1, 7, slice(D, 2 * D))),
                      Case("one k element", [("qkv", (0, S - 1, h + 2 * D + 1))], mask(0, S - 1, slice(h + 2 * D, h + 3 * D))),
                      Case("one v element", [("qkv", (1, 0, 2 * h + 5))], mask(1, 0, 2 * h + 5)),
                      Case("one rope table entry", [("tab", (p, pair, 1))], m_tab),
                      Case("one key norm weight", [("kw", (6,))], m_kw)]


GN_SHAPE = (2, 8, 8, 64, 32)  # B, H, W, C, G


def groupnorm_family(dtype, table=False, silu=True):
    rnd = rounder(dtype)
    B, H, W, C, G = GN_SHAPE
    ops = dict(x=rnd(B, H, W, C, seed=60, scale=2.0, shift=0.7), gamma=rnd(C, seed=61, scale=0.1, shift=1.0), beta=rnd(C, seed=62, scale=0.1))
    cg, c = C // G, C - 3
    grp = slice(c // cg * cg, c // cg * cg + cg)
    if table:
        def ref(o):
            return ref_groupnorm_table(o["x"], o["gamma"], o["beta"], G)

        def mask(*idx):
            m = torch.zeros(B, 2, C, dtype=torch.bool)
            if idx:
                m[idx] = True
            return m
        return ops, ref, [Case("one x element", [("x", (1, 7, 7, c))], mask(1, ALL, grp)),
                          Case("one gamma element", [("gamma", (c,))], mask(ALL, ALL, c)),
                          Case("one beta element", [("beta", (c,))], mask(ALL, 1, c))]

    def ref(o):
        return ref_groupnorm(o["x"], o["gamma"], o["beta"], G, silu=silu)

    def mask(*idx):
        m = torch.zeros(B, H, W, C, dtype=torch.bool)
        if idx:
            m[idx] = True
        return m
    return ops, ref, [Case("one x element of image 0", [("x", (0, 7, 7, c))], mask(0, ALL, ALL, grp)),
                      Case("one x element of image 1", [("x", (1, 0, 0, 1))], mask(1, ALL, ALL, slice(0, cg))),
                      Case("one gamma element", [("gamma", (c,))], mask(ALL, ALL, ALL, c)),
                      Case("one beta element", [("beta", (5,))], mask(ALL, ALL, ALL, 5))]


def conv_pixels(H, W, tile=16):
    """(label, b, y, x): an image corner, a tile seam (both sides of the seam between two tiles of ``tile`` pixels, where the image has one), the last
    row of image 0 and the first row of image 1"""
    seam = tile if min(H, W) > tile else min(H, W) // 2
    return [("corner of image 0", 0, 0, 0), ("far corner of image 1", 1, H - 1, W - 1), ("tile seam", 0, seam - 1, seam),
            ("last row of image 0", 0, H - 1, W // 2), ("first row of image 1", 1, 0, W // 2 - 1)]


def conv_family(B, H, W, C, O, form, dtype, res=False, C2=0, act=None, tile=16):
    """3 x 3 convolution: ``H x W`` is the INPUT size; ``act`` (name -> activation in front of the conv, built from the clean input's statistics) for
    the fused norm -> silu -> conv form.  One channel of one pixel is poisoned, in the last 64-channel chunk."""
    rnd = rounder(dtype)
    Ho, Wo = (2 * H, 2 * W) if form == "up" else (H // 2, W // 2) if form == "s2" else (H, W)
    ops = dict(x=rnd(B, H, W, C, seed=80, scale=1.5, shift=0.3), w=rnd(O, 3, 3, C, seed=83, scale=0.05), b=rnd(O, seed=84, scale=0.1))
    if res:
        ops["res"] = rnd(B, Ho, Wo, O, seed=85)
    if C2:
        ops.update(x2=rnd(B, Ho, Wo, C2, seed=86), ws=rnd(O, C2, seed=87, scale=0.05), bs=rnd(O, seed=88, scale=0.1))

    def ref(o):
        return ref_conv(o["x"], o["w"], o["b"], form, o.get("res"), act, o.get("x2"), o.get("ws"), o.get("bs"))

    def full(m3):
        return m3[..., None].expand(B, Ho, Wo, O).clone()
    cases = [Case(f"one input channel at the {label}", [("x", (b, y, x, C - 2))], full(conv_footprint((B, H, W), form, b, y, x)))
             for label, b, y, x in conv_pixels(H, W, tile)]
    m1 = torch.zeros(B, Ho, Wo, dtype=torch.bool)
    m1[1] = True
    cases.append(Case("image 1 poisoned", [("x", (1,))], full(m1)))
    if res:
        m = torch.zeros(B, Ho, Wo, O, dtype=torch.bool)
        m[0, Ho - 1, 3, O - 1] = True
        cases.append(Case("one residual element", [("res", (0, Ho - 1, 3, O - 1))], m))
    if C2:
        m = torch.zeros(B, Ho, Wo, dtype=torch.bool)
        m[1, 0, Wo - 1] = True
        cases.append(Case("one shortcut input element", [("x2", (1, 0, Wo - 1, C2 - 1))], full(m)))
    return ops, ref, cases


def softmax_family(dtype, rows=64, cols=256):
    rnd = rounder(dtype)
    ops = dict(x=rnd(rows, cols, seed=70, scale=3.0))
    m = torch.zeros(rows, cols, dtype=torch.bool)
    m[rows - 1] = True
    return ops, (lambda o: torch.softmax(o["x"], -1)), [Case("one element", [("x", (rows - 1, cols - 1))], m)]


def transpose_family(dtype, rows=64, cols=256):
    rnd = rounder(dtype)
    ops = dict(x=rnd(rows, cols, seed=70, scale=3.0))
    m = torch.zeros(cols, rows, dtype=torch.bool)
    m[cols - 1, 3] = True
    return ops, (lambda o: o["x"].t().contiguous()), [Case("one element", [("x", (3, cols - 1))], m)]


def patchify_family(flux, n_img=2, Hl=8, Wl=12, C=16, p=2):
    """dk_latent_to_tokens, then dk_euler_cfg_step, at test_patchify_and_euler_step's shape with CFG on.  Outputs: ``tok0`` [2 n_img, S_i, F] (the
    patchified latent, both CFG copies), ``x`` [n_img, Hl, Wl, C] (the Euler step of the latent from ``out`` [2 n_img, S_i, F]) and ``tok`` (the
    patchified NEW latent, which the step writes for the next iteration).

    Hand-written reference: the oracle patchifies through a Linear with an identity weight (test_patchify_and_euler_step), and 0 * NaN = NaN smears
    one poisoned latent element over its whole token there.  The operation is a permutation, so the patch order is taken from the oracle ONCE, on a
    tensor of element indices (finite), and applied to the values as a gather."""
    from diffusionkit_amd.config import tiny_flux, tiny_sd3
    from oracle.mmdit import OracleMMDiT
    S_i, F = (Hl // p) * (Wl // p), p * p * C
    orc = OracleMMDiT(tiny_flux() if flux else tiny_sd3(),
                      {"x_embedder.proj.weight": torch.eye(F).reshape(F, *((1, 1, F) if flux else (p, p, C))), "x_embedder.proj.bias": torch.zeros(F)}, Prec())
    ops = dict(x=torch.randn(n_img, Hl, Wl, C, generator=torch.Generator().manual_seed(80)),
               out=rounder(torch.bfloat16)(2 * n_img, S_i, F, seed=81))
    sigma, sigma_next, wgt = 0.75, 0.5, 5.0
    index = torch.arange(n_img * Hl * Wl * C, dtype=torch.float32).reshape(n_img, Hl, Wl, C)
    where = orc._patch_embed(index).long()  # [n_img, S_i, F]: which latent element each token feature is
    assert torch.equal(torch.sort(where.reshape(-1))[0], torch.arange(index.numel()))  # a permutation

    def patch(x):
        t = x.reshape(-1)[where]
        return torch.cat([t, t])

    def ref(o):
        u = torch.empty(2 * n_img * Hl * Wl * C)
        u[torch.cat([where, where + index.numel()]).reshape(-1)] = o["out"].reshape(-1)  # (unpatchify: the inverse permutation, per CFG copy)
        u = u.reshape(2 * n_img, Hl, Wl, C)
        den, den_neg = o["x"] - u[:n_img] * sigma, o["x"] - u[n_img:] * sigma
        den = den_neg + wgt * (den - den_neg)
        x_new = o["x"] + (o["x"] - den) / sigma * (sigma_next - sigma)
        return dict(tok0=patch(o["x"]), x=x_new, tok=patch(x_new))

    def hands(flat):
        mx = (index == float(flat))
        mt = (where == int(flat))
        assert int(mx.sum()) == 1 and int(mt.sum()) == 1
        return mx, torch.cat([mt, mt])
    mx, mt = hands(index[1, 5, 7, 9])
    cases = [Case("one latent element", [("x", (1, 5, 7, 9))], dict(tok0=mt, x=mx, tok=mt))]
    # one model output element of the conditional copy (image 0) and one of the unconditional copy (image 1): exactly one latent element each
    for copy, b, t, f in ((0, 0, 3, 17), (1, 1, S_i - 1, F - 1)):
        mx, mt = hands(where[b, t, f])
        cases.append(Case(f"one model output element of CFG copy {copy}", [("out", (copy * n_img + b, t, f))],
                          dict(tok0=torch.zeros_like(mt), x=mx, tok=mt)))
    return ops, ref, (sigma, sigma_next, wgt), cases


# ---- fused GEMM tails (tests/_fused_cases.py) ---------------------------------------------------------------------------------------------
def row_index(M, seg_len, seg_stride):
    m = torch.arange(M)
    return (m // seg_len) * seg_stride + m % seg_len


def smallest(cases, size, keep=lambda c: True):
    return min((c for c in cases if keep(c)), key=size)


def pair_family(c):
    """grouped image (a) + text (b) pair on a joint [B, S_t + S_i + gap] buffer: output = the whole C buffer"""
    from tests import _fused_cases as fc
    rnd = rounder(torch.bfloat16)
    B, S_t, S_i, N, K, epi = c["B"], c["S_t"], c["S_i"], c["N"], c["K"], c["epi"]
    S = S_t + S_i + fc.JOINT_GAP
    call = fc.pair_call(c)
    ws = 1.0 / math.sqrt(K)
    ops = dict(A=rnd(B * S, K, seed=10), Wa=rnd(N, K, seed=11, scale=ws), Wb=rnd(N, K, seed=12, scale=ws), bias_a=rnd(1, N, seed=13, scale=0.3),
               bias_b=rnd(1, N, seed=14, scale=0.3), gate_a=rnd(B, 2 * N, seed=15), gate_b=rnd(B, 2 * N, seed=16), C=rnd(*call.buffers["C"], seed=17))
    rows = {"a": S_t + row_index(B * S_i, S_i, S), "b": row_index(B * S_t, S_t, S)}

    def ref(o):
        out = o["C"].clone()
        for sfx, seg, g0 in (("a", S_i, 0), ("b", S_t, N)):
            r = rows[sfx]
            acc = o["A"][r] @ o["W" + sfx].t() + o["bias_" + sfx]
            if epi == fc.EPI_GELU:
                acc = om.gelu_erf(acc, Prec())
            elif epi == fc.EPI_GATE_RES:
                acc = o["C"][r] + o["gate_" + sfx][:, g0:g0 + N].repeat_interleave(seg, 0) * acc
            out[r] = acc
        return out

    def case(sfx, label):
        m = torch.zeros(call.buffers["C"], dtype=torch.bool)
        m[rows[sfx]] = True
        poison = [("A", (rows[sfx],)), ("W" + sfx, (ALL,)), ("bias_" + sfx, (ALL,))]
        if epi == fc.EPI_GATE_RES:
            poison += [("gate_" + sfx, (ALL,)), ("C", (rows[sfx],))]
        return Case(label, poison, m)
    return call, ops, ref, [case("b", "the whole text operand"), case("a", "the whole image operand")]


def knorm_family(c):
    """QKNorm + RoPE in the GEMM tail: output = the M written rows [M, 3h] of C"""
    from tests import _fused_cases as fc
    h, D, seg_len = c["h"], c["D"], c["seg_len"]
    M = c["n_seq"] * seg_len
    call = fc.knorm_call(c)
    ops = fc.knorm_inputs(c)

    def ref(o):
        return fc.knorm_oracle(c, o, o["A"] @ o["W"].t() + o["bias"], Prec())
    m_row = torch.zeros(M, 3 * h, dtype=torch.bool)
    row = seg_len  # position 0 of the second sequence: inside a tile that straddles the sequences
    m_row[row] = True
    d = 10
    pair = (d // 2 * 2, d // 2 * 2 + 1) if c["table"] else (d,)
    m_kw = torch.zeros(M, 3 * h, dtype=torch.bool)
    for hh in range(h // D):
        for e in pair:
            m_kw[:, h + hh * D + e] = True
    rows = row_index(M, call.d["c_seg_len"], call.d["c_seg_stride"])
    return call, ops, ref, rows, [Case("one A row", [("A", (row,))], m_row), Case("one key norm weight", [("kn_w", (0, d))], m_kw)]


def split_family(c):
    """column split: outputs C [M, n1] (bias) and C2 [M, n2] (gelu)"""
    from tests import _fused_cases as fc
    rnd = rounder(torch.bfloat16)
    M, K, n1, n2 = c["M"], c["K"], c["n1"], c["n2"]
    call = fc.split_call(c)
    seg_len, seg_stride = c.get("seg") or (M, 0)
    rows = row_index(M, seg_len, seg_stride)
    ops = dict(A=rnd(*call.buffers["A"], seed=1), W=rnd(n1 + n2, K, seed=2, scale=0.06), bias=rnd(1, n1 + n2, seed=3, scale=0.3))

    def ref(o):
        acc = o["A"][rows] @ o["W"].t() + o["bias"]
        return dict(C=acc[:, :n1], C2=om.gelu_erf(acc[:, n1:], Prec()))

    def masks(r=None, c1=None, c2=None):
        m1, m2 = torch.zeros(M, n1, dtype=torch.bool), torch.zeros(M, n2, dtype=torch.bool)
        if r is not None:
            m1[r], m2[r] = True, True
        if c1 is not None:
            m1[:, c1] = True
        if c2 is not None:
            m2[:, c2] = True
        return dict(C=m1, C2=m2)
    return call, ops, ref, rows, [Case("one A element of the last row", [("A", (int(rows[M - 1]), K - 1))], masks(r=M - 1)),
                                  Case("one W element of the second range", [("W", (n1 + n2 - 1, 0))], masks(c2=n2 - 1)),
                                  Case("one bias element of the first range", [("bias", (0, n1 - 1))], masks(c1=n1 - 1))]


def attention_q_family(c):
    """QKNorm + RoPE of the queries in the attention Q load (tests/_fused_cases.py: ATTN_Q_CASES): the q columns of one head of one row are poisoned"""
    from tests import _fused_cases as fc
    rnd = rounder(torch.bfloat16)
    B, H, S, D, split = c["B"], c["H"], c["S"], c["D"], c["split"]
    h = H * D
    ops = dict(qkv=rnd(B, S, 3 * h, seed=120), qa=rnd(D, seed=121, scale=0.05, shift=0.5), qb=rnd(D, seed=122, scale=0.05, shift=1.5))
    tab = fc.rope_table_for("angle", S, D) if c["rope"] else None

    def ref(o):
        q, k, v = split_heads(o["qkv"], H, D)
        if c["norm"]:
            q = om.rms_norm(q, torch.where((torch.arange(S) < split)[:, None], o["qa"][None, :], o["qb"][None, :]), fc.KN_EPS, Prec())
        if tab is not None:
            q = om.rope_apply(q, tab, Prec())
        return om.sdpa(q, k, v, 1.0 / math.sqrt(D), Prec()).transpose(1, 2).reshape(B, S, h)
    return ops, tab, ref


def q_head_case(B, H, S, D, QB):
    """one head's q of one row poisoned: that row of that head is NaN; soft = the other rows of its query block, same head"""
    h = H * D
    b0, hh, i = B - 1, H - 1, S // 2 + 1
    head = slice(hh * D, (hh + 1) * D)
    m = torch.zeros(B, S, h, dtype=torch.bool)
    m[b0, i, head] = True
    soft = torch.zeros(B, S, h, dtype=torch.bool)
    soft[b0, i // QB * QB:min(S, i // QB * QB + QB), head] = True
    soft[b0, i] = False
    return Case("one head's q of one row", [("qkv", (b0, i, head))], m, soft=soft)


# ---- fp8 ---------------------------------------------------------------------------------------------------------------------------
def assert_mx8_quantiser_footprint(clean_q, clean_e, got_q, got_e, r, c, what):
    """dk_quantize_mx8 with x[r, c] = NaN.  Hand-written, because neither restatement of the block maximum propagates NaN: oracle.fp8.mx8_scale_exponent
    works on the bit pattern of amax (a NaN's exponent field overflows the int32 sum and the clamp returns 1, so the block's other 31 bytes saturate),
    and the device takes the maximum with fmaxf, IEEE 754 maxNum, which returns the number.  What the operation's data dependency does fix:
    the poisoned element's own byte is an e4m3 NaN; no NaN byte outside the 32 bytes of block (r, c / 32); every byte outside that block and every
    scale but the block's own equals the clean run's."""
    clean_q, clean_e, got_q, got_e = (t.detach().cpu() for t in (clean_q, clean_e, got_q, got_e))
    blk = torch.zeros(clean_q.shape, dtype=torch.bool)
    blk[r, c // 32 * 32:c // 32 * 32 + 32] = True
    assert not bool(nan_mask(clean_q).any()), f"{what}: NaN bytes in the clean run"
    assert bool(nan_mask(got_q)[r, c]), f"{what}: byte ({r}, {c}) is not a NaN byte (the poison was not read)"
    leak = nan_mask(got_q) & ~blk
    assert not bool(leak.any()), f"{what}: {int(leak.sum())} NaN bytes outside the block, first at {_first(leak)}"
    diff = (got_q != clean_q) & ~blk
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} bytes outside the block differ, first at {_first(diff)}"
    sd = got_e != clean_e
    sd[r, c // 32] = False
    assert not bool(sd.any()), f"{what}: {int(sd.sum())} scales of other blocks differ, first at {_first(sd)}"


def chosen_fused_cases():
    """the smallest case of each table of tests/_fused_cases.py that still launches the fused form: (column split, image + text pair with gate +
    residual, QKNorm + RoPE tail with query norm, table and two sequences, query norm + RoPE in the attention Q load, MX-fp8 output copy)"""
    from tests import _fused_cases as fc
    fused = lambda c: c["expect"][0] == 1
    return dict(split=smallest(fc.SPLIT_CASES, lambda c: c["M"] * (c["n1"] + c["n2"]), fused),
                pair=smallest(fc.PAIR_CASES, lambda c: c["B"] * (c["S_t"] + c["S_i"]) * c["N"], lambda c: c["epi"] == fc.EPI_GATE_RES),
                knorm=smallest(fc.KNORM_CASES, lambda c: c["n_seq"] * c["seg_len"] * c["h"],
                               lambda c: fused(c) and c["qn"] and c["table"] and c["n_seq"] > 1),
                attn_q=smallest(fc.ATTN_Q_CASES, lambda c: c["B"] * c["H"] * c["S"] * c["D"], lambda c: c["norm"] and c["rope"]),
                attn_o8=smallest(fc.ATTN_O8_CASES, lambda c: c["B"] * c["H"] * c["S"] * c["D"]))


def gn_act(x_clean, gamma, beta, G, eps=1e-5):
    """the activation in front of a fused norm -> silu -> conv whose GroupNorm table was built from the CLEAN input: per-channel scale and shift, SiLU --
    a NaN pixel-channel of the conv's input stays that one element"""
    tab = ref_groupnorm_table(x_clean, gamma, beta, G, eps)

    def act(x):
        y = x * tab[:, 0][:, None, None] + tab[:, 1][:, None, None]
        return y * torch.sigmoid(y)
    return act


def tile_mask(pixel_mask, tile=16):
    """[B, H, W] bool -> [B, (H / tile) * (W / tile)]: the 16 x 16-pixel tiles (index ty * (W / 16) + tx inside an image: conv_halo.hip:71-74,
    conv256v4.hip:55-58) that hold a marked pixel -- the entries of the output-statistics partials [B, tiles, G, 2] such a pixel reaches"""
    B, H, W = pixel_mask.shape
    return pixel_mask.reshape(B, H // tile, tile, W // tile, tile).any(dim=4).any(dim=2).reshape(B, -1)
