"""The launch forms only the MMDiT engine issues -- column split, grouped image + text pair, QKNorm + RoPE in the GEMM tail and in the attention
kernels' Q load, the MX-fp8 copy of the attention output -- each against a plain CPU reference of THAT operation (fp32, the oracle's own rms_norm /
rope_apply / rope_table / gelu_erf / sdpa on the same seeded, bf16-representable inputs), element by element.  Through the model these forms are only
seen behind attention and the residual stream, where a wrong position, weight, head or bias of one stream is diluted below the block-level bounds.

The cases live in tests/_fused_cases.py; tests/test_dispatch_plan.py checks on the CPU that each takes the path (fused / grouped launch of the kernel
it names, or the expansion) it claims.  Where a second device path with the same rounding points exists it is compared as a SECOND assertion.

Bounds (none is taken from the kernels under test):
  TOL_SINGLE_OP, 0.02 * max|ref| + 1e-2      one fp32-accumulated result rounded once to bf16 (tests/_util.py, test_gpu_ops.py)
  torch.equal                                 same kernel, same K order per element (the contract test_gemm_v4_equals_v3 relies on)
  K-split bounds                              test_gemm_small_launch_is_split_automatically
  |diff| <= 2^-6 * max|ref over the row's head|   fused norm + rotation: a bf16 ulp is at most 2^-7 of the value -- one flipped ulp of the larger partner of
                                              a rotated couple on the way in, one on the output rounding; a wrong position / weight / head is an error of the
                                              order of the value itself
  share of differing elements < 1 %           fused tail against the stand-alone pass (other order of the head's squares): tests/test_fused_reference_cpu.py
  rel_l2 < 6e-3, max_abs < 0.03               the project's attention bounds
Every test prints its measured figures."""
import math

import pytest
import torch

from oracle import fp8 as o8
from oracle import mmdit as om
from oracle.mmdit import Prec
from tests import _fp8 as f8
from tests import _fused_cases as fc
from tests._util import BF, TOL_SINGLE_OP, bf16r, max_abs, randn, rel_l2
from tests._fused_cases import SHARE_CAP, head_bound_ok, norm_columns_ok, projection

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def ids(c):
    return c["id"]


def upload(call, host, dev, ws=None):
    """device buffers of a Call: ``host`` tensors where given (fp32 values -> bf16; the rope table stays fp32), sentinel-filled otherwise"""
    bufs = {}
    for name, shape in call.buffers.items():
        if name == "ws":
            bufs[name] = ws
        elif shape[0] == "f32":
            bufs[name] = host[name].to(dev, torch.float32).contiguous()
            assert bufs[name].numel() == shape[1], (name, bufs[name].shape, shape)
        elif name in host:
            assert tuple(host[name].shape) == tuple(shape), (name, host[name].shape, shape)
            bufs[name] = host[name].to(dev, BF).contiguous()
        else:
            bufs[name] = torch.full(shape, SENTINEL, dtype=BF, device=dev)
    return bufs


def launch(call, bufs):
    from diffusionkit_amd import ops
    try:
        for k, v in call.tune.items():
            ops.tune(k, v)
        ops.gemm_fused_call(*fc.resolve(call, lambda name: bufs[name].data_ptr(), bufs["ws"].numel() if bufs.get("ws") is not None else 0))
    finally:
        for k in fc.TUNE_KEYS:
            ops.tune(k, -1)


def row_index(M, seg_len, seg_stride):
    m = torch.arange(M)
    return (m // seg_len) * seg_stride + m % seg_len


def single_op_bounds(ref, got, what):
    r, m = rel_l2(ref, got), max_abs(ref, got)
    print(f"[{what}] rel_l2 {r:.3e} (< {TOL_SINGLE_OP:.0e}), max_abs {m:.3e} (< {0.02 * float(ref.abs().max()) + 1e-2:.3e})")
    assert r < TOL_SINGLE_OP, what
    assert m < 0.02 * float(ref.abs().max()) + 1e-2, what


def untouched(buf, rows, cols, what):
    """everything of ``buf`` outside rows x cols still holds the sentinel"""
    mask = torch.ones(buf.shape, dtype=torch.bool)
    mask[rows[:, None], cols[None, :]] = False
    assert bool((buf.float().cpu()[mask] == SENTINEL).all()), what


# ---- a. column split ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.SPLIT_CASES, ids=ids)
def test_column_split(dev, case):
    """One read of A: columns [0, n1) + bias -> C, gelu(columns [n1, n1 + n2) + bias) -> a column window of the wider C2 (its own pitch); ragged M, two
    row segments with a straddling tile, a half column tile at the end of the second output.  Bytes outside the two windows and rows behind M
    stay untouched; the fused launch equals two plain launches on the same kernel bit for bit."""
    call = fc.split_call(case)
    M, K, n1, n2 = case["M"], case["K"], case["n1"], case["n2"]
    seg_len, seg_stride = case.get("seg") or (M, 0)
    rows = row_index(M, seg_len, seg_stride)
    host = dict(A=randn(*call.buffers["A"], seed=1), W=randn(n1 + n2, K, seed=2, scale=0.06), bias=randn(1, n1 + n2, seed=3, scale=0.3))
    bufs = upload(call, host, dev)
    launch(call, bufs)
    acc = bf16r(host["A"][rows] @ host["W"].t() + host["bias"])
    c2_col0 = call.side["C2"][1]
    got1, got2 = bufs["C"].float().cpu()[rows, :n1], bufs["C2"].float().cpu()[rows, c2_col0:c2_col0 + n2]
    single_op_bounds(acc[:, :n1], got1, f"split {case['id']} C")
    single_op_bounds(om.gelu_erf(acc[:, n1:], Prec()), got2, f"split {case['id']} C2")
    untouched(bufs["C"], rows, torch.arange(n1), "C outside its window")
    untouched(bufs["C2"], rows, c2_col0 + torch.arange(n2), "C2 outside its window")
    # second assertion: two plain launches over the two column ranges
    sep = upload(call, host, dev)
    for single in fc.split_single_calls(case):
        launch(single, sep)
    assert torch.equal(sep["C"], bufs["C"]) and torch.equal(sep["C2"], bufs["C2"]), "fused != two launches of the same kernel"


# ---- b. grouped pair ------------------------------------------------------------------------------------------------------------------
def pair_inputs(c, call):
    N, K, B = c["N"], c["K"], c["B"]
    ws = 1.0 / math.sqrt(K)
    host = dict(A=randn(*call.buffers["A"], seed=10), Wa=randn(N, K, seed=11, scale=ws), Wb=randn(N, K, seed=12, scale=ws),
                bias_a=randn(1, N, seed=13, scale=0.3), bias_b=randn(1, N, seed=14, scale=0.3),
                gate_a=randn(B, 2 * N, seed=15), gate_b=randn(B, 2 * N, seed=16))
    if c["epi"] == fc.EPI_GATE_RES:  # C aliases the residual
        host["C"] = randn(*call.buffers["C"], seed=17)
        host["C"][B * (c["S_t"] + c["S_i"] + fc.JOINT_GAP):] = SENTINEL
        for b in range(B):
            s0 = b * (c["S_t"] + c["S_i"] + fc.JOINT_GAP) + c["S_t"] + c["S_i"]
            host["C"][s0:s0 + fc.JOINT_GAP] = SENTINEL
    return host


@pytest.mark.parametrize("case", fc.PAIR_CASES, ids=ids)
def test_grouped_pair(dev, case):
    """The image rows and the text rows of a joint [B, S_t + S_i (+ gap), .] buffer as ONE launch: own A rows, W, bias, gate, row maps and M per problem
    (gate + residual: C aliases the residual, the o_proj call of post_sdpa).  Each problem against its own oracle; the gap rows and the rows behind the
    buffer's last batch row untouched; and against the two single launches (gemm256v3.hip, which gemm256v4.hip equals bit for bit): torch.equal, or
    the K-split bounds where the rule cuts the pair along K (then the flag region of the workspace is left zero)."""
    from diffusionkit_amd import ops
    call = fc.pair_call(case)
    B, S_t, S_i, N, epi = case["B"], case["S_t"], case["S_i"], case["N"], case["epi"]
    S = S_t + S_i + fc.JOINT_GAP
    host = pair_inputs(case, call)
    ws = ops.gemm_workspace(dev) if case.get("ws") else None
    bufs = upload(call, host, dev, ws)
    launch(call, bufs)
    got = bufs["C"].float().cpu()
    gen = torch.Generator().manual_seed(5)
    cols = torch.sort(torch.randperm(N, generator=gen)[:case["ref_cols"]])[0] if case.get("ref_cols") else torch.arange(N)
    written = []
    for sfx, row0, seg, g0 in (("a", S_t, S_i, 0), ("b", 0, S_t, N)):
        rows = row0 + row_index(B * seg, seg, S)
        written.append(rows)
        o = bf16r(host["A"][rows] @ host["W" + sfx][cols].t() + host["bias_" + sfx][:, cols])
        if epi == fc.EPI_GELU:
            ref = om.gelu_erf(o, Prec())
        elif epi == fc.EPI_GATE_RES:
            gate = host["gate_" + sfx][:, g0:g0 + N][:, cols].repeat_interleave(seg, 0)
            ref = host["C"][rows][:, cols] + bf16r(gate * o)
        else:
            ref = o
        single_op_bounds(ref, got[rows][:, cols], f"pair {case['id']} problem {sfx}")
    untouched(bufs["C"], torch.cat(written), torch.arange(N), "rows of neither stream / behind the last batch row")
    if ws is not None:
        assert int(ws[-4096:].sum()) == 0  # the flag region is left zero
    # second assertion: the two problems one after the other
    singles = fc.pair_call(case, grouped=False)
    sep = upload(singles, host, dev)
    launch(singles, sep)
    if case.get("cut"):
        gs, ss = got, sep["C"].float().cpu()
        share = float((gs != ss).float().mean())
        bound = 0.02 * float(gs.abs().max()) + 1e-2
        print(f"[pair {case['id']}] cut along K against whole tiles: max_abs {max_abs(ss, gs):.3e} (<= {bound:.3e}), differing share {share:.3e} (< 0.05)")
        assert not torch.equal(sep["C"], bufs["C"]), "the pair was expected to be cut along K (other summation order)"
        assert max_abs(ss, gs) <= bound and share < 0.05
    else:
        assert torch.equal(sep["C"], bufs["C"]), "grouped != two single launches"


# ---- c. QKNorm + RoPE in the GEMM tail --------------------------------------------------------------------------------------------------
def two_paths_ok(fused, separate, h, D, what):
    """fused tail against plain projection + stand-alone pass: identical GEMM bits, only the order of a head's squares differs"""
    f, s = fused[:, :2 * h], separate[:, :2 * h]
    worst = head_bound_ok(s, f, D, f"{what} fused against stand-alone pass")
    share = float((f != s).float().mean())
    print(f"[{what}] fused tail against the stand-alone pass: differing share {share:.3e} (< {SHARE_CAP}), worst |diff| / head max {worst:.3e}")
    assert share < SHARE_CAP, what


def standalone_pass(buf, ld, h, D, rows, qw, kw, rope, seg_len, seg_stride, pos_off):
    """dk_qk_norm_rope_bf16 over ``rows`` rows of a [., 3h] buffer starting at ``buf`` (a device address)"""
    from diffusionkit_amd import _lib
    from diffusionkit_amd.engine import _stream
    _lib.check(_lib.load().dk_qk_norm_rope_bf16(buf, ld, 0, h, rows, h // D, D, qw, kw, fc.KN_EPS, rope, seg_len, seg_stride, pos_off, _stream()),
               "dk_qk_norm_rope_bf16")


@pytest.mark.parametrize("case", fc.KNORM_CASES, ids=ids)
def test_qknorm_rope_in_gemm_tail(dev, case):
    """q / k / v projection [M, 3h] whose key columns (and, with qn, query columns, own weight) leave the GEMM normalised and rotated at position
    pos_off + row % seg_len.  Reference: bf16r(x W^T + b), then the oracle's rms_norm and rope_apply with Prec(BF), as test_qk_norm_rope builds it.
    64-column heads: no shipped configuration reaches that branch of the fused tail (SD3.5-large's key columns start at 2432, not a multiple of 256,
    so its projections take the expansion) -- these cases are its only cover.  v columns: the plain projection, bit for bit."""
    call = fc.knorm_call(case)
    h, D, seg_len, n2 = case["h"], case["D"], case["seg_len"], case.get("n2", 0)
    M = case["n_seq"] * seg_len
    t = fc.knorm_inputs(case)
    bufs = upload(call, t, dev)
    launch(call, bufs)
    proj = projection(t["A"], t["W"], t["bias"])
    ref = fc.knorm_oracle(case, t, proj, Prec(BF))
    rows = row_index(M, call.d["c_seg_len"], call.d["c_seg_stride"])
    got = bufs["C"].float().cpu()[rows]
    what = f"knorm {case['id']}"
    norm_columns_ok(ref, got, h, D, what)
    if not case["qn"]:
        single_op_bounds(proj[:, :h], got[:, :h], what + " q (plain)")
    single_op_bounds(proj[:, 2 * h:3 * h], got[:, 2 * h:], what + " v")
    untouched(bufs["C"], rows, torch.arange(3 * h), "rows between the sequences / behind M")
    if n2:
        single_op_bounds(om.gelu_erf(proj[:, 3 * h:], Prec()), bufs["C2"].float().cpu()[rows, :n2], what + " C2")
        untouched(bufs["C2"], rows, torch.arange(n2), "C2 outside its window")
    if case["expect"][0] != 1:
        return  # (the expansion IS the projection followed by the stand-alone pass)
    # second assertion: the same GEMM on the same kernel without the fused tail, then dk_qk_norm_rope_bf16 over its output
    plain = fc.knorm_call(case, fused=False)
    sep = upload(plain, t, dev)
    launch(plain, sep)
    assert torch.equal(sep["C"][:, 2 * h:], bufs["C"][:, 2 * h:]), "v columns differ from the plain projection"
    if n2:
        assert torch.equal(sep["C2"], bufs["C2"])
    q_plain = sep["C"][:, :h].clone()
    c_seg_stride = call.d["c_seg_stride"] or seg_len
    standalone_pass(sep["C"].data_ptr(), 3 * h, h, D, M, sep["qn_w"].data_ptr() if case["qn"] else None, sep["kn_w"].data_ptr(),
                    sep["rope"].data_ptr() if case["table"] else None, seg_len, c_seg_stride, case.get("pos_off", 0))
    if not case["qn"]:
        sep["C"][:, :h] = q_plain  # (the stand-alone pass rotates the queries it does not normalise; the fused tail leaves them alone)
        assert torch.equal(bufs["C"][:, :h], q_plain)
    two_paths_ok(got, sep["C"].float().cpu()[rows], h, D, what)


@pytest.mark.parametrize("case", fc.KNORM_PAIR_CASES, ids=ids)
def test_qknorm_rope_in_gemm_tail_grouped_pair(dev, case):
    """The double block's call: image and text q / k / v projections into a joint [B, S, 3h] buffer as one grouped launch, each stream with its own
    kn_w / qn_w and first position (text 0, image S_t) into one table"""
    call = fc.knorm_pair_call(case)
    B, S_t, S_i, h, D, K = case["B"], case["S_t"], case["S_i"], case["h"], case["D"], case["K"]
    S, N = S_t + S_i + fc.JOINT_GAP, 3 * h
    host = dict(Aa=randn(B * S_i, K, seed=90), Ab=randn(B * S_t, K, seed=91), Wa=randn(N, K, seed=92, scale=1 / math.sqrt(K)),
                Wb=randn(N, K, seed=93, scale=1 / math.sqrt(K)), bias_a=randn(1, N, seed=94, scale=0.3), bias_b=randn(1, N, seed=95, scale=0.3),
                kn_a=bf16r(1.0 + randn(1, D, seed=96, scale=0.1)), qn_a=bf16r(0.6 + randn(1, D, seed=97, scale=0.1)),
                kn_b=bf16r(1.4 + randn(1, D, seed=98, scale=0.1)), qn_b=bf16r(0.8 + randn(1, D, seed=99, scale=0.1)),
                rope=fc.rope_table_for(case["table"], S_t + S_i, D, text_len=S_t))
    bufs = upload(call, host, dev)
    launch(call, bufs)
    got = bufs["C"].float().cpu()
    plain = fc.knorm_pair_call(case, fused=False, grouped=False)
    sep = upload(plain, host, dev)
    launch(plain, sep)
    written = []
    for sfx, row0, seg in (("a", S_t, S_i), ("b", 0, S_t)):
        rows = row0 + row_index(B * seg, seg, S)
        written.append(rows)
        proj = projection(host["A" + sfx], host["W" + sfx], host["bias_" + sfx])
        sub = dict(h=h, D=D, n_seq=B, seg_len=seg, pos_off=row0, table=case["table"], qn=True)
        ref = fc.knorm_oracle(sub, dict(kn_w=host["kn_" + sfx], qn_w=host["qn_" + sfx], rope=host["rope"]), proj, Prec(BF))
        what = f"knorm pair {case['id']} problem {sfx}"
        norm_columns_ok(ref, got[rows], h, D, what)
        single_op_bounds(proj[:, 2 * h:], got[rows][:, 2 * h:], what + " v")
        standalone_pass(sep["C"].data_ptr() + row0 * N * 2, N, h, D, B * seg, sep["qn_" + sfx].data_ptr(), sep["kn_" + sfx].data_ptr(), sep["rope"].data_ptr(),
                        seg, S, row0)
    untouched(bufs["C"], torch.cat(written), torch.arange(N), "rows of neither stream / behind the last batch row")
    assert torch.equal(sep["C"][:, 2 * h:], bufs["C"][:, 2 * h:]), "v columns differ from the plain projections"
    rows = torch.cat(written)
    two_paths_ok(got[rows], sep["C"].float().cpu()[rows], h, D, f"knorm pair {case['id']}")


# ---- d. QKNorm + RoPE of the queries in the attention kernels' Q load ------------------------------------------------------------------------
def attn_tune(case):
    from diffusionkit_amd import ops
    ops.tune("attn", case["mode"])
    ops.tune("attn_split", case.get("attn_split", -1))


def attn_untune():
    from diffusionkit_amd import ops
    ops.tune("attn", -1)
    ops.tune("attn_split", -1)


@pytest.mark.parametrize("case", fc.ATTN_Q_CASES, ids=ids)
def test_query_norm_rope_in_attention_q_load(dev, case):
    """Token s < split of every image is normalised with qn_a, the others with qn_b (0.5 against 1.5: a row on the wrong side is off by 3x), and rotated by
    row s of the table (s, not b * S + s).  Reference: the oracle's rms_norm + rope_apply on q (Prec(BF)), then its sdpa.  Second assertion: the
    stand-alone pass over the q columns (k and v restored) + plain attention on the same kernel; the fused launch may be no further from it than
    twice that path's own distance from the oracle."""
    from diffusionkit_amd import _lib, ops
    B, H, S, D, split = case["B"], case["H"], case["S"], case["D"], case["split"]
    h = H * D
    qkv = randn(B, S, 3 * h, seed=120)
    qa, qb = bf16r(0.5 + randn(D, seed=121, scale=0.05)), bf16r(1.5 + randn(D, seed=122, scale=0.05))
    tab = fc.rope_table_for("angle", S, D) if case["rope"] else None
    scale = 1.0 / math.sqrt(D)
    d_qkv, d_qa, d_qb = qkv.to(dev, BF), qa.to(dev, BF), qb.to(dev, BF)
    d_tab = tab.to(dev) if tab is not None else None
    out = torch.full((B, S, h), SENTINEL, dtype=BF, device=dev)
    base = d_qkv.data_ptr()
    try:
        attn_tune(case)
        desc = dict(q=base, k=base + 2 * h, v=base + 4 * h, out=out, B=B, H=H, S=S, D=D, ld=3 * h, ldo=h, scale=scale,
                    qn_a=d_qa if case["norm"] else None, qn_b=d_qb if case["norm"] else None, qn_split=split, qn_eps=fc.KN_EPS, q_rope=d_tab)
        ops.attention_desc_call(**desc)
        claim = fc.attn_claim(case)  # ... on the kernel and in the key ranges the case names, on THIS device
        plan = ops.attention_plan(workspace_bytes=_lib.load().dk_attention_workspace_bytes(), **desc)
        assert (fc.ATTN_KERNEL_NAMES[plan.kernel], plan.split) == claim, (case["id"], plan.kernel, plan.split, plan.n_cu)
        # the separate path: stand-alone pass over the rows of each side of the split, k / v restored, plain attention
        sep = d_qkv.clone()
        for s0, n, w in ((0, split, d_qa), (split, S - split, d_qb)):
            if n > 0:
                standalone_pass(sep.data_ptr() + s0 * 3 * h * 2, 3 * h, h, D, B * n, w.data_ptr() if case["norm"] else None, None,
                                d_tab.data_ptr() if d_tab is not None else None, n, S, s0)
        sep[..., h:] = d_qkv[..., h:]
        y_sep = ops.attention(sep, H, D)
        y_whole = None
        if claim[1] > 1:  # the key-split jobs: the same fused launch with whole blocks must differ in bits (bf16-rounded partials)
            ops.tune("attn_split", 0)
            y_whole = torch.empty_like(out)
            ops.attention_desc_call(**dict(desc, out=y_whole))
    finally:
        attn_untune()
    P = Prec(BF)
    q, k, v = (qkv[..., i * h:(i + 1) * h].reshape(B, S, H, D).transpose(1, 2) for i in range(3))
    if case["norm"]:
        w_rows = torch.where((torch.arange(S) < split)[:, None], qa[None, :], qb[None, :])  # [S, D]
        q = om.rms_norm(q, w_rows, fc.KN_EPS, P)
    if tab is not None:
        q = om.rope_apply(q, tab, P)
    ref = om.sdpa(q, k, v, scale, Prec()).transpose(1, 2).reshape(B, S, h)
    y = out.float().cpu()
    r, m = rel_l2(ref, y), max_abs(ref, y)
    m_sep, m_two = max_abs(ref, y_sep.float()), max_abs(y_sep.float(), y)
    print(f"[attn q {case['id']}] rel_l2 {r:.3e} (< 6e-3), max_abs {m:.3e} (< 0.03); stand-alone pass + plain attention: {m_sep:.3e} from the oracle, "
          f"{m_two:.3e} from the fused launch (<= {2 * m_sep:.3e})")
    assert r < 6e-3 and m < 0.03
    assert rel_l2(ref, y_sep.float()) < 6e-3
    if y_whole is not None:
        assert not torch.equal(y_whole, out), "attn_split did not select the key-split jobs"
        assert rel_l2(ref, y_whole.float()) < 6e-3 and max_abs(ref, y_whole.float()) < 0.03
    assert m_two <= 2 * m_sep


# ---- e. MX-fp8 copy of the attention output -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.ATTN_O8_CASES, ids=ids)
def test_attention_mx8_output_copy(dev, case):
    """O8 / O8_scales must be EXACTLY the MX-fp8 encoding of the bf16 output of the same launch without O8 ("values rounded to bf16 first, as the separate
    quantiser pass over O sees them", dk_kernels.h); the D = 128 kernels of modes 9 / 10 write it instead of O (O keeps its sentinel), the others write
    O and quantise it.  O8 is a column window [0, H * D) of wider rows (the single block's [attn | gelu] operand): the bytes behind it stay."""
    from diffusionkit_amd import ops
    B, H, S, D = case["B"], case["H"], case["S"], case["D"]
    h, M = H * D, B * S
    ld8 = h + 256
    qkv = randn(B, S, 3 * h, seed=130).to(dev, BF)
    base = qkv.data_ptr()
    kw = dict(q=base, k=base + 2 * h, v=base + 4 * h, B=B, H=H, S=S, D=D, ld=3 * h, ldo=h, scale=1.0 / math.sqrt(D))
    plain = torch.full((B, S, h), SENTINEL, dtype=BF, device=dev)
    out = torch.full((B, S, h), SENTINEL, dtype=BF, device=dev)
    o8b = torch.full((M, ld8), 0xAB, dtype=torch.uint8, device=dev)
    sc = torch.zeros(ops.mx_scale_bytes(M, ld8), dtype=torch.uint8, device=dev)
    try:
        ops.tune("attn", case["mode"])
        ops.tune("attn_split", 0)  # (the key split rounds partial results to bf16; with O8 the launcher never splits)
        ops.attention_desc_call(out=plain, **kw)
        ops.attention_desc_call(out=out, O8=o8b, O8_scales=sc, o8_ld=ld8, o8_rows=M, **kw)
    finally:
        attn_untune()
    y = plain.float().cpu().reshape(M, h)
    assert not bool((y == SENTINEL).all())
    q_ref, e_ref = o8.mx8_encode(y)
    got_q, got_e = o8b.cpu()[:, :h], f8.array_to_scales(sc, M, h, rows=M)
    n_q, n_e = int((got_q != q_ref).sum()), int((got_e != e_ref).sum())
    print(f"[attn o8 {case['id']}] bytes that differ from the encoding of the plain output: {n_q} of {q_ref.numel()}, scales: {n_e} of {e_ref.numel()}")
    assert n_e == 0 and n_q == 0
    assert bool((o8b[:, h:] == 0xAB).all()), "bytes behind the window"
    if case["in_kernel"]:
        assert bool((out == SENTINEL).all()), "O written although the kernel owns the MX-fp8 copy"
    else:
        assert torch.equal(out, plain)
