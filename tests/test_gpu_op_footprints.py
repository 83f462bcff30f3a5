"""NaN footprints of the operators on an MI355X: poison one element (or one region) of an operand with NaN, run the SAME launch on the same buffers
clean and poisoned, and demand that (a) the NaN outputs are exactly the operation's data-dependency footprint, (b) every other output is BIT-identical
to the clean run, (c) the clean run is finite.  Every operand sits inside NaN margins, outputs the caller owns inside sentinel margins, and the margins
must be what they were afterwards.  No tolerance is involved -- except in the one ``soft`` region the attention Q rule allows (below).

What this sees and a whole-tensor rel_l2 on seeded Gaussian data cannot: a kernel that reads data it must not depend on (rows past M or S of a padded
tail tile, the other stream of a joint buffer, the next image behind a conv border, pad columns of a bias table, whatever lies behind a tensor) and masks
it by a multiplication instead of a select or a clamped address; and a localised indexing fault (one tile, one row, one head) that a norm dilutes.

The expectation of a case is ``isnan(reference(poisoned operands))`` with the references of tests/_footprint.py; tests/test_footprint_cpu.py proves on
the CPU that they have exactly the hand-written footprints (which each case carries and which is compared here too).

The attention Q rule (the only use of ``soft``): the deferred rescale of attention2.hip / attention4.hip / attention512.hip is a wave-wide vote
(__all(m_tile - m_run <= threshold)), and a NaN row never votes yes -- its wave's other rows then rescale at every tile, a legitimate other rounding.
So with one Q element poisoned the OTHER rows of the same query block and head are exempt from bit equality: they must be finite and within the oracle
gate of test_attention_kernel_variants (rel_l2 < 6e-3, max_abs < 0.03; fp16: 6e-3 / 8).  The region is capped at one query block x one head, asserted.

The file name sorts behind tests/test_gpu_fullsize.py on purpose (see tests/test_gpu_vae_f16.py)."""
import math

import pytest
import torch

from tests import _footprint as fp
from tests import _fp8 as f8
from tests import _op_launches as L
from tests._util import TOL_SINGLE_OP, rel_l2

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
NAN, SENTINEL = fp.NAN, fp.SENTINEL
PAD = 64  # rows of margin around every guarded tensor


def upload(ops_cpu, dev, dt, dtypes=None):
    """every operand on the device inside NaN margins: name -> (view, guard).  Element type ``dt``, except the fp32 rope tables and ``dtypes``"""
    kinds = dict({"tab": torch.float32, "rope": torch.float32}, **(dtypes or {}))
    return {k: fp.guarded(v.to(dev, kinds.get(k, dt)).contiguous(), PAD) for k, v in ops_cpu.items()}


def restore(bufs, ops_cpu):
    for k, (view, _) in bufs.items():
        view.copy_(ops_cpu[k])


def outputs(y):
    return {k: v.detach().clone().cpu() for k, v in y.items()} if isinstance(y, dict) else y.detach().clone().cpu()


def run_family(dev, dt, ops_cpu, ref, cases, launch, what, soft_gate=None, guards=(), dtypes=None):
    """``launch(views)`` -> output tensor or dict of them.  Clean run, then every case on the same buffers (restored before each launch: launches may work
    in place); the expectation isnan(ref(poisoned)) must equal the case's hand-written mask, the device output must have exactly that footprint."""
    bufs = upload(ops_cpu, dev, dt, dtypes)
    views = {k: v for k, (v, _) in bufs.items()}
    clean = outputs(launch(views))
    ref_clean = ref(ops_cpu)
    n_soft = 0
    for case in cases:
        restore(bufs, ops_cpu)
        for name, idx in case.poison:
            views[name][idx] = NAN
        got = outputs(launch(views))
        want = ref(fp.poisoned(ops_cpu, case))
        for key in (case.hand if isinstance(case.hand, dict) else [None]):
            c, g_, w, h, r = (clean, got, want, case.hand, ref_clean) if key is None else (clean[key], got[key], want[key], case.hand[key], ref_clean[key])
            expect = torch.isnan(w)
            assert torch.equal(expect, h), f"{what}: {case.label}: the reference's footprint is not the hand-written one"
            kw = {}
            if case.soft is not None:
                assert soft_gate is not None, "soft regions are for the attention Q rule only"
                n_soft = int(case.soft.sum())
                assert n_soft <= soft_gate["cap"], f"{what}: soft region of {n_soft} elements exceeds one query block x one head ({soft_gate['cap']})"
                kw = dict(soft=case.soft, soft_ref=r, soft_rel_l2=soft_gate["rel_l2"], soft_max_abs=soft_gate["max_abs"])
            fp.assert_footprint(c, g_, expect, f"{what}: {case.label}" + (f" [{key}]" if key else ""), **kw)
    for k, (_, guard) in bufs.items():
        guard.check(f"{what}: margins of {k}")
    for name, guard in guards:
        guard.check(f"{what}: margins of {name}")
    if n_soft:
        print(f"[footprint] {what}: soft region of the Q case: {n_soft} elements")


tuned = L.tuned  # (ops.tune(key, value) for a block, the defaults afterwards)


def ws_flags_zero(ws):
    assert int(ws[-4096:].sum()) == 0, "the flag region of the K-split workspace was not left zero"


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------
GEMM_FORMS = L.GEMM_FORMS


@pytest.mark.parametrize("epi", ["bias", "gate_res"])
@pytest.mark.parametrize("B,S_t,S_i", fp.GEMM_JOINT_SHAPES)
@pytest.mark.parametrize("form", GEMM_FORMS, ids=lambda f: f[0])
def test_gemm_joint_buffer_text_stream(dev, form, B, S_t, S_i, epi):
    """the text stream of a joint [B, S_t + S_i] buffer (test_gemm_v3_ragged_and_straddling_segments): the image rows between the text segments of A and
    of C / the residual hold NaN and must neither leak nor be written; one A / W / bias / gate / residual element poisons exactly its row / column /
    segment column / element -- the gate's segment map across a tile that straddles two segments included"""
    from diffusionkit_amd import ops
    _, dt, knobs = form
    ops_cpu, ref, cases = fp.gemm_joint_family(B, S_t, S_i, epi, dt)
    ws = ops.gemm_workspace(dev)

    joint = L.gemm_joint(dt, knobs, B, S_t, S_i, epi)

    def launch(v):
        return joint(dict(v, ws=ws))
    run_family(dev, dt, ops_cpu, ref, cases, launch, f"gemm {form[0]} {(B, S_t, S_i)} {epi}")
    ws_flags_zero(ws)


def test_gemm_k_split_finisher_adds_the_last_range(dev):
    """test_gemm_v3_remainder_split's (1024, 768, 640): a NaN in the LAST K range reaches its output row / column -- the finisher really adds the
    producers' slabs -- and nothing else differs from the clean split launch"""
    from diffusionkit_amd import ops
    ops_cpu, ref, cases = fp.gemm_ksplit_family(BF)
    M, N = ops_cpu["res"].shape
    ws = ops.gemm_workspace(dev)
    out, og = fp.guarded(torch.empty(M, N, dtype=BF, device=dev), PAD, SENTINEL)
    plain = {}

    cut, whole = L.gemm_ksplit(1), L.gemm_ksplit(0)

    def launch(v):
        cut(dict(v, out=out, ws=ws))
        if not plain:
            plain["y"] = whole(dict(v, ws=ws))
            assert not torch.equal(plain["y"], out), "gemm_split 1 was expected to cut the remainder tiles along K (other summation order)"
        return out
    run_family(dev, BF, ops_cpu, ref, cases, launch, "gemm K split", guards=[("out", og)])
    ws_flags_zero(ws)


def _fused_launch(call, bufs):
    L.fused(call)(bufs)


def test_fused_pair_streams_are_independent(dev):
    """grouped image + text pair (gate + residual, C aliases the residual): with every operand of one stream poisoned -- its A rows, W, bias, gate and
    residual rows -- the other stream's outputs are bit-identical, the gap rows untouched"""
    case = fp.chosen_fused_cases()["pair"]
    call, ops_cpu, ref, cases = fp.pair_family(case)

    def launch(v):
        _fused_launch(call, v)
        return v["C"]
    run_family(dev, BF, ops_cpu, ref, cases, launch, f"pair {case['id']}")


def test_fused_qknorm_rope_tail(dev):
    """QKNorm + RoPE in the GEMM tail: one A row -> exactly that row of q / k / v (the norm reduces within a row and head); one key norm weight -> that
    rotated column pair of every head of k in every row, q and v bit-identical; rows between the sequences and behind M keep the sentinel"""
    case = fp.chosen_fused_cases()["knorm"]
    call, ops_cpu, ref, rows, cases = fp.knorm_family(case)
    C, cg = fp.guarded(torch.empty(call.buffers["C"], dtype=BF, device=dev), PAD, SENTINEL)
    keep = torch.ones(C.shape[0], dtype=torch.bool)
    keep[rows] = False

    def launch(v):
        C.fill_(SENTINEL)
        _fused_launch(call, dict(v, C=C))
        assert bool((C[keep.to(dev)] == SENTINEL).all()), "rows between the sequences / behind M were written"
        return C[rows.to(dev)]
    run_family(dev, BF, ops_cpu, ref, cases, launch, f"knorm {case['id']}", guards=[("C", cg)])


def test_fused_column_split(dev):
    """column split: one A element -> its row of both outputs; a W element of the second column range -> one column of C2 only; a bias element of the
    first -> one column of C only; bytes outside the two windows keep the sentinel"""
    case = fp.chosen_fused_cases()["split"]
    call, ops_cpu, ref, rows, cases = fp.split_family(case)
    n1, n2, c2_col0 = case["n1"], case["n2"], call.side["C2"][1]
    (C, cg), (C2, c2g) = (fp.guarded(torch.empty(call.buffers[n], dtype=BF, device=dev), PAD, SENTINEL) for n in ("C", "C2"))
    r = rows.to(dev)

    def launch(v):
        C.fill_(SENTINEL)
        C2.fill_(SENTINEL)
        _fused_launch(call, dict(v, C=C, C2=C2))
        for buf, c0, n in ((C, 0, n1), (C2, c2_col0, n2)):
            m = torch.ones(buf.shape, dtype=torch.bool, device=dev)
            m[r[:, None], c0 + torch.arange(n, device=dev)[None, :]] = False
            assert bool((buf[m] == SENTINEL).all()), "bytes outside the output windows were written"
        return dict(C=C[r, :n1], C2=C2[r, c2_col0:c2_col0 + n2])
    run_family(dev, BF, ops_cpu, ref, cases, launch, f"split {case['id']}", guards=[("C", cg), ("C2", c2g)])


# ---- fp8 ----------------------------------------------------------------------------------------------------------------------------
ROWS8, K8 = 384, 384  # tests/test_gpu_fp8_ragged.py


def _act8():
    x = fp.rounder(BF)(ROWS8, K8, seed=801)
    x[:, :K8 // 2] *= 4.0
    return x


def test_quantize_mx8_block_footprint(dev):
    """one NaN element: its own byte is a NaN byte, nothing outside its 32-byte block and no other block's scale changes (why the inside of the block is
    left open: fp.assert_mx8_quantiser_footprint)"""
    from diffusionkit_amd import ops
    x = _act8()
    xd, xg = fp.guarded(x.to(dev, BF), PAD)
    q0, s0 = ops.quantize_mx8(xd)
    e0 = f8.array_to_scales(s0, ROWS8, K8)
    for r, c in ((0, 0), (ROWS8 - 1, K8 - 1), (130, 70)):
        xd.copy_(x)
        xd[r, c] = NAN
        q1, s1 = ops.quantize_mx8(xd)
        fp.assert_mx8_quantiser_footprint(q0, e0, q1, f8.array_to_scales(s1, ROWS8, K8), r, c, f"quantize_mx8 ({r}, {c})")
    xg.check("quantize_mx8: margins of x")


@pytest.mark.parametrize("M", [120, 376])
def test_gemm_fp8_rows_behind_m_and_row_independence(dev, M):
    """rows >= M of the activation bytes (0x7F: e4m3 NaN) and of their scales (0xFF: E8M0 NaN) poisoned: rows [0, M) bit-identical, rows >= M of the
    output keep the sentinel; one NaN byte in row m < M: exactly row m"""
    from diffusionkit_amd import ops
    from diffusionkit_amd.weights import quantize_weight_e4m3
    N = 256
    a8, sa = ops.quantize_mx8(_act8().to(dev, BF))
    qw, wsc = quantize_weight_e4m3(fp.rounder(BF)(N, K8, seed=802, scale=0.02).to(BF))
    w8, wsc = qw.to(dev), wsc.to(dev)
    bias = fp.rounder(BF)(N, seed=803, scale=0.5).to(dev, BF)
    (a8g, ag), (sag, sg) = fp.guarded(a8, PAD, 0x7F), fp.guarded(sa, 1, 0xFF)
    out, og = fp.guarded(torch.empty(ROWS8, N, dtype=BF, device=dev), PAD, SENTINEL)

    def run():
        out.fill_(SENTINEL)
        ops.gemm_fp8(a8g, sag, w8, wsc, bias=bias, M=M, k=K8, out=out)
        assert bool((out[M:] == SENTINEL).all()), "rows >= M were written"
        return out[:M].clone()
    clean = run()
    none = torch.zeros(M, N, dtype=torch.bool)
    a8g[M:] = 0x7F
    r = torch.arange(M, ROWS8)[:, None].expand(ROWS8 - M, K8 // 32)
    kb = torch.arange(K8 // 32)[None, :].expand(ROWS8 - M, K8 // 32)
    sag[f8.scale_index(r, kb, f8.n_blk128(ROWS8)).reshape(-1).to(dev)] = 0xFF
    fp.assert_footprint(clean, run(), none, f"gemm_fp8 M={M}: rows >= M poisoned")
    m = M - 1
    a8g[m, K8 - 1] = 0x7F
    one = none.clone()
    one[m] = True
    fp.assert_footprint(clean, run(), one, f"gemm_fp8 M={M}: one byte of row {m}")
    for name, g_ in (("a8", ag), ("scales", sg), ("out", og)):
        g_.check(f"gemm_fp8 M={M}: margins of {name}")


# ---- attention ------------------------------------------------------------------------------------------------------------------------
# (id, dtype, knobs, (B, H, S, D), query block of the kernel: attention2.hip QB = NW * 32 = 128, attention4.hip 256, attention5.hip 4 waves x 64)
ATTN_FORMS = L.ATTN_FORMS


def _attn_gate(dt, QB, D):
    return dict(cap=QB * D, rel_l2=6e-3 if dt == BF else 6e-3 / 8, max_abs=0.03)


@pytest.mark.parametrize("form", ATTN_FORMS, ids=lambda f: f[0])
def test_attention_footprints(dev, form):
    """packed qkv inside NaN margins: image 1 poisoned (the ragged last key tile of image 0 reads on into it) -> image 0 bit-identical; one K element ->
    its whole (batch, head); one V element in the ragged last tile (the last key range of the key-split launch: the merge kernel read it) -> one column;
    one Q element -> its row of its head, the block's other rows soft (module docstring)"""
    from diffusionkit_amd import ops
    name, dt, knobs, (B, H, S, D), QB = form
    h = H * D
    ops_cpu, ref, cases = fp.attention_family(B, H, S, D, QB, dt)
    out, og = fp.guarded(torch.empty(B, S, h, dtype=dt, device=dev), 8, SENTINEL)
    whole = {}

    run, run_whole = L.attention(dt, knobs, B, H, S, D), L.attention(dt, dict(attn=knobs.get("attn", -1), attn_split=0), B, H, S, D)

    def launch(v):
        out.fill_(SENTINEL)
        run(dict(v, out=out))
        if "attn_split" in knobs and not whole:  # (the switch does select the key-split jobs: their partials are rounded to bf16)
            whole["y"] = torch.empty_like(out)
            run_whole(dict(v, out=whole["y"]))
            assert not torch.equal(whole["y"], out), "attn_split did not select the key-split jobs"
        return out
    run_family(dev, dt, ops_cpu, ref, cases, launch, f"attention {name}", soft_gate=_attn_gate(dt, QB, D), guards=[("out", og)])


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_attention_d512_footprints(dev, dt):
    from diffusionkit_amd import ops
    ops_cpu, ref, cases = fp.attention_d512_family(2, 100, dt)
    run_family(dev, dt, ops_cpu, ref, cases, lambda v: ops.attention_d512(v["q"], v["k"], v["v"]), f"attention d512 {dt}",
               soft_gate=_attn_gate(dt, 64, 512))


@pytest.mark.parametrize("B,H,S,D,per_head", [(1, 4, 150, 64, True), (2, 2, 77, 64, False)])
def test_attention_score_bias_footprints(dev, B, H, S, D, per_head):
    """the pad columns S..ldb of every bias row hold NaN: bit-identical output; one bias[h, i, j]: row i of head h (shared table: of every head) in
    every image.  (The first case found attention2.hip adding the bias to the already masked scores of the tail tile: -1e30 + NaN made every output of
    the launch NaN.  The mask is now a select behind the bias.)"""
    from diffusionkit_amd.text import attention_bias
    ops_cpu, ref, scale, cases = fp.attention_bias_family(B, H, S, D, per_head)

    def launch(v):
        return attention_bias(v["qkv"], H, D, scale, v["bias"] if per_head else v["bias"][0], per_head)
    run_family(dev, BF, ops_cpu, ref, cases, launch, f"attention bias {(B, H, S, D)}")


def test_attention_q_load_norm_rope_footprint(dev):
    """QKNorm + RoPE of the queries in the Q load: one head's q of one row -> exactly that row of that head"""
    from diffusionkit_amd import ops
    c = fp.chosen_fused_cases()["attn_q"]
    B, H, S, D = c["B"], c["H"], c["S"], c["D"]
    h = H * D
    ops_cpu, tab, ref = fp.attention_q_family(c)
    QB = {4: 128, 9: 256, 10: 256}[c["mode"]]
    tabd, tg = fp.guarded(tab.to(dev), PAD) if tab is not None else (None, None)
    out, og = fp.guarded(torch.empty(B, S, h, dtype=BF, device=dev), 8, SENTINEL)

    run = L.attention(BF, dict(attn=c["mode"], attn_split=c.get("attn_split", -1)), B, H, S, D, L.attention_q_extra(c))

    def launch(v):
        out.fill_(SENTINEL)
        return run(dict(v, out=out, **({"rope": tabd} if tabd is not None else {})))
    run_family(dev, BF, ops_cpu, ref, [fp.q_head_case(B, H, S, D, QB)], launch, f"attention q load {c['id']}", soft_gate=_attn_gate(BF, QB, D),
               guards=[("out", og)] + ([("rope", tg)] if tg else []))


def test_attention_mx8_copy_footprint(dev):
    """the MX-fp8 copy of the output: one head's q of one row poisoned -> exactly that row's bytes of that head are NaN bytes; the bytes and scales of
    every row outside the poisoned row's query block equal the clean run's, the block's other rows (soft in O) hold no NaN byte"""
    from diffusionkit_amd import ops
    c = fp.chosen_fused_cases()["attn_o8"]
    B, H, S, D = c["B"], c["H"], c["S"], c["D"]
    h, M = H * D, B * S
    QB = 256 if (c["mode"] in (9, 10) and D == 128) else 128
    ops_cpu, ref, _ = fp.attention_family(B, H, S, D, QB, BF)
    case = fp.q_head_case(B, H, S, D, QB)
    qkv, qg = fp.guarded(ops_cpu["qkv"].to(dev, BF), PAD)
    out, og = fp.guarded(torch.empty(B, S, h, dtype=BF, device=dev), 8, SENTINEL)
    o8b, o8g = fp.guarded(torch.empty(M, h, dtype=torch.uint8, device=dev), 8, 0xAB)

    copy = L.attention_mx8(c)

    def run():
        sc = torch.zeros(ops.mx_scale_bytes(M, h), dtype=torch.uint8, device=dev)
        out.fill_(SENTINEL)
        o8b.fill_(0xAB)
        copy(dict(qkv=qkv, out=out, o8=o8b, o8_scales=sc))
        return out.clone().cpu(), o8b.clone().cpu().reshape(B, S, h), f8.array_to_scales(sc, M, h).reshape(B, S, h // 32)
    y0, q0, e0 = run()
    for name, idx in case.poison:
        qkv[idx] = NAN
    y1, q1, e1 = run()
    assert not c["in_kernel"]  # (the chosen case writes O and quantises it; a kernel that owns the copy leaves O at its sentinel)
    fp.assert_footprint(y0, y1, case.hand, f"attention o8 {c['id']}: O", soft=case.soft, soft_ref=ref(ops_cpu), soft_rel_l2=6e-3, soft_max_abs=0.03)
    assert int(case.soft.sum()) <= QB * D
    rows = (case.hand | case.soft).any(dim=-1)  # [B, S]: the rows of the poisoned row's block
    assert torch.equal(fp.nan_mask(q1), case.hand), "NaN bytes of the MX-fp8 copy are not exactly the poisoned row's bytes of its head"
    assert torch.equal(q1[~rows], q0[~rows]) and torch.equal(e1[~rows], e0[~rows]), "bytes / scales of rows outside the block differ"
    for name, g_ in (("qkv", qg), ("out", og), ("o8", o8g)):
        g_.check(f"attention o8: margins of {name}")


# ---- row kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1536, 2432])
@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_ln_modulate_footprints(dev, dt, h):
    from diffusionkit_amd import ops
    ops_cpu, ref, cases = fp.ln_modulate_family(2, 77, h, dt)
    run_family(dev, dt, ops_cpu, ref, cases, lambda v: ops.ln_modulate(v["x"], v["shift"], v["scale"]), f"ln_modulate {dt} h={h}")


@pytest.mark.parametrize("dt,D", [(BF, 128), (BF, 64), (F16, 64)], ids=["bf16_d128", "bf16_d64", "f16_d64"])
def test_qk_norm_rope_footprints(dev, dt, D):
    """one q / k element -> that head's q / k of that row only; one v element -> itself; one rope table entry at position p -> the rotated pair of every
    head of q and k at the rows mapped to p; one key norm weight -> its column of every head of k"""
    from diffusionkit_amd import ops
    ops_cpu, ref, cases = fp.qk_norm_rope_family(D, dt)

    def launch(v):
        return ops.qk_norm_rope_(v["qkv"], 3, D, v["qw"], v["kw"], v["tab"])
    run_family(dev, dt, ops_cpu, ref, cases, launch, f"qk_norm_rope {dt} D={D}")


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_groupnorm_footprints(dev, dt):
    from diffusionkit_amd import ops
    G = fp.GN_SHAPE[4]
    ops_cpu, ref, cases = fp.groupnorm_family(dt)
    run_family(dev, dt, ops_cpu, ref, cases, lambda v: ops.groupnorm(v["x"], v["gamma"], v["beta"], G, 1e-5, True), f"groupnorm {dt}")
    ops_cpu, ref, cases = fp.groupnorm_family(dt, table=True)
    run_family(dev, dt, ops_cpu, ref, cases, lambda v: ops.groupnorm_table(v["x"], v["gamma"], v["beta"], G, 1e-5), f"groupnorm_table {dt}")


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_softmax_and_transpose_footprints(dev, dt):
    from diffusionkit_amd import ops
    ops_cpu, ref, cases = fp.softmax_family(dt)
    run_family(dev, dt, ops_cpu, ref, cases, lambda v: ops.softmax_rows_(v["x"]), f"softmax_rows_ {dt}")
    ops_cpu, ref, cases = fp.transpose_family(dt)
    run_family(dev, dt, ops_cpu, ref, cases, lambda v: ops.transpose(v["x"]), f"transpose {dt}")


@pytest.mark.parametrize("flux", [True, False], ids=["flux", "sd3"])
def test_patchify_and_euler_step_footprints(dev, flux):
    """dk_latent_to_tokens + dk_euler_cfg_step, CFG on: one latent element -> exactly one token feature, in both CFG copies; one model output element ->
    exactly one latent element (and its token feature of the next step's input)"""
    ops_cpu, ref, (sigma, sigma_next, w), cases = fp.patchify_family(flux)
    tok0, g0 = fp.guarded(torch.empty(ops_cpu["out"].shape, dtype=BF, device=dev), 8, SENTINEL)
    tok, g1 = fp.guarded(torch.empty(ops_cpu["out"].shape, dtype=BF, device=dev), 8, SENTINEL)

    step = L.patchify_step(flux, (sigma, sigma_next, w))

    def launch(v):
        return step(dict(v, tok0=tok0, tok=tok))
    run_family(dev, BF, ops_cpu, ref, cases, launch, f"patchify flux={flux}", guards=[("tok0", g0), ("tok", g1)], dtypes={"x": torch.float32})


# ---- convolutions ------------------------------------------------------------------------------------------------------------------------
def _conv_launch(ops, form, res):
    return L.conv(form, res)


@pytest.mark.parametrize("form,res", [("plain", False), ("plain", True), ("s2", False), ("up", False)])
@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_conv3x3_footprints(dev, dt, form, res):
    """the conv forms of the GEMM kernels (gemm.hip's 128^2 tiles), two images of 16 x 16: one channel of one pixel -> the 3 x 3 neighbourhood clipped to
    its own image (upsample: the 2 x 2 block dilated by one; stride 2: the outputs whose window holds it), all output channels; image 1 poisoned ->
    image 0 bit-identical (the zero-page border against the neighbouring image's rows)"""
    from diffusionkit_amd import ops
    ops_cpu, ref, cases = fp.conv_family(2, 16, 16, 64, 128, form, dt, res=res)
    run_family(dev, dt, ops_cpu, ref, cases, _conv_launch(ops, form, res), f"conv3x3 {dt} {form} res={res}")


@pytest.mark.parametrize("form,shape", [("plain", (2, 16, 24, 128, 256)), ("up", (2, 8, 12, 128, 256))])
def test_conv3x3_on_256_tile_kernel_footprints(dev, form, shape):
    """the same on gemm256v3.hip's conv form (O % 256 == 0, forced: test_conv3x3_on_256_tile_kernel's two-image shape; padding taps through out-of-range
    buffer offsets)"""
    from diffusionkit_amd import ops
    ops_cpu, ref, cases = fp.conv_family(*shape, form, BF, res=form == "plain", tile=8)
    forced = L.conv(form, form == "plain", dict(gemm=9, gemm_mf=8))
    run_family(dev, BF, ops_cpu, ref, cases, forced, f"conv3x3 on gemm256v3 {form}")


# (id, dtype, conv_v4 knob, (B, H, W, C, O) with H x W the INPUT size, upsample, table, residual, shortcut columns)
HALO_FORMS = L.HALO_FORMS


@pytest.mark.parametrize("form", HALO_FORMS, ids=lambda f: f[0])
def test_conv3x3_gn_footprints(dev, form):
    """norm -> silu -> conv in one launch on conv_halo.hip and on conv256v4.hip (256- and 128-channel tiles, upsample form): the GroupNorm table is built
    from the CLEAN input and only the conv's input is poisoned, so the footprint stays the 3 x 3 neighbourhood; a residual element -> one output
    element, a shortcut input element -> one pixel in all channels; image 1 poisoned -> image 0 bit-identical.
    Output statistics (one (sum, M2) pair per image, 16 x 16-pixel tile and group; tile ty * (W / 16) + tx: conv_halo.hip:71-74,
    conv256v4.hip:55-58): exactly the entries of the tiles that hold a NaN output pixel are NaN, every other entry is bit-identical."""
    from diffusionkit_amd import ops
    name, dt, v4, (B, H, W, C, O), ups, table, res, C2 = form
    G = 32
    rnd = fp.rounder(dt)
    gamma, beta = rnd(C, seed=81, scale=0.1, shift=1.0), rnd(C, seed=82, scale=0.1)
    x_clean = fp.conv_family(B, H, W, C, O, "up" if ups else "plain", dt)[0]["x"]
    act = fp.gn_act(x_clean, gamma, beta, G) if table else None
    ops_cpu, ref_y, cases = fp.conv_family(B, H, W, C, O, "up" if ups else "plain", dt, res=res, C2=C2, act=act)
    stats = not ups
    tab = ops.groupnorm_table(x_clean.to(dev, dt), gamma.to(dev, dt), beta.to(dev, dt), G, 1e-5) if table else None

    def ref(o):
        y = ref_y(o)
        if not stats:
            return y
        # the partials' values are sums over the stored outputs: NaN where a tile holds a NaN output (every group: all output channels are poisoned,
        # or -- one residual element -- the one group of that channel); finite values are not compared against this stand-in, only the NaN set
        n = torch.isnan(y)
        Bn, Ho, Wo, _ = y.shape
        per_group = n.reshape(Bn, Ho, Wo, G, O // G).any(dim=-1)  # [B, Ho, Wo, G]
        part = torch.stack([fp.tile_mask(per_group[..., g_]) for g_ in range(G)], dim=-1)  # [B, tiles, G]
        part = part[..., None].expand(*part.shape, 2)
        return dict(y=y, part=torch.where(part, torch.tensor(NAN), torch.tensor(0.0)))
    if stats:
        for case in cases:  # hand-written footprint of the partials from the hand-written footprint of y
            per_group = case.hand.reshape(B, H, W, G, O // G).any(dim=-1)
            part = torch.stack([fp.tile_mask(per_group[..., g_]) for g_ in range(G)], dim=-1)
            case.hand = dict(y=case.hand, part=part[..., None].expand(*part.shape, 2).clone())

    launch = L.conv_gn(v4, O, C2, G, stats, ups, tab)
    run_family(dev, dt, ops_cpu, ref, cases, launch, f"conv3x3_gn {name}")


def test_conv_out_image_tail_footprints(dev):
    """conv_norm_out -> silu -> conv_out -> clip / uint8 in one launch (test_conv_out_image_tail_halo's shape): the footprint is asserted on ``raw``;
    the clipped image and the uint8 image go through a clip and an integer conversion (tests/test_footprint_cpu.py), so only "outside the footprint
    bit-identical" is asserted on them"""
    from diffusionkit_amd import ops
    B, H, W, C, G = 2, 32, 48, 128, 32
    rnd = fp.rounder(BF)
    gamma, beta = rnd(C, seed=92, scale=0.1, shift=1.0), rnd(C, seed=93, scale=0.1)
    x_clean = fp.conv_family(B, H, W, C, 3, "plain", BF)[0]["x"]
    ops_cpu, ref, cases = fp.conv_family(B, H, W, C, 3, "plain", BF, act=fp.gn_act(x_clean, gamma, beta, G))
    tab = ops.groupnorm_table(x_clean.to(dev, BF), gamma.to(dev, BF), beta.to(dev, BF), G, 1e-5)
    bufs = upload(ops_cpu, dev, BF)
    v = {k: t for k, (t, _) in bufs.items()}

    tail = L.image_tail(tab)

    def run():
        y = tail(v)
        return y["img"].clone().cpu(), y["u8"].clone().cpu(), y["raw"].clone().cpu()
    img0, u80, raw0 = run()
    assert bool(torch.isfinite(img0).all())
    for case in cases:
        restore(bufs, ops_cpu)
        for name, idx in case.poison:
            v[name][idx] = NAN
        img1, u81, raw1 = run()
        expect = torch.isnan(ref(fp.poisoned(ops_cpu, case)))
        assert torch.equal(expect, case.hand)
        e4 = torch.cat([expect, torch.zeros_like(expect[..., :1])], dim=-1)  # (raw has a fourth, zero channel)
        fp.assert_footprint(raw0, raw1, e4, f"image tail raw: {case.label}")
        assert torch.equal(fp.bits(img1)[~expect], fp.bits(img0)[~expect]), f"image tail img: {case.label}: outputs outside the footprint differ"
        assert torch.equal(u81[~expect], u80[~expect]), f"image tail u8: {case.label}: outputs outside the footprint differ"
    for k, (_, guard) in bufs.items():
        guard.check(f"image tail: margins of {k}")


# ---- degenerate rows (finite inputs, fp64 oracle, TOL_SINGLE_OP) ------------------------------------------------------------------------------
def _degenerate_rows(x):
    """rows 0, 1, 2 of x [rows, n] become: all zero, constant, one channel of 2^14 among values of order 1"""
    x = x.clone()
    x[0] = 0.0
    x[1] = 3.0
    x[2, x.shape[1] // 3] = 2.0 ** 14
    return x


def _row_gate(ref, got, what):
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    for i, name in enumerate(("all-zero", "constant", "one channel of 2^14")):
        e = rel_l2(ref[i], got[i])
        print(f"[degenerate] {what}, {name}: rel_l2 {e:.3e} (< {TOL_SINGLE_OP})")
        assert e < TOL_SINGLE_OP, f"{what}, {name} row: {e:.3e}"


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_degenerate_rows_ln_modulate(dev, dt):
    """variance 0 gives exactly the shift (all-zero and constant row), never a NaN from a negative variance"""
    from diffusionkit_amd import ops
    rnd = fp.rounder(dt)
    h = 1536
    x = _degenerate_rows(rnd(8, h, seed=1))[None]
    shift, scale = rnd(1, h, seed=2), rnd(1, h, seed=3, scale=0.5)
    y = ops.ln_modulate(x.to(dev, dt), shift.to(dev, dt), scale.to(dev, dt)).float().cpu()[0]
    xd = x[0].double()
    mu = xd.mean(-1, keepdim=True)
    ref = (xd - mu) * torch.rsqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + 1e-6) * (1.0 + scale).to(dt).double() + shift.double()
    _row_gate(ref, y, f"ln_modulate {dt}")
    assert torch.equal(y[0], shift[0]) and torch.equal(y[1], shift[0])


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_degenerate_heads_qk_norm(dev, dt):
    from diffusionkit_amd import ops
    rnd = fp.rounder(dt)
    H, D = 1, 64
    q = _degenerate_rows(rnd(8, D, seed=4))
    qkv = torch.cat([q, q, q], dim=-1)[None]  # [1, 8, 3 D]
    w = rnd(D, seed=5, scale=0.1, shift=1.0)
    d = qkv.to(dev, dt).contiguous()
    ops.qk_norm_rope_(d, H, D, w.to(dev, dt), w.to(dev, dt), None)
    got = d.float().cpu()[0]
    qd = q.double()
    ref = qd * torch.rsqrt((qd * qd).mean(-1, keepdim=True) + 1e-6) * w.double()
    _row_gate(ref, got[:, :D], f"qk_norm q {dt}")
    _row_gate(ref, got[:, D:2 * D], f"qk_norm k {dt}")
    assert bool((got[0, :2 * D] == 0).all())


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_degenerate_groups_groupnorm(dev, dt):
    """an all-zero group and a constant group come out as beta, a group with one value of 2^14 stays finite and accurate"""
    from diffusionkit_amd import ops
    rnd = fp.rounder(dt)
    B, H, W, C, G = 1, 8, 8, 64, 32
    cg = C // G
    x = rnd(B, H, W, C, seed=6)
    x[..., 0:cg] = 0.0
    x[..., cg:2 * cg] = 3.0
    x[0, 3, 4, 2 * cg] = 2.0 ** 14
    gamma, beta = rnd(C, seed=7, scale=0.1, shift=1.0), rnd(C, seed=8, scale=0.1)
    y = ops.groupnorm(x.to(dev, dt), gamma.to(dev, dt), beta.to(dev, dt), G, 1e-5, False).float().cpu()
    xg = x.double().reshape(B, H * W, G, cg)
    mu = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mu) ** 2).mean(dim=(1, 3), keepdim=True)
    ref = ((xg - mu) * torch.rsqrt(var + 1e-5)).reshape(B, H, W, C) * gamma.double() + beta.double()
    groups = lambda t: t.reshape(-1, G, cg).permute(1, 0, 2).reshape(G, -1)
    _row_gate(groups(ref), groups(y), f"groupnorm {dt}")


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_attention_identical_keys_gives_the_mean_of_v(dev, dt):
    """the lean kernel with all keys identical: every score of a row is the same, the output is the mean of V (fp64), at the attention gates"""
    from diffusionkit_amd import ops
    B, H, S, D = 1, 2, 200, 64
    h = H * D
    rnd = fp.rounder(dt)
    qkv = rnd(B, S, 3 * h, seed=9)
    qkv[:, :, h:2 * h] = qkv[:, :1, h:2 * h]
    out = torch.empty(B, S, h, dtype=dt, device=dev)
    d = qkv.to(dev, dt).contiguous()
    base = d.data_ptr()
    with tuned(attn=4):
        ops.attention_desc_call(dtype=dt, q=base, k=base + 2 * h, v=base + 4 * h, out=out, B=B, H=H, S=S, D=D, ld=3 * h, ldo=h, scale=1.0 / math.sqrt(D))
    ref = qkv[..., 2 * h:].double().mean(dim=1, keepdim=True).expand(B, S, h)
    e, m = rel_l2(ref, out.float()), float((ref - out.double().cpu()).abs().max())
    gate = 6e-3 if dt == BF else 6e-3 / 8
    print(f"[degenerate] attention {dt}, identical keys: rel_l2 {e:.3e} (< {gate:.2e}), max_abs {m:.3e} (< 0.03)")
    assert e < gate and m < 0.03
