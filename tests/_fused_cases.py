"""The cases of tests/test_gpu_fused_ops.py (GPU: every engine-only launch form against a CPU reference of that operation) and of the plan checks in
tests/test_dispatch_plan.py (CPU: each case really takes the path it claims).  ONE table for both files: a GPU case cannot drift onto a path that is
tested elsewhere without the CPU suite noticing.

A case is a plain dict.  ``*_call(case)`` turns it into a ``Call``: the buffers the launch touches (name -> shape) and the descriptor / side-struct
fields with every pointer written as ``(buffer name, element offset)``.  ``resolve`` replaces those by addresses -- made-up aligned ones for
dk_gemm_fused_plan (which dereferences nothing), device addresses for the launch.

``expect`` = (launches, kernel): launches 1 = fused / grouped in ONE launch of the 256-column kernel ``kernel`` (3: gemm256v3.hip, 4: gemm256v4.hip);
launches 2 = the expansion of gemm.hip's gemm_call (PAIR / COLUMNS / KNORM), kernel None."""
from dataclasses import dataclass, field

EPI_BIAS, EPI_GELU, EPI_GATE_RES = 0, 1, 2
TUNE_KEYS = ("gemm", "gemm_mf", "gemm_split")
PAD_ROWS = 8  # rows behind the last one a launch may write (sentinel: must stay untouched)
JOINT_GAP = 3  # rows of neither stream behind every batch row of a joint [B, S_t + S_i + gap, .] buffer (must stay untouched)


@dataclass
class Call:
    buffers: dict                      # name -> (rows, cols) of a bf16 matrix, or ("f32", n) / ("u8", n)
    d: dict
    side: dict = None
    d2: dict = None
    side2: dict = None
    tune: dict = field(default_factory=dict)


def phys_rows(M, seg_len, seg_stride):
    """physical rows a row map (m -> (m / seg_len) * seg_stride + m % seg_len) reaches"""
    return ((M - 1) // seg_len) * seg_stride + (M - 1) % seg_len + 1


def resolve(call, address, ws_bytes=0):
    """(d, side, d2, side2) with every (buffer, element offset) replaced by address(buffer) + 2 * offset (4 * for the fp32 table)"""
    def one(dct):
        if dct is None:
            return None
        out = {}
        for k, v in dct.items():
            if isinstance(v, tuple):
                name, off = v
                esz = 4 if call.buffers[name][0] == "f32" else 1 if call.buffers[name][0] == "u8" else 2
                v = address(name) + esz * off
            elif v == "ws_bytes":
                v = ws_bytes
            out[k] = v
        return out
    return one(call.d), one(call.side), one(call.d2), one(call.side2)


def fake_address(call):
    """aligned addresses that are never dereferenced (plan mode looks at alignment and NULL-ness only)"""
    names = sorted(call.buffers)
    return lambda name: 0x10000000 * (1 + names.index(name))


def tune_of(case):
    return {"gemm": case.get("mode", -1), "gemm_mf": case.get("mf", -1), "gemm_split": case.get("split", -1)}


# ---------------------------------------------------------------------------------------------------------------------------------
# a. column split: columns [0, n1) -> C (bias), columns [n1, n1 + n2) -> C2 (gelu), one read of A.  ``seg`` = (seg_len, seg_stride): the row map of
# A, C and C2 (a joint buffer; None: plain matrices).  C2 is a column window [c2_col0, c2_col0 + n2) of a buffer with c2_pad columns behind it.
# ---------------------------------------------------------------------------------------------------------------------------------
SPLIT_CASES = [
    dict(id="v3_mf8_ragged", M=1100, K=320, n1=512, n2=768, mode=9, mf=8, expect=(1, 3)),
    dict(id="v3_mf7_ragged", M=1100, K=320, n1=512, n2=768, mode=9, mf=7, expect=(1, 3)),
    dict(id="v4_ragged", M=1100, K=320, n1=512, n2=768, mode=10, expect=(1, 4)),
    dict(id="auto_short_k", M=1100, K=320, n1=512, n2=768, expect=(1, 3)),          # K < 2048: the automatic choice stays on gemm256v3.hip
    dict(id="auto_long_k", M=2048, K=2048, n1=512, n2=512, expect=(1, 4)),          # 32 whole tiles, long reduction: gemm256v4.hip
    dict(id="v3_two_segments", M=1000, K=320, n1=256, n2=512, seg=(500, 600), mode=9, mf=8, expect=(1, 3)),  # tile 1 (rows 256..511) straddles
    dict(id="v4_two_segments", M=1000, K=320, n1=256, n2=512, seg=(500, 600), mode=10, expect=(1, 4)),
    dict(id="v3_half_column_tile", M=700, K=192, n1=512, n2=640, mode=9, mf=8, expect=(1, 3)),  # (n1 + n2) % 256 == 128
    dict(id="v3_half_column_tile_mf7", M=700, K=192, n1=512, n2=640, mode=9, mf=7, expect=(1, 3)),
    dict(id="columns_on_128", M=600, K=192, n1=256, n2=384, mode=128, expect=(2, None)),        # COLUMNS expansion
]


def split_call(c):
    M, K, n1, n2 = c["M"], c["K"], c["n1"], c["n2"]
    seg_len, seg_stride = c.get("seg") or (M, 0)
    rows = phys_rows(M, seg_len, seg_stride)
    c2_col0, c2_pad, c_pad = c.get("c2_col0", 64), c.get("c2_pad", 72), 8
    ldc, ldc2 = n1 + c_pad, c2_col0 + n2 + c2_pad
    buffers = {"A": (rows, K), "W": (n1 + n2, K), "bias": (1, n1 + n2), "C": (rows + PAD_ROWS, ldc), "C2": (rows + PAD_ROWS, ldc2)}
    d = dict(A=("A", 0), W=("W", 0), C=("C", 0), bias=("bias", 0), M=M, N=n1 + n2, K=K, lda=K, ldc=ldc,
             a_seg_len=seg_len, a_seg_stride=seg_stride, c_seg_len=seg_len, c_seg_stride=seg_stride, alpha=1.0, epilogue=EPI_BIAS)
    side = dict(n_split=n1, C2=("C2", c2_col0), ldc2=ldc2, epi2=EPI_GELU)
    return Call(buffers, d, side, tune=tune_of(c))


def split_single_calls(c):
    """the two plain launches the fused one must equal bit for bit (same forced kernel, same K order per element)"""
    call = split_call(c)
    n1, n2, K = c["n1"], c["n2"], c["K"]
    a = dict(call.d, N=n1)
    b = dict(call.d, N=n2, W=("W", n1 * K), bias=("bias", n1), C=call.side["C2"], ldc=call.side["ldc2"], epilogue=EPI_GELU)
    return Call(call.buffers, a, tune=call.tune), Call(call.buffers, b, tune=call.tune)


# ---------------------------------------------------------------------------------------------------------------------------------
# b. grouped pair: the image rows (problem a) and the text rows (problem b) of a joint [B, S_t + S_i, .] buffer, same N, K, epilogue; different
# A rows, W, bias, gate, row maps and M.  gate_res: C aliases the residual (post_sdpa).  ``ws``: the K-split workspace is handed in.
# ---------------------------------------------------------------------------------------------------------------------------------
PAIR_CASES = [
    dict(id="one_round_bias", B=2, S_t=128, S_i=512, N=512, K=512, epi=EPI_BIAS, expect=(1, 3)),
    dict(id="one_round_gelu", B=2, S_t=128, S_i=512, N=512, K=512, epi=EPI_GELU, expect=(1, 3)),
    dict(id="one_round_gate_res", B=2, S_t=128, S_i=512, N=512, K=512, epi=EPI_GATE_RES, expect=(1, 3)),
    # M_a = 1200, M_b = 154: the last tile of a and the first of b are different workgroups with different row limits; tiles straddle the segments
    dict(id="ragged_gate_res_v3", B=2, S_t=77, S_i=600, N=512, K=384, epi=EPI_GATE_RES, expect=(1, 3)),
    dict(id="ragged_gate_res_v4", B=2, S_t=77, S_i=600, N=512, K=384, epi=EPI_GATE_RES, mode=10, expect=(1, 4)),
    dict(id="ragged_gelu_v4", B=2, S_t=77, S_i=600, N=512, K=384, epi=EPI_GELU, mode=10, expect=(1, 4)),
    # FLUX's q / k / v pair at 1024 x 1024 (reference on a seeded subset of the output columns)
    dict(id="flux_qkv", B=1, S_t=256, S_i=4096, N=9216, K=3072, epi=EPI_BIAS, ref_cols=384, expect=(1, 4)),
    # FLUX's o_proj pair at 512 x 512: (48 + 12) tiles, 48 K-tiles -- the rule cuts every tile along K into four pieces
    dict(id="flux_512_o_proj_cut_along_k", B=1, S_t=256, S_i=1024, N=3072, K=3072, epi=EPI_GATE_RES, ws=True, ref_cols=512, expect=(1, 3), cut=True),
]


def pair_call(c, grouped=True):
    B, S_t, S_i, N, K, epi = c["B"], c["S_t"], c["S_i"], c["N"], c["K"], c["epi"]
    S = S_t + S_i + JOINT_GAP
    buffers = {"A": (B * S, K), "C": (B * S + PAD_ROWS, N), "Wa": (N, K), "Wb": (N, K), "bias_a": (1, N), "bias_b": (1, N),
               "gate_a": (B, 2 * N), "gate_b": (B, 2 * N)}
    if c.get("ws"):
        buffers["ws"] = ("u8", 0)

    def prob(sfx, row0, seg, g_off):
        d = dict(A=("A", row0 * K), W=("W" + sfx, 0), C=("C", row0 * N), bias=("bias_" + sfx, 0), M=B * seg, N=N, K=K, lda=K, ldc=N,
                 a_seg_len=seg, a_seg_stride=S, c_seg_len=seg, c_seg_stride=S, alpha=1.0, epilogue=epi)
        if epi == EPI_GATE_RES:
            d.update(res=("C", row0 * N), ldr=N, r_seg_len=seg, r_seg_stride=S, gate=("gate_" + sfx, g_off), gate_seg_len=seg, gate_stride=2 * N)
        if c.get("ws") and grouped:
            d.update(workspace=("ws", 0), workspace_bytes="ws_bytes")  # (resolve: dk_gemm_workspace_bytes())
        return d
    a, b = prob("a", S_t, S_i, 0), prob("b", 0, S_t, N)
    tune = tune_of(c)
    if not grouped:  # under "gemm" 9 a pair expands into two launches of gemm256v3.hip (bit-identical to gemm256v4.hip); no K split
        tune = dict(tune, gemm=9, gemm_split=0)
    return Call(buffers, a, None, b, None, tune=tune)


# ---------------------------------------------------------------------------------------------------------------------------------
# c. QKNorm + RoPE in the tail of a q / k / v projection [M, 3h] (keys [h, 2h), queries [0, h)).  M = n_seq sequences of seg_len rows; the output is
# dense (c_seg_len = M) or a joint buffer (``c_gap`` rows between the sequences: c_seg_len = seg_len).  ``table``: "real" (oracle rope_table of FLUX,
# D = 128), "angle" (cos / sin of an angle that depends on position and pair), "ident" (entries that identify (position, pair, cos | sin): not a
# rotation, a swapped index cannot cancel), None (SD3.5 form: no rotation).  ``n2``: with the column split (gelu(fc1) columns behind 3h).
# ---------------------------------------------------------------------------------------------------------------------------------
KNORM_CASES = [
    # gemm256v3.hip: FAST tail (sequences of whole tiles) at both heights; two column tiles per range
    dict(id="v3_mf8_fast", h=512, D=128, n_seq=2, seg_len=512, K=256, table="real", qn=True, mode=9, mf=8, expect=(1, 3)),
    # ... dense output, 224-row tiles: the positions wrap INSIDE a FAST tile (its prefetched table rows)
    dict(id="v3_mf7_dense_wrap", h=512, D=128, n_seq=2, seg_len=512, K=256, table="real", qn=True, mode=9, mf=7, expect=(1, 3)),
    dict(id="v3_dense_wrap_300", h=256, D=128, n_seq=3, seg_len=300, K=256, table="angle", qn=True, mode=9, mf=8, expect=(1, 3)),
    # ... joint output: a tile holds the last positions of one sequence and position 0 of the next (per-lane path); ragged last tile
    dict(id="v3_straddle", h=256, D=128, n_seq=2, seg_len=300, c_gap=64, K=256, table="real", qn=True, mode=9, mf=8, expect=(1, 3)),
    dict(id="v3_straddle_mf7", h=256, D=128, n_seq=2, seg_len=300, c_gap=64, K=256, table="ident", qn=False, mode=9, mf=7, expect=(1, 3)),
    # image stream: positions start behind the text's, the table is longer than the segment
    dict(id="v3_pos_off", h=256, D=128, n_seq=2, seg_len=256, c_gap=40, pos_off=40, K=256, table="real", qn=True, mode=9, mf=8, expect=(1, 3)),
    dict(id="v3_ident_table", h=256, D=128, n_seq=2, seg_len=256, pos_off=24, K=256, table="ident", qn=True, mode=9, mf=8, expect=(1, 3)),
    dict(id="v3_keys_only", h=256, D=128, n_seq=1, seg_len=600, K=256, table="real", qn=False, mode=9, mf=8, expect=(1, 3)),
    dict(id="v3_no_table", h=256, D=128, n_seq=2, seg_len=300, c_gap=64, K=256, table=None, qn=False, mode=9, mf=8, expect=(1, 3)),
    # 64-column heads: no shipped configuration reaches this branch of the fused tail (SD3.5-large: kn_col0 = 2432 is not a multiple of 256)
    dict(id="v3_d64", h=256, D=64, n_seq=2, seg_len=300, c_gap=64, K=256, table="angle", qn=True, mode=9, mf=8, expect=(1, 3)),
    dict(id="v3_d64_fast_no_table", h=256, D=64, n_seq=2, seg_len=256, K=256, table=None, qn=True, mode=9, mf=7, expect=(1, 3)),
    dict(id="v4_d64", h=256, D=64, n_seq=2, seg_len=256, K=256, table="ident", qn=True, mode=10, expect=(1, 4)),
    # gemm256v4.hip on each of its tail paths: FAST, CUT (one sequence, ragged last tile), the per-row walk (tiles straddle the output's segments)
    dict(id="v4_fast", h=512, D=128, n_seq=2, seg_len=512, pos_off=8, K=256, table="real", qn=True, mode=10, expect=(1, 4)),
    dict(id="v4_cut", h=256, D=128, n_seq=1, seg_len=600, pos_off=16, K=256, table="real", qn=True, mode=10, expect=(1, 4)),
    dict(id="v4_per_row", h=256, D=128, n_seq=2, seg_len=300, c_gap=64, K=256, table="real", qn=True, mode=10, expect=(1, 4)),
    dict(id="v4_dense_wrap_300", h=256, D=128, n_seq=3, seg_len=300, pos_off=5, K=256, table="ident", qn=True, mode=10, expect=(1, 4)),
    # the automatic choice (M >= 1024)
    dict(id="auto", h=256, D=128, n_seq=2, seg_len=640, K=256, table="real", qn=True, expect=(1, 3)),
    # the single block's call: with the column split, keys inside the first output
    dict(id="v3_with_column_split", h=256, D=128, n_seq=2, seg_len=300, K=256, table="real", qn=True, n2=512, mode=9, mf=8, expect=(1, 3)),
    dict(id="v4_with_column_split", h=256, D=128, n_seq=2, seg_len=512, K=256, table="angle", qn=True, n2=512, mode=10, expect=(1, 4)),
    # KNORM expansion: the projection on the 128^2 kernel, then the stand-alone pass
    dict(id="expansion_on_128", h=256, D=128, n_seq=2, seg_len=300, c_gap=64, pos_off=8, K=256, table="real", qn=True, mode=128, expect=(2, None)),
    dict(id="expansion_on_128_keys_only", h=256, D=64, n_seq=2, seg_len=300, K=256, table="angle", qn=False, mode=128, expect=(2, None)),
]
KN_EPS = 1e-6
# the tail paths a case must reach (checked on the CPU by knorm_tail_paths): "fast" / "cut" / "row" = tile-uniform maps / the same with a row limit
# (gemm256v4.hip only; gemm256v3.hip walks such a tile per lane) / the per-row (per-lane) walk; "wrap" = the positions wrap inside a fast tile
KNORM_PATHS = {
    "v3_mf8_fast": {"fast"}, "v3_mf7_dense_wrap": {"fast", "wrap", "row"}, "v3_dense_wrap_300": {"fast", "wrap", "row"},
    "v3_straddle": {"fast", "row"}, "v3_straddle_mf7": {"fast", "row"}, "v3_pos_off": {"fast"}, "v3_ident_table": {"fast"},
    "v3_keys_only": {"fast", "row"}, "v3_no_table": {"fast", "row"}, "v3_d64": {"fast", "row"}, "v3_d64_fast_no_table": {"fast", "wrap", "row"},
    "v4_d64": {"fast"}, "v4_fast": {"fast"}, "v4_cut": {"fast", "cut"}, "v4_per_row": {"fast", "row", "cut"},
    "v4_dense_wrap_300": {"fast", "wrap", "cut"}, "auto": {"fast", "wrap"}, "v3_with_column_split": {"fast", "wrap", "row"},
    "v4_with_column_split": {"fast"},
}


def knorm_tail_paths(c, kernel, tile_rows):
    """the tail paths the row tiles of a fused KNORM case take: the `fast` / `cut` tests of gemm256v3.hip / gemm256v4.hip (bias-only epilogue: the
    output's row map alone decides) restated over the case's tiles"""
    M, seg_len = c["n_seq"] * c["seg_len"], c["seg_len"]
    c_seg_len = seg_len if c.get("c_gap") else M
    paths = set()
    for m0 in range(0, M, tile_rows):
        last = m0 + tile_rows - 1
        if last < M and m0 // c_seg_len == last // c_seg_len:
            paths.add("fast")
            if m0 // seg_len != last // seg_len:
                paths.add("wrap")
        elif kernel == 4 and last >= M and m0 // c_seg_len == (M - 1) // c_seg_len:
            paths.add("cut")
        else:
            paths.add("row")
    return paths


def knorm_call(c, fused=True):
    h, D, n_seq, seg_len, K = c["h"], c["D"], c["n_seq"], c["seg_len"], c["K"]
    M, n2, pos_off = n_seq * seg_len, c.get("n2", 0), c.get("pos_off", 0)
    c_seg_len, c_seg_stride = (seg_len, seg_len + c["c_gap"]) if c.get("c_gap") else (M, 0)
    rows = phys_rows(M, c_seg_len, c_seg_stride)
    N = 3 * h + n2
    buffers = {"A": (M, K), "W": (N, K), "bias": (1, N), "C": (rows + PAD_ROWS, 3 * h), "kn_w": (1, D), "qn_w": (1, D)}
    if c["table"]:
        buffers["rope"] = ("f32", (pos_off + seg_len) * D)
    d = dict(A=("A", 0), W=("W", 0), C=("C", 0), bias=("bias", 0), M=M, N=N, K=K, lda=K, ldc=3 * h, c_seg_len=c_seg_len, c_seg_stride=c_seg_stride,
             alpha=1.0, epilogue=EPI_BIAS)
    side = {}
    if n2:
        buffers["C2"] = (rows + PAD_ROWS, n2 + 8)
        side.update(n_split=3 * h, C2=("C2", 0), ldc2=n2 + 8, epi2=EPI_GELU)
    if fused:
        side.update(kn_w=("kn_w", 0), kn_col0=h, kn_col1=2 * h, kn_D=D, kn_pos_off=pos_off, kn_seg_len=seg_len, kn_eps=KN_EPS)
        if c["table"]:
            side.update(kn_rope=("rope", 0))
        if c["qn"]:
            side.update(qn_w=("qn_w", 0), qn_col0=0, qn_col1=h)
    return Call(buffers, d, side or None, tune=tune_of(c))


# the double block's call: image (a) and text (b) q / k / v projections into a joint [B, S, 3h] buffer, own kn_w / qn_w / first position per stream
KNORM_PAIR_CASES = [
    dict(id="auto", B=2, S_t=256, S_i=512, h=256, D=128, K=256, table="real", expect=(1, 3)),
    dict(id="v4", B=2, S_t=256, S_i=512, h=256, D=128, K=256, table="ident", mode=10, expect=(1, 4)),
    dict(id="v4_ragged_text", B=2, S_t=77, S_i=600, h=256, D=128, K=256, table="real", mode=10, expect=(1, 4)),
]


def knorm_pair_call(c, fused=True, grouped=True):
    B, S_t, S_i, h, D, K = c["B"], c["S_t"], c["S_i"], c["h"], c["D"], c["K"]
    S, N = S_t + S_i + JOINT_GAP, 3 * h
    buffers = {"Aa": (B * S_i, K), "Ab": (B * S_t, K), "Wa": (N, K), "Wb": (N, K), "bias_a": (1, N), "bias_b": (1, N), "C": (B * S + PAD_ROWS, N),
               "kn_a": (1, D), "qn_a": (1, D), "kn_b": (1, D), "qn_b": (1, D), "rope": ("f32", (S_t + S_i) * D)}

    def prob(sfx, row0, seg):
        d = dict(A=("A" + sfx, 0), W=("W" + sfx, 0), C=("C", row0 * N), bias=("bias_" + sfx, 0), M=B * seg, N=N, K=K, lda=K, ldc=N,
                 c_seg_len=seg, c_seg_stride=S, alpha=1.0, epilogue=EPI_BIAS)
        side = dict(kn_w=("kn_" + sfx, 0), kn_rope=("rope", 0), kn_col0=h, kn_col1=2 * h, kn_D=D, kn_pos_off=row0, kn_seg_len=seg, kn_eps=KN_EPS,
                    qn_w=("qn_" + sfx, 0), qn_col0=0, qn_col1=h)
        return d, (side if fused else None)
    (a, fa), (b, fb) = prob("a", S_t, S_i), prob("b", 0, S_t)
    tune = tune_of(c)
    if not grouped:
        tune = dict(tune, gemm=9, gemm_split=0)
    return Call(buffers, a, fa, b, fb, tune=tune)


# ---------------------------------------------------------------------------------------------------------------------------------
# forms that must EXPAND (or be refused by the 256-column kernels) rather than launch fused: (id, call, launches)
# ---------------------------------------------------------------------------------------------------------------------------------
def ineligible_calls():
    out = []
    # SD3.5-large: h = 38 * 64 = 2432, the key columns start inside a column tile
    c = knorm_call(dict(h=2432, D=64, n_seq=2, seg_len=1024, K=256, table=None, qn=False))
    out.append(("kn_col0 % 256 != 0 (SD3.5-large)", c, 2))
    c = knorm_call(dict(h=768, D=96, n_seq=2, seg_len=1024, K=256, table=None, qn=False))
    out.append(("kn_D = 96", c, 2))
    c = knorm_call(dict(h=256, D=128, n_seq=2, seg_len=1024, K=256, table=None, qn=True))
    c.side.update(qn_col0=256, qn_col1=512)  # the key range itself
    out.append(("query range overlaps the key range", c, 2))
    c = knorm_call(dict(h=256, D=128, n_seq=2, seg_len=1024, K=256, table=None, qn=False))
    c.d.update(epilogue=EPI_GELU)
    out.append(("first epilogue is not bias-only", c, 2))
    c = split_call(dict(M=2048, K=256, n1=384, n2=640))
    out.append(("n_split % 256 != 0", c, 2))
    for what, key in (("N", "N"), ("K", "K")):
        c = pair_call(dict(B=1, S_t=256, S_i=1024, N=512, K=512, epi=EPI_BIAS))
        c.d2[key] = 256
        if key == "K":
            c.d2["lda"] = 512
        out.append((f"pair with different {what}", c, 2))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# d. QKNorm + RoPE of the queries in the attention kernels' Q load.  mode: dk_tune_set("attn", .) -- 4 lean kernel (attention2.hip), 9 phase-alternating
# (attention4.hip, D = 128), 10 one wave per SIMD (attention5.hip, D = 128, S % 256 == 0, S >= 768).  split: rows s < split of every image take qn_a.
# ---------------------------------------------------------------------------------------------------------------------------------
ATTN_Q_CASES = [
    dict(id="lean_d64_inside_block", mode=4, B=2, H=2, S=300, D=64, split=77, norm=True, rope=True),
    dict(id="lean_d64_block_boundary", mode=4, B=1, H=3, S=333, D=64, split=128, norm=True, rope=True),
    dict(id="lean_d128_inside_block", mode=4, B=2, H=2, S=300, D=128, split=150, norm=True, rope=True),
    dict(id="lean_d128_split_0", mode=4, B=1, H=2, S=200, D=128, split=0, norm=True, rope=True),
    dict(id="lean_d128_split_S", mode=4, B=1, H=2, S=200, D=128, split=200, norm=True, rope=True),
    dict(id="lean_d64_norm_only", mode=4, B=1, H=2, S=200, D=64, split=50, norm=True, rope=False),
    dict(id="lean_d64_table_only", mode=4, B=1, H=2, S=200, D=64, split=0, norm=False, rope=True),
    dict(id="alt_inside_block", mode=9, B=2, H=2, S=700, D=128, split=77, norm=True, rope=True),
    dict(id="alt_block_boundary", mode=9, B=2, H=2, S=700, D=128, split=256, norm=True, rope=True),
    dict(id="alt_split_0", mode=9, B=1, H=2, S=333, D=128, split=0, norm=True, rope=True),
    dict(id="alt_split_S", mode=9, B=1, H=2, S=333, D=128, split=333, norm=True, rope=True),
    dict(id="alt_norm_only", mode=9, B=1, H=2, S=333, D=128, split=100, norm=True, rope=False),
    dict(id="alt_table_only", mode=9, B=1, H=2, S=333, D=128, split=0, norm=False, rope=True),
    dict(id="wave_inside_block", mode=10, B=2, H=2, S=1024, D=128, split=300, norm=True, rope=True),
    dict(id="wave_block_boundary", mode=10, B=2, H=2, S=1024, D=128, split=256, norm=True, rope=True),
    dict(id="wave_split_0", mode=10, B=1, H=2, S=768, D=128, split=0, norm=True, rope=True),
    dict(id="wave_split_S", mode=10, B=1, H=2, S=768, D=128, split=768, norm=True, rope=True),
    dict(id="wave_norm_only", mode=10, B=1, H=2, S=768, D=128, split=100, norm=True, rope=False),
    dict(id="wave_table_only", mode=10, B=1, H=2, S=768, D=128, split=0, norm=False, rope=True),
    # attention5.hip's key-split jobs (a range holds at least 12 key tiles: two ranges from S = 1536, four from 3072) load the same fused queries
    dict(id="wave_key_split_2", mode=10, attn_split=2, B=2, H=2, S=1536, D=128, split=300, norm=True, rope=True),
    dict(id="wave_key_split_4", mode=10, attn_split=4, B=1, H=2, S=3072, D=128, split=256, norm=True, rope=True),
    # ... and the smallest shape at which the AUTOMATIC rule cuts: 96 blocks, all in the last round, two ranges on 256 CUs
    dict(id="wave_auto_key_split_2", mode=10, B=1, H=16, S=1536, D=128, split=300, norm=True, rope=True),
]


def attn_plan_desc(c):
    """the dk_attention_desc fields of an ATTN_Q_CASES / ATTN_O8_CASES launch for dk_attention_plan: made-up aligned addresses (nothing is
    dereferenced), q | k | v in one [B * S, 3h] buffer"""
    B, H, S, D = c["B"], c["H"], c["S"], c["D"]
    h, qkv, w = H * D, 0x10000000, 0x30000000
    d = dict(q=qkv, k=qkv + 2 * h, v=qkv + 4 * h, out=0x20000000, B=B, H=H, S=S, D=D, ld=3 * h, ldo=h, scale=D ** -0.5)
    if c.get("norm"):
        d.update(qn_a=w, qn_b=w + 2 * D, qn_split=c["split"], qn_eps=KN_EPS)
    if c.get("rope"):
        d.update(q_rope=w + 4 * D)
    if "in_kernel" in c:
        d.update(O8=0x40000000, O8_scales=0x50000000, o8_ld=h, o8_rows=B * S)
    return d


ATTN_KERNEL_NAMES = {4: "lean", 9: "alt", 10: "wave"}  # dk_attention_plan_t.kernel -> the prefix of a case's id


def attn_claim(c):
    """what the case's id says it runs: "lean_" / "alt_" / "wave_" prefix, "key_split_<n>" suffix"""
    name = c["id"]
    kernel = "lean" if name.startswith("lean") or "falls_back" in name else name.split("_")[0]
    m = name.split("key_split_")
    return kernel, (int(m[1]) if len(m) == 2 else 1)


# e. MX-fp8 copy of the attention output (B * S a multiple of 128).  in_kernel: the kernel writes O8 from its accumulators INSTEAD of O
ATTN_O8_CASES = [
    dict(id="alt_d128", mode=9, B=1, H=2, S=640, D=128, in_kernel=True),
    dict(id="alt_d128_two_images", mode=9, B=2, H=3, S=384, D=128, in_kernel=True),
    dict(id="wave_d128", mode=10, B=1, H=2, S=768, D=128, in_kernel=True),
    dict(id="wave_d128_two_images", mode=10, B=2, H=2, S=1024, D=128, in_kernel=True),
    dict(id="lean_d128", mode=4, B=1, H=2, S=384, D=128, in_kernel=False),
    dict(id="lean_d64", mode=4, B=2, H=4, S=320, D=64, in_kernel=False),
    dict(id="alt_falls_back_d64", mode=9, B=1, H=4, S=256, D=64, in_kernel=False),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and CPU references shared by the GPU tests and the CPU check of the reordered sum (torch is imported on use: the plan tests need none)
# ---------------------------------------------------------------------------------------------------------------------------------
def rope_table_for(kind, n_pos, D, text_len=0):
    """f32 [n_pos, D / 2, 2] (cos, sin).  "real": the oracle's table of FLUX (D = 128) with ``text_len`` text positions, then a 16-wide image grid;
    "angle": cos / sin of an angle that depends on position and pair; "ident": c in [0.5, 1), s in [-0.25, 0.25) that identify (position, pair)"""
    import torch
    if kind == "real":
        from diffusionkit_amd.config import FLUX_SCHNELL
        from oracle import mmdit as om
        assert D == 128
        return om.rope_table(FLUX_SCHNELL, text_len, -(-(n_pos - text_len) // 16), 16)[:n_pos].contiguous()
    s = torch.arange(n_pos, dtype=torch.float32)[:, None]
    i = torch.arange(D // 2, dtype=torch.float32)[None, :]
    if kind == "angle":
        ang = 0.37 * s / (1.0 + 0.11 * i) + 0.05 * i
        return torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).contiguous()
    assert kind == "ident"
    c = 0.5 + torch.remainder(s * 131 + i * 17, 251) / 512  # (251: prime -- no power-of-two first position maps a row onto itself)
    sn = torch.remainder(s * 37 + i * 101 + 7, 251) / 512 - 0.25
    return torch.stack([c, sn], dim=-1).contiguous()


def knorm_inputs(c):
    """seeded, bf16-representable operands of a KNORM_CASES entry (fp32 tensors on the CPU)"""
    from tests._util import bf16r, randn
    h, D, K = c["h"], c["D"], c["K"]
    M, N = c["n_seq"] * c["seg_len"], 3 * h + c.get("n2", 0)
    t = dict(A=randn(M, K, seed=80), W=randn(N, K, seed=81, scale=1.0 / K ** 0.5), bias=randn(1, N, seed=82, scale=0.3),
             kn_w=bf16r(1.0 + randn(1, D, seed=83, scale=0.1)), qn_w=bf16r(0.6 + randn(1, D, seed=84, scale=0.1)))
    if c["table"]:
        t["rope"] = rope_table_for(c["table"], c.get("pos_off", 0) + c["seg_len"], D, text_len=c.get("pos_off", 0))
    return t


def norm_rope_oracle(x, w, tab, D, P, order=None):
    """x: [n_seq, seg_len, n_heads * D] -> the oracle's rms_norm (weight w [D] or [seg_len, D]) + rope_apply (tab [seg_len, D / 2, 2] or None) per head.
    ``order`` "fwd" / "rev": the head's squares summed one after the other in fp32, first to last / last to first (the CPU check of the device's
    freedom to reorder that sum); None: the oracle's own rms_norm"""
    import torch
    from oracle import mmdit as om
    n_seq, seg_len, hd = x.shape
    v = x.reshape(n_seq, seg_len, hd // D, D).transpose(1, 2)  # [n_seq, H, seg_len, D]
    if w is not None:
        if order is None:
            v = om.rms_norm(v, w, KN_EPS, P)
        else:
            sq = v * v
            ss = torch.zeros_like(sq[..., :1])
            for j in (range(D) if order == "fwd" else reversed(range(D))):  # (one fp32 addition after the other: no wider accumulator)
                ss = ss + sq[..., j:j + 1]
            v = P.r(v * torch.rsqrt(ss / D + KN_EPS) * w)
    if tab is not None:
        v = om.rope_apply(v, tab, P)
    return v.transpose(1, 2).reshape(n_seq, seg_len, hd)


def knorm_oracle(c, t, proj, P, order=None):
    """[q | k | v] of a KNORM_CASES entry from its rounded projection ``proj`` [M, >= 3h]"""
    import torch
    h, D, seg_len, pos_off = c["h"], c["D"], c["seg_len"], c.get("pos_off", 0)
    tab = t["rope"][pos_off:pos_off + seg_len] if c["table"] else None
    q, k, v = (proj[:, i * h:(i + 1) * h].reshape(c["n_seq"], seg_len, h) for i in range(3))
    k = norm_rope_oracle(k, t["kn_w"][0], tab, D, P, order)
    if c["qn"]:
        q = norm_rope_oracle(q, t["qn_w"][0], tab, D, P, order)
    return torch.cat([q, k, v], dim=-1).reshape(-1, 3 * h)


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds and checks shared by tests/test_gpu_fused_ops.py, tests/test_gpu_fp8.py and tests/test_fused_reference_cpu.py
# ---------------------------------------------------------------------------------------------------------------------------------
HEAD_BOUND = 2.0 ** -6  # per element of a normalised + rotated head: |diff| <= 2^-6 * max|ref over that row's head| (two bf16 ulps of at most 2^-7)
SHARE_CAP = 0.01        # share of elements in which the fused tail and the stand-alone pass may differ (tests/test_fused_reference_cpu.py)


def projection(a, w, bias):
    """bf16r(a w^T + bias) with the sum taken in fp64: the reference's own summation order must not add flipped roundings to the per-element bound"""
    from tests._util import bf16r
    return bf16r((a.double() @ w.double().t() + bias.double()).float())


def head_bound_ok(ref, got, D, what):
    """per element: |diff| <= HEAD_BOUND * max|ref| over that row's head; returns the worst ratio diff / head max"""
    r = ref.reshape(ref.shape[0], -1, D)
    d = (got.reshape(r.shape) - r).abs()
    hm = r.abs().amax(dim=-1, keepdim=True)
    worst = float((d / hm.clamp_min(1e-30)).max())
    assert bool((d <= HEAD_BOUND * hm).all()), f"{what}: worst |diff| / head max {worst:.3e} > 2^-6"
    return worst


def norm_columns_ok(ref, got, h, D, what):
    """the q and the k columns separately against the emulating oracle"""
    from tests._util import TOL_SINGLE_OP, rel_l2
    for name, sl in (("q", slice(0, h)), ("k", slice(h, 2 * h))):
        r = rel_l2(ref[:, sl], got[:, sl])
        worst = head_bound_ok(ref[:, sl], got[:, sl], D, f"{what} {name}")
        print(f"[{what}] {name} columns: rel_l2 {r:.3e} (< {TOL_SINGLE_OP:.0e}), worst |diff| / head max {worst:.3e} (<= {HEAD_BOUND:.3e})")
        assert r < TOL_SINGLE_OP, f"{what} {name}"
