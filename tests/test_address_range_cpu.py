"""The address-range guards, swept across their edges on the CPU (no GPU: the planners are host code and take made-up, aligned pointers).

Every hot kernel addresses memory through 32-bit quantities and is fenced by a guard that hands the launch to a kernel with 64-bit addressing or
refuses the call ("Address-range guards").  For each guard the guarded quantity is moved across its edge by one unit of the alignment the
kernel requires, and the plan must name the guarded kernel on the near side and NEVER on the far side; a forced kernel that cannot take the shape and
a launch nothing can take must come back with their documented error text.  tests/test_gpu_address_extents.py runs both sides of the same edges on
the device.  The arithmetic of tests/_bigmem.py (which the GPU tests rely on to put a boundary inside an operand) is swept here too."""
import pytest
import torch

from diffusionkit_amd import _lib, ops
from tests import _bigmem as bm
from tests._address_cases import ATTN_KERNELS, ATTN_TEXT, F8_TEXT, FORCED_TEXT, GEMM_KERNELS, HALO_TEXT, a_rows, attn_edge_ld, edge_rows
from tests._op_launches import tuned

BF, F16 = torch.bfloat16, torch.float16
P = 0x10000000  # made-up pointers: multiples of 256 MiB, never dereferenced

def gemm_plan(M, seg_len, seg_stride, knobs, dt, lda=3072, ldw=0, ldc=256, N=256, K=192):
    d = dict(A=P, W=2 * P, C=3 * P, bias=4 * P, M=M, N=N, K=K, lda=lda, ldc=ldc, a_seg_len=seg_len, a_seg_stride=seg_stride, c_seg_len=M, c_seg_stride=0,
             alpha=1.0, epilogue=0, ldw=ldw)
    with tuned(**knobs):
        return ops.gemm_plan(d, dtype=dt)


@pytest.mark.parametrize("kern", GEMM_KERNELS, ids=lambda k: k[0])
def test_gemm_a_span_guard(kern):
    """gemm256v3.hip:713 (and through it gemm256v4.hip:283, gemm256v3_f16.hip): a_rows * lda * 2 < 2^32.  lda = 3072: 6144 bytes a row, 699 050 rows are
    the last accepted (2^32 - 4096 bytes).  Three segments of 128 rows keep M small; the row count moves by one through M and the segment stride."""
    _, dt, knobs, kernel, tile_rows = kern
    edge = edge_rows(6144)
    assert edge == 699050 and edge * 6144 == 2 ** 32 - 4096
    for M, stride in ((382, 349462), (384, 349461)):  # both reach exactly the last accepted row
        assert a_rows(M, 128, stride) == edge
        p = gemm_plan(M, 128, stride, knobs, dt)
        assert p.kernel == kernel and (tile_rows is None or p.tile_rows == tile_rows) and p.launches == 1
    for M, stride in ((383, 349462), (384, 349462), (384, 2 ** 22)):  # one row beyond, two rows beyond, 2^35 bytes
        assert a_rows(M, 128, stride) > edge
        if kernel == 3:  # gemm256v3 forced: refused, never launched on such a span
            with pytest.raises(_lib.DkHipError, match=FORCED_TEXT):
                gemm_plan(M, 128, stride, knobs, dt)
        else:
            assert gemm_plan(M, 128, stride, knobs, dt).kernel == 128
    # the automatic route never names a 256-column kernel beyond the edge, whatever the size of the problem
    for dtype in (BF, F16):
        for M, seg, stride in ((384, 128, 349462), (700000, 700000, 0), (8192, 4096, 699052)):
            assert a_rows(M, seg, stride) > edge
            assert gemm_plan(M, seg, stride, {}, dtype).kernel == 128, (M, seg, stride)
        p = gemm_plan(8192, 4096, 699050 - 4096, {}, dtype)  # the same large problem on the near side does get one
        assert a_rows(8192, 4096, 699050 - 4096) == edge and p.kernel in (3, 4)


@pytest.mark.parametrize("kern", GEMM_KERNELS, ids=lambda k: k[0])
def test_gemm_w_pitch_guards(kern):
    """gemm256v3.hip:713: 8 rows of W below 2^31 bytes (ldw * 16 < 2^31: ldw < 2^27); gemm256v4.hip:286: 256 rows (ldw * 512 < 2^31: ldw < 2^22).
    ldw moves in steps of 8 elements (16-byte rows).  Beyond v4's edge a forced v4 falls to the 128^2 kernel; gemm256v3 still takes the shape."""
    _, dt, knobs, kernel, _ = kern
    e3, e4 = 2 ** 27, 2 ** 22
    if kernel == 4:
        assert gemm_plan(384, 384, 0, knobs, dt, lda=192, ldw=e4 - 8).kernel == 4
        for ldw in (e4, e4 + 8, e3 - 8, e3):
            assert gemm_plan(384, 384, 0, knobs, dt, lda=192, ldw=ldw).kernel == 128, ldw
        return
    for ldw in (e4 - 8, e4, e3 - 8):
        assert gemm_plan(384, 384, 0, knobs, dt, lda=192, ldw=ldw).kernel == 3, ldw
    for ldw in (e3, e3 + 8):
        with pytest.raises(_lib.DkHipError, match=FORCED_TEXT):
            gemm_plan(384, 384, 0, knobs, dt, lda=192, ldw=ldw)
        assert gemm_plan(384, 384, 0, {}, dt, lda=192, ldw=ldw).kernel == 128
        assert gemm_plan(4096, 4096, 0, {}, dt, lda=192, ldw=ldw, K=2048).kernel == 128  # (a shape the automatic route gives to a 256-column kernel)
    assert gemm_plan(4096, 4096, 0, {}, dt, lda=2048, ldw=e4 - 8, K=2048).kernel in (3, 4)


def test_fused_plan_respects_the_a_span_guard():
    """dk_gemm_fused_plan: a column split whose A span passes 2^32 bytes is expanded onto the 128^2 kernel (two launches), not fused on a 256-column one"""
    from tests import _fused_cases as fc
    case = next(c for c in fc.SPLIT_CASES if c["id"] == "auto_short_k")
    call = fc.split_call(case)
    near = ops.gemm_fused_plan(*fc.resolve(call, fc.fake_address(call)))
    assert (near.launches, near.kernel) == (1, 3)
    rows = edge_rows(2 * 3072) + 1
    far = fc.Call(call.buffers, dict(call.d, lda=3072, a_seg_len=550, a_seg_stride=rows - 550), call.side, tune=call.tune)
    assert a_rows(case["M"], 550, rows - 550) == rows
    p = ops.gemm_fused_plan(*fc.resolve(far, fc.fake_address(far)))
    assert p.kernel not in (3, 4), (p.kernel, p.launches)
    ok = fc.Call(call.buffers, dict(call.d, lda=3072, a_seg_len=550, a_seg_stride=rows - 551), call.side, tune=call.tune)
    p = ops.gemm_fused_plan(*fc.resolve(ok, fc.fake_address(ok)))
    assert (p.launches, p.kernel) == (1, 3)


def attn_plan(ld, S, D, knobs, dt, B=2, H=1, ldo=None):
    ws = int(_lib.load().dk_attention_workspace_bytes())
    with tuned(**knobs):
        return ops.attention_plan(dtype=dt, workspace_bytes=ws, q=P, k=P + 2 * H * D, v=P + 4 * H * D, out=5 * P, B=B, H=H, S=S, D=D, ld=ld,
                                  ldo=ldo or H * D, scale=0.1)


@pytest.mark.parametrize("kern", ATTN_KERNELS, ids=lambda k: k[0])
def test_attention_batch_row_guard(kern):
    """attention.hip:70 / attention5.hip:317: S * ld * 2 < 2^32, ld in steps of 8 elements.  On the near side the forced kernel is planned (the key-split
    form with its two ranges), one step beyond the call is refused with its text -- by every kernel, since none addresses a batch row with 64 bits"""
    _, dt, knobs, D, S, kernel = kern
    ld = attn_edge_ld(S)
    assert S * ld * 2 < 2 ** 32 <= S * (ld + 8) * 2
    for pitch in (ld - 8, ld):
        p = attn_plan(pitch, S, D, knobs, dt)
        assert p.kernel == kernel
        if "attn_split" in knobs:
            assert p.split == 2 and p.jobs > 0
    for pitch in (ld + 8, ld + 16, 2 ** 24):
        with pytest.raises(_lib.DkHipError, match=ATTN_TEXT):
            attn_plan(pitch, S, D, knobs, dt)
    attn_plan(ld, S, D, knobs, dt, ldo=2 ** 24)  # (the output pitch is not part of the guard: the kernels form output addresses in 64 bits)


# conv3x3: (B, H, W, C, O, upsample) of the OUTPUT -> on the near side gemm256v3.hip's conv form, beyond it the 128^2 kernel
CONV_EDGES = [
    ("batch field b:8", (256, 16, 16, 64, 256, 0), [(257, 16, 16, 64, 256, 0)]),
    ("row field y:12", (1, 4096, 16, 64, 256, 0), [(1, 4097, 16, 64, 256, 0), (1, 4112, 16, 64, 256, 0)]),
    ("column field x:12", (1, 16, 4096, 64, 256, 0), [(1, 16, 4097, 64, 256, 0), (1, 16, 4112, 64, 256, 0)]),
    ("input bytes, one image", (1, 2048, 1023, 512, 256, 0), [(1, 2048, 1024, 512, 256, 0)]),
    ("input bytes, issue shape", (1, 2048, 1008, 512, 256, 0), [(1, 2048, 1024, 512, 256, 0)]),
    ("input bytes count the batch", (2, 1024, 1023, 512, 256, 0), [(2, 1024, 1024, 512, 256, 0)]),
    ("input bytes of the upsample form are the source's", (1, 4096, 2046, 512, 256, 1), [(1, 4096, 2048, 512, 256, 1)]),
]


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("edge", CONV_EDGES, ids=lambda e: e[0].replace(" ", "_").replace(",", "").replace(":", ""))
def test_conv3x3_packing_and_byte_guards(edge, dt):
    """gemm256v3.hip:703-704: pixels packed as b:8 | y:12 | x:12 (B <= 256, H <= 4096, W <= 4096) and 31-bit byte offsets into the input
    (cB * H * W * C * 2 < 2^31, over the source of the upsample form)"""
    _, near, far = edge
    B, H, W, C, O, ups = near
    if C == 512:
        src = B * (H >> ups) * (W >> ups) * C * 2
        assert src < 2 ** 31
    for knobs in ({}, dict(gemm=9)):
        with tuned(**knobs):
            assert ops.conv3x3_plan(B, H, W, C, O, ups, dtype=dt).kernel == 3, near
            for shape in far:
                B2, H2, W2, C2, O2, ups2 = shape
                assert ops.conv3x3_plan(B2, H2, W2, C2, O2, ups2, dtype=dt).kernel == 128, shape


# ---- tests/_bigmem.py ---------------------------------------------------------------------------------------------------------------------
def test_boundaries_lie_inside_their_margins():
    for base in (0x7f0000000000, 0x7f00ffffe000, 0x7f0080000200, 0x7f0100000000 - 512, 0x7f01c0000000, 2 ** 32 - 2 ** 28):
        b32, b31 = bm.boundaries(base)
        lo, hi = base + bm.MARGIN, base + bm.ARENA_BYTES - bm.MARGIN
        assert b32 % 2 ** 32 == 0 and lo <= b32 - 2 ** 32 and b32 <= hi and b32 + 2 ** 32 > hi  # the UPPER one, and the one 4 GiB below is inside too
        assert b31 % 2 ** 31 == 0 and (b31 // 2 ** 31) % 2 == 1 and lo <= b31 - 2 ** 31 and b31 <= hi


SHAPES = [((3, 88, 192), 2), ((3, 88, 512), 2), ((512,), 2), ((2, 8, 8, 64), 2), ((2, 16, 16, 64), 2), ((128, 3, 3, 64), 2), ((64,), 2), ((29, 64, 2), 4),
          ((384, 384), 1), ((1, 768), 2), ((2, 2), 4), ((2, 77, 2432), 2), ((77,), 4), ((1100, 320), 2), ((5,), 2)]


@pytest.mark.parametrize("at", [0.4, "row", 0.0, 0.999])
@pytest.mark.parametrize("shape,isz", SHAPES)
def test_place_offset_is_aligned_inside_and_mid_row(shape, isz, at):
    stride = [1] * len(shape)
    for i in range(len(shape) - 2, -1, -1):
        stride[i] = stride[i + 1] * shape[i + 1]
    nbytes = bm.span_elems(shape, stride) * isz
    rows = bm.row_sizes(shape, stride, isz)
    frac = (rows[0] / nbytes if rows else 0.4) if at == "row" else at
    off, align = bm.place_offset(nbytes, rows, frac, isz)
    assert 0 < off < nbytes, "the boundary lies strictly inside the operand"
    assert off % align == 0 and align >= isz and off % isz == 0
    if nbytes > 2 * bm.ALIGN:
        assert align == bm.ALIGN, "an operand of more than two alignment units keeps the allocator's alignment"
    usable = [r for r in rows if align % r != 0 and r < nbytes]
    if usable:
        assert off % usable[0] != 0, "the boundary falls on a row edge"
    if align == bm.ALIGN and frac * nbytes + 3 * align < nbytes:
        assert frac * nbytes <= off <= frac * nbytes + 3 * align, "the boundary is not where it was asked for"


def test_place_offset_uses_the_image_row_where_a_pixel_divides_the_alignment():
    """a 64-channel bf16 pixel is 128 bytes: every 512-byte aligned offset is a pixel edge, so the image row (16 pixels) is the row that counts"""
    off, align = bm.place_offset(2 * 16 * 16 * 128, [128, 16 * 128, 16 * 16 * 128], 0.4, 2)
    assert align == 512 and off % 128 == 0 and off % 2048 != 0


# ---- guards without a planner entry: the refused side through the launch entry points, with made-up pointers -------------------------------------
def no_device():
    """These tests hand made-up pointers to real launch entry points and rely on the refusal coming first.  Should a guard ever regress, the call
    would enqueue kernels on those addresses: where a GPU is visible that is a fault on a shared machine instead of a failed assertion, so they run
    only where none is.  There the launch itself fails in the HIP runtime, which also lets each test call the NEAR side of its edge: that call
    must fail with anything but the guard's text, so a refusal one step further is the address guard's and no other condition's.
    The device modules repeat with pointers into their arena: the attention batch row, the fp8 A span, attention_d512's ld and the 2048 x 1024 fused
    conv.  The count guards (qk_norm_rope, block_residual, guided step, GroupNorm), the fp8 W pitch and the other fused-conv bounds are met here
    only, on a machine without a GPU."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers go to launch entry points: run only where no GPU is visible (tests/test_gpu_address_extents.py and "
                    "test_gpu_address_long.py repeat some of these refusals with real operands; the count guards, the fp8 W pitch and most fused-conv "
                    "bounds are met on a GPU-less machine only)")


def near_side(rc, lib, text):
    """a call on the accepted side of an edge, on a machine without a GPU: it passes every host-side check and fails at the launch"""
    assert rc != 0 and text.encode() not in lib.dk_last_error(), lib.dk_last_error()


def test_row_kernel_count_guards_refuse_with_their_text():
    """elementwise.hip:386 (qk_norm_rope: rows * 2H * D/8 < 2^31 - 512), elementwise.hip:1160 (block_residual: rows * h/8 < 2^31 - 256),
    elementwise.hip:977 (guided step: one image's latent < 2^31 - 2^18 elements) and vae_ops.hip:210 (GroupNorm: one batch row < 2^31 16-byte
    chunks) index their threads with 32 bits.  Their edges lie at 32 GiB of operands, so the accepted side cannot be run; the first count beyond
    each edge must come back with the documented text -- from the launcher's first lines, before any kernel is enqueued (the GroupNorm bound used
    to be asked behind the statistics pass: two launches were enqueued before the refusal)."""
    no_device()
    lib = _lib.load()
    rows = (2 ** 31 - 512) // (2 * 16 * 8)  # H = 16, D = 64: 256 threads' worth of 16-byte chunks a row
    assert rows * 256 == 2 ** 31 - 512
    assert lib.dk_qk_norm_rope_bf16(P, 3072, 0, 1024, rows, 16, 64, 2 * P, 3 * P, 1e-6, None, rows, rows, 0, None) != 0
    assert b"qk_norm_rope: rows * 2H * D/8 must stay below 2^31" in lib.dk_last_error()
    M = -(-(2 ** 31 - 256) // 384)  # h = 3072: 384 chunks a row
    assert (M - 1) * 384 < 2 ** 31 - 256 <= M * 384
    for fn in (lib.dk_block_residual_bf16, lib.dk_block_residual_f16):
        assert fn(P, 3072, 4096, 4352, 2 * P, M, 3072, 0, None) != 0
        assert b"block_residual: rows * h / 8 must stay below 2^31" in lib.dk_last_error()
    for fn in (lib.dk_groupnorm_bf16, lib.dk_groupnorm_f16):
        for HW, Cc in ((2 ** 28, 64), (2 ** 25, 512), (2 ** 31, 8)):
            assert HW * (Cc // 8) == 2 ** 31
            assert fn(P, 2 * P, 1, HW, Cc, 8, 3 * P, 4 * P, 1e-5, 1, 5 * P, None) != 0
            assert b"one batch row must hold < 2^31 16-byte chunks" in lib.dk_last_error(), lib.dk_last_error()
    # guided step (rescale and APG): Hl * Wl * C = 32768 * 32760 * 2 = 2^31 - 2^19 is the first multiple of the patch size at or beyond 2^31 - 2^18
    Hl, Wl, Cc = 32768, 32764, 2
    assert (Hl * (Wl - 2) * Cc < 2 ** 31 - 2 ** 18 <= Hl * Wl * Cc) and Wl % 2 == 0
    for fn in (lib.dk_guided_cfg_step, lib.dk_guided_cfg_step_f16):
        for mode in (1, 2):
            rc = fn(P, 2 * P, 64, 3 * P, 1, 1, Hl, Wl, Cc, 2, 0, 0.75, 5.0, None, 1.0, -0.25, 0.0, 0.0, 0.0, 0.5, 0, 0, None, None, None, 0,
                    mode, 0.5, 0.0, 0.0, 0.0, 0, 0, None, 4 * P, 2 ** 62, None)
            assert rc != 0 and b"the latent of one image must hold fewer than 2^31 elements" in lib.dk_last_error(), lib.dk_last_error()


def fp8_desc(M, seg, stride, lda, ldw, rows):
    d = _lib.dk_gemm_fp8_desc()
    d.A, d.A_scales, d.W, d.w_scale, d.C, d.bias = P, 2 * P, 3 * P, 4 * P, 5 * P, 6 * P
    d.M, d.N, d.K, d.lda, d.ldw, d.ldc = M, 256, 384, lda, ldw, 256
    d.a_seg_len, d.a_seg_stride, d.a_row0, d.a_rows, d.epilogue = seg, stride, 0, rows, 0
    return d


def test_gemm_fp8_guards_refuse_with_their_text():
    """gemm256f8.hip:528: a_rows * lda < 2^32 (1-byte elements) and ldw * 8 < 2^31.  There is no other fp8 kernel and no planner entry: beyond either
    edge dk_gemm_fp8 refuses with the launcher's text.  The A span moves by one segment stride unit (128 rows: whole scale blocks), the W pitch by 16
    bytes; the accepted sides are run on the device (A span) or need a 64 GiB weight (W)"""
    no_device()
    import ctypes as C
    lib = _lib.load()
    near_side(lib.dk_gemm_fp8(C.byref(fp8_desc(384, 128, 349440, 6144, 384, a_rows(384, 128, 349440))), None), lib, F8_TEXT)
    near_side(lib.dk_gemm_fp8(C.byref(fp8_desc(edge_rows(6144), edge_rows(6144), 0, 6144, 384, edge_rows(6144))), None), lib, F8_TEXT)
    near_side(lib.dk_gemm_fp8(C.byref(fp8_desc(384, 384, 0, 384, 2 ** 28 - 16, 384)), None), lib, F8_TEXT)
    for stride in (349568, 349696):  # 349 440 is the last accepted one at lda = 6144 (tests/test_gpu_address_extents.py runs it)
        rows = a_rows(384, 128, stride)
        assert (a_rows(384, 128, 349440) * 6144 < 2 ** 32 <= rows * 6144) and stride % 128 == 0
        assert lib.dk_gemm_fp8(C.byref(fp8_desc(384, 128, stride, 6144, 384, rows)), None) != 0
        assert F8_TEXT.encode() in lib.dk_last_error(), lib.dk_last_error()
    one = edge_rows(6144) + 1  # one segment: any row count; the first one beyond the edge
    assert lib.dk_gemm_fp8(C.byref(fp8_desc(one, one, 0, 6144, 384, one)), None) != 0 and F8_TEXT.encode() in lib.dk_last_error()
    for ldw in (2 ** 28, 2 ** 28 + 16):  # 2^28 - 16 is the last accepted pitch
        assert (2 ** 28 - 16) * 8 < 2 ** 31 <= ldw * 8
        assert lib.dk_gemm_fp8(C.byref(fp8_desc(384, 384, 0, 384, ldw, 384)), None) != 0
        assert F8_TEXT.encode() in lib.dk_last_error(), lib.dk_last_error()


def conv_gn_desc(B, H, W, Cc, O, ldw=None, C2=0, ups=0):
    d = _lib.dk_conv_gn_desc()
    d.x, d.w, d.bias, d.y = P, 2 * P, 3 * P, 4 * P
    if C2:
        d.x2, d.bias2 = 5 * P, 6 * P
    d.gn_silu, d.B, d.H, d.W, d.C, d.O, d.C2 = 0, B, H, W, Cc, O, C2
    d.ldw, d.ldy, d.upsample = ldw or 9 * Cc + C2, O, ups
    return d


@pytest.mark.parametrize("v4", [0, 2], ids=["conv_halo", "conv256v4"])
def test_fused_conv_guards_refuse_with_their_text(v4):
    """conv_halo.hip:525-526 (and conv256v4.hip:288 through them): one image H * W * C * 2 < 2^31 (the source of the upsample form), O * ldw * 2 < 2^31,
    the shortcut's H * W * C2 * 2 < 2^31.  H and W move in steps of 16 pixels, ldw in steps of 8 elements; the first shape beyond each edge is refused
    by dk_conv3x3_gn with the launcher's text under either kernel choice.  (The last accepted shapes launch: tests/test_gpu_address_long.py runs
    2048 x 1008 x 512; conv256v4.hip:293's own bound, ldw * 512 < 2^31, hands over to conv_halo.hip, which no entry point reports.)"""
    no_device()
    import ctypes as C
    lib = _lib.load()
    far = [conv_gn_desc(1, 2048, 1024, 512, 256), conv_gn_desc(1, 2096, 1008, 512, 256), conv_gn_desc(3, 1024, 2048, 512, 256),
           conv_gn_desc(1, 4096, 2048, 512, 256, ups=1), conv_gn_desc(1, 4192, 2016, 512, 256, ups=1),
           conv_gn_desc(1, 64, 64, 128, 256, ldw=2 ** 22), conv_gn_desc(1, 64, 64, 128, 128, ldw=2 ** 23),
           conv_gn_desc(1, 2048, 1024, 64, 128, C2=512), conv_gn_desc(1, 2096, 1008, 64, 128, C2=512)]
    assert 2048 * 1008 * 512 * 2 < 2 ** 31 <= 2048 * 1024 * 512 * 2 and 2080 * 1008 * 512 * 2 < 2 ** 31 <= 2096 * 1008 * 512 * 2 and 256 * (2 ** 22 - 8) * 2 < 2 ** 31
    near = [conv_gn_desc(1, 2048, 1008, 512, 256), conv_gn_desc(1, 2080, 1008, 512, 256), conv_gn_desc(3, 1024, 2032, 512, 256),
            conv_gn_desc(1, 4096, 2016, 512, 256, ups=1), conv_gn_desc(1, 64, 64, 128, 256, ldw=2 ** 22 - 8), conv_gn_desc(1, 64, 64, 128, 128, ldw=2 ** 23 - 8),
            conv_gn_desc(1, 2080, 1008, 64, 128, C2=512)]
    with tuned(conv_v4=v4):
        for d in near:  # the last accepted step of each bound
            near_side(lib.dk_conv3x3_gn_bf16(C.byref(d), None), lib, HALO_TEXT)
        for d in far:
            assert lib.dk_conv3x3_gn_bf16(C.byref(d), None) != 0
            assert HALO_TEXT.encode() in lib.dk_last_error(), ((d.B, d.H, d.W, d.C, d.O, d.ldw, d.C2, d.upsample), lib.dk_last_error())


def test_conv256v4_weight_pitch_guard_hands_over_to_conv_halo():
    """conv256v4.hip:293: ldw * 2 * 256 < 2^31 (ldw < 2^22, in steps of 8 elements).  No entry point reports which fused-conv kernel a launch
    takes, and the two kernels give the same bits; on a machine without a GPU the launch fails in the first HIP call of the launcher it was routed
    to, whose text names that launcher's kernel.  Under conv_v4 = 2 (conv256v4 wherever eligible) the last accepted pitch reaches
    dk_conv256v4_kernel, the first two beyond it dk_conv_halo_kernel; under conv_v4 = 0 every pitch reaches dk_conv_halo_kernel.  (The values on
    both sides: tests/test_gpu_address_extents.py: test_fused_conv_weight_pitch_guards.)"""
    no_device()
    import ctypes as C
    lib = _lib.load()

    def routed_to(v4, O, ldw):
        with tuned(conv_v4=v4):
            near_side(lib.dk_conv3x3_gn_bf16(C.byref(conv_gn_desc(1, 64, 64, 128, O, ldw=ldw)), None), lib, HALO_TEXT)
        text = lib.dk_last_error()
        hits = [k for k in (b"dk_conv256v4_kernel", b"dk_conv_halo_kernel") if k in text]
        assert len(hits) == 1, text
        return hits[0].decode()
    for O in (128, 256):
        assert routed_to(2, O, 2 ** 22 - 16) == routed_to(2, O, 2 ** 22 - 8) == "dk_conv256v4_kernel"
        assert routed_to(0, O, 2 ** 22 - 8) == "dk_conv_halo_kernel"
    for ldw in (2 ** 22, 2 ** 22 + 8, 2 ** 23 - 8):  # (O = 128: still inside conv_halo.hip's own O * ldw * 2 < 2^31)
        assert routed_to(2, 128, ldw) == routed_to(0, 128, ldw) == "dk_conv_halo_kernel"
