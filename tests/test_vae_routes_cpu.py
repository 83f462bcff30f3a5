"""Host-only pins of the VAE's kernel routes (no GPU): what tests/test_gpu_vae_routes.py relies on.

The VAE engines pick a kernel per stage from the stage's pixel size (vae_engine.hip: VaeRun::halo_stage) and the implicit-GEMM convolution picks
its kernel, tile height and K split from the tile count (gemm.hip: dk_gemm_route, route_v3, dk_plan_split).  The GPU tests compare those paths
with the oracle at the smallest shapes that reach them; this file pins the planner's answer for every one of those shapes, so that a later routing
change cannot quietly empty them -- it fails here first, on a laptop (without a GPU the rules assume 256 compute units, the MI355X's count).

Two tables, both imported by the GPU tests:
  KSPLIT_NATURAL / KSPLIT_FORCED -- the conv shapes and the dk_gemm_plan_t fields they must report through dk_conv3x3_ws_plan(_f16);
  ENGINE_ROUTES -- per engine case the fused (F) / unfused (U) pattern of its stages, re-derived below from halo_stage's conditions."""
import pytest
import torch

from diffusionkit_amd import _lib, ops
from diffusionkit_amd.config import VAEDecoderConfig, VAEEncoderConfig

BF, F16 = torch.bfloat16, torch.float16
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(F16, id="f16")]


def ws_bytes():
    return _lib.load().dk_gemm_workspace_bytes()


def plan_fields(p):
    return {n: getattr(p, n) for n, _ in p._fields_}


class tuned:
    """dk_tune_set knobs for the body, back to -1 (automatic) afterwards"""

    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            ops.tune(k, v)

    def __exit__(self, *exc):
        for k in self.knobs:
            ops.tune(k, -1)


# ---- the K split of the implicit-GEMM convolution ---------------------------------------------------------------------------------------------
# (B, H, W, C, O, residual) with H x W the OUTPUT size -> plan fields with the engines' workspace attached.  The automatic route: 96 .. 128
# 256^2-tiles send the launch to gemm256v3's conv form, route_v3 picks 224-row tiles and dk_plan_split cuts EVERY tile in two.  The second piece
# starts at K-tile ks: 18 with 4 K-tiles per tap (C = 256), 36 with 8 (C = 512) -- the middle of tap 4 both times; in the two-image shape a
# 224-row tile straddles the image border (12480 pixels per image = 55.7 tiles).
KSPLIT_NATURAL = {
    (1, 152, 176, 256, 256, True): dict(kernel=3, tile_rows=224, tiles=120, split_tiles=120, k_pieces=2, ks=18, workgroups=240),
    (2, 104, 120, 512, 256, True): dict(kernel=3, tile_rows=224, tiles=112, split_tiles=112, k_pieces=2, ks=36, workgroups=224),
    (1, 110, 110, 256, 512, False): dict(kernel=3, tile_rows=224, tiles=110, split_tiles=110, k_pieces=2, ks=18, workgroups=220),
}
# Forced (tune gemm = 9, gemm_split = 1): (B, H, W, C, O, upsample, residual, gemm_mf) -> plan fields.  Four K pieces each; ks = 5 with two
# K-tiles per tap and ks = 18 with eight start pieces in the middle of a tap, the 64-channel shape holds three whole images in ONE tile, the first
# goes through the nearest-x2 gather, the second through the residual tail behind the merge (224- and 256-row tiles).
KSPLIT_FORCED = {
    (1, 24, 40, 128, 256, 1, False, -1): dict(kernel=3, tile_rows=256, tiles=4, split_tiles=4, k_pieces=4, ks=5, workgroups=16),
    (2, 12, 20, 512, 512, 0, True, -1): dict(kernel=3, tile_rows=224, tiles=6, split_tiles=6, k_pieces=4, ks=18, workgroups=24),
    (2, 12, 20, 512, 512, 0, True, 8): dict(kernel=3, tile_rows=256, tiles=4, split_tiles=4, k_pieces=4, ks=18, workgroups=16),
    (3, 6, 10, 64, 256, 0, False, -1): dict(kernel=3, tiles=1, split_tiles=1, k_pieces=4, ks=3, workgroups=4),
}
FORCED_KNOBS = dict(gemm=9, gemm_split=1)


def forced_plan(shape, mf):
    """the plan of a KSPLIT_FORCED shape (B, H, W, C, O, upsample, residual) under FORCED_KNOBS and gemm_mf = mf: the table's entry for -1 (the
    automatic height); for a forced height 7 / 8 every tile of 32 mf rows in four pieces, the cut points (ks) those of the table"""
    if mf == -1:
        return dict(KSPLIT_FORCED[tuple(shape) + (-1,)])
    B, H, W, C, O = shape[:5]
    tiles = -(-B * H * W // (32 * mf)) * (O // 256)
    ks = {v["ks"] for k, v in KSPLIT_FORCED.items() if k[:7] == tuple(shape)}
    assert len(ks) == 1
    return dict(kernel=3, tile_rows=32 * mf, tiles=tiles, split_tiles=tiles, k_pieces=4, ks=ks.pop(), workgroups=4 * tiles)


def assert_plan(p, want, what):
    got = plan_fields(p)
    assert got["launches"] == 1 and got["n_cu"] == 256, (what, got)
    assert {k: got[k] for k in want} == want, (what, got)


@pytest.mark.parametrize("dtype", DTYPES)
def test_natural_shapes_take_the_k_split_with_a_workspace_only(dtype):
    for (B, H, W, C, O, res), want in KSPLIT_NATURAL.items():
        assert_plan(ops.conv3x3_plan(B, H, W, C, O, dtype=dtype, res=res, workspace=ws_bytes()), want, (B, H, W, C, O))
        assert want["split_tiles"] == want["tiles"] and want["workgroups"] == 2 * want["tiles"]
        # the second piece starts inside a tap: ks is no multiple of the K-tiles per tap
        assert want["ks"] % (C // 64) != 0 and want["ks"] // (C // 64) == 4
        # without a workspace (dk_conv3x3_bf16 / ops.conv3x3 as before): the 128^2 tiles, whole
        for p in (ops.conv3x3_plan(B, H, W, C, O, dtype=dtype, res=res), ops.conv3x3_plan(B, H, W, C, O, dtype=dtype, res=res, workspace=0)):
            assert_plan(p, dict(kernel=128, tile_rows=128, split_tiles=0, k_pieces=1, ks=9 * C // 64), (B, H, W, C, O, "no workspace"))
    B, H, W, C, O, _ = (2, 104, 120, 512, 256, True)
    assert (H * W) % 224 != 0 and (H * W) // 224 < (B * H * W) // 224  # a tile that holds the last rows of image 0 and the first of image 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_forced_shapes_are_cut_in_four(dtype):
    for (B, H, W, C, O, ups, res, mf), want in KSPLIT_FORCED.items():
        with tuned(gemm_mf=mf, **FORCED_KNOBS):
            assert_plan(ops.conv3x3_plan(B, H, W, C, O, ups, dtype=dtype, res=res, workspace=ws_bytes()), want, (B, H, W, C, O, ups, mf))
    for mf in (7, 8):  # (the GPU tests run every forced shape at both heights: still four pieces, the same cut points)
        with tuned(gemm_mf=mf, **FORCED_KNOBS):
            for shape in sorted({k[:7] for k in KSPLIT_FORCED}):
                B, H, W, C, O, ups, res = shape
                want = forced_plan(shape, mf)
                assert_plan(ops.conv3x3_plan(B, H, W, C, O, ups, dtype=dtype, res=res, workspace=ws_bytes()), want, (shape, mf))
                if shape + (mf,) in KSPLIT_FORCED:
                    assert {k: want[k] for k in KSPLIT_FORCED[shape + (mf,)]} == KSPLIT_FORCED[shape + (mf,)]
    with tuned(**FORCED_KNOBS):
        # three whole images in one tile; pieces that start inside a tap
        assert 3 * 6 * 10 <= 224
        assert KSPLIT_FORCED[(1, 24, 40, 128, 256, 1, False, -1)]["ks"] % (128 // 64) != 0
        assert KSPLIT_FORCED[(2, 12, 20, 512, 512, 0, True, -1)]["ks"] % (512 // 64) != 0
        # the stride-2 form has no 256-column kernel: the 128^2 tiles, whole, whatever the knobs say
        assert_plan(ops.conv3x3_plan(2, 20, 12, 256, 256, 2, dtype=dtype, workspace=ws_bytes()),
                    dict(kernel=128, tile_rows=128, split_tiles=0, k_pieces=1, workgroups=8), "stride 2")
    # without the knobs the small shapes stay on the 128^2 tiles, workspace or not
    for (B, H, W, C, O, ups, res, mf) in KSPLIT_FORCED:
        assert ops.conv3x3_plan(B, H, W, C, O, ups, dtype=dtype, res=res, workspace=ws_bytes()).kernel == 128


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_in_at_full_size_is_not_split(dtype):
    """conv_in of a 128 x 128 latent (64 -> 512 channels): 128 tiles, inside the workspace rule's 96 .. 128 window, so the launch goes to
    gemm256v3's conv form -- but two pieces of a 9-step reduction save 4 K-tile steps, which dk_plan_split's cost model declines"""
    assert_plan(ops.conv3x3_plan(1, 128, 128, 64, 512, dtype=dtype, workspace=ws_bytes()),
                dict(kernel=3, tiles=128, split_tiles=0, k_pieces=1, workgroups=128, ks=9), "conv_in 128 x 128")


def test_a_workspace_the_split_cannot_use_is_refused():
    """dk_conv3x3_ws_*: short, misaligned or NULL -> an error that names the rule, never an unsplit launch (host only: the checks come first)"""
    import ctypes as C
    lib = _lib.load()
    with pytest.raises(_lib.DkHipError, match="too small"):
        ops.conv3x3_plan(1, 110, 110, 256, 512, workspace=ws_bytes() - 1)
    with pytest.raises(_lib.DkHipError, match="too small"):
        ops.conv3x3_plan(1, 110, 110, 256, 512, dtype=F16, workspace=4096)
    d, plan = _lib.dk_conv_desc(), _lib.dk_gemm_plan_t()
    assert lib.dk_conv3x3_ws_plan(C.byref(d), ws_bytes(), None) != 0 and b"null plan" in lib.dk_last_error()
    for fn in (lib.dk_conv3x3_ws_bf16, lib.dk_conv3x3_ws_f16):
        assert fn(C.byref(d), 0x10000, ws_bytes() - 1, None) != 0 and b"too small" in lib.dk_last_error()
        assert fn(C.byref(d), 0x10080, ws_bytes(), None) != 0 and b"256-byte aligned" in lib.dk_last_error()
        assert fn(C.byref(d), None, ws_bytes(), None) != 0 and b"256-byte aligned" in lib.dk_last_error()
    assert plan.launches == 0


def test_new_symbols_in_header_library_and_ctypes_table():
    import re
    lib = _lib.load()
    header = set(re.findall(r"\b(dk_[a-z0-9_]+)\s*\(", open(_lib.HEADER_PATH).read()))
    for s in ("dk_conv3x3_ws_bf16", "dk_conv3x3_ws_f16", "dk_conv3x3_ws_plan", "dk_conv3x3_ws_plan_f16"):
        assert s in header and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.dk_abi_version() == 5  # (additive)


# ---- the engines' stages ------------------------------------------------------------------------------------------------------------------------
# Per engine case the route of every stage, F = fused norm -> silu -> conv (conv_halo.hip / conv256v4.hip), U = gn() + conv():
#   decoder (kind, batch, latent h, w, conv_halo knob) -> (levels, ups, tail): `levels` one letter per resolution level in execution order
#       (latent size and the mid block first, 512 / 512 / 256 / 128 channels), `ups` the three upsampling convs, `tail` the image tail
#       (conv_norm_out -> silu -> conv_out -> clip / uint8 in one launch, or gn + conv + dk_launch_image_post);
#   encoder (kind, batch, image H, W, knob) -> (levels, mid): the four levels (128 / 256 / 512 / 512 channels) and the mid block; the stride-2
#       convs, conv_in and conv_out are always implicit GEMMs.
ENGINE_ROUTES = {
    # route transitions (B = 2)
    ("dec", 2, 8, 8, -1): ("UFFF", "FFF", "F"),
    ("dec", 2, 4, 8, -1): ("UUFF", "UFF", "F"),
    ("dec", 2, 6, 8, -1): ("UUUF", "UUF", "F"),
    ("dec", 2, 3, 4, -1): ("UUUU", "UUU", "U"),   # no fused stage, and the unfused image tail
    ("dec", 2, 8, 8, 0): ("UUUU", "UUU", "U"),
    ("dec", 2, 4, 8, 0): ("UUUU", "UUU", "U"),
    ("dec", 2, 6, 8, 0): ("UUUU", "UUU", "U"),
    ("dec", 2, 3, 4, 0): ("UUUU", "UUU", "U"),
    # knob 3: fused resnets around unfused upsampling convs (the resnet behind one takes a statistics pass for its norm1)
    ("dec", 2, 8, 8, 3): ("UFFF", "UUU", "F"),
    ("dec", 2, 6, 8, 3): ("UUUF", "UUU", "F"),
    # knob 2: stages with 256 and more output channels stay unfused
    ("dec", 2, 8, 8, 2): ("UUUF", "UUU", "F"),
    ("dec", 2, 6, 8, 2): ("UUUF", "UUU", "F"),
    # natural K-split stages: the 256-channel level is unfused at 152 x 176 (B = 1) / 104 x 120 (B = 2), the last level fused
    ("dec", 1, 38, 44, -1): ("UUUF", "UUF", "F"),
    ("dec", 2, 26, 30, -1): ("UUUF", "UUF", "F"),
    ("enc", 2, 96, 80, -1): ("FUUU", "U"),
    ("enc", 1, 304, 352, -1): ("FUUU", "U"),
}


def halo_stage(H, W, Cin, Cout, knob, G):
    """VaeRun::halo_stage (vae_engine.hip)"""
    if knob == 0 or H % 16 or W % 16 or Cin % 64 or Cout % 128:
        return False
    if H * W * max(Cin, Cout) * 2 >= 1 << 31:
        return False
    if G <= 0 or Cout % G or 128 % (Cout // G) or Cout // G > 64:
        return False
    return knob != 2 or Cout < 256


def _letter(flags):
    assert len(set(flags)) == 1, flags  # every resnet of a level takes the same route in these cases
    return "F" if flags[0] else "U"


def decoder_routes(cfg, h, w, knob):
    """dk_vae_decode's walk: mid block and up_blocks n-1 .. 0, each followed by its upsampling conv, then the image tail"""
    ch, G = cfg.block_out_channels, cfg.resnet_groups
    H, W, C = h, w, ch[-1]
    levels, ups = [], []
    for j in range(len(ch) - 1, -1, -1):
        flags = [halo_stage(H, W, C, C, knob, G)] * 2 if j == len(ch) - 1 else []  # mid_blocks.0 / .2
        flags += [halo_stage(H, W, C if r == 0 else ch[j], ch[j], knob, G) for r in range(cfg.layers_per_block)]
        levels.append(_letter(flags))
        C = ch[j]
        if j > 0:
            H, W = 2 * H, 2 * W
            ups.append("F" if knob != 3 and halo_stage(H, W, C, C, knob, G) else "U")
    tail = knob != 0 and H % 16 == 0 and W % 16 == 0 and C % 64 == 0 and cfg.out_channels <= 4 and H * W * C * 2 < 1 << 31
    return "".join(levels), "".join(ups), "F" if tail else "U"


def encoder_routes(cfg, Hi, Wi, knob):
    ch, G = cfg.block_out_channels, cfg.resnet_groups
    H, W, C = Hi, Wi, ch[0]
    levels = []
    for i in range(len(ch)):
        levels.append(_letter([halo_stage(H, W, C if r == 0 else ch[i], ch[i], knob, G) for r in range(cfg.layers_per_block)]))
        C = ch[i]
        if i < len(ch) - 1:
            H, W = H // 2, W // 2
    return "".join(levels), "F" if halo_stage(H, W, C, C, knob, G) else "U"


def test_engine_route_table_follows_halo_stage():
    dec, enc = VAEDecoderConfig(), VAEEncoderConfig()
    assert dec.block_out_channels == enc.block_out_channels == (128, 256, 512, 512) and dec.resnet_groups == enc.resnet_groups == 32
    for (kind, B, h, w, knob), want in ENGINE_ROUTES.items():
        got = decoder_routes(dec, h, w, knob) if kind == "dec" else encoder_routes(enc, h, w, knob)
        assert got == want, ((kind, B, h, w, knob), got, want)
    # what the GPU tests were chosen for
    R = ENGINE_ROUTES
    assert [R[("dec", 2, h, w, -1)][0] for h, w in ((8, 8), (4, 8), (6, 8), (3, 4))] == ["UFFF", "UUFF", "UUUF", "UUUU"]
    assert R[("dec", 2, 3, 4, -1)][2] == "U" and R[("dec", 2, 6, 8, 0)][2] == "U"  # the unfused image tail, twice
    assert R[("dec", 2, 8, 8, 3)] == ("UFFF", "UUU", "F")  # fused resnet -> unfused upsample -> fused resnet
    assert R[("dec", 2, 8, 8, 2)][0] == "UUUF" and R[("dec", 2, 8, 8, 2)][2] == "F"
    assert R[("enc", 2, 96, 80, -1)] == ("FUUU", "U") and R[("enc", 1, 304, 352, -1)] == ("FUUU", "U")


@pytest.mark.parametrize("dtype", DTYPES)
def test_engine_cases_reach_the_k_split_in_their_256_channel_stage(dtype):
    """the unfused 256-channel level of the natural cases: its 512 -> 256 and 256 -> 256 convs (decoder: conv1 of the first resnet and every other
    conv of the level; encoder at 152 x 176: every conv but the first) are routed to the K split with the engine's workspace"""
    W_ = ws_bytes()
    for (B, H, W) in ((1, 152, 176), (2, 104, 120)):
        for cin in (512, 256):
            p = ops.conv3x3_plan(B, H, W, cin, 256, dtype=dtype, res=cin == 256, workspace=W_)
            assert (p.kernel, p.tile_rows, p.k_pieces) == (3, 224, 2) and p.split_tiles == p.tiles, (B, H, W, cin, plan_fields(p))
    # the encoder's 128 -> 256 conv at 152 x 176 goes to the same kernel whole: 9 saved K-tile steps do not pay for the slab round trip
    p = ops.conv3x3_plan(1, 152, 176, 128, 256, dtype=dtype, workspace=W_)
    assert (p.kernel, p.tile_rows, p.tiles, p.k_pieces) == (3, 256, 105, 1), plan_fields(p)
    # the decoder's upsampling conv INTO that level (512 -> 512 over the nearest-x2 view): two column tiles per row tile, more than 192 tiles, whole
    p = ops.conv3x3_plan(1, 152, 176, 512, 512, 1, dtype=dtype, workspace=W_)
    assert (p.kernel, p.k_pieces) == (3, 1) and p.tiles >= 192, plan_fields(p)
    # latent 8 x 8 ... 6 x 8 (the transition cases): no conv of theirs is split -- they exercise the stage hand-offs, not the K split
    for (B, H, W, cin, O) in ((2, 8, 8, 512, 512), (2, 48, 64, 256, 256), (2, 24, 32, 512, 256)):
        assert ops.conv3x3_plan(B, H, W, cin, O, dtype=dtype, workspace=W_).k_pieces == 1
