"""The VAE at odd sizes on an MI355X: stages that switch between the fused and the unfused route, and the K split of the implicit-GEMM convolution.

The engines pick a kernel per stage from the stage's pixel size (vae_engine.hip: VaeRun::halo_stage): both sides a multiple of 16 -> the fused
norm -> silu -> conv kernels with GroupNorm statistics as tile partials; anything else -> a statistics pass, an apply pass and the implicit-GEMM conv
with the engine's K-split workspace attached.  At the sizes the other files decode (latent 16 x 16, 128 x 128; the tiny configs) every stage takes ONE
of the two routes.  Here:

  operator level: the conv form of gemm256v3.hip with every tile cut along K -- reachable only through a workspace (dk_conv3x3_ws_bf16 / _f16) --
      on the automatic route (96 .. 128 tiles, two pieces, the second starts in the middle of tap 4) and forced onto small shapes (four pieces that
      start mid-tap, three whole images in one tile, the nearest-x2 gather, the residual tail behind the merge); a NaN footprint of one forced shape
      with the workspace and the output's padding columns poisoned;
  engine level: production channel plan (128, 256, 512, 512), decodes whose stages turn from unfused to fused one, two or three upsamplings in,
      encodes that go the other way, the knob values of dk_tune_set("conv_halo", v), and the sizes whose 256-channel stage takes the K split.

Expectations come from tests/test_vae_routes_cpu.py, which pins the planner's answer and the per-stage route table on the CPU.

Gates are the suite's own, nothing is tuned here:
  operators: relative L2 against oracle.vae.conv2d_nhwc in fp32 on the rounded operands < TOL_SINGLE_OP (fp16: tests/test_gpu_vae_f16.py's op_gate,
      TOL_SINGLE_OP / 8); against the same launch with the split off: not bit-identical (the split ran), max |diff| <= 0.02 max|ref| + 1e-2 and fewer
      than 5 % of the elements different -- the bounds of test_conv3x3_on_256_tile_kernel / test_gemm_v3_remainder_split across summation orders;
  decoder bf16: tests/test_gpu_model.py::test_vae_decode_tiny (yardstick on raw, image PSNR > 35 dB, the exact uint8 rule);
  decoder fp16: tests/test_gpu_vae_f16.py::decode_case; encoder: the yardstick / that file's gate on the moments.
Two runs of one problem whose stages take the same routes must agree bit for bit; runs whose routes differ must not (that is the proof that the
default run took the route the table names).  Every figure is printed before it is asserted.

Measured when the file was written (relative L2 of raw / moments, hip-vs-fp32 | emulating-oracle-vs-fp32; PSNR between the two routes' images):
  decoder B = 2 default | conv_halo 0: 8 x 8 bf16 1.677e-2, 1.718e-2 | 1.716e-2, 51.4 dB; f16 2.068e-3, 2.124e-3 | 2.025e-3, 69.3 dB;
      4 x 8 bf16 1.672e-2, 1.700e-2 | 1.692e-2, 52.0 dB; f16 2.083e-3, 2.103e-3 | 2.111e-3, 70.0 dB; 6 x 8 bf16 1.747e-2, 1.768e-2 | 1.806e-2, 54.5 dB;
      f16 2.221e-3, 2.250e-3 | 2.240e-3, 72.8 dB; 3 x 4 bf16 1.807e-2 | 1.755e-2, f16 2.047e-3 | 2.098e-3 (both routes the same bits);
  conv_halo 2, 3: 8 x 8 1.697e-2, 1.696e-2 | 1.716e-2; 6 x 8 1.745e-2 (the same bits) | 1.806e-2;
  K split on | off: 38 x 44 bf16 1.796e-2, 1.790e-2 | 1.804e-2, 53.8 dB; f16 2.211e-3, 2.213e-3 | 2.237e-3, 71.7 dB; 2 x 26 x 30 bf16 1.768e-2,
      1.769e-2 | 1.779e-2, 53.8 dB;
  encoder default, conv_halo 0 (, gemm_split 0): 96 x 80 bf16 2.044e-2, 2.050e-2 | 2.055e-2; f16 2.591e-3, 2.620e-3 | 2.564e-3; 304 x 352 bf16
      2.137e-2, 2.148e-2, 2.138e-2 | 2.131e-2.
What the file found: the unfused image tail (gn + conv + dk_launch_image_post) left the fourth column of `raw` unwritten, where the fused tail stores
zeros and tests/test_gpu_vae_f16.py::decode_case asserts zeros (test_decoder_route_transitions, conv_halo = 0); dk_vae_decode now clears it.

The file name sorts behind tests/test_gpu_fullsize.py on purpose (see the head of tests/test_gpu_vae_f16.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from diffusionkit_amd.config import VAEDecoderConfig, VAEEncoderConfig, float16_vae_config
from diffusionkit_amd.weights import pack_vae, synth_vae_encoder_weights, synth_vae_weights
from oracle import vae as ov
from oracle.mmdit import Prec
from oracle.vae import OracleVAEDecoder, OracleVAEEncoder, to_uint8
from tests import _footprint as fp
from tests._util import BF, TOL_SINGLE_OP, bf16r, max_abs, psnr, rel_l2
from tests.test_vae_routes_cpu import ENGINE_ROUTES, FORCED_KNOBS, KSPLIT_FORCED, KSPLIT_NATURAL, forced_plan, plan_fields

pytestmark = pytest.mark.gpu

F16 = torch.float16
SLAB_FLOATS, FLAG_BYTES = 256 * 256, 4096  # dk_ksplit.h: 256 slabs of 256 x 256 fp32, then the flag region


def tuned(**knobs):
    from tests.test_gpu_op_footprints import tuned as t
    return t(**knobs)


def rnd(dt, *shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dt).float()


def flags_zero(ws, what):
    assert int(ws[-FLAG_BYTES:].sum()) == 0, f"{what}: the flag region of the K-split workspace was not left zero"


# ---- operator level -----------------------------------------------------------------------------------------------------------------------------
def conv_operands(dt, B, H, W, C, O, ups, res):
    """(x, w, b, r) as fp32 values of the element type, H x W the OUTPUT size; the fp32 oracle's result on them"""
    Hs, Ws = (H // 2, W // 2) if ups else (H, W)
    x, w, b = rnd(dt, B, Hs, Ws, C, seed=20), rnd(dt, O, 3, 3, C, seed=21, scale=0.05), rnd(dt, O, seed=22, scale=0.1)
    r = rnd(dt, B, H, W, O, seed=23) if res else None
    ref = ov.conv2d_nhwc(ov.upsample_nearest(x) if ups else x, w, b, Prec())
    return x, w, b, r, (ref + r if res else ref)


def split_conv_case(dev, dt, shape, knobs, want):
    """one conv through dk_conv3x3_ws_*: the device's plan, the oracle gate, and the same launch with the split off"""
    from diffusionkit_amd import ops
    B, H, W, C, O, ups, res = shape
    what = f"conv {shape} {'f16' if dt == F16 else 'bf16'} {knobs}"
    x, w, b, r, ref = conv_operands(dt, *shape)
    ws = ops.gemm_workspace(dev)
    flags_zero(ws, what + " (before)")
    g = lambda t: None if t is None else t.to(dev, dt).contiguous()
    xd, wd, bd, rd = g(x), g(w), g(b), g(r)
    with tuned(**dict(dict(gemm_split=-1), **knobs)):  # (gemm_split is set below: restored with the others)
        got = plan_fields(ops.conv3x3_plan(B, H, W, C, O, int(ups), dtype=dt, res=res, workspace=ws.numel()))
        assert got["n_cu"] == 256 and {k: got[k] for k in want} == want, (what, got)  # what tests/test_vae_routes_cpu.py pins, on the device
        y = ops.conv3x3(xd, wd, bd, upsample=ups, res=rd, workspace=ws)
        flags_zero(ws, what)
        ops.tune("gemm_split", 0)
        p0 = ops.conv3x3_plan(B, H, W, C, O, int(ups), dtype=dt, res=res, workspace=ws.numel())
        assert (p0.kernel, p0.tile_rows, p0.k_pieces, p0.split_tiles) == (3, want["tile_rows"], 1, 0), plan_fields(p0)
        y0 = ops.conv3x3(xd, wd, bd, upsample=ups, res=rd, workspace=ws)
        flags_zero(ws, what + " (split off)")
    assert y.dtype == dt and y.shape == ref.shape
    tol = TOL_SINGLE_OP / 8 if dt == F16 else TOL_SINGLE_OP
    e, e0 = rel_l2(ref, y.float()), rel_l2(ref, y0.float())
    d, frac = max_abs(y0.float(), y.float()), float((y0.float() != y.float()).float().mean())
    bound = 0.02 * float(ref.abs().max()) + 1e-2
    print(f"[vae routes op] {what}: rel-L2 split {e:.3e}, whole {e0:.3e} (gate {tol:.3e}); split against whole: max |diff| {d:.3e} "
          f"(bound {bound:.3e}), {100 * frac:.3f} % of the elements differ")
    assert e < tol and e0 < tol
    assert not torch.equal(y, y0), f"{what}: bit-identical to the unsplit launch -- the K split did not run"
    assert d <= bound
    assert frac < 0.05


NATURAL = [pytest.param(BF, (1, 110, 110, 256, 512, False), id="bf16-110x110-256to512"),
           pytest.param(BF, (2, 104, 120, 512, 256, True), id="bf16-2x104x120-512to256-res"),
           pytest.param(F16, (1, 152, 176, 256, 256, True), id="f16-152x176-256to256-res")]


@pytest.mark.parametrize("dt,key", NATURAL)
def test_conv_k_split_automatic_route(dev, dt, key):
    """96 .. 128 tiles of 256 x 256 and a workspace: gemm256v3's conv form, 224-row tiles, every tile in two pieces; the second piece starts at K-tile
    18 (36) of 4 (8) per tap -- the middle of tap 4 -- and in the two-image shape a tile straddles the image border"""
    B, H, W, C_, O, res = key
    split_conv_case(dev, dt, (B, H, W, C_, O, False, res), {}, KSPLIT_NATURAL[key])


FORCED_SHAPES = sorted({k[:7] for k in KSPLIT_FORCED})
FORCED = [pytest.param(BF, s, mf, id=f"bf16-{'x'.join(map(str, s[:5]))}-mf{mf}") for s in FORCED_SHAPES for mf in (7, 8)]
FORCED.append(pytest.param(F16, (2, 12, 20, 512, 512, 0, True), -1, id="f16-2x12x20x512x512-auto-height"))


@pytest.mark.parametrize("dt,shape,mf", FORCED)
def test_conv_k_split_forced_on_small_shapes(dev, dt, shape, mf):
    """gemm = 9, gemm_split = 1: four K pieces per tile -- pieces that begin in the middle of a tap (ks = 5 at two K-tiles per tap, 18 at eight),
    one tile that holds three whole images, the nearest-x2 gather, the residual tail behind the merge"""
    B, H, W, C_, O, ups, res = shape
    split_conv_case(dev, dt, (B, H, W, C_, O, bool(ups), res), dict(gemm_mf=mf, **FORCED_KNOBS), forced_plan(shape, mf))


def test_conv_k_split_footprint(dev):
    """NaN footprint of one forced shape (2 x 12 x 20, 512 -> 512, residual, 224-row tiles: 6 tiles x 4 pieces, a tile across the image border).
    tests/_footprint.py's conv family: a poisoned input channel of the LAST 64-channel chunk reaches exactly its 3 x 3 neighbourhood, through every
    piece of the reduction (the producers' slabs included), image 1 poisoned leaves image 0 bit-identical.  The workspace is private and poisoned:
    the launch may write rows [0, 224) of the first tiles x (pieces - 1) slabs and its flags; every other slab row keeps its NaN, the flag region ends
    zero.  The output has 8 padding columns per pixel and sentinel margins: untouched."""
    from diffusionkit_amd import _lib, ops
    from tests.test_gpu_op_footprints import run_family
    shape = (2, 12, 20, 512, 512, 0, True)
    B, H, W, C_, O, _, _ = shape
    want = forced_plan(shape, 7)
    lib = _lib.load()
    nbytes = lib.dk_gemm_workspace_bytes()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    slabs = ws[:nbytes - FLAG_BYTES].view(torch.float32).view(256, 256, 256)
    slabs.fill_(fp.NAN)
    ws[-FLAG_BYTES:].zero_()
    ldy = O + 8
    y, guard = fp.guarded(torch.full((B, H, W, ldy), fp.SENTINEL, dtype=BF, device=dev), 64, fp.SENTINEL)
    ops_cpu, ref, cases = fp.conv_family(B, H, W, C_, O, "plain", BF, res=True, tile=8)

    def launch(v):
        d = _lib.dk_conv_desc()
        d.x, d.w, d.bias, d.res, d.y = v["x"].data_ptr(), v["w"].data_ptr(), v["b"].data_ptr(), v["res"].data_ptr(), y.data_ptr()
        d.zeros = ops.zero_page(dev).data_ptr()
        d.B, d.H, d.W, d.C, d.O, d.ldy, d.ldr, d.upsample, d.epilogue = B, H, W, C_, O, ldy, O, 0, ops.DK_EPI_RES
        with tuned(gemm_mf=7, **FORCED_KNOBS):
            plan = _lib.dk_gemm_plan_t()
            _lib.check(lib.dk_conv3x3_ws_plan(C.byref(d), nbytes, C.byref(plan)), "dk_conv3x3_ws_plan")
            got = plan_fields(plan)
            assert {k: got[k] for k in want} == want, got
            _lib.check(lib.dk_conv3x3_ws_bf16(C.byref(d), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "dk_conv3x3_ws_bf16")
        flags_zero(ws, "footprint launch")
        return y[..., :O]
    run_family(dev, BF, ops_cpu, ref, cases, launch, "conv3x3 K split on gemm256v3", guards=[("y", guard)])
    pad = y[..., O:].float()
    assert bool((pad == fp.SENTINEL).all()), "padding columns of the output were written"
    used = want["split_tiles"] * (want["k_pieces"] - 1)
    assert used == 18 and want["tile_rows"] == 224
    torch.cuda.synchronize()
    assert bool(torch.isnan(slabs[used:]).all()), "a slab beyond tiles x (pieces - 1) was written"
    assert bool(torch.isnan(slabs[:used, 224:]).all()), "slab rows beyond the tile height were written"
    # (the last case poisons one residual element, which enters behind the merge: every partial sum of that launch is finite)
    assert not bool(torch.isnan(slabs[:used, :224]).any()), "a producer piece left rows of its slab unwritten"
    assert int(ws[-FLAG_BYTES:].to(torch.int32).abs().sum()) == 0


# ---- engine level -------------------------------------------------------------------------------------------------------------------------------
def _rounded(named, f16):
    return {k: (v.to(F16) if f16 else v).float() for k, v in named.items()}


@functools.lru_cache(maxsize=None)
def decoder(dev, f16):
    """(config, fp32 view of the weights the engine holds, engine): production plan, seeded synthetic weights; one engine per element type"""
    from diffusionkit_amd.engine import VAEDecoderEngine
    vcfg = VAEDecoderConfig()
    named = synth_vae_weights(vcfg, seed=4321)
    c = float16_vae_config(vcfg) if f16 else vcfg
    return vcfg, _rounded(named, f16), VAEDecoderEngine(c, pack_vae(c, named, dev))


@functools.lru_cache(maxsize=None)
def encoder(dev, f16):
    from diffusionkit_amd.engine import VAEEncoderEngine
    cfg = VAEEncoderConfig()
    named = synth_vae_encoder_weights(cfg, seed=99)
    c = float16_vae_config(cfg) if f16 else cfg
    return cfg, _rounded(named, f16), VAEEncoderEngine(c, pack_vae(c, named, dev))


def latent(B, h, w):
    return torch.randn(B, h, w, 16, generator=torch.Generator().manual_seed(1000 * h + w))


def image(B, H, W):
    """an image in [-1, 1] as oracle.pipeline.read_image_array makes it (that function takes the pipeline's multiples of 64 only)"""
    from tests.test_gpu_model import _test_image
    img = torch.from_numpy((_test_image(H, W, seed=3).astype(np.float32) / 255) * 2 - 1.0)[None]
    return torch.cat([img, -img], 0) if B == 2 else img


def _precs(f16):
    return (("fp32", Prec()), ("emu16", Prec(F16)), ("emubf", Prec(BF))) if f16 else (("fp32", Prec()), ("emu", Prec(BF)))


@functools.lru_cache(maxsize=None)
def decoder_oracle(f16, B, h, w):
    """the live oracle of one case, computed once: name -> un-clipped decoder output (shared by the tests of that case, never modified)"""
    vcfg = VAEDecoderConfig()
    wf = _rounded(synth_vae_weights(vcfg, seed=4321), f16)
    z = latent(B, h, w)
    zin = z.to(F16).float() if f16 else bf16r(z)
    return {n: OracleVAEDecoder(vcfg, wf, P)(zin) for n, P in _precs(f16)}


@functools.lru_cache(maxsize=None)
def encoder_oracle(f16, B, H, W):
    cfg = VAEEncoderConfig()
    wf = _rounded(synth_vae_encoder_weights(cfg, seed=99), f16)
    return {n: OracleVAEEncoder(cfg, wf, P)(image(B, H, W)) for n, P in _precs(f16)}


def decode(eng, z, dev, **knobs):
    with tuned(**knobs):
        out = eng.decode(z.to(dev), want_raw=True)
        torch.cuda.synchronize()
    return tuple(t.clone() for t in out)


def gate_decode(out, res, f16, what):
    """bf16: the gates of test_vae_decode_tiny; fp16: those of tests/test_gpu_vae_f16.py::decode_case.  Prints the figures first."""
    img, u8, raw = out
    ref_img = torch.clip(res["fp32"] / 2 + 0.5, 0, 1)
    assert img.shape == ref_img.shape and img.dtype == torch.float32 and u8.dtype == torch.uint8
    if f16:
        from tests.test_gpu_vae_f16 import gate, image16
        assert raw.dtype == F16
        print(f"[vae routes] {what}: hip-vs-fp32 {rel_l2(res['fp32'], raw[..., :3].float()):.3e}, emu-vs-fp32 {rel_l2(res['fp32'], res['emu16']):.3e}")
        gate(raw[..., :3].float(), res["emu16"], res["emubf"], res["fp32"], what + " raw")
        p_h, p_16 = psnr(ref_img, img), psnr(ref_img, image16(res["emu16"]))
        print(f"[vae routes] {what} image: PSNR hip {p_h:.2f} dB, fp16-emulating oracle {p_16:.2f} dB (gate {p_16 - 2.0:.2f} dB)")
        assert p_h >= p_16 - 2.0
        assert torch.equal(img, image16(raw[..., :3].float()))
        assert torch.equal(u8, (img.to(F16) * 255).to(F16).to(torch.uint8))
    else:
        from tests.test_gpu_model import yardstick_ok
        e_h, e_e = rel_l2(res["fp32"], raw[..., :3].float()), rel_l2(res["fp32"], res["emu"])
        p_h = psnr(ref_img, img)
        print(f"[vae routes] {what}: hip-vs-fp32 {e_h:.3e}, emu-vs-fp32 {e_e:.3e}, image PSNR {p_h:.2f} dB")
        yardstick_ok(raw[..., :3].float(), res["emu"], res["fp32"], what + " raw")
        assert p_h > 35.0
        assert torch.equal(u8, (img.to(BF) * 255).to(BF).to(torch.uint8))  # truncation of the bf16 product (mlx/__init__.py:525-526)
        assert psnr(to_uint8(ref_img).float(), u8.float()) > 30.0
    assert torch.all(raw[..., 3].float() == 0)


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def fused_somewhere(routes):
    return "F" in "".join(routes)


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "f16"])
@pytest.mark.parametrize("hw", [(8, 8), (4, 8), (6, 8), (3, 4)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_decoder_route_transitions(dev, hw, f16):
    """B = 2; the stages start unfused and turn fused one (8 x 8), two (4 x 8) or three (6 x 8) upsamplings later, or never (3 x 4: the unfused
    image tail, dk_launch_image_post).  The hand-offs: n_part and the statistics table from a pass against from a conv's tile partials.  The same
    decode with conv_halo = 0 passes the same gates and, where the table has a fused stage, differs in its bits (the default took the fused stages);
    without one it is the same sequence of launches, bit for bit."""
    h, w = hw
    routes, routes0 = ENGINE_ROUTES[("dec", 2, h, w, -1)], ENGINE_ROUTES[("dec", 2, h, w, 0)]
    assert not fused_somewhere(routes0)
    _, _, eng = decoder(dev, f16)
    res = decoder_oracle(f16, 2, h, w)
    z = latent(2, h, w)
    what = f"decoder {'f16' if f16 else 'bf16'} latent {h} x {w}"
    out = decode(eng, z, dev)
    gate_decode(out, res, f16, what + f" routes {routes}")
    out0 = decode(eng, z, dev, conv_halo=0)
    gate_decode(out0, res, f16, what + " conv_halo 0")
    print(f"[vae routes] {what}: PSNR between the default and the conv_halo = 0 image {psnr(out0[0], out[0]):.2f} dB")
    if fused_somewhere(routes):
        assert not torch.equal(out[2], out0[2]), f"{what}: bit-identical to conv_halo = 0 -- no stage took the fused route"
    else:
        assert same_bits(out, out0), f"{what}: no stage is fused, yet conv_halo = 0 changes the result"


@pytest.mark.parametrize("hw", [(8, 8), (6, 8)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_decoder_conv_halo_knob_values(dev, hw):
    """dk_tune_set("conv_halo", 2 / 3) at the engine level, bf16.  3: fused resnets around upsampling convs on the implicit-GEMM kernel -- the resnet
    behind one finds n_part = 0 and takes a statistics pass for its norm1.  2: stages with 256 and more output channels unfused, the 128-channel
    level and the image tail fused.  Each passes the oracle gates; and over the knob values -1, 0, 2, 3 two decodes agree bit for bit exactly when the
    table gives their stages the same routes (6 x 8: knobs 2 and 3 coincide; 8 x 8: all four differ)."""
    h, w = hw
    _, _, eng = decoder(dev, False)
    res = decoder_oracle(False, 2, h, w)
    z = latent(2, h, w)
    outs = {}
    for knob in (-1, 0, 2, 3):
        outs[knob] = decode(eng, z, dev, conv_halo=knob)
        if knob in (2, 3):
            gate_decode(outs[knob], res, False, f"decoder bf16 latent {h} x {w} conv_halo {knob} routes {ENGINE_ROUTES[('dec', 2, h, w, knob)]}")
    knobs = sorted(outs)
    for i, a in enumerate(knobs):
        for b in knobs[i + 1:]:
            same_routes = ENGINE_ROUTES[("dec", 2, h, w, a)] == ENGINE_ROUTES[("dec", 2, h, w, b)]
            print(f"[vae routes] latent {h} x {w}: conv_halo {a} against {b}: same routes {same_routes}, image PSNR {psnr(outs[a][0], outs[b][0]):.2f} dB")
            assert same_bits(outs[a], outs[b]) == same_routes, f"conv_halo {a} against {b}: routes equal {same_routes}, bits say otherwise"
    assert ENGINE_ROUTES[("dec", 2, h, w, 3)] != ENGINE_ROUTES[("dec", 2, h, w, -1)]  # (so the loop above sees the knob-3 branch)


@pytest.mark.parametrize("B,h,w,f16", [(1, 38, 44, False), (1, 38, 44, True), (2, 26, 30, False)], ids=["bf16-38x44", "f16-38x44", "bf16-2x26x30"])
def test_decoder_natural_k_split_stage(dev, B, h, w, f16):
    """the 256-channel level at 152 x 176 (one image) / 104 x 120 (two): unfused, 96 .. 128 tiles, so its convs run cut in two along K through the
    engine's workspace.  The decode with gemm_split = 0 passes the same gates and differs in its bits; a third decode on the same engine equals the
    first bit for bit (the flag region was left clean, the statistics are deterministic)."""
    assert ENGINE_ROUTES[("dec", B, h, w, -1)] == ("UUUF", "UUF", "F")
    _, _, eng = decoder(dev, f16)
    res = decoder_oracle(f16, B, h, w)
    z = latent(B, h, w)
    what = f"decoder {'f16' if f16 else 'bf16'} {B} x latent {h} x {w}"
    out = decode(eng, z, dev)
    gate_decode(out, res, f16, what)
    out0 = decode(eng, z, dev, gemm_split=0)
    gate_decode(out0, res, f16, what + " gemm_split 0")
    print(f"[vae routes] {what}: PSNR between the split and the unsplit image {psnr(out0[0], out[0]):.2f} dB")
    assert not torch.equal(out[2], out0[2]), f"{what}: bit-identical with gemm_split = 0 -- no conv was cut along K"
    again = decode(eng, z, dev)
    assert same_bits(out, again), f"{what}: a repeated decode on the same engine differs"


def encode(eng, img, dev, **knobs):
    with tuned(**knobs):
        mom = eng.encode(img.to(dev))
        torch.cuda.synchronize()
    return mom.clone()


def gate_encode(mom, res, f16, cfg, what):
    hid = mom[..., :cfg.out_channels].float()
    assert hid.shape == res["fp32"].shape
    if f16:
        from tests.test_gpu_vae_f16 import gate
        assert mom.dtype == F16
        print(f"[vae routes] {what}: hip-vs-fp32 {rel_l2(res['fp32'], hid):.3e}, emu-vs-fp32 {rel_l2(res['fp32'], res['emu16']):.3e}")
        gate(hid, res["emu16"], res["emubf"], res["fp32"], what + " moments")
    else:
        from tests.test_gpu_model import yardstick_ok
        print(f"[vae routes] {what}: hip-vs-fp32 {rel_l2(res['fp32'], hid):.3e}, emu-vs-fp32 {rel_l2(res['fp32'], res['emu']):.3e}")
        yardstick_ok(hid, res["emu"], res["fp32"], what + " moments")


@pytest.mark.parametrize("B,H,W,f16", [(2, 96, 80, False), (2, 96, 80, True), (1, 304, 352, False)], ids=["bf16-2x96x80", "f16-2x96x80", "bf16-304x352"])
def test_encoder_fused_then_unfused(dev, B, H, W, f16):
    """the encoder goes the other way: a fused first level, then halved sizes that are no multiples of 16 -- three unfused levels and the mid block.
    304 x 352: the 152 x 176 level's 256 -> 256 convs take the K split; the encode with gemm_split = 0 passes the same gate and differs in its bits,
    a third encode equals the first."""
    assert ENGINE_ROUTES[("enc", B, H, W, -1)] == ("FUUU", "U")
    cfg, _, eng = encoder(dev, f16)
    res = encoder_oracle(f16, B, H, W)
    img = image(B, H, W)
    what = f"encoder {'f16' if f16 else 'bf16'} {B} x image {H} x {W}"
    mom = encode(eng, img, dev)
    gate_encode(mom, res, f16, cfg, what)
    mom_u = encode(eng, img, dev, conv_halo=0)
    gate_encode(mom_u, res, f16, cfg, what + " conv_halo 0")
    assert not torch.equal(mom, mom_u), f"{what}: bit-identical to conv_halo = 0 -- the first level did not take the fused route"
    if (H, W) == (304, 352):
        mom0 = encode(eng, img, dev, gemm_split=0)
        gate_encode(mom0, res, f16, cfg, what + " gemm_split 0")
        assert not torch.equal(mom, mom0), f"{what}: bit-identical with gemm_split = 0 -- no conv was cut along K"
        assert torch.equal(mom, encode(eng, img, dev)), f"{what}: a repeated encode on the same engine differs"
