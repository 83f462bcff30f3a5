"""Tiny latent decoder on an MI355X (csrc/tae.hip) against the float64 reference of tests/_tae.py with the kernels' rounding points on:
the fused Block at its tile edges, its bit-identity with the chain of single convs, the zero padding of every conv inside the fusion, the
single convs per element, and the whole decoder (PSNR, batch consistency, poisoned workspace)."""
import pytest
import torch

from diffusionkit_amd import ops
from diffusionkit_amd.weights import pack_tae, synth_tae_weights
from tests import _engine_state as es
from tests import _tae as T
from tests._gates import C_GEMM, conv_ref64, epilogue_bound
from tests._numeric_range import BF, spacing, worst
from tests._util import psnr, randn

pytestmark = pytest.mark.gpu


def run_block(x, ws, bs, dev):
    g = lambda t: t.to(BF).to(dev)
    return ops.tae_block(g(x), [g(w) for w in ws], [g(b) for b in bs])


@pytest.mark.parametrize("grid", T.BLOCK_GRIDS, ids=str)
def test_block_at_the_tile_edges_and_equal_to_its_chain(dev, grid):
    assert (T.TH, T.TW) == (ops.TAE_TILE, ops.TAE_TILE)  # (the grids are laid around the kernel's tile)
    x, ws, bs = T.block_operands(grid)
    got, ref = run_block(x, ws, bs, dev), T.block(x, ws, bs, True)
    r = worst((got.double().cpu() - ref).abs(), spacing(ref, BF) + T.C_BLOCK * T.block_unit(x, ws, bs))
    print(f"block {grid}: worst |got - ref| / gate = {r:.3g}")
    assert r <= 1.0
    # three single launches (bias, ReLU), the last with the skip: the same bits -- both walk K tap by tap, low 32 channels first
    g = lambda t: t.to(BF).to(dev)
    xd = g(x)
    h = ops.tae_conv(xd, g(ws[0]), g(bs[0]))
    h = ops.tae_conv(h, g(ws[1]), g(bs[1]))
    chain = ops.tae_conv(h, g(ws[2]), g(bs[2]), skip=xd)
    es.assert_identical({"chain": chain, "fused": got}, f"block {grid}")


def test_block_pads_every_conv_with_zeros(dev):
    """all operands positive: no ReLU is inactive, and intermediates left un-zeroed outside the image would move the border by more than ten
    gates (tests/test_tae_cpu.py::test_measured_constants holds the reference to that); a partial tile in both directions"""
    x, ws, bs = T.block_operands((1, 5, 7), positive=True)
    ref, bad = T.block(x, ws, bs, True), T.block(x, ws, bs, True, keep_out_of_image=True)
    gate = spacing(ref, BF) + T.C_BLOCK * T.block_unit(x, ws, bs)
    d = (ref - bad).abs() / gate
    assert min(float(d[:, 0].min()), float(d[:, -1].min()), float(d[:, :, 0].min()), float(d[:, :, -1].min())) > 10.0
    assert worst((run_block(x, ws, bs, dev).double().cpu() - ref).abs(), gate) <= 1.0


def conv_case(kind, grid):
    B, H, W = grid
    if kind == "first":
        lat = randn(B, H, W, 16, seed=340, scale=2.0)
        return lat, T.clamp_latent(lat, 0.5, 0.25).float(), randn(64, 3, 3, 16, seed=341, scale=0.1), randn(64, seed=342, scale=0.1)
    x = randn(B, H, W, 64, seed=343)
    if kind == "last":
        return x, x, randn(3, 3, 3, 64, seed=344, scale=0.02), T.rb(randn(3, seed=345, scale=0.1) + 0.5)
    return x, x, randn(64, 3, 3, 64, seed=346, scale=0.06), (torch.zeros(64) if kind == "ups" else randn(64, seed=347, scale=0.1))


@pytest.mark.parametrize("grid", T.CONV_GRIDS, ids=str)
@pytest.mark.parametrize("kind", ["first", "ups", "plain", "skip", "last"])
def test_single_convs(dev, kind, grid):
    raw, xin, w, b = conv_case(kind, grid)
    g = lambda t: t.to(BF).to(dev)
    packed = pack_tae({"w": w, "b": b}, dev)
    pre, unit = conv_ref64(xin, w, b, "ups" if kind == "ups" else "plain")
    if kind == "last":
        img, u8 = ops.tae_conv(g(raw), packed["w"], packed["b"], kind="last")
        _, bound = epilogue_bound(pre, unit, BF, "bias")
        assert worst((img.double().cpu() - pre.clamp(0, 1)).abs(), bound) <= 1.0
        # bytes: exact, except where the fp64 value lies within the fp32-accumulation distance of a rounding boundary (every step of the tail is monotone)
        lo, hi = T.image_tail(pre - C_GEMM * unit)[1], T.image_tail(pre + C_GEMM * unit)[1]
        assert float((lo != hi).double().mean()) <= 0.01, "more than 1 % of the reference bytes sit on a rounding boundary"
        u8 = u8.cpu()
        assert bool(((u8 >= lo) & (u8 <= hi)).all()) and int((hi - lo).max()) <= 1
        return
    if kind == "first":
        got = ops.tae_conv(raw.to(dev), packed["w"], packed["b"], kind="first", scale=0.5, shift=0.25)
    elif kind == "ups":
        got = ops.tae_conv(g(raw), packed["w"], None, relu=False, upsample=True)
    else:
        skip = randn(*raw.shape, seed=348) if kind == "skip" else None
        got = ops.tae_conv(g(raw), packed["w"], packed["b"], skip=g(skip) if kind == "skip" else None)
    ref, bound = epilogue_bound(pre, unit, BF, "res" if kind == "skip" else "bias", skip if kind == "skip" else None)
    ref = ref if kind == "ups" else torch.relu(ref)  # (ReLU is monotone and 1-Lipschitz: the bound of the pre-activation holds behind it)
    r = worst((got.double().cpu() - ref).abs(), bound)
    print(f"conv {kind} {grid}: worst |got - ref| / gate = {r:.3g}")
    assert got.shape == ref.shape and r <= 1.0


@pytest.fixture(scope="module")
def decoder(dev):
    from diffusionkit_amd.engine import TinyDecoderEngine
    w = synth_tae_weights()
    return TinyDecoderEngine(pack_tae(w, dev)), {k: v.float() for k, v in w.items()}


@pytest.mark.parametrize("case", range(len(T.LATENTS)), ids=[str(s) for s in T.LATENTS])
def test_whole_decoder(dev, decoder, case):
    eng, w = decoder
    lat_shape = B, h, ww = T.LATENTS[case]
    lat = T.latent(case)
    img, u8 = eng.decode(lat.to(dev))
    exact, _ = T.decode(lat, w, False)
    p = psnr(exact, img)
    print(f"decoder {lat_shape}: PSNR against the exact float64 reference {p:.1f} dB (gate {T.PSNR_MIN})")
    assert img.shape == (B, 8 * h, 8 * ww, 3) and u8.dtype == torch.uint8 and p >= T.PSNR_MIN
    for i in range(B if B > 1 else 0):  # image i of a batch has the bits of its single decode
        es.assert_identical({"single": eng.decode(lat[i:i + 1].to(dev)), "batch": (img[i:i + 1], u8[i:i + 1])}, f"decoder {lat_shape} image {i}")
    ops.tune("tae_block", 1)  # every Block as its one fused launch instead of the chain the engine takes by measurement: the same bits
    try:
        es.assert_identical({"chains": (img, u8), "fused blocks": eng.decode(lat.to(dev))}, f"decoder {lat_shape}")
    finally:
        ops.tune("tae_block", -1)
    # a second decode on the same engine with an exact-size workspace full of NaN: the same bits, nothing written outside
    nbytes = eng.lib.dk_tae_workspace_bytes(B, h, ww)
    ws = es.GuardedWorkspace(nbytes, dev)
    ws.fill(es.FILL_NAN)
    keep = eng._ws
    es.lend(eng, ws, nbytes)
    again = eng.decode(lat.to(dev))
    torch.cuda.synchronize()
    ws.check(nbytes, f"decoder {lat_shape}", es.FILL_NAN)
    eng._ws = keep
    es.assert_identical({"first": (img, u8), "nan workspace": again}, f"decoder {lat_shape}")
