"""The MX-fp6 (E2M3) activation format on the host: weights.quantize_activation_mxfp6 is its definition, the kernels are held to it
(tests/test_gpu_fp6.py).  Here: the OCP code table, exactness, ties, saturation, the scale rule, the non-finite decision and the fragment packing."""
import pytest
import torch

from diffusionkit_amd.weights import (_e2m3_round, dequantize_activation_mxfp6, pack_activation_mxfp6, quantize_activation_mxfp6,
                                      unpack_activation_mxfp6)

# OCP MX v1.0, E2M3: exponent bias 1, subnormals m / 8, normals (1 + m / 8) * 2^(e - 1)
OCP = [m / 8.0 for m in range(8)] + [(1 + m / 8.0) * 2.0 ** (e - 1) for e in (1, 2, 3) for m in range(8)]


def _block(vals):
    x = torch.zeros(1, 32)
    x[0, :len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return x


def test_codes_decode_to_the_ocp_table():
    code = torch.cat([torch.arange(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)])[None]
    got = dequantize_activation_mxfp6(code, torch.full((1, 4), 127, dtype=torch.uint8))[0, :64]
    assert got.tolist() == OCP + [-v for v in OCP] and max(OCP) == 7.5


@pytest.mark.parametrize("shift", [-20, 0, 9])
def test_representable_values_are_exact(shift):
    """every code times a power of two, the block maximum 7.5: quantise - dequantise gives the values back, with the scale 2^shift"""
    x = torch.tensor(OCP + [-v for v in OCP[1:]] + [7.5], dtype=torch.float32).view(2, 32) * 2.0 ** shift
    x[:, 31] = 7.5 * 2.0 ** shift
    code, e8 = quantize_activation_mxfp6(x)
    assert e8.tolist() == [[127 + shift]] * 2 and torch.equal(dequantize_activation_mxfp6(code, e8), x)


def test_ties_go_to_even_and_values_saturate():
    # block maximum 7.5 -> scale 1; halfway points of the three steps (0.125, 0.25, 0.5) land on the even code
    code, e8 = quantize_activation_mxfp6(_block([7.5, 0.0625, 0.1875, 1.9375, 2.125, 2.375, 4.25, 4.75, 7.25, -0.0625, -2.125]))
    assert int(e8[0, 0]) == 127
    got = dequantize_activation_mxfp6(code, e8)[0, :11].tolist()
    assert got == [7.5, 0.0, 0.25, 2.0, 2.0, 2.5, 4.0, 5.0, 7.0, 0.0, -2.0] and int(code[0, 9]) == 0  # (a zero carries no sign)
    # the element rounding saturates: whatever lies above 7.5 after scaling becomes code 31
    assert _e2m3_round(torch.tensor([7.5, 7.74, 7.76, 8.0, 1e6])).tolist() == [31] * 5


@pytest.mark.parametrize("amax,want", [(1.0, 125), (0.99999994, 125), (4.0, 127), (8.0, 128), (7.5, 127), (7.5000005, 128), (2.0 ** -10, 115), (0.0, 1)])
def test_scale_rule(amax, want):
    """the smallest power of two s with amax / s <= 7.5, on the fp32 bit pattern of amax * fp32(1 / 7.5): maxima that are a power of two and just
    below one take the same scale; an all-zero block takes exponent 1, as in the MX-fp8 quantiser"""
    _, e8 = quantize_activation_mxfp6(_block([amax, -amax / 2]))
    assert int(e8[0, 0]) == want
    if amax:  # the smallest such power of two: half of it would not do
        assert 3.75 < amax * 2.0 ** (127 - want) <= 7.5


def test_non_finite_blocks_leave_as_nan_scale():
    x = torch.ones(2, 64)
    x[0, 3], x[1, 40] = float("inf"), float("nan")
    code, e8 = quantize_activation_mxfp6(x)
    assert e8.tolist() == [[255, 125], [125, 255]] and int(code[0, :32].max()) == 0 and int(code[1, 32:].max()) == 0
    d = dequantize_activation_mxfp6(code, e8)
    assert bool(d[0, :32].isnan().all()) and bool((d[0, 32:] == 1).all())


@pytest.mark.parametrize("M,K", [(1, 128), (17, 384)])
def test_fragment_packing_round_trips(M, K):
    code = torch.randint(0, 64, (M, K), generator=torch.Generator().manual_seed(M), dtype=torch.uint8)
    a6 = pack_activation_mxfp6(code)
    assert a6.shape == ((M + 15) // 16 * 16, K // 128 * 96) and torch.equal(unpack_activation_mxfp6(a6, M, K), code)
    # MFMA lane (row 0, q = 1) of K-tile 0: 16 bytes at (16 + 0) * 16, 8 at 1024 + 16 * 8; element e in bits [6 e, 6 e + 6), little-endian
    frag = a6.reshape(-1)[:1536]
    bits = int.from_bytes(bytes(frag[256:272].tolist()) + bytes(frag[1024 + 128:1024 + 136].tolist()), "little")
    assert [(bits >> (6 * e)) & 63 for e in range(32)] == code[0, 32:64].tolist()
    assert int(unpack_activation_mxfp6(a6, a6.shape[0], K)[M:].sum()) == 0  # the rows behind M


def test_interface_refusals_by_name():
    """validate_activation_quant / fp4_config and the CLI flag: what is refused, by name, without a GPU"""
    from dataclasses import replace

    from diffusionkit_amd import cli
    from diffusionkit_amd.config import MMDIT_CKPT, fp4_config, fp8_config, tiny_flux, validate_activation_quant
    cfg = fp4_config(tiny_flux(), "speed", activations="mxfp6")
    assert (cfg.weight_dtype, cfg.activation_quant) == ("mxfp4", "mxfp6") and fp4_config(tiny_flux(), "speed").activation_quant == "mxfp8"
    validate_activation_quant(cfg)
    with pytest.raises(ValueError, match="unknown activation_quant"):
        fp4_config(tiny_flux(), "speed", activations="mxfp4")
    for other in (tiny_flux(), fp8_config(tiny_flux(), "speed")):  # bf16 and e4m3 weights
        with pytest.raises(ValueError, match="needs weight_dtype mxfp4"):
            validate_activation_quant(replace(other, activation_quant="mxfp6"))
    parse = cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args
    with pytest.raises(ValueError, match="--fp4-activations mxfp6 needs --fp4"):
        cli.resolve(parse(["--prompt", "x", "--fp4-activations", "mxfp6"]))
    with pytest.raises(ValueError, match="--fp4-activations mxfp6 needs --fp4"):
        cli.resolve(parse(["--prompt", "x", "--fp8", "speed", "--fp4-activations", "mxfp6"]))
    r = cli.resolve(parse(["--prompt", "x", "--fp4", "speed", "--fp4-activations", "mxfp6"]))
    assert (r["mmdit_config"].weight_dtype, r["mmdit_config"].activation_quant) == ("mxfp4", "mxfp6")
    assert cli.resolve(parse(["--prompt", "x", "--fp4", "speed"]))["mmdit_config"].activation_quant == "mxfp8"


def test_plan_sweeps_the_launch_rules():
    """dk_gemm_fp4a6_plan, host only: the K split of the W4A6 launch is the shared rule on a launch of at most half a round of tiles"""
    from diffusionkit_amd import _lib, ops
    from tests import _mxfp6 as f6
    M, N, K = f6.smallest_split_shape()
    cut, whole = ops.gemm_fp4a6_plan(f6.plan_desc(M, N, K)), ops.gemm_fp4a6_plan(f6.plan_desc(M, N, K, workspace=False))
    assert (cut.kernel, cut.tile_rows, cut.launches, cut.tiles, cut.split_tiles) == (46, 256, 1, N // 256, N // 256)
    assert cut.k_pieces > 1 and cut.workgroups == cut.tiles * cut.k_pieces and 0 < cut.ks < K // 128
    assert (whole.k_pieces, whole.split_tiles, whole.workgroups, whole.ks) == (1, 0, N // 256, K // 128)
    for m, n in ((4096, 9216), (cut.n_cu // 2 * 256 + 1, 256)):  # FLUX's qkv at 1024^2; one tile more than half a round
        p = ops.gemm_fp4a6_plan(f6.plan_desc(m, n, 128 * 128))
        assert p.k_pieces == 1 and p.workgroups == p.tiles == (m + 255) // 256 * (n // 256)
    d2 = f6.plan_desc(128, N, K)
    d2.update(A=0x10000 + 256 * (K // 128 * 96), a_row0=256, a_rows=384)
    pair = ops.gemm_fp4a6_plan(dict(f6.plan_desc(M, N, K), a_rows=384), None, d2)
    assert pair.tiles == 2 * (N // 256) and pair.launches == 1
    with pytest.raises(_lib.DkHipError, match="K is not a multiple of 128"):
        ops.gemm_fp4a6_plan(dict(f6.plan_desc(M, N, K), K=K + 64))
    print(f"smallest cut shape {M} x {N} x {K}: {cut.k_pieces} pieces, finisher {cut.ks} K-tiles")
