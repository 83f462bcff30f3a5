"""The guarded-workspace instrument (tests/_engine_state.py) proved on the CPU: the 0xFF fill is a NaN wherever an engine could read it, a
one-byte write into either margin is found and located, the interior keeps the alignment the engines ask for, and the output comparator
rejects what it must."""
import pytest
import torch

from tests import _engine_state as es
from tests import _footprint as fp
from tests import _fp8 as f8

CPU = torch.device("cpu")


@pytest.mark.parametrize("dtype", es.NAN_DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_ff_bytes_are_nan_in_every_element_type_of_the_workspaces(dtype):
    raw = torch.full((64,), es.FILL_NAN, dtype=torch.uint8)
    v = raw.view(dtype)
    assert v.numel() == 64 // v.element_size()
    assert bool(torch.isnan(v.float()).all())
    assert bool(fp.nan_mask(raw).all())  # (the e4m3 NaN rule tests/_footprint.py applies to uint8 buffers)
    assert not bool(torch.isnan(torch.zeros(64, dtype=torch.uint8).view(dtype).float()).any())  # and the 0x00 fill is 0.0 in each of them


def test_ff_is_the_e8m0_nan_code_of_the_scale_arrays():
    """tests/_fp8.py decodes a scale byte e as 2^(e - 127): 0xFF (the OCP MX NaN code) leaves fp32's range, so a block under that scale decodes
    to no finite value whatever its e4m3 bytes are -- zero bytes give inf * 0 = NaN, 0xFF bytes NaN, anything else +-inf"""
    M, K = 4, 64
    e = torch.full((M, K // 32), es.FILL_NAN, dtype=torch.uint8)
    for q in (torch.zeros(M, K, dtype=torch.uint8), torch.full((M, K), es.FILL_NAN, dtype=torch.uint8),
              torch.arange(M * K, dtype=torch.int32).remainder(0x7F).to(torch.uint8).reshape(M, K)):
        assert not bool(torch.isfinite(f8.mx8_decode(q, e)).any())
    assert bool(torch.isnan(f8.mx8_decode(torch.full((M, K), es.FILL_NAN, dtype=torch.uint8), e)).all())
    # one poisoned scale touches its own 32 columns of its own row only
    e = torch.full((M, K // 32), 127, dtype=torch.uint8)
    e[2, 1] = es.FILL_NAN
    bad = ~torch.isfinite(f8.mx8_decode(torch.full((M, K), 0x38, dtype=torch.uint8), e))
    want = torch.zeros(M, K, dtype=torch.bool)
    want[2, 32:64] = True
    assert torch.equal(bad, want)
    # and the byte survives the side-array layout the fp8 GEMM reads (a whole-buffer 0xFF fill is 0xFF at every scale position)
    arr = torch.full_like(f8.scales_to_array(e, rows=128), es.FILL_NAN)
    assert bool((f8.array_to_scales(arr, M, K, rows=128) == es.FILL_NAN).all())


@pytest.mark.parametrize("fill", [es.FILL_ZERO, es.FILL_NAN])
def test_a_one_byte_write_into_either_margin_is_found(fill):
    nbytes = 4096 + 256
    ws = es.GuardedWorkspace(nbytes, CPU)
    ws.fill(fill)
    ws.arm(nbytes)
    ws.interior(nbytes).fill_(0x5A)  # the engine may write every byte it declared
    ws.check(nbytes, "interior only", fill=fill)
    assert ws.first_written(nbytes) is None
    for pos, off in ((ws.margin - 1, -1), (0, -ws.margin), (ws.margin + nbytes, nbytes), (ws.whole.numel() - 1, nbytes + ws.margin - 1)):
        old = int(ws.whole[pos])
        ws.whole[pos] = old ^ 0x01
        assert ws.first_written(nbytes) == off
        with pytest.raises(AssertionError, match=rf"first at offset {off} relative to the workspace"):
            ws.check(nbytes, "one byte", fill=fill)
        ws.whole[pos] = old
        ws.check(nbytes, "restored", fill=fill)


def test_a_stale_buffer_is_guarded_behind_the_smaller_interior():
    """after a run at a larger shape the bytes behind the smaller interior are that run's, not a fill: they are compared with what they were"""
    big, small = 8192, 2048
    ws = es.GuardedWorkspace(big, CPU)
    ws.fill(es.FILL_NAN)
    ws.interior(big).copy_(torch.arange(big, dtype=torch.int32).remainder(251).to(torch.uint8))  # "the previous image's activations"
    ws.arm(small)
    ws.interior(small).zero_()
    ws.check(small, "stale")
    ws.whole[ws.margin + small + 100] ^= 0x80
    with pytest.raises(AssertionError, match=rf"first at offset {small + 100} relative to the workspace \(100 bytes behind its end\)"):
        ws.check(small, "stale")
    with pytest.raises(AssertionError, match="another interior"):
        ws.check(big, "not armed for this size")


def test_a_fill_that_was_not_applied_is_reported():
    ws = es.GuardedWorkspace(1024, CPU)
    ws.fill(es.FILL_ZERO)
    ws.arm(1024)
    with pytest.raises(AssertionError, match="were not filled with 0xff"):
        ws.check(1024, "wrong fill", fill=es.FILL_NAN)


@pytest.mark.parametrize("nbytes", [256, 4096 + 256, 1000003])
def test_the_interior_is_256_byte_aligned_relative_to_the_base(nbytes):
    assert es.MARGIN >= 1 << 20 and es.MARGIN % 256 == 0
    ws = es.GuardedWorkspace(nbytes, CPU)
    v = ws.interior(nbytes)
    assert v.numel() == nbytes and v.dtype == torch.uint8 and v.is_contiguous()
    assert (v.data_ptr() - ws.whole.data_ptr()) == ws.margin and (v.data_ptr() - ws.whole.data_ptr()) % 256 == 0
    assert ws.whole.data_ptr() % 256 == 0 and v.data_ptr() % 256 == 0  # (what dk_mmdit_prepare / dk_vae_decode / dk_vae_encode require)
    assert ws.whole.numel() == nbytes + 2 * ws.margin
    with pytest.raises(AssertionError):
        es.GuardedWorkspace(nbytes, CPU, margin=es.MARGIN + 128)  # not a multiple of 256
    with pytest.raises(AssertionError):
        es.GuardedWorkspace(nbytes, CPU, margin=4096)  # below 1 MiB


def test_lend_hands_over_exactly_the_declared_size():
    class Wrapper:
        _ws = None
    ws, eng = es.GuardedWorkspace(8192, CPU), Wrapper()
    ws.fill(es.FILL_NAN)
    es.lend(eng, ws, 4352)
    assert eng._ws.numel() == 4352 and eng._ws.data_ptr() == ws.whole.data_ptr() + ws.margin
    ws.check(4352, "lent", fill=es.FILL_NAN)


def test_output_comparator():
    a = torch.randn(3, 5, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    u = torch.arange(15, dtype=torch.uint8).reshape(3, 5)
    es.assert_identical({"zero": (a, u), "nan": (a.clone(), u.clone()), "stale": (a.clone(), u.clone())}, "same")
    b = fp.bits(a).clone()
    b[2, 4] ^= 1
    with pytest.raises(AssertionError, match=r"output 0 of the 'stale' run differs from the 'zero' run in 1 of 15 elements, first at \(2, 4\)"):
        es.assert_identical({"zero": (a, u), "nan": (a.clone(), u), "stale": (b.view(torch.bfloat16), u)}, "one ulp")
    z = torch.zeros(4)
    with pytest.raises(AssertionError, match="differs"):
        es.assert_identical({"zero": z, "nan": -z}, "signed zero")  # (torch.equal alone would accept it)
    n = a.clone()
    n[1, 1] = float("nan")
    with pytest.raises(AssertionError, match=r"non-finite values, first at \(1, 1\)"):
        es.assert_identical({"zero": n, "nan": n}, "NaN in both runs")
    u2 = u.clone()
    u2[0, 0] = 9
    with pytest.raises(AssertionError, match="output 1 of the 'nan' run"):
        es.assert_identical({"zero": (a, u), "nan": (a, u2)}, "uint8 image")
