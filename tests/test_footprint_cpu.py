"""The NaN-footprint instrument (tests/_footprint.py) proved on the CPU.

1. The comparator rejects each fabricated defect (an extra NaN, a footprint element left finite, one flipped low bit outside the footprint, a NaN in
   the clean run), and ``guarded`` notices a written margin.
2. For every case family of tests/test_gpu_op_footprints.py, at that test's own shape: the reference the GPU test takes its expectation from
   (``isnan(reference(poisoned))``) has exactly the HAND-WRITTEN dependency footprint, and is bit-equal to its own clean run outside it.  The
   reference alone therefore meets every condition the GPU tests state.
3. Where the oracle does not propagate NaN faithfully the expectation is hand-written in tests/_footprint.py, and the reason is pinned here: the
   patchify Linear (0 * NaN), the MX-fp8 quantiser's block maximum, the clip / uint8 tail of the image.
"""
import pytest
import torch

from oracle import fp8 as o8
from tests import _footprint as fp
from tests import _fp8 as f8
from tests import _fused_cases as fc

BF, F16 = torch.bfloat16, torch.float16


# ---- 1. the instrument ---------------------------------------------------------------------------------------------------------------
def _fabricated(dtype):
    clean = torch.randn(6, 8, generator=torch.Generator().manual_seed(1)).to(dtype)
    expect = torch.zeros(6, 8, dtype=torch.bool)
    expect[2] = True
    good = clean.clone()
    good[2] = fp.NAN
    return clean, good, expect


@pytest.mark.parametrize("dtype", [BF, F16, torch.float32])
def test_comparator_accepts_the_exact_footprint_and_rejects_each_defect(dtype):
    clean, good, expect = _fabricated(dtype)
    fp.assert_footprint(clean, good, expect, "exact")
    extra = good.clone()
    extra[4, 1] = fp.NAN
    with pytest.raises(AssertionError, match=r"1 NaN outputs outside the footprint.*\(4, 1\)"):
        fp.assert_footprint(clean, extra, expect, "extra NaN")
    missing = good.clone()
    missing[2, 5] = 1.0
    with pytest.raises(AssertionError, match=r"1 of 8 footprint elements stayed finite.*\(2, 5\)"):
        fp.assert_footprint(clean, missing, expect, "footprint element left finite")
    flipped = good.clone()
    b = fp.bits(flipped).clone()
    b[5, 7] ^= 1
    flipped = b.view(dtype)
    assert float((flipped[5, 7].double() - clean[5, 7].double()).abs()) < 1e-2  # (one unit in the last place: far below any rel_l2 gate)
    with pytest.raises(AssertionError, match=r"1 outputs outside the footprint differ in their bits.*\(5, 7\)"):
        fp.assert_footprint(clean, flipped, expect, "flipped low bit")
    dirty = clean.clone()
    dirty[0, 0] = fp.NAN
    with pytest.raises(AssertionError, match=r"clean run holds 1 non-finite"):
        fp.assert_footprint(dirty, good, expect, "NaN in clean")


def test_comparator_bytes_and_soft_region():
    clean = torch.randint(0, 0x7E, (4, 32), generator=torch.Generator().manual_seed(2)).to(torch.uint8)
    expect = torch.zeros(4, 32, dtype=torch.bool)
    expect[1, :3] = True
    got = clean.clone()
    got[1, 0], got[1, 1], got[1, 2] = 0x7F, 0xFF, 0x7F  # both e4m3 NaN bytes
    fp.assert_footprint(clean, got, expect, "bytes")
    got[3, 3] ^= 1
    with pytest.raises(AssertionError, match="differ in their bits"):
        fp.assert_footprint(clean, got, expect, "bytes, flipped bit")
    # soft: exempt from bit equality, but finite and within the stated gate of a reference
    c, g, e = _fabricated(torch.float32)
    soft = torch.zeros_like(e)
    soft[3] = True
    g[3] += 1e-4
    with pytest.raises(AssertionError, match="differ in their bits"):
        fp.assert_footprint(c, g, e, "no soft region")
    fp.assert_footprint(c, g, e, "soft", soft=soft, soft_ref=c, soft_rel_l2=6e-3, soft_max_abs=0.03)
    g[3, 0] += 1.0
    with pytest.raises(AssertionError, match="soft region"):
        fp.assert_footprint(c, g, e, "soft, out of the gate", soft=soft, soft_ref=c, soft_rel_l2=6e-3, soft_max_abs=0.03)
    g[3, 0] = float("inf")
    with pytest.raises(AssertionError, match="non-finite output in the soft region"):
        fp.assert_footprint(c, g, e, "soft, Inf", soft=soft, soft_ref=c, soft_rel_l2=6e-3, soft_max_abs=0.03)


@pytest.mark.parametrize("dtype,fill", [(BF, fp.NAN), (F16, fp.SENTINEL), (torch.float32, fp.NAN), (torch.uint8, 0xAB)])
def test_guarded_view_and_margins(dtype, fill):
    t = (torch.arange(5 * 3 * 16).reshape(5, 3, 16) % 100).to(dtype)
    v, guard = fp.guarded(t, 2, fill)
    assert v.shape == t.shape and v.stride() == t.stride() and v.dtype == t.dtype and torch.equal(v, t)
    assert v.data_ptr() % 128 == guard.whole.data_ptr() % 128
    assert guard.intact()
    v.fill_(1)  # writing the view itself leaves the margins alone
    guard.check("view written")
    guard.whole[guard.hi] = 1  # first element behind the view
    assert not guard.intact()
    with pytest.raises(AssertionError, match="1 margin elements"):
        guard.check("margin written")
    v2, g2 = fp.guarded(t[:, :, :8], 1, fill)  # a strided view keeps its strides
    assert v2.stride() == t[:, :, :8].stride() and torch.equal(v2, t[:, :, :8]) and g2.intact()
    g2.whole[g2.lo - 1] = 1  # last element in front of it
    assert g2.written() == 1


# ---- 2. the references have the hand-written footprints -------------------------------------------------------------------------------------
def check_family(ops, ref, cases, what):
    clean = ref(ops)
    for case in cases:
        got = ref(fp.poisoned(ops, case))
        for key in (case.hand if isinstance(case.hand, dict) else [None]):
            c, g, h = (clean, got, case.hand) if key is None else (clean[key], got[key], case.hand[key])
            fp.assert_footprint(c, g, h, f"{what}: {case.label}" + (f" [{key}]" if key else ""))
        if case.soft is not None:  # the cap of the Q rule: at most one query block x one head, and never inside the footprint
            assert not bool((case.soft & case.hand).any())


@pytest.mark.parametrize("epi", ["bias", "gate_res"])
@pytest.mark.parametrize("B,S_t,S_i", fp.GEMM_JOINT_SHAPES)
@pytest.mark.parametrize("dtype", [BF, F16])
def test_gemm_joint_reference(B, S_t, S_i, epi, dtype):
    check_family(*fp.gemm_joint_family(B, S_t, S_i, epi, dtype), f"gemm joint {(B, S_t, S_i)} {epi}")


def test_gemm_ksplit_reference():
    check_family(*fp.gemm_ksplit_family(BF), "gemm K split")


def test_fused_tail_references():
    chosen = fp.chosen_fused_cases()
    call, ops, ref, rows, cases = fp.split_family(chosen["split"])
    check_family(ops, ref, cases, f"split {chosen['split']['id']}")
    call, ops, ref, cases = fp.pair_family(chosen["pair"])
    check_family(ops, ref, cases, f"pair {chosen['pair']['id']}")
    call, ops, ref, rows, cases = fp.knorm_family(chosen["knorm"])
    check_family(ops, ref, cases, f"knorm {chosen['knorm']['id']}")
    print({k: v["id"] for k, v in chosen.items()})


ATTN_SHAPES = [(2, 2, 100, 64, 128), (2, 2, 129, 128, 128), (1, 2, 250, 128, 256), (2, 2, 768, 128, 256), (1, 2, 3072, 128, 256)]


@pytest.mark.parametrize("B,H,S,D,QB", ATTN_SHAPES)
def test_attention_reference(B, H, S, D, QB):
    ops, ref, cases = fp.attention_family(B, H, S, D, QB, BF)
    check_family(ops, ref, cases, f"attention {(B, H, S, D)}")
    for case in cases:
        if case.soft is not None:
            assert int(case.soft.sum()) <= QB * D


def test_attention_d512_and_bias_references():
    check_family(*fp.attention_d512_family(2, 100, BF), "attention d512")
    for B, H, S, D, per_head in ((1, 4, 150, 64, True), (2, 2, 77, 64, False)):
        ops, ref, scale, cases = fp.attention_bias_family(B, H, S, D, per_head)
        check_family(ops, ref, cases, f"attention bias {(B, H, S, D)}")


def test_attention_q_load_reference():
    c = fp.chosen_fused_cases()["attn_q"]
    ops, tab, ref = fp.attention_q_family(c)
    check_family(ops, ref, [fp.q_head_case(c["B"], c["H"], c["S"], c["D"], 128)], f"attention q load {c['id']}")


@pytest.mark.parametrize("dtype", [BF, F16])
def test_row_kernel_references(dtype):
    for h in (1536, 2432):
        check_family(*fp.ln_modulate_family(2, 77, h, dtype), f"ln_modulate h={h}")
    for D in (128, 64):
        check_family(*fp.qk_norm_rope_family(D, dtype), f"qk_norm_rope D={D}")
    check_family(*fp.groupnorm_family(dtype), "groupnorm")
    check_family(*fp.groupnorm_family(dtype, table=True), "groupnorm table")
    check_family(*fp.softmax_family(dtype), "softmax")
    check_family(*fp.transpose_family(dtype), "transpose")


def test_groupnorm_table_reference_is_the_norm():
    """the table restatement (scale | shift) applied to x IS the oracle's GroupNorm"""
    ops, _, _ = fp.groupnorm_family(BF)
    B, H, W, C, G = fp.GN_SHAPE
    tab = fp.ref_groupnorm_table(ops["x"], ops["gamma"], ops["beta"], G)
    y = ops["x"] * tab[:, 0][:, None, None] + tab[:, 1][:, None, None]
    assert torch.allclose(y, fp.ref_groupnorm(ops["x"], ops["gamma"], ops["beta"], G), rtol=1e-4, atol=1e-5)


CONV_FORMS = [(2, 16, 16, 64, 128, "plain", False, 0), (2, 16, 16, 64, 128, "s2", False, 0), (2, 16, 16, 64, 128, "up", False, 0),
              (2, 16, 16, 64, 128, "plain", True, 0), (2, 16, 16, 64, 128, "plain", False, 64),
              (2, 32, 48, 128, 256, "plain", True, 0), (2, 32, 48, 128, 128, "plain", False, 0), (2, 16, 24, 128, 256, "up", False, 0)]


@pytest.mark.parametrize("B,H,W,C,O,form,res,C2", CONV_FORMS)
def test_conv_reference(B, H, W, C, O, form, res, C2):
    ops, ref, cases = fp.conv_family(B, H, W, C, O, form, BF, res=res, C2=C2)
    check_family(ops, ref, cases, f"conv {form} {(B, H, W, C, O)}")
    # with a GroupNorm table built from the CLEAN input in front (the fused norm -> silu -> conv): the same local footprints
    gamma, beta = fp.rounder(BF)(C, seed=81, scale=0.1, shift=1.0), fp.rounder(BF)(C, seed=82, scale=0.1)
    ops, ref, cases = fp.conv_family(B, H, W, C, O, form, BF, res=res, C2=C2, act=fp.gn_act(ops["x"], gamma, beta, 32))
    check_family(ops, ref, cases, f"norm -> silu -> conv {form} {(B, H, W, C, O)}")


def test_tile_mask_geometry():
    m = torch.zeros(2, 32, 48, dtype=torch.bool)
    m[0, 15, 16], m[1, 31, 47] = True, True
    t = fp.tile_mask(m)
    assert t.shape == (2, 6) and t[0].tolist() == [False, True, False, False, False, False] and t[1].tolist() == [False] * 5 + [True]


@pytest.mark.parametrize("flux", [True, False])
def test_patchify_reference(flux):
    ops, ref, _, cases = fp.patchify_family(flux)
    check_family(ops, ref, cases, f"patchify flux={flux}")
    # the gather restatement against the oracle's own patchify / unpatchify on finite data
    from diffusionkit_amd.config import tiny_flux, tiny_sd3
    from oracle.mmdit import OracleMMDiT, Prec
    n_img, Hl, Wl, C = ops["x"].shape
    F = ops["out"].shape[-1]
    orc = OracleMMDiT(tiny_flux() if flux else tiny_sd3(),
                      {"x_embedder.proj.weight": torch.eye(F).reshape(F, *((1, 1, F) if flux else (2, 2, C))), "x_embedder.proj.bias": torch.zeros(F)}, Prec())
    got = ref(ops)
    assert torch.equal(got["tok0"][:n_img], orc._patch_embed(ops["x"]))
    u = orc._unpatch(ops["out"], Hl, Wl)
    den, den_neg = ops["x"] - u[:n_img] * 0.75, ops["x"] - u[n_img:] * 0.75
    den = den_neg + 5.0 * (den - den_neg)
    assert torch.equal(got["x"], ops["x"] + (ops["x"] - den) / 0.75 * (0.5 - 0.75))
    # ... and why it is hand-written: the oracle's identity Linear smears one NaN over its whole token
    x = ops["x"].clone()
    x[1, 5, 7, 9] = fp.NAN
    assert int(torch.isnan(orc._patch_embed(x)).sum()) == F


# ---- 3. where the oracle does not propagate NaN -----------------------------------------------------------------------------------------------
def test_mx8_quantiser_expectation_is_hand_written():
    """oracle.fp8.mx8_encode of a block with one NaN: the NaN's own byte is a NaN byte, but the block scale comes out as 1 (int32 overflow of the
    exponent arithmetic, then the clamp) and the block's other bytes saturate -- not a dependency statement.  fp.assert_mx8_quantiser_footprint states
    what holds for any treatment of the block maximum; it accepts the oracle's result and the maxNum result, and rejects a leak."""
    x = fp.rounder(BF)(8, 128, seed=3)
    r, c = 5, 70
    q0, e0 = o8.mx8_encode(x)
    xp = x.clone()
    xp[r, c] = fp.NAN
    q1, e1 = o8.mx8_encode(xp)
    assert bool(fp.nan_mask(q1)[r, c]) and int(fp.nan_mask(q1).sum()) == 1
    assert int(e1[r, c // 32]) == 1 and int(e0[r, c // 32]) != 1
    fp.assert_mx8_quantiser_footprint(q0, e0, q1, e1, r, c, "oracle")
    q2 = q0.clone()  # maxNum: the maximum of the other 31 elements, every other byte as before
    q2[r, c] = 0x7F
    fp.assert_mx8_quantiser_footprint(q0, e0, q2, e0, r, c, "maxNum")
    q3 = q2.clone()
    q3[r, c + 32] = 0x7F
    with pytest.raises(AssertionError, match="outside the block"):
        fp.assert_mx8_quantiser_footprint(q0, e0, q3, e0, r, c, "leak into the next block")
    e3 = e0.clone()
    e3[r + 1, c // 32] += 1
    with pytest.raises(AssertionError, match="scales of other blocks"):
        fp.assert_mx8_quantiser_footprint(q0, e0, q2, e3, r, c, "another block's scale")
    with pytest.raises(AssertionError, match="not a NaN byte"):
        fp.assert_mx8_quantiser_footprint(q0, e0, q0, e0, r, c, "poison not read")


def test_fp8_gemm_reference_rows_are_independent():
    """decode(a8, scales) @ w^T: a NaN byte (0x7F) or a NaN scale (E8M0 0xFF) of row m reaches exactly output row m"""
    x = fp.rounder(BF)(16, 128, seed=4)
    w = fp.rounder(BF)(32, 128, seed=5, scale=0.05)
    q, e = o8.mx8_encode(x)
    clean = f8.mx8_decode(q, e) @ w.t()
    hand = torch.zeros(16, 32, dtype=torch.bool)
    hand[9] = True
    qp = q.clone()
    qp[9, 100] = 0x7F
    fp.assert_footprint(clean, f8.mx8_decode(qp, e) @ w.t(), hand, "one activation byte")
    ep = e.clone()
    ep[9, 1] = 0xFF
    assert not bool(torch.isfinite(f8.mx8_decode(q, ep)[9, 32:64]).any())  # (the test-side decoder reads 0xFF as 2^128: Inf, not finite either)


def test_clip_and_uint8_tail_of_the_image():
    """the image tail: clip(raw / 2 + 0.5, 0, 1) keeps a NaN (torch.clip propagates it), the uint8 conversion of a NaN is undefined -- so the GPU test
    asserts the footprint on ``raw`` only and "outside the footprint bit-identical" on the clipped image and the uint8 image"""
    raw = torch.tensor([0.3, fp.NAN, -5.0, 5.0])
    img = torch.clip(raw / 2 + 0.5, 0, 1)
    assert torch.equal(torch.isnan(img), torch.tensor([False, True, False, False]))
    assert float(img[2]) == 0.0 and float(img[3]) == 1.0
