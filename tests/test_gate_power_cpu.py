"""The per-element and per-row gates of tests/_gates.py, proved on the host on the shapes, seeds and constructors of the GPU tests: the fp32
restatement of every operator passes its gate at half the bound (the constants are twice its worst), every mutant misses it by >= 2 x, and no
mutant leaves the restatement bit-identical.  Each case prints the restatement's worst ratio and every mutant's (pytest -s).

Findings (DESIGN.md section 4 has the table):
  * attention, "64 rows x (1 + 1/64)": a row error of 1.56e-2 against bounds of 6.3e-3 (D = 512) and 7.8e-3 -- 2.0 x to 2.5 x at every bf16 shape, so it
    separates from the restatement (<= 0.5) by 4 x only just: the weakest fault the row gate sees.  Under the key split's bound (8.4e-3: the partial
    results are rounded once more) it is 1.9 x to 2.0 x; the mutant is not run on the key-split cases and the gate is not narrowed or widened for it.
  * LN-modulate, "last 8 channels not in the mean": on the tests' own rows (3 N(0, 1) + 0.5) it moves the result by 0.42 of the bound, less than the
    rounding of a correct result; it is proved on rows at mean / sigma 16 (h = 2432, both element types), which the GPU files run as well.
  * GroupNorm: statistics that miss one pixel move the output by less than its rounding; they are gated in the (scale | shift) table with the rstd bound
    of tests/_numeric_range.py.  beta missing on the LAST channel alone is 0.95 / 1.5 of the bound at two of the four shapes (that beta is nearly zero
    there); the mutant takes the last 16-byte vector (8 channels), and the output is gated per (image, channel) as well as per (image, group).
  * the whole-tensor gates pass the faults of test_old_gates_table; that is why this file exists."""
import pytest
import torch

from tests import _gates as G
from tests import _numeric_range as NR
from tests._gates import BF
from tests._util import max_abs, rel_l2


def check(name, base_ratio, base, mutants, ratio):
    line = [f"{name}: restatement {base_ratio:.3f}"]
    assert base_ratio <= 0.5, f"{name}: restatement at {base_ratio:.3f} of the bound"
    for mname, fn in mutants.items():
        got = fn()
        assert not torch.equal(got, base), f"{name}: mutant '{mname}' left the result bit-identical"
        r = ratio(got)
        line.append(f"{mname} {r:.1f}")
        assert r >= 2.0, f"{name}: mutant '{mname}' at {r:.2f} of the bound"
    print(" | ".join(line))


@pytest.mark.parametrize("c", G.GEMM_CASES, ids=lambda c: c["name"])
def test_gemm_gate(c):
    r = G.GemmRestatement(c, "steps")
    e_steps = r.unit_error()
    e_torch = float(((G.gemm_f32(r.x, r.w, r.b, "torch").double() - r.pre64).abs() / r.unit).max())
    print(f"{c['name']}: |fp32 - ref| / unit: 32-wide steps {e_steps:.3e}, torch {e_torch:.3e} (C_GEMM {G.C_GEMM:.2e})")
    assert 2.0 * max(e_steps, e_torch) <= G.C_GEMM
    base = r.out()
    check(c["name"], r.ratio(base), base, r.mutants(), r.ratio)


@pytest.mark.parametrize("case", G.CONV_CASES, ids=str)
def test_conv_gate(case):
    dt = BF
    r = G.ConvRestatement(case, dt, "steps")
    e_torch = float(((G.conv_f32(r.x, r.w, r.b, r.mode, "torch").double() - r.pre64).abs() / r.unit).max())
    print(f"conv {case}: |fp32 - ref| / unit: steps {r.unit_error():.3e}, torch {e_torch:.3e}")
    assert 2.0 * max(r.unit_error(), e_torch) <= G.C_GEMM
    base = r.out()
    check(f"conv {case[:7]}", r.ratio(base), base, r.mutants(), r.ratio)


@pytest.mark.parametrize("c", G.ATTN_CASES, ids=lambda c: c["name"])
def test_attention_gate(c):
    r = G.AttnRestatement(c)
    print(f"{c['name']}: worst row of the restatement {G.row_rel(r.base, r.ref):.3e}")
    check(c["name"], r.ratio(r.base), r.base, r.mutants(), r.ratio)


@pytest.mark.parametrize("case", G.D512_CASES, ids=str)
def test_attention_d512_gate(case):
    q, k, v, c = G.d512_operands(case)
    imgs = [q.shape[0] - 1]  # (one image of a pair: the second, as the cost of the fp64 reference is the CPU's)
    r = G.AttnRestatement(c, qkv3=(q[imgs], k[imgs], v[imgs]))
    print(f"{c['name']}: worst row of the restatement {G.row_rel(r.base, r.ref):.3e}")
    check(c["name"], r.ratio(r.base), r.base, r.mutants(), r.ratio)


def test_attention_tile_width_does_not_move_the_constant():
    """one restatement, the tile width a parameter: 32- and 128-key tiles stay inside the same gate at half the bound"""
    c = next(c for c in G.ATTN_CASES if c["name"] == "variants 2x2x653x64")
    for tile in (32, 64, 128):
        r = G.AttnRestatement(c, tile=tile)
        print(f"{c['name']} tile {tile}: worst row {G.row_rel(r.base, r.ref):.3e}")
        assert r.ratio(r.base) <= 0.5


@pytest.mark.parametrize("case", G.LN_CASES, ids=str)
def test_ln_gate(case):
    dt = case[0]
    x, shift, scale = G.ln_operands(case)
    ref = G.ln_ref64(x, shift, scale, dt)
    base = G.ln_f32(x, shift, scale, dt)
    print(f"ln {case}: worst row of the restatement {G.row_rel(base, ref):.3e}")
    check(f"ln {case[:4]}", G.row_ratio(base, ref, G.C_ROW[("ln", dt)], dt), base, G.ln_mutants(case), lambda got: G.row_ratio(got, ref, G.C_ROW[("ln", dt)], dt))


def test_ln_mutants_cover_the_list():
    names = set().union(*(G.ln_mutants(c).keys() for c in G.LN_CASES))
    assert names == {"other image's shift", "last 8 channels not in the mean"}


@pytest.mark.parametrize("case", G.QK_CASES, ids=str)
def test_qk_gate(case):
    dt, D = case[0], case[1]
    qkv, qw, kw, tab = G.qk_operands(case)
    ref = G.qk_ref64(qkv, qw, kw, tab, D)
    base = G.qk_f32(qkv, qw, kw, tab, D, dt)
    print(f"qk {case}: worst row of the restatement {G.row_rel(base, ref):.3e}")
    check(f"qk {case[:4]}", G.row_ratio(base, ref, G.C_ROW[("qk", dt)], dt), base, G.qk_mutants(case), lambda got: G.row_ratio(got, ref, G.C_ROW[("qk", dt)], dt))


@pytest.mark.parametrize("case", G.GN_CASES, ids=str)
def test_gn_gate(case):
    C, Gr, HW, silu = case
    x, gamma, beta = G.gn_operands(case)
    ref = G.gn_apply(x, gamma, beta, Gr, silu, BF, True)
    base = G.gn_apply(x, gamma, beta, Gr, silu, BF, False)
    cpg = C // Gr
    ch = lambda t: t.reshape(2, Gr, -1, cpg).permute(0, 1, 3, 2).reshape(2, C, -1)  # noqa: E731
    print(f"gn {case}: worst (image, group) of the restatement {G.row_rel(base, ref):.3e}, worst (image, channel) {G.row_rel(ch(base), ch(ref)):.3e}")
    check(f"gn {case}", G.gn_ratio(base, ref, cpg), base, G.gn_mutants(case), lambda got: G.gn_ratio(got, ref, cpg))
    # the statistics, gated in the table (tests/_numeric_range.py's rstd bound): a literal fp32 two-pass at half the bound, one pixel missed >= 2 x
    tab = NR.gn_table_f32(x, gamma, beta, Gr)
    r_tab, r_mut = G.gn_stats_ratio(tab, x, gamma, beta, Gr), G.gn_stats_ratio(G.gn_table_mutant(x, gamma, beta, Gr), x, gamma, beta, Gr)
    print(f"gn {case} table: restatement {r_tab:.3f} | statistics miss the last pixel of one group {r_mut:.1f}")
    assert r_tab <= 0.5 and r_mut >= 2.0


def test_old_gates_table():
    """What the whole-tensor gates (rel-L2 < 3e-3 + max_abs < 0.02 max|ref| + 1e-2 for GEMMs; rel-L2 < 6e-3 + max_abs < 0.03 for attention) say about
    the same mutants, on the cases measured when these gates were written: they pass the attention faults and the zeroed GEMM element outright and catch
    the other two GEMM faults by max_abs alone -- which test_gemm_epilogues, test_gemm_segment_mapping_in_place and the float16 tests do not have."""
    rows = []

    def old_attn(ref, got):
        return rel_l2(ref, got), max_abs(ref, got), rel_l2(ref, got) < 6e-3 and max_abs(ref, got) < 0.03

    for name, muts in (("attention 2x4x4685x64", ("last key dropped", "ragged key tile dropped", "64 rows x (1 + 1/64)")),
                       ("attention 1x2x2304x128", ("last key dropped", "64 rows x (1 + 1/64)"))):
        r = G.AttnRestatement(next(c for c in G.ATTN_CASES if c["name"] == name))
        all_m = r.mutants()
        for m in muts:
            got = all_m[m]()
            l2, ma, ok = old_attn(r.ref, got)
            rows.append((name, m, l2, ma, ok, r.ratio(got)))
            assert ok, f"{name} / {m}: the whole-tensor gate was expected to pass this fault"
    for name, muts in (("bias 4352x3072x3072", (("one element zero", True, True), ("k step dropped", True, False))),
                       ("bias 1178x1536x1536", (("bias missing", True, False),))):
        r = G.GemmRestatement(next(c for c in G.GEMM_CASES if c["name"] == name))
        all_m = r.mutants()
        for m, l2_passes, ma_passes in muts:
            got = r.m_one_zero(0.05) if m == "one element zero" else all_m[m]()  # (a small element, |ref| < 0.02 max|ref|: a typical one max_abs sees)
            l2, ma = rel_l2(r.ref, got), max_abs(r.ref, got)
            ok_l2, ok_ma = l2 < 3e-3, ma < 0.02 * float(r.ref.abs().max()) + 1e-2
            rows.append((name, m, l2, ma, ok_l2 and ok_ma, r.ratio(got)))
            assert ok_l2 == l2_passes and ok_ma == ma_passes, f"{name} / {m}: rel_l2 {l2:.2e} max_abs {ma:.3f}"
    print("case | mutant | rel_l2 | max_abs | old gate | new gate (error / bound)")
    for name, m, l2, ma, ok, new in rows:
        print(f"{name} | {m} | {l2:.2e} | {ma:.4f} | {'passes' if ok else 'fails'} | {new:.1f}")
        assert new >= 1.0
