"""attention5.hip's second generated body -- the tile loop WITHOUT the running row maximum, for launches whose caller bounds |scale q.k|
(AttnParams::score_bound; the engine: from the QKNorm weights) -- on the CPU: the committed include file against the generator, the instruction
list in the emulator at the edges of the admitted range, the route through dk_attention_plan, and the host code of the bound as a stand-alone
program under the host sanitizers."""
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch

from diffusionkit_amd import _lib, ops
from tests import _fused_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusionkit_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.fixture(scope="module")
def nt_program():
    import gen_attn5 as gen
    assert gen.ABL == 0 and not gen.OPT
    return gen.program(track=False)


def test_untracked_include_is_the_generators(nt_program):
    """attention5_asm_nt.inc is what gen_attn5.program(track=False) writes; its first asm statement (the DMA pieces of K(0)) is the tracked body's
    attention5_dma.inc, which both kernels include"""
    import gen_attn5 as gen
    P = nt_program
    k = [i for i, x in enumerate(P) if x.op == "split"][0]
    for part, name in ((P[:k], "attention5_dma.inc"), (P[k + 1:], "attention5_asm_nt.inc")):
        text = "\n".join('    "' + ins.text + '\\n"' for ins in part) + "\n"
        committed = open(os.path.join(CSRC, name)).read()
        assert committed.split("\n", 2)[2] == text, f"{name} is stale: run python scripts/gen_attn5.py"
    assert "v232" not in "".join(i.text or "" for i in P) and "s[56:57]" not in "".join(i.text or "" for i in P)  # no pend, no pending-rows mask
    assert gen.CLOBBERS and os.path.exists(os.path.join(CSRC, "attention5_clobbers.inc"))  # (shared: a superset of what this body writes)


def test_untracked_program_has_no_maximum_behind_the_prologue(nt_program):
    """no v_max3_f32 behind the prologue (the loop label), no rescale block anywhere; the prologue's one offset per row is there"""
    P = nt_program
    loop = [i for i, x in enumerate(P) if x.op == "label" and x.name == "LOOP"][0]
    assert not [x.text for x in P[loop:] if "v_max3_f32" in (x.text or "") or "v_max_f32" in (x.text or "")]
    assert not [x.name for x in P if x.op == "label" and "RESC" in x.name]
    assert not [x for x in P if x.op in ("s_cmp_lg64", "s_or_vcc", "v_cndmask", "v_cmp_lt_s")]
    assert sum(1 for x in P[:loop] if "v_max3_f32" in (x.text or "")) == 26  # 8 chains x 3 + one per query block
    mc_writes = [x.text for x in P if x.op != "label" and any((x.text or "").startswith(f"{op} v{r},") for r in (224, 225) for op in ("v_mul_f32", "v_mov_b32"))]
    assert sorted(mc_writes) == ["v_mov_b32 v224, 0xf149f2ca", "v_mov_b32 v225, 0xf149f2ca", "v_mul_f32 v224, s51, v234", "v_mul_f32 v225, s51, v236"]
    assert sum(1 for x in P if x.op == "mfma32") == sum(1 for x in __import__("gen_attn5").program() if x.op == "mfma32")


@pytest.mark.parametrize("kind", ["random", "spike", "first"])
def test_untracked_body_passes_the_emulator(nt_program, kind):
    """12 key tiles (one pass of the four-tile loop + the eight peeled tiles), DMA pieces and LDS reads completing as late as the waits allow and at
    issue, against the fp64 softmax.  random: plain scores.  spike: every key at the bottom of the admitted range (first-tile maximum near -B) but
    one in the middle of the sequence and one in the last tile near +B, with 2 B log2(e) = 64.  first: the row's maximum in tile 0 and everything
    later at the bottom of the range (attn5_emu.bounded_inputs asserts that the scores do reach, and stay inside, the range)."""
    import attn5_emu as emu
    assert abs(2 * emu.B_MAX * math.log2(math.e) - 64.0) < 1e-9
    edit = None if kind == "random" else emu.bounded_inputs(kind, 12)
    for late in (True, False):
        assert emu.run(nt_program, 12, late, int(late), seed=12, edit=edit), (kind, late)


def test_emulator_notices_an_offset_that_is_not_the_first_tiles(nt_program):
    """the emulator itself: with the one write of the offset taken out (mc stays -1e30) the exponentials overflow and the run comes out wrong"""
    import attn5_emu as emu
    import gen_attn5 as gen
    P = [x for x in gen.program(track=False) if not (x.op == "v_mul_s" and x.dst in gen.MC)]
    assert len(P) == len(nt_program) - 2
    assert not emu.run(P, 12, True, 0, seed=12)


# ---- route ------------------------------------------------------------------------------------------------------------------------------
def plan(score_bound=0.0, track=-1, dtype=None, norm=True, rope=True, **shape):
    lib = _lib.load()
    c = dict(B=1, H=24, S=4352, D=128, split=256, norm=norm, rope=rope)
    c.update(shape)
    d = fc.attn_plan_desc(c)
    d["score_bound"] = score_bound
    try:
        assert lib.dk_tune_set(b"attn_track", track) == 0
        return ops.attention_plan(dtype=dtype or ops.BF, workspace_bytes=lib.dk_attention_workspace_bytes(), **d)
    finally:
        lib.dk_tune_set(b"attn_track", -1)


def test_route_takes_the_untracked_body_only_under_an_admitted_bound():
    """FLUX 1024^2 (S = 4352, 24 heads of 128) double- (two norm weights, split at the text rows) and single-block launches (one weight) with the
    synthetic weights' bound B = 13: the untracked body; and nothing else about the route moves.  No bound, a bound past 32 / log2(e) = 22.18, the knob,
    a plain Q load, D = 64 and fp16: what they got before."""
    base = plan()
    assert (base.kernel, base.qfuse, base.untracked) == (10, 1, 0)
    for split in (256, 0):  # double block / single block
        p = plan(13.0, split=split)
        assert p.untracked == 1
        assert [getattr(p, f) for f, _ in p._fields_ if f != "untracked"] == [getattr(base, f) for f, _ in base._fields_ if f != "untracked"]
    assert plan(13.0, B=4).untracked == 1 and plan(13.0, B=4).split == 2  # the key-split jobs take it too
    assert plan(22.18).untracked == 1 and plan(22.19).untracked == 0  # 2 B log2(e) <= 64
    assert plan(23.0).untracked == 0 and plan(0.0).untracked == 0 and plan(float("nan")).untracked == 0
    assert plan(13.0, track=1).untracked == 0 and plan(13.0, track=0).untracked == 1
    assert plan(13.0, norm=False, rope=False).untracked == 0 and plan(13.0, norm=False, rope=False).kernel == 10  # plain Q load: the tracked body
    assert plan(13.0, norm=False, rope=True).untracked == 1  # (a RoPE table alone is a fused query load)
    p = plan(13.0, D=64, H=24)
    assert (p.kernel, p.untracked) == (4, 0)
    p = plan(13.0, D=64, H=24, dtype=torch.float16)
    assert (p.kernel, p.untracked) == (4, 0)
    p = plan(13.0, S=4352 + 64)  # not a multiple of 256: the phase-alternating kernel
    assert (p.kernel, p.untracked) == (9, 0)
    with pytest.raises(Exception, match="score_bound"):
        plan(-1.0)
    assert _lib.load().dk_abi_version() == 5


# ---- the host code of the bound ----------------------------------------------------------------------------------------------------------
def test_score_bound_host_code_under_the_host_sanitizers(tmp_path):
    """scripts/score_bound_check.cpp: dk_score_bound.h (the per-block maxima of the norm weights, the formula, the "unknown" answers, and what the
    bound promises on QK-normed, rotated rows) as a program of its own with -fsanitize=address,undefined, run directly"""
    # (clang links the sanitizer runtimes statically: the program runs as it is, whatever else the process environment loads)
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("needs clang++ (the ROCm LLVM tools)")
    exe = str(tmp_path / "score_bound_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "scripts", "score_bound_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
