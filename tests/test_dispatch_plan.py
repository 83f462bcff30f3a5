"""CPU-side sweep over the GEMM dispatch rules (round 6, VERDICT r5 item 6 / "dispatch rules are fitted constants"): dk_gemm_plan asks the launchers
themselves what they would launch -- no kernel runs, no GPU is needed; without a device the rules assume the MI355X's 256 compute units -- for the
block Linears of FLUX and SD3 over the resolutions and batch sizes a user can ask for (512 x 512 is what the reference's CLI defaults to,
mlx/scripts/generate_images.py:15-30).  The properties pinned here are the ones whose absence was the 512 x 512 cliff this round found:
a long-K Linear of at most half a round of tiles must be cut along K, the measured 1024 x 1024 choices must stay what the profiles were taken on,
and no launch of a production shape may leave more than two thirds of the chip idle without a K split."""
import ctypes as C

import pytest

from diffusionkit_amd import _lib

FAKE_WS = 0x10000  # (never dereferenced in plan mode: only "non-NULL, 256-byte aligned" matters)


def plan(M, N, K, ws=True, M2=0, lda=None, ldw=0):
    lib = _lib.load()

    def desc(m):
        d = _lib.dk_gemm_desc()
        d.M, d.N, d.K = m, N, K
        d.lda, d.ldc, d.ldr = lda or K, N, N
        d.alpha, d.epilogue, d.ldw = 1.0, 0, ldw
        if ws:
            d.workspace, d.workspace_bytes = FAKE_WS, lib.dk_gemm_workspace_bytes()
        return d
    p = _lib.dk_gemm_plan_t()
    a = desc(M)
    b = desc(M2) if M2 else None
    rc = lib.dk_gemm_plan(C.byref(a), C.byref(b) if b is not None else None, C.byref(p))
    assert rc == 0, lib.dk_last_error()
    return p


def flux_linears(h=3072):
    return {"qkv": (3 * h, h), "o_proj": (h, h), "fc1": (4 * h, h), "fc2": (h, 4 * h), "linear1": (7 * h, h), "linear2": (h, 5 * h)}


def test_plan_runs_without_a_gpu_and_reports_the_mi355x():
    p = plan(4352, 3072, 3072)
    assert p.n_cu == 256 or p.n_cu > 0
    assert p.kernel in (3, 4, 128) and p.launches == 1 and p.tiles > 0


def test_headline_shapes_keep_their_measured_choices():
    """FLUX.1-schnell 1024 x 1024 (M = 4352; double blocks: 4096 image + 256 text rows grouped): the one-wave-per-SIMD kernel on every block Linear, the
    tile heights of profiles/r05_flux_schnell_kernel_stats.md / r06_*: 224-row tiles where they save a round, 256 on linear1 (1428 tiles = 5.6 rounds)"""
    lin = flux_linears()
    p = plan(4352, *lin["linear1"])
    assert (p.kernel, p.tile_rows, p.tiles, p.split_tiles) == (4, 256, 17 * 84, 0)
    p = plan(4352, *lin["linear2"])
    assert (p.kernel, p.tile_rows, p.tiles, p.split_tiles) == (4, 224, 20 * 12, 0)
    for name in ("qkv", "o_proj", "fc1", "fc2"):  # grouped image + text launches of the double blocks
        p = plan(4096, *lin[name], M2=256)
        assert p.kernel == 4 and p.split_tiles == 0, name
        assert p.tile_rows == 224 and p.tiles == 21 * (lin[name][0] // 256), name


@pytest.mark.parametrize("res,batch", [(512, 1), (640, 1), (768, 1), (512, 2)])
def test_small_launches_with_long_reductions_are_cut_along_k(res, batch):
    """below 1024 x 1024 fc2 / linear2 are a fraction of a round of 256 x 256 tiles: every tile is cut along K (gemm256v3.hip's split; the cliff of
    profiles/r06_flux_512_kernel_stats_before.md: 72 workgroups, 229 us), and o_proj (K = 3072) only where four ranges save 36 steps"""
    S_i = (res // 16) ** 2
    lin = flux_linears()
    M = batch * (256 + S_i)
    p = plan(M, *lin["linear2"])
    tiles256 = -(-M // 256) * 12
    if tiles256 * 2 <= 256:
        assert p.kernel == 3 and p.split_tiles == p.tiles and p.k_pieces >= 2, (res, batch, p.kernel, p.tiles, p.split_tiles)
        assert p.workgroups > 128 and p.ks <= lin["linear2"][1] // 64 // 2
        q = plan(batch * S_i, *lin["fc2"], M2=batch * 256)
        assert q.kernel == 3 and q.split_tiles == q.tiles
        # o_proj (K = 3072: 48 steps): cut only where that saves a workgroup at least 32 steps -- four ranges at 512 x 512 (36), not two at 768 x 768 (24)
        o = plan(batch * S_i, *lin["o_proj"], M2=batch * 256)
        S = min(4, 256 // o.tiles)
        assert (o.split_tiles > 0) == (48 - -(-48 // S) >= 32), (res, batch, o.tiles, o.split_tiles)
    # without the workspace nothing can be cut -- and nothing is
    assert plan(M, *lin["linear2"], ws=False).split_tiles == 0


def test_no_production_launch_wastes_the_chip_silently():
    """the sweep the 1024 x 1024-fitted constants never had: FLUX and SD3-medium block Linears over resolutions 384 ... 1536 and batches 1 ... 8.  A launch
    may under-fill the CUs when its reduction is short (K <= 3072: the split's slab round trips cost more than they save), never when it is long."""
    worst = []
    for h, txt, fam in ((3072, 256, "flux"), (1536, 589, "sd3")):
        for res in (384, 512, 640, 768, 896, 1024, 1280, 1536):
            for batch in (1, 2, 4, 8):
                rows = batch * (2 if fam == "sd3" else 1)
                M_img, M_txt = rows * (res // 16) ** 2, rows * txt
                for name, (N, K) in flux_linears(h).items():
                    if fam == "sd3" and name.startswith("linear"):
                        continue
                    single = name.startswith("linear")
                    p = plan(M_img + M_txt, N, K) if single else plan(M_img, N, K, M2=M_txt)
                    assert p.launches >= 1 and p.workgroups >= p.tiles
                    fill = min(1.0, p.workgroups / p.n_cu)
                    if K >= 6144 and p.kernel != 128:
                        worst.append((fill, fam, res, batch, name, p.kernel, p.tiles, p.workgroups))
    worst.sort()
    fill, *what = worst[0]
    assert fill >= 0.55, f"long-K launch fills only {fill:.2f} of the CUs: {what}"


def test_plan_mode_leaves_no_state_behind():
    """two plans of the same shape agree, and a forced kernel choice shows up in the plan (dk_tune_set drives the same code)"""
    lib = _lib.load()
    a, b = plan(1280, 3072, 15360), plan(1280, 3072, 15360)
    assert [getattr(a, f) for f, _ in a._fields_] == [getattr(b, f) for f, _ in b._fields_]
    try:
        assert lib.dk_tune_set(b"gemm_split", 0) == 0
        assert plan(1280, 3072, 15360).split_tiles == 0
    finally:
        lib.dk_tune_set(b"gemm_split", -1)
    assert plan(1280, 3072, 15360).split_tiles > 0


# ---- the engine-only launch forms (dk_gemm_fused_plan): every case of tests/test_gpu_fused_ops.py takes the path it claims -----------------------
from tests import _fused_cases as fc  # noqa: E402


def fused_plan(call):
    from diffusionkit_amd import ops
    lib = _lib.load()
    try:
        for k, v in call.tune.items():
            assert lib.dk_tune_set(k.encode(), v) == 0
        return ops.gemm_fused_plan(*fc.resolve(call, fc.fake_address(call), lib.dk_gemm_workspace_bytes()))
    finally:
        for k in fc.TUNE_KEYS:
            lib.dk_tune_set(k.encode(), -1)


def check_expect(case, p):
    launches, kernel = case["expect"]
    assert p.launches == launches, (case["id"], p.launches, p.kernel)
    if kernel is not None:
        assert p.kernel == kernel, (case["id"], p.kernel)
        if case.get("mf", -1) in (7, 8):
            assert p.tile_rows == 32 * case["mf"], (case["id"], p.tile_rows)
    else:
        assert launches == 2  # an expansion names no single kernel


@pytest.mark.parametrize("case", fc.SPLIT_CASES, ids=lambda c: c["id"])
def test_column_split_cases_take_the_path_they_claim(case):
    check_expect(case, fused_plan(fc.split_call(case)))
    if case["expect"][0] == 1:  # ... and the two launches they are compared with run on the same kernel
        for single in fc.split_single_calls(case):
            p = fused_plan(single)
            assert p.launches == 1 and p.kernel in (3, 4), (case["id"], p.kernel)


@pytest.mark.parametrize("case", fc.PAIR_CASES, ids=lambda c: c["id"])
def test_pair_cases_are_grouped(case):
    p = fused_plan(fc.pair_call(case))
    check_expect(case, p)
    assert (p.split_tiles > 0) == bool(case.get("cut")), (case["id"], p.split_tiles)
    if case.get("cut"):  # the rule the case names: a small extra share of a round, a long reduction
        ta, tb = -(-case["B"] * case["S_i"] // 256) * (case["N"] // 256), -(-case["B"] * case["S_t"] // 256) * (case["N"] // 256)
        assert (ta + tb) % p.n_cu <= p.n_cu // 4 and case["K"] // 64 >= 24
    q = fused_plan(fc.pair_call(case, grouped=False))  # the comparison: two launches of gemm256v3.hip, whole tiles
    assert (q.launches, q.kernel, q.split_tiles) == (2, 3, 0), (case["id"], q.launches, q.kernel)


@pytest.mark.parametrize("case", fc.KNORM_CASES, ids=lambda c: c["id"])
def test_qknorm_cases_take_the_path_they_claim(case):
    check_expect(case, fused_plan(fc.knorm_call(case)))
    if case["expect"][0] == 1:  # the plain projection of the second assertion: one launch of the same kernel
        p = fused_plan(fc.knorm_call(case, fused=False))
        assert (p.launches, p.kernel) == case["expect"], (case["id"], p.kernel)


@pytest.mark.parametrize("case", fc.KNORM_PAIR_CASES, ids=lambda c: c["id"])
def test_qknorm_pair_cases_are_grouped(case):
    check_expect(case, fused_plan(fc.knorm_pair_call(case)))
    q = fused_plan(fc.knorm_pair_call(case, fused=False, grouped=False))
    assert (q.launches, q.kernel) == (2, 3)


def test_ineligible_forms_expand():
    """forms the 256-column kernels cannot fuse must run as the equivalent sequence of launches, never as a fused launch that ignores a field"""
    for what, call, launches in fc.ineligible_calls():
        assert fused_plan(call).launches == launches, what


def test_fused_plan_without_a_side_struct_is_the_plain_plan():
    a = plan(4352, 3072, 3072)
    d = dict(M=4352, N=3072, K=3072, lda=3072, ldc=3072, ldr=3072, alpha=1.0, epilogue=0, workspace=FAKE_WS,
             workspace_bytes=_lib.load().dk_gemm_workspace_bytes())
    from diffusionkit_amd import ops
    b = ops.gemm_fused_plan(d)
    assert [getattr(a, f) for f, _ in a._fields_] == [getattr(b, f) for f, _ in b._fields_]


@pytest.mark.parametrize("case", fc.KNORM_CASES, ids=lambda c: c["id"])
def test_qknorm_cases_reach_the_tail_paths_they_name(case):
    """dk_gemm_plan_t names kernel and tile height, not the tail path of a tile: the `fast` / `cut` arithmetic of the two kernels over the case's row
    tiles (tests/_fused_cases.py: knorm_tail_paths) must give exactly the paths the table lists for it"""
    if case["expect"][0] != 1:
        assert case["id"] not in fc.KNORM_PATHS
        return
    p = fused_plan(fc.knorm_call(case))
    assert fc.knorm_tail_paths(case, p.kernel, p.tile_rows) == fc.KNORM_PATHS[case["id"]], (case["id"], p.kernel, p.tile_rows)


def test_qknorm_table_covers_every_tail_path_of_both_kernels():
    seen = {3: set(), 4: set()}
    for case in fc.KNORM_CASES:
        if case["expect"][0] == 1:
            seen[case["expect"][1]] |= fc.KNORM_PATHS[case["id"]]
    assert seen[3] == {"fast", "wrap", "row"} and seen[4] == {"fast", "wrap", "cut", "row"}


# ---- attention: dk_attention_plan asks dk_attention_route, the function the launchers take their kernel and key split from --------------------------
def attn_plan(desc=None, ws=True, dtype=None, o8_split=0, attn=-1, attn_split=-1, **shape):
    """the plan of a launch under the knobs "attn" / "attn_split" (reset afterwards); ``shape``: B, H, S, D of a dense q | k | v buffer instead of
    ``desc``; ws: a workspace of dk_attention_workspace_bytes(), or none"""
    from diffusionkit_amd import ops
    lib = _lib.load()
    if desc is None:
        desc = fc.attn_plan_desc(shape)
    try:
        assert lib.dk_tune_set(b"attn", attn) == 0 and lib.dk_tune_set(b"attn_split", attn_split) == 0
        return ops.attention_plan(dtype=dtype or ops.BF, workspace_bytes=lib.dk_attention_workspace_bytes() if ws else 0, o8_split=o8_split, **desc)
    finally:
        lib.dk_tune_set(b"attn", -1)
        lib.dk_tune_set(b"attn_split", -1)


def fields(p):
    return [getattr(p, f) for f, _ in p._fields_]


@pytest.mark.parametrize("case", fc.ATTN_Q_CASES + fc.ATTN_O8_CASES, ids=lambda c: c["id"])
def test_attention_cases_run_the_kernel_they_name(case):
    """dk_attention_route turns mode 10 into 9 and 9 into the lean kernel without a word when a shape is not eligible, and attention5.hip's key split
    needs 12 key tiles per range: what the route answers for the case's knobs against what the case's name claims"""
    p = attn_plan(fc.attn_plan_desc(case), attn=case["mode"], attn_split=case.get("attn_split", -1))
    assert (fc.ATTN_KERNEL_NAMES[p.kernel], p.split) == fc.attn_claim(case), (case["id"], p.kernel, p.split)
    assert p.merge == (p.split > 1) and p.jobs == (p.blocks - p.whole) * p.split * p.merge
    if "in_kernel" in case:  # only the D = 128 kernels of modes 9 / 10 write the MX-fp8 copy themselves: a quantiser pass follows the others
        assert case["in_kernel"] == (p.kernel in (9, 10) and case["D"] == 128)
        assert p.quantize == (0 if case["in_kernel"] else 1) and p.launches == 1 + p.quantize
        assert (case["B"] * case["S"]) % 128 == 0
    else:
        assert p.qfuse == 1 and p.quantize == 0 and p.launches == 1 + p.merge


FLUX = dict(H=24, D=128)


def test_attention_headline_shapes_keep_their_measured_choices():
    """the automatic choices the profiles were taken on (256 CUs, the workspace of dk_attention_workspace_bytes()); the expected values are worked out
    by hand from the rules: FLUX 1024 x 1024 is S = 4352 = 17 blocks per head"""
    assert attn_plan(B=1, S=4352, **FLUX).n_cu == 256
    p = attn_plan(B=1, S=4352, **FLUX)  # 408 blocks: one round + 152, which no number of ranges fits into one sub-round
    assert (p.kernel, p.blocks, p.whole, p.split, p.jobs, p.merge, p.launches) == (10, 408, 408, 1, 0, 0, 1)
    p = attn_plan(B=2, S=4352, **FLUX)  # 816 = 3 rounds + 48: four ranges fill 192 CUs
    assert (p.kernel, p.blocks - p.whole, p.split, p.jobs, p.merge, p.launches) == (10, 48, 4, 192, 1, 2)
    p = attn_plan(B=4, S=4352, **FLUX)  # 1632 = 6 rounds + 96
    assert (p.kernel, p.blocks - p.whole, p.split, p.jobs, p.whole) == (10, 96, 2, 192, 1536)
    p = attn_plan(B=1, S=4608, **FLUX)  # FLUX-dev, S_t = 512: 432 = one round + 176
    assert (p.kernel, p.split, p.whole) == (10, 1, 432)
    p = attn_plan(B=1, S=2560, **FLUX)  # 768 x 768: 240 blocks in one round; two or three ranges overflow it, four would hold 8 tiles each
    assert (p.kernel, p.blocks, p.split) == (10, 240, 1)
    p = attn_plan(B=1, S=1280, **FLUX)  # 512 x 512: 120 blocks are less than three quarters of a round
    assert (p.kernel, p.blocks, p.split, p.launches) == (4, 120, 1, 1)
    p = attn_plan(B=2, S=1280, **FLUX)  # ... 240 are not; five tiles of 256 keys do not make two ranges
    assert (p.kernel, p.split) == (10, 1)
    assert attn_plan(B=1, S=4225, **FLUX).kernel == 9  # ragged: the one-wave-per-SIMD kernel wants S % 256 == 0
    p = attn_plan(fc.attn_plan_desc(dict(B=1, S=4352, in_kernel=True, **FLUX)), o8_split=256)
    assert (p.kernel, p.quantize, p.launches) == (9, 0, 1)  # the engines' row order of the MX-fp8 copy: attention5.hip does not write it
    assert attn_plan(fc.attn_plan_desc(dict(B=1, S=1280, in_kernel=True, **FLUX)), o8_split=256).quantize == 2  # (the lean kernel: two-range pass)


def test_attention_head_dim_64_and_score_bias_take_the_lean_kernel():
    from diffusionkit_amd import ops
    for H, S_txt in ((24, 589), (38, 333)):  # SD3-medium, SD3.5-large
        for res in (512, 1024):
            for dtype in (ops.BF, ops.F16):
                for attn in (-1, 9, 10):
                    p = attn_plan(B=2, H=H, S=S_txt + (res // 16) ** 2, D=64, dtype=dtype, attn=attn)
                    assert (p.kernel, p.split, p.launches) == (4, 1, 1), (H, res, dtype, attn)
    d = dict(fc.attn_plan_desc(dict(B=1, S=4352, **FLUX)), bias=0x60000000, bias_head_stride=4352 * 4352, ldb=4352)
    for attn in (-1, 9, 10):  # a score bias: only the lean kernel has the form, whatever the knob says
        assert attn_plan(d, attn=attn).kernel == 4
    with pytest.raises(_lib.DkHipError, match="fp16 attention: head_dim 64"):
        attn_plan(B=1, S=4352, dtype=ops.F16, **FLUX)


def test_attention_plan_without_a_workspace_never_splits():
    """workspace_bytes = 0 turns every split into 1 and changes nothing else; so does a workspace one job short"""
    from diffusionkit_amd import ops
    job = _lib.load().dk_attention_workspace_bytes() // 1020  # (the workspace holds 255 blocks x 4 ranges)
    for B, S in ((1, 4352), (2, 4352), (4, 4352), (1, 4608), (1, 2560), (2, 1280), (1, 1280), (1, 4225)):
        a, b = attn_plan(B=B, S=S, **FLUX), attn_plan(B=B, S=S, ws=False, **FLUX)
        want = dict(zip([f for f, _ in a._fields_], fields(a)), split=1, whole=a.blocks, jobs=0, merge=0, launches=a.launches - a.merge)
        assert fields(b) == list(want.values()), (B, S)
        if a.split > 1:
            d = fc.attn_plan_desc(dict(B=B, S=S, **FLUX))
            assert ops.attention_plan(workspace_bytes=a.jobs * job, **d).split == a.split
            assert fields(ops.attention_plan(workspace_bytes=a.jobs * job - 1, **d)) == fields(b)


def test_attention_plan_mode_leaves_no_state_behind():
    """two plans of one shape agree; a forced "attn_split" shows in the plan and is gone after the reset"""
    assert fields(attn_plan(B=4, S=4352, **FLUX)) == fields(attn_plan(B=4, S=4352, **FLUX))
    p = attn_plan(B=1, S=4352, attn_split=3, **FLUX)
    assert (p.split, p.jobs, p.whole, p.merge) == (3, 456, 256, 1)
    assert attn_plan(B=4, S=4352, attn_split=0, **FLUX).split == 1
    assert attn_plan(B=1, S=4352, **FLUX).split == 1 and attn_plan(B=4, S=4352, **FLUX).split == 2
