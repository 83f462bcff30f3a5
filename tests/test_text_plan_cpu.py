"""What dk_gemm_plan launches for the text encoders' Linears (CPU only, as tests/test_dispatch_plan.py): ops.linear passes no workspace, so nothing may be
cut along K, and every kernel a text Linear is routed to must have a parity case at a text shape in tests/test_gpu_text_ops.py.  A route that appears
later -- another kernel for one of these shapes -- fails here until tests/_textcases.py: GEMM_CASES names it."""
from tests import _textcases as tc
from tests.test_dispatch_plan import plan


def test_every_text_linear_plans_one_unsplit_launch():
    """at 1, 2, 77, 154, 256, 512 and 1024 rows, every Linear: without a workspace nothing is cut along K, whatever kernel the rows select"""
    assert set(tc.text_linears()) <= set(tc.text_linears(reachable=False))
    for what, M, N, K in tc.text_linears(reachable=False):
        p = plan(M, N, K, ws=False)  # (asserts that the planner accepted the shape)
        assert p.launches == 1 and p.tiles > 0 and p.workgroups == p.tiles, (what, M, p.launches, p.tiles, p.workgroups)
        assert p.split_tiles == 0 and p.k_pieces == 1, (what, M, p.split_tiles, p.k_pieces)
        assert p.ks == K // 64, (what, M, p.ks)  # the whole reduction in one workgroup


def test_gpu_parity_cases_sit_on_the_routes_they_name():
    for M, N, K, tail, bias, kernel, tile_rows in tc.GEMM_CASES:
        p = plan(M, N, K, ws=False)
        assert (p.kernel, p.tile_rows, p.split_tiles) == (kernel, tile_rows, 0), (M, N, K, p.kernel, p.tile_rows)
        assert (M, N, K) in {(m, n, k) for _, m, n, k in tc.text_linears()}, f"{(M, N, K)} is no text Linear"


def test_planned_kernels_are_exactly_the_ones_with_a_parity_case():
    planned = {}
    for what, M, N, K in tc.text_linears():
        p = plan(M, N, K, ws=False)
        planned.setdefault((p.kernel, p.tile_rows), (what, M))
    named = {(kernel, tile_rows) for *_, kernel, tile_rows in tc.GEMM_CASES}
    assert set(planned) == named, f"planned (kernel, tile rows) -> first Linear: {planned}; with a parity case: {sorted(named)}"


def test_t5_long_reduction_and_route_flip():
    """T5 wo (K = 10240) is 160 K tiles on the 128-tile kernel up to 512 rows; qkv at 256 rows is 192 tiles; two 512-token prompts flip wo to
    gemm256v4 with 224-row tiles on 80 workgroups"""
    for M in (77, 256):
        p = plan(M, 4096, 10240, ws=False)
        assert (p.kernel, p.ks) == (tc.KERNEL_128, 160)
    assert plan(256, 12288, 4096, ws=False).tiles == 192
    p = plan(1024, 4096, 10240, ws=False)
    assert (p.kernel, p.tile_rows, p.workgroups, p.split_tiles) == (tc.KERNEL_V4, 224, 80, 0)
