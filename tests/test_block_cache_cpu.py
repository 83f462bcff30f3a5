"""First-block cache without a GPU: the two host policies against known answers, the CLI flag, the new names in the header, the library's
export table and the ctypes table, and the workspace rule (off: today's bytes; on: three image-row buffers and the probe's partial sums more)."""
import ctypes
import math
import re

import pytest

from diffusionkit_amd import _lib, cli
from diffusionkit_amd.config import MMDIT_CKPT, tiny_flux, tiny_sd3
from diffusionkit_amd.sampler import BlockCachePolicy, FixedSchedule, block_cache_rel
from tests.test_abi_and_host import _mmdit_handle

INF = math.inf
NEW_NAMES = ("dk_mmdit_set_block_cache", "dk_mmdit_reset_block_cache", "dk_mmdit_forward_head", "dk_mmdit_forward_tail",
             "dk_block_probe_bf16", "dk_block_probe_f16", "dk_block_residual_bf16", "dk_block_residual_f16")


def decisions(policy, rels):
    return [policy.decide(i, len(rels), r) for i, r in enumerate(rels)]


# ---- the policies ------------------------------------------------------------------------------------------------------------------
def test_first_and_last_step_always_compute():
    for policy in (BlockCachePolicy(INF), BlockCachePolicy(0.5), FixedSchedule(range(6))):
        assert decisions(policy, [0.0] * 6) == [False, True, True, True, True, False]
    assert decisions(BlockCachePolicy(INF), [0.0]) == [False]          # one step: it is the first and the last
    assert decisions(BlockCachePolicy(INF), [0.0, 0.0]) == [False, False]


def test_threshold_rule_is_strict():
    """skip iff rel < threshold"""
    assert decisions(BlockCachePolicy(0.1), [0.0, 0.05, 0.1, 0.2, 0.0999, 0.0]) == [False, True, False, False, True, False]


def test_threshold_zero_never_skips_and_inf_skips_everything_between():
    rels = [INF, 0.0, 1e-30, 5.0, 0.0]
    assert decisions(BlockCachePolicy(0.0), rels) == [False] * 5
    assert decisions(BlockCachePolicy(INF), [INF, 0.0, 1e30, 5.0, 0.0]) == [False, True, True, True, False]


def test_den_zero_gives_inf_and_computes():
    """rel = max over the batch rows of num / den; den == 0 gives inf, which is below no threshold -- not even inf"""
    assert block_cache_rel([(3.0, 0.0)]) == INF
    assert block_cache_rel([(0.0, 0.0)]) == INF
    assert block_cache_rel([(1.0, 4.0), (3.0, 4.0)]) == 0.75
    assert block_cache_rel([(1.0, 4.0), (3.0, 0.0)]) == INF
    assert block_cache_rel([(2.0, 8.0)]) == 0.25
    assert decisions(BlockCachePolicy(INF), [INF, INF, 0.0, 0.0]) == [False, False, True, False]
    assert math.isnan(block_cache_rel([(float("nan"), 1.0), (0.0, 1.0)]))
    assert decisions(BlockCachePolicy(INF), [0.0, float("nan"), 0.0]) == [False, False, False]


def test_skip_cap():
    rels = [0.0] * 8
    assert decisions(BlockCachePolicy(1.0, max_consecutive_skips=2), rels) == [False, True, True, False, True, True, False, False]
    assert decisions(BlockCachePolicy(1.0, max_consecutive_skips=1), rels) == [False, True, False, True, False, True, False, False]
    assert decisions(BlockCachePolicy(1.0, max_consecutive_skips=0), rels) == [False] * 8
    # a computed step in between restarts the count; a second run of the same object starts over at step 0
    p = BlockCachePolicy(1.0, max_consecutive_skips=2)
    assert decisions(p, [0.0, 0.0, 5.0, 0.0, 0.0, 0.0, 0.0]) == [False, True, False, True, True, False, False]
    assert decisions(p, [0.0, 0.0, 0.0, 0.0]) == [False, True, True, False]


def test_fixed_schedule_ignores_rel():
    assert decisions(FixedSchedule([1, 2]), [INF, INF, 0.0, 0.0]) == [False, True, True, False]
    assert decisions(FixedSchedule([0, 2, 3, 9]), [0.0] * 4) == [False, False, True, False]
    assert decisions(FixedSchedule([]), [0.0] * 4) == [False] * 4


def test_policy_rejects_bad_arguments():
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match=">= 0"):
            BlockCachePolicy(bad)
    with pytest.raises(ValueError):
        BlockCachePolicy(0.1, max_consecutive_skips=-1)


# ---- the CLI flag ------------------------------------------------------------------------------------------------------------------
def _args(*extra):
    return cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(["--prompt", "a cat", *extra])


def test_cli_flag_parses_and_rejects_negatives():
    assert "block_cache" not in cli.resolve(_args())  # (a key only when the flag is given)
    assert cli.resolve(_args("--block-cache", "0.1"))["block_cache"] == 0.1
    assert cli.resolve(_args("--block-cache", "0"))["block_cache"] == 0.0
    assert cli.resolve(_args("--block-cache", "inf"))["block_cache"] == INF
    for bad in ("-0.1", "nan"):
        with pytest.raises(ValueError, match="Block cache threshold"):
            cli.resolve(_args("--block-cache", bad))
    with pytest.raises(SystemExit):
        _args("--block-cache", "often")


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def test_new_names_in_header_export_table_and_ctypes_table():
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    declared = set(re.findall(r"\b(dk_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for name in NEW_NAMES:
        assert name in declared, f"{name} is not declared in include/dk_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in _lib.SIGNATURES, f"{name} is missing from the ctypes table"
    assert lib.dk_abi_version() == 5  # (additive)
    # one implementation per operator pair: the two entries of a pair have the same signature
    for op in ("dk_block_probe", "dk_block_residual"):
        assert _lib.SIGNATURES[op + "_bf16"] == _lib.SIGNATURES[op + "_f16"]


@pytest.mark.parametrize("cfg,shape", [(tiny_flux(), (1, 8, 8, 16, 3)), (tiny_sd3(), (2, 8, 12, 20, 3))])
def test_workspace_grows_only_with_the_cache_on(cfg, shape):
    """off: the bytes an engine reports that never heard of the option (tests/test_abi_and_host.py pins them); on: three image-row buffers and
    the (num, den) pair per image row more, each on its own 256-byte boundary; off again: the first number"""
    lib = _lib.load()
    h = _mmdit_handle(lib, cfg)
    try:
        off = lib.dk_mmdit_workspace_bytes(h, *shape)
        assert lib.dk_mmdit_set_block_cache(h, 1) == 0
        on = lib.dk_mmdit_workspace_bytes(h, *shape)
        assert lib.dk_mmdit_set_block_cache(h, 0) == 0
        assert lib.dk_mmdit_workspace_bytes(h, *shape) == off
    finally:
        lib.dk_mmdit_destroy(h)
    B, Hl, Wl = shape[:3]
    rows = B * (Hl // cfg.patch_size) * (Wl // cfg.patch_size)
    payload = 3 * rows * cfg.hidden_size * 2 + rows * 2 * 4
    assert payload <= on - off < payload + 4 * 256, (off, on, payload)


def test_head_and_tail_refuse_an_unprepared_engine():
    """no launch without a prepared, cache-enabled engine: the entries answer with an error that names the rule (no GPU is touched)"""
    lib = _lib.load()
    h = _mmdit_handle(lib, tiny_flux())
    try:
        assert lib.dk_mmdit_forward_tail(h, 0, 1, ctypes.c_void_p(256), None) != 0
        assert b"prepare" in lib.dk_last_error()
        assert lib.dk_mmdit_forward_head(h, ctypes.c_void_p(256), None, 0, ctypes.c_void_p(256), None) != 0
        assert b"prepare" in lib.dk_last_error()
        assert lib.dk_mmdit_debug_buffer(h, 3) is None
    finally:
        lib.dk_mmdit_destroy(h)
