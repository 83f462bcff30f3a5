"""The control flow of the host step loops (``pipeline.sample_euler`` / ``sample_steps``) without a GPU: every call they make to the engine and to the
step operators, in order and with every scalar argument, against the committed traces (tests/golden/step_loop_traces.json, written by
tests/golden/make_step_loop_traces.py from fakes of the engine, of the ``ops`` wrappers and of ``torch.cuda.synchronize``)."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_step_loop_traces as gen  # noqa: E402

with open(gen.FIXTURE) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_holds_the_cases():
    assert sorted(GOLDEN) == sorted(gen.CASES)


@pytest.mark.parametrize("name", sorted(gen.CASES))
def test_step_loop_trace(name):
    got, want = gen.run_case(**gen.CASES[name]), GOLDEN[name]
    for k, (g, w) in enumerate(zip(got["events"], want["events"])):
        assert g == w, f"{name}: event {k}"
    assert len(got["events"]) == len(want["events"])
    assert got["n_iter_time"] == want["n_iter_time"]
    assert got["block_cache_record"] == want["block_cache_record"]
    assert got["guidance_record"] == want["guidance_record"]
    assert got == want


def test_the_cases_reach_every_branch():
    """what the traces are there to pin: each operator, a skipped and a recomputed cached step, a decision overruled after a change of rows, and a
    momentum buffer that is left, read and left unread"""
    ops_seen = {e["op"] for t in GOLDEN.values() for e in t["events"] if isinstance(e, dict)}
    assert ops_seen == {"euler_cfg_step", "euler_cfg_step_masked", "lms_cfg_step", "lms_cfg_step_masked", "guided_cfg_step"}
    assert GOLDEN["euler_block_cache"]["block_cache_record"]["skipped"] == [1]
    assert GOLDEN["ab2_block_cache"]["block_cache_record"]["skipped"] == [1]
    assert GOLDEN["interval_block_cache"]["block_cache_record"]["skipped"] == []  # (FixedSchedule({1}) overruled: the engine was re-prepared)
    assert sum(e == ["reset_block_cache"] for e in GOLDEN["interval_block_cache"]["events"]) == 2
    for name in ("euler_cfg_off", "euler_cfg_on", "euler_masked", "euler_block_cache"):  # (the default path calls no coefficient-row entry)
        assert {e["op"] for e in GOLDEN[name]["events"] if isinstance(e, dict)} <= {"euler_cfg_step", "euler_cfg_step_masked"}
    guided = [e for e in GOLDEN["interval_apg_momentum_heun"]["events"] if isinstance(e, dict) and e["op"] == "guided_cfg_step"]
    assert [(e["reads_m"], e["writes_m"]) for e in guided] == [(False, True), (True, False)]
    guided = [e for e in GOLDEN["ab2_apg_momentum"]["events"] if isinstance(e, dict) and e["op"] == "guided_cfg_step"]
    assert [(e["reads_m"], e["writes_m"]) for e in guided] == [(False, True), (True, True), (True, False)]
