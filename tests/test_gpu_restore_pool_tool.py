"""tools/restore_pool_time.py runs on tools/timing.py: ``main(argv)`` is called in this process at the smallest arguments it takes
(T = 64, one round, four requests), and what it prints is checked the way tests/test_gpu_likelihood_tool.py checks its tool: the
records and their order, the leg names, the bytes of every kernel record, JSON lines, finite positive times, the bandwidth
arithmetic, one capture per pool, the workload's results bit-identical three ways.  No time is asserted: at these sizes they
measure overheads."""
import importlib
import json
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

BT = 8 * 2 * 64 * 256  # elements of the pooled [8, 2, 64, 256] batch
KERNELS = [("ddimx_pool_update (for comparison)", 7), ("rpx_pool_update, every slot plain", 7), ("rpx_pool_update, every slot known", 9)]
LEGS = ("restore_pool", "generate_pool", "sampler_pool", "inpaint_replace")
TIMES = ("ms", "us", "ms_per_step", "pool_s", "grouped_b8_s", "one_by_one_b1_s")


def _check_numbers(value, key=None):
    if isinstance(value, dict):
        for k, v in value.items():
            _check_numbers(v, k)
    elif isinstance(value, float):
        assert math.isfinite(value), key
        assert value > 0 or key not in TIMES, (key, value)
        assert value >= 0 or key not in ("spread_ms", "margin_ms"), (key, value)


def test_tool_prints_its_records(capsys):
    mod = importlib.import_module("restore_pool_time")
    assert "usage: python tools/restore_pool_time.py [T=1024] [rounds=6] [what=abc] [n=32]" in mod.__doc__
    mod.main("64 1 abc 4".split())
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    records = [json.loads(ln) for ln in lines]  # every line is JSON
    kernel_order = [k for k, _ in KERNELS]
    assert [r["what"] for r in records] == (["ms per replayed step, 8 busy slots vs B = 8"] + kernel_order + kernel_order[::-1]
                                            + ["4 requests, half restoration (20 steps), half generation (20 / 50 steps), order 2: wall seconds"])
    for rec in records:
        print(json.dumps(rec))
        _check_numbers(rec)
    step = records[0]
    legs = tuple(k for k, v in step.items() if isinstance(v, dict) and "spread_ms" in v)
    assert legs == LEGS and (step["B"], step["T"], step["steps_timed"], step["rounds"]) == (8, 64, 18, 1)
    assert all(step[k]["ms_per_step"] > 0 for k in legs) and step["inpaint_replace"]["captures_while_timed"] == 0
    for k in LEGS[1:]:
        assert step[f"restore_pool_minus_{k}_ms"] == step["restore_pool"]["ms_per_step"] - step[k]["ms_per_step"]
    assert step["margin_ms"] == max(step[k]["spread_ms"] for k in legs)
    passes = dict(KERNELS)
    for rec in records[1:7]:
        assert (rec["B"], rec["T"]) == (8, 64)
        assert rec["bytes"] == passes[rec["what"]] * BT * 4 and rec["frac_of_8TBps"] == rec["bytes"] / 8e12 / (rec["ms"] * 1e-3), rec["what"]
    wall = records[-1]
    assert wall["bit_identical_to_one_by_one"] is True
    assert wall["pool_stats"]["captures"] == 1 and wall["pool_stats"]["busy"] == wall["slot_steps"] >= 4 * 20
    assert wall["pool_over_grouped"] == wall["pool_s"] / wall["grouped_b8_s"]
