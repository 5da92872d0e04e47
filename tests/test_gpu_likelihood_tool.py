"""tools/likelihood_time.py runs on tools/timing.py: ``main(argv)`` is called in this process at the smallest arguments it takes
(T = 64, one round, two samples), and what it prints is checked the way tests/test_gpu_consistency_tool.py checks its tool: the
records and their order, the leg names, the bytes of every kernel record, JSON lines, finite positive times, the bandwidth
arithmetic, no capture inside a timed round.  No time is asserted: at these sizes they measure overheads."""
import importlib
import json
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

BT = 2 * 2 * 64 * 256  # elements of a [2, 2, 64, 256] sample
KERNELS = [("lkx_stage, Heun trapezoid row", 6), ("lkx_stage, Euler row", 5), ("lkx_finish", None), ("lkx_sumsq (2 launches)", 1)]
TIMES = ("ms", "us", "ms_per_step")


def _check_numbers(value, key=None):
    if isinstance(value, dict):
        for k, v in value.items():
            _check_numbers(v, k)
    elif isinstance(value, float):
        assert math.isfinite(value), key
        assert value > 0 or key not in TIMES, (key, value)
        assert value >= 0 or key not in ("spread_ms", "margin_ms"), (key, value)


def test_tool_prints_its_records(capsys):
    mod = importlib.import_module("likelihood_time")
    assert "usage: python tools/likelihood_time.py [T=1024] [rounds=6] [B=8]" in mod.__doc__
    mod.main("64 1 2".split())
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    records = [json.loads(ln) for ln in lines]  # every line is JSON
    assert [r["what"] for r in records] == ["ms per replayed network evaluation"] + [k for k, _ in KERNELS]
    for rec in records:
        print(json.dumps(rec))
        _check_numbers(rec)
    step = records[0]
    legs = tuple(k for k, v in step.items() if isinstance(v, dict) and "spread_ms" in v)
    assert legs == ("likelihood", "inpaint_guided") and (step["B"], step["T"]) == (2, 64) and step["rows"] >= 4
    assert all(step[k]["ms_per_step"] > 0 and step[k]["captures_while_timed"] == 0 for k in legs), step
    assert step["likelihood"]["captures"] >= 1
    assert step["likelihood_minus_inpaint_guided_ms"] == step["likelihood"]["ms_per_step"] - step["inpaint_guided"]["ms_per_step"]
    assert step["margin_ms"] == max(step[k]["spread_ms"] for k in legs)
    for rec, (what, passes) in zip(records[1:], KERNELS):
        assert (rec["B"], rec["T"]) == (2, 64), what
        if passes is None:
            assert rec["us"] > 0 and rec["bytes"] == 2 * rec["blocks_per_sample"] * 8
        else:
            assert rec["bytes"] == passes * BT * 4 and rec["frac_of_8TBps"] == rec["bytes"] / 8e12 / (rec["ms"] * 1e-3), what
