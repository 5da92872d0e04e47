"""tools/consistency_time.py runs on tools/timing.py: ``main(argv)`` is called in this process at the smallest arguments it takes
(T = 64, one round, two samples, one step per window), and what it prints is checked the way tests/test_gpu_timing_tools.py checks the
other tools: the records and their order, the leg names, the bytes of every kernel record, JSON lines, finite positive times, the
bandwidth arithmetic, no capture inside a timed round.  No time is asserted: at these sizes they measure overheads."""
import importlib
import json
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

BT = 2 * 2 * 64 * 256  # elements of a [2, 2, 64, 256] sample
KERNELS = [("cmx_consistency_out", 3), ("cmx_consistency_loss (2 launches)", 3), ("cmx_consistency_loss pseudo-Huber (2 launches)", 3),
           ("cmx_consistency_loss_bwd", 4), ("cmx_consistency_update, drawn in the kernel", 4), ("cmx_consistency_update, noise buffer", 5),
           ("cmx_consistency_update, final row", 4)]
TIMES = ("ms", "us", "ms_per_step")


def _check_numbers(value, key=None):
    if isinstance(value, dict):
        for k, v in value.items():
            _check_numbers(v, k)
    elif isinstance(value, float):
        assert math.isfinite(value), key
        assert value > 0 or key not in TIMES, (key, value)
        assert value >= 0 or key != "spread_ms", (key, value)


def test_tool_prints_its_records(capsys):
    mod = importlib.import_module("consistency_time")
    assert "usage: python tools/consistency_time.py [T=1024] [rounds=6] [B=32] [iters=3] [SB=8]" in mod.__doc__
    mod.main("64 1 2 1 2".split())
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    records = [json.loads(ln) for ln in lines]  # every line is JSON
    assert [r["what"] for r in records] == ["ms per eager optimisation step", "ms per replayed sampler step"] + [k for k, _ in KERNELS]
    for rec in records:
        print(json.dumps(rec))
        _check_numbers(rec)
    step, sampler = records[:2]
    assert tuple(k for k, v in step.items() if isinstance(v, dict) and "spread_ms" in v) == ("train", "distill", "consistency", "teacher_eval_forward")
    assert all(step[k]["ms_per_step"] > 0 for k in ("train", "distill", "consistency")) and (step["B"], step["T"]) == (2, 64)
    assert step["consistency_over_train"] == step["consistency"]["ms_per_step"] / step["train"]["ms_per_step"]
    legs = tuple(k for k, v in sampler.items() if isinstance(v, dict) and "spread_ms" in v)
    assert legs == ("consistency", "ddim_eta1") and (sampler["B"], sampler["T"]) == (2, 64) and sampler["steps"] >= 4
    assert all(sampler[k]["ms_per_step"] > 0 and sampler[k]["captures"] == 1 and sampler[k]["captures_while_timed"] == 0 for k in legs), sampler
    for rec, (what, passes) in zip(records[2:], KERNELS):
        assert rec["bytes"] == passes * BT * 4 and (rec["B"], rec["T"]) == (2, 64), what
        assert "ms" in rec and rec["frac_of_8TBps"] == rec["bytes"] / 8e12 / (rec["ms"] * 1e-3), what
