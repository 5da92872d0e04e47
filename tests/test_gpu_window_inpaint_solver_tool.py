"""tools/window_inpaint_solver_time.py runs on tools/timing.py: ``main(argv)`` is called in this process at the smallest arguments
it takes (one round; the canvas of L = 4608 is built in; the ``wall`` leg, 220 guided steps, is left out through the tool's own
selector), and what it prints is checked the way tests/test_gpu_timing_tools.py checks the other tools: the records and their order,
the leg names, the bytes of every kernel record, JSON lines, finite positive times, the bandwidth arithmetic, no capture inside a
timed round.  No time is asserted."""
import importlib
import json
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

STEP = "ms per replayed sampler step"
M18, C18 = 8 * 2 * 1024 * 256, 2 * (1024 + 7 * 512) * 256  # window batch and canvas elements of the fixed 1 x 8 case
LEGS = ("winp_guided", "wis_guided_order2", "wis_guided_order3", "window_solver_o2", "wis_replace_order2")
# (what, passes over the window batch, passes over the canvas)
KERNELS = [("ddimxwis_residual", 2, 5), ("ddimxwi_update guided + replace (for comparison)", 1, 6),
           ("ddimxwis_multistep_update guided + replace, order-1 row", 1, 7), ("ddimxwis_multistep_update guided + replace, order 2 (h1)", 1, 8),
           ("ddimxwis_multistep_update guided + replace, order 3 (h1, h2)", 1, 10), ("ddimxwi_update replace only (for comparison)", 1, 5),
           ("ddimxwis_multistep_update replace only, order 2 (h1)", 1, 7),
           ("ddimxi_multistep_update guided + replace, order 2 (h1), at batch N W", 9, 0)]
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
    mod = importlib.import_module("window_inpaint_solver_time")
    assert "usage: python tools/window_inpaint_solver_time.py [rounds=5] [wall]" in mod.__doc__
    mod.main(["1"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    records = [json.loads(ln) for ln in lines]  # every line is JSON
    assert [r["what"] for r in records] == [k[0] for k in KERNELS] + [STEP]
    for rec, (what, m_passes, c_passes) in zip(records, KERNELS):
        print(json.dumps(rec))
        _check_numbers(rec)
        assert rec["bytes"] == (m_passes * M18 + c_passes * C18) * 4, what
        assert "us" in rec and "ms" not in rec
        assert rec["frac_of_8TBps"] == pytest.approx(rec["bytes"] / 8e12 / (rec["us"] * 1e-6), rel=1e-12), what
    rec = records[-1]
    print(json.dumps(rec))
    _check_numbers(rec)
    assert tuple(k for k, v in rec.items() if isinstance(v, dict) and "spread_ms" in v) == LEGS
    assert all(rec[k]["ms_per_step"] > 0 and rec[k]["captures_while_timed"] == 0 for k in LEGS), rec
    assert (rec["N"], rec["W"], rec["T"], rec["H"], rec["L"]) == (1, 8, 1024, 512, 4608)
