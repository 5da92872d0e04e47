"""Every feature timing tool (tools/*_time.py) runs on tools/timing.py: each ``main(argv)`` is called in this process at the smallest
arguments it takes, and what it prints is checked against a table copied from the tools as they were before they shared a harness --
the records and their order, the leg names, the bytes of every kernel record -- and for sanity: JSON lines, finite positive times,
the bandwidth arithmetic.  No time is asserted: at these sizes they measure overheads.

T = 64 is two multiples of the 32 the six-level audio model requires: the smallest size at which the order-3 history buffers, the
guided path and the per-sample grid are all live.  The windowed tools have T = 1024 built in and take the 1 x 2 case;
window_inpaint_time has no size argument.  window_time's and window_solver_time's ``long`` legs (L = 8192) and pool_time's wall-clock
workload (``what`` b, c: 32 requests of up to 100 steps) are left out through the tools' own selectors: they run for many seconds."""
import importlib
import json
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

STEP = "ms per replayed sampler step"
BT = 2 * 2 * 64 * 256                                  # elements of a [2, 2, 64, 256] sample
M12, C12 = 2 * 2 * 1024 * 256, 2 * (1024 + 512) * 256  # window batch and canvas elements of the 1 x 2 case
M18, C18 = 8 * 2 * 1024 * 256, 2 * (1024 + 7 * 512) * 256  # ... of window_inpaint_time's fixed 1 x 8


def legs(what, *names):
    return ("legs", what, names)


def kern(what, passes, numel=BT):
    """A kernel record: ``passes`` sample-sized fp32 passes over ``numel`` elements."""
    return ("kernel", what, passes * numel * 4)


def win(what, m_passes, c_passes, m=M12, c=C12):
    """A windowed kernel's record: passes over the window batch and over the canvas."""
    return ("kernel", what, (m_passes * m + c_passes * c) * 4)


def other(what, nbytes=None):
    return ("other", what, nbytes)


_INPAINT_SOLVER_KERNELS = [kern("ddimx_inpaint_update guided+replace (for comparison)", 6),
                           kern("ddimxi_multistep_update guided+replace, order-1 row", 8),
                           kern("ddimxi_multistep_update guided+replace, order 2 (h1)", 9),
                           kern("ddimxi_multistep_update guided+replace, order 3 (h1, h2)", 11),
                           kern("ddimxi_multistep_update replace only, order 2 (h1)", 8), kern("ddimxi_residual", 6)]
_UNIC_KERNELS = [kern("ddimx_multistep_update order 2", 5), kern("ddimx_multistep_update order 3", 7),
                 kern("ddimxu_multistep_update order-2 row of the plain solver, no history buffer", 5),
                 kern("ddimxu_multistep_update corrector at order 2 (hist)", 7),
                 kern("ddimxu_multistep_update corrector at order 3 (hist, hist2)", 9)]
_BROWNIAN_ROWS = [other(f"{k}, the row with the {row}") for row in ("most draws", "fewest draws")
                  for k in ("ddimxb_multistep_update order 2", "ddimxb_path_fill increment", "ddimxb_path_fill path")]

# tool -> (argv, the records it prints, in order)
TOOLS = {
    "brownian": ("64 1 2", [legs(STEP, "order2_tau0", "order2_tau1_stream", "order2_tau1_path", "order3_tau1_path"),
                            other("ddimxs_multistep_update order 2, drawn in the kernel"), *_BROWNIAN_ROWS]),
    "distill": ("64 1 2 1", [legs("ms per eager optimisation step", "train", "weighted", "distill", "teacher_eval_forward"),
                             kern("ddimxd_distill_half", 4), kern("ddimxd_distill_target", 5)]),
    # the data-gradient kernel reads dy [B, T, 256, 32] (bf16 or fp32) and writes d_x [B, 2, T, 256] fp32
    "input_grad": ("64 1 2", [legs("fwd+bwd", "full", "full_dx", "data_only"),
                              ("kernel", "ddimx_conv_in_bwd_data", 2 * 64 * 256 * 32 * 2 + BT * 4),
                              ("kernel", "ddimx_conv_in_bwd_data", 2 * 64 * 256 * 32 * 4 + BT * 4)]),
    "inpaint": ("64 1 2", [legs("ms per sampler step", "generalized", "replace", "guided", "guided_eager", "recipe"),
                           kern("ddimx_inpaint_residual", 6), kern("ddimx_inpaint_update guided+replace", 6),
                           kern("ddimx_inpaint_update replace", 6), kern("ddimx_ddim_update (for comparison)", 4)]),
    "inpaint_solver": ("64 1 2", [legs(STEP, "inpaint_guided", "solver_order2", "guided_order2", "guided_order3", "replace_order2"),
                                  *_INPAINT_SOLVER_KERNELS, *_INPAINT_SOLVER_KERNELS[::-1],
                                  legs("wall ms, guided inpainting", "inpaint_solver_steps 20 x order 2", "inpaint_steps 200")]),
    "invert": ("64 1 2", [legs("ms per replayed step", "ddim_a", "invert", "ddim_b"), kern("ddimx_ddim_update (for comparison)", 4),
                          kern("ddimx_invert_update, first row of a level", 5), kern("ddimx_invert_update, later row", 5),
                          other("ddimx_slerp, M = 11", (4 + 11) * 1 * (BT // 2) * 4)]),
    "noise": ("64 1 2", [legs("ms per sampler step", "eta0", "eta1_stream", "eta1_torch"), kern("ddimx_noise_fill normals", 1),
                         kern("ddimx_noise_fill words", 1), kern("ddimx_ddim_update without noise", 4),
                         kern("ddimx_ddim_update with noise", 5)]),
    "pool": ("64 1 what=a", [legs("ms per replayed step, 8 busy slots vs B = 8", "ddim_eta0", "pool_eta0", "ddim_eta1", "pool_eta1")]),
    "sde": ("64 1 2", [legs(STEP, "order2_tau0", "order2_tau1", "order3_tau1", "ddim_eta1"),
                       kern("ddimx_multistep_update order 2 (tau = 0)", 5), kern("ddimxs_multistep_update order 2, c1 = 0 row", 5),
                       kern("ddimxs_multistep_update order 2, drawn in the kernel", 5),
                       kern("ddimxs_multistep_update order 2, noise buffer", 6),
                       kern("ddimxs_multistep_update order 3, drawn in the kernel", 7),
                       kern("ddimx_noise_fill + ddimx_ddim_update (eta = 1)", 6),
                       kern("ddimxs_multistep_update first-order row, drawn in the kernel", 4)]),
    "solver": ("64 1 2", [legs(STEP, "generalized", "order2", "order3"), kern("ddimx_ddim_update (for comparison)", 4),
                          kern("ddimx_multistep_update order 1 row", 4), kern("ddimx_multistep_update order 2", 5),
                          kern("ddimx_multistep_update order 3", 7)]),
    "threshold": ("64 1 2", [legs(STEP, "none", "clip", "dynamic"), kern("ddimxq_x0_quantile (4 launches)", 6),
                             kern("ddimxq_threshold_eps", 3)]),
    "unic": ("64 1 2", [legs(STEP, "order2", "order2_unic", "order3", "order3_unic"), *_UNIC_KERNELS, *_UNIC_KERNELS[::-1]]),
    "vpred": ("64 1 2", [legs(STEP, "eps", "v"), kern("ddimx_v_to_eps", 3), kern("ddimx_v_to_eps in place", 3),
                         kern("ddimx_qsample_v", 4)]),
    "window": ("1 1x2", [win("ddimx_window_gather", 2, 0), win("ddimx_window_update", 1, 3), win("ddimx_window_update with noise", 1, 4),
                         win("gather + update back to back", 3, 3), win("ddimx_ddim_update at batch N W", 4, 0),
                         legs("ms per sampler step", "generalized", "windowed")]),
    "window_inpaint": ("1", [win("ddimxwi_residual", 2, 5, M18, C18), win("ddimxwi_update guided + replace", 1, 6, M18, C18),
                             win("ddimxwi_update replace only", 1, 5, M18, C18),
                             win("ddimxwi_update replace only, with noise", 1, 6, M18, C18),
                             win("ddimx_inpaint_residual at batch N W", 6, 0, M18, C18),
                             win("ddimx_inpaint_update guided + replace at batch N W", 6, 0, M18, C18),
                             legs(STEP, "windowed_ddim", "inpaint_guided", "winp_replace_only", "winp_guided")]),
    "window_solver": ("1 1x2", [win("ddimx_window_update", 1, 3), win("ddimxw_multistep_update order 1 row", 1, 3),
                                win("ddimxw_multistep_update order 2 row", 1, 4), win("ddimxw_multistep_update order 2 row, z drawn", 1, 4),
                                win("ddimxw_multistep_update order 2 row, z from a buffer", 1, 5),
                                win("ddimxw_multistep_update order 3 row", 1, 6), win("ddimxw_blend", 1, 1),
                                legs(STEP, "windowed_ddim", "solver_o2", "solver_o2_tau1", "solver_o2_threshold", "solver_o2_path")]),
}
TIMES = ("ms", "us", "ms_per_step", "fwd_bwd_ms", "fwd_ms", "bwd_ms")  # durations: positive.  spread_ms is 0 after one round


def _check_numbers(value, key=None):
    if isinstance(value, dict):
        for k, v in value.items():
            _check_numbers(v, k)
    elif isinstance(value, list):
        for v in value:
            _check_numbers(v, key)
    elif isinstance(value, float):
        assert math.isfinite(value), key
        assert value > 0 or key not in TIMES, (key, value)
        assert value >= 0 or key != "spread_ms", (key, value)


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_tool_prints_what_it_printed_before(tool, capsys):
    argv, table = TOOLS[tool]
    importlib.import_module(tool + "_time").main(argv.split())
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    records = [json.loads(ln) for ln in lines]  # every line is JSON
    assert [r["what"] for r in records] == [what for _, what, _ in table]
    for rec, (kind, what, want) in zip(records, table):
        print(json.dumps(rec))
        _check_numbers(rec)
        if kind == "legs":
            got = [k for k, v in rec.items() if isinstance(v, dict) and "spread_ms" in v]
            assert tuple(got) == want, what
            assert all(set(TIMES) & set(rec[k]) for k in got)
        elif want is not None:
            assert rec["bytes"] == want, what
        if kind == "kernel":
            assert ("ms" in rec) != ("us" in rec)
            if "ms" in rec:
                assert rec["frac_of_8TBps"] == rec["bytes"] / 8e12 / (rec["ms"] * 1e-3), what
            else:  # printed in us: the last bit of the time is not the one the share was computed from
                assert rec["frac_of_8TBps"] == pytest.approx(rec["bytes"] / 8e12 / (rec["us"] * 1e-6), rel=1e-12), what
        if tool == "inpaint_solver" and kind == "legs" and what == STEP:
            assert all(rec[k]["captures_while_timed"] == 0 for k in want), rec
