"""Windowed multistep sampler timing on one MI355X: the audio config (bf16 activations), windows of T = 1024 at hop 512, HIP events
after warm-up (every round times each leg once, 10 replayed steps between two events, the order within a round alternates, the
spread of every leg over the rounds is reported).

For every (N canvases, W windows per canvas) case, in one process, ms per replayed sampler step over the same 20-entry log-SNR
schedule of
  windowed_ddim        -- WindowStepper (windowed_steps, eta = 0): what existed before, the yardstick;
  solver_o2            -- WindowSolverStepper, order 2, tau = 0: the fused kernel (ddimxw_multistep_update);
  solver_o2_tau1       -- the same at tau = 1 with a NoiseStream: the fused kernel draws z itself;
  solver_o2_threshold  -- tau = 0 with an X0Threshold: ddimxw_blend, the quantile and rewrite on the canvas, ddimx_multistep_update;
  solver_o2_path       -- tau = 1 with a BrownianStream: ddimxw_blend, then ddimxb_multistep_update.
Then the kernels alone (50 calls captured into one graph, the replay between two events): us per call and the bytes they move as a
share of the 8 TB/s HBM peak.  With ``long``: wall time of whole runs on one canvas of L = 8192 (15 windows) -- 20 logsnr_seq steps
of windowed_solver_steps at order 2 against 200 uniform steps of windowed_steps, each run three times in alternation after one
warm-up run, host clock around a synchronised run.
usage: python tools/window_solver_time.py [rounds=5] [long] [NxW ...=1x8 1x32]   (rounds = 0: the kernels alone)
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.sampler import _threshold  # noqa: E402
from ddim_audio_amd.schedule import (X0Threshold, brownian_plan, ddim_coefficients, dpm_coefficients, logsnr_seq, make_schedule,  # noqa: E402
                                     make_seq, window_plan)
from ddim_audio_amd.window import WindowSolverStepper, WindowStepper  # noqa: E402

T, H, F = 1024, 512, 256
N_TIMED = 10
SEED = 0x5EED


def time_case(m, n, w, rounds):
    length = T + (w - 1) * H
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    x = torch.randn((n, 2, length, F), device="cuda")
    c0, c1 = dpm_coefficients(seq, alphas, 2), dpm_coefficients(seq, alphas, 2, tau=1.0)
    with torch.no_grad():
        xs = [x.clone() for _ in range(5)]
        steppers = {
            "windowed_ddim": WindowStepper(m, xs[0], ddim_coefficients(seq, alphas, 0.0), T, H, "tri"),
            "solver_o2": WindowSolverStepper(m, xs[1], c0, 2, T, H, "tri"),
            "solver_o2_tau1": WindowSolverStepper(m, xs[2], c1, 2, T, H, "tri", noise=D.NoiseStream(SEED)),
            "solver_o2_threshold": WindowSolverStepper(m, xs[3], c0, 2, T, H, "tri", threshold=_threshold(X0Threshold(0.995, 1.0), alphas)),
            "solver_o2_path": WindowSolverStepper(m, xs[4], c1, 2, T, H, "tri", noise=D.BrownianStream(SEED),
                                                  plan=brownian_plan(seq, alphas, 1.0))}
    r, _ = timing.time_legs({k: timing.stepper_leg(st, xt, x, N_TIMED) for (k, st), xt in zip(steppers.items(), xs)}, rounds)
    base = r["windowed_ddim"]["ms_per_step"]
    return {"what": "ms per replayed sampler step", "N": n, "W": w, "T": T, "H": H, "L": length, "dtype": "bf16", "rounds": rounds, **r,
            "minus_windowed_ddim_ms": {k: v["ms_per_step"] - base for k, v in r.items() if k != "windowed_ddim"}}


def time_kernels(n, w):
    lib, P = _lib.load(), _lib.ptr
    length = T + (w - 1) * H
    canvas, x0, hist, nz, beps = (torch.randn((n, 2, length, F), device="cuda") for _ in range(5))
    eps = torch.randn((n * w, 2, T, F), device="cuda")
    p = window_plan(length, T, H, "tri")
    jf, cn, wt = (torch.from_numpy(v.copy()).cuda() for v in (p.jfirst, p.cnt, p.wt))
    row = [500.0, 0.6, 0.8, 0.6, 0.4, 0.1, 0.05, 0.02]
    coef6 = torch.tensor([row[:6]], device="cuda")
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    geom = (n, w, 2, length, T, H, F)
    m_b, c_b = eps.numel() * 4, canvas.numel() * 4
    out = []

    def report(name, fn, nbytes, note):
        canvas.normal_()
        ms = timing.time_graph_replay(fn, reps=50, warm=3)
        out.append({**timing.bandwidth_record(name, ms, 1, nbytes, unit="us", N=n, W=w), "note": note})

    def fused(c1, w1, w2, h, noise):
        coef = torch.tensor([row[:5] + [c1, w1, w2]], device="cuda")
        return lambda: _lib.check(lib.ddimxw_multistep_update(P(canvas), P(eps), P(noise), P(x0), P(h), P(jf), P(cn), P(wt), P(coef), P(ctr),
                                                              *geom, SEED, 0, 0, _lib.stream()))

    report("ddimx_window_update", lambda: _lib.check(lib.ddimx_window_update(P(canvas), P(eps), None, P(x0), P(jf), P(cn), P(wt), P(coef6),
                                                                             P(ctr), *geom, _lib.stream())),
           m_b + 3 * c_b, "eps read; canvas read and written, x0 written")
    report("ddimxw_multistep_update order 1 row", fused(0.0, 0.0, 0.0, None, None), m_b + 3 * c_b, "the same traffic")
    report("ddimxw_multistep_update order 2 row", fused(0.0, row[6], 0.0, None, None), m_b + 4 * c_b, "+ x0 read")
    report("ddimxw_multistep_update order 2 row, z drawn", fused(row[5], row[6], 0.0, None, None), m_b + 4 * c_b, "+ Philox and Box-Muller")
    report("ddimxw_multistep_update order 2 row, z from a buffer", fused(row[5], row[6], 0.0, None, nz), m_b + 5 * c_b, "+ the noise read")
    report("ddimxw_multistep_update order 3 row", fused(0.0, row[6], row[7], hist, None), m_b + 6 * c_b, "+ hist read and written")
    report("ddimxw_blend", lambda: _lib.check(lib.ddimxw_blend(P(eps), P(beps), P(jf), P(cn), P(wt), *geom, _lib.stream())), m_b + c_b,
           "eps read, the canvas-shaped blend written")
    return out


def time_long(m, reps=3):
    """Whole runs on one canvas of L = 8192: wall ms, synchronised, of 20 logsnr_seq steps at order 2 and of 200 uniform DDIM steps."""
    alphas = make_schedule(m._full_config.diffusion)[1]
    x = torch.randn((1, 2, 8192, F), device="cuda")
    runs = {"solver_o2_20_logsnr_steps": lambda: D.windowed_solver_steps(x.clone(), logsnr_seq(alphas, 20), m, alphas, [-1], window=T, hop=H,
                                                                         order=2),
            "windowed_ddim_200_uniform_steps": lambda: D.windowed_steps(x.clone(), make_seq(1000, 200), m, alphas, [-1], window=T, hop=H)}
    res = {k: [] for k in runs}
    for r in range(reps + 1):  # one warm-up run of each
        for name in timing.leg_order(runs, r):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runs[name]()
            torch.cuda.synchronize()
            if r:
                res[name].append((time.perf_counter() - t0) * 1e3)
    out = {k: {"wall_ms": statistics.median(v), "spread_ms": max(v) - min(v)} for k, v in res.items()}
    return {"what": "wall ms of a whole run, one canvas of L = 8192 as 15 windows of 1024", "dtype": "bf16", "reps": reps, **out,
            "ddim_200_over_solver_20": out["windowed_ddim_200_uniform_steps"]["wall_ms"] / out["solver_o2_20_logsnr_steps"]["wall_ms"]}


def main(argv=None):
    a = timing.parse_args(argv, {"rounds": 5, "cases": [(1, 8), (1, 32)]}, flags=("long",))
    torch.manual_seed(0)
    m = timing.audio_model()
    for n, w in a.cases:
        for rec in time_kernels(n, w):
            print(json.dumps(rec), flush=True)
        if a.rounds > 0:
            print(json.dumps(time_case(m, n, w, a.rounds)), flush=True)
    if a.long:
        print(json.dumps(time_long(m)), flush=True)


if __name__ == "__main__":
    main()
