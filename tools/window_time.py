"""Windowed sampler timing on one MI355X: the audio config (bf16 activations), windows of T = 1024 at hop 512, HIP events after
warm-up.

For every (N canvases, W windows per canvas) case, in one process, ms per replayed sampler step over the same 20-entry log-SNR
schedule (tools/solver_time.py's) of
  generalized -- DDIMStepper (generalized_steps, eta = 0) at batch N W: what existed before, the yardstick;
  windowed    -- WindowStepper over the same number of windows (canvas [N, 2, T + (W - 1) H, 256]).
Every round times each of them once, 10 replayed steps between two events; the order within a round alternates so that no leg always
runs first.  The difference is judged against what the two new kernels must move: with M window-batch elements and C canvas
elements ddim_update moves 4 M floats, the windowed step 2 M (gather) + M + 3 C (update), i.e. 3 C - M more, plus one kernel
boundary of about 4 us; accepted is twice [extra bytes / (0.65 x 8 TB/s) + 4 us].  Then the two kernels alone, back to back (50 pairs
captured into one graph, the replay between two events): us per pair and the bytes they move as a share of the 8 TB/s HBM peak.
With ``long``: one canvas of L = 8192 as W = 15 windows against the native B = 1 x T = 8192 step (a second model instance, so
that neither leg's graph goes stale when the other changes the tables' length) -- for orientation, not a pass criterion.
usage: python tools/window_time.py [rounds=5] [long] [NxW ...=1x8 4x8]   (rounds = 0: the kernels alone)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, logsnr_seq, make_schedule, window_plan  # noqa: E402
from ddim_audio_amd.window import WindowStepper  # noqa: E402

T, H, F = 1024, 512, 256
N_TIMED = 10


def time_case(m, n, w, rounds):
    length = T + (w - 1) * H
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    coef = ddim_coefficients(seq, alphas, 0.0)
    xb, xc = torch.randn((n * w, 2, T, F), device="cuda"), torch.randn((n, 2, length, F), device="cuda")
    xtb, xtc = xb.clone(), xc.clone()
    with torch.no_grad():
        legs = {"generalized": timing.stepper_leg(DDIMStepper(m, xtb, coef), xtb, xb, N_TIMED),
                "windowed": timing.stepper_leg(WindowStepper(m, xtc, coef, T, H, "tri"), xtc, xc, N_TIMED)}
    r, _ = timing.time_legs(legs, rounds)
    a, b = r["generalized"]["ms_per_step"], r["windowed"]["ms_per_step"]
    m_el, c_el = xb.numel(), xc.numel()
    extra = (3 * c_el - m_el) * 4
    allowed_ms = 2.0 * (extra / (0.65 * timing.HBM_PEAK) + 4e-6) * 1e3
    return {"what": "ms per sampler step", "N": n, "W": w, "windows": n * w, "T": T, "H": H, "L": length, "dtype": "bf16", "rounds": rounds,
            **r, "windowed_minus_generalized_ms": b - a, "extra_bytes": extra, "allowed_ms": allowed_ms, "within_allowed": b - a <= allowed_ms}


def time_long(rounds):
    """One canvas of L = 8192: W = 15 windows of 1024 against the native B = 1 x T = 8192 step."""
    mw, mn = timing.audio_model(), timing.audio_model()
    alphas = make_schedule(mw._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    coef = ddim_coefficients(seq, alphas, 0.0)
    x = torch.randn((1, 2, 8192, F), device="cuda")
    xa, xb = x.clone(), x.clone()
    with torch.no_grad():
        legs = {"native_T8192": timing.stepper_leg(DDIMStepper(mn, xa, coef), xa, x, N_TIMED),
                "windowed_15x1024": timing.stepper_leg(WindowStepper(mw, xb, coef, T, H, "tri"), xb, x, N_TIMED)}
    r, _ = timing.time_legs(legs, rounds)
    return {"what": "ms per sampler step, one canvas of L = 8192 (orientation only)", "dtype": "bf16", "rounds": rounds, **r,
            "rows_evaluated_ratio": 15 * T / 8192, "windowed_over_native": r["windowed_15x1024"]["ms_per_step"] / r["native_T8192"]["ms_per_step"]}


def time_kernels(n, w):
    lib, P = _lib.load(), _lib.ptr
    length = T + (w - 1) * H
    canvas, x0, nz = (torch.randn((n, 2, length, F), device="cuda") for _ in range(3))
    win, eps = (torch.randn((n * w, 2, T, F), device="cuda") for _ in range(2))
    p = window_plan(length, T, H, "tri")
    jf, cn, wt = (torch.from_numpy(v.copy()).cuda() for v in (p.jfirst, p.cnt, p.wt))
    coef = torch.tensor([[500.0, 0.6, 0.8, 0.6, 0.4, 0.1]], device="cuda")
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    geom = (n, w, 2, length, T, H, F)
    m_b, c_b = win.numel() * 4, canvas.numel() * 4
    out = []

    def report(name, fn, nbytes, note):
        ms = timing.time_graph_replay(fn, reps=50, warm=3)
        out.append({**timing.bandwidth_record(name, ms, 1, nbytes, unit="us", N=n, W=w), "note": note})

    gather = lambda: _lib.check(lib.ddimx_window_gather(P(canvas), P(win), *geom, _lib.stream()))  # noqa: E731

    def update(noise=None):
        _lib.check(lib.ddimx_window_update(P(canvas), P(eps), P(noise), P(x0), P(jf), P(cn), P(wt), P(coef), P(ctr), *geom, _lib.stream()))

    report("ddimx_window_gather", gather, 2 * m_b, "window batch read from the canvas and written once")
    canvas.normal_()
    report("ddimx_window_update", update, m_b + 3 * c_b, "eps read; canvas read and written, x0 written")
    canvas.normal_()
    report("ddimx_window_update with noise", lambda: update(nz), m_b + 4 * c_b, "+ the canvas-shaped noise read")
    canvas.normal_()
    report("gather + update back to back", lambda: (gather(), update()), 3 * m_b + 3 * c_b, "the pair a step adds")
    xt, e2, p0 = (torch.randn((n * w, 2, T, F), device="cuda") for _ in range(3))
    report("ddimx_ddim_update at batch N W",
           lambda: _lib.check(lib.ddimx_ddim_update(P(xt), P(e2), None, P(p0), P(coef), P(ctr), xt.numel(), _lib.stream())), 4 * m_b,
           "what the pair replaces in the step")
    return out


def main(argv=None):
    a = timing.parse_args(argv, {"rounds": 5, "cases": [(1, 8), (4, 8)]}, flags=("long",))
    torch.manual_seed(0)
    m = timing.audio_model()
    for n, w in a.cases:
        for rec in time_kernels(n, w):
            print(json.dumps(rec), flush=True)
        if a.rounds > 0:
            print(json.dumps(time_case(m, n, w, a.rounds)), flush=True)
    if a.long and a.rounds > 0:
        del m
        print(json.dumps(time_long(a.rounds)), flush=True)


if __name__ == "__main__":
    main()
