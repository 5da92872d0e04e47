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
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib, configs, synth  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, logsnr_seq, make_schedule, window_plan  # noqa: E402
from ddim_audio_amd.window import WindowStepper  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec
T, H, F = 1024, 512, 256
N_TIMED = 10


def _model():
    cfg = configs.dict2namespace(configs.audio_dict("torch.cuda.BFloat16Tensor"))
    m = D.Model(cfg)
    synth.fill_module(m, 0)
    return m.eval()


def time_legs(legs, rounds):
    """legs: {name: (stepper, xt, x_init)}; median ms per replayed step and the spread over the rounds."""
    names = tuple(legs)
    res = {k: [] for k in names}
    try:
        for r in range(rounds + 2):  # two warm-up rounds (the first also captures the graphs)
            for name in (names if r % 2 == 0 else names[::-1]):
                st, xt, x_init = legs[name]
                xt.copy_(x_init)
                st.rewind()
                with torch.no_grad():
                    st.step()  # row 0 (the eager step in the first round)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(N_TIMED):
                        st.step()
                    e1.record()
                torch.cuda.synchronize()
                if r >= 2:
                    res[name].append(e0.elapsed_time(e1) / N_TIMED)
        assert all(st.captures == 1 for st, _, _ in legs.values())
    finally:
        for st, _, _ in legs.values():
            st.close()
    return {k: {"ms_per_step": statistics.median(v), "spread_ms": max(v) - min(v)} for k, v in res.items()}


def time_case(m, n, w, rounds):
    length = T + (w - 1) * H
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    coef = ddim_coefficients(seq, alphas, 0.0)
    xb, xc = torch.randn((n * w, 2, T, F), device="cuda"), torch.randn((n, 2, length, F), device="cuda")
    xtb, xtc = xb.clone(), xc.clone()
    with torch.no_grad():
        legs = {"generalized": (DDIMStepper(m, xtb, coef), xtb, xb), "windowed": (WindowStepper(m, xtc, coef, T, H, "tri"), xtc, xc)}
    r = time_legs(legs, rounds)
    a, b = r["generalized"]["ms_per_step"], r["windowed"]["ms_per_step"]
    m_el, c_el = xb.numel(), xc.numel()
    extra = (3 * c_el - m_el) * 4
    allowed_ms = 2.0 * (extra / (0.65 * HBM_PEAK) + 4e-6) * 1e3
    return {"what": "ms per sampler step", "N": n, "W": w, "windows": n * w, "T": T, "H": H, "L": length, "dtype": "bf16", "rounds": rounds,
            **r, "windowed_minus_generalized_ms": b - a, "extra_bytes": extra, "allowed_ms": allowed_ms, "within_allowed": b - a <= allowed_ms}


def time_long(rounds):
    """One canvas of L = 8192: W = 15 windows of 1024 against the native B = 1 x T = 8192 step."""
    mw, mn = _model(), _model()
    alphas = make_schedule(mw._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    coef = ddim_coefficients(seq, alphas, 0.0)
    x = torch.randn((1, 2, 8192, F), device="cuda")
    xa, xb = x.clone(), x.clone()
    with torch.no_grad():
        legs = {"native_T8192": (DDIMStepper(mn, xa, coef), xa, x), "windowed_15x1024": (WindowStepper(mw, xb, coef, T, H, "tri"), xb, x)}
    r = time_legs(legs, rounds)
    return {"what": "ms per sampler step, one canvas of L = 8192 (orientation only)", "dtype": "bf16", "rounds": rounds, **r,
            "rows_evaluated_ratio": 15 * T / 8192, "windowed_over_native": r["windowed_15x1024"]["ms_per_step"] / r["native_T8192"]["ms_per_step"]}


def _events(fn, reps):
    """ms per call of ``fn``: ``reps`` calls captured into one graph, the replay timed (tools/noise_time.py)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    for _ in range(3):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    del g
    torch.cuda.synchronize()
    return ms


def time_kernels(n, w, reps=50):
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

    def report(name, ms, nbytes, note):
        out.append({"what": name, "N": n, "W": w, "us": ms * 1e3, "bytes": nbytes, "TB_per_s": nbytes / ms / 1e9,
                    "frac_of_8TBps": nbytes / HBM_PEAK / (ms * 1e-3), "note": note})

    gather = lambda: _lib.check(lib.ddimx_window_gather(P(canvas), P(win), *geom, _lib.stream()))  # noqa: E731

    def update(noise=None):
        _lib.check(lib.ddimx_window_update(P(canvas), P(eps), P(noise), P(x0), P(jf), P(cn), P(wt), P(coef), P(ctr), *geom, _lib.stream()))

    report("ddimx_window_gather", _events(gather, reps), 2 * m_b, "window batch read from the canvas and written once")
    canvas.normal_()
    report("ddimx_window_update", _events(update, reps), m_b + 3 * c_b, "eps read; canvas read and written, x0 written")
    canvas.normal_()
    report("ddimx_window_update with noise", _events(lambda: update(nz), reps), m_b + 4 * c_b, "+ the canvas-shaped noise read")
    canvas.normal_()
    report("gather + update back to back", _events(lambda: (gather(), update()), reps), 3 * m_b + 3 * c_b, "the pair a step adds")
    xt, e2, p0 = (torch.randn((n * w, 2, T, F), device="cuda") for _ in range(3))
    ms = _events(lambda: _lib.check(lib.ddimx_ddim_update(P(xt), P(e2), None, P(p0), P(coef), P(ctr), xt.numel(), _lib.stream())), reps)
    report("ddimx_ddim_update at batch N W", ms, 4 * m_b, "what the pair replaces in the step")
    return out


def main():
    args = sys.argv[1:]
    rounds = int(args.pop(0)) if args and args[0].isdigit() else 5
    long_leg = "long" in args
    cases = [tuple(int(v) for v in a.split("x")) for a in args if a != "long"] or [(1, 8), (4, 8)]
    torch.manual_seed(0)
    m = _model()
    for n, w in cases:
        for rec in time_kernels(n, w):
            print(json.dumps(rec), flush=True)
        if rounds > 0:
            print(json.dumps(time_case(m, n, w, rounds)), flush=True)
    if long_leg and rounds > 0:
        del m
        print(json.dumps(time_long(rounds)), flush=True)


if __name__ == "__main__":
    main()
