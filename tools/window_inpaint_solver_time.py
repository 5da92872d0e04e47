"""Windowed multistep inpainting timing on one MI355X: the audio config (bf16 activations), N W = 8 windows of T = 1024 at hop 512 on
one canvas of L = 4608, HIP events after warm-up (every round times each leg once, 10 replayed steps between two events, the order
within a round alternates, the spread of every leg over the rounds is reported).

In one process, ms per replayed sampler step over the same 20-entry log-SNR schedule of
  winp_guided        -- WindowInpaintStepper, guidance 0.3 (windowed_inpaint_steps' guided step): the yardstick of the guided step;
  wis_guided_order2  -- WindowInpaintSolverStepper, rho 0.3, order 2: gather, tape-keeping forward, ddimxwis_residual, data-only
                        backward, ddimxwis_multistep_update (h1);
  wis_guided_order3  -- the same at order 3 (h1 and h2);
  window_solver_o2   -- WindowSolverStepper, order 2 (windowed_solver_steps' step): the yardstick of the replacement-only step;
  wis_replace_order2 -- WindowInpaintSolverStepper, rho 0, order 2: gather, forward, one ddimxwis_multistep_update launch.
Then the kernels alone (50 calls captured into one graph, the replay between two events): us per call and the bytes they must move
as a share of the 8 TB/s HBM peak, ddimxwis_multistep_update beside ddimxwi_update and, at B = N W = 8 (as many network elements),
ddimxi_multistep_update.  With ``wall``: the wall time of 20 log-SNR guided steps at order 2 against 200 uniform guided
windowed_inpaint_steps steps, through the public functions (seconds of GPU time: left out unless asked for).
usage: python tools/window_inpaint_solver_time.py [rounds=5] [wall]   (rounds = 0: the kernels alone)
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
from ddim_audio_amd.schedule import (dpm_coefficients, inpaint_coefficients, inpaint_solver_coefficients, logsnr_seq, make_schedule,  # noqa: E402
                                     make_seq, window_plan)
from ddim_audio_amd.window import WindowSolverStepper  # noqa: E402
from ddim_audio_amd.window_inpaint import WindowInpaintStepper  # noqa: E402
from ddim_audio_amd.window_inpaint_solver import WindowInpaintSolverStepper  # noqa: E402

T, H, F = 1024, 512, 256
N_TIMED = 10
N, W = 1, 8
L = T + (W - 1) * H
RHO = 0.3


def _known(shape):
    """A packet-loss mask (a quarter of the rows missing) and the known content, canvas- or batch-shaped."""
    y = torch.randn(shape, device="cuda")
    mask = torch.ones(shape, device="cuda")
    mask[:, :, shape[2] // 4: shape[2] // 2] = 0
    return y * mask, mask


def time_case(m, rounds):
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    xc = torch.randn((N, 2, L, F), device="cuda")
    yc, mc = _known(xc.shape)
    names = ("winp_guided", "wis_guided_order2", "wis_guided_order3", "window_solver_o2", "wis_replace_order2")
    xs = {k: xc.clone() for k in names}
    geo = (T, H, "tri")
    with torch.no_grad():
        # the backward packing is allocated before any leg captures: allocating it later would make the graphs captured so far stale
        m.prepare(xc.device, T)
        m._ensure_packed_bwd(_lib.load(), xc.device)
        st = {"winp_guided": WindowInpaintStepper(m, xs["winp_guided"], yc, mc, inpaint_coefficients(seq, alphas, 0.0, RHO), True, True, *geo),
              "window_solver_o2": WindowSolverStepper(m, xs["window_solver_o2"], dpm_coefficients(seq, alphas, 2), 2, *geo)}
        for k, order, rho in (("wis_guided_order2", 2, RHO), ("wis_guided_order3", 3, RHO), ("wis_replace_order2", 2, 0.0)):
            st[k] = WindowInpaintSolverStepper(m, xs[k], yc, mc, inpaint_solver_coefficients(seq, alphas, order, 0.0, rho), order, rho != 0,
                                               True, *geo)
    r, counts = timing.time_legs({k: timing.stepper_leg(st[k], xs[k], xc, N_TIMED) for k in names}, rounds, expect_captures=None)
    r = {k: {**v, "captures_while_timed": counts[k]["captures_while_timed"]} for k, v in r.items()}
    ms = lambda k: r[k]["ms_per_step"]  # noqa: E731
    return {"what": "ms per replayed sampler step", "N": N, "W": W, "T": T, "H": H, "L": L, "dtype": "bf16", "steps": 20, "rounds": rounds,
            "lib": os.path.basename(_lib.LIB_PATH), **r,
            "wis_guided_order2_minus_winp_guided_ms": ms("wis_guided_order2") - ms("winp_guided"),
            "wis_guided_order3_minus_winp_guided_ms": ms("wis_guided_order3") - ms("winp_guided"),
            "wis_replace_order2_minus_window_solver_o2_ms": ms("wis_replace_order2") - ms("window_solver_o2")}


def time_kernels():
    lib, P = _lib.load(), _lib.ptr
    canvas, x0, beps, h1, h2 = (torch.randn((N, 2, L, F), device="cuda") for _ in range(5))
    y, mask = _known(canvas.shape)
    eps, seed, dwin = (torch.randn((N * W, 2, T, F), device="cuda") for _ in range(3))
    p = window_plan(L, T, H, "tri")
    jf, cn, wt = (torch.from_numpy(v.copy()).cuda() for v in (p.jfirst, p.cnt, p.wt))
    # rows: order 1, 2, 3; the coefficients contract so that x stays finite over the launches
    base = [500.0, 0.6, 0.8, 0.6, 0.3, 0.0, -1.5, 2.5, RHO, 0.5, 0.2]
    coef = torch.tensor([base + [0.0, 0.0], base + [0.1, 0.0], base + [0.1, -0.05]], device="cuda")
    coef9 = coef[:, :9].contiguous()
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    geom = (N, W, 2, L, T, H, F)
    parts = torch.zeros(int(lib.ddimxwi_partials_floats(N, canvas[0].numel())), device="cuda")
    m_b, c_b = eps.numel() * 4, canvas.numel() * 4
    out = []

    def report(name, row, fn, nbytes, note, **fields):
        ctr.fill_(row)
        canvas.normal_()
        residual()  # a norm for the weight
        ms = timing.time_graph_replay(fn, reps=50, warm=3)
        out.append({**timing.bandwidth_record(name, ms, 1, nbytes, unit="us", **(fields or dict(N=N, W=W))), "note": note})

    def residual():
        _lib.check(lib.ddimxwis_residual(P(canvas), P(eps), P(y), P(mask), P(x0), P(beps), P(seed), P(parts), P(jf), P(cn), P(wt), P(coef),
                                         P(ctr), *geom, _lib.stream()))

    def new(flags, e, h):
        return lambda: _lib.check(lib.ddimxwis_multistep_update(P(canvas), P(e), None, P(x0), P(h1), P(h), P(y), P(mask), P(dwin), P(parts), P(jf),
                                                                P(cn), P(wt), P(coef), P(ctr), *geom, flags, 0, 0, 0, _lib.stream()))

    def old(flags, e):
        return lambda: _lib.check(lib.ddimxwi_update(P(canvas), P(e), None, P(x0), P(y), P(mask), P(dwin), P(parts), P(jf), P(cn), P(wt),
                                                     P(coef9), P(ctr), *geom, flags, _lib.stream()))

    report("ddimxwis_residual", 0, residual, 2 * m_b + 5 * c_b, "eps read, seed written; x, y, mask read, x0 and the blend written")
    report("ddimxwi_update guided + replace (for comparison)", 0, old(3, beps), m_b + 6 * c_b, "d_win read; blend, x0, y, mask, x read; x written")
    report("ddimxwis_multistep_update guided + replace, order-1 row", 0, new(3, beps, None), m_b + 7 * c_b, "+ h1 written")
    report("ddimxwis_multistep_update guided + replace, order 2 (h1)", 1, new(3, beps, None), m_b + 8 * c_b, "+ h1 read")
    report("ddimxwis_multistep_update guided + replace, order 3 (h1, h2)", 2, new(3, beps, h2), m_b + 10 * c_b, "+ h2 read and written")
    report("ddimxwi_update replace only (for comparison)", 0, old(1, eps), m_b + 5 * c_b, "eps read; x, y, mask read; x0 and x written")
    report("ddimxwis_multistep_update replace only, order 2 (h1)", 1, new(1, eps, None), m_b + 7 * c_b, "+ h1 read and written")
    # the yardstick at B = N W, T: as many network elements
    xb, eb, db, x0b, h1b = (torch.randn((N * W, 2, T, F), device="cuda") for _ in range(5))
    yb, mb = _known(xb.shape)
    per = xb[0].numel()
    pb = torch.ones(int(lib.ddimx_inpaint_partials_floats(N * W, per)), device="cuda")
    report("ddimxi_multistep_update guided + replace, order 2 (h1), at batch N W", 1, lambda: _lib.check(lib.ddimxi_multistep_update(
        P(xb), P(eb), None, P(x0b), P(h1b), None, P(yb), P(mb), P(db), P(pb), P(coef), P(ctr), N * W, per, 3, 0, 0, 0, _lib.stream())), 9 * m_b,
        "x, eps, x0, y, mask, d_x, h1 read; x, h1 written", B=N * W, T=T)
    return out


def time_wall(m, reps=2):
    """20 log-SNR guided steps at order 2 against 200 uniform guided windowed_inpaint_steps steps: wall ms of the public calls."""
    alphas = make_schedule(m._full_config.diffusion)[1]
    x = torch.randn((N, 2, L, F), device="cuda")
    y, mk = _known(x.shape)
    kw = dict(window=T, hop=H, taper="tri", y=y, mask=mk, guidance=RHO)
    runs = {"windowed_inpaint_solver_steps 20 x order 2": lambda: D.windowed_inpaint_solver_steps(x.clone(), logsnr_seq(alphas, 20), m, alphas,
                                                                                                  [-1], order=2, **kw),
            "windowed_inpaint_steps 200": lambda: D.windowed_inpaint_steps(x.clone(), make_seq(1000, 200), m, alphas, [-1], **kw)}
    res = {k: [] for k in runs}
    for r in range(reps + 1):  # one warm-up
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                res[k].append((time.perf_counter() - t0) * 1e3)
    out = {k: {"ms": statistics.median(v), "spread_ms": max(v) - min(v)} for k, v in res.items()}
    return {**out, "ratio": out["windowed_inpaint_steps 200"]["ms"] / out["windowed_inpaint_solver_steps 20 x order 2"]["ms"]}


def main(argv=None):
    a = timing.parse_args(argv, {"rounds": 5}, flags=("wall",))
    timing.require_gpu()
    torch.manual_seed(0)
    for rec in time_kernels():
        print(json.dumps(rec), flush=True)
    if a.rounds > 0:
        m = timing.audio_model()
        print(json.dumps(time_case(m, a.rounds)), flush=True)
        if a.wall:
            print(json.dumps({"what": "wall ms, guided windowed inpainting", "N": N, "W": W, "T": T, "L": L, **time_wall(m)}), flush=True)


if __name__ == "__main__":
    main()
