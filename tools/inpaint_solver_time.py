"""Multistep inpainting timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Times ms per replayed sampler step of five steppers over the same 20-entry log-SNR schedule, in one process:
  inpaint_guided -- InpaintStepper, guided + replacement (inpaint_steps' step: the first-order yardstick);
  solver_order2  -- MultistepStepper, DPM-Solver++ order 2 (dpm_solver_steps' step: the unmasked yardstick);
  guided_order2  -- InpaintSolverStepper, guided + replacement, order 2 (ddimxi_residual, ddimxi_multistep_update, h1);
  guided_order3  -- the same at order 3 (h1 and h2);
  replace_order2 -- InpaintSolverStepper, replacement only, order 2.
Every round times each of them once; the order within a round alternates (forwards, then backwards) so that no leg always runs
first or always runs behind the same neighbour.  Then ddimxi_multistep_update alone (back-to-back launches between two events),
with the bytes it must move over its time as a share of the HBM peak, beside ddimx_inpaint_update; then the wall time of 20
log-SNR guided steps at order 2 against 200 uniform guided inpaint_steps steps, through the public functions.
With ``unchanged``: only inpaint_guided and solver_order2 -- the steps that existed before -- so no ddimxi_ function is touched and
the same file can time a library built from the commit before (``DDIMX_LIB``): one process per library, alternated by the caller.
usage: python tools/inpaint_solver_time.py [T=1024] [rounds=5] [unchanged] [B ...=8]   (rounds = 0: the kernels alone)
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
from ddim_audio_amd.inpaint import InpaintStepper  # noqa: E402
from ddim_audio_amd.schedule import dpm_coefficients, inpaint_coefficients, logsnr_seq, make_schedule, make_seq  # noqa: E402
from ddim_audio_amd.solver import MultistepStepper  # noqa: E402

RHO = 0.3


def _known(b, t_len):
    shape = (b, 2, t_len, 256)
    mk = torch.ones(b, 1, t_len, 1, device="cuda")
    mk[:, :, t_len // 4: t_len // 2] = 0
    mk = mk.expand(shape).contiguous()
    return (torch.randn(shape, device="cuda") * mk).contiguous(), mk


def time_steps(m, b, t_len, rounds, unchanged):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    y, mk = _known(b, t_len)
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    names = ("inpaint_guided", "solver_order2") + (() if unchanged else ("guided_order2", "guided_order3", "replace_order2"))
    xts = {k: x_init.clone() for k in names}
    with torch.no_grad():
        steppers = {"inpaint_guided": InpaintStepper(m, xts["inpaint_guided"], y, mk, inpaint_coefficients(seq, alphas, 0.0, RHO), True, True),
                    "solver_order2": MultistepStepper(m, xts["solver_order2"], dpm_coefficients(seq, alphas, 2), 2)}
        if not unchanged:
            from ddim_audio_amd.inpaint_solver import InpaintSolverStepper
            from ddim_audio_amd.schedule import inpaint_solver_coefficients
            for k, order, rho in (("guided_order2", 2, RHO), ("guided_order3", 3, RHO), ("replace_order2", 2, 0.0)):
                steppers[k] = InpaintSolverStepper(m, xts[k], y, mk, inpaint_solver_coefficients(seq, alphas, order, 0.0, rho), order,
                                                   rho != 0, True)
    # a guided stepper's first step allocates the model's backward packing, so graphs captured before it are captured twice: the
    # count is not asserted, what is reported is that none was captured inside the timed rounds
    res, counts = timing.time_legs({k: timing.stepper_leg(steppers[k], xts[k], x_init, len(seq) - 1) for k in names}, rounds,
                                   expect_captures=None)
    return {k: {**v, "captures_while_timed": counts[k]["captures_while_timed"]} for k, v in res.items()}


def time_kernels(b, t_len):
    lib = _lib.load()
    shape, per = (b, 2, t_len, 256), 2 * t_len * 256
    xt, eps, y, mk, dx, x0, h1, h2 = (torch.randn(shape, device="cuda") for _ in range(8))
    mk = (mk > 0).float()
    seed = torch.empty_like(xt)
    part = torch.empty(int(lib.ddimx_inpaint_partials_floats(b, per)), device="cuda")
    # rows: order 1, 2, 3; the coefficients contract so that xt stays finite over the launches
    base = [500.0, 0.6, 0.8, 0.6, 0.3, 0.0, -1.5, 2.5, RHO, 0.5, 0.2]
    coef = torch.tensor([base + [0.0, 0.0], base + [0.1, 0.0], base + [0.1, -0.05]], device="cuda")
    coef9 = coef[:, :9].contiguous()
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    P, n = _lib.ptr, xt.numel() * 4
    out = []

    def residual():
        _lib.check(lib.ddimxi_residual(P(xt), P(eps), P(y), P(mk), P(x0), P(seed), P(part), P(coef), P(ctr), b, per, _lib.stream()))

    def new(flags, h):
        _lib.check(lib.ddimxi_multistep_update(P(xt), P(eps), None, P(x0), P(h1), P(h), P(y), P(mk), P(dx), P(part), P(coef), P(ctr), b, per,
                                               flags, 0, 0, 0, _lib.stream()))

    def old(flags):
        _lib.check(lib.ddimx_inpaint_update(P(xt), P(eps), None, P(x0), P(y), P(mk), P(dx), P(part), P(coef9), P(ctr), b, per, flags,
                                            _lib.stream()))

    # passes (sample-sized reads + writes).  guided + replace: x_t, eps, x0, y, m, d_x read, x_t, h1 written (8); + h1 read at
    # order 2 (9); + h2 read and written at order 3 (11).  replace only at order 2: x_t, eps, y, m, h1 read, x0, h1, x_t written (8)
    legs = [(0, lambda: old(3), "ddimx_inpaint_update guided+replace (for comparison)", 6),
            (0, lambda: new(3, None), "ddimxi_multistep_update guided+replace, order-1 row", 8),
            (1, lambda: new(3, None), "ddimxi_multistep_update guided+replace, order 2 (h1)", 9),
            (2, lambda: new(3, h2), "ddimxi_multistep_update guided+replace, order 3 (h1, h2)", 11),
            (1, lambda: new(1, None), "ddimxi_multistep_update replace only, order 2 (h1)", 8),
            (0, residual, "ddimxi_residual", 6)]
    for rnd in range(2):  # every leg twice, the second time in reverse order
        for row, fn, name, passes in timing.leg_order(legs, rnd):
            ctr.fill_(row)
            xt.normal_()
            residual()  # a norm for the weight
            out.append(timing.bandwidth_record(name, timing.time_launches(fn, reps=20, warm=3), passes, n, B=b, T=t_len))
    return out


def time_wall(m, b, t_len, reps=2):
    """20 log-SNR guided steps at order 2 against 200 uniform guided inpaint_steps steps: wall ms of the public calls."""
    alphas = make_schedule(m._full_config.diffusion)[1]
    y, mk = _known(b, t_len)
    x = torch.randn((b, 2, t_len, 256), device="cuda")
    runs = {"inpaint_solver_steps 20 x order 2": lambda: D.inpaint_solver_steps(x.clone(), logsnr_seq(alphas, 20), m, alphas, [-1], y=y, mask=mk,
                                                                                guidance=RHO, order=2),
            "inpaint_steps 200": lambda: D.inpaint_steps(x.clone(), make_seq(1000, 200), m, alphas, [-1], y=y, mask=mk, guidance=RHO)}
    res = {k: [] for k in runs}
    for r in range(reps + 1):  # one warm-up
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                res[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"ms": statistics.median(v), "spread_ms": max(v) - min(v)} for k, v in res.items()}


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 5, "B": [8]}, flags=("unchanged",))
    torch.manual_seed(0)
    m = timing.audio_model()
    for b in a.B if a.rounds > 0 else []:
        r = time_steps(m, b, a.T, a.rounds, a.unchanged)
        print(json.dumps({"what": "ms per replayed sampler step", "lib": os.path.basename(_lib.LIB_PATH), "B": b, "T": a.T, "dtype": "bf16",
                          "steps": 20, "rounds": a.rounds, **r}), flush=True)
    if a.unchanged:
        return
    for b in a.B:
        for rec in time_kernels(b, a.T):
            print(json.dumps(rec), flush=True)
        if a.rounds > 0:
            print(json.dumps({"what": "wall ms, guided inpainting", "B": b, "T": a.T, **time_wall(m, b, a.T)}), flush=True)


if __name__ == "__main__":
    main()
