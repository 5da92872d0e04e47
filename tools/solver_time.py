"""Multistep sampler timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Times ms per replayed sampler step of three steppers over the same 20-entry log-SNR schedule, in one process:
  generalized -- DDIMStepper (generalized_steps, eta = 0), the first-order step;
  order2      -- MultistepStepper, DPM-Solver++ order 2 (one more read pass over the sample);
  order3      -- MultistepStepper, order 3 (two more read passes, one more write pass).
Every round times each of them once; the order within a round alternates (forwards, then backwards) so that no leg always runs
first or always runs behind the same neighbour.  Then each update kernel alone (back-to-back launches between two events), with the
bytes it must move over its time as a share of the HBM peak.
usage: python tools/solver_time.py [T=1024] [rounds=6] [B ...=8]   (rounds = 0: the kernels alone)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, dpm_coefficients, logsnr_seq, make_schedule  # noqa: E402
from ddim_audio_amd.solver import MultistepStepper  # noqa: E402


def time_steps(m, b, t_len, rounds):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    xts = {k: x_init.clone() for k in ("generalized", "order2", "order3")}
    with torch.no_grad():
        steppers = {"generalized": DDIMStepper(m, xts["generalized"], ddim_coefficients(seq, alphas, 0.0)),
                    "order2": MultistepStepper(m, xts["order2"], dpm_coefficients(seq, alphas, 2), 2),
                    "order3": MultistepStepper(m, xts["order3"], dpm_coefficients(seq, alphas, 3), 3)}
    return timing.time_legs({k: timing.stepper_leg(st, xts[k], x_init, len(seq) - 1) for k, st in steppers.items()}, rounds)[0]


def time_kernels(b, t_len):
    lib = _lib.load()
    xt, eps, x0, hist = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(4))
    # rows: first order (w = 0), second, third; the counter selects one.  w small enough that xt stays finite over the launches
    coef = torch.tensor([[500.0, 0.6, 0.8, 0.6, 0.4, 0.0, 0.0, 0.0], [500.0, 0.6, 0.8, 0.6, 0.4, 0.0, 0.1, 0.0],
                         [500.0, 0.6, 0.8, 0.6, 0.4, 0.0, 0.1, -0.05]], device="cuda")
    P, n, nbytes = _lib.ptr, xt.numel(), xt.numel() * 4
    out = []

    def report(name, fn, passes):
        out.append(timing.bandwidth_record(name, timing.time_launches(fn, reps=20, warm=3), passes, nbytes, B=b, T=t_len))

    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    coef6 = coef[:, :6].contiguous()
    # x_t, eps read; x0, x_t written
    report("ddimx_ddim_update (for comparison)",
           lambda: _lib.check(lib.ddimx_ddim_update(P(xt), P(eps), None, P(x0), P(coef6), P(ctr), n, _lib.stream())), 4)
    for row, h, name, passes in ((0, None, "ddimx_multistep_update order 1 row", 4), (1, None, "ddimx_multistep_update order 2", 5),
                                 (2, hist, "ddimx_multistep_update order 3", 7)):
        ctr.fill_(row)
        xt.normal_()
        # + x0 read (order 2); + hist read and written (order 3)
        report(name, lambda h=h: _lib.check(lib.ddimx_multistep_update(P(xt), P(eps), P(x0), P(h), P(coef), P(ctr), n, _lib.stream())),
               passes)
    return out


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 6, "B": [8]})
    torch.manual_seed(0)
    m = timing.audio_model()
    for b in a.B if a.rounds > 0 else []:
        r = time_steps(m, b, a.T, a.rounds)
        for k in ("order2", "order3"):
            r[k + "_over_generalized"] = r[k]["ms_per_step"] / r["generalized"]["ms_per_step"]
        print(json.dumps({"what": "ms per replayed sampler step", "B": b, "T": a.T, "dtype": "bf16", "steps": 20, "rounds": a.rounds,
                          **r}), flush=True)
    for b in a.B:
        for rec in time_kernels(b, a.T):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
