"""DDIM-inversion timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Times ms per replayed step of three steppers, in one process:
  ddim_a, ddim_b -- DDIMStepper (generalized_steps, eta = 0) twice: the difference between the two legs of the same run is the
                    spread the inversion row has to be read against;
  invert         -- InvertStepper: one row of the inversion table (one network evaluation of one fixed-point iteration), over
                    the same grid upwards, iters = 2 (half the rows keep the base point, half read it).
Every round times each of them once; the order within a round alternates (forwards, then backwards) so that no leg always runs
first or always runs behind the same neighbour.  Then each update kernel alone (back-to-back launches between two events), with
the bytes it must move over its time as a share of the HBM peak, and ddimx_slerp at M = 11.
usage: python tools/invert_time.py [T=1024] [rounds=6] [B ...=8]   (rounds = 0: the kernels alone)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.invert import InvertStepper  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, invert_coefficients, make_schedule  # noqa: E402


def time_steps(m, b, t_len, rounds):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = list(range(0, 200, 20))  # 10 levels; a fine grid, on which the random-weight network's iteration stays bounded
    names = ("ddim_a", "invert", "ddim_b")
    xts = {k: x_init.clone() for k in names}
    ddim = ddim_coefficients(list(range(0, 400, 20)), alphas, 0.0)  # 20 rows, like the inversion's 10 levels x 2 iterations
    with torch.no_grad():
        steppers = {"ddim_a": DDIMStepper(m, xts["ddim_a"], ddim), "ddim_b": DDIMStepper(m, xts["ddim_b"], ddim),
                    "invert": InvertStepper(m, xts["invert"], invert_coefficients(seq, alphas, 2))}
    assert len({st.n_iter for st in steppers.values()}) == 1  # 20 rows each
    n_replayed = steppers["invert"].n_iter - 1
    return timing.time_legs({k: timing.stepper_leg(steppers[k], xts[k], x_init, n_replayed) for k in names}, rounds)[0]


def time_kernels(b, t_len):
    lib = _lib.load()
    xt, eps, x0, base = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(4))
    per = xt[0].numel()
    # rows: a level's first evaluation (base written), a later one (base read); p, q chosen so that xt stays finite over the launches
    coef = torch.tensor([[500.0, 0.6, 0.8, 0.9, 0.1, 1.0], [500.0, 0.6, 0.8, 0.9, 0.1, 0.0]], device="cuda")
    coef6 = torch.tensor([[500.0, 0.6, 0.8, 0.6, 0.4, 0.0]], device="cuda")
    log = torch.zeros((2, b), device="cuda")
    partials = torch.empty(int(lib.ddimx_invert_partials_doubles(b, per)), dtype=torch.float64, device="cuda")
    P, n, nbytes = _lib.ptr, xt.numel(), xt.numel() * 4
    out = []

    def report(name, fn, passes):
        out.append(timing.bandwidth_record(name, timing.time_launches(fn, reps=20, warm=3), passes, nbytes, B=b, T=t_len))

    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    # x_t, eps read; x0, x_t written
    report("ddimx_ddim_update (for comparison)",
           lambda: _lib.check(lib.ddimx_ddim_update(P(xt), P(eps), None, P(x0), P(coef6), P(ctr), n, _lib.stream())), 4)
    for row, name in ((0, "ddimx_invert_update, first row of a level"), (1, "ddimx_invert_update, later row")):
        ctr.fill_(row)
        xt.normal_()
        # + base written (first) or read (later); both launches of the call
        report(name, lambda: _lib.check(lib.ddimx_invert_update(P(xt), P(eps), P(base), P(x0), P(partials), P(log), 2, P(coef), P(ctr),
                                                                b, per, _lib.stream())), 5)
    if b >= 2:
        w = torch.linspace(0.0, 1.0, 11, device="cuda")
        pairs = b // 2
        z = torch.empty((pairs * 11, 2, t_len, 256), device="cuda")
        ms = timing.time_launches(lambda: _lib.check(lib.ddimx_slerp(P(xt), P(eps), P(w), 11, P(z), P(partials), pairs, per, _lib.stream())),
                                  reps=20, warm=3)
        out.append({"what": "ddimx_slerp, M = 11", "pairs": pairs, "T": t_len, "ms": ms, "bytes": (4 + 11) * pairs * per * 4,
                    "TB_per_s": (4 + 11) * pairs * per * 4 / ms / 1e9})  # z1, z2 read twice (sums, blend); M outputs written
    return out


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 6, "B": [8]})
    torch.manual_seed(0)
    m = timing.audio_model()
    for b in a.B if a.rounds > 0 else []:
        r = time_steps(m, b, a.T, a.rounds)
        r["ddim_legs_differ_by"] = abs(r["ddim_a"]["ms_per_step"] - r["ddim_b"]["ms_per_step"])
        r["invert_minus_ddim"] = r["invert"]["ms_per_step"] - 0.5 * (r["ddim_a"]["ms_per_step"] + r["ddim_b"]["ms_per_step"])
        print(json.dumps({"what": "ms per replayed step", "B": b, "T": a.T, "dtype": "bf16", "rows": 20, "rounds": a.rounds, **r}),
              flush=True)
    for b in a.B:
        for rec in time_kernels(b, a.T):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
