"""Brownian-path timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Times ms per replayed sampler step of four steppers over the same 20-entry log-SNR schedule, in one process:
  order2_tau0        -- MultistepStepper, DPM-Solver++ order 2, deterministic (ddimx_multistep_update);
  order2_tau1_stream -- the same at tau = 1 with a NoiseStream (ddimxs_multistep_update: one draw per group of four);
  order2_tau1_path   -- the same with a BrownianStream (ddimxb_multistep_update: the two descents of the step's plan row);
  order3_tau1_path   -- order 3 on the path.
Every round times each of them once; the order within a round alternates (forwards, then backwards) so that no leg always runs
first or always runs behind the same neighbour.  Then the update kernels and the path fill alone (back-to-back launches between
two events), with the draws a group of four costs on the row that is timed.
usage: python tools/brownian_time.py [T=1024] [rounds=6] [B ...=8]   (rounds = 0: the kernels alone)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.schedule import brownian_plan, dpm_coefficients, logsnr_seq, make_schedule  # noqa: E402
from ddim_audio_amd.solver import MultistepStepper  # noqa: E402

SEED = 0x5EED


def time_steps(m, b, t_len, rounds):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    names = ("order2_tau0", "order2_tau1_stream", "order2_tau1_path", "order3_tau1_path")
    xts = {k: x_init.clone() for k in names}
    ns, bs, plan = D.NoiseStream(SEED), D.BrownianStream(SEED), brownian_plan(seq, alphas, 1.0)
    with torch.no_grad():
        steppers = {"order2_tau0": MultistepStepper(m, xts["order2_tau0"], dpm_coefficients(seq, alphas, 2), 2),
                    "order2_tau1_stream": MultistepStepper(m, xts["order2_tau1_stream"], dpm_coefficients(seq, alphas, 2, tau=1.0), 2,
                                                           noise=ns),
                    "order2_tau1_path": MultistepStepper(m, xts["order2_tau1_path"], dpm_coefficients(seq, alphas, 2, tau=1.0), 2,
                                                         noise=bs, plan=plan),
                    "order3_tau1_path": MultistepStepper(m, xts["order3_tau1_path"], dpm_coefficients(seq, alphas, 3, tau=1.0), 3,
                                                         noise=bs, plan=plan)}
    res, _ = timing.time_legs({k: timing.stepper_leg(steppers[k], xts[k], x_init, len(seq) - 1) for k in names}, rounds)
    assert all(st.noise_buf is None for st in steppers.values())
    draws = [int(p[1] + p[2] - p[0]) for p in plan if p[2]]
    return {"draws_per_group_mean": sum(draws) / len(draws), "draws_per_group_max": max(draws), **res}


def time_kernels(m, b, t_len):
    lib = _lib.load()
    xt, eps, x0, out = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(4))
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    plan64 = brownian_plan(seq, alphas, 1.0)
    draws = [int(p[1] + p[2] - p[0]) for p in plan64]
    rows = {"most draws": max(range(len(draws)), key=draws.__getitem__), "fewest draws": min(range(len(draws) - 1), key=draws.__getitem__)}
    plan = torch.from_numpy(plan64).cuda()
    # contracting coefficients (s3 / s2 + c2 < 1 with eps ~ x), the same in every row, so that xt stays finite over the launches
    coef = torch.tensor([[500.0, 0.6, 0.8, 0.6, 0.3, 0.2, 0.1, 0.0]] * len(seq), device="cuda")
    P, per = _lib.ptr, xt[0].numel()
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = []

    def report(name, fn, n_draws):
        res.append({"what": name, "B": b, "T": t_len, "ms": timing.time_launches(fn, reps=20, warm=3), "draws_per_group": n_draws})

    def stream():
        _lib.check(lib.ddimxs_multistep_update(P(xt), P(eps), None, P(x0), None, P(coef), P(ctr), b, per, SEED, 0, 0, _lib.stream()))

    def path():
        _lib.check(lib.ddimxb_multistep_update(P(xt), P(eps), P(x0), None, P(coef), P(plan), P(ctr), b, per, SEED, 0, _lib.stream()))

    report("ddimxs_multistep_update order 2, drawn in the kernel", stream, 1)
    for name, k in rows.items():
        ctr.fill_(k)
        xt.normal_()
        report(f"ddimxb_multistep_update order 2, the row with the {name}", path, draws[k])
        row = plan[k].contiguous()
        for kind, label in ((_lib.DDIMXB_INCREMENT, "increment"), (_lib.DDIMXB_PATH, "path")):
            report(f"ddimxb_path_fill {label}, the row with the {name}",
                   lambda: _lib.check(lib.ddimxb_path_fill(P(out), b, per, SEED, 0, P(row), kind, _lib.stream())),
                   draws[k] if kind == _lib.DDIMXB_INCREMENT else int(plan64[k, 2]))
    return res


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 6, "B": [8]})
    torch.manual_seed(0)
    m = timing.audio_model()
    for b in a.B if a.rounds > 0 else []:
        r = time_steps(m, b, a.T, a.rounds)
        for k in ("order2_tau1_stream", "order2_tau1_path", "order3_tau1_path"):
            r[k + "_over_order2_tau0"] = r[k]["ms_per_step"] / r["order2_tau0"]["ms_per_step"]
        r["path_minus_stream_ms"] = r["order2_tau1_path"]["ms_per_step"] - r["order2_tau1_stream"]["ms_per_step"]
        print(json.dumps({"what": "ms per replayed sampler step", "B": b, "T": a.T, "dtype": "bf16", "steps": 20, "rounds": a.rounds,
                          **r}), flush=True)
    for b in a.B:
        for rec in time_kernels(m, b, a.T):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
