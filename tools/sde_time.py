"""SDE-DPM-Solver++ timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Times ms per replayed sampler step of four steppers over the same 20-entry log-SNR schedule, in one process:
  order2_tau0 -- MultistepStepper, DPM-Solver++ order 2, deterministic (ddimx_multistep_update: what the step was before tau);
  order2_tau1 -- the same at tau = 1 (ddimxs_multistep_update: the noise drawn inside the update kernel);
  order3_tau1 -- order 3 at tau = 1;
  ddim_eta1   -- DDIMStepper, generalized_steps(eta = 1, noise = NoiseStream): a fill launch, then ddimx_ddim_update reads the buffer.
Every round times each of them once; the order within a round alternates (forwards, then backwards) so that no leg always runs
first or always runs behind the same neighbour.  Then each update alone (back-to-back launches between two events), with the
bytes it must move over its time as a share of the HBM peak.
usage: python tools/sde_time.py [T=1024] [rounds=6] [B ...=8]   (rounds = 0: the kernels alone)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, dpm_coefficients, logsnr_seq, make_schedule  # noqa: E402
from ddim_audio_amd.solver import MultistepStepper  # noqa: E402

SEED = 0x5EED


def time_steps(m, b, t_len, rounds):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    names = ("order2_tau0", "order2_tau1", "order3_tau1", "ddim_eta1")
    xts = {k: x_init.clone() for k in names}
    ns = D.NoiseStream(SEED)
    with torch.no_grad():
        steppers = {"order2_tau0": MultistepStepper(m, xts["order2_tau0"], dpm_coefficients(seq, alphas, 2), 2),
                    "order2_tau1": MultistepStepper(m, xts["order2_tau1"], dpm_coefficients(seq, alphas, 2, tau=1.0), 2, noise=ns),
                    "order3_tau1": MultistepStepper(m, xts["order3_tau1"], dpm_coefficients(seq, alphas, 3, tau=1.0), 3, noise=ns),
                    "ddim_eta1": DDIMStepper(m, xts["ddim_eta1"], ddim_coefficients(seq, alphas, 1.0), noise=ns)}
    res, _ = timing.time_legs({k: timing.stepper_leg(steppers[k], xts[k], x_init, len(seq) - 1) for k in names}, rounds)
    assert all(steppers[k].noise_buf is None for k in names[:3]) and steppers["ddim_eta1"].noise_buf is not None
    return res


def time_kernels(b, t_len):
    lib = _lib.load()
    xt, eps, x0, hist, zbuf = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(5))
    # rows: order 2 without noise, order 2 with, order 3 with, first order with; the counter selects one.  The coefficients contract
    # (s3 / s2 + c2 < 1 with eps ~ x) so that xt stays finite over the launches
    coef = torch.tensor([[500.0, 0.6, 0.8, 0.6, 0.3, 0.0, 0.1, 0.0], [500.0, 0.6, 0.8, 0.6, 0.3, 0.2, 0.1, 0.0],
                         [500.0, 0.6, 0.8, 0.6, 0.3, 0.2, 0.1, -0.05], [500.0, 0.6, 0.8, 0.6, 0.3, 0.2, 0.0, 0.0]], device="cuda")
    P, n, per, nbytes = _lib.ptr, xt.numel(), xt[0].numel(), xt.numel() * 4
    out = []

    def report(name, fn, passes):
        out.append(timing.bandwidth_record(name, timing.time_launches(fn, reps=20, warm=3), passes, nbytes, B=b, T=t_len))

    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    coef6 = coef[:, :6].contiguous()
    ns = D.NoiseStream(SEED)

    def sde(h, z):
        _lib.check(lib.ddimxs_multistep_update(P(xt), P(eps), P(z), P(x0), P(h), P(coef), P(ctr), b, per, SEED, 0, 0, _lib.stream()))

    # x_t, eps, x0 read; x0, x_t written
    report("ddimx_multistep_update order 2 (tau = 0)",
           lambda: _lib.check(lib.ddimx_multistep_update(P(xt), P(eps), P(x0), None, P(coef), P(ctr), n, _lib.stream())), 5)
    for row, h, z, name, passes in ((0, None, None, "ddimxs_multistep_update order 2, c1 = 0 row", 5),
                                    (1, None, None, "ddimxs_multistep_update order 2, drawn in the kernel", 5),
                                    (1, None, zbuf, "ddimxs_multistep_update order 2, noise buffer", 6),
                                    (2, hist, None, "ddimxs_multistep_update order 3, drawn in the kernel", 7)):
        ctr.fill_(row)
        xt.normal_()
        report(name, lambda h=h, z=z: sde(h, z), passes)
    ctr.fill_(3)
    xt.normal_()

    def ddim_eta1():
        ns.fill(zbuf, ctr)
        _lib.check(lib.ddimx_ddim_update(P(xt), P(eps), P(zbuf), P(x0), P(coef6), P(ctr), n, _lib.stream()))

    report("ddimx_noise_fill + ddimx_ddim_update (eta = 1)", ddim_eta1, 6)  # + the noise written, then read
    report("ddimxs_multistep_update first-order row, drawn in the kernel", lambda: sde(None, None), 4)
    return out


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 6, "B": [8]})
    torch.manual_seed(0)
    m = timing.audio_model()
    for b in a.B if a.rounds > 0 else []:
        r = time_steps(m, b, a.T, a.rounds)
        for k in ("order2_tau1", "order3_tau1", "ddim_eta1"):
            r[k + "_over_order2_tau0"] = r[k]["ms_per_step"] / r["order2_tau0"]["ms_per_step"]
        print(json.dumps({"what": "ms per replayed sampler step", "B": b, "T": a.T, "dtype": "bf16", "steps": 20, "rounds": a.rounds,
                          **r}), flush=True)
    for b in a.B:
        for rec in time_kernels(b, a.T):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
