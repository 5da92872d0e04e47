"""UniC corrector timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Times ms per replayed sampler step of four steppers over the same 20-entry log-SNR schedule, in one process:
  order2      -- MultistepStepper, DPM-Solver++ order 2 (ddimx_multistep_update: the step without the corrector);
  order2_unic -- the same with the corrector folded in (ddimxu_multistep_update, one history tensor more);
  order3      -- order 3 without the corrector;
  order3_unic -- order 3 with it (two history tensors: hist and hist2).
Every round times each of them once; the order within a round alternates (forwards, then backwards) so that no leg always runs
first or always runs behind the same neighbour.  Then each update alone (back-to-back launches between two events), with the
bytes it must move over its time as a share of the HBM peak.
With ``unchanged``: only order2 and order3 -- the steps that existed before -- so no ddimxu_ function is touched and the same file
can time a library built from the commit before (``DDIMX_LIB``): one process per library, alternated by the caller.
usage: python tools/unic_time.py [T=1024] [rounds=6] [unchanged] [B ...=8]   (rounds = 0: the kernels alone)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.schedule import dpm_coefficients, logsnr_seq, make_schedule, unic_coefficients  # noqa: E402
from ddim_audio_amd.solver import MultistepStepper  # noqa: E402


def time_steps(m, b, t_len, rounds, unchanged):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    names = ("order2", "order3") if unchanged else ("order2", "order2_unic", "order3", "order3_unic")
    xts = {k: x_init.clone() for k in names}
    with torch.no_grad():
        steppers = {k: MultistepStepper(m, xts[k], (unic_coefficients if k.endswith("unic") else dpm_coefficients)(seq, alphas, int(k[5])),
                                        int(k[5])) for k in names}
    res, _ = timing.time_legs({k: timing.stepper_leg(steppers[k], xts[k], x_init, len(seq) - 1) for k in names}, rounds)
    if not unchanged:
        assert steppers["order2_unic"].hist is not None and steppers["order2_unic"].hist2 is None
        assert steppers["order3_unic"].hist2 is not None
    return res


def time_kernels(b, t_len, unchanged):
    lib = _lib.load()
    xt, eps, x0, hist, hist2 = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(5))
    # rows: order 1, 2 and 3 of the plain solver, then of the corrector; the counter selects one.  The coefficients contract
    # (s3 / s2 + c2 < 1 with eps ~ x) so that xt stays finite over the launches
    base = [500.0, 0.6, 0.8, 0.6, 0.3, 0.0]
    coef = torch.tensor([base + [0.0, 0.0, 0.0], base + [0.1, 0.0, 0.0], base + [0.1, -0.05, 0.0], base + [0.1, -0.05, 0.02]], device="cuda")
    coef8 = coef[:, :8].contiguous()
    P, n, nbytes = _lib.ptr, xt.numel(), xt.numel() * 4
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = []

    def plain(h):
        _lib.check(lib.ddimx_multistep_update(P(xt), P(eps), P(x0), P(h), P(coef8), P(ctr), n, _lib.stream()))

    def unic(h, h2):
        _lib.check(lib.ddimxu_multistep_update(P(xt), P(eps), P(x0), P(h), P(h2), P(coef), P(ctr), n, _lib.stream()))

    # passes: x_t, eps, x0 read and x0, x_t written (5); + hist read and written (7); + hist2 read and written (9)
    legs = [(1, lambda: plain(None), "ddimx_multistep_update order 2", 5), (2, lambda: plain(hist), "ddimx_multistep_update order 3", 7)]
    if not unchanged:
        legs += [(1, lambda: unic(None, None), "ddimxu_multistep_update order-2 row of the plain solver, no history buffer", 5),
                 (2, lambda: unic(hist, None), "ddimxu_multistep_update corrector at order 2 (hist)", 7),
                 (3, lambda: unic(hist, hist2), "ddimxu_multistep_update corrector at order 3 (hist, hist2)", 9)]
    for rnd in range(2):  # every leg twice, the second time in reverse order
        for row, fn, name, passes in timing.leg_order(legs, rnd):
            ctr.fill_(row)
            xt.normal_()
            out.append(timing.bandwidth_record(name, timing.time_launches(fn, reps=20, warm=3), passes, nbytes, B=b, T=t_len))
    return out


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 6, "B": [8]}, flags=("unchanged",))
    torch.manual_seed(0)
    m = timing.audio_model()
    for b in a.B if a.rounds > 0 else []:
        r = time_steps(m, b, a.T, a.rounds, a.unchanged)
        if not a.unchanged:
            for k in ("order2", "order3"):
                r[k + "_unic_over_" + k] = r[k + "_unic"]["ms_per_step"] / r[k]["ms_per_step"]
        print(json.dumps({"what": "ms per replayed sampler step", "lib": os.path.basename(_lib.LIB_PATH), "B": b, "T": a.T, "dtype": "bf16",
                          "steps": 20, "rounds": a.rounds, **r}), flush=True)
    for b in a.B:
        for rec in time_kernels(b, a.T, a.unchanged):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
