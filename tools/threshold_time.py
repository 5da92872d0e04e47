"""x0 clip / dynamic threshold timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Times ms per replayed step of ``generalized_steps``' stepper (DDIMStepper, eta = 0) over the same 20-entry uniform schedule, in
one process, under the three settings of ``threshold=``:
  none    -- the frame as it is without one: timestep fill, forward, ddimx_ddim_update, counter advance;
  clip    -- X0Clip(1.0): one ddimxq_threshold_eps launch between the forward and the update;
  dynamic -- X0Threshold(0.995, 1.0): the four launches of ddimxq_x0_quantile in front of that one.
Every round times each leg once; the order within a round alternates so that no leg always runs first.  Then the two exports alone
(back-to-back calls between two events) on the eps and the x of a replayed run's first iteration, with the bytes they must move
over their time as a share of the HBM peak.
usage: python tools/threshold_time.py [T=1024] [rounds=8] [B=8] [legs=none,clip,dynamic]
(legs = none needs nothing of the feature but the keyword: the un-thresholded leg alone, for a same-box comparison with
tools/vpred_time.py's eps leg.)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper, _threshold  # noqa: E402
from ddim_audio_amd.schedule import (X0Clip, X0Threshold, ddim_coefficients, make_schedule, make_seq, threshold_rank,  # noqa: E402
                                     v_table)

RULES = {"none": None, "clip": X0Clip(1.0), "dynamic": X0Threshold(0.995, 1.0)}


def time_steps(m, b, t_len, rounds, legs):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = make_seq(1000, 20)
    coef = ddim_coefficients(seq, alphas, 0.0)
    xts = {k: x_init.clone() for k in legs}
    with torch.no_grad():
        steppers = {k: DDIMStepper(m, xts[k], coef, threshold=_threshold(RULES[k], alphas)) for k in legs}
    return timing.time_legs({k: timing.stepper_leg(steppers[k], xts[k], x_init, len(seq) - 1) for k in legs}, rounds)[0]


def time_kernels(m, b, t_len):
    """The two exports alone, on the (x, eps) the network makes of Gaussian x at t = 900: its own spread of |x0|."""
    lib = _lib.load()
    alphas = make_schedule(m._full_config.diffusion)[1]
    x = torch.randn((b, 2, t_len, 256), device="cuda")
    t = torch.full((b,), 900, dtype=torch.int64, device="cuda")
    with torch.no_grad():
        eps = m(x, t).float().contiguous().clone()
    out_e = torch.empty_like(eps)
    tab = torch.from_numpy(v_table(alphas).astype("float32")).cuda()
    work = torch.zeros(int(lib.ddimxq_quantile_work_bytes(b)), dtype=torch.uint8, device="cuda")
    scale = torch.zeros(b, 2, device="cuda")
    P, per, nbytes = _lib.ptr, x[0].numel(), x.numel() * 4
    rank = threshold_rank(0.995, per)
    out = []

    def report(name, fn, passes):
        out.append(timing.bandwidth_record(name, timing.time_launches(fn, reps=20, warm=3), passes, nbytes, B=b, T=t_len))

    # x, eps read by each of the three passes
    report("ddimxq_x0_quantile (4 launches)",
           lambda: _lib.check(lib.ddimxq_x0_quantile(P(x), P(eps), P(tab), tab.size(0), P(t), rank, 1.0, float("inf"), P(work), P(scale), b,
                                                     per, _lib.stream())), 6)
    # x, eps read; eps written
    report("ddimxq_threshold_eps",
           lambda: _lib.check(lib.ddimxq_threshold_eps(P(x), P(eps), P(out_e), P(scale), P(tab), tab.size(0), P(t), b, per, _lib.stream())), 3)
    out[-1]["scale_rows"] = scale.cpu().tolist()
    return out


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 8, "B": 8, "legs": "none,clip,dynamic"})
    legs = tuple(a.legs.split(","))
    if any(k not in RULES for k in legs):
        raise SystemExit("legs: a comma-separated choice of none, clip, dynamic")
    torch.manual_seed(0)
    m = timing.audio_model()
    if a.rounds > 0:
        r = time_steps(m, a.B, a.T, a.rounds, legs)
        if "none" in legs:
            for k in legs:
                if k != "none":
                    r[f"{k}_over_none"] = r[k]["ms_per_step"] / r["none"]["ms_per_step"]
        print(json.dumps({"what": "ms per replayed sampler step", "B": a.B, "T": a.T, "dtype": "bf16", "steps": 20, "rounds": a.rounds,
                          **r}), flush=True)
    if len(legs) > 1:
        for rec in time_kernels(m, a.B, a.T):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
