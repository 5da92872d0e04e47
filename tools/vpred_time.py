"""v-prediction sampler timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Times ms per replayed step of ``generalized_steps``' stepper (DDIMStepper, eta = 0) over the same 20-entry uniform schedule, in
one process, under both readings of the network's output:
  eps -- the frame as it is without a v table: timestep fill, forward, ddimx_ddim_update, counter advance;
  v   -- the same with one ddimx_v_to_eps launch between the forward and the update (three sample-sized fp32 passes).
Every round times each leg once; the order within a round alternates so that no leg always runs first.  Then ddimx_v_to_eps and
ddimx_qsample_v alone (back-to-back launches between two events), with the bytes they must move over their time as a share of
the HBM peak.
usage: python tools/vpred_time.py [T=1024] [rounds=8] [B=8] [legs=eps,v]
(legs = eps needs nothing of the v path: the same file times a tree that does not have it, for a same-box comparison.)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
from ddim_audio_amd import _lib, configs  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, make_schedule, make_seq  # noqa: E402


def time_steps(m, b, t_len, rounds, legs):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = make_seq(1000, 20)
    coef = ddim_coefficients(seq, alphas, 0.0)
    xts = {k: x_init.clone() for k in legs}
    with torch.no_grad():
        steppers = {}
        for k in legs:
            kw = {}
            if k == "v":
                from ddim_audio_amd.schedule import v_table
                kw["v_table"] = v_table(alphas)
            steppers[k] = DDIMStepper(m, xts[k], coef, **kw)
    return timing.time_legs({k: timing.stepper_leg(steppers[k], xts[k], x_init, len(seq) - 1) for k in legs}, rounds)[0]


def time_kernels(b, t_len):
    from ddim_audio_amd.schedule import v_table
    lib = _lib.load()
    x, v, eps, out2 = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(4))
    alphas = make_schedule(configs.audio_config().diffusion)[1]
    vt = torch.from_numpy(v_table(alphas).astype("float32")).cuda()
    ad = alphas.cuda()
    t = torch.full((b,), 900, dtype=torch.int64, device="cuda")
    P, per, nbytes = _lib.ptr, x[0].numel(), x.numel() * 4
    out = []

    def report(name, fn, passes):
        out.append(timing.bandwidth_record(name, timing.time_launches(fn, reps=20, warm=3), passes, nbytes, B=b, T=t_len))

    # x, v read; eps written
    report("ddimx_v_to_eps", lambda: _lib.check(lib.ddimx_v_to_eps(P(x), P(v), P(eps), P(vt), vt.size(0), P(t), b, per, _lib.stream())), 3)
    report("ddimx_v_to_eps in place",
           lambda: _lib.check(lib.ddimx_v_to_eps(P(x), P(eps), P(eps), P(vt), vt.size(0), P(t), b, per, _lib.stream())), 3)
    # x0, e read; x, v written
    report("ddimx_qsample_v", lambda: _lib.check(lib.ddimx_qsample_v(P(x), P(v), P(ad), P(t), P(eps), P(out2), b, per, _lib.stream())), 4)
    return out


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 8, "B": 8, "legs": "eps,v"})
    legs = tuple(a.legs.split(","))
    if any(k not in ("eps", "v") for k in legs):
        raise SystemExit("legs: eps, v or eps,v")
    torch.manual_seed(0)
    m = timing.audio_model()
    if a.rounds > 0:
        r = time_steps(m, a.B, a.T, a.rounds, legs)
        if len(legs) == 2:
            r["v_over_eps"] = r["v"]["ms_per_step"] / r["eps"]["ms_per_step"]
        print(json.dumps({"what": "ms per replayed sampler step", "B": a.B, "T": a.T, "dtype": "bf16", "steps": 20, "rounds": a.rounds,
                          **r}), flush=True)
    if "v" in legs:
        for rec in time_kernels(a.B, a.T):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
