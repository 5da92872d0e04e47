"""x0 clip / dynamic threshold timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Times ms per replayed step of ``generalized_steps``' stepper (DDIMStepper, eta = 0) over the same 20-entry uniform schedule, in
one process, under the three settings of ``threshold=``:
  none    -- the frame as it is without one: timestep fill, forward, ddimx_ddim_update, counter advance;
  clip    -- X0Clip(1.0): one ddimxq_threshold_eps launch between the forward and the update;
  dynamic -- X0Threshold(0.995, 1.0): the four launches of ddimxq_x0_quantile in front of that one.
Every round times each leg once; the order within a round rotates so that no leg always runs first.  Then the two exports alone
(back-to-back calls between two events) on the eps and the x of a replayed run's first iteration, with the bytes they must move
over their time as a share of the HBM peak.
usage: python tools/threshold_time.py [T=1024] [rounds=8] [B=8] [legs=none,clip,dynamic]
(legs = none needs nothing of the feature but the keyword: the un-thresholded leg alone, for a same-box comparison with
tools/vpred_time.py's eps leg.)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib, configs, synth  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper, _threshold  # noqa: E402
from ddim_audio_amd.schedule import (X0Clip, X0Threshold, ddim_coefficients, make_schedule, make_seq, threshold_rank,  # noqa: E402
                                     v_table)

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec
RULES = {"none": None, "clip": X0Clip(1.0), "dynamic": X0Threshold(0.995, 1.0)}


def time_steps(m, b, t_len, rounds, legs):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = make_seq(1000, 20)
    coef = ddim_coefficients(seq, alphas, 0.0)
    xts = {k: x_init.clone() for k in legs}
    with torch.no_grad():
        steppers = {k: DDIMStepper(m, xts[k], coef, threshold=_threshold(RULES[k], alphas)) for k in legs}
    res = {k: [] for k in legs}
    n_replayed = len(seq) - 1
    try:
        for r in range(rounds + 2):  # two warm-up rounds (the first also captures every graph)
            for name in legs[r % len(legs):] + legs[:r % len(legs)]:
                st = steppers[name]
                xts[name].copy_(x_init)
                st.rewind()
                with torch.no_grad():
                    st.step()  # row 0 outside the window, like tools/solver_time.py
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n_replayed):
                        st.step()
                    e1.record()
                torch.cuda.synchronize()
                if r >= 2:
                    res[name].append(e0.elapsed_time(e1) / n_replayed)
        assert all(st.captures == 1 for st in steppers.values())
    finally:
        for st in steppers.values():
            st.close()
    return {k: {"ms_per_step": statistics.median(v), "spread_ms": max(v) - min(v)} for k, v in res.items()}


def _events(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def time_kernels(m, b, t_len, reps=20):
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

    def report(name, ms, passes):
        out.append({"what": name, "B": b, "T": t_len, "ms": ms, "bytes": passes * nbytes, "TB_per_s": passes * nbytes / ms / 1e9,
                    "frac_of_8TBps": passes * nbytes / HBM_PEAK / (ms * 1e-3)})

    ms = _events(lambda: _lib.check(lib.ddimxq_x0_quantile(P(x), P(eps), P(tab), tab.size(0), P(t), rank, 1.0, float("inf"), P(work),
                                                           P(scale), b, per, _lib.stream())), reps)
    report("ddimxq_x0_quantile (4 launches)", ms, 6)  # x, eps read by each of the three passes
    ms = _events(lambda: _lib.check(lib.ddimxq_threshold_eps(P(x), P(eps), P(out_e), P(scale), P(tab), tab.size(0), P(t), b, per,
                                                             _lib.stream())), reps)
    report("ddimxq_threshold_eps", ms, 3)  # x, eps read; eps written
    out[-1]["scale_rows"] = scale.cpu().tolist()
    return out


def main():
    t_len = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    b = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    legs = tuple(sys.argv[4].split(",")) if len(sys.argv) > 4 else ("none", "clip", "dynamic")
    if not legs or any(k not in RULES for k in legs):
        raise SystemExit("legs: a comma-separated choice of none, clip, dynamic")
    torch.manual_seed(0)
    cfg = configs.dict2namespace(configs.audio_dict("torch.cuda.BFloat16Tensor"))
    m = D.Model(cfg)
    synth.fill_module(m, 0)
    m.eval()
    if rounds > 0:
        r = time_steps(m, b, t_len, rounds, legs)
        if "none" in legs:
            for k in legs:
                if k != "none":
                    r[f"{k}_over_none"] = r[k]["ms_per_step"] / r["none"]["ms_per_step"]
        print(json.dumps({"what": "ms per replayed sampler step", "B": b, "T": t_len, "dtype": "bf16", "steps": 20, "rounds": rounds,
                          **r}), flush=True)
    if len(legs) > 1:
        for rec in time_kernels(m, b, t_len):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
