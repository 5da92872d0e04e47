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
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib, configs, synth  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, make_schedule, make_seq  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec


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
    res = {k: [] for k in legs}
    n_replayed = len(seq) - 1
    try:
        for r in range(rounds + 2):  # two warm-up rounds (the first also captures every graph)
            for name in (legs if r % 2 == 0 else legs[::-1]):
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


def time_kernels(b, t_len, reps=20):
    from ddim_audio_amd.schedule import v_table
    lib = _lib.load()
    x, v, eps, out2 = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(4))
    alphas = make_schedule(configs.audio_config().diffusion)[1]
    vt = torch.from_numpy(v_table(alphas).astype("float32")).cuda()
    ad = alphas.cuda()
    t = torch.full((b,), 900, dtype=torch.int64, device="cuda")
    P, per, nbytes = _lib.ptr, x[0].numel(), x.numel() * 4
    out = []

    def report(name, ms, passes):
        out.append({"what": name, "B": b, "T": t_len, "ms": ms, "bytes": passes * nbytes, "TB_per_s": passes * nbytes / ms / 1e9,
                    "frac_of_8TBps": passes * nbytes / HBM_PEAK / (ms * 1e-3)})

    ms = _events(lambda: _lib.check(lib.ddimx_v_to_eps(P(x), P(v), P(eps), P(vt), vt.size(0), P(t), b, per, _lib.stream())), reps)
    report("ddimx_v_to_eps", ms, 3)  # x, v read; eps written
    ms = _events(lambda: _lib.check(lib.ddimx_v_to_eps(P(x), P(eps), P(eps), P(vt), vt.size(0), P(t), b, per, _lib.stream())), reps)
    report("ddimx_v_to_eps in place", ms, 3)
    ms = _events(lambda: _lib.check(lib.ddimx_qsample_v(P(x), P(v), P(ad), P(t), P(eps), P(out2), b, per, _lib.stream())), reps)
    report("ddimx_qsample_v", ms, 4)  # x0, e read; x, v written
    return out


def main():
    t_len = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    b = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    legs = tuple(sys.argv[4].split(",")) if len(sys.argv) > 4 else ("eps", "v")
    if not legs or any(k not in ("eps", "v") for k in legs):
        raise SystemExit("legs: eps, v or eps,v")
    torch.manual_seed(0)
    cfg = configs.dict2namespace(configs.audio_dict("torch.cuda.BFloat16Tensor"))
    m = D.Model(cfg)
    synth.fill_module(m, 0)
    m.eval()
    if rounds > 0:
        r = time_steps(m, b, t_len, rounds, legs)
        if len(legs) == 2:
            r["v_over_eps"] = r["v"]["ms_per_step"] / r["eps"]["ms_per_step"]
        print(json.dumps({"what": "ms per replayed sampler step", "B": b, "T": t_len, "dtype": "bf16", "steps": 20, "rounds": rounds,
                          **r}), flush=True)
    if "v" in legs:
        for rec in time_kernels(b, t_len):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
