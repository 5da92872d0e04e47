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
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib, configs, synth  # noqa: E402
from ddim_audio_amd.invert import InvertStepper  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, invert_coefficients, make_schedule  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec


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
    res = {k: [] for k in names}
    n_replayed = steppers["invert"].n_iter - 1
    try:
        for r in range(rounds + 2):  # two warm-up rounds (the first also captures every graph)
            for name in (names if r % 2 == 0 else names[::-1]):
                st = steppers[name]
                xts[name].copy_(x_init)
                st.rewind()
                with torch.no_grad():
                    st.step()  # row 0, eager in the capturing round
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

    def report(name, ms, passes):
        out.append({"what": name, "B": b, "T": t_len, "ms": ms, "bytes": passes * nbytes, "TB_per_s": passes * nbytes / ms / 1e9,
                    "frac_of_8TBps": passes * nbytes / HBM_PEAK / (ms * 1e-3)})

    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    ms = _events(lambda: _lib.check(lib.ddimx_ddim_update(P(xt), P(eps), None, P(x0), P(coef6), P(ctr), n, _lib.stream())), reps)
    report("ddimx_ddim_update (for comparison)", ms, 4)  # x_t, eps read; x0, x_t written
    for row, name in ((0, "ddimx_invert_update, first row of a level"), (1, "ddimx_invert_update, later row")):
        ctr.fill_(row)
        xt.normal_()
        ms = _events(lambda: _lib.check(lib.ddimx_invert_update(P(xt), P(eps), P(base), P(x0), P(partials), P(log), 2, P(coef), P(ctr),
                                                                b, per, _lib.stream())), reps)
        report(name, ms, 5)  # + base written (first) or read (later); both launches of the call
    if b >= 2:
        w = torch.linspace(0.0, 1.0, 11, device="cuda")
        pairs = b // 2
        z = torch.empty((pairs * 11, 2, t_len, 256), device="cuda")
        ms = _events(lambda: _lib.check(lib.ddimx_slerp(P(xt), P(eps), P(w), 11, P(z), P(partials), pairs, per, _lib.stream())), reps)
        out.append({"what": "ddimx_slerp, M = 11", "pairs": pairs, "T": t_len, "ms": ms, "bytes": (4 + 11) * pairs * per * 4,
                    "TB_per_s": (4 + 11) * pairs * per * 4 / ms / 1e9})  # z1, z2 read twice (sums, blend); M outputs written
    return out


def main():
    t_len = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    bs = [int(a) for a in sys.argv[3:]] or [8]
    torch.manual_seed(0)
    cfg = configs.dict2namespace(configs.audio_dict("torch.cuda.BFloat16Tensor"))
    m = D.Model(cfg)
    synth.fill_module(m, 0)
    m.eval()
    for b in bs if rounds > 0 else []:
        r = time_steps(m, b, t_len, rounds)
        r["ddim_legs_differ_by"] = abs(r["ddim_a"]["ms_per_step"] - r["ddim_b"]["ms_per_step"])
        r["invert_minus_ddim"] = r["invert"]["ms_per_step"] - 0.5 * (r["ddim_a"]["ms_per_step"] + r["ddim_b"]["ms_per_step"])
        print(json.dumps({"what": "ms per replayed step", "B": b, "T": t_len, "dtype": "bf16", "rows": 20, "rounds": rounds, **r}),
              flush=True)
    for b in bs:
        for rec in time_kernels(b, t_len):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
