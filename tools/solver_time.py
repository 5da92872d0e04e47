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
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib, configs, synth  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, dpm_coefficients, logsnr_seq, make_schedule  # noqa: E402
from ddim_audio_amd.solver import MultistepStepper  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec


def time_steps(m, b, t_len, rounds):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    names = ("generalized", "order2", "order3")
    xts = {k: x_init.clone() for k in names}
    with torch.no_grad():
        steppers = {"generalized": DDIMStepper(m, xts["generalized"], ddim_coefficients(seq, alphas, 0.0)),
                    "order2": MultistepStepper(m, xts["order2"], dpm_coefficients(seq, alphas, 2), 2),
                    "order3": MultistepStepper(m, xts["order3"], dpm_coefficients(seq, alphas, 3), 3)}
    res = {k: [] for k in names}
    n_replayed = len(seq) - 1
    try:
        for r in range(rounds + 2):  # two warm-up rounds (the first also captures every graph)
            for name in (names if r % 2 == 0 else names[::-1]):
                st = steppers[name]
                xts[name].copy_(x_init)
                st.rewind()
                with torch.no_grad():
                    st.step()  # row 0: after a rewind the history buffers are stale, and row 0 never reads them
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
    xt, eps, x0, hist = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(4))
    # rows: first order (w = 0), second, third; the counter selects one.  w small enough that xt stays finite over the launches
    coef = torch.tensor([[500.0, 0.6, 0.8, 0.6, 0.4, 0.0, 0.0, 0.0], [500.0, 0.6, 0.8, 0.6, 0.4, 0.0, 0.1, 0.0],
                         [500.0, 0.6, 0.8, 0.6, 0.4, 0.0, 0.1, -0.05]], device="cuda")
    P, n, nbytes = _lib.ptr, xt.numel(), xt.numel() * 4
    out = []

    def report(name, ms, passes):
        out.append({"what": name, "B": b, "T": t_len, "ms": ms, "bytes": passes * nbytes, "TB_per_s": passes * nbytes / ms / 1e9,
                    "frac_of_8TBps": passes * nbytes / HBM_PEAK / (ms * 1e-3)})

    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    coef6 = coef[:, :6].contiguous()
    ms = _events(lambda: _lib.check(lib.ddimx_ddim_update(P(xt), P(eps), None, P(x0), P(coef6), P(ctr), n, _lib.stream())), reps)
    report("ddimx_ddim_update (for comparison)", ms, 4)  # x_t, eps read; x0, x_t written
    for row, h, name, passes in ((0, None, "ddimx_multistep_update order 1 row", 4), (1, None, "ddimx_multistep_update order 2", 5),
                                 (2, hist, "ddimx_multistep_update order 3", 7)):
        ctr.fill_(row)
        xt.normal_()
        ms = _events(lambda h=h: _lib.check(lib.ddimx_multistep_update(P(xt), P(eps), P(x0), P(h), P(coef), P(ctr), n, _lib.stream())),
                     reps)
        report(name, ms, passes)  # + x0 read (order 2); + hist read and written (order 3)
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
        for k in ("order2", "order3"):
            r[k + "_over_generalized"] = r[k]["ms_per_step"] / r["generalized"]["ms_per_step"]
        print(json.dumps({"what": "ms per replayed sampler step", "B": b, "T": t_len, "dtype": "bf16", "steps": 20, "rounds": rounds,
                          **r}), flush=True)
    for b in bs:
        for rec in time_kernels(b, t_len):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
