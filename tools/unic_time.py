"""UniC corrector timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Times ms per replayed sampler step of four steppers over the same 20-entry log-SNR schedule, in one process:
  order2      -- MultistepStepper, DPM-Solver++ order 2 (ddimx_multistep_update: the step without the corrector);
  order2_unic -- the same with the corrector folded in (ddimxu_multistep_update, one history tensor more);
  order3      -- order 3 without the corrector;
  order3_unic -- order 3 with it (two history tensors: hist and hist2).
Every round times each of them once; the order within a round alternates (forwards, then backwards) so that no leg always runs
first or always runs behind the same neighbour.  Then each update alone (back-to-back launches between two events), with the
bytes it must move over its time as a share of the HBM peak.
With ``unchanged``: only order2 and order3 -- the steps that existed before -- and the eighth header is not bound, so that the same
file can time a library built from the commit before (``DDIMX_LIB``): one process per library, alternated by the caller.
usage: python tools/unic_time.py [T=1024] [rounds=6] [unchanged] [B ...=8]   (rounds = 0: the kernels alone)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib, configs, synth  # noqa: E402
from ddim_audio_amd.schedule import dpm_coefficients, logsnr_seq, make_schedule, unic_coefficients  # noqa: E402
from ddim_audio_amd.solver import MultistepStepper  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec


def time_steps(m, b, t_len, rounds, unchanged):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    names = ("order2", "order3") if unchanged else ("order2", "order2_unic", "order3", "order3_unic")
    xts = {k: x_init.clone() for k in names}
    with torch.no_grad():
        steppers = {k: MultistepStepper(m, xts[k], (unic_coefficients if k.endswith("unic") else dpm_coefficients)(seq, alphas, int(k[5])),
                                        int(k[5])) for k in names}
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
        if not unchanged:
            assert steppers["order2_unic"].hist is not None and steppers["order2_unic"].hist2 is None
            assert steppers["order3_unic"].hist2 is not None
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


def time_kernels(b, t_len, unchanged, reps=20):
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

    def report(name, ms, passes):
        out.append({"what": name, "B": b, "T": t_len, "ms": ms, "bytes": passes * nbytes, "TB_per_s": passes * nbytes / ms / 1e9,
                    "frac_of_8TBps": passes * nbytes / HBM_PEAK / (ms * 1e-3)})

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
        for row, fn, name, passes in (legs if rnd == 0 else legs[::-1]):
            ctr.fill_(row)
            xt.normal_()
            report(name, _events(fn, reps), passes)
    return out


def main():
    args = sys.argv[1:]
    unchanged = "unchanged" in args
    args = [a for a in args if a != "unchanged"]
    t_len = int(args[0]) if len(args) > 0 else 1024
    rounds = int(args[1]) if len(args) > 1 else 6
    bs = [int(a) for a in args[2:]] or [8]
    if unchanged:
        _lib._UNIC_FUNCS.clear()  # a library from before the corrector has no ddimxu_ symbol to bind
    torch.manual_seed(0)
    cfg = configs.dict2namespace(configs.audio_dict("torch.cuda.BFloat16Tensor"))
    m = D.Model(cfg)
    synth.fill_module(m, 0)
    m.eval()
    for b in bs if rounds > 0 else []:
        r = time_steps(m, b, t_len, rounds, unchanged)
        if not unchanged:
            for k in ("order2", "order3"):
                r[k + "_unic_over_" + k] = r[k + "_unic"]["ms_per_step"] / r[k]["ms_per_step"]
        print(json.dumps({"what": "ms per replayed sampler step", "lib": os.path.basename(_lib.LIB_PATH), "B": b, "T": t_len, "dtype": "bf16",
                          "steps": 20, "rounds": rounds, **r}), flush=True)
    for b in bs:
        for rec in time_kernels(b, t_len, unchanged):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
