"""Stochastic sampler timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Times ms per sampler step of three DDIMSteppers over the same 20-entry log-SNR schedule (tools/solver_time.py's), in one process:
  eta0        -- eta = 0, the deterministic step replayed from its hipGraph;
  eta1_stream -- eta = 1 with a NoiseStream: the noise is filled inside the step, which replays from its hipGraph;
  eta1_torch  -- eta = 1 the way it ran before the stream existed: noise_fn = torch.randn_like, every step launched eagerly.
Every round times each of them once; the order within a round alternates (forwards, then backwards) so that no leg always runs
first or always runs behind the same neighbour.  Before that, ddimx_noise_fill alone (50 launches captured into one graph, the
replay between two events): its time, the bytes it writes over that time, and that as a share of the 8 TB/s HBM peak -- the write
bandwidth of a VALU-heavy kernel, not a roofline claim (the kernel is bound by its ~230 vector instructions per four outputs, not
by the store) -- and ddimx_ddim_update with and without the noise read; their sum is the share of the step the noise costs.
usage: python tools/noise_time.py [T=1024] [rounds=6] [B ...=8]   (rounds = 0: the kernels alone)
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
from ddim_audio_amd.schedule import ddim_coefficients, logsnr_seq, make_schedule  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec
SEED = 0x5EED


def time_steps(m, b, t_len, rounds):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    names = ("eta0", "eta1_stream", "eta1_torch")
    xts = {k: x_init.clone() for k in names}
    with torch.no_grad():
        steppers = {"eta0": DDIMStepper(m, xts["eta0"], ddim_coefficients(seq, alphas, 0.0)),
                    "eta1_stream": DDIMStepper(m, xts["eta1_stream"], ddim_coefficients(seq, alphas, 1.0), noise=D.NoiseStream(SEED)),
                    "eta1_torch": DDIMStepper(m, xts["eta1_torch"], ddim_coefficients(seq, alphas, 1.0), noise_fn=torch.randn_like)}
    res = {k: [] for k in names}
    n_timed = len(seq) - 1
    try:
        for r in range(rounds + 2):  # two warm-up rounds (the first also captures the two graphs)
            for name in (names if r % 2 == 0 else names[::-1]):
                st = steppers[name]
                xts[name].copy_(x_init)
                st.rewind()
                with torch.no_grad():
                    st.step()  # row 0 (the graph steppers' eager step in the first round)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n_timed):
                        st.step()
                    e1.record()
                torch.cuda.synchronize()
                if r >= 2:
                    res[name].append(e0.elapsed_time(e1) / n_timed)
        assert steppers["eta0"].captures == 1 and steppers["eta1_stream"].captures == 1 and steppers["eta1_torch"].captures == 0
    finally:
        for st in steppers.values():
            st.close()
    return {k: {"ms_per_step": statistics.median(v), "spread_ms": max(v) - min(v)} for k, v in res.items()}


def _events(fn, reps):
    """ms per call of ``fn`` (one kernel launch): ``reps`` launches captured into one graph, the replay timed -- a kernel of a few
    microseconds launched from Python would be timed by the interpreter, not by the GPU."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    for _ in range(3):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    del g
    torch.cuda.synchronize()
    return ms


def time_kernels(b, t_len, reps=50):
    lib = _lib.load()
    xt, eps, x0, nz = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(4))
    coef = torch.tensor([[500.0, 0.6, 0.8, 0.6, 0.4, 0.1]], device="cuda")
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    P, n, nbytes = _lib.ptr, xt.numel(), xt.numel() * 4
    ns = D.NoiseStream(SEED)
    out = []

    def report(name, ms, passes, note):
        out.append({"what": name, "B": b, "T": t_len, "ms": ms, "bytes": passes * nbytes, "TB_per_s": passes * nbytes / ms / 1e9,
                    "frac_of_8TBps": passes * nbytes / HBM_PEAK / (ms * 1e-3), "note": note})

    report("ddimx_noise_fill normals", _events(lambda: ns.fill(nz, ctr), reps), 1,
           "bytes written over time: write bandwidth of a VALU-heavy kernel, not a roofline claim")
    words = torch.empty(nz.shape, dtype=torch.int32, device="cuda")
    report("ddimx_noise_fill words", _events(lambda: ns.fill(words, ctr), reps), 1, "the Philox rounds without the normal transform")
    ms0 = _events(lambda: _lib.check(lib.ddimx_ddim_update(P(xt), P(eps), None, P(x0), P(coef), P(ctr), n, _lib.stream())), reps)
    report("ddimx_ddim_update without noise", ms0, 4, "x_t, eps read; x0, x_t written")
    xt.normal_()
    ms1 = _events(lambda: _lib.check(lib.ddimx_ddim_update(P(xt), P(eps), P(nz), P(x0), P(coef), P(ctr), n, _lib.stream())), reps)
    report("ddimx_ddim_update with noise", ms1, 5, "+ the noise buffer read")
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
    for b in bs:
        recs = time_kernels(b, t_len)
        if rounds > 0:
            r = time_steps(m, b, t_len, rounds)
            a, s, t = (r[k]["ms_per_step"] for k in ("eta0", "eta1_stream", "eta1_torch"))
            spread = max(r["eta1_stream"]["spread_ms"], r["eta1_torch"]["spread_ms"])
            r["stream_over_eta0"] = s / a
            r["stream_over_torch"] = s / t
            r["stream_vs_torch"] = "equal within spread" if abs(s - t) <= spread else ("stream faster" if s < t else "stream slower")
            fill = recs[0]["ms"]
            extra_read = max(recs[3]["ms"] - recs[2]["ms"], 0.0)
            r["fill_plus_extra_read_ms"] = fill + extra_read
            r["fill_plus_extra_read_share_of_stream_step"] = (fill + extra_read) / s
            print(json.dumps({"what": "ms per sampler step", "B": b, "T": t_len, "dtype": "bf16", "steps": 20, "rounds": rounds, **r}),
                  flush=True)
        for rec in recs:
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
