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
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, logsnr_seq, make_schedule  # noqa: E402

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
    return timing.time_legs({k: timing.stepper_leg(steppers[k], xts[k], x_init, len(seq) - 1) for k in names}, rounds,
                            expect_captures={"eta1_torch": 0})[0]  # every step of that leg is launched eagerly


def time_kernels(b, t_len):
    lib = _lib.load()
    xt, eps, x0, nz = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(4))
    coef = torch.tensor([[500.0, 0.6, 0.8, 0.6, 0.4, 0.1]], device="cuda")
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    P, n, nbytes = _lib.ptr, xt.numel(), xt.numel() * 4
    ns = D.NoiseStream(SEED)
    out = []

    def report(name, fn, passes, note):
        ms = timing.time_graph_replay(fn, reps=50, warm=3)
        out.append({**timing.bandwidth_record(name, ms, passes, nbytes, B=b, T=t_len), "note": note})

    report("ddimx_noise_fill normals", lambda: ns.fill(nz, ctr), 1,
           "bytes written over time: write bandwidth of a VALU-heavy kernel, not a roofline claim")
    words = torch.empty(nz.shape, dtype=torch.int32, device="cuda")
    report("ddimx_noise_fill words", lambda: ns.fill(words, ctr), 1, "the Philox rounds without the normal transform")
    report("ddimx_ddim_update without noise",
           lambda: _lib.check(lib.ddimx_ddim_update(P(xt), P(eps), None, P(x0), P(coef), P(ctr), n, _lib.stream())), 4,
           "x_t, eps read; x0, x_t written")
    xt.normal_()
    report("ddimx_ddim_update with noise",
           lambda: _lib.check(lib.ddimx_ddim_update(P(xt), P(eps), P(nz), P(x0), P(coef), P(ctr), n, _lib.stream())), 5,
           "+ the noise buffer read")
    return out


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 6, "B": [8]})
    torch.manual_seed(0)
    m = timing.audio_model()
    for b in a.B:
        recs = time_kernels(b, a.T)
        if a.rounds > 0:
            r = time_steps(m, b, a.T, a.rounds)
            e, s, t = (r[k]["ms_per_step"] for k in ("eta0", "eta1_stream", "eta1_torch"))
            spread = max(r["eta1_stream"]["spread_ms"], r["eta1_torch"]["spread_ms"])
            r["stream_over_eta0"] = s / e
            r["stream_over_torch"] = s / t
            r["stream_vs_torch"] = "equal within spread" if abs(s - t) <= spread else ("stream faster" if s < t else "stream slower")
            fill = recs[0]["ms"]
            extra_read = max(recs[3]["ms"] - recs[2]["ms"], 0.0)
            r["fill_plus_extra_read_ms"] = fill + extra_read
            r["fill_plus_extra_read_share_of_stream_step"] = (fill + extra_read) / s
            print(json.dumps({"what": "ms per sampler step", "B": b, "T": a.T, "dtype": "bf16", "steps": 20, "rounds": a.rounds, **r}),
                  flush=True)
        for rec in recs:
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
