"""Log-likelihood timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up, everything
in one process.

1. ms per replayed network evaluation of two legs over the same model, legs alternating from round to round:
  likelihood     -- ``LikelihoodStepper`` on the Heun rows of 11 levels (20 rows): tape-keeping forward, data-only backward of the
                    probe, lkx_stage, lkx_finish;
  inpaint_guided -- ``InpaintStepper`` with ``guided=True`` over a 20-entry schedule: the same forward and backward around
                    ddimx_inpaint_residual and ddimx_inpaint_update.  The margin of the comparison is the larger of the two spreads.
2. lkx_stage alone on a Heun trapezoid row (u, k1, e, g read; xin, u written: 6 passes) and on an Euler row (u, e, g read; xin, u
   written: 5 passes), lkx_finish alone (microseconds: timed as one graph of 50 launches), and lkx_sumsq alone (x read: 1 pass),
   with the bytes each must move over its time as a share of the HBM peak.
usage: python tools/likelihood_time.py [T=1024] [rounds=6] [B=8]   (rounds = 0: the kernels alone)

Measured with the defaults on one MI355X box (one process, 6 rounds; spread = max - min over the rounds): likelihood 11.530 ms per
evaluation (spread 0.048), inpaint_guided 11.558 ms (spread 0.030): equal within the margin.  lkx_stage 16.7 us on the Heun row
(101 MB, 75 % of 8 TB/s) and 14.4 us on the Euler row (84 MB, 73 %), lkx_finish 10.6 us (128 blocks per sample), lkx_sumsq 15.4 us
(17 MB, 14 %: two launches).  The working sets fit the Infinity Cache: the shares are upper bounds on HBM alone.  Times move by
about 3 % from box to box.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.inpaint import InpaintStepper  # noqa: E402
from ddim_audio_amd.likelihood import LikelihoodStepper  # noqa: E402
from ddim_audio_amd.schedule import inpaint_coefficients, likelihood_coefficients, logsnr_seq, make_schedule  # noqa: E402

SEED = 0x5EED
ZETA = 0.5


def time_steps(m, b, t_len, rounds):
    shape = (b, 2, t_len, 256)
    x_init = torch.randn(shape, device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    table = likelihood_coefficients(sorted(set(logsnr_seq(alphas, 11))), alphas, 2, "eps")
    seq = logsnr_seq(alphas, 20)
    y, mk = torch.randn(shape, device="cuda"), torch.ones(shape, device="cuda")
    mk[:, :, t_len // 4: t_len // 2] = 0
    with torch.no_grad():
        # the backward packing is allocated before any leg captures: allocating it later would make the graphs captured so far stale
        m.prepare(x_init.device, t_len)
        m._ensure_packed_bwd(_lib.load(), x_init.device)
        xin, u, xg = x_init.clone(), x_init.clone(), x_init.clone()
        lk = LikelihoodStepper(m, xin, u, table, 1, SEED, 0)
        guided = InpaintStepper(m, xg, (y * mk).contiguous(), mk, inpaint_coefficients(seq, alphas, 0.0, ZETA), True, True)

    def reset():
        xin.copy_(x_init)
        u.copy_(x_init)
        lk.acc.zero_()
        lk.rewind()

    legs = {"likelihood": timing.Leg(reset, lk.step, table.rows.shape[0] - 1, 1, None, lk),
            "inpaint_guided": timing.stepper_leg(guided, xg, x_init, len(seq) - 1)}
    r, counts = timing.time_legs(legs, rounds, expect_captures=None)
    r = {k: {**v, **counts[k]} for k, v in r.items()}
    r["likelihood_minus_inpaint_guided_ms"] = r["likelihood"]["ms_per_step"] - r["inpaint_guided"]["ms_per_step"]
    r["margin_ms"] = max(r["likelihood"]["spread_ms"], r["inpaint_guided"]["spread_ms"])
    return r, table.rows.shape[0]


def time_kernels(b, t_len):
    lib = _lib.load()
    u, k1, e, g, xin = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(5))
    per, nbytes = u[0].numel(), u.numel() * 4
    nb = int(lib.lkx_partials_doubles(1, per))
    partial = torch.empty(b * nb, dtype=torch.float64, device="cuda")
    acc, out = torch.zeros(b, dtype=torch.float64, device="cuda"), torch.empty(b, dtype=torch.float64, device="cuda")
    # rows: a Heun trapezoid row, an Euler row, both committing; the weights are small, so u stays of order one over the launches
    coef = torch.tensor([[500.0, 1e-3, -1e-3, 0.5, 0.1, 2.0, 0.0, 0.0], [500.0, 0.0, 1e-3, 0.5, 0.1, 2.0, 0.0, 0.0]], device="cuda")
    wd = torch.tensor([0.1, 0.1], dtype=torch.float64, device="cuda")
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    P, st = _lib.ptr, _lib.stream
    recs = []

    def stage():
        _lib.check(lib.lkx_stage(P(u), P(k1), P(e), P(g), P(xin), P(partial), P(coef), P(ctr), b, per, SEED, 0, 0, st()))

    def record(name, ms, passes, **kw):
        recs.append(timing.bandwidth_record(name, ms, passes, nbytes, B=b, T=t_len, **kw))

    record("lkx_stage, Heun trapezoid row", timing.time_launches(stage, reps=20, warm=3, sync=True), 6)
    ctr.fill_(1)
    record("lkx_stage, Euler row", timing.time_launches(stage, reps=20, warm=3, sync=True), 5)
    fin = lambda: _lib.check(lib.lkx_finish(P(partial), P(acc), P(wd), P(ctr), b, nb, st()))  # noqa: E731
    ms = timing.time_graph_replay(fin, reps=50, warm=3)
    recs.append({"what": "lkx_finish", "B": b, "T": t_len, "us": ms * 1e3, "blocks_per_sample": nb, "bytes": b * nb * 8})
    record("lkx_sumsq (2 launches)",
           timing.time_launches(lambda: _lib.check(lib.lkx_sumsq(P(xin), P(partial), P(out), b, per, st())), reps=20, warm=3, sync=True), 1)
    return recs


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 6, "B": 8})
    timing.require_gpu()
    torch.manual_seed(0)
    if a.rounds > 0:
        r, rows = time_steps(timing.audio_model(), a.B, a.T, a.rounds)
        print(json.dumps({"what": "ms per replayed network evaluation", "B": a.B, "T": a.T, "dtype": "bf16", "rows": rows,
                          "rounds": a.rounds, **r}), flush=True)
        torch.cuda.empty_cache()
    for rec in time_kernels(a.B, a.T):
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
