"""Consistency-distillation and consistency-sampling timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP
events after warm-up, everything in one process.

1. ms per eager optimisation step of three legs, each with a model, optimizer state and EMA of its own over the same batch:
  train       -- ``train.train_step``, v model (the step as it was);
  distill     -- ``distill.distill_step`` of that student against an eval-mode teacher over a 16-step teacher sequence;
  consistency -- ``consistency.consistency_step`` of that student against the same teacher and an eval-mode target model of its own
                 on 16 levels: the q-sample, the teacher's forward, ddimxd_distill_half, the target's forward, cmx_consistency_out,
                 then cmx_consistency_loss, the backward, the train step's tail and the one-launch target update.
   Every round times each leg once (``iters`` steps between two events); the order within a round alternates.  Then the teacher's
   eval forward alone, for the "train step plus two eval forwards" estimate.
2. ms per replayed sampler step at SB samples over the same 20-entry schedule:
  consistency -- ``ConsistencyStepper`` with a ``NoiseStream``: the noise is drawn inside cmx_consistency_update;
  ddim_eta1   -- ``DDIMStepper``, generalized_steps(eta = 1, noise = NoiseStream): a fill launch, then ddimx_ddim_update.
3. the four kernels alone (back-to-back launches between two events), with the bytes each must move over its time as a share of the
   HBM peak.
usage: python tools/consistency_time.py [T=1024] [rounds=6] [B=32] [iters=3] [SB=8]   (rounds = 0: the kernels alone)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib, configs, synth, train  # noqa: E402
from ddim_audio_amd.consistency import ConsistencyStepper  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import (consistency_coefficients, consistency_table, ddim_coefficients, logsnr_seq,  # noqa: E402
                                     make_schedule)

LEGS = ("train", "distill", "consistency")
SEED = 0x5EED
LEVELS = [0] + list(range(40, 1000, 64))  # 16 student levels from t_min = 0


def _model(seed, mode):
    d = configs.audio_dict("torch.cuda.BFloat16Tensor")
    d["model"]["type"] = "v"
    d["optimization"]["optimizer"]["default"]["optimizer"] = "AdamW"
    cfg = configs.dict2namespace(d)
    m = synth.fill_module(D.Model(cfg), seed)
    return cfg, (m.eval() if mode == "eval" else m)


def time_steps(b, t_len, rounds, iters):
    """Not timing.time_legs: the legs are eager training steps under autograd (tools/distill_time.py's method): one warm-up round
    sizes every workspace, and each window follows one untimed step and a synchronise."""
    x, e = torch.randn((b, 2, t_len, 256), device="cuda"), torch.randn((b, 2, t_len, 256), device="cuda")
    students = {}
    for name in LEGS:
        cfg, m = _model(0, "train")
        students[name] = (m, train.TrainingState(cfg, m))
    alphas = make_schedule(cfg.diffusion)[1].cuda()
    teacher, target = _model(1, "eval")[1], _model(0, "eval")[1]
    seq = list(range(40, 1000, 60))  # 16 teacher steps -> 8 student steps
    k = torch.arange(b) % (len(seq) // 2)
    t = torch.tensor([seq[2 * int(i) + 1] for i in k])
    n = torch.arange(b) % (len(LEVELS) - 1)

    def leg(name):
        m, st = students[name]
        if name == "consistency":
            return lambda: D.consistency_step(m, target, teacher, x, st, alphas, LEVELS, e=e, n=n)
        if name == "distill":
            return lambda: D.distill_step(m, teacher, x, st, alphas, seq, e=e, k=k)
        return lambda: train.train_step(m, x, st, alphas, e=e, t=t)

    fns = {name: leg(name) for name in LEGS}
    res = {name: [] for name in LEGS}
    for r in range(rounds + 1):
        for name in timing.leg_order(LEGS, r):
            ms = timing.time_launches(fns[name], reps=iters, warm=1, sync=True)
            if r >= 1:
                res[name].append(ms)
    out = {name: timing.summary(v) for name, v in res.items()}
    with torch.no_grad():
        fwd = [timing.time_launches(lambda: teacher(x, t.cuda()), reps=iters, warm=1, sync=True) for _ in range(max(3, rounds))]
    out["teacher_eval_forward"] = {"ms": statistics.median(fwd), "spread_ms": max(fwd) - min(fwd)}
    out["distill_over_train"] = out["distill"]["ms_per_step"] / out["train"]["ms_per_step"]
    out["consistency_over_train"] = out["consistency"]["ms_per_step"] / out["train"]["ms_per_step"]
    out["consistency_minus_train_minus_two_forwards_ms"] = (out["consistency"]["ms_per_step"] - out["train"]["ms_per_step"]
                                                            - 2 * out["teacher_eval_forward"]["ms"])
    return out


def time_sampler(m, b, t_len, rounds):
    x_init = torch.randn((b, 2, t_len, 256), device="cuda")
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = [t for t in logsnr_seq(alphas, 20) if t > 0]
    names = ("consistency", "ddim_eta1")
    xts = {k: x_init.clone() for k in names}
    ns = D.NoiseStream(SEED)
    with torch.no_grad():
        # the v table whatever the synthetic weights predict: |p|, |q| <= 1, the sample stays finite over the rounds
        steppers = {"consistency": ConsistencyStepper(m, xts["consistency"], consistency_coefficients(seq, alphas, "v"), noise=ns),
                    "ddim_eta1": DDIMStepper(m, xts["ddim_eta1"], ddim_coefficients(seq, alphas, 1.0), noise=ns)}
    res, counts = timing.time_legs({k: timing.stepper_leg(steppers[k], xts[k], x_init, len(seq) - 1) for k in names}, rounds)
    assert steppers["consistency"].noise_buf is None and steppers["ddim_eta1"].noise_buf is not None
    return {k: {**res[k], **counts[k]} for k in names}, len(seq)


def time_kernels(b, t_len):
    lib = _lib.load()
    x, out, y, f, d, zbuf, x0 = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(7))
    alphas = make_schedule(configs.audio_config().diffusion)[1]
    tab = torch.from_numpy(consistency_table(alphas, "v").astype("float32")).cuda()
    t = torch.tensor([LEVELS[1 + i % (len(LEVELS) - 1)] for i in range(b)], device="cuda")
    partial, loss, g = torch.empty(b * 64, device="cuda"), torch.empty(b + 1, device="cuda"), torch.ones(b + 1, device="cuda")
    # rows: re-noising, final; the counter selects one.  a_next |p x + q out| + c1 |z| keeps xt of order one over the launches
    coef = torch.tensor([[500.0, 0.3, -0.6, 0.6, 0.0, 0.8, 0.0, 0.0], [500.0, 0.3, -0.6, 1.0, 0.0, 0.0, 0.0, 0.0]], device="cuda")
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    P, per, nbytes = _lib.ptr, x[0].numel(), x.numel() * 4
    recs = []

    def report(name, fn, passes):
        recs.append(timing.bandwidth_record(name, timing.time_launches(fn, reps=20, warm=3, sync=True), passes, nbytes, B=b, T=t_len))

    st = _lib.stream
    # x, out read; f written
    report("cmx_consistency_out", lambda: _lib.check(lib.cmx_consistency_out(P(x), P(out), P(tab), 1000, P(t), P(f), b, per, st())), 3)
    # x, out, y read
    report("cmx_consistency_loss (2 launches)",
           lambda: _lib.check(lib.cmx_consistency_loss(P(x), P(out), P(y), P(tab), 1000, P(t), 0.0, P(partial), P(loss), b, per, st())), 3)
    report("cmx_consistency_loss pseudo-Huber (2 launches)",
           lambda: _lib.check(lib.cmx_consistency_loss(P(x), P(out), P(y), P(tab), 1000, P(t), 0.5, P(partial), P(loss), b, per, st())), 3)
    # x, out, y read; d_out written
    report("cmx_consistency_loss_bwd",
           lambda: _lib.check(lib.cmx_consistency_loss_bwd(P(x), P(out), P(y), P(tab), 1000, P(t), 0.5, P(loss), P(g), P(d), b, per, st())), 4)

    def update(z):
        _lib.check(lib.cmx_consistency_update(P(x), P(out), P(z), P(x0), P(coef), P(ctr), b, per, SEED, 0, 0, st()))

    # xt, out read; x0, xt written (+ the noise buffer read)
    report("cmx_consistency_update, drawn in the kernel", lambda: update(None), 4)
    report("cmx_consistency_update, noise buffer", lambda: update(zbuf), 5)
    ctr.fill_(1)
    report("cmx_consistency_update, final row", lambda: update(None), 4)
    return recs


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 6, "B": 32, "iters": 3, "SB": 8})
    timing.require_gpu()
    torch.manual_seed(0)
    if a.rounds > 0:
        r = time_steps(a.B, a.T, a.rounds, a.iters)
        print(json.dumps({"what": "ms per eager optimisation step", "B": a.B, "T": a.T, "dtype": "bf16", "rounds": a.rounds,
                          "iters": a.iters, **r}), flush=True)
        torch.cuda.empty_cache()
        r, steps = time_sampler(timing.audio_model(), a.SB, a.T, a.rounds)
        r["consistency_over_ddim_eta1"] = r["consistency"]["ms_per_step"] / r["ddim_eta1"]["ms_per_step"]
        print(json.dumps({"what": "ms per replayed sampler step", "B": a.SB, "T": a.T, "dtype": "bf16", "steps": steps,
                          "rounds": a.rounds, **r}), flush=True)
    for rec in time_kernels(a.SB, a.T):
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
