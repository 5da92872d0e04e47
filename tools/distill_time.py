"""Progressive-distillation and loss-weighting timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP
events after warm-up, everything in one process.

Times ms per eager optimisation step of three legs, each with a model, optimizer state and EMA of its own over the same batch:
  train    -- ``train.train_step``, eps model, no loss weight (the step as it was);
  weighted -- the same with ``loss_weight: min_snr``: ddimxd_sqerr_loss_w and its backward in the unweighted kernels' place;
  distill  -- ``distill.distill_step`` of that student against an eval-mode teacher of the same size over a 16-step teacher
              sequence: the q-sample, two teacher forwards, ddimxd_distill_half / ddimxd_distill_target, then the train step's
              loss, backward and tail.
Every round times each leg once (``iters`` steps between two events); the order within a round alternates so that no leg always
runs first.  Then the teacher's eval forward alone, for the "train step plus two eval forwards" estimate, and the two target
kernels alone with the bytes they must move over their time as a share of the HBM peak.
usage: python tools/distill_time.py [T=1024] [rounds=6] [B=32] [iters=3]
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
from ddim_audio_amd.schedule import distill_coefficients, make_schedule  # noqa: E402

LEGS = ("train", "weighted", "distill")


def _student(weight):
    d = configs.audio_dict("torch.cuda.BFloat16Tensor")
    d["optimization"]["optimizer"]["default"]["optimizer"] = "AdamW"
    if weight:
        d["model"]["loss_weight"] = "min_snr"
    cfg = configs.dict2namespace(d)
    m = synth.fill_module(D.Model(cfg), 0)
    return cfg, m, train.TrainingState(cfg, m)


def time_steps(b, t_len, rounds, iters):
    """Not timing.time_legs: the legs are eager training steps under autograd, nothing is rewound, one warm-up round sizes every
    workspace, and each window follows one untimed step and a synchronise."""
    x, e = torch.randn((b, 2, t_len, 256), device="cuda"), torch.randn((b, 2, t_len, 256), device="cuda")
    students = {"train": _student(False), "weighted": _student(True), "distill": _student(False)}
    cfg = students["train"][0]
    alphas = make_schedule(cfg.diffusion)[1].cuda()
    teacher = synth.fill_module(D.Model(cfg), 1).eval()
    seq = list(range(40, 1000, 60))  # 16 teacher steps -> 8 student steps
    k = torch.arange(b) % (len(seq) // 2)
    t = torch.tensor([seq[2 * int(i) + 1] for i in k])  # the same timesteps for all three legs

    def leg(name):
        _, m, st = students[name]
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
    out["weighted_over_train"] = out["weighted"]["ms_per_step"] / out["train"]["ms_per_step"]
    out["distill_over_train"] = out["distill"]["ms_per_step"] / out["train"]["ms_per_step"]
    out["distill_minus_train_minus_two_forwards_ms"] = (out["distill"]["ms_per_step"] - out["train"]["ms_per_step"]
                                                        - 2 * out["teacher_eval_forward"]["ms"])
    return out


def time_kernels(b, t_len):
    lib = _lib.load()
    z, e0, e1, zmid, m0, tg = (torch.randn((b, 2, t_len, 256), device="cuda") for _ in range(6))
    alphas = make_schedule(configs.audio_config().diffusion)[1]
    coef = distill_coefficients(list(range(40, 1000, 60)), alphas, "eps")
    rows = torch.from_numpy(coef[[i % coef.shape[0] for i in range(b)]].astype("float32")).cuda()
    P, per, nbytes = _lib.ptr, z[0].numel(), z.numel() * 4
    out = []

    def report(name, fn, passes):
        out.append(timing.bandwidth_record(name, timing.time_launches(fn, reps=20, warm=3, sync=True), passes, nbytes, B=b, T=t_len))

    # z, eps0 read; zmid, m0 written
    report("ddimxd_distill_half", lambda: _lib.check(lib.ddimxd_distill_half(P(z), P(e0), P(rows), P(zmid), P(m0), b, per, _lib.stream())), 4)
    # z, zmid, eps1, m0 read; target written
    report("ddimxd_distill_target",
           lambda: _lib.check(lib.ddimxd_distill_target(P(z), P(zmid), P(e1), P(m0), P(rows), P(tg), None, b, per, _lib.stream())), 5)
    return out


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 6, "B": 32, "iters": 3})
    timing.require_gpu()
    torch.manual_seed(0)
    r = time_steps(a.B, a.T, a.rounds, a.iters)
    print(json.dumps({"what": "ms per eager optimisation step", "B": a.B, "T": a.T, "dtype": "bf16", "rounds": a.rounds, "iters": a.iters,
                      **r}), flush=True)
    for rec in time_kernels(a.B, a.T):
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
