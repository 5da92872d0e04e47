"""Sampler pool timing on one MI355X: the audio config (bf16 activations), [8, 2, T, 256], HIP events after warm-up, one process.

(a), (b)  ms per replayed step of four legs over the same 100-entry uniform schedule:
  ddim_eta0 / ddim_eta1 -- ``DDIMStepper`` at B = 8, eta = 0 and eta = 1 with a ``NoiseStream`` (fill launch + update);
  pool_eta0 / pool_eta1 -- ``SamplerPool.step()`` with 8 busy slots of the same requests (the noise is drawn inside the update).
Every round times each leg once over the same rows (1 .. 90: no admission and no completion inside the timed region); the order
within a round alternates so that no leg always runs first or always behind the same neighbour.  One pool serves both eta.
(c)  wall time (host clock around a device synchronise, results on the host) of a fixed workload of 32 single-sample requests,
step counts {20, 50, 100} in turn, eta = 0, three ways: one 8-slot pool; the same requests grouped by schedule into
``generalized_steps`` calls of up to B = 8; the same requests one by one at B = 1.  Each way runs once unmeasured first.
usage: python tools/pool_time.py [T=1024] [rounds=6] [what=abc]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, make_schedule, make_seq  # noqa: E402

SEED, B, N_TIMED = 0x5EED, 8, 90


def time_steps(m, alphas, t_len, rounds):
    x_init = torch.randn((B, 2, t_len, 256), device="cuda")
    seq = make_seq(1000, 100)
    etas = {"eta0": 0.0, "eta1": 1.0}
    xts = {k: x_init.clone() for k in etas}
    with torch.no_grad():
        steppers = {k: DDIMStepper(m, xts[k], ddim_coefficients(seq, alphas, eta), noise=D.NoiseStream(SEED) if eta else None)
                    for k, eta in etas.items()}
    pool = D.SamplerPool(m, alphas, slots=B, t_size=t_len, max_steps=len(seq))
    tickets = []

    def pool_leg(eta):
        def submit():
            tickets.append(pool.submit(x_init, seq, eta=eta, noise=D.NoiseStream(SEED) if eta else None))

        def drain():
            pool.drain()
            assert tickets.pop().done
        return timing.Leg(submit, pool.step, N_TIMED, after=drain)

    legs = {}
    for k, eta in etas.items():
        legs["ddim_" + k] = timing.stepper_leg(steppers[k], xts[k], x_init, N_TIMED)
        legs["pool_" + k] = pool_leg(eta)
    try:
        out, _ = timing.time_legs(legs, rounds)
        stats = pool.stats
        assert stats["captures"] == 1 and stats["idle"] == 0
    finally:
        pool.close()
    for eta in etas:
        out[f"pool_over_ddim_{eta}"] = out[f"pool_{eta}"]["ms_per_step"] / out[f"ddim_{eta}"]["ms_per_step"]
    return out


def workload(t_len):
    g = torch.Generator(device="cuda").manual_seed(7)
    return [(torch.randn((1, 2, t_len, 256), device="cuda", generator=g), make_seq(1000, (20, 50, 100)[i % 3])) for i in range(32)]


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def time_workload(m, alphas, t_len):
    reqs = workload(t_len)

    def pooled():
        with D.SamplerPool(m, alphas, slots=B, t_size=t_len, max_steps=100) as pool:
            tickets = [pool.submit(x, seq) for x, seq in reqs]
            pool.drain()
            return [tk.result().cpu() for tk in tickets], pool.stats

    def grouped():
        out = [None] * len(reqs)
        for n in (20, 50, 100):
            idx = [i for i, (_, seq) in enumerate(reqs) if len(seq) == n]
            for lo in range(0, len(idx), B):
                part = idx[lo:lo + B]
                xs, _ = D.generalized_steps(torch.cat([reqs[i][0] for i in part]), reqs[part[0]][1], m, alphas, [-1], eta=0.0)
                for j, i in enumerate(part):
                    out[i] = xs[-1][j:j + 1]
        return out

    def one_by_one():
        return [D.generalized_steps(x.clone(), seq, m, alphas, [-1], eta=0.0)[0][-1] for x, seq in reqs]

    res, outs = {}, {}
    for name, fn in (("pool", pooled), ("grouped_b8", grouped), ("one_by_one_b1", one_by_one)):
        fn()  # unmeasured: workspaces, packings, the allocator's blocks
        res[name + "_s"], outs[name] = _wall(fn)
    (pool_out, stats), grp, solo = outs["pool"], outs["grouped_b8"], outs["one_by_one_b1"]
    res["pool_stats"] = stats
    res["bit_identical_to_one_by_one"] = all(torch.equal(p, s) and torch.equal(g, s) for p, g, s in zip(pool_out, grp, solo))
    res["pool_over_grouped"] = res["pool_s"] / res["grouped_b8_s"]
    res["pool_over_one_by_one"] = res["pool_s"] / res["one_by_one_b1_s"]
    return res


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 6, "what": "abc"})
    torch.manual_seed(0)
    m = timing.audio_model()
    alphas = make_schedule(m._full_config.diffusion)[1]
    head = {"B": B, "T": a.T, "dtype": "bf16"}
    if "a" in a.what or "b" in a.what:
        print(json.dumps({"what": "ms per replayed step, 8 busy slots vs B = 8", **head, "steps_timed": N_TIMED, "rounds": a.rounds,
                          **time_steps(m, alphas, a.T, a.rounds)}), flush=True)
    if "c" in a.what:
        print(json.dumps({"what": "32 requests, step counts 20 / 50 / 100 in turn, eta 0: wall seconds", **head,
                          **time_workload(m, alphas, a.T)}), flush=True)


if __name__ == "__main__":
    main()
