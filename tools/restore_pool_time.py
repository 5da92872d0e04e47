"""Restoring pool timing on one MI355X: the audio config (bf16 activations), [8, 2, T, 256], HIP events after warm-up, one process.

(a)  ms per replayed step of four legs over the same 20-entry log-SNR schedule at order 2:
  restore_pool   -- ``RestorePool.step()`` with 8 busy restoration slots (``rpx_pool_update``, every slot known);
  generate_pool  -- the same pool with 8 busy generation slots (``rpx_pool_update``, every slot plain);
  sampler_pool   -- ``SamplerPool.step()`` with 8 busy slots of the same generation request (``ddimx_pool_update``);
  inpaint_replace -- ``InpaintSolverStepper`` at B = 8, replacement only (``inpaint_solver_steps``' step).
Every round times each leg once over the same rows (1 .. 18: no admission and no completion inside the timed region); the order
within a round alternates so that no leg always runs first or always behind the same neighbour.
(b)  ``rpx_pool_update`` alone, all slots known and all slots plain, beside ``ddimx_pool_update`` in the same run, on an order-3
row (back-to-back launches between two events): the bytes each must move over its time, as a share of the HBM peak.
(c)  wall time (host clock around a device synchronise, results on the host) of ``n`` single-sample requests -- half restoration
at 20 steps and order 2, half generation at order 2 on the 20- and the 50-level log-SNR grid in turn (the latter has 49 distinct
timesteps) -- three ways: one 8-slot ``RestorePool``; the same requests grouped by kind and schedule into
``inpaint_solver_steps`` / ``dpm_solver_steps`` calls of up to B = 8; the same requests one by one at B = 1.  Each way runs once
unmeasured first.
usage: python tools/restore_pool_time.py [T=1024] [rounds=6] [what=abc] [n=32]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.schedule import logsnr_seq, make_schedule  # noqa: E402

B, STEPS, ORDER = 8, 20, 2
N_TIMED = STEPS - 2


def _known(b, t_len):
    """(y, mask) [b, 2, t_len, 256]: the second quarter of every clip is the gap."""
    mk = torch.ones(b, 1, t_len, 1, device="cuda")
    mk[:, :, t_len // 4: t_len // 2] = 0
    mk = mk.expand(b, 2, t_len, 256).contiguous()
    return (torch.randn((b, 2, t_len, 256), device="cuda") * mk).contiguous(), mk


def time_steps(m, alphas, t_len, rounds):
    from ddim_audio_amd.inpaint_solver import InpaintSolverStepper
    from ddim_audio_amd.schedule import inpaint_solver_coefficients
    x_init = torch.randn((B, 2, t_len, 256), device="cuda")
    y, mk = _known(B, t_len)
    seq = logsnr_seq(alphas, STEPS)
    xt = x_init.clone()
    with torch.no_grad():
        alone = InpaintSolverStepper(m, xt, y, mk, inpaint_solver_coefficients(seq, alphas, ORDER, 0.0, 0.0), ORDER, False, True)
    rpool = D.RestorePool(m, alphas, slots=B, t_size=t_len, max_steps=STEPS)
    spool = D.SamplerPool(m, alphas, slots=B, t_size=t_len, max_steps=STEPS)
    tickets = []

    def pool_leg(pool, **known):
        def submit():
            tickets.append(pool.submit(x_init, seq, order=ORDER, **known))

        def drain():
            pool.drain()
            assert tickets.pop().done
        return timing.Leg(submit, pool.step, N_TIMED, after=drain)

    legs = {"restore_pool": pool_leg(rpool, y=y, mask=mk), "generate_pool": pool_leg(rpool), "sampler_pool": pool_leg(spool),
            "inpaint_replace": timing.stepper_leg(alone, xt, x_init, N_TIMED)}
    try:
        out, counts = timing.time_legs(legs, rounds)
        for pool in (rpool, spool):
            stats = pool.stats
            assert stats["captures"] == 1 and stats["idle"] == 0, stats
    finally:
        rpool.close()
        spool.close()
    out["inpaint_replace"]["captures_while_timed"] = counts["inpaint_replace"]["captures_while_timed"]
    for k in ("generate_pool", "sampler_pool", "inpaint_replace"):
        out[f"restore_pool_minus_{k}_ms"] = out["restore_pool"]["ms_per_step"] - out[k]["ms_per_step"]
    out["margin_ms"] = max(out[k]["spread_ms"] for k in legs)
    return out


def time_kernels(t_len):
    lib = _lib.load()
    shape, per = (B, 2, t_len, 256), 2 * t_len * 256
    xt, eps, x0, hist, y, mk = (torch.randn(shape, device="cuda") for _ in range(6))
    mk = (mk > 0).float()
    # one order-3 row per slot at pos 0; the coefficients contract so that xt stays finite over the launches
    arena = torch.tensor([[500.0, 0.6, 0.8, 0.6, 0.3, 0.0, 0.1, -0.05]] * B, device="cuda")
    known = torch.tensor([[0.5, 0.2]] * B, device="cuda")
    heads = {}
    for name, flag in (("known", _lib.RPX_KNOWN), ("plain", 0)):
        heads[name] = torch.tensor([[0, 1, 0, 0, b, 0, flag, 0] for b in range(B)], dtype=torch.int32, device="cuda")
    P, n = _lib.ptr, xt.numel() * 4

    def new(head):
        _lib.check(lib.rpx_pool_update(P(xt), P(eps), P(x0), P(hist), P(y), P(mk), P(arena), P(known), P(head), B, 1, per, _lib.stream()))

    def old():
        _lib.check(lib.ddimx_pool_update(P(xt), P(eps), P(x0), P(hist), P(arena), P(heads["plain"]), B, 1, per, _lib.stream()))

    # passes (sample-sized reads + writes) at order 3: x_t, eps, x0, hist read, x_t, x0, hist written (7); a known slot reads y and m too (9)
    legs = [(old, "ddimx_pool_update (for comparison)", 7), (lambda: new(heads["plain"]), "rpx_pool_update, every slot plain", 7),
            (lambda: new(heads["known"]), "rpx_pool_update, every slot known", 9)]
    out = []
    for rnd in range(2):  # every leg twice, the second time in reverse order
        for fn, name, passes in timing.leg_order(legs, rnd):
            xt.normal_()
            out.append(timing.bandwidth_record(name, timing.time_launches(fn, reps=20, warm=3), passes, n, B=B, T=t_len))
    return out


def workload(t_len, n, alphas):
    """n single-sample requests: (x, seq, y or None), restoration and generation in turn; one mask for all."""
    g = torch.Generator(device="cuda").manual_seed(7)
    seqs = {k: logsnr_seq(alphas, k) for k in (20, 50)}
    reqs = []
    for i in range(n):
        x = torch.randn((1, 2, t_len, 256), device="cuda", generator=g)
        if i % 2 == 0:
            reqs.append((x, seqs[20], torch.randn((1, 2, t_len, 256), device="cuda", generator=g)))
        else:
            reqs.append((x, seqs[(20, 50)[i // 2 % 2]], None))
    return reqs


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def time_workload(m, alphas, t_len, n):
    reqs = workload(t_len, n, alphas)
    mk = _known(1, t_len)[1][0]

    def restore(xs, seq, ys):
        return D.inpaint_solver_steps(xs, seq, m, alphas, [-1], y=ys, mask=mk, guidance=0.0, replace=True, order=ORDER)[0][-1]

    def generate(xs, seq):
        return D.dpm_solver_steps(xs, seq, m, alphas, [-1], order=ORDER)[0][-1]

    def pooled():
        with D.RestorePool(m, alphas, slots=B, t_size=t_len, max_steps=50) as pool:
            tickets = [pool.submit(x, seq, order=ORDER, **({} if y is None else dict(y=y, mask=mk))) for x, seq, y in reqs]
            pool.drain()
            return [tk.result().cpu() for tk in tickets], pool.stats

    def grouped():
        out = [None] * len(reqs)
        for kind, key in sorted({(y is not None, len(seq)) for _, seq, y in reqs}):
            idx = [i for i, (_, seq, y) in enumerate(reqs) if (y is not None, len(seq)) == (kind, key)]
            for lo in range(0, len(idx), B):
                part = idx[lo:lo + B]
                xs, seq = torch.cat([reqs[i][0] for i in part]), reqs[part[0]][1]
                res = restore(xs, seq, torch.cat([reqs[i][2] for i in part])) if kind else generate(xs, seq)
                for j, i in enumerate(part):
                    out[i] = res[j:j + 1]
        return out

    def one_by_one():
        return [generate(x.clone(), seq) if y is None else restore(x.clone(), seq, y) for x, seq, y in reqs]

    res, outs = {}, {}
    for name, fn in (("pool", pooled), ("grouped_b8", grouped), ("one_by_one_b1", one_by_one)):
        fn()  # unmeasured: workspaces, packings, the allocator's blocks
        res[name + "_s"], outs[name] = _wall(fn)
    (pool_out, stats), grp, solo = outs["pool"], outs["grouped_b8"], outs["one_by_one_b1"]
    res["pool_stats"], res["slot_steps"] = stats, sum(len(seq) for _, seq, _ in reqs)
    res["bit_identical_to_one_by_one"] = all(torch.equal(p, s) and torch.equal(g, s) for p, g, s in zip(pool_out, grp, solo))
    res["pool_over_grouped"] = res["pool_s"] / res["grouped_b8_s"]
    res["pool_over_one_by_one"] = res["pool_s"] / res["one_by_one_b1_s"]
    return res


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 6, "what": "abc", "n": 32})
    torch.manual_seed(0)
    m = timing.audio_model()
    alphas = make_schedule(m._full_config.diffusion)[1]
    head = {"B": B, "T": a.T, "dtype": "bf16"}
    if "a" in a.what:
        print(json.dumps({"what": "ms per replayed step, 8 busy slots vs B = 8", "lib": os.path.basename(_lib.LIB_PATH), **head,
                          "steps_timed": N_TIMED, "rounds": a.rounds, **time_steps(m, alphas, a.T, a.rounds)}), flush=True)
    if "b" in a.what:
        for rec in time_kernels(a.T):
            print(json.dumps(rec), flush=True)
    if "c" in a.what:
        print(json.dumps({"what": f"{a.n} requests, half restoration (20 steps), half generation (20 / 50 steps), order 2: wall seconds",
                          **head, **time_workload(m, alphas, a.T, a.n)}), flush=True)


if __name__ == "__main__":
    main()
