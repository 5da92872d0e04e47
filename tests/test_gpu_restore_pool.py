"""Restoring pool on the GPU (ddim_audio_amd.RestorePool; rpx_pool_update).

The kernel alone through guarded buffers (tests/kernel_harness.py): known, plain and idle slots in one launch; every zero /
non-zero combination of (w1, w2, c1), a first row with the history poisoned, a final row; masks of 0, 1 and 0.25 in one sample;
whatever a slot must not read poisoned.  A plain slot against ``ddimx_pool_update`` in every buffer, a known slot against
``ddimxi_multistep_update(flags = DDIMXI_REPLACE)`` at B = 1 on its row and noise identity, both against the fp32 restatement
(tests/restore_pool_ref.py), bit for bit; an idle slot's buffers unchanged; the launcher's refusals write nothing.  Then the
identity contract on the tiny model: restoration and generation requests served together by a 4-slot and a 2-slot pool, each
``torch.equal`` to its run alone, the restored samples equal to y where the mask is 1, one capture, a v model, a closed pool."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, restore_pool as RP, synth
import gpu_util as G
import kernel_harness as KH
import model_harness as MH
from model_harness import MODES, MODE_IDS, PATTERN
import restore_pool_ref as R

pytestmark = pytest.mark.gpu

# ---- 1. the kernel through the C ABI ----------------------------------------------------------------------------------------------------
MAX_STEPS = 8
PERS = [4, 4 * 255, 4 * (3 * 256 + 1)]  # one float4 | a short last block | one float4 beyond three full blocks
IDLE_HEADERS = [[0, 0], [5, 5], [7, 3]]  # never used | finished | pos beyond len
SEEDS = {"known": (0xDEADBEEF12345678, 4000000000, 3), "plain": (0x5EED, 9, 0)}  # seed, sample, draw_base


def _rows():
    """(name, pool row, (cx, w0), pos): the eight zero / non-zero combinations of (w1, w2, c1) cut from a middle row of an order-3
    tau = 1 schedule, then that schedule's first row and its final row as they stand."""
    rows, known = RP.restore_rows(MH.spread(MAX_STEPS), MH.alphas(), 3, 1.0)
    assert (rows[3, 5:8] != 0).all() and rows[0, 6] == 0 and rows[0, 7] == 0 and known[-1].tolist() == [0.0, 1.0]
    out = []
    for keep in range(8):
        r = rows[3].copy()
        r[[6, 7, 5]] *= [keep & 1, keep >> 1 & 1, keep >> 2 & 1]
        out.append((f"w1{keep & 1}w2{keep >> 1 & 1}c1{keep >> 2 & 1}", r, known[3], 3))
    return out + [("first", rows[0], known[0], 0), ("final", rows[-1], known[-1], MAX_STEPS - 1)]


ROWS = _rows()


def _nan_like(t):
    return torch.full(t.shape, PATTERN, dtype=torch.int32).view(torch.float32)


def _launch(n_slots, per, row, kn, pos, case):
    """One launch: slot 0 known, then (n_slots = 3) an idle slot and a plain one.  Returns what went in and what came out."""
    kinds = ["known", "idle", "plain"][:n_slots]
    use1, use2, add_z = R.flags_of(row)
    tag = f"rpool.k.{per}.{case}"
    v = {s: synth.gaussian(f"{tag}.{s}", (n_slots, per)) for s in ("x", "e", "m1", "m2", "y")}
    v["m"] = torch.tensor([0.0, 1.0, 0.25], dtype=torch.float32)[(torch.arange(n_slots * per) * 7 // 3) % 3].view(n_slots, per)
    assert per > 4 or set(v["m"][0].tolist()) == {0.0, 1.0, 0.25}
    if not (use1 or use2):
        v["m1"] = _nan_like(v["m1"])  # read for the history shift alone: it never enters u
    if not use2:
        v["m2"] = _nan_like(v["m2"])  # not read at all
    arena = np.full((n_slots, MAX_STEPS, 8), np.nan, np.float32)  # every row but the current one of an active slot is never read
    known = np.full((n_slots, MAX_STEPS, 2), np.nan, np.float32)
    head = np.zeros((n_slots, 8), np.uint32)
    for b, kind in enumerate(kinds):
        if kind == "idle":
            head[b, :2], head[b, RP.FLAGS] = IDLE_HEADERS[case % 3], RP.KNOWN
            for s in v:
                v[s][b] = _nan_like(v[s][b])
            continue
        seed, sample, base = SEEDS[kind]
        arena[b, pos] = row
        head[b] = [pos, MAX_STEPS, seed & 0xFFFFFFFF, seed >> 32, sample, base, RP.KNOWN if kind == "known" else 0, 0]
        if kind == "known":
            known[b, pos] = kn
        else:
            v["y"][b], v["m"][b] = _nan_like(v["y"][b]), _nan_like(v["m"][b])
    outs = {s: KH.Out(n_slots * per, init=v[k].reshape(-1)) for s, k in (("xt", "x"), ("x0", "m1"), ("hist", "m2"))}
    ro = {s: KH.Ro(v[s]) for s in ("e", "y", "m")}
    ro.update(arena=KH.Ro(arena), known=KH.Ro(known), head=KH.Ro(head.view(np.int32), torch.int32))
    rc = KH.lib().rpx_pool_update(outs["xt"].ptr, ro["e"].ptr, outs["x0"].ptr, outs["hist"].ptr, ro["y"].ptr, ro["m"].ptr, ro["arena"].ptr,
                                  ro["known"].ptr, ro["head"].ptr, n_slots, MAX_STEPS, per, _lib.stream())
    _lib.check(rc)
    KH.sync()
    for r in ro.values():
        r.check(f"{case} per {per}")
    got = {s: o.read(f"{s}, {case} per {per}").view(n_slots, per) for s, o in outs.items()}
    return kinds, v, ro, got, (use1, use2, add_z)


def _z(kind, per, pos):
    seed, sample, base = SEEDS[kind]
    return D.NoiseStream(seed, sample).step_noise((1, per), base + pos, G.dev())[0].cpu().numpy()  # what ddimx_noise_fill writes


@pytest.mark.parametrize("case", range(len(ROWS)), ids=[r[0] for r in ROWS])
@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("n_slots", [1, 3])
def test_kernel_known_plain_and_idle_slots(n_slots, per, case):
    name, row, kn, pos = ROWS[case]
    kinds, v, ro, got, (use1, use2, add_z) = _launch(n_slots, per, row, kn, pos, case)
    lib, dev, P, st = KH.lib(), G.dev(), _lib.ptr, _lib.stream()
    # ddimx_pool_update on the same buffers: word 6 of the header means nothing to it
    pool = {s: v[k].to(dev).contiguous() for s, k in (("xt", "x"), ("x0", "m1"), ("hist", "m2"))}
    _lib.check(lib.ddimx_pool_update(P(pool["xt"]), ro["e"].ptr, P(pool["x0"]), P(pool["hist"]), ro["arena"].ptr, ro["head"].ptr, n_slots,
                                     MAX_STEPS, per, st))
    KH.sync()
    for b, kind in enumerate(kinds):
        what = f"{name}: {kind} slot {b}"
        if kind == "idle":
            for s, k in (("xt", "x"), ("x0", "m1"), ("hist", "m2")):
                assert bool((MH.bits(got[s][b]) == PATTERN).all()), f"{what}: {s} was written"
            continue
        KH.same(got["hist"][b], v["m1"][b], f"{what}: hist holds the previous x0")
        z = _z(kind, per, pos) if add_z else None
        flag = R.KNOWN if kind == "known" else 0
        u, m0, _ = R.update32(v["x"][b].numpy(), v["e"][b].numpy(), v["m1"][b].numpy(), v["m2"][b].numpy(), v["y"][b].numpy(),
                              v["m"][b].numpy(), row, kn, flag, z)
        assert not torch.isnan(got["xt"][b]).any() and not torch.isnan(got["x0"][b]).any(), f"{what}: a poisoned buffer reached the output"
        KH.same(got["xt"][b], torch.from_numpy(u), f"{what}: xt against the fp32 restatement")
        KH.same(got["x0"][b], torch.from_numpy(m0), f"{what}: x0 against the fp32 restatement")
        if kind == "plain":
            for s in ("xt", "x0", "hist"):
                KH.same(got[s][b], pool[s][b].cpu(), f"{what}: {s} against ddimx_pool_update")
            continue
        # the known slot alone: ddimxi_multistep_update at B = 1 on its row (row index = pos) and its noise identity
        seed, sample, base = SEEDS[kind]
        coef = np.zeros((MAX_STEPS, _lib.DDIMXI_STRIDE), np.float32)
        coef[pos] = np.concatenate([row[:6], [0, 0, 0], kn, row[6:8]])
        coef, ctr = KH.Ro(coef), KH.Ro([pos], torch.int32)
        xa, x0a = KH.Out(per, init=v["x"][b]), KH.Out(per)
        h1, h2 = KH.Out(per, init=v["m1"][b]), KH.Out(per, init=v["m2"][b]) if use2 else None
        yb, mb, eb = KH.Ro(v["y"][b]), KH.Ro(v["m"][b]), KH.Ro(v["e"][b])
        _lib.check(lib.ddimxi_multistep_update(xa.ptr, eb.ptr, None, x0a.ptr, h1.ptr, None if h2 is None else h2.ptr, yb.ptr, mb.ptr, None, None,
                                               coef.ptr, ctr.ptr, 1, per, _lib.DDIMXI_REPLACE, seed, sample, base, st))
        KH.sync()
        KH.same(got["xt"][b], xa.read("alone xt"), f"{what}: xt against ddimxi_multistep_update")
        KH.same(got["x0"][b], h1.read("alone h1"), f"{what}: the prediction against ddimxi_multistep_update's history")
        KH.same(got["x0"][b], x0a.read("alone x0"), f"{what}: the prediction against ddimxi_multistep_update's x0")
        if name == "final":
            one = v["m"][b] == 1
            KH.same(got["xt"][b][one], v["y"][b][one], f"{what}: y's bits where the mask is 1")
        zero = v["m"][b] == 0
        KH.same(got["xt"][b][zero], pool["xt"][b].cpu()[zero], f"{what}: the plain update's bits where the mask is 0")
    if n_slots == 3 and case == 7:  # the two active slots really drew, each from its own identity
        assert add_z and not np.array_equal(_z("known", per, pos), _z("plain", per, pos))


def test_kernel_grid_stride_tail():
    """More float4s in a sample than its blocks have threads (3 slots: 682 blocks of 256): the walk runs twice for the first 77
    threads of a block's last pass."""
    per = 4 * (682 * 256 + 77)
    name, row, kn, pos = ROWS[7]
    kinds, v, ro, got, (use1, use2, add_z) = _launch(3, per, row, kn, pos, 7)
    assert use1 and use2 and add_z
    for b, kind in enumerate(kinds):
        if kind == "idle":
            assert all(bool((MH.bits(got[s][b]) == PATTERN).all()) for s in got)
            continue
        u, m0, h = R.update32(v["x"][b].numpy(), v["e"][b].numpy(), v["m1"][b].numpy(), v["m2"][b].numpy(), v["y"][b].numpy(),
                              v["m"][b].numpy(), row, kn, R.KNOWN if kind == "known" else 0, _z(kind, per, pos))
        KH.same(got["xt"][b], torch.from_numpy(u), f"{kind}: xt")
        KH.same(got["x0"][b], torch.from_numpy(m0), f"{kind}: x0")
        KH.same(got["hist"][b], v["m1"][b], f"{kind}: hist")


def test_kernel_refusals_write_nothing():
    lib, st = KH.lib(), _lib.stream()
    n, per = 2, 16
    outs = [KH.Out(n * per) for _ in range(3)]
    ro = [KH.Ro(np.zeros(n * per, np.float32)) for _ in range(3)] + [KH.Ro(np.zeros((n, MAX_STEPS, 8), np.float32)),
                                                                     KH.Ro(np.zeros((n, MAX_STEPS, 2), np.float32))]
    head = np.zeros((n, 8), np.int32)
    head[:, 1] = MAX_STEPS  # both slots active: an accepted call would write
    head = KH.Ro(head, torch.int32)
    good = dict(xt=outs[0].ptr, eps=ro[0].ptr, x0=outs[1].ptr, hist=outs[2].ptr, y=ro[1].ptr, mask=ro[2].ptr, arena=ro[3].ptr, known=ro[4].ptr,
                slots=head.ptr, n_slots=n, max_steps=MAX_STEPS, per=per)
    bad = [dict(((k, None),)) for k in ("xt", "eps", "x0", "hist", "y", "mask", "arena", "known", "slots")]
    bad += [dict(n_slots=0), dict(n_slots=65536), dict(max_steps=0), dict(per=0), dict(per=14), dict(per=-16)]
    for edit in bad:
        a = dict(good, **edit)
        rc = lib.rpx_pool_update(a["xt"], a["eps"], a["x0"], a["hist"], a["y"], a["mask"], a["arena"], a["known"], a["slots"], a["n_slots"],
                                 a["max_steps"], a["per"], st)
        KH.refused(rc, *outs, who="rpx_pool_update")
    for r in ro + [head]:
        r.check("refusals")


# ---- 2. the identity contract, end to end ---------------------------------------------------------------------------------------------
T = 32
SEED_R, SEED_G = 0x0123456789ABCDEF, 0x5EED


def _requests(f_size):
    """The four requests served together: name -> (submit keywords, x, y / mask or None)."""
    mask = torch.zeros(2, T, f_size)
    mask[:, :12] = 1
    mask[:, 12:14, ::2] = 0.25
    shape = (2, T, f_size)
    g = lambda tag, n: synth.gaussian(f"rpool.e2e.{tag}", (n,) + shape)  # noqa: E731
    return {
        "restore2": (dict(seq=MH.spread(6), order=2), g("r2.x", 1), (g("r2.y", 1), mask)),
        "restore3": (dict(seq=MH.spread(7), order=3, tau=1.0, seed=SEED_R, first=100), g("r3.x", 2), (g("r3.y", 2), mask > 0)),
        "ddim": (dict(seq=MH.spread(5), eta=0.5, seed=SEED_G, first=7), g("g1.x", 1), None),
        "solver2": (dict(seq=MH.spread(6), order=2), g("g2.x", 1), None),
    }


def _alone(m, a, kw, x, known, prediction=None):
    out = []
    for j in range(x.size(0)):
        xj = x[j:j + 1].cuda()
        ns = D.NoiseStream(kw["seed"], first_sample=kw["first"] + j) if "seed" in kw else None
        if known is not None:
            y, mask = known
            xs, _ = D.inpaint_solver_steps(xj, kw["seq"], m, a, [-1], y=y[j], mask=mask, guidance=0.0, replace=True, order=kw["order"],
                                           tau=kw.get("tau", 0.0), noise=ns, prediction=prediction)
        elif kw.get("order", 1) == 1:
            xs, _ = D.generalized_steps(xj, kw["seq"], m, a, [-1], eta=kw["eta"], noise=ns, prediction=prediction)
        else:
            xs, _ = D.dpm_solver_steps(xj, kw["seq"], m, a, [-1], order=kw["order"], prediction=prediction)
        out.append(xs[-1][0])
    return torch.stack(out)


def _serve(m, a, reqs, slots, names):
    pool = D.RestorePool(m, a, slots=slots, t_size=T, max_steps=8)
    tickets = {}
    for k in names:
        kw, x, known = reqs[k]
        ns = D.NoiseStream(kw["seed"], first_sample=kw["first"]) if "seed" in kw else None
        y, mask = known if known is not None else (None, None)
        tickets[k] = pool.submit(x, kw["seq"], eta=kw.get("eta", 0.0), order=kw.get("order", 1), noise=ns, tau=kw.get("tau", 0.0), y=y, mask=mask)
    done = pool.drain()
    assert sorted(map(id, done)) == sorted(map(id, tickets.values()))
    stats, st = pool.stats, pool._stepper
    out = {k: tk.result().cpu() for k, tk in tickets.items()}
    pool.close()
    assert st.graph is None and st._ctx is None and st._refs is None
    with pytest.raises(ValueError, match="closed"):
        pool.submit(reqs[names[0]][1], reqs[names[0]][0]["seq"])
    return out, stats


_CASES = {}


def _case(mode, kind=None):
    key = (mode[0], kind)
    if key not in _CASES:
        cfg, m = MH.build("tiny", mode[0], 5, mode="eval", kind=kind)
        a = MH.alphas(cfg)
        reqs = _requests(cfg.model.f_size)
        names = list(reqs) if kind is None else ["restore2", "restore3"]
        solo = {k: _alone(m, a, *reqs[k]) for k in names}
        _CASES[key] = (m, a, reqs, names, solo)
    return _CASES[key]


def _check(got, solo, reqs, what):
    for k, want in solo.items():
        for j in range(want.size(0)):
            assert torch.equal(got[k][j], want[j]), f"{what}: request {k} sample {j} differs from its run alone"
        if reqs[k][2] is not None:
            y, mask = reqs[k][2]
            one = torch.broadcast_to(mask.float() == 1, want.shape)
            assert bool(one.any()) and torch.equal(got[k][one], torch.broadcast_to(y, want.shape)[one]), f"{what}: {k} is y where the mask is 1"
            assert not torch.equal(got[k][~one], torch.broadcast_to(y, want.shape)[~one])


@pytest.mark.parametrize("slots", [4, 2])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_every_request_equals_its_run_alone(mode, slots):
    m, a, reqs, names, solo = _case(mode)
    got, stats = _serve(m, a, reqs, slots, names)
    _check(got, solo, reqs, f"{slots} slots")
    busy = sum(reqs[k][1].size(0) * len(reqs[k][0]["seq"]) for k in names)
    assert stats["captures"] == 1 and stats["busy"] == busy and stats["idle"] == slots * stats["steps"] - busy
    if slots == 2:
        assert stats["steps"] > max(len(reqs[k][0]["seq"]) for k in names), "two slots queue the five samples"
        rev, stats = _serve(m, a, reqs, slots, names[::-1])  # other slots, other neighbours
        _check(rev, solo, reqs, "reverse order")
        assert stats["captures"] == 1
    else:
        # the noise matters: the same request with tau = 0 ends elsewhere
        kw, x, known = reqs["restore3"]
        det, _ = _serve(m, a, {"restore3": (dict(kw, tau=0.0), x, known)}, 4, ["restore3"])
        assert not torch.equal(det["restore3"], got["restore3"])


def test_restoration_identity_on_a_v_model():
    m, a, reqs, names, solo = _case(MODES[1], kind="v")
    assert m.prediction == "v"
    got, stats = _serve(m, a, reqs, 2, names)
    _check(got, solo, reqs, "v model")
    assert stats["captures"] == 1
