"""Sampler pool on the GPU (ddim_audio_amd.SamplerPool; ddimx_pool_begin / _update / _end).

The kernels alone, one active slot among four, against the launches they stand in for, bit for bit, idle slots untouched; the
identity contract -- every request of the mixed workload of tests/pool_ref.py, more samples than slots, ``torch.equal`` to the
same request run alone through ``generalized_steps`` / ``dpm_solver_steps`` --; placement invariance (submission order, number
of slots, seven idle slots); one graph for the pool's life, replay = eager, with and without the two-shard fork; the live graph
across ``load_state_dict`` and a re-allocation; a closed pool."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, configs, synth
from ddim_audio_amd.pool import request_rows
from ddim_audio_amd.sampler import DDIMStepper
from ddim_audio_amd.schedule import ddim_coefficients, dpm_coefficients, logsnr_seq
from ddim_audio_amd.solver import MultistepStepper
import gpu_util as G
import model_harness as MH
from model_harness import MODES, MODE_IDS, PATTERN
import pool_ref as P

pytestmark = pytest.mark.gpu
NAMES = ["tiny", "audio"]
T_SIZE = {"tiny": 32, "audio": 64}


# ---- 1. the kernels through the C ABI ---------------------------------------------------------------------------------------------------
N_STRIDE = 4 * (512 * 256 + 1000)  # more float4s in one sample than its 512 blocks have threads: the grid-stride loop runs twice
SLOTS, MAX_STEPS, LIVE = 4, 24, 2
IDLE_HEADERS = {0: [0, 0], 1: [5, 5], 3: [7, 3]}  # never used | finished | pos beyond len


def _pattern(n):
    return torch.full((SLOTS, n), PATTERN, dtype=torch.int32, device=G.dev()).view(torch.float32)


def _tables(rows, pos, seed=0, sample=0, draw_base=0):
    arena = np.zeros((SLOTS, MAX_STEPS, 8), np.float32)
    arena[LIVE, :rows.shape[0]] = rows
    for b in IDLE_HEADERS:
        arena[b] = np.float32(np.nan)  # an idle slot's rows are not read: t stays 0 and nothing of it changes
    head = np.zeros((SLOTS, 8), np.uint32)
    head[LIVE] = [pos, rows.shape[0], seed & 0xFFFFFFFF, seed >> 32, sample, draw_base, 0, 0]
    for b, (p, n) in IDLE_HEADERS.items():
        head[b, :2] = [p, n]
    return torch.from_numpy(arena).to(G.dev()), torch.from_numpy(head.view(np.int32)).to(G.dev())


def _pool_update(xt, eps, x0, hist, arena, head, n):
    lib = _lib.load()
    _lib.check(lib.ddimx_pool_update(_lib.ptr(xt), _lib.ptr(eps), _lib.ptr(x0), _lib.ptr(hist), _lib.ptr(arena), _lib.ptr(head), SLOTS,
                                     MAX_STEPS, n, _lib.stream()))
    torch.cuda.synchronize()


def _check_idle(xt, x0, hist):
    for b in IDLE_HEADERS:
        for name, v in (("xt", xt), ("x0", x0), ("hist", hist)):
            assert bool((MH.bits(v[b]) == PATTERN).all()), f"idle slot {b}: {name} was written"


@pytest.mark.parametrize("n", [20, 3 * 5132, N_STRIDE])
def test_kernel_ddim_rows_equal_ddim_update_with_and_without_noise(n):
    lib, dev = _lib.load(), G.dev()
    a = MH.alphas()
    seq = logsnr_seq(a, 20)
    x, e = synth.gaussian(f"pool.k.x.{n}", (n,)).to(dev), synth.gaussian(f"pool.k.e.{n}", (n,)).to(dev)
    seed, sample, base = P.SEED_C, 4000000000, 3
    for eta in (0.0, 1.0):
        rows = request_rows(seq, a, eta, 1)
        c6 = torch.from_numpy(ddim_coefficients(seq, a, eta).astype(np.float32)).to(dev)
        for k in (0, 7, len(seq) - 1):
            ctr = torch.full((1,), k, dtype=torch.int32, device=dev)
            want_x, want_x0, nz = x.clone(), torch.empty_like(x), None
            if eta > 0:
                nz = D.NoiseStream(seed, sample).fill(torch.empty(1, n, device=dev), ctr, base)
            _lib.check(lib.ddimx_ddim_update(_lib.ptr(want_x), _lib.ptr(e), _lib.ptr(nz), _lib.ptr(want_x0), _lib.ptr(c6), _lib.ptr(ctr), n,
                                             _lib.stream()))
            arena, head = _tables(rows, k, seed, sample, base)
            xt, eps, x0, hist = _pattern(n), _pattern(n), _pattern(n), _pattern(n)
            xt[LIVE], eps[LIVE] = x, e
            _pool_update(xt, eps, x0, hist, arena, head, n)
            assert torch.equal(xt[LIVE], want_x) and torch.equal(x0[LIVE], want_x0), (eta, k)
            assert bool((MH.bits(hist[LIVE]) == PATTERN).all()), "hist <- the old x0, copied bit for bit"
            _check_idle(xt, x0, hist)
            if eta > 0 and k < len(seq) - 1:
                assert float(rows[k, 5]) != 0 and not torch.equal(want_x, _no_noise(x, e, c6, ctr, n)), "the row really draws"


def _no_noise(x, e, c6, ctr, n):
    lib = _lib.load()
    out, x0 = x.clone(), torch.empty_like(x)
    _lib.check(lib.ddimx_ddim_update(_lib.ptr(out), _lib.ptr(e), None, _lib.ptr(x0), _lib.ptr(c6), _lib.ptr(ctr), n, _lib.stream()))
    return out


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("n", [20, 3 * 5132, N_STRIDE])
def test_kernel_solver_rows_equal_multistep_update(n, order):
    lib, dev = _lib.load(), G.dev()
    a = MH.alphas()
    seq = logsnr_seq(a, 20)
    rows = request_rows(seq, a, 0.0, order)
    coef = torch.from_numpy(dpm_coefficients(seq, a, order).astype(np.float32)).to(dev)
    x, e, m1, m2 = (synth.gaussian(f"pool.k{order}.{s}.{n}", (n,)).to(dev) for s in "xepq")
    for k in (0, order - 1, 5, 12, len(seq) - 2, len(seq) - 1):
        assert (rows[k, 6] != 0) == (1 <= k < len(seq) - 1) and (rows[k, 7] != 0) == (order == 3 and 2 <= k < len(seq) - 1)
        ctr = torch.full((1,), k, dtype=torch.int32, device=dev)
        want_x, want_x0, want_h = x.clone(), m1.clone(), m2.clone()
        _lib.check(lib.ddimx_multistep_update(_lib.ptr(want_x), _lib.ptr(e), _lib.ptr(want_x0), _lib.ptr(want_h), _lib.ptr(coef),
                                              _lib.ptr(ctr), n, _lib.stream()))
        arena, head = _tables(rows, k)
        xt, eps, x0, hist = _pattern(n), _pattern(n), _pattern(n), _pattern(n)
        xt[LIVE], eps[LIVE], x0[LIVE], hist[LIVE] = x, e, m1, m2
        _pool_update(xt, eps, x0, hist, arena, head, n)
        assert torch.equal(xt[LIVE], want_x) and torch.equal(x0[LIVE], want_x0) and torch.equal(hist[LIVE], want_h), k
        assert torch.equal(hist[LIVE], m1)
        _check_idle(xt, x0, hist)


def test_kernel_begin_and_end_act_on_active_slots_only_and_arguments_are_validated():
    lib, dev = _lib.load(), G.dev()
    a = MH.alphas()
    seq = logsnr_seq(a, 20)
    rows = request_rows(seq, a, 0.0, 2)
    P_, s = _lib.ptr, _lib.stream()
    for k in (0, 11, len(seq) - 1):
        arena, head = _tables(rows, k, P.SEED_B, 9, 1)
        before = head.clone()
        t = torch.full((SLOTS,), -1, dtype=torch.int64, device=dev)
        _lib.check(lib.ddimx_pool_begin(P_(arena), P_(head), P_(t), SLOTS, MAX_STEPS, s))
        assert t.tolist() == [0, 0, list(reversed(seq))[k], 0]
        assert torch.equal(head, before)
        _lib.check(lib.ddimx_pool_end(P_(head), SLOTS, MAX_STEPS, s))
        before[LIVE, 0] += 1
        assert torch.equal(head, before), "pos += 1 for the active slot, every other word as it was"
    # the last row's end made the slot idle: a further step leaves all of it alone
    assert head[LIVE, :2].tolist() == [len(seq), len(seq)]
    xt, eps, x0, hist = _pattern(8), _pattern(8), _pattern(8), _pattern(8)
    _pool_update(xt, eps, x0, hist, arena, head, 8)
    _lib.check(lib.ddimx_pool_end(P_(head), SLOTS, MAX_STEPS, s))
    assert all(bool((MH.bits(v) == PATTERN).all()) for v in (xt, x0, hist)) and torch.equal(head, before)
    x = torch.zeros(SLOTS, 16, device=dev)
    bad = [(lambda: lib.ddimx_pool_begin(None, P_(head), P_(t), SLOTS, MAX_STEPS, s), "null"),
           (lambda: lib.ddimx_pool_begin(P_(arena), P_(head), P_(t), 0, MAX_STEPS, s), "n_slots"),
           (lambda: lib.ddimx_pool_end(None, SLOTS, MAX_STEPS, s), "null"),
           (lambda: lib.ddimx_pool_end(P_(head), SLOTS, 0, s), "max_steps"),
           (lambda: lib.ddimx_pool_update(P_(x), P_(x), P_(x), None, P_(arena), P_(head), SLOTS, MAX_STEPS, 16, s), "null"),
           (lambda: lib.ddimx_pool_update(P_(x), P_(x), P_(x), P_(x), P_(arena), P_(head), 65536, MAX_STEPS, 16, s), "n_slots"),
           (lambda: lib.ddimx_pool_update(P_(x), P_(x), P_(x), P_(x), P_(arena), P_(head), SLOTS, MAX_STEPS, 14, s), "multiple of 4"),
           (lambda: lib.ddimx_pool_update(P_(x), P_(x), P_(x), P_(x), P_(arena), P_(head), SLOTS, MAX_STEPS, 0, s), "multiple of 4")]
    for call, msg in bad:
        assert call() != 0
        assert msg in lib.ddimx_last_error().decode()


# ---- the workload and its solo runs, once per (mode, config) ---------------------------------------------------------------------------
_CASES = {}


def _case(mode, name):
    """(cfg, model, alphas, requests, inputs, {request name: [n, C, T, F] CPU tensor of its samples run alone})."""
    key = (mode[0], name)
    if key not in _CASES:
        cfg, m = MH.build(name, mode[0], 5, mode="eval")
        a = MH.alphas(cfg)
        reqs = P.workload()
        xs = [synth.gaussian(f"pool.{name}.{r['name']}", (r["n"], 2, T_SIZE[name], cfg.model.f_size)) for r in reqs]
        solo = {}
        for r, x in zip(reqs, xs):
            rows = []
            for j in range(r["n"]):
                xj = x[j:j + 1].cuda()
                if r["order"] == 1:
                    ns = D.NoiseStream(r["seed"], first_sample=r["first"] + j) if r["eta"] > 0 else None
                    out, _ = D.generalized_steps(xj, r["seq"], m, a, [-1], eta=r["eta"], noise=ns)
                else:
                    out, _ = D.dpm_solver_steps(xj, r["seq"], m, a, [-1], order=r["order"])
                rows.append(out[-1][0])
            solo[r["name"]] = torch.stack(rows)
        _CASES[key] = (cfg, m, a, reqs, xs, solo)
    return _CASES[key]


def _serve(m, a, name, reqs, xs, slots, before_step=None):
    """The requests through a fresh pool; returns ({request name: result on the CPU}, stats, tickets)."""
    pool = D.SamplerPool(m, a, slots=slots, t_size=T_SIZE[name], max_steps=25)
    tickets = {}
    for r, x in zip(reqs, xs):
        ns = D.NoiseStream(r["seed"], first_sample=r["first"]) if r["eta"] > 0 else None
        tickets[r["name"]] = pool.submit(x, r["seq"], eta=r["eta"], order=r["order"], noise=ns)
    assert not any(tk.done for tk in tickets.values())
    with pytest.raises(RuntimeError, match="not finished"):
        tickets[reqs[0]["name"]].result()
    done, i = [], 0
    while pool.table.queue or pool.table.active():
        if before_step is not None:
            before_step(i, pool)
        done += pool.step()
        i += 1
    assert pool.drain() == [] and sorted(map(id, done)) == sorted(map(id, tickets.values())) and all(tk.done for tk in done)
    stats = pool.stats
    out = {}
    for k, tk in tickets.items():
        res = tk.result()
        assert res.is_cuda and res.dtype == torch.float32 and tuple(res.shape) == (tk.n,) + tuple(xs[0].shape[1:])
        out[k] = res.cpu()
    pool.close()
    assert all(torch.equal(tk.result().cpu(), out[k]) for k, tk in tickets.items()), "results outlive the pool"
    return out, stats, tickets


def _assert_identity(got, solo, what):
    for k, want in solo.items():
        if k in got:
            for j in range(want.size(0)):
                assert torch.equal(got[k][j], want[j]), f"{what}: request {k} sample {j} differs from its run alone"


# ---- 2. the identity contract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_every_request_equals_the_same_request_alone(mode, name):
    cfg, m, a, reqs, xs, solo = _case(mode, name)
    got, stats, tickets = _serve(m, a, name, reqs, xs, 8)
    assert sum(r["n"] for r in reqs) > 8 and any(r["n"] == 3 for r in reqs)
    _assert_identity(got, solo, "8 slots")
    busy = sum(r["n"] * len(r["seq"]) for r in reqs)
    assert stats["busy"] == busy and stats["idle"] == 8 * stats["steps"] - busy and stats["captures"] == 1
    assert max(tk.step_done for tk in tickets.values()) == stats["steps"]
    # the stochastic requests really drew: the same request with eta = 0 differs
    r = next(r for r in reqs if r["eta"] > 0 and len(r["seq"]) > 1)
    det, _, _ = _serve(m, a, name, [dict(r, eta=0.0)], [xs[reqs.index(r)]], 4)
    assert not torch.equal(det[r["name"]], got[r["name"]])


# ---- 3. placement invariance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_result_does_not_depend_on_order_slots_or_idle_neighbours(mode, name):
    cfg, m, a, reqs, xs, solo = _case(mode, name)
    got, stats, _ = _serve(m, a, name, reqs[::-1], xs[::-1], 8)
    _assert_identity(got, solo, "reverse order")
    got, stats, _ = _serve(m, a, name, reqs, xs, 3)  # three slots: the captured step does not fork
    _assert_identity(got, solo, "3 slots")
    assert stats["captures"] == 1
    for i in (2, 9):  # one single-sample request alone among seven idle slots: order 3, and eta = 0.5
        assert reqs[i]["n"] == 1
        got, stats, _ = _serve(m, a, name, [reqs[i]], [xs[i]], 8)
        _assert_identity(got, solo, "alone in 8 slots")
        assert stats["idle"] == 7 * stats["steps"] and stats["steps"] == len(reqs[i]["seq"])


# ---- 4. one graph -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [8, 3], ids=["forked", "unforked"])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_one_capture_serves_the_workload_and_replay_equals_eager(mode, name, slots):
    cfg, m, a, reqs, xs, solo = _case(mode, name)
    got, stats, _ = _serve(m, a, name, reqs, xs, slots)
    assert stats["captures"] == 1 and stats["steps"] > 25
    with MH.eager_steps():
        eager, e_stats, _ = _serve(m, a, name, reqs, xs, slots)
    assert e_stats == dict(stats, captures=0)
    assert all(torch.equal(eager[k], got[k]) for k in got)


# ---- 5. the live graph ---------------------------------------------------------------------------------------------------------------------
def test_live_graph_sees_load_state_dict_between_two_steps():
    """As test_gpu_configs' live-graph test: new parameter values are repacked in place before the next replay, one capture
    throughout.  Two requests, the second admitted two steps after the first; the weights change before the pool's fifth step,
    i.e. before iteration 4 of the first and iteration 2 of the second -- where the solo steppers change them."""
    dtype = "torch.cuda.BFloat16Tensor"
    cfg = configs.dict2namespace(configs.tiny_dict(dtype))
    m = synth.fill_module(D.Model(cfg), 3).eval()
    other = synth.fill_module(D.Model(cfg), 11).eval().state_dict()
    first = {k: v.clone() for k, v in m.state_dict().items()}
    a = MH.alphas(cfg)
    seq_a, seq_b = list(range(0, 1000, 100)), P.spread(7)
    xa, xb = synth.gaussian("pool.live.a", (1, 2, 32, 32)), synth.gaussian("pool.live.b", (1, 2, 32, 32))

    def solo(stepper, n, switch_at):
        m.load_state_dict(first)
        for k in range(n):
            if k == switch_at:
                m.load_state_dict(other)
            stepper.step()
        torch.cuda.synchronize()
        out = stepper.xt.clone()
        stepper.close()
        return out

    with torch.no_grad():
        want_a = solo(DDIMStepper(m, xa.cuda(), ddim_coefficients(seq_a, a, 0.0), use_graph=False), len(seq_a), 4)
        want_b = solo(MultistepStepper(m, xb.cuda(), dpm_coefficients(seq_b, a, 2), 2, use_graph=False), len(seq_b), 2)
        unswitched = solo(DDIMStepper(m, xa.cuda(), ddim_coefficients(seq_a, a, 0.0), use_graph=False), len(seq_a), -1)
    assert not torch.equal(unswitched, want_a), "the new weights change the trajectory"
    m.load_state_dict(first)
    pool = D.SamplerPool(m, a, slots=4, t_size=32, max_steps=16)
    ta = pool.submit(xa, seq_a)
    for i in range(len(seq_a)):
        if i == 2:
            tb = pool.submit(xb, seq_b, order=2)
        if i == 4:
            m.load_state_dict(other)
        pool.step()
    assert ta.done and tb.done and pool.stats["captures"] == 1 and pool._stepper.graph is not None
    assert torch.equal(ta.result(), want_a) and torch.equal(tb.result(), want_b)
    pool.close()


def test_pool_recaptures_when_the_model_reallocates_and_a_closed_pool_refuses():
    mode, name = MODES[1], "audio"
    cfg, m, a, reqs, xs, solo = _case(mode, name)

    def grow(i, pool):
        if i == 6:
            assert pool._stepper.graph is not None
            ws = m._workspace[0]
            m.reserve(ws.device, 32, T_SIZE[name], 0)  # what a forward of a larger batch does first
            assert m._workspace[0] is not ws, "a larger batch re-allocates the workspace the graph points at"

    got, stats, _ = _serve(m, a, name, reqs, xs, 8, before_step=grow)
    assert stats["captures"] == 2, "the pool must capture again after the model re-allocated a buffer"
    _assert_identity(got, solo, "re-captured")
    pool = D.SamplerPool(m, a, slots=4, t_size=T_SIZE[name], max_steps=25)
    tk = pool.submit(xs[0], reqs[0]["seq"])
    pool.step()
    st = pool._stepper
    pool.close()
    assert st.graph is None and st._ctx is None and st._refs is None and not tk.done
    with pytest.raises(ValueError, match="closed"):
        pool.submit(xs[0], reqs[0]["seq"])
    with pytest.raises(ValueError, match="closed"):
        pool.step()
    pool.close()  # idempotent
