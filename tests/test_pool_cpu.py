"""Sampler pool, host side (no GPU, no library): ``pool.SlotTable`` driven through a mixed workload with the float64 kernels of
tests/pool_ref.py as its device -- every request against its own run alone, admission order, the schedule and statistics
against a greedy list schedule computed here, the layout of the two table images -- and ``SamplerPool``'s argument validation
before the library is loaded."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, configs
from ddim_audio_amd.pool import SlotTable, Ticket, request_rows
from ddim_audio_amd.schedule import ddim_coefficients, dpm_coefficients

import model_harness as MH
import pool_ref as P
import solver_ref as S

REL = 1e-12  # float64 agreement of two runs of the same arithmetic on the same fp32 table rows; the margin is for other libm builds
SHAPE = (2, 8, 4)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _inputs(reqs):
    rng = np.random.default_rng(11)
    return [rng.standard_normal((r["n"],) + SHAPE) for r in reqs]


def _submit(table, reqs, xs, alphas):
    tickets = []
    for r, x in zip(reqs, xs):
        tk = Ticket(r["n"])
        rows = request_rows(r["seq"], alphas, r["eta"], r["order"])
        for j in range(r["n"]):
            table.push(tk, j, rows, r["seed"] or 0, r["first"] + j, 0, x[j])
        tickets.append(tk)
    return tickets


def _list_schedule(lens, slots):
    """Greedy list schedule of jobs of ``lens`` steps on ``slots`` machines: before every step the free machines, lowest first,
    take the waiting jobs in order; returns (per job (start step, machine, the step count after its last step), steps, busy)."""
    left, who, waiting = [0] * slots, [None] * slots, list(range(len(lens)))
    plan, step, busy = [None] * len(lens), 0, 0
    while waiting or any(left):
        for m in range(slots):
            if waiting and not left[m]:
                who[m] = waiting.pop(0)
                left[m] = lens[who[m]]
                plan[who[m]] = [step, m, None]
        step += 1
        for m in range(slots):
            if left[m]:
                busy += 1
                left[m] -= 1
                if not left[m]:
                    plan[who[m]][2] = step
    return plan, step, busy


@pytest.mark.parametrize("slots", [3, 4, 8])
def test_mixed_workload_equals_every_request_alone(slots):
    a = MH.alphas()
    model = S.gaussian_model(a, 0.25)  # linear in x with a gain per timestep: a wrong t, row or slot shows
    reqs = P.workload()
    assert len(reqs) == 11 and sum(r["n"] for r in reqs) > 8
    assert {len(r["seq"]) for r in reqs} >= {1, 2, 25} and {r["order"] for r in reqs} == {1, 2, 3} and {r["eta"] for r in reqs} == {0.0, 0.5, 1.0}
    xs = _inputs(reqs)
    table = SlotTable(slots, 25)
    pool = P.RefPool(table, SHAPE)
    tickets = _submit(table, reqs, xs, a)
    assert not any(tk.done for tk in tickets)
    pool.drain(model)
    # (a) every sample of every request equals its own run alone
    worst = 0.0
    for r, x, tk in zip(reqs, xs, tickets):
        assert tk.done
        rows = P.table32(r["seq"], a, r["eta"], r["order"])
        for j in range(r["n"]):
            want = P.solo(x[j], rows, model, r["seed"] or 0, r["first"] + j)
            worst = max(worst, _rel(pool.results[(tk, j)], want))
    print(f"[pool reference, {slots} slots] worst relative difference to the solo runs {worst:.2e}")
    assert worst <= REL
    # (b) FIFO, lowest slot first, and the greedy list schedule
    jobs = [(tk, j, len(r["seq"])) for r, tk in zip(reqs, tickets) for j in range(r["n"])]
    plan, steps, busy = _list_schedule([n for _, _, n in jobs], slots)
    assert [(tk, j) for _, _, tk, j in pool.log] == [(tk, j) for tk, j, _ in jobs], "admission is FIFO"
    assert [(s, b) for s, b, _, _ in pool.log] == [(p[0], p[1]) for p in plan], "each at its step, into the lowest free slot"
    assert table.stats == {"steps": steps, "busy": busy, "idle": steps * slots - busy}
    assert busy == sum(n for _, _, n in jobs)
    for tk in tickets:
        assert tk.step_done == max(p[2] for p, (t2, _, _) in zip(plan, jobs) if t2 is tk)
    # (c) everything has left
    assert not table.queue and not table.active() and (table.header[:, 0] == table.header[:, 1]).all()


def test_stochastic_requests_really_draw_and_depend_on_their_noise_identity():
    a = MH.alphas()
    model = S.gaussian_model(a, 0.25)
    x = np.random.default_rng(2).standard_normal(SHAPE)
    rows = P.table32(P.spread(12), a, 0.5, 1)
    base = P.solo(x, rows, model, P.SEED_B, 100)
    assert _rel(P.solo(x, rows, model, P.SEED_B, 101), base) > 1e-3 and _rel(P.solo(x, rows, model, P.SEED_A, 100), base) > 1e-3
    assert _rel(P.solo(x, P.table32(P.spread(12), a, 0.0, 1), model), base) > 1e-3


def test_table_images_have_the_documented_layout():
    a = MH.alphas()
    table = SlotTable(4, 30)
    assert table.arena.shape == (4, 30, _lib.DDIMX_POOL_STRIDE) and table.arena.dtype == np.float32 and not table.arena.any()
    assert table.header.shape == (4, _lib.DDIMX_POOL_SLOT_WORDS) and table.header.dtype == np.int32 and not table.header.any()
    seq = P.spread(9)
    ddim, dpm = request_rows(seq, a, 0.5, 1), request_rows(seq[:6], a, 0.0, 3)
    # padding a DDIM table, and a solver table as it stands, bit for bit
    assert ddim.dtype == np.float32 and ddim.shape == (9, 8) and dpm.shape == (6, 8)
    assert np.array_equal(ddim[:, :6], ddim_coefficients(seq, a, 0.5).astype(np.float32)) and not ddim[:, 6:].any()
    assert (ddim[:-1, 5] != 0).all()
    assert np.array_equal(dpm, dpm_coefficients(seq[:6], a, 3).astype(np.float32)) and (dpm[2:-1, 7] != 0).all()
    assert np.array_equal(request_rows(seq, a, 0.0, 1), dpm_coefficients(seq, a, 1).astype(np.float32))
    tk = Ticket(3)
    table.push(tk, 0, ddim, P.SEED_C, 4000000000, 5, "x0")
    table.push(tk, 1, dpm, 0, 0, 0, "x1")
    table.push(tk, 2, ddim, 1, 2, 3, "x2")
    got = table.admit()
    assert [(b, e.index, e.payload) for b, e in got] == [(0, 0, "x0"), (1, 1, "x1"), (2, 2, "x2")] and table.active() == [0, 1, 2]
    u = table.header.view(np.uint32)
    assert u[0].tolist() == [0, 9, P.SEED_C & 0xFFFFFFFF, P.SEED_C >> 32, 4000000000, 5, 0, 0]
    assert u[1].tolist() == [0, 6, 0, 0, 0, 0, 0, 0] and u[2].tolist() == [0, 9, 1, 0, 2, 3, 0, 0] and not u[3].any()
    assert np.array_equal(table.arena[0, :9], ddim) and np.array_equal(table.arena[1, :6], dpm) and not table.arena[1, 6:].any()
    assert not table.arena[3].any()
    # the host moves pos as the device does, and knows who finishes without looking
    for step in range(1, 10):
        assert table.finishing() == ([1] if step == 6 else [0, 2] if step == 9 else [])
        finished, tickets = table.advance()
        assert [b for b, _ in finished] == ([1] if step == 6 else [0, 2] if step == 9 else [])
        assert tickets == ([tk] if step == 9 else [])
        assert table.header[:, 0].tolist() == [step, min(step, 6), step, 0]
    assert tk.done and tk.step_done == 9 and table.stats == {"steps": 9, "busy": 24, "idle": 12}
    # a slot that was used is taken again, lowest first, and only its own rows are rewritten
    table.push(Ticket(1), 0, dpm[:2].copy())
    assert [b for b, _ in table.admit()] == [0] and table.header[0, :2].tolist() == [0, 2]
    assert np.array_equal(table.arena[0, :2], dpm[:2]) and np.array_equal(table.arena[0, 2:9], ddim[2:])
    for bad in (np.zeros((3, 6), np.float32), np.zeros((3, 8)), np.zeros((0, 8), np.float32), np.zeros((31, 8), np.float32)):
        with pytest.raises(ValueError):
            table.push(tk, 0, bad)
    for args in ((0, 10), (4, 0), (2.0, 10), (True, 10), (65536, 10)):
        with pytest.raises(ValueError):
            SlotTable(*args)


def test_argument_errors_raise_before_the_library_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    a = MH.alphas()
    model = lambda x, t: x  # noqa: E731  (never called)
    pool = D.SamplerPool(model, a, slots=4, t_size=32, max_steps=10)
    x = torch.zeros(2, 2, 32, 8)
    seq = list(range(0, 1000, 200))
    ns = D.NoiseStream(3)
    with pytest.raises(ValueError, match="max_steps"):
        pool.submit(x, list(range(11)))
    for bad in (torch.zeros(2, 2, 16, 8), torch.zeros(2, 32, 8), np.zeros((2, 2, 32, 8))):
        with pytest.raises(ValueError, match="x"):
            pool.submit(bad, seq)
    with pytest.raises(ValueError, match="batch size"):
        pool.submit(torch.zeros(0, 2, 32, 8), seq)
    with pytest.raises(ValueError, match="eta must be 0"):
        pool.submit(x, seq, eta=0.5, order=2, noise=ns)
    with pytest.raises(ValueError, match="NoiseStream"):
        pool.submit(x, seq, eta=0.5)
    with pytest.raises(TypeError, match="NoiseStream"):
        pool.submit(x, seq, eta=0.5, noise=torch.Generator())
    for eta in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="eta"):
            pool.submit(x, seq, eta=eta, noise=ns)
    for order in (0, 4, 2.0, True):
        with pytest.raises(ValueError, match="order"):
            pool.submit(x, seq, order=order)
    for bad_seq in ([], [5, 5], [10, 3], [0, 1000], [0.5, 3]):
        with pytest.raises(ValueError, match="seq"):
            pool.submit(x, bad_seq)
    with pytest.raises(ValueError, match="2\\^32"):
        pool.submit(x, seq, eta=1.0, noise=D.NoiseStream(3, first_sample=2 ** 32 - 1))
    assert pool.step() == [] and pool.drain() == [] and pool.stats == {"steps": 0, "busy": 0, "idle": 0, "captures": 0}
    pool.close()
    with pytest.raises(ValueError, match="closed"):
        pool.submit(x, seq)
    with pytest.raises(ValueError, match="closed"):
        pool.step()
    # a Model's own shape is checked when the pool is made, and on every request
    cfg = configs.tiny_config("torch.FloatTensor")
    m = D.Model(cfg)
    with pytest.raises(ValueError, match="t_size"):
        D.SamplerPool(m, a, slots=4, t_size=33)
    for kw in (dict(slots=0), dict(max_steps=0), dict(t_size=0), dict(slots=1.5)):
        with pytest.raises(ValueError):
            D.SamplerPool(m, a, **kw)
    pool = D.SamplerPool(m, a, slots=4, t_size=32)
    with pytest.raises(ValueError, match="x"):
        pool.submit(torch.zeros(1, cfg.model.channels + 1, 32, cfg.model.f_size), seq)
    with pytest.raises(ValueError, match="x"):
        pool.submit(torch.zeros(1, cfg.model.channels, 64, cfg.model.f_size), seq)
