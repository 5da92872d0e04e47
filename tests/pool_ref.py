"""fp64 restatement of the sampler pool's device side (test infrastructure), and the workload the pool tests share.

``begin`` / ``update`` / ``end`` are ``csrc/pool_kernels.hip``'s three kernels in numpy float64, acting on copies of
``pool.SlotTable``'s own two tables -- the "device" of ``RefPool``, which uploads exactly what ``SlotTable.admit`` names, the way
``pool.PoolStepper`` does, and checks after every step that the host's header image equals the device's.  ``solo`` is the plain
loop of one sample alone over its own coefficient table.  Both take one update from ``solver_ref.table_row``.  The noise is the
float64 normal of the stream's words (``noise_ref``), indexed by (seed, sample, draw) only."""
import numpy as np

import noise_ref as N
import solver_ref as R
from ddim_audio_amd.schedule import ddim_coefficients, dpm_coefficients
from model_harness import spread

SEED_A, SEED_B, SEED_C = 0x5EED, 0x0123456789ABCDEF, 0xDEADBEEF12345678


def workload():
    """11 requests, 14 samples: step counts 1..25, orders 1-3, eta in {0, 0.5, 1}, one request of three samples and one of two;
    seeds above 2^32 and a sample index above 2^31 (the slot table keeps them as bit patterns in int32 words)."""
    spec = [  # steps, order, eta, n, seed, first_sample
        (20, 1, 0.0, 1, None, 0), (5, 2, 0.0, 1, None, 0), (25, 3, 0.0, 1, None, 0), (1, 1, 1.0, 1, SEED_A, 7),
        (12, 1, 0.5, 3, SEED_B, 100), (2, 3, 0.0, 1, None, 0), (17, 1, 1.0, 1, SEED_A, 3), (9, 2, 0.0, 2, None, 0),
        (3, 1, 0.0, 1, None, 0), (25, 1, 0.5, 1, SEED_C, 4000000000), (7, 3, 0.0, 1, None, 0)]
    out = []
    for i, (steps, order, eta, n, seed, first) in enumerate(spec):
        seq = spread(steps)
        assert len(seq) == steps
        out.append(dict(name=f"r{i}", seq=seq, order=order, eta=eta, n=n, seed=seed, first=first))
    return out


def z64(seed, sample, draw, shape):
    """The float64 normals of one sample's draw: counter (group, sample, draw, tag 0), key ``seed``."""
    return N.normals64(N.words(seed, sample, (1,) + tuple(shape), draw))[0][0]


def table32(seq, alpha, eta, order):
    """One request's rows from the schedule functions, rounded to fp32 as every device table is, as float64 [len, 8]."""
    c = dpm_coefficients(seq, alpha, order) if order > 1 else np.concatenate([ddim_coefficients(seq, alpha, eta), np.zeros((len(seq), 2))], 1)
    return c.astype(np.float32).astype(np.float64)


def solo(x, rows, model_fn, seed=0, sample=0):
    """One sample alone: every row of its table in turn; returns the final x_{t-1}."""
    x = np.asarray(x, dtype=np.float64)
    m1 = m2 = None
    for k, row in enumerate(rows):
        eps = np.asarray(model_fn(x, int(row[0])), dtype=np.float64)
        u, m0 = R.table_row(x, eps, m1, m2, None, row, lambda: z64(seed, sample, k, x.shape))
        x, m1, m2 = u, m0, m1
    return x


# ---- the three kernels ---------------------------------------------------------------------------------------------------------------
def _pos(header, b, max_steps):
    pos, n = int(header[b, 0]), int(header[b, 1])
    return pos if 0 <= pos < n <= max_steps else -1


def begin(arena, header):
    """t[b]: the t of slot b's current row, 0 for an idle slot."""
    return [int(arena[b, _pos(header, b, arena.shape[1]), 0]) if _pos(header, b, arena.shape[1]) >= 0 else 0 for b in range(arena.shape[0])]


def update(xt, eps, x0, hist, arena, header):
    """In place on the active slots of xt / x0 / hist (float64 [slots, ...]); idle slots are not touched."""
    u32 = header.view(np.uint32)
    for b in range(arena.shape[0]):
        pos = _pos(header, b, arena.shape[1])
        if pos < 0:
            continue
        seed = int(u32[b, 2]) | (int(u32[b, 3]) << 32)
        z = lambda: z64(seed, int(u32[b, 4]), (int(u32[b, 5]) + pos) & 0xFFFFFFFF, xt[b].shape)  # noqa: E731
        m1 = x0[b].copy()
        xt[b], x0[b] = R.table_row(xt[b], eps[b], m1, hist[b], None, arena[b, pos], z)
        hist[b] = m1


def end(header, max_steps):
    for b in range(header.shape[0]):
        pos = _pos(header, b, max_steps)
        if pos >= 0:
            header[b, 0] = pos + 1


class RefPool:
    """A ``SlotTable`` driven the way ``SamplerPool.step`` drives it, with the float64 kernels above as its device.
    ``log``: one (step, slot, ticket, index) per admission, ``step`` counted from 0."""

    def __init__(self, table, sample_shape):
        self.table = table
        s = (table.slots,) + tuple(sample_shape)
        self.xt, self.x0, self.hist = np.zeros(s), np.zeros(s), np.zeros(s)
        self.d_arena, self.d_header = np.zeros_like(table.arena), np.zeros_like(table.header)
        self.results, self.log = {}, []

    def step(self, model_fn):
        tb = self.table
        for b, e in tb.admit():
            n = e.rows.shape[0]
            self.d_arena[b, :n] = tb.arena[b, :n]
            self.d_header[b] = tb.header[b]
            self.xt[b] = e.payload
            self.log.append((tb.stats["steps"], b, e.ticket, e.index))
        if not tb.active():
            return []
        t = begin(self.d_arena, self.d_header)
        eps = np.stack([np.asarray(model_fn(self.xt[b], t[b]), dtype=np.float64) for b in range(tb.slots)])  # idle slots too
        update(self.xt, eps, self.x0, self.hist, self.d_arena, self.d_header)
        end(self.d_header, tb.max_steps)
        finished, tickets = tb.advance()
        assert np.array_equal(self.d_header, tb.header), "the host's image of the slot table must follow the device's"
        for b, e in finished:
            self.results[(e.ticket, e.index)] = self.xt[b].copy()
        return tickets

    def drain(self, model_fn):
        while self.table.queue or self.table.active():
            self.step(model_fn)
