"""``SamplerPool`` -- continuous batching: a fixed batch of ``slots`` samples on the device, a schedule per slot.

Every other sampler here takes one batch through one schedule: one device counter indexes one coefficient table, so all samples
are at the same iteration of the same ``seq`` and a run ends when all of them end.  A pool serves a stream of requests instead --
20-step previews next to 200-step finals, DDIM of any ``eta`` next to DPM-Solver++ of any ``tau`` -- in one batch: each slot carries its own
coefficient rows, its own position in them and its own noise identity (``csrc/pool_kernels.hip``), a request's samples enter free
slots and leave when their schedule ends, and every step is one network evaluation over all slots, replayed from one hipGraph
that is captured once and lives as long as the pool.

The identity contract: a request's result is bit-identical to the same request run alone --
``generalized_steps(x_j[None], seq, model, alphas, [-1], eta=eta, noise=NoiseStream(seed, first_sample + j))`` or
``dpm_solver_steps(x_j[None], seq, model, alphas, [-1], order=order, tau=tau, noise=NoiseStream(seed, first_sample + j))`` --
whatever else the pool serves, whichever slot it gets
and however many slots idle.  It rests on four pinned facts: ``Model.forward`` takes one ``t`` per sample; a sample's eps does
not depend on its batch; ``NoiseStream`` noise is a pure function of (seed, sample, draw, element); and ``step_math.h`` is the
one copy of the update arithmetic.

``SlotTable`` is the host side -- queue, slot assignment, the two table images, statistics -- and needs neither the library nor
a GPU: the host knows every schedule's length, so it never reads the device to learn which slots finish.
"""
import collections

import numpy as np
import torch

from . import _lib
from .sampler import DDIMStepper, _check_eta, _check_model, _check_noise, _check_sample, _device, _prediction, _threshold, _v_table
from .schedule import ddim_coefficients, dpm_coefficients, unic_coefficients
from .solver import _check_corrector

STRIDE, SLOT_WORDS = _lib.DDIMX_POOL_STRIDE, _lib.DDIMX_POOL_SLOT_WORDS
POS, LEN, SEED_LO, SEED_HI, SAMPLE, DRAW_BASE = range(6)  # words of a slot-table row; 6 and 7 are reserved (zero)
_U32 = 1 << 32


def _positive_int(name, v, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 or (hi is not None and v > hi):
        raise ValueError(f"{name} must be an integer in 1..{hi}, got {v!r}" if hi else f"{name} must be a positive integer, got {v!r}")
    return int(v)


def request_rows(seq, alpha, eta=0.0, order=1, tau=0.0, corrector=False):
    """The arena rows of one request, fp32 [len(seq), 8] in execution order, columns (t, s1, s2, s3, c2, c1, w1, w2):
    ``schedule.dpm_coefficients`` as it stands for ``order`` 2 or 3 (``eta`` must be 0), ``schedule.ddim_coefficients`` of ``eta``
    padded with w1 = w2 = 0 for order 1.  ``tau`` > 0: ``schedule.dpm_coefficients(seq, alpha, order, tau)`` for any ``order``
    (SDE-DPM-Solver++; ``eta`` must be 0: the noise is ``tau``'s).  ``seq``, ``order`` and ``tau`` are checked by
    ``dpm_coefficients`` in every case.  ``corrector=True`` (``order`` 1 or 2, ``eta`` = ``tau`` = 0): the first eight columns of
    ``schedule.unic_coefficients`` -- the UniC corrector folded into w1 and w2; its ninth column is 0 at these orders, and order 3,
    whose w3 the arena row has no place for, is refused."""
    eta = _check_eta(eta)
    coef = dpm_coefficients(seq, alpha, order, tau)
    if _check_corrector(corrector, float(tau)):
        if order > 2:
            raise ValueError("corrector=True is served at order 1 or 2: the arena row has no ninth column for order 3's w3")
        if eta > 0:
            raise ValueError(f"corrector=True needs eta = 0 (got eta = {eta}): a stochastic corrector is not built")
        return np.ascontiguousarray(unic_coefficients(seq, alpha, order)[:, :STRIDE], dtype=np.float32)
    if order > 1 and eta > 0:
        raise ValueError(f"order = {order} takes its noise from tau: eta must be 0, got {eta}")
    if tau > 0 and eta > 0:
        raise ValueError(f"tau = {tau} and eta = {eta}: a request takes its noise from one of them, with tau > 0 eta must be 0")
    if order == 1 and not tau > 0:
        coef = np.concatenate([ddim_coefficients(seq, alpha, eta), np.zeros((coef.shape[0], 2))], axis=1)
    return np.ascontiguousarray(coef, dtype=np.float32)


class Ticket:
    """What ``SamplerPool.submit`` returns: ``done`` once every sample of the request has left its slot, ``result()`` then."""

    def __init__(self, n):
        self.n = n
        self.step_done = None  # the pool's step count after the step that completed the request
        self._left = n
        self._out = None

    @property
    def done(self):
        return self._left == 0

    def result(self):
        """[n, C, T, F] fp32 on the device: the final x_{t-1} of every sample, in stream order behind the pool's last step."""
        if not self.done:
            raise RuntimeError(f"{self._left} of the request's {self.n} samples have not finished: step() or drain() the pool")
        return self._out


class _Entry:
    """One queued sample: its ticket and index in the request, its rows, its noise identity, and what the caller attached."""
    __slots__ = ("ticket", "index", "rows", "seed", "sample", "draw_base", "payload")

    def __init__(self, ticket, index, rows, seed, sample, draw_base, payload):
        self.ticket, self.index, self.rows, self.seed, self.sample, self.draw_base, self.payload = \
            ticket, index, rows, seed, sample, draw_base, payload


class SlotTable:
    """Host state of a pool of ``slots`` slots with schedules of at most ``max_steps`` rows.

    ``arena`` (fp32 [slots, max_steps, 8]) and ``header`` (int32 [slots, 8]: pos, len, seed_lo, seed_hi, sample, draw_base, two
    reserved words) are the images of the two device tables: ``admit`` writes a slot's rows and header row here and names the
    slot, so the caller uploads exactly those; ``advance`` moves ``pos`` the way ``ddimx_pool_end`` does on the device, so the
    two stay equal without a read-back.  A slot is active iff pos < len.  Samples are queued one by one and admitted FIFO, the
    lowest free slot first.  ``stats``: ``steps``, and over them the ``busy`` and ``idle`` slot-steps."""

    def __init__(self, slots, max_steps):
        self.slots = _positive_int("slots", slots, 65535)
        self.max_steps = _positive_int("max_steps", max_steps)
        self.arena = np.zeros((self.slots, self.max_steps, STRIDE), dtype=np.float32)
        self.header = np.zeros((self.slots, SLOT_WORDS), dtype=np.int32)
        self.queue = collections.deque()
        self.owner = [None] * self.slots
        self.stats = {"steps": 0, "busy": 0, "idle": 0}

    def push(self, ticket, index, rows, seed=0, sample=0, draw_base=0, payload=None):
        """Queue one sample.  ``rows``: fp32 [len, 8] with 1 <= len <= max_steps (``request_rows``)."""
        rows = np.asarray(rows)
        if rows.dtype != np.float32 or rows.ndim != 2 or rows.shape[1] != STRIDE:
            raise ValueError(f"rows must be float32 [len, {STRIDE}]")
        if not 1 <= rows.shape[0] <= self.max_steps:
            raise ValueError(f"a schedule of {rows.shape[0]} steps does not fit the pool: 1..{self.max_steps} (max_steps)")
        if not (0 <= seed < 1 << 64 and 0 <= sample < _U32 and 0 <= draw_base < _U32):
            raise ValueError("seed outside 0 .. 2^64 - 1, or sample / draw_base outside 0 .. 2^32 - 1")
        self.queue.append(_Entry(ticket, index, rows, int(seed), int(sample), int(draw_base), payload))

    def active(self):
        return [b for b, e in enumerate(self.owner) if e is not None]

    def admit(self):
        """Move queued samples into the free slots; returns [(slot, entry)] in admission order."""
        out = []
        for b in range(self.slots):
            if not self.queue:
                break
            if self.owner[b] is not None:
                continue
            e = self.owner[b] = self.queue.popleft()
            n = e.rows.shape[0]
            self.arena[b, :n] = e.rows
            words = np.array([0, n, e.seed & (_U32 - 1), e.seed >> 32, e.sample, e.draw_base, 0, 0], dtype=np.uint32)
            self.header[b] = words.view(np.int32)
            out.append((b, e))
        return out

    def finishing(self):
        """The slots whose schedule ends with the next step."""
        return [b for b in self.active() if self.header[b, POS] + 1 == self.header[b, LEN]]

    def advance(self):
        """Account for one step over the active slots.  Returns ([(slot, entry)] that finished -- their slots are free again --,
        [tickets] whose last sample was among them)."""
        act, fin = self.active(), self.finishing()
        self.header[act, POS] += 1
        self.stats["steps"] += 1
        self.stats["busy"] += len(act)
        self.stats["idle"] += self.slots - len(act)
        finished, tickets = [], []
        for b in fin:
            e, self.owner[b] = self.owner[b], None
            finished.append((b, e))
            e.ticket._left -= 1
            if e.ticket._left == 0:
                e.ticket.step_done = self.stats["steps"]
                tickets.append(e.ticket)
        return finished, tickets


class PoolStepper(DDIMStepper):
    """The device side of a pool: a ``sampler.DDIMStepper`` whose ``xt`` is the pooled batch and whose frame reads a row and a
    position per slot: ``ddimx_pool_begin`` / ``_update`` / ``_end`` in the places of the base class's three launches, around the
    same forward.  ``coef`` is the arena ([slots * max_steps, 8]), ``slots_dev`` the slot table; the base class's single
    ``counter`` is not used.  Buffers are allocated here, once, on the launch stream and outside any capture, idle slots
    zero-filled; capture, staleness, re-capture and ``close`` are the base class's (``graphs.GraphOwner``)."""

    def __init__(self, model, table, sample_shape, device, use_graph=True, slot=0, fork=True, v_table=None, threshold=None):
        xt = torch.zeros((table.slots,) + tuple(sample_shape), dtype=torch.float32, device=device)
        super().__init__(model, xt, table.arena.reshape(-1, STRIDE), use_graph=use_graph, slot=slot, fork=fork, v_table=v_table,
                         threshold=threshold)
        self.table = table
        self.arena = self.coef.view(table.slots, table.max_steps, STRIDE)
        self.slots_dev = torch.from_numpy(table.header).to(device)
        self.x0.zero_()
        self.hist = torch.zeros_like(xt)
        self.per_sample = xt[0].numel()

    def admit(self, b, entry):
        """Slot ``b`` <- ``entry``, eagerly on the launch stream: its sample, its rows, its header row (``SlotTable.admit`` has
        written the images)."""
        self.xt[b].copy_(entry.payload)
        self.arena[b, :entry.rows.shape[0]].copy_(torch.from_numpy(entry.rows))
        self.slots_dev[b].copy_(torch.from_numpy(self.table.header[b]))

    def _shape(self):
        return self.table.slots, self.table.max_steps

    def _begin(self, st):
        _lib.check(self.lib.ddimx_pool_begin(_lib.ptr(self.coef), _lib.ptr(self.slots_dev), _lib.ptr(self.t), *self._shape(), st))

    def _update(self, et, noise, st):
        _lib.check(self.lib.ddimx_pool_update(_lib.ptr(self.xt), _lib.ptr(et), _lib.ptr(self.x0), _lib.ptr(self.hist), _lib.ptr(self.coef),
                                              _lib.ptr(self.slots_dev), *self._shape(), self.per_sample, st))

    def _end(self, st):
        _lib.check(self.lib.ddimx_pool_end(_lib.ptr(self.slots_dev), *self._shape(), st))

    def rewind(self):
        raise NotImplementedError("a pool has a position per slot; there is no table to restart")


class SamplerPool:
    """``SamplerPool(model, alphas, slots=8, t_size=1024, max_steps=1000, prediction=None, threshold=None)``: see the module
    docstring.
    ``prediction``: ``"eps"`` or ``"v"``, what the network's output is (None: ``model.prediction`` if it has one, else ``"eps"``);
    for ``"v"`` every slot's output is converted with the row of the slot's own timestep (an idle slot's is t = 0: finite, unused).
    ``threshold``: None, ``schedule.X0Clip`` or ``schedule.X0Threshold``, pool-wide like ``prediction``: every slot's x0 prediction
    is clipped or thresholded by that rule with the row of the slot's own timestep, as ``generalized_steps(threshold=)`` and
    ``dpm_solver_steps(threshold=)`` do it (the identity contract holds with the same ``threshold`` on both sides).

    ``submit(x, seq, eta=0.0, order=1, noise=None, tau=0.0, corrector=False)`` queues the n samples of ``x`` [n, C, t_size, F] (read now: the caller may
    reuse ``x``) and returns a ``Ticket``.  ``order`` 1 with any ``eta`` >= 0 is ``generalized_steps`` (``eta`` > 0 needs
    ``noise``, a ``NoiseStream``: sample j draws from sample index ``noise.first_sample + j``, draw index = its own iteration);
    ``order`` 2 or 3 is ``dpm_solver_steps`` and needs ``eta`` = 0.  ``tau`` > 0 with any ``order`` is ``dpm_solver_steps(tau=)``,
    SDE-DPM-Solver++: it needs ``noise`` like ``eta`` > 0, draws from it the same way, and excludes ``eta`` > 0.
    ``corrector=True`` is ``dpm_solver_steps(corrector=True)`` at ``order`` 1 or 2 (``eta`` = ``tau`` = 0): the folded UniC weights
    travel in the slot's w1 and w2 and the pool's update kernel is unchanged; order 3 with a corrector raises ValueError.
    Invalid arguments raise ValueError or TypeError before any device work.  ``step()`` admits queued samples into free slots
    (FIFO, lowest slot first), runs one network evaluation over all slots and returns the tickets it completed; ``drain()`` steps until queue and slots are empty.  ``stats``: ``steps``,
    ``busy`` and ``idle`` slot-steps, ``captures``.  ``close()`` destroys the graph, then frees the buffers; results already
    handed out stay valid.  Everything runs on the stream that is current when ``submit`` / ``step`` are called: use one."""

    def __init__(self, model, alphas, slots=8, t_size=1024, max_steps=1000, prediction=None, threshold=None):
        self.prediction = _prediction(model, prediction)
        self._threshold = _threshold(threshold, alphas)  # (rule, table) or None
        self.threshold = threshold
        self.table = SlotTable(slots, max_steps)
        self.t_size = _positive_int("t_size", t_size)
        self.model, self.alphas = model, alphas
        self._sample_shape = None  # (C, t_size, F): the model's, or the first request's for any other callable
        if hasattr(model, "forward_slot"):
            mc = model.config
            self._sample_shape = (mc.channels, self.t_size, mc.f_size)
            _check_model(model, (1,) + self._sample_shape, self.t_size, what="t_size")
        self._stepper = None
        self._captures = 0  # of a stepper that is gone (close)
        self._closed = False

    def _check_open(self):
        if self._closed:
            raise ValueError("the pool is closed")

    @property
    def stats(self):
        return dict(self.table.stats, captures=self._stepper.captures if self._stepper is not None else self._captures)

    def submit(self, x, seq, eta=0.0, order=1, noise=None, tau=0.0, corrector=False):
        self._check_open()
        shape = _check_sample(x, self.model)
        want = self._sample_shape or (shape[1], self.t_size, shape[3])
        if shape[1:] != want:
            raise ValueError(f"x of shape {shape} does not fit the pool: expected [n, {want[0]}, {want[1]}, {want[2]}]")
        eta = _check_eta(eta)
        _check_noise(noise, None)
        seq = list(seq)
        if len(seq) > self.table.max_steps:
            raise ValueError(f"len(seq) = {len(seq)} exceeds the pool's max_steps = {self.table.max_steps}")
        rows = request_rows(seq, self.alphas, eta, order, tau, corrector)
        if (eta > 0 or tau > 0) and noise is None:
            raise ValueError("eta > 0 or tau > 0 needs noise= (a NoiseStream): the pool draws on the device and has no host-generator path")
        n = shape[0]
        seed, first = (noise.seed, noise.first_sample) if noise is not None else (0, 0)
        if first + n > _U32:
            raise ValueError(f"first_sample + n = {first + n} exceeds 2^32")
        # ---- device work from here on
        device = self._stepper.xt.device if self._stepper is not None else _device(self.model, x)
        with torch.no_grad(), torch.cuda.device(device):
            if self._stepper is None:
                self._sample_shape = want
                self._stepper = PoolStepper(self.model, self.table, want, device, v_table=_v_table(self.prediction, self.alphas),
                                             threshold=self._threshold)
            xin = torch.empty(shape, dtype=torch.float32, device=device).copy_(x.detach())
            tk = Ticket(n)
            tk._out = torch.empty_like(xin)
        for j in range(n):
            self.table.push(tk, j, rows, seed, first + j, 0, xin[j])
        return tk

    def step(self):
        self._check_open()
        st = self._stepper
        if st is None:
            return []
        with torch.no_grad(), torch.cuda.device(st.xt.device):
            for b, e in self.table.admit():
                st.admit(b, e)
                e.payload = None
            if not self.table.active():
                return []
            st.step()
            finished, tickets = self.table.advance()
            for b, e in finished:  # before the slot can be reused: the next admission is behind this copy in stream order
                e.ticket._out[e.index].copy_(st.xt[b])
        return tickets

    def drain(self):
        """Step until the queue and every slot are empty; returns the tickets completed on the way."""
        out = []
        while self.table.queue or self.table.active():
            out += self.step()
        return out

    def close(self):
        """The graph goes first, then the buffers it points at.  Samples still queued or in a slot are dropped."""
        self._closed = True
        st, self._stepper = self._stepper, None
        if st is not None:
            self._captures = st.captures
            st.close()
        self.table.queue.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
