"""``RestorePool`` -- a ``SamplerPool`` that also serves restoration requests: gap filling, bandwidth extension, continuing a
clip, in the same slots and the same captured graph as generation.

A restoration request is ``inpaint_solver_steps`` in its replacement-only mode (``guidance=0.0, replace=True``): the network is
evaluated as for sampling -- the inference forward, no tape, no backward -- and after every update the known region is put back
along its exact path kv = cx x_t + w0 y (+ c1 z).  That costs a sampling step, so it fits a pool whose every step is one network
evaluation over all slots: a restoring slot carries, beside what every slot carries, its known clip ``y``, its mask, two more
coefficients per row (cx, w0) and one flag, and the pool's update kernel is ``rpx_pool_update``
(include/features/restore_pool/rpx_restore_pool.h), which reads them.  ``ddimx_pool_begin`` / ``ddimx_pool_end``, the arena's
8-column row and the slot table's 8 words are ``SamplerPool``'s, unchanged; the flag is word 6 of a slot's header row, which
they never read.

The identity contract: a request without ``y`` and ``mask`` is ``SamplerPool``'s request -- ``request_rows``,
the same noise identity, the bits of ``generalized_steps`` / ``dpm_solver_steps`` alone --; a request with them is bit-identical
to ``inpaint_solver_steps(x_j[None], seq, model, alphas, [-1], y=y_j, mask=mask_j, guidance=0.0, replace=True, order=order,
tau=tau, noise=NoiseStream(seed, first_sample + j), prediction=...)`` alone, whatever else the pool serves, whichever slot it
gets and however many slots idle; its final sample equals ``y`` wherever ``mask == 1``.  Every number of a restoring slot's rows
comes from ``schedule.inpaint_solver_coefficients`` and is cast to fp32 as ``InpaintSolverStepper`` casts its table, and the
kernel calls ``step_math.h``'s operations in ``ddimxi_multistep_update``'s order, so the identity holds by construction.

Not built: guidance in the pool (a guided step is the tape-keeping forward and the data-only backward over
ALL slots, about 11.5 ms against 3.3 ms for every request, and nothing pins the tape-keeping forward's eps to the inference
forward's bits, so a generation request's result would depend on its neighbours); windows, inversion and consistency models in
the pool; thresholds or trajectories per request; a ``BrownianStream``; UniC with a mask; skipping idle slots in the forward.

``RestoreTable`` is the host side and, like ``SlotTable``, needs neither the library nor a GPU.
"""
import collections

import numpy as np
import torch

from . import _lib
from .inpaint import _check_known, _known
from .noise import BrownianStream
from .pool import PoolStepper, SamplerPool, SlotTable, Ticket, _U32, request_rows
from .sampler import _check_eta, _check_noise, _check_sample, _device, _v_table
from .schedule import inpaint_solver_coefficients
from .solver import _check_corrector

KNOWN_STRIDE, FLAGS, KNOWN = _lib.RPX_KNOWN_STRIDE, _lib.RPX_FLAGS_WORD, _lib.RPX_KNOWN
_ROW_COLUMNS = [0, 1, 2, 3, 4, 5, 11, 12]  # t, s1, s2, s3, c2, c1, w1, w2 of schedule.inpaint_solver_coefficients
_KNOWN_COLUMNS = [9, 10]  # cx, w0

# What a restoring sample carries through the queue in the place of its tensor (``_Entry.payload``): the sample, its known clip
# and mask (fp32 [C, T, F], or None on a host without a device) and its (cx, w0) rows.
Known = collections.namedtuple("Known", "x y mask rows")


def restore_rows(seq, alpha, order=2, tau=0.0, prediction="eps"):
    """The rows of one restoration request in execution order: (fp32 [len(seq), 8] with the pool's columns (t, s1, s2, s3, c2,
    c1, w1, w2), fp32 [len(seq), 2] with (cx, w0)).  Every number is a column of ``schedule.inpaint_solver_coefficients(seq,
    alpha, order, tau, 0.0, prediction)``, the whole table cast to fp32 the way ``InpaintSolverStepper`` casts it; the final row
    has (cx, w0) = (0, 1).  Raises what that function raises."""
    c = np.ascontiguousarray(inpaint_solver_coefficients(seq, alpha, order, tau, 0.0, prediction), dtype=np.float32)
    return np.ascontiguousarray(c[:, _ROW_COLUMNS]), np.ascontiguousarray(c[:, _KNOWN_COLUMNS])


class RestoreTable(SlotTable):
    """``SlotTable`` plus the image of the second arena, ``known`` (fp32 [slots, max_steps, 2]: a restoring slot's (cx, w0)
    rows), and the flags word of the header rows.  A sample whose payload is a ``Known`` restores: ``admit`` writes its rows
    into ``known`` and ``RPX_KNOWN`` into word 6 of its header row; every other admission leaves that word 0, as ``SlotTable``
    writes it, so a slot that a restoration request has just left serves generation again."""

    def __init__(self, slots, max_steps):
        super().__init__(slots, max_steps)
        self.known = np.zeros((self.slots, self.max_steps, KNOWN_STRIDE), dtype=np.float32)

    def push(self, ticket, index, rows, seed=0, sample=0, draw_base=0, payload=None):
        if isinstance(payload, Known):
            k = np.asarray(payload.rows)
            if k.dtype != np.float32 or k.shape != (np.asarray(rows).shape[0], KNOWN_STRIDE):
                raise ValueError(f"the (cx, w0) rows must be float32 [len, {KNOWN_STRIDE}], one per row of the schedule")
        super().push(ticket, index, rows, seed, sample, draw_base, payload)

    def admit(self):
        out = super().admit()
        for b, e in out:
            if isinstance(e.payload, Known):
                self.known[b, :e.rows.shape[0]] = e.payload.rows
                self.header[b, FLAGS] = KNOWN
        return out


class RestoreStepper(PoolStepper):
    """``PoolStepper`` whose update is ``rpx_pool_update``: beside the pool's buffers it owns ``y`` and ``mask`` (fp32
    [slots, C, T, F]) and ``known`` (the second arena, [slots * max_steps, 2]), allocated here, once, on the launch stream and
    outside any capture, zero-filled.  The captured step points at them, so they live and die with this object like every buffer
    of the base classes (``close`` destroys the graph first).  No kernel reads ``y`` or ``mask`` of a slot that
    is idle or does not restore."""

    def __init__(self, model, table, sample_shape, device, **kw):
        super().__init__(model, table, sample_shape, device, **kw)
        self.y = torch.zeros_like(self.xt)
        self.mask = torch.zeros_like(self.xt)
        self.known = torch.from_numpy(table.known.reshape(-1, KNOWN_STRIDE)).to(device).contiguous()
        self.known_arena = self.known.view(table.slots, table.max_steps, KNOWN_STRIDE)

    def admit(self, b, entry):
        """``PoolStepper.admit``, and for a restoring sample its clip, its mask and its (cx, w0) rows first: the header row, with
        the flag, is the last copy."""
        p = entry.payload
        if isinstance(p, Known):
            self.y[b].copy_(p.y)
            self.mask[b].copy_(p.mask)
            self.known_arena[b, :entry.rows.shape[0]].copy_(torch.from_numpy(np.ascontiguousarray(p.rows)))
            entry.payload = p.x
        super().admit(b, entry)

    def _update(self, et, noise, st):
        P = _lib.ptr
        _lib.check(self.lib.rpx_pool_update(P(self.xt), P(et), P(self.x0), P(self.hist), P(self.y), P(self.mask), P(self.coef),
                                            P(self.known), P(self.slots_dev), *self._shape(), self.per_sample, st))


class RestorePool(SamplerPool):
    """``RestorePool(model, alphas, slots=8, t_size=1024, max_steps=1000, prediction=None)``: see the module docstring.
    ``threshold`` other than None raises ValueError: ``inpaint_solver_steps`` has no threshold to compare a request against.

    ``submit(x, seq, eta=0.0, order=1, noise=None, tau=0.0, corrector=False, y=None, mask=None)``.  Without ``y`` and ``mask``
    it is ``SamplerPool.submit``: the same checks, rows and noise identity.  With both it queues restoration requests: ``y``
    (the known content) and ``mask`` (1 = known; bool, integer or float with values in [0, 1]) follow ``inpaint_steps``' rules,
    are broadcast to ``x`` and are read now, like ``x``; ``order`` 1-3 and ``tau`` >= 0 are ``inpaint_solver_steps``'; ``tau`` > 0
    needs ``noise`` (a ``NoiseStream``), sample j drawing from sample index ``noise.first_sample + j``.  Raised as ValueError
    before any device work, naming the argument: ``y`` without ``mask`` or ``mask`` without ``y``; ``eta`` > 0 with a mask (a
    restoration request takes its noise from ``tau``); ``corrector=True`` with a mask; a ``BrownianStream``; ``tau`` > 0 without
    a ``NoiseStream``.  ``step``, ``drain``, ``stats``, ``close`` and the one captured graph are ``SamplerPool``'s."""

    def __init__(self, model, alphas, slots=8, t_size=1024, max_steps=1000, prediction=None, threshold=None):
        if threshold is not None:
            raise ValueError("RestorePool takes no threshold= (inpaint_solver_steps has none to compare a restoration request against)")
        super().__init__(model, alphas, slots=slots, t_size=t_size, max_steps=max_steps, prediction=prediction)
        self.table = RestoreTable(slots, max_steps)

    def submit(self, x, seq, eta=0.0, order=1, noise=None, tau=0.0, corrector=False, y=None, mask=None):
        # SamplerPool.submit names PoolStepper, so its body is restated here for both kinds of request, in its order
        self._check_open()
        if (y is None) != (mask is None):
            raise ValueError("y= (the known content) and mask= (1 = known) come together: " + ("mask" if mask is None else "y") + " is missing")
        restore = y is not None
        shape = _check_sample(x, self.model)
        want = self._sample_shape or (shape[1], self.t_size, shape[3])
        if shape[1:] != want:
            raise ValueError(f"x of shape {shape} does not fit the pool: expected [n, {want[0]}, {want[1]}, {want[2]}]")
        eta = _check_eta(eta)
        if isinstance(noise, BrownianStream):
            raise ValueError("noise: RestorePool does not take a BrownianStream: give a NoiseStream")
        _check_noise(noise, None)
        seq = list(seq)
        if len(seq) > self.table.max_steps:
            raise ValueError(f"len(seq) = {len(seq)} exceeds the pool's max_steps = {self.table.max_steps}")
        if restore:
            if eta > 0:
                raise ValueError(f"eta = {eta} with a mask: a restoration request takes its noise from tau, eta must be 0")
            if _check_corrector(corrector, 0.0):
                raise ValueError("corrector=True with a mask: UniC is not built for inpainting")
            _check_known(shape, seq, y, mask, 0.0, 0.0, self.alphas, self.prediction, who="RestorePool.submit")
            rows, known = restore_rows(seq, self.alphas, order, tau, self.prediction)
            if tau > 0 and noise is None:
                raise ValueError("tau > 0 needs noise= (a NoiseStream): the pool draws on the device and has no host-generator path")
        else:
            rows, known = request_rows(seq, self.alphas, eta, order, tau, corrector), None
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
                self._stepper = RestoreStepper(self.model, self.table, want, device, v_table=_v_table(self.prediction, self.alphas))
            xin = torch.empty(shape, dtype=torch.float32, device=device).copy_(x.detach())
            if restore:
                yk, m = _known(y.detach(), mask.detach(), shape, device)
            tk = Ticket(n)
            tk._out = torch.empty_like(xin)
        for j in range(n):
            self.table.push(tk, j, rows, seed, first + j, 0, Known(xin[j], yk[j], m[j], known) if restore else xin[j])
        return tk
