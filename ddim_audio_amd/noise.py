"""``NoiseStream`` -- seeded, counter-based Gaussian noise drawn on the device (``ddimx_noise_fill``).

The normal added to element ``i`` of global sample ``s`` at draw ``k`` is a pure function of ``(seed, s, k, i)`` (stream
definition, version 1: Philox4x32-10 words, Box-Muller normals; ``csrc/noise.h``).  Such noise needs no
generator state, so a sampler step that draws it replays from a captured hipGraph (the draw index comes from the device step
counter), and it is the same whatever the batch size, the shard or the number of GPUs.  The object itself is host-only state:
``seed`` and ``first_sample``, the global index of the first sample of the tensors it fills.

``BrownianStream`` -- the same identity read as one Brownian path per element: the noise of a step of
``dpm_solver_steps(tau > 0)`` is the path's normalised increment between the two levels of the step, evaluated inside the update
kernel (``ddimxb_multistep_update``), so runs of 20, 50 and 200 steps from one seed follow the same path.
"""
import torch

from . import _lib

TAG_STEP, TAG_INITIAL, TAG_PATH = 0, 1, 2  # purpose word of the counter: a sampler step's noise | the initial x_T | a path's node
TAG_PROBE = 3  # the Rademacher probe of ``likelihood.log_likelihood`` (signs of the words, drawn by the lkx_ kernels; draw = probe index)
_U32, _U64 = 1 << 32, 1 << 64


def _integer(name, v, hi):
    """``v`` as a Python int in 0 .. hi - 1 (bool and non-integers rejected, as ``schedule.logsnr_seq`` does)."""
    import numpy as np
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    v = int(v)
    if not 0 <= v < hi:
        raise ValueError(f"{name} = {v} outside 0 .. {hi - 1}")
    return v


def _sample_shape(shape):
    """(B, per_sample) of a [B, ...] shape the library accepts."""
    shape = tuple(int(s) for s in shape)
    if len(shape) < 2 or not 1 <= shape[0] <= 65535:
        raise ValueError(f"shape {shape}: need [B, ...] with B in 1..65535")
    per = 1
    for s in shape[1:]:
        per *= s
    if per <= 0 or per % 4:
        raise ValueError("the size of one sample must be a positive multiple of 4 elements")
    if per // 4 > _U32:
        raise ValueError("one sample has more than 2^32 groups of four elements")
    return shape[0], per


class NoiseStream:
    """``NoiseStream(seed, first_sample=0)``: ``seed`` in 0 .. 2^64 - 1, ``first_sample`` in 0 .. 2^32 - 1."""

    def __init__(self, seed, first_sample=0):
        self.seed = _integer("seed", seed, _U64)
        self.first_sample = _integer("first_sample", first_sample, _U32)

    def __repr__(self):
        return f"NoiseStream(seed={self.seed:#x}, first_sample={self.first_sample})"

    def shard(self, lo):
        """The stream of the samples from ``lo`` on: row ``b`` of what it fills is row ``lo + b`` of what this one fills."""
        return NoiseStream(self.seed, self.first_sample + _integer("lo", lo, _U32))

    def for_rank(self, n_total, rank=None, world=None):
        """The stream of this rank's shard of ``n_total`` samples (``dist.shard_bounds``; rank and world size default to
        ``torch.distributed``'s, or to one process, like ``dist.shard_batch``)."""
        from .dist import shard_bounds
        if rank is None:
            import torch.distributed as td
            rank, world = (td.get_rank(), td.get_world_size()) if td.is_available() and td.is_initialized() else (0, 1)
        return self.shard(shard_bounds(_integer("n_total", n_total, _U32), rank, world)[0])

    def fill(self, buf, step_counter=None, draw_base=0, tag=TAG_STEP):
        """Enqueue the fill of ``buf`` ([B, ...], contiguous, fp32: normals; int32 / uint32: the raw words) on the current stream.
        The draw index is ``draw_base + step_counter[0]`` (``step_counter``: a device int32 tensor or None), read when the launch
        runs.  No allocation and no synchronisation: safe inside a graph capture."""
        if not buf.is_cuda or not buf.is_contiguous():
            raise ValueError("buf must be a contiguous GPU tensor")
        if buf.dtype == torch.float32:
            kind = _lib.DDIMX_NOISE_NORMALS
        elif buf.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)):
            kind = _lib.DDIMX_NOISE_WORDS
        else:
            raise ValueError(f"buf must be float32 (normals) or int32 / uint32 (words), got {buf.dtype}")
        b, per = _sample_shape(buf.shape)
        if self.first_sample + b > _U32:
            raise ValueError(f"first_sample + B = {self.first_sample + b} exceeds 2^32")
        if step_counter is not None and (step_counter.dtype != torch.int32 or step_counter.device != buf.device):
            raise ValueError("step_counter must be an int32 tensor on buf's device")
        draw_base, tag = _integer("draw_base", draw_base, _U32), _integer("tag", tag, _U32)
        _lib.check(_lib.load().ddimx_noise_fill(_lib.ptr(buf), b, per, self.seed, self.first_sample, _lib.ptr(step_counter), draw_base,
                                                tag, kind, _lib.stream()))
        return buf

    def _make(self, shape, device, dtype, k, tag):
        device = torch.device(device)
        _sample_shape(shape)
        with torch.cuda.device(device):
            return self.fill(torch.empty(tuple(shape), dtype=dtype, device=device), None, k, tag)

    def initial(self, shape, device):
        """x_T for the samples ``first_sample .. first_sample + B - 1`` (tag 1, draw 0): fp32 ``shape`` on ``device``."""
        return self._make(shape, device, torch.float32, 0, TAG_INITIAL)

    def step_noise(self, shape, k, device):
        """The tensor iteration ``k`` of a sampler adds (tag 0): what the captured step draws, materialised."""
        return self._make(shape, device, torch.float32, k, TAG_STEP)

    def words(self, shape, k, device, tag=TAG_STEP):
        """The raw 32-bit words of draw ``k`` as an int32 tensor of ``shape`` (reinterpret as unsigned: ``.view(torch.uint32)``
        or numpy's ``.view(np.uint32)``)."""
        return self._make(shape, device, torch.int32, k, tag)


class BrownianStream:
    """``BrownianStream(seed, first_sample=0)``: the seeded stream read as one standard Brownian motion W per element, on the clock
    u_t = (a_t / (1 - a_t))^tau of a run (``schedule.brownian_clock``).  P(t) = W(u_t) is a pure function of (seed, global sample,
    element, t) given the table and ``tau``: a virtual Brownian tree over the timestep index whose node n draws the normals of
    counter (group of four, sample, n, tag 2) (``include/ddimx_brownian.h``).  The z of a step from level i to level j is
    [P(j) - P(i)] / sqrt(u_j - u_i): a unit normal, independent across the steps of a run, and additive across step grids --
    which is what makes a preview of few steps preview the final of many.

    A class of its own and no ``NoiseStream``: only ``dpm_solver_steps`` honours a path, and every other sampler keeps refusing
    what is no ``NoiseStream``.  ``initial`` is ``NoiseStream``'s (tag 1), so the same seed starts from the same x_T."""

    def __init__(self, seed, first_sample=0):
        self.seed = _integer("seed", seed, _U64)
        self.first_sample = _integer("first_sample", first_sample, _U32)

    def __repr__(self):
        return f"BrownianStream(seed={self.seed:#x}, first_sample={self.first_sample})"

    def shard(self, lo):
        """The stream of the samples from ``lo`` on (``NoiseStream.shard``)."""
        return BrownianStream(self.seed, self.first_sample + _integer("lo", lo, _U32))

    for_rank = NoiseStream.for_rank  # written on ``shard`` alone

    def initial(self, shape, device):
        """x_T for the samples ``first_sample .. first_sample + B - 1``: ``NoiseStream(seed, first_sample).initial``."""
        return NoiseStream(self.seed, self.first_sample).initial(shape, device)

    def _fill(self, shape, device, row, kind):
        device = torch.device(device)
        b, per = _sample_shape(shape)
        if self.first_sample + b > _U32:
            raise ValueError(f"first_sample + B = {self.first_sample + b} exceeds 2^32")
        with torch.cuda.device(device):
            out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
            row = torch.from_numpy(row).to(device)  # freed behind the launch: the allocator orders it on this stream
            _lib.check(_lib.load().ddimxb_path_fill(_lib.ptr(out), b, per, self.seed, self.first_sample, _lib.ptr(row), kind,
                                                    _lib.stream()))
        return out

    def path(self, shape, t, alpha, tau, device):
        """P(t) = W(u_t) for timestep ``t`` of the table ``alpha`` at ``tau`` > 0: fp32 ``shape`` on ``device``, the bits the update
        kernel works with."""
        from .schedule import brownian_clock, brownian_row
        return self._fill(shape, device, brownian_row(brownian_clock(alpha, tau), None, t), _lib.DDIMXB_PATH)

    def increment(self, shape, i, j, alpha, tau, device):
        """The z of the step from level ``i`` down to level ``j`` < ``i``: [P(j) - P(i)] / sqrt(u_j - u_i), what the update kernel
        adds c1 times on that step."""
        from .schedule import brownian_clock, brownian_row
        return self._fill(shape, device, brownian_row(brownian_clock(alpha, tau), i, j), _lib.DDIMXB_INCREMENT)
