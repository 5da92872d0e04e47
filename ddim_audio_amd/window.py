"""``windowed_steps`` -- windowed long-form DDIM sampling with overlap-averaged noise predictions on the HIP library.

The reference has no such function; this follows ``generalized_steps``'s conventions (``select_index`` rules, CPU copies at the
selected iterations, ``xs[0]`` is the caller's ``x``, updated in place when it already is a contiguous fp32 GPU tensor).  One long
canvas x_t [N, C, L, F] is the only state.  Per iteration (row (t, s1, s2, s3, c2, c1) of ``schedule.ddim_coefficients``, plan of
``schedule.window_plan``):

1. gather: the canvas is cut into W = (L - T) / H + 1 windows of the network's length T at hop H, window j of canvas sample n
   being sample n W + j of one [N W, C, T, F] batch (``ddimx_window_gather``);
2. eps = eps_theta(windows, t): one forward over that batch, every sample at the length the network was trained at;
3. per canvas row the predictions of the windows that cover it are blended with the row's normalised weights (a partition of
   unity) and the canvas takes one DDIM update, x0 = (x_t - s1 e) / s2, x_{t-1} = s3 x0 + c2 e (+ c1 z), rounded as
   ``ddim_update`` rounds it (``ddimx_window_update``).

All windows read the same canvas value and the update is affine in eps, so blending eps, x0 or x_{t-1} agrees up to rounding; eps
is the cheapest to form.  With one window (L = T) the run is ``generalized_steps`` bit for bit, with H = T it is
``generalized_steps`` over the segments as a batch.  The whole step replays as one hipGraph.
"""
import numpy as np
import torch

from . import _lib
from .sampler import DDIMStepper, _check_noise, _device, _run
from .schedule import ddim_coefficients, window_plan


class WindowStepper(DDIMStepper):
    """One windowed run's device state and its step function: a ``sampler.DDIMStepper`` (first step eager, then one captured
    generic step replayed for every later one, the same ownership of the graph) whose ``xt`` / ``x0`` / ``noise_buf`` are
    canvas-shaped while the network sees the window batch ``win`` -> ``eps`` with ``t`` of N W entries.  Those and the plan
    tables are allocated here, on the launch stream and outside any capture."""

    def __init__(self, model, xt, coef64, window, hop=None, taper="tri", use_graph=True, noise_fn=None, slot=0, fork=True, noise=None):
        if xt.dim() != 4:
            raise ValueError("x must be a [N, C, L, F] tensor")
        n, c, length, f = (int(s) for s in xt.shape)
        hop = window // 2 if hop is None else hop
        plan = window_plan(length, window, hop, taper)
        if f < 4 or f % 4:
            raise ValueError(f"x: the row width F = {f} must be a positive multiple of 4")
        if not 1 <= n * plan.W <= 65535:
            raise ValueError(f"x: N = {n} canvas samples x W = {plan.W} windows = {n * plan.W} outside 1..65535")
        super().__init__(model, xt, coef64, use_graph=use_graph, noise_fn=noise_fn, slot=slot, fork=fork, noise=noise)
        dev = xt.device
        # the base class sized t and eps for a network that sees xt itself; here it sees the window batch
        self.plan, self.geom = plan, (n, plan.W, c, length, int(window), int(hop), f)
        self.win = torch.empty((n * plan.W, c, int(window), f), dtype=torch.float32, device=dev)
        self.t = torch.zeros(n * plan.W, dtype=torch.int64, device=dev)
        self.eps = torch.empty_like(self.win) if self.native else None
        self.jfirst = torch.from_numpy(plan.jfirst).to(dev)
        self.cnt = torch.from_numpy(plan.cnt).to(dev)
        self.wt = torch.from_numpy(np.ascontiguousarray(plan.wt)).to(dev)

    def _prepare(self):
        if self.native:
            dev, t_len = self.win.device, self.win.size(2)
            self.model.prepare(dev, t_len)
            self.model.reserve(dev, self.win.size(0), t_len, self.slot)

    def _launch(self, noise):
        lib, st, P = self.lib, _lib.stream(), _lib.ptr
        xt, t, win = self.xt, self.t, self.win
        _lib.check(lib.ddimx_step_begin(P(self.coef), P(self.counter), P(t), t.numel(), st))
        _lib.check(lib.ddimx_window_gather(P(xt), P(win), *self.geom, st))
        if self.native:
            # as DDIMStepper: eager launches of a graph stepper stay on one stream, the two-shard fork is for the captured step
            fork = self.fork and (not self.use_graph or torch.cuda.is_current_stream_capturing())
            et = self.model(win, t, _slot=self.slot, _fork=fork, _ctx=self._ctx, _out=self.eps)
        else:
            et = self.model(win, t)
            if et.shape != win.shape:
                raise RuntimeError(f"model returned {tuple(et.shape)} for a window batch of {tuple(win.shape)}")
            if et.dtype != torch.float32 or not et.is_contiguous():
                et = et.float().contiguous()
        noise = self._draw(noise)  # canvas-shaped: a NoiseStream fills the stepper's buffer here
        _lib.check(lib.ddimx_window_update(P(xt), P(et), P(noise), P(self.x0), P(self.jfirst), P(self.cnt), P(self.wt), P(self.coef),
                                           P(self.counter), *self.geom, st))
        _lib.check(lib.ddimx_step_end(P(self.counter), st))

    def step(self):
        """``DDIMStepper.step`` with the capture's fork decided by the size of the window batch, which is what the forward sees."""
        if self.graph is not None and self._stale():
            self._drop_graph()
            self._capture_pending = self.use_graph
        if self.graph is not None:
            self.graph.replay()
        else:
            self._prepare()
            self._launch(self.noise_fn(self.xt) if self.noise_fn is not None else None)
            if self._capture_pending and not (self.native and self.model.training):
                self._capture_pending = False
                m = self.model
                fork = self.native and self.fork and m.fork_mask and self.win.size(0) >= 4
                self._capture_graph(lambda: self._launch(None), self.xt.device, self._captured_refs,
                                    fork=m.new_fork_context if fork else None, error_mode="thread_local")
        self.done += 1


def _validate(x, seq, model, window, hop, taper, eta):
    """Every argument check, before any device work; returns (window, hop)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("x must be a [N, C, L, F] tensor")
    n, c, length, f = (int(s) for s in x.shape)
    if n < 1:
        raise ValueError("x holds no canvas sample")
    if f < 4 or f % 4:
        raise ValueError(f"x: the row width F = {f} must be a positive multiple of 4")
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f"window must be a positive integer, got {window!r}")
    window = int(window)
    if hasattr(model, "forward_slot"):
        mc = model.config
        if c != mc.channels or f != mc.f_size:
            raise ValueError(f"x of shape {tuple(x.shape)} does not match the model: expected [N, {mc.channels}, L, {mc.f_size}]")
        step = 1 << (len(mc.ch) - 1)
        if window % step:
            raise ValueError(f"window = {window} must be a multiple of {step} for this model")
    hop = window // 2 if hop is None else hop
    plan = window_plan(length, window, hop, taper)  # hop, L against window and hop, K, taper
    if n * plan.W > 65535:
        raise ValueError(f"x: N = {n} canvas samples x W = {plan.W} windows = {n * plan.W} exceeds 65535")
    eta = float(eta)
    if not np.isfinite(eta) or eta < 0:
        raise ValueError("eta must be finite and >= 0")
    if len(seq) == 0:
        raise ValueError("seq is empty")
    return window, int(hop)


def windowed_steps(x, seq, model, alphas, select_index, *, window, hop=None, taper="tri", eta=0.0, noise=None):
    """x [N, C, L, F]: the canvas (the starting noise); seq: increasing timesteps; alphas: fp32 alphas-cumprod table; window = T,
    the length the network sees; hop = H in 1..T (default T // 2) with (L - T) % H == 0 and ceil(T / H) <= 8; taper: ``"flat"``
    or ``"tri"`` (``schedule.window_plan``); model: a ``Model`` or any callable ``model(x, t)``, called on the [N W, C, T, F]
    window batch.  Returns (xs, x0_preds) like ``generalized_steps``, canvas-shaped.  ``eta > 0``: the noise of a step is one
    canvas-shaped draw -- ``torch.randn_like`` from torch's generator with eager steps, or with ``noise=`` a ``NoiseStream`` from
    the seeded device stream inside the replayed step (sample index = canvas sample).  Invalid arguments raise ValueError naming
    the argument before any device work."""
    _check_noise(noise, None)
    seq = list(seq)
    window, hop = _validate(x, seq, model, window, hop, taper, eta)
    eta = float(eta)
    coef = ddim_coefficients(seq, alphas, eta)
    device = _device(model, x)
    with torch.no_grad(), torch.cuda.device(device):
        xt = x if (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()) else x.to(device, torch.float32).contiguous()
        noise_fn = None
        if eta != 0.0 and noise is None:
            noise_fn = lambda ref: torch.randn_like(ref)  # noqa: E731  (drawn every step, as generalized_steps does)
        stepper = WindowStepper(model, xt, coef, window, hop, taper, use_graph=(len(seq) >= 4), noise_fn=noise_fn, noise=noise)
        return _run(stepper, x, select_index)
