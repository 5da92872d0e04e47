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
from .sampler import (DDIMStepper, _as_state, _check_eta, _check_model, _check_noise, _device, _host_noise_fn, _prediction, _run,
                      _v_table)
from .schedule import ddim_coefficients, window_plan


class WindowStepper(DDIMStepper):
    """One windowed run's device state: a ``sampler.DDIMStepper`` whose ``xt`` / ``x0`` / ``noise_buf`` are canvas-shaped while
    the network sees the window batch ``win`` (its ``net_in``) -> ``eps`` with ``t`` of N W entries.  ``win`` and the plan tables
    are allocated here, on the launch stream and outside any capture."""

    def __init__(self, model, xt, coef64, window, hop=None, taper="tri", use_graph=True, noise_fn=None, slot=0, fork=True, noise=None,
                 v_table=None):
        if xt.dim() != 4:
            raise ValueError("x must be a [N, C, L, F] tensor")
        n, c, length, f = (int(s) for s in xt.shape)
        hop = window // 2 if hop is None else hop
        plan = window_plan(length, window, hop, taper)
        if f < 4 or f % 4:
            raise ValueError(f"x: the row width F = {f} must be a positive multiple of 4")
        if not 1 <= n * plan.W <= 65535:
            raise ValueError(f"x: N = {n} canvas samples x W = {plan.W} windows = {n * plan.W} outside 1..65535")
        dev = xt.device
        win = torch.empty((n * plan.W, c, int(window), f), dtype=torch.float32, device=dev)
        super().__init__(model, xt, coef64, use_graph=use_graph, noise_fn=noise_fn, slot=slot, fork=fork, noise=noise, net_in=win,
                         v_table=v_table)
        self.win, self.plan, self.geom = win, plan, (n, plan.W, c, length, int(window), int(hop), f)
        self.jfirst = torch.from_numpy(plan.jfirst).to(dev)
        self.cnt = torch.from_numpy(plan.cnt).to(dev)
        self.wt = torch.from_numpy(np.ascontiguousarray(plan.wt)).to(dev)

    def _gather(self, st):
        _lib.check(self.lib.ddimx_window_gather(_lib.ptr(self.xt), _lib.ptr(self.win), *self.geom, st))

    def _update(self, et, noise, st):  # noise: canvas-shaped
        P = _lib.ptr
        _lib.check(self.lib.ddimx_window_update(P(self.xt), P(et), P(noise), P(self.x0), P(self.jfirst), P(self.cnt), P(self.wt),
                                                P(self.coef), P(self.counter), *self.geom, st))


def _validate(x, seq, model, window, hop, taper, eta):
    """Every argument check, before any device work; returns (window, hop)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("x must be a [N, C, L, F] tensor")
    n, _, length, f = (int(s) for s in x.shape)
    if n < 1:
        raise ValueError("x holds no canvas sample")
    if f < 4 or f % 4:
        raise ValueError(f"x: the row width F = {f} must be a positive multiple of 4")
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f"window must be a positive integer, got {window!r}")
    window = int(window)
    _check_model(model, tuple(x.shape), window, batch="N", length="L", what="window", positive="")
    hop = window // 2 if hop is None else hop
    plan = window_plan(length, window, hop, taper)  # hop, L against window and hop, K, taper
    if n * plan.W > 65535:
        raise ValueError(f"x: N = {n} canvas samples x W = {plan.W} windows = {n * plan.W} exceeds 65535")
    _check_eta(eta)
    if len(seq) == 0:
        raise ValueError("seq is empty")
    return window, int(hop)


def windowed_steps(x, seq, model, alphas, select_index, *, window, hop=None, taper="tri", eta=0.0, noise=None, prediction=None):
    """x [N, C, L, F]: the canvas (the starting noise); seq: increasing timesteps; alphas: fp32 alphas-cumprod table; window = T,
    the length the network sees; hop = H in 1..T (default T // 2) with (L - T) % H == 0 and ceil(T / H) <= 8; taper: ``"flat"``
    or ``"tri"`` (``schedule.window_plan``); model: a ``Model`` or any callable ``model(x, t)``, called on the [N W, C, T, F]
    window batch.  Returns (xs, x0_preds) like ``generalized_steps``, canvas-shaped.  ``eta > 0``: the noise of a step is one
    canvas-shaped draw -- ``torch.randn_like`` from torch's generator with eager steps, or with ``noise=`` a ``NoiseStream`` from
    the seeded device stream inside the replayed step (sample index = canvas sample).  ``prediction``: ``"eps"`` or ``"v"``, what
    the network's output is (None: ``model.prediction`` if it has one, else ``"eps"``); every window's v is converted with the
    window's own input before the blend.  Invalid arguments raise ValueError naming the argument before any device work."""
    _check_noise(noise, None)
    prediction = _prediction(model, prediction)
    seq = list(seq)
    window, hop = _validate(x, seq, model, window, hop, taper, eta)
    eta = float(eta)
    coef = ddim_coefficients(seq, alphas, eta)
    device = _device(model, x)
    with torch.no_grad(), torch.cuda.device(device):
        stepper = WindowStepper(model, _as_state(x, device), coef, window, hop, taper, use_graph=(len(seq) >= 4),
                                noise_fn=_host_noise_fn(eta, noise, None), noise=noise, v_table=_v_table(prediction, alphas))
        return _run(stepper, x, select_index)
