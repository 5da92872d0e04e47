"""``windowed_steps`` -- windowed long-form DDIM sampling with overlap-averaged noise predictions on the HIP library -- and
``windowed_solver_steps``, the same canvas under the DPM-Solver++ multistep update (orders 1-3, deterministic or stochastic).

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
from .noise import BrownianStream
from .sampler import (DDIMStepper, _as_state, _check_eta, _check_model, _check_noise, _device, _host_noise_fn, _prediction, _run,
                      _threshold, _v_table)
from .schedule import brownian_plan, ddim_coefficients, dpm_coefficients, unic_coefficients, window_plan
from .solver import MultistepStepper, _check_corrector, _check_solver_noise


class _Windows:
    """The window geometry of a canvas stepper, in front of its sampler class: ``_cut`` (before the sampler's ``__init__``) checks
    the canvas against the plan and allocates the window batch the network sees, ``_own`` (behind it) puts the plan tables on the
    device -- all on the launch stream and outside any capture --, ``_gather`` cuts the windows out of the canvas every step."""

    @staticmethod
    def _cut(xt, window, hop, taper):
        if xt.dim() != 4:
            raise ValueError("x must be a [N, C, L, F] tensor")
        n, c, length, f = (int(s) for s in xt.shape)
        hop = window // 2 if hop is None else hop
        plan = window_plan(length, window, hop, taper)
        if f < 4 or f % 4:
            raise ValueError(f"x: the row width F = {f} must be a positive multiple of 4")
        if not 1 <= n * plan.W <= 65535:
            raise ValueError(f"x: N = {n} canvas samples x W = {plan.W} windows = {n * plan.W} outside 1..65535")
        win = torch.empty((n * plan.W, c, int(window), f), dtype=torch.float32, device=xt.device)
        return win, plan, (n, plan.W, c, length, int(window), int(hop), f)

    def _own(self, win, plan, geom):
        dev = self.xt.device
        self.win, self.windows, self.geom = win, plan, geom
        self.jfirst = torch.from_numpy(plan.jfirst).to(dev)
        self.cnt = torch.from_numpy(plan.cnt).to(dev)
        self.wt = torch.from_numpy(np.ascontiguousarray(plan.wt)).to(dev)

    def _gather(self, st):
        _lib.check(self.lib.ddimx_window_gather(_lib.ptr(self.xt), _lib.ptr(self.win), *self.geom, st))


class WindowStepper(_Windows, DDIMStepper):
    """One windowed run's device state: a ``sampler.DDIMStepper`` whose ``xt`` / ``x0`` / ``noise_buf`` are canvas-shaped while
    the network sees the window batch ``win`` (its ``net_in``) -> ``eps`` with ``t`` of N W entries.  ``win`` and the plan tables
    are allocated here, on the launch stream and outside any capture."""

    def __init__(self, model, xt, coef64, window, hop=None, taper="tri", use_graph=True, noise_fn=None, slot=0, fork=True, noise=None,
                 v_table=None):
        win, plan, geom = self._cut(xt, window, hop, taper)
        super().__init__(model, xt, coef64, use_graph=use_graph, noise_fn=noise_fn, slot=slot, fork=fork, noise=noise, net_in=win,
                         v_table=v_table)
        self._own(win, plan, geom)
        self.plan = plan

    def _update(self, et, noise, st):  # noise: canvas-shaped
        P = _lib.ptr
        _lib.check(self.lib.ddimx_window_update(P(self.xt), P(et), P(noise), P(self.x0), P(self.jfirst), P(self.cnt), P(self.wt),
                                                P(self.coef), P(self.counter), *self.geom, st))


class WindowSolverStepper(_Windows, MultistepStepper):
    """One windowed multistep run's device state: the window geometry of ``WindowStepper`` in front of the table and history
    handling of ``solver.MultistepStepper``.  ``xt`` / ``x0`` / ``hist`` are canvas-shaped and hold the predictions of the blended
    eps; the network sees ``win`` -> ``eps`` with ``t`` of N W entries, and a v network's output is converted per window, with
    the window's own input, before the blend.

    Two paths to the update.  Fused (``ddimxw_multistep_update``): blend and update in one pass over the canvas, z from the host's
    tensor or drawn in the kernel for a ``NoiseStream``.  Materialised (``ddimxw_blend`` into ``ceps``, canvas-shaped, then the
    parent's update kernels on the canvas) where the blended eps must exist whole before any element is updated: with a
    ``threshold`` -- it acts on the CANVAS: per canvas sample, on the x0 prediction of the blended eps, its rows, histograms and
    rank sized from ``xt`` and its launches on (``xt``, ``ceps``, ``t[:N]``) behind the blend -- and with a ``BrownianStream``,
    whose update kernel keeps its own z source.  ``ceps`` is allocated only then; like ``win``, the plan tables, ``hist`` and the
    Brownian plan it is allocated here, on the launch stream and outside any capture, and owned by this object."""

    def __init__(self, model, xt, coef64, order, window, hop=None, taper="tri", use_graph=True, slot=0, fork=True, v_table=None,
                 threshold=None, noise=None, noise_fn=None, plan=None, folded=False):
        win, wplan, geom = self._cut(xt, window, hop, taper)
        if np.ndim(coef64) == 2 and np.shape(coef64)[1] != _lib.DDIMX_SOLVER_STRIDE:
            raise ValueError(f"coefficient table must be [n_iter, {_lib.DDIMX_SOLVER_STRIDE}]: the canvas kernels read rows of "
                             "schedule.dpm_coefficients (a corrector's table: its first eight columns, folded=True)")
        super().__init__(model, xt, coef64, order, use_graph=use_graph, slot=slot, fork=fork, v_table=v_table, threshold=threshold,
                         noise=noise, noise_fn=noise_fn, plan=plan, net_in=win, folded=folded)
        self._own(win, wplan, geom)
        if not self.native and self.vtab is None:
            self.eps = None  # the threshold's result lands in ceps: nothing window-shaped is needed for another callable's eps
        self.ceps = torch.empty_like(xt) if (self.threshold is not None or self.plan is not None) else None

    def _threshold_in(self):
        return self.xt

    def _to_eps(self, out, st):
        """The v conversion alone, per window; the threshold waits for the blend (``_update``)."""
        return self._v_eps(out, st)

    def _update(self, et, noise, st):  # et: the window batch's eps; noise: canvas-shaped
        P = _lib.ptr
        if self.ceps is not None:
            _lib.check(self.lib.ddimxw_blend(P(et), P(self.ceps), P(self.jfirst), P(self.cnt), P(self.wt), *self.geom, st))
            if self.threshold is not None:
                self._threshold_eps(self.xt, self.ceps, self.ceps, st)
            return super()._update(self.ceps, noise, st)
        seed = first = 0
        if self.stochastic:
            noise, seed, first = self._noise_args(noise)
        _lib.check(self.lib.ddimxw_multistep_update(P(self.xt), P(et), P(noise if self.stochastic else None), P(self.x0), P(self.hist),
                                                    P(self.jfirst), P(self.cnt), P(self.wt), P(self.coef), P(self.counter), *self.geom,
                                                    seed, first, 0, st))


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


def windowed_solver_steps(x, seq, model, alphas, select_index, *, window, hop=None, taper="tri", order=2, tau=0.0, noise=None,
                          noise_fn=None, prediction=None, threshold=None, corrector=False):
    """Windowed long-form sampling with DPM-Solver++ (orders 1-3, ``tau`` > 0: SDE-DPM-Solver++): ``windowed_steps``'s canvas with
    ``dpm_solver_steps``'s update, so a long clip needs about 20 network evaluations per window instead of 200.

    The canvas conventions are ``windowed_steps``'s: x [N, C, L, F], ``window`` = T, ``hop`` = H in 1..T (default T // 2) with
    (L - T) % H == 0 and ceil(T / H) <= 8, ``taper`` ``"flat"`` or ``"tri"``; returns (xs, x0_preds), canvas-shaped, ``xs[0]`` the
    caller's ``x`` (updated in place when it already is a contiguous fp32 GPU tensor); ``select_index`` as there.  The solver
    conventions are ``dpm_solver_steps``'s: seq strictly increasing (``schedule.logsnr_seq`` for orders 2 and 3), the coefficients
    are ``schedule.dpm_coefficients(seq, alphas, order, tau)`` and the start runs at lower order; ``tau`` = 0 is the ODE solver,
    accepts and ignores a given stream and allocates nothing extra; with ``tau`` > 0 ``noise`` is a ``NoiseStream`` (one
    canvas-shaped draw per step, drawn inside the update kernel; sample index = canvas sample) or a ``BrownianStream`` (one path
    per canvas element at any step count), or ``noise_fn(x_t)`` a callable, whose steps run eagerly (neither:
    ``torch.randn_like``).  Per iteration: gather the windows, one forward over the [N W, C, T, F] batch, for ``prediction="v"``
    the conversion of every window's v with its own input, the blend of eps per canvas row with the plan's weights, one multistep
    update of the canvas; ``x0_preds`` and the history hold the predictions of the blended eps.  ``threshold`` (``X0Clip`` /
    ``X0Threshold``) acts on the canvas: per canvas sample, on the x0 prediction of the blended eps, the rank from the canvas
    sample's element count -- not per window.  A schedule of 4 or more steps replays one hipGraph unless the noise is host-drawn.

    With one window (L = T) the run is ``dpm_solver_steps`` bit for bit, with H = T it is ``dpm_solver_steps`` over the segments
    as a batch, and order 1 is ``windowed_steps`` (``tau`` = 0: ``eta`` = 0; ``tau`` = 1 with a ``NoiseStream``: ``eta`` = 1 with
    the same stream).  ``corrector=True`` (``order`` 1 or 2, ``tau`` = 0) is ``dpm_solver_steps(corrector=True)`` on the canvas: the
    folded UniC weights of ``schedule.unic_coefficients`` in the same kernels -- the blend is linear, so the fold holds for the
    blended predictions --, with a canvas-shaped ``hist`` at order 2; ``xs`` holds the predictor's canvases.  Order 3 with a
    corrector is not built for the canvas.  Invalid arguments raise ValueError (TypeError for a ``noise`` of another type) before
    any device work."""
    _check_solver_noise(noise, noise_fn)
    prediction = _prediction(model, prediction)
    threshold = _threshold(threshold, alphas)
    seq = list(seq)
    window, hop = _validate(x, seq, model, window, hop, taper, 0.0)
    coef = dpm_coefficients(seq, alphas, order, tau)
    tau = float(tau)
    if _check_corrector(corrector, tau):
        if order > 2:
            raise ValueError("corrector=True is served at order 1 or 2 on the canvas: its kernels have no third history term")
        coef = unic_coefficients(seq, alphas, order)[:, :_lib.DDIMX_SOLVER_STRIDE]
    plan = brownian_plan(seq, alphas, tau) if tau > 0 and isinstance(noise, BrownianStream) else None
    device = _device(model, x)
    with torch.no_grad(), torch.cuda.device(device):
        stepper = WindowSolverStepper(model, _as_state(x, device), coef, int(order), window, hop, taper, use_graph=(len(seq) >= 4),
                                      v_table=_v_table(prediction, alphas), threshold=threshold, noise=noise if tau > 0 else None,
                                      noise_fn=_host_noise_fn(tau, noise, noise_fn), plan=plan, folded=bool(corrector))
        return _run(stepper, x, select_index)
