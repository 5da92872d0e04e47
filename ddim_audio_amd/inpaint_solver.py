"""``inpaint_solver_steps`` -- multistep (DPM-Solver++, orders 1-3) masked inpainting with reconstruction guidance on the HIP
library: ``inpaint_steps``' problem at ``dpm_solver_steps``' step counts.

The reference has no such function; this follows ``inpaint_steps``' and ``dpm_solver_steps``' conventions (``select_index``
rules, CPU copies at the selected iterations, ``xs[0]`` is the caller's ``x``, updated in place when it already is a contiguous
fp32 GPU tensor).  Stacking the solver's history terms on ``inpaint_steps`` does not raise its order; two things differ here.

* The known region follows its own exact path.  ``inpaint_steps`` puts it back as s3 y + c2 eps, which pairs the true x0 with
  the network's eps for another x0: a first-order replacement whatever the history does.  Here it follows the exact solution
  of the sampler's ODE / SDE for the constant data prediction y, kv = cx x_t + w0 y (+ c1 z) with cx = c2 / s1 and
  w0 = s3 - c2 s2 / s1.
* The guidance lives inside the data prediction.  ``inpaint_steps`` subtracts zeta / sqrt(L) g once per step: an Euler term,
  first order, whose total grows with the number of steps.  Here the prediction itself is moved, mt = m0 - (rho / sqrt(L)) g,
  and the step coefficient and the history both act on mt, so one rho means the same guidance on every grid.  Order 1 of this
  form is ``inpaint_steps``' guided step with zeta_i = rho w0_i (``schedule.guidance_per_step``).

Per iteration (row (t, s1, s2, s3, c2, c1, k1, k2, rho, cx, w0, w1, w2) of ``schedule.inpaint_solver_coefficients``, mask m,
known content y, m1 and m2 the guided predictions of the two iterations before):

1. eps = eps_theta(x_t, t): the inference forward when every rho is 0, else the tape-keeping forward with dropout off;
2. m0 = (x_t - s1 eps) / s2, rounded as ``ddim_update`` rounds it;
3. guided: r = m (m0 - y), L_b = sum of r^2 per sample, g = k2 m r + J_eps^T (k1 m r) = d L_b / d x_t (the data-only backward
   of the seed k1 m r gives the second term), mt = m0 - rho / sqrt(L_b) g (mt = m0 when L_b = 0 or rho = 0);
4. u = [s3 m0 + c2 eps] + w0 (mt - m0) + w1 (mt - m1) + w2 (m1 - m2) + c1 z;
5. replace: x_{t-1} = m (cx x_t + w0 y + c1 z) + (1 - m) u, else u; the final row makes that y where m = 1;
6. m2 <- m1, m1 <- mt: the history holds the guided prediction.

All tensor arithmetic of a step runs in libddimx kernels (``ddimxi_residual`` / ``ddimxi_multistep_update``, the U-Net forward
and its data-only backward; include/ddimx_inpaint_solver.h has the exact operation order); the whole step replays as one
hipGraph.  Guided WITHOUT replacement is erratic at orders 2-3: the 1 / sqrt(L) normalisation is not smooth where the residual
nearly vanishes (README); use ``replace=True`` with guidance, or order 1.
"""
import numpy as np
import torch

from . import _lib
from .inpaint import InpaintStepper, _check_known, _known
from .noise import BrownianStream
from .sampler import _as_state, _check_noise, _check_sample, _device, _host_noise_fn, _prediction, _run, _v_table
from .schedule import inpaint_solver_coefficients
from .solver import MultistepStepper


class InpaintSolverStepper(InpaintStepper):
    """One multistep inpainting run's device state: an ``inpaint.InpaintStepper`` -- its guided forward, tape, training workspace
    and captured references -- whose residual pass and update are ddimxi_residual / ddimxi_multistep_update on the 13-column
    table.  ``x0`` holds the network's prediction m0 of the iteration (the residual pass writes it; what ``x0_preds`` copies),
    ``h1`` the guided prediction of the previous iteration and ``h2`` (order 3 only) the one before: one buffer more than
    ``InpaintStepper``, because the residual pass must not write this step's m0 over last step's guided prediction.  Both are
    owned here like every buffer the captured step points at.

    A table that adds noise (some c1 != 0: ``tau`` > 0) needs ``noise`` (a ``NoiseStream``) or ``noise_fn``, as in
    ``solver.MultistepStepper``: the stream is carried as an identity only -- (seed, first_sample) go to the kernel, which draws for
    the device counter's iteration itself, so there is no fill buffer and no fill launch --; ``noise_fn(x_t)`` is called on the host
    every step, which therefore runs eagerly.  ``net_in`` (None: ``xt``) is ``InpaintStepper``'s: what the network sees, where that
    is not the state (``window_inpaint_solver.WindowInpaintSolverStepper``: the window batch of a canvas)."""

    def __init__(self, model, xt, y, mask, coef64, order, guided, replace, use_graph=True, noise=None, noise_fn=None, slot=0, fork=True,
                 v_table=None, net_in=None):
        coef64 = np.asarray(coef64, dtype=np.float64)
        if coef64.ndim != 2 or coef64.shape[1] != _lib.DDIMXI_STRIDE:
            raise ValueError(f"coefficient table must be [n_iter, {_lib.DDIMXI_STRIDE}] (schedule.inpaint_solver_coefficients)")
        if order not in (1, 2, 3):
            raise ValueError(f"order must be 1, 2 or 3, got {order!r}")
        if (order < 2 and (coef64[:, 11] != 0).any()) or (order < 3 and (coef64[:, 12] != 0).any()):
            raise ValueError("a table with a history weight beyond its order (w1 != 0 at order 1, w2 != 0 below order 3)")
        _check_noise(noise, noise_fn)
        self.stochastic = bool((coef64[:, 5] != 0).any())
        if not self.stochastic:
            noise = noise_fn = None
        elif noise is None and noise_fn is None:
            raise ValueError("a table that adds noise (c1 != 0) needs noise= (a NoiseStream) or noise_fn= (a callable)")
        elif noise is not None and noise.first_sample + xt.size(0) > 1 << 32:
            raise ValueError(f"first_sample + B = {noise.first_sample + xt.size(0)} exceeds 2^32")
        super().__init__(model, xt, y, mask, coef64, guided, replace, use_graph=use_graph, noise_fn=noise_fn, slot=slot, fork=fork,
                         v_table=v_table, net_in=net_in)
        self.noise = noise  # an identity: the base class was given none and owns no fill buffer
        self.h1 = torch.empty_like(xt)
        self.h2 = torch.empty_like(xt) if order >= 3 else None

    def _residual(self, st):
        """m0 (into ``x0``), the seed of the data-only backward and the partials of the norm, from ``eps``."""
        P = _lib.ptr
        _lib.check(self.lib.ddimxi_residual(P(self.xt), P(self.eps), P(self.y), P(self.mask), P(self.x0), P(self.seed), P(self.partials),
                                            P(self.coef), P(self.counter), self.xt.size(0), self.per_sample, st))

    def _update(self, et, noise, st):
        P = _lib.ptr
        noise, seed, first = MultistepStepper._noise_args(self, noise) if self.stochastic else (None, 0, 0)
        _lib.check(self.lib.ddimxi_multistep_update(P(self.xt), P(et), P(noise), P(self.x0), P(self.h1), P(self.h2), P(self.y),
                                                    P(self.mask), P(self.d_x), P(self.partials), P(self.coef), P(self.counter),
                                                    self.xt.size(0), self.per_sample, self.flags, seed, first, 0, st))


def _refuse(noise, noise_fn, corrector, threshold, who="inpaint_solver_steps"):
    """The keywords of the other samplers that this one (and ``windowed_inpaint_solver_steps``) does not take, by name; ``noise``
    against ``noise_fn``."""
    if isinstance(noise, BrownianStream):
        raise ValueError(f"{who} does not take a BrownianStream: give a NoiseStream or noise_fn=")
    if corrector is not False and corrector is not None:
        raise ValueError(f"{who} has no corrector (UniC is not built for inpainting)")
    if threshold is not None:
        raise ValueError(f"{who} has no threshold= (x0 clipping is not built for inpainting)")
    _check_noise(noise, noise_fn)


def inpaint_solver_steps(x, seq, model, alpha, select_index, y=None, mask=None, guidance=0.0, replace=True, order=2, tau=0.0,
                         noise=None, noise_fn=None, prediction=None, corrector=False, threshold=None):
    """x [B,C,T,F] (the starting noise); seq: strictly increasing timesteps (``schedule.logsnr_seq`` for orders 2 and 3); alpha:
    fp32 alphas-cumprod table; y: the known content and mask (1 = known, values in [0, 1], bool / integer / float), both broadcast
    to x; guidance: rho >= 0, one float or one value per iteration in execution order -- the scale of the move of the data
    prediction, the same guidance on every grid (``schedule.guidance_per_step`` gives the ``inpaint_steps`` list that equals it at
    order 1; it is NOT ``inpaint_steps``' zeta); replace: put the known region back along its exact path after every update;
    order: 1, 2 or 3; tau (finite, >= 0): 0 is the ODE solver, > 0 SDE-DPM-Solver++ as in ``dpm_solver_steps`` -- with ``noise=`` a
    ``NoiseStream`` the noise is drawn inside the update kernel and the step replays from one hipGraph (``len(seq)`` >= 4), else it
    is ``torch.randn_like`` or ``noise_fn(x_t)`` and every step runs eagerly.  ``prediction``: ``"eps"`` or ``"v"`` (None:
    ``model.prediction`` if it has one, else ``"eps"``).  Returns (xs, x0_preds) like ``inpaint_steps``: CPU copies of x_{t-1} and
    of the network's x0 prediction (before guidance or replacement) at the selected iterations, ``xs[0]`` the caller's ``x``; with
    ``replace`` the final sample equals y where mask = 1.

    Guidance without replacement is erratic at orders 2-3 (the module's docstring).  Not built, and refused with ValueError: a
    ``BrownianStream``, ``corrector=``, ``threshold=``.  Invalid arguments -- those, ``noise`` together with ``noise_fn``, a bad
    ``order`` or ``tau``, and ``inpaint_steps``' checks of y, mask and guidance -- raise before any device work."""
    _refuse(noise, noise_fn, corrector, threshold)
    prediction = _prediction(model, prediction)
    seq = list(seq)
    _check_known(_check_sample(x, model), seq, y, mask, guidance, 0.0, alpha, prediction, who="inpaint_solver_steps")
    coef = inpaint_solver_coefficients(seq, alpha, order, tau, guidance, prediction)
    tau = float(tau)
    guided = bool((coef[:, 8] != 0).any())
    device = _device(model, x)
    with torch.no_grad(), torch.cuda.device(device):
        xt = _as_state(x, device)
        yk, m = _known(y, mask, tuple(xt.shape), device)
        stepper = InpaintSolverStepper(model, xt, yk, m, coef, int(order), guided, replace, use_graph=(len(seq) >= 4),
                                       noise=noise if tau > 0 else None, noise_fn=_host_noise_fn(tau, noise, noise_fn),
                                       v_table=_v_table(prediction, alpha))
        return _run(stepper, x, select_index)
