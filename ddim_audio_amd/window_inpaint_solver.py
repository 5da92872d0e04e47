"""``windowed_inpaint_solver_steps`` -- multistep (DPM-Solver++, orders 1-3) masked inpainting with reconstruction guidance on a
canvas of any length: ``inpaint_solver_steps``' update, known-region path and folded guidance on ``windowed_inpaint_steps``'
canvas, so a long recording is restored in about 20 network evaluations per window instead of 200.

One long canvas x_t [N, C, L, F] is the only state; y, the mask and the history are canvas-shaped.  Per iteration (row (t, s1, s2,
s3, c2, c1, k1, k2, rho, cx, w0, w1, w2) of ``schedule.inpaint_solver_coefficients``, plan (jfirst, cnt, wt) of
``schedule.window_plan``, m1 and m2 the guided predictions of the two iterations before):

1. gather: the N W windows of length T at hop H (``ddimx_window_gather``);
2. one forward over the [N W, C, T, F] batch -- the inference forward when every rho is 0, else the tape-keeping forward with
   dropout off, on one stream; a v network's output becomes eps per window, with the window's own input;
3. on the canvas e = the blend of eps with the plan's weights, bit for bit ``ddimxw_blend``'s, and m0 = (x_t - s1 e) / s2;
4. guided: r = m (m0 - y), L_n = sum of r^2 per CANVAS sample, canvas seed s = k1 m r;
5. the blend's adjoint hands window j, at its row l - j H, the seed wt[k][l] s[l] (s[l] itself where one window covers l); the
   data-only backward of the window batch on these seeds, once, gives d_win; the gather's adjoint sums d_win over the windows
   that cover l, in ascending window order; g = k2 m r + that sum = d L_n / d x_t, and mt = m0 - rho / sqrt(L_n) g (mt = m0 when
   L_n = 0 or rho = 0);
6. u = [s3 m0 + c2 e] + w0 (mt - m0) + w1 (mt - m1) + w2 (m1 - m2) + c1 z; replace: x_{t-1} = m (cx x_t + w0 y + c1 z) + (1 - m) u,
   the known region on its exact path, which the final row makes y where m = 1; then m2 <- m1, m1 <- mt.

Steps 3-6 run in ``ddimxwis_residual`` / ``ddimxwis_multistep_update`` (include/ddimx_window_inpaint_solver.h has the exact
operation order); a replacement-only step is gather, forward and one launch.  With one window (L = T) the run is
``inpaint_solver_steps`` bit for bit; with an empty mask and rho = 0 it is ``windowed_solver_steps``; with H = T and no guidance
it is ``inpaint_solver_steps`` over the segments as a batch (a guided run is not: the norm belongs to the canvas sample); order 1
without replacement is ``windowed_inpaint_steps`` with zeta = ``schedule.guidance_per_step`` up to rounding.  The whole step
replays as one hipGraph.  Guided WITHOUT replacement is erratic at orders 2-3: the 1 / sqrt(L) normalisation is not smooth where
the residual nearly vanishes (``inpaint_solver``'s docstring, README); use ``replace=True`` with guidance, or order 1.
"""
import torch

from . import _lib
from . import inpaint as _inpaint
from . import window as _window
from .inpaint_solver import InpaintSolverStepper, _refuse
from .sampler import _as_state, _device, _host_noise_fn, _prediction, _run, _v_table
from .schedule import inpaint_solver_coefficients
from .solver import MultistepStepper
from .window import _Windows


class WindowInpaintSolverStepper(_Windows, InpaintSolverStepper):
    """One windowed multistep inpainting run's device state: the window geometry of ``window.WindowStepper`` in front of
    ``inpaint_solver.InpaintSolverStepper``.  ``xt`` / ``y`` / ``mask`` / ``x0`` / ``h1`` / ``h2`` and, guided, the blended eps
    ``beps`` and the norm's partials are canvas-shaped; the network sees ``win`` (its ``net_in``) -> ``eps`` with ``t`` of N W
    entries, and ``seed`` / ``d_x``, the tape and the training workspace are sized for N W windows of length T.  All of it is
    allocated here or in the parents, on the launch stream and outside any capture, and owned by this object; a guided capture
    keeps the model's backward buffers too (``Model.captured_refs(backward=True)``).  A ``NoiseStream`` is an
    identity, as in the parent: z is drawn inside the update kernel for the canvas sample's global index."""

    def __init__(self, model, xt, y, mask, coef64, order, guided, replace, window, hop=None, taper="tri", use_graph=True, noise=None,
                 noise_fn=None, slot=0, fork=True, v_table=None):
        win, plan, geom = self._cut(xt, window, hop, taper)
        for name in _lib.WINDOW_INPAINT_SOLVER_EXPORTS:  # before any allocation: a library without the two functions is refused by name
            getattr(_lib.load(), name)
        super().__init__(model, xt, y, mask, coef64, order, guided, replace, use_graph=use_graph, noise=noise, noise_fn=noise_fn,
                         slot=slot, fork=fork, v_table=v_table, net_in=win)
        self._own(win, plan, geom)
        self.beps = torch.empty_like(xt) if self.guided else None

    def _partials_floats(self):
        return self.lib.ddimxwi_partials_floats(self.xt.size(0), self.per_sample)

    def _residual(self, st):
        P = _lib.ptr
        _lib.check(self.lib.ddimxwis_residual(P(self.xt), P(self.eps), P(self.y), P(self.mask), P(self.x0), P(self.beps), P(self.seed),
                                              P(self.partials), P(self.jfirst), P(self.cnt), P(self.wt), P(self.coef), P(self.counter),
                                              *self.geom, st))

    def _update(self, et, noise, st):  # et: the window batch's eps (guided: blended already, in beps); noise: canvas-shaped
        P = _lib.ptr
        noise, seed, first = MultistepStepper._noise_args(self, noise) if self.stochastic else (None, 0, 0)
        _lib.check(self.lib.ddimxwis_multistep_update(P(self.xt), P(self.beps if self.guided else et), P(noise), P(self.x0), P(self.h1),
                                                      P(self.h2), P(self.y), P(self.mask), P(self.d_x), P(self.partials), P(self.jfirst),
                                                      P(self.cnt), P(self.wt), P(self.coef), P(self.counter), *self.geom, self.flags,
                                                      seed, first, 0, st))


def windowed_inpaint_solver_steps(x, seq, model, alphas, select_index, *, window, hop=None, taper="tri", y=None, mask=None,
                                  guidance=0.0, replace=True, order=2, tau=0.0, noise=None, noise_fn=None, prediction=None,
                                  corrector=False, threshold=None):
    """x [N, C, L, F]: the canvas (the starting noise); seq: strictly increasing timesteps (``schedule.logsnr_seq`` for orders 2
    and 3); the geometry -- ``window`` = T, ``hop`` = H in 1..T (default T // 2) with (L - T) % H == 0 and ceil(T / H) <= 8,
    ``taper`` ``"flat"`` or ``"tri"`` -- is ``windowed_steps``'; y (the known content), mask (1 = known, values in [0, 1]), replace
    and prediction are ``inpaint_steps``', y and mask broadcast to the CANVAS; guidance is ``inpaint_solver_steps``' rho >= 0 (one
    float or one value per iteration in execution order; NOT ``inpaint_steps``' zeta: ``schedule.guidance_per_step`` is the bridge);
    order (1, 2 or 3) and tau (finite, >= 0; 0 is the ODE solver) are ``dpm_solver_steps``'.  With tau > 0 and ``noise=`` a
    ``NoiseStream`` z is drawn inside the update kernel (sample index = canvas sample; no buffer, no fill launch) and the step
    replays from one hipGraph; else it is ``noise_fn(x_t)`` or ``torch.randn_like``, canvas-shaped, and every step runs eagerly.
    model: a ``Model`` (guidance needs one: the tape-keeping forward and the data-only backward) or, without guidance, any callable
    ``model(x, t)``, called on the [N W, C, T, F] window batch.

    Returns (xs, x0_preds) like ``generalized_steps``, canvas-shaped: ``xs[0]`` is the caller's ``x`` (updated in place when it
    already is a contiguous fp32 GPU tensor), ``x0_preds`` the predictions of the blended eps before guidance or replacement; with
    ``replace`` the final canvas equals y where mask = 1.  The norm of the guidance, L_n, is taken per canvas sample, not per
    window.  A guided run keeps the tape of N W windows of length T.  A schedule of 4 or more steps replays one hipGraph unless
    the noise is host-drawn.

    Guidance without replacement is erratic at orders 2-3 (the module's docstring).  Not built, and refused with ValueError: a
    ``BrownianStream``, ``corrector=``, ``threshold=``.  Invalid arguments -- those, ``noise`` together with ``noise_fn``, a bad
    geometry, ``order`` or ``tau``, and ``inpaint_steps``' checks of y, mask and guidance -- raise before any device work
    (TypeError for a ``noise``, y or mask of another type; RuntimeError for guidance with a model that is no ``Model``)."""
    _refuse(noise, noise_fn, corrector, threshold, who="windowed_inpaint_solver_steps")
    prediction = _prediction(model, prediction)
    seq = list(seq)
    window, hop = _window._validate(x, seq, model, window, hop, taper, 0.0)
    _inpaint._check_known(tuple(x.shape), seq, y, mask, guidance, 0.0, alphas, prediction, who="windowed_inpaint_solver_steps")
    coef = inpaint_solver_coefficients(seq, alphas, order, tau, guidance, prediction)
    tau = float(tau)
    guided = bool((coef[:, 8] != 0).any())
    if guided and not hasattr(model, "forward_slot"):
        raise RuntimeError("guided inpainting needs a ddim_audio_amd.Model (tape-keeping forward and data-only backward)")
    device = _device(model, x)
    with torch.no_grad(), torch.cuda.device(device):
        xt = _as_state(x, device)
        yk, m = _inpaint._known(y, mask, tuple(xt.shape), device)
        stepper = WindowInpaintSolverStepper(model, xt, yk, m, coef, int(order), guided, replace, window, hop, taper,
                                             use_graph=(len(seq) >= 4), noise=noise if tau > 0 else None,
                                             noise_fn=_host_noise_fn(tau, noise, noise_fn), v_table=_v_table(prediction, alphas))
        return _run(stepper, x, select_index)
