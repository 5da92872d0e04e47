"""``windowed_inpaint_steps`` -- masked DDIM inpainting with reconstruction guidance on a canvas of any length: ``inpaint_steps``'s
known content, mask and guidance on ``windowed_steps``'s canvas, so a long recording is restored with every network evaluation at
the length the network was trained at and with context across the window boundaries.

One long canvas x_t [N, C, L, F] is the only state; y and the mask are canvas-shaped.  Per iteration (row (t, s1, s2, s3, c2, c1,
k1, k2, zeta) of ``schedule.inpaint_coefficients``, plan (jfirst, cnt, wt) of ``schedule.window_plan``):

1. gather: the N W windows of length T at hop H (``ddimx_window_gather``);
2. one forward over the [N W, C, T, F] batch -- the inference forward when every zeta is 0, else the tape-keeping forward with
   dropout off, on one stream; a v network's output becomes eps per window, with the window's own input;
3. on the canvas e = the blend of eps with the plan's weights, bit for bit ``ddimx_window_update``'s, and x0 = (x_t - s1 e) / s2;
4. guided: r = m (x0 - y), L_n = sum of r^2 per CANVAS sample, canvas seed s = k1 m r.  The blend's adjoint hands window j, at its
   row l - j H, the seed wt[k][l] s[l] (s[l] itself where one window covers l); the data-only backward of the window batch on
   these seeds gives d_win; the gather's adjoint sums d_win over the windows that cover l, in ascending window order;
   g = k2 m r + that sum = d L_n / d x_t (the weights are a partition of unity, so k1 and k2 are ``inpaint_steps``'s, for eps and v);
5. u = s3 x0 + c2 e (+ c1 z); guided: u -= zeta / sqrt(L_n) g, skipped where L_n = 0 or zeta = 0;
6. replace: x_{t-1} = m (s3 y + c2 e (+ c1 z)) + (1 - m) u, exactly u where m = 0 and the known path where m = 1.

Steps 3-6 run in ``ddimxwi_residual`` / ``ddimxwi_update`` (include/ddimx_window_inpaint.h); a replacement-only step is gather,
forward and one launch, like ``windowed_steps``'s.  With one window (L = T) the run is ``inpaint_steps`` bit for bit; with an
empty mask and no guidance it is ``windowed_steps``; with H = T and no guidance it is ``inpaint_steps`` over the segments as a
batch (a guided run is not: the norm belongs to the canvas sample).  The whole step replays as one hipGraph.
"""
import torch

from . import _lib
from . import inpaint as _inpaint
from . import window as _window
from .inpaint import InpaintStepper
from .sampler import _as_state, _check_noise, _device, _host_noise_fn, _prediction, _run, _v_table
from .window import _Windows


class WindowInpaintStepper(_Windows, InpaintStepper):
    """One windowed inpainting run's device state: the window geometry of ``window.WindowStepper`` in front of
    ``inpaint.InpaintStepper``.  ``xt`` / ``y`` / ``mask`` / ``x0`` / ``noise_buf`` and, guided, the blended eps ``beps`` and the
    norm's partials are canvas-shaped; the network sees ``win`` (its ``net_in``) -> ``eps`` with ``t`` of N W entries, and ``seed`` /
    ``d_x``, the tape and the training workspace are sized for N W windows of length T.  All of it is allocated here or in the
    parents, on the launch stream and outside any capture, and owned by this object; a guided capture keeps the model's backward
    buffers too (``Model.captured_refs(backward=True)``)."""

    def __init__(self, model, xt, y, mask, coef64, guided, replace, window, hop=None, taper="tri", use_graph=True, noise_fn=None, slot=0,
                 fork=True, noise=None, v_table=None):
        win, plan, geom = self._cut(xt, window, hop, taper)
        super().__init__(model, xt, y, mask, coef64, guided, replace, use_graph=use_graph, noise_fn=noise_fn, slot=slot, fork=fork,
                         noise=noise, v_table=v_table, net_in=win)
        self._own(win, plan, geom)
        self.beps = torch.empty_like(xt) if self.guided else None

    def _partials_floats(self):
        return self.lib.ddimxwi_partials_floats(self.xt.size(0), self.per_sample)

    def _residual(self, st):
        P = _lib.ptr
        _lib.check(self.lib.ddimxwi_residual(P(self.xt), P(self.eps), P(self.y), P(self.mask), P(self.x0), P(self.beps), P(self.seed),
                                             P(self.partials), P(self.jfirst), P(self.cnt), P(self.wt), P(self.coef), P(self.counter),
                                             *self.geom, st))

    def _update(self, et, noise, st):  # et: the window batch's eps (guided: blended already, in beps); noise: canvas-shaped
        P = _lib.ptr
        _lib.check(self.lib.ddimxwi_update(P(self.xt), P(self.beps if self.guided else et), P(noise), P(self.x0), P(self.y), P(self.mask),
                                           P(self.d_x), P(self.partials), P(self.jfirst), P(self.cnt), P(self.wt), P(self.coef),
                                           P(self.counter), *self.geom, self.flags, st))


def windowed_inpaint_steps(x, seq, model, alphas, select_index, *, window, hop=None, taper="tri", y=None, mask=None, guidance=0.0,
                           replace=True, eta=0.0, noise=None, prediction=None):
    """x [N, C, L, F]: the canvas (the starting noise); the geometry -- ``window`` = T, ``hop`` = H in 1..T (default T // 2) with
    (L - T) % H == 0 and ceil(T / H) <= 8, ``taper`` ``"flat"`` or ``"tri"`` -- is ``windowed_steps``'s; y (the known content), mask
    (1 = known, values in [0, 1]), guidance (zeta >= 0, one float or one value per iteration in execution order), replace and
    prediction are ``inpaint_steps``'s, y and mask broadcast to the CANVAS; eta and noise are ``windowed_steps``'s: one
    canvas-shaped draw per step, ``torch.randn_like`` (eager steps) or, with ``noise=`` a ``NoiseStream``, the seeded device stream
    inside the replayed step (sample index = canvas sample).  model: a ``Model`` (guidance needs one: the tape-keeping forward and
    the data-only backward) or, without guidance, any callable ``model(x, t)``, called on the [N W, C, T, F] window batch.

    Returns (xs, x0_preds) like ``generalized_steps``, canvas-shaped: ``xs[0]`` is the caller's ``x`` (updated in place when it
    already is a contiguous fp32 GPU tensor), ``x0_preds`` the predictions of the blended eps before any replacement.  The norm
    of the guidance, L_n, is taken per canvas sample, not per window.  A guided run keeps the tape of N W windows of length T.  A
    schedule of 4 or more steps replays one hipGraph unless the noise is host-drawn.  Invalid arguments raise before any device
    work (ValueError naming the argument; TypeError for a ``noise``, y or mask of another type; RuntimeError for guidance with a
    model that is no ``Model``)."""
    _check_noise(noise, None)
    prediction = _prediction(model, prediction)
    seq = list(seq)
    window, hop = _window._validate(x, seq, model, window, hop, taper, eta)
    coef = _inpaint._check_known(tuple(x.shape), seq, y, mask, guidance, eta, alphas, prediction, who="windowed_inpaint_steps")
    guided = bool((coef[:, 8] != 0).any())
    if guided and not hasattr(model, "forward_slot"):
        raise RuntimeError("guided inpainting needs a ddim_audio_amd.Model (tape-keeping forward and data-only backward)")
    device = _device(model, x)
    with torch.no_grad(), torch.cuda.device(device):
        xt = _as_state(x, device)
        yk, m = _inpaint._known(y, mask, tuple(xt.shape), device)
        stepper = WindowInpaintStepper(model, xt, yk, m, coef, guided, replace, window, hop, taper, use_graph=(len(seq) >= 4),
                                       noise_fn=_host_noise_fn(float(eta), noise, None), noise=noise, v_table=_v_table(prediction, alphas))
        return _run(stepper, x, select_index)
