"""``dpm_solver_steps`` -- DPM-Solver++ multistep sampling (orders 1-3) on the HIP library.

The reference has no such function (its only deterministic sampler is the first-order ``generalized_steps``); this follows that
function's conventions (``select_index`` rules, CPU copies at the selected iterations, ``xs[0]`` is the caller's ``x``, updated
in place when it already is a contiguous fp32 GPU tensor).  The method is DPM-Solver++ in its multistep, data-prediction form
(Lu et al. 2022): the same noise predictor, one evaluation per step, and the x0 predictions of the previous one or two steps
extrapolate the current one.  Per iteration (row (t, s1, s2, s3, c2, c1 = 0, w1, w2) of ``schedule.dpm_coefficients``):

1. eps = eps_theta(x_t, t), the inference forward;
2. m0 = (x_t - s1 eps) / s2, rounded as ``ddim_update`` rounds it;
3. x_{t-1} = [s3 m0 + c2 eps] + w1 (m0 - m1) + w2 (m1 - m2), the bracket being exactly the DDIM update and m1, m2 the
   predictions of the two iterations before; rows of order 1 (the first, and the final jump to t = -1) have w1 = w2 = 0.

Order 1 is ``generalized_steps(eta=0)`` bit for bit.  The gain of orders 2 and 3 needs a step grid that is even in log-SNR:
``schedule.logsnr_seq``.  Steps 2-3 are one libddimx pass (``ddimx_multistep_update``); the whole step replays as one hipGraph.
"""
import numpy as np
import torch

from . import _lib
from .sampler import DDIMStepper, _as_state, _check_sample, _device, _prediction, _run, _threshold, _v_table
from .schedule import dpm_coefficients


class MultistepStepper(DDIMStepper):
    """One multistep run's device state: a ``sampler.DDIMStepper`` whose update also reads and keeps the history
    of x0 predictions: ``x0`` holds the last one between steps, ``hist`` (order 3 only) the one before.  The order of an
    iteration lives in the coefficient table, so the one captured step serves every row."""

    def __init__(self, model, xt, coef64, order, use_graph=True, slot=0, fork=True, v_table=None, threshold=None):
        coef64 = np.asarray(coef64, dtype=np.float64)
        if coef64.ndim != 2 or coef64.shape[1] != _lib.DDIMX_SOLVER_STRIDE:
            raise ValueError(f"coefficient table must be [n_iter, {_lib.DDIMX_SOLVER_STRIDE}] (schedule.dpm_coefficients)")
        if order < 3 and (coef64[:, 7] != 0).any():
            raise ValueError("a table with a second history weight (w2 != 0) needs order = 3")
        super().__init__(model, xt, coef64, use_graph=use_graph, noise_fn=None, slot=slot, fork=fork, v_table=v_table, threshold=threshold)
        self.hist = torch.empty_like(xt) if order >= 3 else None

    def _update(self, et, noise, st):
        xt = self.xt
        _lib.check(self.lib.ddimx_multistep_update(_lib.ptr(xt), _lib.ptr(et), _lib.ptr(self.x0), _lib.ptr(self.hist),
                                                   _lib.ptr(self.coef), _lib.ptr(self.counter), xt.numel(), st))


def dpm_solver_steps(x, seq, model, alpha, select_index, order=2, prediction=None, threshold=None):
    """x [B,C,T,F] (the starting noise); seq: strictly increasing timesteps (``schedule.logsnr_seq`` for orders 2 and 3);
    alpha: fp32 alphas-cumprod table; order: 1, 2 or 3.  Deterministic (no eta).  Returns (xs, x0_preds) like
    ``generalized_steps``: CPU copies of x_{t-1} and of the network's x0 prediction m0 (not the extrapolated one) at the
    selected iterations, ``xs[0]`` the caller's ``x``.  ``prediction``: ``"eps"`` or ``"v"``, what the network's output is (None:
    ``model.prediction`` if it has one, else ``"eps"``).  ``threshold``: None, ``schedule.X0Clip`` or ``schedule.X0Threshold`` -- what
    the data-prediction form is for: m0 is clipped or dynamically thresholded, per sample, before it is extrapolated, so the
    history terms and ``x0_preds`` hold the clipped predictions.  Invalid arguments raise ValueError before any device work."""
    seq = list(seq)
    _check_sample(x, model)
    prediction = _prediction(model, prediction)
    threshold = _threshold(threshold, alpha)
    coef = dpm_coefficients(seq, alpha, order)
    device = _device(model, x)
    with torch.no_grad(), torch.cuda.device(device):
        return _run(MultistepStepper(model, _as_state(x, device), coef, int(order), use_graph=(len(seq) >= 4),
                                     v_table=_v_table(prediction, alpha), threshold=threshold), x, select_index)
