"""``dpm_solver_steps`` -- DPM-Solver++ multistep sampling (orders 1-3), deterministic or stochastic, on the HIP library.

The reference has no such function (its only deterministic sampler is the first-order ``generalized_steps``); this follows that
function's conventions (``select_index`` rules, CPU copies at the selected iterations, ``xs[0]`` is the caller's ``x``, updated
in place when it already is a contiguous fp32 GPU tensor).  The method is DPM-Solver++ in its multistep, data-prediction form
(Lu et al. 2022): the same noise predictor, one evaluation per step, and the x0 predictions of the previous one or two steps
extrapolate the current one.  Per iteration (row (t, s1, s2, s3, c2, c1, w1, w2) of ``schedule.dpm_coefficients``):

1. eps = eps_theta(x_t, t), the inference forward;
2. m0 = (x_t - s1 eps) / s2, rounded as ``ddim_update`` rounds it;
3. x_{t-1} = [s3 m0 + c2 eps] + w1 (m0 - m1) + w2 (m1 - m2) + c1 z, the bracket being exactly the DDIM update and m1, m2 the
   predictions of the two iterations before; rows of order 1 (the first, and the final jump to t = -1) have w1 = w2 = 0.

``tau`` = 0 (the default) is the ODE solver: c1 = 0, no noise.  Order 1 is then ``generalized_steps(eta=0)`` bit for bit, and
steps 2-3 are one libddimx pass (``ddimx_multistep_update``).  ``tau`` > 0 is SDE-DPM-Solver++ (the paper's appendix; "DPM++ 2M
SDE" at order 2, "3M SDE" at order 3): every step but the last adds the noise c1 z, which corrects accumulated error; order 1 at
``tau`` = 1 is ``generalized_steps(eta=1)`` bit for bit.  Steps 2-3 are then one pass of ``ddimxs_multistep_update``, which with
a ``NoiseStream`` draws z inside the kernel: no noise buffer, no fill launch.  With a ``BrownianStream`` the pass is
``ddimxb_multistep_update``: z is the normalised increment of one Brownian path between the two levels of the step, evaluated inside
the kernel from the plan table beside the coefficients (``schedule.brownian_plan``), so runs of different step counts from one seed
follow the same path.  The gain of orders 2 and 3 needs a step grid that
is even in log-SNR: ``schedule.logsnr_seq``; order 3 with noise needs about 20 steps or more.  The whole step replays as one
hipGraph (with ``tau`` > 0: when the noise is a ``NoiseStream`` or a ``BrownianStream``).

``corrector=True`` adds the UniC corrector of UniPC (Zhao et al. 2023) to the ODE solver: the prediction m0 that a step makes at
the predicted sample first corrects that sample, and the step then predicts from the corrected one.  Both are linear in the sample
and in the predictions, so the pair folds into the update above with other history weights and one more history term,
w3 (m2 - m3) (``schedule.unic_coefficients``, one pass of ``ddimxu_multistep_update``): one order of accuracy more per evaluation,
no extra forward, no second sample buffer, no extra launch.
"""
import numpy as np
import torch

from . import _lib
from .sampler import (DDIMStepper, _as_state, _check_noise, _check_sample, _device, _host_noise_fn, _prediction, _run, _threshold,
                      _v_table)
from .noise import BrownianStream
from .schedule import BROWNIAN_STRIDE, brownian_plan, dpm_coefficients, unic_coefficients


def _check_solver_noise(noise, noise_fn):
    """``sampler._check_noise`` for the one sampler that also takes a ``BrownianStream``."""
    if not isinstance(noise, BrownianStream):
        return _check_noise(noise, noise_fn)
    if noise_fn is not None:
        raise ValueError("give either noise= (a stream, drawn on the device) or noise_fn= (a callable, eager steps), not both")


def _check_corrector(corrector, tau):
    """``corrector`` if it is a bool and, when True, ``tau`` is 0 (the UniC fold is the ODE solver's), else ValueError."""
    if not isinstance(corrector, (bool, np.bool_)):
        raise ValueError(f"corrector must be True or False, got {corrector!r}")
    if corrector and tau > 0:
        raise ValueError(f"corrector=True needs tau = 0 (got tau = {tau!r}): a stochastic corrector is not built")
    return bool(corrector)


class MultistepStepper(DDIMStepper):
    """One multistep run's device state: a ``sampler.DDIMStepper`` whose update also reads and keeps the history
    of x0 predictions: ``x0`` holds the last one between steps, ``hist`` (order 3 only) the one before.  The order of an
    iteration lives in the coefficient table, so the one captured step serves every row.

    A table without noise (every c1 = 0: ``tau`` = 0) runs ``ddimx_multistep_update`` and ignores ``noise`` / ``noise_fn``.  A table
    with noise runs ``ddimxs_multistep_update`` and needs one of them: ``noise`` (a ``NoiseStream``) is carried here as an
    identity only -- (seed, first_sample) go to the kernel, which draws for the device counter's iteration itself, so the base
    class is given no stream, allocates no fill buffer (``noise_buf`` stays None) and launches no fill -- ; ``noise_fn(x_t)`` is
    called on the host every step, which therefore runs eagerly, and its tensor is what the kernel adds.  ``noise`` a
    ``BrownianStream`` runs ``ddimxb_multistep_update`` and needs ``plan`` (``schedule.brownian_plan`` of the same seq, table and
    tau: int32 [n_iter, BROWNIAN_STRIDE], a non-empty row exactly where c1 != 0); its device copy ``plan`` sits beside ``coef``, is
    indexed by the same counter and is one more buffer the captured step points at (owned here, alive while
    the graph is).

    A table of ``_lib.DDIMXU_STRIDE`` columns (``schedule.unic_coefficients``: the solver with the UniC corrector folded in, a ninth
    column w3) runs ``ddimxu_multistep_update``.  It adds no noise (any c1 != 0 is refused) and its history is as deep as its
    weights: ``hist`` is allocated iff some w2' != 0 (orders 2 and 3), ``hist2`` -- the prediction before ``hist``'s -- iff some
    w3 != 0 (order 3); an order whose table has a weight beyond it (w2' != 0 at order 1, w3 != 0 below order 3) is refused.  Both
    are owned here like every buffer the captured step points at.  ``folded=True`` says that an 8-column table is the first
    eight columns of such a table (orders 1-2, where w3 is 0: what the windowed solver's kernels read): w2 != 0 is then legal
    below order 3 and allocates ``hist``."""

    def __init__(self, model, xt, coef64, order, use_graph=True, slot=0, fork=True, v_table=None, threshold=None, noise=None,
                 noise_fn=None, plan=None, net_in=None, folded=False):
        coef64 = np.asarray(coef64, dtype=np.float64)
        self.corrector = coef64.ndim == 2 and coef64.shape[1] == _lib.DDIMXU_STRIDE
        if coef64.ndim != 2 or (coef64.shape[1] != _lib.DDIMX_SOLVER_STRIDE and not self.corrector):
            raise ValueError(f"coefficient table must be [n_iter, {_lib.DDIMX_SOLVER_STRIDE}] (schedule.dpm_coefficients) or "
                             f"[n_iter, {_lib.DDIMXU_STRIDE}] (schedule.unic_coefficients)")
        if self.corrector:
            if (coef64[:, 5] != 0).any():
                raise ValueError("a corrector table (schedule.unic_coefficients) adds no noise: every c1 must be 0")
            if (order < 2 and (coef64[:, 7] != 0).any()) or (order < 3 and (coef64[:, 8] != 0).any()):
                raise ValueError("a corrector table with a history weight beyond its order (w2' != 0 at order 1, w3 != 0 below order 3)")
        elif order < 3 and (coef64[:, 7] != 0).any() and not folded:
            raise ValueError("a table with a second history weight (w2 != 0) needs order = 3")
        _check_solver_noise(noise, noise_fn)
        self.stochastic = bool((coef64[:, 5] != 0).any())
        brownian = self.stochastic and isinstance(noise, BrownianStream)
        if brownian:
            plan = None if plan is None else np.ascontiguousarray(plan, dtype=np.int32)
            if plan is None or plan.shape != (coef64.shape[0], BROWNIAN_STRIDE):
                raise ValueError(f"a BrownianStream needs plan= [n_iter, {BROWNIAN_STRIDE}] (schedule.brownian_plan)")
            if ((plan[:, 2] > 0) != (coef64[:, 5] != 0)).any():
                raise ValueError("plan must hold a descent exactly in the rows that add noise (c1 != 0)")
        if not self.stochastic:
            noise_fn = None
        elif noise is None and noise_fn is None:
            raise ValueError("a table that adds noise (c1 != 0) needs noise= (a NoiseStream) or noise_fn= (a callable)")
        elif noise is not None and noise.first_sample + xt.size(0) > 1 << 32:
            raise ValueError(f"first_sample + B = {noise.first_sample + xt.size(0)} exceeds 2^32")
        super().__init__(model, xt, coef64, use_graph=use_graph, noise_fn=noise_fn, slot=slot, fork=fork, v_table=v_table, threshold=threshold,
                         net_in=net_in)
        self.noise = noise
        if self.corrector:
            self.hist = torch.empty_like(xt) if (coef64[:, 7] != 0).any() else None
            self.hist2 = torch.empty_like(xt) if (coef64[:, 8] != 0).any() else None
        else:
            self.hist = torch.empty_like(xt) if order >= 3 or (folded and (coef64[:, 7] != 0).any()) else None
            self.hist2 = None
        self.plan = torch.from_numpy(plan).to(xt.device).contiguous() if brownian else None

    def _update(self, et, noise, st):
        xt = self.xt
        if self.corrector:
            _lib.check(self.lib.ddimxu_multistep_update(_lib.ptr(xt), _lib.ptr(et), _lib.ptr(self.x0), _lib.ptr(self.hist),
                                                        _lib.ptr(self.hist2), _lib.ptr(self.coef), _lib.ptr(self.counter), xt.numel(), st))
            return
        if not self.stochastic:
            _lib.check(self.lib.ddimx_multistep_update(_lib.ptr(xt), _lib.ptr(et), _lib.ptr(self.x0), _lib.ptr(self.hist),
                                                       _lib.ptr(self.coef), _lib.ptr(self.counter), xt.numel(), st))
            return
        if self.plan is not None:
            _lib.check(self.lib.ddimxb_multistep_update(_lib.ptr(xt), _lib.ptr(et), _lib.ptr(self.x0), _lib.ptr(self.hist),
                                                        _lib.ptr(self.coef), _lib.ptr(self.plan), _lib.ptr(self.counter), xt.size(0),
                                                        xt[0].numel(), self.noise.seed, self.noise.first_sample, st))
            return
        noise, seed, first = self._noise_args(noise)
        _lib.check(self.lib.ddimxs_multistep_update(_lib.ptr(xt), _lib.ptr(et), _lib.ptr(noise), _lib.ptr(self.x0), _lib.ptr(self.hist),
                                                    _lib.ptr(self.coef), _lib.ptr(self.counter), xt.size(0), xt[0].numel(), seed, first,
                                                    0, st))

    def _noise_args(self, noise):
        """(noise buffer, seed, first_sample) of a stochastic update kernel: the host's tensor, checked and made fp32 on the device,
        or none and the identity of the stream the kernel draws from."""
        if noise is None:
            return None, self.noise.seed, self.noise.first_sample
        xt = self.xt
        if noise.shape != xt.shape:
            raise RuntimeError(f"noise_fn returned {tuple(noise.shape)} for a sample of {tuple(xt.shape)}")
        if noise.dtype != torch.float32 or noise.device != xt.device or not noise.is_contiguous():
            noise = noise.to(xt.device, torch.float32).contiguous()
        return noise, 0, 0


def dpm_solver_steps(x, seq, model, alpha, select_index, order=2, prediction=None, threshold=None, tau=0.0, noise=None, noise_fn=None,
                     corrector=False):
    """x [B,C,T,F] (the starting noise); seq: strictly increasing timesteps (``schedule.logsnr_seq`` for orders 2 and 3);
    alpha: fp32 alphas-cumprod table; order: 1, 2 or 3.  Returns (xs, x0_preds) like ``generalized_steps``: CPU copies of
    x_{t-1} and of the network's x0 prediction m0 (not the extrapolated one) at the selected iterations, ``xs[0]`` the caller's
    ``x``.  ``prediction``: ``"eps"`` or ``"v"``, what the network's output is (None: ``model.prediction`` if it has one, else
    ``"eps"``).  ``threshold``: None, ``schedule.X0Clip`` or ``schedule.X0Threshold`` -- what the data-prediction form is for: m0 is
    clipped or dynamically thresholded, per sample, before it is extrapolated, so the history terms and ``x0_preds`` hold the
    clipped predictions.

    ``tau`` (finite, >= 0) is the amount of noise: 0, the default, is the deterministic ODE solver -- the run is launch for launch
    what it is without the keyword, a given ``noise`` is accepted and unused and nothing extra is allocated.  ``tau`` > 0 is
    SDE-DPM-Solver++ ("DPM++ 2M SDE" / "3M SDE"; ``tau`` = 1 is the usual choice, order 1 at ``tau`` = 1 is
    ``generalized_steps(eta=1)``): every step but the last adds noise.  With ``noise=`` a ``NoiseStream`` it is drawn inside the
    update kernel from the seeded device stream (draw index = the iteration), the step replays from one hipGraph (``len(seq)`` >=
    4, as without noise) and a sample's result depends on (seed, global sample index) only -- not on the batch, the shard or the
    number of GPUs.  Without a stream it is ``torch.randn_like`` from torch's generator, or ``noise_fn(x_t)`` if that keyword is
    given, and every step runs eagerly as in ``generalized_steps``.  Order 3 with ``tau`` > 0 is unstable on coarse grids: use
    about 20 steps or more (order 2 has no such limit).  With a ``NoiseStream`` the noise of a run depends on the number of steps.
    With ``noise=`` a ``noise.BrownianStream`` it does not: the z of a step is the normalised increment [W(u_j) - W(u_i)] /
    sqrt(u_j - u_i) of one Brownian motion per element on the clock u_t = (a_t / (1 - a_t))^tau, evaluated inside the update kernel
    (``schedule.brownian_plan``, ``ddimxb_multistep_update``); increments add up across step grids, so the 20-, 50- and 200-step
    runs of a seed follow one path and converge to one sample as the steps grow.  Graph replay and the independence of batch,
    shard and GPU count are a ``NoiseStream``'s.

    ``corrector`` (a bool): False, the default, is the run above -- the same launches and the same allocations.  True adds the
    UniC corrector of UniPC (``schedule.unic_coefficients``, ``ddimxu_multistep_update``): one order of accuracy more at the same
    number of evaluations and launches (on ``logsnr_seq`` grids of about 20 steps or more; on grids of 8-10 steps it does not help
    order 2).  The corrector is folded into the update, so ``xs`` holds the PREDICTOR's samples, which are
    what the network sees next; the corrected sample is never materialised; and the final sample is the last x0 prediction, as
    without the corrector.  ``prediction="v"`` and ``threshold=`` act on eps before the update as they do without it, so the
    history holds the clipped predictions.  The history is one tensor at order 2 and two at order 3, owned by the stepper; graph
    replay is as without the corrector.  ``corrector=True`` needs ``tau`` = 0: there is no stochastic corrector.

    Invalid arguments -- ``noise`` together with ``noise_fn``, a ``tau`` that is negative or not finite, a ``corrector`` that is
    not a bool or comes with ``tau`` > 0 among them -- raise
    ValueError (TypeError for a ``noise`` that is neither a ``NoiseStream`` nor a ``BrownianStream``) before any device work."""
    seq = list(seq)
    _check_sample(x, model)
    _check_solver_noise(noise, noise_fn)
    prediction = _prediction(model, prediction)
    threshold = _threshold(threshold, alpha)
    coef = dpm_coefficients(seq, alpha, order, tau)
    tau = float(tau)
    if _check_corrector(corrector, tau):
        coef = unic_coefficients(seq, alpha, order)
    plan = brownian_plan(seq, alpha, tau) if tau > 0 and isinstance(noise, BrownianStream) else None
    device = _device(model, x)
    with torch.no_grad(), torch.cuda.device(device):
        return _run(MultistepStepper(model, _as_state(x, device), coef, int(order), use_graph=(len(seq) >= 4),
                                     v_table=_v_table(prediction, alpha), threshold=threshold, noise=noise if tau > 0 else None,
                                     noise_fn=_host_noise_fn(tau, noise, noise_fn), plan=plan), x, select_index)
