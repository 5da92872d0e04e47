"""``invert_steps`` / ``slerp`` -- DDIM inversion with fixed-point refinement, and spherical interpolation of latents.

``invert_steps`` runs the deterministic sampler the other way: from a clip (alphas-cumprod 1) up ``seq`` to the latent that
``generalized_steps(eta=0)`` on the same ``seq`` turns back into it.  The reference has no such function; this follows
``generalized_steps``'s conventions (``select_index`` rules, CPU copies, ``xs[0]`` is the caller's ``x``, updated in place when
it already is a contiguous fp32 GPU tensor).  Level i = seq[k], the level below it j = seq[k-1] (j = -1, the data, for k = 0).
The decoder's step from i down to j is x_j = s3_j (x_i - s1_i e) / s2_i + c2_j e with e = eps_theta(x_i, t_i); solved for x_i
with e held fixed it is x_i = p x_j + q e (p = sqrt(a_i / a_j), q = s1_i - p c2_j, ``schedule.invert_coefficients``).  As e
depends on x_i the inverse is implicit, and one level solves it by a fixed number of fixed-point iterations:

    base = x_j;  cand_0 = base;  for m = 1..iters:  e = eps_theta(cand_{m-1}, t_i);  cand_m = p base + q e;    x_i = cand_iters

``iters = 1`` is the usual ("naive") inversion: the network evaluated at the target timestep on the point below.  ``iters`` ->
infinity is the exact inverse of the decoder wherever the map contracts; the residual |cand_m - cand_{m-1}| / |cand_m| of every
iteration is logged per sample so a caller can see whether it does.  ``iters`` is fixed per call -- no data-dependent stopping --
so every network evaluation is the same step (timestep fill, forward, ``ddimx_invert_update``, counter advance) and replays
from one hipGraph; the network is evaluated len(seq) * iters times, always at a timestep of ``seq``.

``slerp`` is the reference's interpolation between two latents (``runners/diffusion.py:427-432``) per pair and on the device
(``ddimx_slerp``), ready for ``generalized_steps``.
"""
import numpy as np
import torch

from . import _lib
from .sampler import DDIMStepper, _as_state, _check_sample, _device, _prediction, _run, _v_table
from .schedule import invert_coefficients


class InvertStepper(DDIMStepper):
    """One inversion run's device state: a ``sampler.DDIMStepper`` whose step is one NETWORK EVALUATION -- one row
    of ``schedule.invert_coefficients`` -- and whose update keeps the level's base point: ``base`` holds x_j from the first
    evaluation of a level to its last, ``log`` [rows, B] the residual of every evaluation.  Whether a row starts a level lives in
    the coefficient table, so the one captured step serves every row.  ``base``, ``log`` and the reduction's partials are
    allocated here, on the launch stream and outside any capture, like ``eps``."""

    def __init__(self, model, xt, coef64, use_graph=True, slot=0, fork=True, v_table=None):
        coef64 = np.asarray(coef64, dtype=np.float64)
        if coef64.ndim != 2 or coef64.shape[0] < 1 or coef64.shape[1] != _lib.DDIMX_INVERT_STRIDE:
            raise ValueError(f"coefficient table must be [rows, {_lib.DDIMX_INVERT_STRIDE}] (schedule.invert_coefficients)")
        if coef64[0, 5] == 0:
            raise ValueError("the first row of the table must start a level (first = 1)")
        super().__init__(model, xt, coef64, use_graph=use_graph, noise_fn=None, slot=slot, fork=fork, v_table=v_table)
        self.b, self.per_sample = xt.size(0), xt[0].numel()
        n = int(self.lib.ddimx_invert_partials_doubles(self.b, self.per_sample))
        if n <= 0:
            raise RuntimeError("libddimx: bad inversion partials size for B=%d" % self.b)
        self.base = torch.empty_like(xt)
        self.partials = torch.empty(n, dtype=torch.float64, device=xt.device)
        self.log = torch.zeros((self.n_iter, self.b), dtype=torch.float32, device=xt.device)

    def _update(self, et, noise, st):
        P = _lib.ptr
        _lib.check(self.lib.ddimx_invert_update(P(self.xt), P(et), P(self.base), P(self.x0), P(self.partials), P(self.log), self.n_iter,
                                                P(self.coef), P(self.counter), self.b, self.per_sample, st))


def invert_steps(x, seq, model, alpha, select_index, iters=1, stats=None, prediction=None):
    """x [B,C,T,F]: the clip (alphas-cumprod 1); seq: strictly increasing timesteps, walked upwards; alpha: fp32 alphas-cumprod
    table; iters: fixed-point iterations per level, an integer in 1..16 (1 = naive inversion).  Returns (xs, x0_preds) like
    ``generalized_steps``: ``xs[0]`` the caller's ``x`` (updated in place when it already is a contiguous fp32 GPU tensor), then
    CPU copies of the latent at the selected LEVELS -- ``select_index`` counts levels, not network evaluations (None = all,
    negative allowed); the copy is taken after the level's last iteration, and ``x0_preds`` holds that last evaluation's x0
    prediction.  With ``select_index=[-1]``, ``xs[-1]`` is the latent at ``seq[-1]``: ``generalized_steps(xs[-1], seq, ...,
    eta=0)`` decodes it.  If ``stats`` is a dict it receives ``stats["residual"]``, a CPU fp32 tensor [len(seq), iters, B]: the
    residual |cand_m - cand_{m-1}|_2 / |cand_m|_2 of every iteration, copied once after the run.  ``prediction``: ``"eps"`` or
    ``"v"``, what the network's output is (None: ``model.prediction`` if it has one, else ``"eps"``).  Invalid arguments raise
    ValueError before any device work."""
    seq = list(seq)
    _check_sample(x, model)
    prediction = _prediction(model, prediction)
    coef = invert_coefficients(seq, alpha, iters)
    if stats is not None and not isinstance(stats, dict):
        raise ValueError("stats must be a dict or None")
    iters = int(iters)
    device = _device(model, x)
    with torch.no_grad(), torch.cuda.device(device):
        def keep_log(stepper):
            stats["residual"] = stepper.log.to("cpu").view(len(seq), iters, x.size(0))

        stepper = InvertStepper(model, _as_state(x, device), coef, use_graph=(coef.shape[0] >= 4), v_table=_v_table(prediction, alpha))
        return _run(stepper, x, select_index, per=iters, finish=keep_log if stats is not None else None)


def slerp(z1, z2, weights):
    """Spherical interpolation between latents: z1, z2 [P, C, T, F] (P pairs), weights a 1-D sequence of M finite floats; returns
    a contiguous fp32 GPU tensor [P * M, C, T, F], pair-major (row p M + m is pair p at weights[m]), ready for
    ``generalized_steps``.  Per pair, cos(theta) = <z1, z2> / (|z1| |z2|) over the whole sample (what the reference computes for
    its batch of one) and out = sin((1 - w) theta) / sin(theta) z1 + sin(w theta) / sin(theta) z2; the weights are rounded once
    to fp32 and those values are the w of the formula.  w = 0 returns z1 and w = 1 returns z2 exactly.  A fix, not the
    reference's behaviour: where its formula yields NaN (sin(theta) = 0: parallel or all-zero inputs) the result is the straight
    line (1 - w) z1 + w z2.  Raises ValueError for a shape mismatch, empty or non-finite weights, or a sample whose element
    count is not a multiple of 4."""
    if not isinstance(z1, torch.Tensor) or not isinstance(z2, torch.Tensor) or z1.dim() != 4:
        raise ValueError("z1 and z2 must be [P, C, T, F] tensors")
    if tuple(z1.shape) != tuple(z2.shape):
        raise ValueError(f"z1 of shape {tuple(z1.shape)} and z2 of shape {tuple(z2.shape)} differ")
    try:
        w = np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("weights must be a 1-D sequence of floats") from None
    if w.ndim != 1 or w.size == 0:
        raise ValueError("weights must be a non-empty 1-D sequence of floats")
    if not np.isfinite(w).all() or not np.isfinite(w.astype(np.float32)).all():
        raise ValueError("weights must be finite")
    pairs, per_sample = z1.size(0), z1[0].numel() if z1.size(0) else 0
    if not 1 <= pairs <= 65535:
        raise ValueError(f"number of pairs {pairs} outside 1..65535")
    if per_sample == 0 or per_sample % 4:
        raise ValueError("the size of one sample (C * T * F) must be a positive multiple of 4 elements")
    lib = _lib.load()
    device = z1.device if z1.is_cuda else z2.device if z2.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.no_grad(), torch.cuda.device(device):
        a, b = (z.to(device, torch.float32).contiguous() for z in (z1, z2))
        wd = torch.from_numpy(w.astype(np.float32)).to(device)
        out = torch.empty((pairs * w.size,) + tuple(z1.shape[1:]), dtype=torch.float32, device=device)
        partials = torch.empty(int(lib.ddimx_invert_partials_doubles(pairs, per_sample)), dtype=torch.float64, device=device)
        _lib.check(lib.ddimx_slerp(_lib.ptr(a), _lib.ptr(b), _lib.ptr(wd), int(w.size), _lib.ptr(out), _lib.ptr(partials), pairs,
                                   per_sample, _lib.stream()))
    return out
