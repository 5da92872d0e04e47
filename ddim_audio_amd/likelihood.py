"""``log_likelihood`` -- the exact log-likelihood of data under a diffusion model, in nats and bits/dim, along the
probability-flow ODE (Song et al. 2021, section 4.3 and appendix D.2) with the Skilling-Hutchinson trace estimator (Grathwohl
et al. 2019); kernels in include/features/lkx_likelihood.h.

With abar the cumulative-alpha entry of a level, alpha = sqrt(abar), sigma = sqrt(1 - abar), s = sigma / alpha and u = x / alpha
the DDIM ODE is du/ds = eps_theta(alpha u, t), and the instantaneous change of variables gives

    log p_{t0}(x_0) = log N(x_T; 0, I) + D log(alpha_T / alpha_0) + integral over s of alpha(s) tr J_eps(x(s), t(s)) ds

D the number of elements of a sample.  tr J_eps is estimated as r . (J_eps^T r) with one fixed Rademacher probe r per trajectory;
J_eps^T r is the data-only backward of the seed r.  The timestep embedding is a table lookup, so the network exists at integer t
only: the integrator walks the levels of an increasing ``seq`` from ``seq[0]`` up to ``seq[-1]`` and never evaluates between
them.  ``order=1`` is Euler (one evaluation per interval), ``order=2`` Heun (two); the variable is s, in which the ODE's right-hand
side is eps alone -- a log-SNR grid or the data-prediction form integrate this worse (README), so neither is offered.

Every evaluation is one row of ``schedule.likelihood_coefficients`` and one pass of two kernels: ``lkx_stage`` (the state update,
the next network input and the per-block sums of r . g in double) and ``lkx_finish`` (the quadrature weight, read from a table of
doubles, times the sample's sum, added to its accumulator).  A ``ddim_audio_amd.Model`` runs the tape-keeping forward with dropout
off, the v -> eps conversion and the data-only backward of the probe on one stream, captured once with the two kernels into a
hipGraph that replays for every row; no autograd, parameter ``.grad``, flat gradient buffer, all-reduce hook or dropout counter is
touched.  Any other callable gives eps from its call and g from ``torch.autograd.grad``; the steps then run eagerly through the same
kernels.  Not built: adaptive step size, Gaussian probes, likelihood in ``SamplerPool``, the variational bound, a canvas longer
than the training length (windows).
"""
import collections
import math

import numpy as np
import torch

from . import _lib, sampler
from .model import _unet_bwd, _unet_fwd_train
from .schedule import likelihood_coefficients

Likelihood = collections.namedtuple("Likelihood", "logp bpd stderr latent")


class LikelihoodStepper(sampler.DDIMStepper):
    """``DDIMStepper`` on ``schedule.likelihood_coefficients`` rows, one ``step()`` per network evaluation.  ``xt`` is the network's
    input ``xin`` [K B, C, T, F] (probe-major: rows k B .. k B + B - 1 are the B samples under probe k), ``u`` the ODE state, the
    base class's ``x0`` buffer holds k1, ``acc`` [K B] the float64 integral.  The forward of a native model is
    ``InpaintStepper``'s guided one -- tape-keeping forward (dropout p = 0), v -> eps, data-only backward of the probe ``r`` into
    ``d_x`` -- and its capture keeps ``Model.captured_refs(backward=True)``; a callable's is its call under ``enable_grad`` and
    ``torch.autograd.grad(out, x, r)``, eager.  The update is one ``lkx_stage`` per probe (each on its B rows, with its probe
    index) and one ``lkx_finish``."""

    def __init__(self, model, xin, u, table, probes, seed, first_sample, v_table=None, use_graph=True):
        native = hasattr(model, "forward_slot")
        super().__init__(model, xin, table.rows, use_graph=use_graph and native, fork=False, v_table=v_table)
        dev, lib = xin.device, self.lib
        self.u, self.k1 = u, self.x0
        self.probes, self.b = int(probes), xin.size(0) // int(probes)
        self.seed, self.first_sample = seed, first_sample
        self.per_sample, self.t_len = xin[0].numel(), xin.size(2)
        self.wd = torch.from_numpy(np.ascontiguousarray(table.wd, dtype=np.float64)).to(dev)
        self.acc = torch.zeros(xin.size(0), dtype=torch.float64, device=dev)
        self.blocks = int(lib.lkx_partials_doubles(1, self.per_sample))
        if self.blocks <= 0:
            raise RuntimeError("libddimx: bad likelihood partials size for per_sample=%d" % self.per_sample)
        self.partials = torch.empty(xin.size(0) * self.blocks, dtype=torch.float64, device=dev)
        self.r, self.d_x = torch.empty_like(xin), (torch.empty_like(xin) if native else None)
        for k in range(self.probes):
            _lib.check(lib.lkx_probe_fill(_lib.ptr(self._rows(self.r, k)), self.b, self.per_sample, seed, first_sample, k, _lib.stream()))
        self.tape = self.ws = None

    def _rows(self, buf, k):
        """The B rows of probe ``k`` of a [K B, ...] buffer (a view)."""
        return buf[k * self.b:(k + 1) * self.b]

    def _prepare(self):
        if not self.native:
            return
        m, dev, lib = self.model, self.xt.device, self.lib
        m.prepare(dev, self.t_len)
        m._ensure_packed_bwd(lib, dev)
        if self.tape is None:
            n = self.xt.size(0)
            self.tape = torch.empty(int(lib.ddimx_train_tape_bytes(m._handle, n, self.t_len)), dtype=torch.uint8, device=dev)
            self.ws = torch.empty(int(lib.ddimx_train_workspace_bytes(m._handle, n, self.t_len)), dtype=torch.uint8, device=dev)

    def _forward(self):
        x, t, m = self.xt, self.t, self.model
        if self.native:
            tables = m._ensure_tables(self.t_len, x.device)
            _unet_fwd_train(m, tables, self.ws, self.tape, x, t, self.eps)
            self._v_eps(self.eps, _lib.stream())
            _unet_bwd(m, tables, self.ws, self.tape, x, t, self.r, d_x=self.d_x, data_only=True)
            return self.eps
        with torch.enable_grad():
            xg = x.detach().requires_grad_(True)
            out = m(xg, t)
            if out.shape != x.shape:
                raise RuntimeError(f"model returned {tuple(out.shape)} for an input of {tuple(x.shape)}")
            g, = torch.autograd.grad(out, xg, self.r.to(out.dtype))
        self.d_x = g.detach().float().contiguous()
        return self._v_eps(out.detach().float().contiguous(), _lib.stream())

    def _to_eps(self, out, st):
        return out  # the forward has converted already (the seed is the gradient w.r.t. the network's own output)

    def _update(self, et, noise, st):
        P, lib = _lib.ptr, self.lib
        for k in range(self.probes):
            s = lambda buf: P(self._rows(buf, k))
            _lib.check(lib.lkx_stage(s(self.u), s(self.k1), s(et), s(self.d_x), s(self.xt), P(self.partials[k * self.b * self.blocks:]),
                                     P(self.coef), P(self.counter), self.b, self.per_sample, self.seed, self.first_sample, k, st))
        _lib.check(lib.lkx_finish(P(self.partials), P(self.acc), P(self.wd), P(self.counter), self.xt.size(0), self.blocks, st))

    def _captured_refs(self):
        return self.model.captured_refs(backward=True) if self.native else None

    def divergence(self):
        """r . g of the evaluation just run, per network row, float64 on the host (the partials summed in block order)."""
        return self.partials.view(self.xt.size(0), self.blocks).cpu().numpy().cumsum(axis=1)[:, -1].copy()


def _abar(alphas, t):
    """abar of level ``t`` as ``schedule.v_table`` reads it: the fp32 table's value as a Python double."""
    return float(torch.as_tensor(alphas).to("cpu", torch.float32).reshape(-1)[int(t)])


def _check_x(x, model):
    shape = sampler._check_sample(x, model)
    if not x.dtype.is_floating_point:
        raise ValueError("x must be a floating-point tensor")
    return shape


def log_likelihood(x, seq, model, alphas, order=2, probes=1, noise=None, prediction=None, stats=None, **kwargs):
    """log p(x) of every sample of ``x`` [B, C, T, F] under ``model`` on the increasing levels ``seq`` (at least 2), as
    ``Likelihood(logp, bpd, stderr, latent)``:

    ``logp``   float64 [B] (CPU), nats: the density of the MODEL'S MARGINAL AT LEVEL ``seq[0]``, in the network's own data scale.
               Any dequantisation or data-scaling offset is the caller's.
    ``bpd``    -logp / (D ln 2), D = C T F.
    ``stderr`` the standard error of ``logp`` over the probes; NaN for ``probes=1``.
    ``latent`` x_T, the ODE latent of every sample, fp32 [B, C, T, F] on the GPU.

    ``seq[-1]`` should be the table's last level: the prior term takes x_T for N(0, I), which is wrong by more than the
    integration error anywhere below it.  ``order``: 1 (Euler, ``len(seq) - 1`` evaluations) or 2 (Heun, twice that; second order:
    README has the measured convergence).  ``probes=K`` repeats every sample K times along the network batch with probe indices
    0 .. K-1; the kernels are batch-invariant, so the K trajectories are bit-identical and only the divergence estimates differ;
    ``logp`` is their mean.  ``noise``: a ``NoiseStream`` whose seed and ``first_sample`` (``for_rank``) key the probes -- nothing
    is drawn from it otherwise; None means seed 0.  A sample's result depends on (seed, global sample index, probe index) only,
    whatever the batch or the shard.  ``prediction``: ``"eps"`` or ``"v"`` (None: the model's own, else ``"eps"``).
    ``model``: a ``ddim_audio_amd.Model`` in eval mode (one hipGraph, replayed per evaluation) or any differentiable callable
    ``model(x, t)`` (eager, g by ``torch.autograd.grad``).  ``stats``: a dict that receives ``divergence`` (float64
    [rows, K B], r . g per evaluation and network row, probe-major), ``evaluations``, ``captures`` (graph captures of the run) and
    ``latents`` (x_T of every probe's trajectory, fp32 [K, B, C, T, F] on the GPU).
    Refused before any device work: a ``BrownianStream`` or anything else that is no ``NoiseStream`` (TypeError), ``threshold=``
    and windows (ValueError), any other keyword (TypeError), a bad ``seq`` / ``order`` / ``probes`` / ``x`` (ValueError)."""
    if kwargs.get("threshold") is not None:
        raise ValueError("log_likelihood has no threshold=: a clipped x0 prediction has no density")
    kwargs.pop("threshold", None)
    for name in ("window", "windows", "hop", "taper"):
        if kwargs.get(name) is not None:
            raise ValueError(f"log_likelihood has no {name}=: the likelihood of a canvas longer than the training length is not built")
        kwargs.pop(name, None)
    if kwargs:
        raise TypeError(f"log_likelihood got unexpected keyword arguments {sorted(kwargs)}")
    sampler._check_noise(noise, None)
    prediction = sampler._prediction(model, prediction)
    if isinstance(probes, bool) or not isinstance(probes, (int, np.integer)) or probes < 1:
        raise ValueError(f"probes must be a positive integer, got {probes!r}")
    if stats is not None and not isinstance(stats, dict):
        raise ValueError("stats must be a dict or None")
    table = likelihood_coefficients(list(seq), alphas, order, prediction)
    shape = _check_x(x, model)
    b, k_probes = shape[0], int(probes)
    if b * k_probes > 65535:
        raise ValueError(f"B * probes = {b * k_probes} exceeds 65535 network rows")
    native = hasattr(model, "forward_slot")
    if native and model.training:
        raise ValueError("the model must be in eval mode (model.eval()): dropout is no part of the density")
    seed, first = (noise.seed, noise.first_sample) if noise is not None else (0, 0)
    if first + b > 1 << 32:
        raise ValueError(f"first_sample + B = {first + b} exceeds 2^32")
    _lib.load()
    device = sampler._device(model, x)
    d = x[0].numel()
    a0 = float(np.float32(_abar(alphas, table.rows[0, 0]) ** -0.5))  # rn(1 / alpha_0): u_0 = rn(x rn(1 / alpha_0))
    with torch.no_grad(), torch.cuda.device(device):
        xin = x.detach().to(device, torch.float32).repeat(k_probes, 1, 1, 1).contiguous()  # a copy: x is not written
        u = torch.mul(xin, a0)
        stepper = LikelihoodStepper(model, xin, u, table, k_probes, seed, first, v_table=sampler._v_table(prediction, alphas),
                                    use_graph=(table.rows.shape[0] >= 4))
        try:
            div = []
            for _ in range(stepper.n_iter):
                stepper.step()
                if stats is not None:
                    div.append(stepper.divergence())
            captures = stepper.captures
            sq = torch.empty(b * k_probes, dtype=torch.float64, device=device)
            _lib.check(stepper.lib.lkx_sumsq(_lib.ptr(xin), _lib.ptr(stepper.partials), _lib.ptr(sq), b * k_probes, d, _lib.stream()))
            acc, sq = stepper.acc.cpu().numpy(), sq.cpu().numpy()
            latent = xin[:b].clone()
            if stats is not None:
                stats["latents"] = xin.view(k_probes, *shape).clone()
        finally:
            stepper.close()
    per = (-0.5 * sq - 0.5 * d * math.log(2.0 * math.pi) + d * table.logdet_per_dim + acc + d * table.trace_per_dim).reshape(k_probes, b)
    logp = per.mean(axis=0)
    stderr = per.std(axis=0, ddof=1) / math.sqrt(k_probes) if k_probes > 1 else np.full(b, np.nan)
    if stats is not None:
        stats["divergence"] = np.asarray(div, dtype=np.float64).reshape(len(div), b * k_probes)
        stats["evaluations"] = int(stepper.n_iter)
        stats["captures"] = int(captures)
    return Likelihood(torch.from_numpy(logp), torch.from_numpy(-logp / (d * math.log(2.0))), torch.from_numpy(stderr), latent)
