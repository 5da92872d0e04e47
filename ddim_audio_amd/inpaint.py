"""``inpaint_steps`` -- masked DDIM inpainting with reconstruction guidance on the HIP library.

The reference has no such function; this follows ``generalized_steps``'s conventions (``select_index`` rules, CPU copies at
the selected iterations, ``xs[0]`` is the caller's ``x``, updated in place when it already is a contiguous fp32 GPU tensor).
Per iteration (row (t, s1, s2, s3, c2, c1, k1, k2, zeta) of ``schedule.inpaint_coefficients``, mask m, known content y):

1. eps = eps_theta(x_t, t): the inference forward when every zeta is 0, else the tape-keeping forward with dropout off;
2. x0 = (x_t - s1 eps) / s2, rounded as ``ddim_update`` rounds it;
3. guided: r = m (x0 - y), L_b = sum of r^2 per sample, g = k2 m r + J_eps^T (k1 m r) = d L_b / d x_t (the data-only backward
   of the seed k1 m r gives the second term);
4. u = s3 x0 + c2 eps (+ c1 z); guided: u -= zeta / sqrt(L_b) g (DPS, Chung et al. 2023, Algorithm 1, per sample; skipped
   when L_b = 0);
5. replace: x_{t-1} = m (s3 y + c2 eps (+ c1 z)) + (1 - m) u, else u.

All tensor arithmetic of a step runs in libddimx kernels (``ddimx_inpaint_residual`` / ``ddimx_inpaint_update``, the U-Net
forward and its data-only backward); the whole step replays as one hipGraph.
"""
import torch

from . import _lib
from .model import _unet_bwd, _unet_fwd_train
from .sampler import (DDIMStepper, _as_state, _check_eta, _check_noise, _check_sample, _device, _host_noise_fn, _prediction, _run,
                      _v_table)
from .schedule import inpaint_coefficients


class InpaintStepper(DDIMStepper):
    """One inpainting run's device state: a ``sampler.DDIMStepper`` whose update is ddimx_inpaint_update.

    Guided (``guided=True``): the forward calls the C ABI directly, on one stream -- the tape-keeping forward (dropout p = 0,
    this object's tape and training workspace), ddimx_inpaint_residual, the data-only backward into ``d_x``.  No autograd: no
    parameter ``.grad``, flat gradient buffer or all-reduce hook is touched and the dropout call counter does not move.  Its
    capture keeps the model's backward buffers too (``Model.captured_refs(backward=True)``).  Replacement only: the base
    class's forward.  With a ``v_table`` the guided forward converts the network's v to eps in place in ``eps`` right after the
    tape-keeping forward; the table's k1 / k2 must then be ``inpaint_coefficients(..., prediction="v")``'s, which make the seed
    the gradient w.r.t. v.
    ``net_in`` (None: ``xt``) is what the network sees: ``seed`` / ``d_x``, the tape and the training workspace are sized from it,
    while ``y`` / ``mask`` / ``x0`` / the norm's partials belong to ``xt`` (``window_inpaint.WindowInpaintStepper``, whose
    ``_residual`` and ``_update`` cross from one to the other)."""

    def __init__(self, model, xt, y, mask, coef64, guided, replace, use_graph=True, noise_fn=None, slot=0, fork=True, noise=None,
                 v_table=None, net_in=None):
        guided = bool(guided)
        if guided and not hasattr(model, "forward_slot"):
            raise RuntimeError("guided inpainting needs a ddim_audio_amd.Model (tape-keeping forward and data-only backward)")
        # the guided step is one stream: its forward never forks into batch shards
        super().__init__(model, xt, coef64, use_graph=use_graph, noise_fn=noise_fn, slot=slot, fork=fork and not guided, noise=noise,
                         v_table=v_table, net_in=net_in)
        self.y, self.mask = y, mask
        self.guided, self.replace = guided, bool(replace)
        self.b, self.t_len = self.net_in.size(0), self.net_in.size(2)  # the network's batch and length: tape, workspace
        self.per_sample = xt[0].numel()
        self.flags = (_lib.DDIMX_INPAINT_REPLACE if self.replace else 0) | (_lib.DDIMX_INPAINT_GUIDED if self.guided else 0)
        self.seed = self.d_x = self.partials = self.tape = self.ws = None
        if self.guided:
            self.seed, self.d_x = torch.empty_like(self.net_in), torch.empty_like(self.net_in)
            n = int(self._partials_floats())
            if n <= 0:
                raise RuntimeError("libddimx: bad inpainting partials size for B=%d" % xt.size(0))
            self.partials = torch.empty(n, dtype=torch.float32, device=xt.device)

    def _partials_floats(self):
        return self.lib.ddimx_inpaint_partials_floats(self.xt.size(0), self.per_sample)

    def _prepare(self):
        """On the launch stream: weight packing (a no-op unless a parameter changed), tables, workspaces; guided: the backward
        packing and this object's tape / training workspace."""
        if not self.guided:
            return super()._prepare()
        m, dev, lib = self.model, self.xt.device, self.lib
        m.prepare(dev, self.t_len)
        m._ensure_packed_bwd(lib, dev)
        if self.tape is None:
            self.tape = torch.empty(int(lib.ddimx_train_tape_bytes(m._handle, self.b, self.t_len)), dtype=torch.uint8, device=dev)
            self.ws = torch.empty(int(lib.ddimx_train_workspace_bytes(m._handle, self.b, self.t_len)), dtype=torch.uint8, device=dev)

    def _forward(self):
        if not self.guided:
            return super()._forward()
        x, t, m = self.net_in, self.t, self.model
        tables = m._ensure_tables(self.t_len, x.device)
        _unet_fwd_train(m, tables, self.ws, self.tape, x, t, self.eps)
        super()._to_eps(self.eps, _lib.stream())
        self._residual(_lib.stream())
        _unet_bwd(m, tables, self.ws, self.tape, x, t, self.seed, d_x=self.d_x, data_only=True)
        return self.eps

    def _residual(self, st):
        """x0, the seed of the data-only backward and the partials of the norm, from ``eps``."""
        P = _lib.ptr
        _lib.check(self.lib.ddimx_inpaint_residual(P(self.xt), P(self.eps), P(self.y), P(self.mask), P(self.x0), P(self.seed), P(self.partials),
                                                   P(self.coef), P(self.counter), self.xt.size(0), self.per_sample, st))

    def _to_eps(self, out, st):
        return out if self.guided else super()._to_eps(out, st)  # the guided forward has converted already

    def _update(self, et, noise, st):
        P = _lib.ptr
        _lib.check(self.lib.ddimx_inpaint_update(P(self.xt), P(et), P(noise), P(self.x0), P(self.y), P(self.mask), P(self.d_x),
                                                 P(self.partials), P(self.coef), P(self.counter), self.xt.size(0), self.per_sample, self.flags, st))

    def _captured_refs(self):
        return self.model.captured_refs(backward=self.guided) if self.native else None


def _check_tensor(name, v, shape):
    if not isinstance(v, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    try:
        full = torch.broadcast_shapes(tuple(v.shape), shape)
    except RuntimeError:
        full = None
    if full != shape:
        raise ValueError(f"{name} of shape {tuple(v.shape)} does not broadcast to x's {tuple(shape)}")


def _validate(x, seq, model, y, mask, guidance, eta, alpha, prediction):
    """Every argument check, before any device work; returns the coefficient table."""
    return _check_known(_check_sample(x, model), seq, y, mask, guidance, eta, alpha, prediction)


def _check_known(shape, seq, y, mask, guidance, eta, alpha, prediction, who="inpaint_steps"):
    """``_validate`` behind the checks on ``x``, whose ``shape`` y and mask broadcast to (``windowed_inpaint_steps``: the canvas)."""
    if y is None or mask is None:
        raise ValueError(f"{who} needs y= (the known content) and mask= (1 = known)")
    _check_tensor("y", y, shape)
    _check_tensor("mask", mask, shape)
    if mask.dtype.is_complex:
        raise ValueError("mask must be bool, integer or real floating point")
    if y.dtype.is_complex or not y.dtype.is_floating_point:
        raise ValueError("y must be a floating-point tensor")
    mf = mask.detach().to(torch.float64)
    if not bool(((mf >= 0) & (mf <= 1)).all()):
        raise ValueError("mask values must lie in [0, 1]")
    eta = _check_eta(eta)
    if len(seq) == 0:
        raise ValueError("seq is empty")
    return inpaint_coefficients(seq, alpha, eta, guidance, prediction)


def _known(y, mask, shape, device):
    """``y`` and ``mask`` expanded once, before the loop, to contiguous fp32 of the state's ``shape``; y is 0 wherever the mask is 0."""
    m = torch.broadcast_to(mask.to(device, torch.float32), shape).contiguous()
    yk = torch.broadcast_to(y.to(device, torch.float32), shape)
    return torch.where(m == 0, torch.zeros((), device=device), yk).contiguous(), m


def inpaint_steps(x, seq, model, alpha, select_index, y=None, mask=None, guidance=0.0, replace=True, eta=0.0, noise=None,
                  noise_fn=None, prediction=None):
    """x [B,C,T,F] (the starting noise); seq: increasing timesteps; alpha: fp32 alphas-cumprod table; y: the known content and
    mask (1 = known, values in [0, 1], bool / integer / float), both broadcast to x; guidance: zeta >= 0, one float or one value
    per iteration in execution order; replace: put the known region back along the DDIM path after every update.  Returns
    (xs, x0_preds) like ``generalized_steps``: CPU copies of x_{t-1} and of the network's x0 prediction (before any
    replacement) at the selected iterations, ``xs[0]`` the caller's ``x``.  ``eta > 0``: the noise of a step is drawn as
    ``generalized_steps`` draws it -- ``torch.randn_like`` (or ``noise_fn(x_t)``), eager steps; with ``noise=`` a ``NoiseStream``
    from the seeded device stream inside the replayed step.  ``prediction``: ``"eps"`` or ``"v"``, what the network's output is
    (None: ``model.prediction`` if it has one, else ``"eps"``).  Invalid arguments raise before any device work."""
    _check_noise(noise, noise_fn)
    prediction = _prediction(model, prediction)
    seq = list(seq)
    coef = _validate(x, seq, model, y, mask, guidance, eta, alpha, prediction)
    guided = bool((coef[:, 8] != 0).any())
    device = _device(model, x)
    with torch.no_grad(), torch.cuda.device(device):
        xt = _as_state(x, device)
        yk, m = _known(y, mask, tuple(xt.shape), device)
        stepper = InpaintStepper(model, xt, yk, m, coef, guided, replace, use_graph=(len(seq) >= 4),
                                 noise_fn=_host_noise_fn(float(eta), noise, noise_fn), noise=noise, v_table=_v_table(prediction, alpha))
        return _run(stepper, x, select_index)
