"""``noise_estimation_loss`` (reference ``functions/losses.py:4-18``) on libddimx kernels.

q-sample, model forward and the squared-error reduction run in HIP.  In training mode with autograd enabled the model
call is an autograd node (``ddim_audio_amd.model._UNetTrainFn``) and the reduction gets its hand-written backward
(``ddimx_sqerr_loss_bwd``), so ``loss.backward()`` works as in the reference runner (``runners/diffusion.py:143-150``).
If ``x0`` requires grad, the q-sample is an autograd node too and ``x0.grad`` is filled as the reference's autograd fills it.

``v_prediction_loss`` is the same step for a network that predicts v = sqrt(a_t) e - sqrt(1 - a_t) x0 (Salimans & Ho 2022;
``model.type: v``): one kernel writes the noised sample and the v target (``ddimx_qsample_v``), the reduction and its backward
are the eps loss's with the target in ``e``'s place.

Both are their q-sample plus ``target_loss``, the shared core: model forward, squared error against a given target, and -- with
``weight=``, an fp32 device table indexed by the timestep (``schedule.loss_weight_table``: min-SNR and truncated-SNR weighting) --
one weight per sample (``ddimxd_sqerr_loss_w``, include/ddimx_distill.h).  ``distill.distill_step`` calls the core with the
distillation target.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib


class _QSampleFn(torch.autograd.Function):
    """x = x0 sqrt(a[t]) + e sqrt(1 - a[t]) (functions/losses.py:10-11), differentiable in x0 only (e, a, t are constants, as in
    the reference's training step).  d x0 = d x sqrt(a[t]): the same kernel on (d x, 0), so the scale is the forward's own."""

    @staticmethod
    def forward(ctx, x0, e, a, t):
        b = x0.size(0)
        x = torch.empty_like(x0)
        _lib.check(_lib.load().ddimx_qsample(_lib.ptr(x0), _lib.ptr(e), _lib.ptr(a), _lib.ptr(t), _lib.ptr(x), b, x0.numel() // b,
                                             _lib.stream()))
        ctx.save_for_backward(a, t)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, t = ctx.saved_tensors
        gc = g.contiguous()
        b = gc.size(0)
        zero = torch.zeros_like(gc)
        d = torch.empty_like(gc)
        with torch.cuda.device(gc.device):
            _lib.check(_lib.load().ddimx_qsample(_lib.ptr(gc), _lib.ptr(zero), _lib.ptr(a), _lib.ptr(t), _lib.ptr(d), b,
                                                 gc.numel() // b, _lib.stream()))
        return d, None, None, None


class _SqErrFn(torch.autograd.Function):
    """per-sample sum of (e - out)^2 over (1, 2, 3): returns [B + 1] = per-sample losses and their batch mean."""

    @staticmethod
    def forward(ctx, out, e):
        lib = _lib.load()
        b = out.size(0)
        per = out.numel() // b
        partial = torch.empty(b * 64, dtype=torch.float32, device=out.device)
        loss = torch.empty(b + 1, dtype=torch.float32, device=out.device)
        _lib.check(lib.ddimx_sqerr_loss(_lib.ptr(e), _lib.ptr(out), _lib.ptr(partial), _lib.ptr(loss), b, per, _lib.stream()))
        ctx.save_for_backward(out, e)
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        out, e = ctx.saved_tensors
        b = out.size(0)
        per = out.numel() // b
        # the [B] entry is the batch mean (functions/losses.py:18): the kernel folds its upstream gradient into the per-sample ones
        gc = g.contiguous()  # (what autograd hands over already is: no launch)
        d = torch.empty_like(out)
        with torch.cuda.device(out.device):
            _lib.check(lib.ddimx_sqerr_loss_bwd_mean(_lib.ptr(e), _lib.ptr(out), _lib.ptr(gc), _lib.ptr(d), b, per, _lib.stream()))
        return d, None


class _SqErrWFn(torch.autograd.Function):
    """``_SqErrFn`` with sample b weighted by w[t[b]] (``ddimxd_sqerr_loss_w`` and its backward): [B + 1] = the weighted per-sample
    losses and their batch mean.  ``w``: fp32 device table, ``t``: the int64 device tensor the network was given, read by the
    launches themselves (nothing is gathered on the host: a captured step serves every replay)."""

    @staticmethod
    def forward(ctx, out, e, w, t):
        lib = _lib.load()
        b = out.size(0)
        per = out.numel() // b
        partial = torch.empty(b * 64, dtype=torch.float32, device=out.device)
        loss = torch.empty(b + 1, dtype=torch.float32, device=out.device)
        _lib.check(lib.ddimxd_sqerr_loss_w(_lib.ptr(e), _lib.ptr(out), _lib.ptr(w), w.numel(), _lib.ptr(t), _lib.ptr(partial),
                                           _lib.ptr(loss), b, per, _lib.stream()))
        ctx.save_for_backward(out, e, w, t)
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        out, e, w, t = ctx.saved_tensors
        b = out.size(0)
        per = out.numel() // b
        gc = g.contiguous()
        d = torch.empty_like(out)
        with torch.cuda.device(out.device):
            _lib.check(lib.ddimxd_sqerr_loss_w_bwd_mean(_lib.ptr(e), _lib.ptr(out), _lib.ptr(gc), _lib.ptr(w), w.numel(), _lib.ptr(t),
                                                        _lib.ptr(d), b, per, _lib.stream()))
        return d, None, None, None


def _check_weight(weight, device):
    if weight is None:
        return None
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32 or weight.dim() != 1 or weight.numel() < 1:
        raise ValueError("weight must be None or a 1-D fp32 tensor (schedule.loss_weight_table, rounded to fp32)")
    if weight.device != device:
        raise ValueError(f"weight lives on {weight.device}, the batch on {device}: move the table once, outside the step")
    return weight.contiguous()


def target_loss(model, x, t, target, weight=None, keepdim=False):
    """sum over (1, 2, 3) of (target - model(x, t))^2, per sample times ``weight[t[b]]`` if a table is given: the batch mean, or
    the per-sample values with ``keepdim``.  ``x``, ``target``: [B, C, T, F] on the GPU, ``target`` a constant; ``weight``: None
    or a 1-D fp32 table on ``x``'s device that every ``t[b]`` indexes (a ``t[b]`` outside it gives NaN, it reads no row)."""
    if not x.is_cuda:
        raise RuntimeError("target_loss runs only on a ROCm GPU (no CPU fallback)")
    w = _check_weight(weight, x.device)
    with torch.cuda.device(x.device):
        with torch.no_grad():
            tg = target.to(x.device, torch.float32).contiguous()
            tc = t.to(x.device, torch.int64).contiguous()
        b = x.size(0)
        out = model(x.float().contiguous(), tc).contiguous()
        loss = _SqErrFn.apply(out, tg) if w is None else _SqErrWFn.apply(out, tg, w, tc)
    return loss[:b] if keepdim else loss[b]


def noise_estimation_loss(model, x0, t, e, a, keepdim=False, weight=None):
    lib = _lib.load()
    if not x0.is_cuda:
        raise RuntimeError("noise_estimation_loss runs only on a ROCm GPU (no CPU fallback)")
    _check_weight(weight, x0.device)
    want_x0 = torch.is_grad_enabled() and x0.requires_grad  # gradient w.r.t. x0 (guidance, inversion): q-sample on the tape
    with torch.cuda.device(x0.device):
        with torch.no_grad():
            x0c, ec = x0.float().contiguous(), e.float().contiguous()
            ac = a.to(x0.device, torch.float32).contiguous()
            tc = t.to(x0.device, torch.int64).contiguous()
            b = x0c.size(0)
            per = x0c.numel() // b
            if not want_x0:
                x = torch.empty_like(x0c)
                _lib.check(lib.ddimx_qsample(_lib.ptr(x0c), _lib.ptr(ec), _lib.ptr(ac), _lib.ptr(tc), _lib.ptr(x), b, per,
                                             _lib.stream()))
        if want_x0:
            x = _QSampleFn.apply(x0.float().contiguous(), ec, ac, tc)
    return target_loss(model, x, tc, ec, weight=weight, keepdim=keepdim)


def v_prediction_loss(model, x0, t, e, a, keepdim=False, weight=None):
    """sum over (1, 2, 3) of (v - model(x_t, t))^2 with x_t = x0 sqrt(a[t]) + e sqrt(1 - a[t]) -- bit for bit
    ``noise_estimation_loss``'s x_t -- and the target v = e sqrt(a[t]) - x0 sqrt(1 - a[t]); arguments and return value are
    ``noise_estimation_loss``'s (the batch mean, or the per-sample sums with ``keepdim``).  The target depends on x0 as well, and
    its gradient is not implemented: ``x0.requires_grad`` with autograd enabled raises NotImplementedError.  ``weight``: as in
    ``target_loss``."""
    lib = _lib.load()
    if not x0.is_cuda:
        raise RuntimeError("v_prediction_loss runs only on a ROCm GPU (no CPU fallback)")
    if torch.is_grad_enabled() and x0.requires_grad:
        raise NotImplementedError("v_prediction_loss has no gradient w.r.t. x0 (x_t and the target v both depend on it): "
                                  "detach x0, or use noise_estimation_loss for guidance through an eps model")
    _check_weight(weight, x0.device)
    with torch.cuda.device(x0.device):
        with torch.no_grad():
            x0c, ec = x0.float().contiguous(), e.float().contiguous()
            ac = a.to(x0.device, torch.float32).contiguous()
            tc = t.to(x0.device, torch.int64).contiguous()
            b = x0c.size(0)
            x, v = torch.empty_like(x0c), torch.empty_like(x0c)
            _lib.check(lib.ddimx_qsample_v(_lib.ptr(x0c), _lib.ptr(ec), _lib.ptr(ac), _lib.ptr(tc), _lib.ptr(x), _lib.ptr(v), b,
                                           x0c.numel() // b, _lib.stream()))
    return target_loss(model, x, tc, v, weight=weight, keepdim=keepdim)


loss_registry = {"simple": noise_estimation_loss, "v": v_prediction_loss}
