"""Consistency distillation and few-step consistency sampling (Song et al. 2023, Algorithm 2 and multistep consistency sampling,
in the discrete-time parametrisation of Luo et al. 2023; kernels in include/cmx_consistency.h).

A consistency model maps a noisy sample at ANY level straight to the data: f(x, t) = c_skip(t) x + c_out(t) x0_hat(x, t), with
f(x, t_min) = x.  The kernels see f = p_t x + q_t out with ``out`` the network's raw output and (p_t, q_t) a row of
``schedule.consistency_table`` -- an eps network and a v network differ in the table alone.

Training (``consistency_step``).  On the student levels ``seq`` = S[0..N-1], S[0] = t_min, every sample draws an index n, takes
t_hi = S[n + skip], t_lo = S[n], and with z the q-sample of the data at t_hi:

    z_hat = one eta = 0 DDIM step of the frozen TEACHER from (z, t_hi) to t_lo          ``ddimxd_distill_half`` on
                                                                                         ``schedule.consistency_pairs`` rows
    y     = f_target(z_hat, t_lo)                          the target network, eval mode, no_grad (``consistency_target``)
    loss  = mean_b d(y_b, f_student(z_b, t_hi))            ``cmx_consistency_loss`` and its backward, f never materialised

d is the per-sample sum of squares, or the pseudo-Huber S / (sqrt(S + c^2) + c) with ``huber_c`` > 0.  Then ``train.finish_step``
and the target update theta- <- mu theta- + (1 - mu) theta: ONE ``ddimx_ema_update_multi_coef`` launch whose shadow pointers are
the target model's parameters.  The fixed point of the recursion on N levels is the teacher's N-step DDIM map in one evaluation
(tests/test_consistency_cpu.py states it on the Gaussian model).  Eager only, single rank as tested: a graphed or data-parallel
step, loss weighting, consistency TRAINING without a teacher and guided distillation are not built.

Sampling (``consistency_steps``).  ``len(seq)`` evaluations: x0 = f(x, seq[-1]); then, per further level going down, the
prediction is re-noised to that level, x = alpha x0 + sigma z, and mapped to the data again.  One kernel per step
(``cmx_consistency_update``) forms the prediction and the re-noised sample; with a ``NoiseStream`` z is drawn inside it and the
step replays from one hipGraph.  Windows, inpainting, the pool, ``threshold=`` and a ``BrownianStream`` are not built on
consistency models.  No trained checkpoint exists here: what is verified is the arithmetic and the closed-form Gaussian case, not
perceptual quality.
"""
import numpy as np
import torch

from . import _lib, sampler, train
from .distill import _teacher_eps
from .ema import EMAHelper
from .schedule import consistency_coefficients, consistency_pairs, consistency_table, v_table


def _dev32(a64, dev):
    return torch.from_numpy(np.ascontiguousarray(a64, dtype=np.float32)).to(dev)


def _check_index(n, b, hi):
    """``n`` as a host int64 array of ``b`` pair indices inside 0 .. hi - 1."""
    if not isinstance(n, torch.Tensor) or n.dim() != 1 or n.numel() != b or n.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"n must be an integer tensor of shape [{b}] (one level index per sample)")
    nh = n.to("cpu", torch.int64).numpy()
    if nh.min() < 0 or nh.max() >= hi:
        raise ValueError(f"n entries must lie in 0..{hi - 1} (seq and skip make {hi} pairs of levels)")
    return nh


def _check_huber(huber_c):
    c = float(huber_c)
    if not np.isfinite(c) or c < 0:
        raise ValueError(f"huber_c must be finite and >= 0, got {huber_c!r}")
    return c


def _eval_only(model, what):
    if isinstance(model, torch.nn.Module) and model.training:
        raise ValueError(f"the {what} must be in eval mode ({what.split()[0]}.eval()): its dropout is not part of the target")


def mirrored_indices(b, n_pairs, generator=None):
    """CPU draw of ceil(b / 2) pair indices, mirrored (n, n_pairs - 1 - n), truncated to b: ``distill.mirrored_steps`` on the
    pairs of levels."""
    return train.antithetic_timesteps(b, n_pairs, generator=generator)


def consistency_target(target_model, teacher, z, n, seq, alphas, skip=1, teacher_prediction=None, target_prediction=None,
                       sigma_data=0.5, timestep_scale=10.0, t_min=0):
    """The distillation target at the noised samples ``z`` ([B, C, T, F]; sample b sits at t_hi = seq[n[b] + skip]):
    y = f_target(z_hat, t_lo), z_hat the teacher's eta = 0 DDIM step from (z, t_hi) to t_lo = seq[n[b]].

    ``teacher`` / ``target_model``: a ``Model`` in eval mode or any callable ``model(x, t)``; ``*_prediction`` what each one's
    output is (None: the model's own, else ``"eps"``) -- a v or eps teacher and a v or eps target mix freely; ``n``: integer [B]
    tensor of indices into the pairs of ``schedule.consistency_pairs(seq, alphas, skip, t_min)``, read on the host.  Two forwards
    under ``no_grad`` and two kernels (``ddimxd_distill_half``, ``cmx_consistency_out``; a v teacher's output passes
    ``ddimx_v_to_eps`` first).  Returns (y, t_hi), t_hi the int64 device tensor of the students' timesteps.  Invalid arguments
    raise ValueError before any launch."""
    t_pred = sampler._prediction(teacher, teacher_prediction)
    y_pred = sampler._prediction(target_model, target_prediction)
    shape = sampler._check_sample(z, teacher)
    sampler._check_model(target_model, shape, shape[2])
    _eval_only(teacher, "teacher")
    _eval_only(target_model, "target model")
    rows, t_hi, t_lo = consistency_pairs(seq, alphas, skip, t_min)
    tab = consistency_table(alphas, y_pred, sigma_data, timestep_scale, t_min)
    nh = _check_index(n, shape[0], rows.shape[0])
    dev = sampler._device(teacher, z)
    lib = _lib.load()
    b, per = shape[0], z[0].numel()
    with torch.cuda.device(dev), torch.no_grad():
        zc = z.detach().to(dev, torch.float32).contiguous()
        rows_d, tab_d = _dev32(rows[nh], dev), _dev32(tab, dev)
        thi, tlo = torch.from_numpy(t_hi[nh]).to(dev), torch.from_numpy(t_lo[nh]).to(dev)
        vt = _dev32(v_table(alphas), dev) if t_pred == "v" else None
        eps = _teacher_eps(teacher, zc, thi, t_pred, vt)
        zhat, m0 = torch.empty_like(zc), torch.empty_like(zc)
        _lib.check(lib.ddimxd_distill_half(_lib.ptr(zc), _lib.ptr(eps), _lib.ptr(rows_d), _lib.ptr(zhat), _lib.ptr(m0), b, per,
                                           _lib.stream()))
        out = target_model(zhat, tlo).float().contiguous()
        # in place: y takes m0's buffer (the callable's own tensor is read, never rewritten)
        _lib.check(lib.cmx_consistency_out(_lib.ptr(zhat), _lib.ptr(out), _lib.ptr(tab_d), tab_d.size(0), _lib.ptr(tlo), _lib.ptr(m0), b,
                                           per, _lib.stream()))
    return m0, thi


class _ConsistencyLossFn(torch.autograd.Function):
    """d(y, f(z, t)) per sample with f = p z + q out formed inside the kernels: returns [B + 1] = the per-sample distances and their
    batch mean.  Differentiable in ``out`` only (z, y, the table and t are constants of the step)."""

    @staticmethod
    def forward(ctx, out, z, y, tab, t, huber_c):
        lib = _lib.load()
        b = out.size(0)
        per = out.numel() // b
        partial = torch.empty(b * 64, dtype=torch.float32, device=out.device)
        loss = torch.empty(b + 1, dtype=torch.float32, device=out.device)
        _lib.check(lib.cmx_consistency_loss(_lib.ptr(z), _lib.ptr(out), _lib.ptr(y), _lib.ptr(tab), tab.size(0), _lib.ptr(t), huber_c,
                                            _lib.ptr(partial), _lib.ptr(loss), b, per, _lib.stream()))
        ctx.save_for_backward(out, z, y, tab, t, loss)
        ctx.huber_c = huber_c
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        out, z, y, tab, t, loss = ctx.saved_tensors
        b = out.size(0)
        per = out.numel() // b
        gc = g.contiguous()
        d = torch.empty_like(out)
        with torch.cuda.device(out.device):
            _lib.check(lib.cmx_consistency_loss_bwd(_lib.ptr(z), _lib.ptr(out), _lib.ptr(y), _lib.ptr(tab), tab.size(0), _lib.ptr(t),
                                                    ctx.huber_c, _lib.ptr(loss), _lib.ptr(gc), _lib.ptr(d), b, per, _lib.stream()))
        return d, None, None, None, None, None


def consistency_loss(model, z, t, y, table, huber_c=0.0, keepdim=False):
    """mean over the batch (or, with ``keepdim``, the per-sample values) of d(y_b, p z_b + q model(z, t)_b), (p, q) = table[t[b]]:
    the loss of ``consistency_step`` on a given target.  ``z``, ``y``: [B, C, T, F] on the GPU, constants; ``table``: fp32
    [n_table, 2] on the same device (``schedule.consistency_table``, rounded); a t[b] outside it gives NaN."""
    if not z.is_cuda:
        raise RuntimeError("consistency_loss runs only on a ROCm GPU (no CPU fallback)")
    huber_c = _check_huber(huber_c)
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.dim() != 2 or table.size(1) != 2 or table.size(0) < 1:
        raise ValueError("table must be an fp32 [n_table, 2] tensor (schedule.consistency_table, rounded to fp32)")
    if table.device != z.device:
        raise ValueError(f"table lives on {table.device}, the batch on {z.device}: move it once, outside the step")
    if z[0].numel() == 0 or z[0].numel() % 4:
        raise ValueError("the size of one sample (C * T * F) must be a positive multiple of 4 elements")
    with torch.cuda.device(z.device):
        with torch.no_grad():
            zc, yc = z.float().contiguous(), y.to(z.device, torch.float32).contiguous()
            tc = t.to(z.device, torch.int64).contiguous()
        b = zc.size(0)
        out = model(zc, tc).contiguous()
        loss = _ConsistencyLossFn.apply(out, zc, yc, table.contiguous(), tc, huber_c)
    return loss[:b] if keepdim else loss[b]


def _target_update(student, target_model, state, mu):
    """theta- <- mu theta- + (1 - mu) theta over every trainable parameter, in one launch; the pointer tables are kept on
    ``state`` and rebuilt only when a parameter of either model has moved (``EMAHelper.update``'s rule and rounding)."""
    theirs = dict(target_model.named_parameters())
    pairs = []
    for name, p in student.named_parameters():
        if p.requires_grad:
            s = theirs.get(name)
            if s is None or s.shape != p.shape:
                raise RuntimeError(f"consistency_step: the target model has no parameter {name} of shape {tuple(p.shape)}")
            s, p = s.data, p.data
            if not (p.is_cuda and s.is_cuda and p.dtype == s.dtype == torch.float32 and p.is_contiguous() and s.is_contiguous()):
                raise RuntimeError(f"consistency_step: {name} must be contiguous fp32 on the GPU in both models (no CPU fallback)")
            pairs.append((s, p))
    if not pairs:
        return
    dev = pairs[0][1].device
    key = tuple([s.data_ptr() for s, _ in pairs] + [p.data_ptr() for _, p in pairs])
    tb = getattr(state, "_consistency_tables", None)
    if tb is None or tb["key"] != key:
        tb = state._consistency_tables = EMAHelper()._build_tables(pairs, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ddimx_ema_update_multi_coef(_lib.ptr(tb["sh"]), _lib.ptr(tb["p"]), _lib.ptr(tb["n"]), _lib.ptr(tb["bt"]),
                                                           _lib.ptr(tb["bo"]), tb["nblk"], 1.0 - mu, mu, _lib.stream()))
    if hasattr(target_model, "invalidate"):
        target_model.invalidate()  # written through raw pointers: its packed weights must be rebuilt


def consistency_step(student, target_model, teacher, x, state, alphas, seq, skip=1, huber_c=0.0, mu=0.95, e=None, n=None,
                     sigma_data=0.5, timestep_scale=10.0, t_min=0):
    """One optimisation step of the student (``state``: its ``train.TrainingState``) on the data batch ``x`` [B, C, T, F]:
    z = the q-sample of x at t_hi (``ddimx_qsample``), y = ``consistency_target`` (target model and teacher in eval mode, only
    read), ``consistency_loss`` of the student at (z, t_hi) in its own prediction, ``train.finish_step``, then the target update
    theta- <- mu theta- + (1 - mu) theta in one ``ddimx_ema_update_multi_coef`` launch and ``target_model.invalidate()``.
    ``e`` / ``n`` default to fresh noise / ``mirrored_indices``.  Returns (loss, {clip group: total grad norm}) as device tensors.
    Eager, single rank; ``state.loss_weight`` is not applied (loss weighting is not built here).  Invalid arguments raise
    ValueError before any launch."""
    mu, huber_c = float(mu), _check_huber(huber_c)
    if not np.isfinite(mu) or not 0.0 <= mu <= 1.0:
        raise ValueError(f"mu must lie in [0, 1], got {mu!r}")
    if target_model is student:
        raise ValueError("the target model must be a model of its own (a copy of the student): the step updates it in place")
    s_pred = sampler._prediction(student, None)
    rows, _, _ = consistency_pairs(seq, alphas, skip, t_min)
    tab = consistency_table(alphas, s_pred, sigma_data, timestep_scale, t_min)
    b = x.size(0)
    if n is None:
        n = mirrored_indices(b, rows.shape[0])
    nh = _check_index(n, b, rows.shape[0])
    student.train()
    if e is None:
        e = torch.randn_like(x)
    lib = _lib.load()
    with torch.cuda.device(x.device), torch.no_grad():
        xc, ec = x.float().contiguous(), e.float().contiguous()
        ac = torch.as_tensor(alphas).to(x.device, torch.float32).contiguous()
        tq = torch.from_numpy(rows[nh, 0].astype(np.int64)).to(x.device)
        z = torch.empty_like(xc)
        _lib.check(lib.ddimx_qsample(_lib.ptr(xc), _lib.ptr(ec), _lib.ptr(ac), _lib.ptr(tq), _lib.ptr(z), b, xc.numel() // b, _lib.stream()))
        tab_d = _dev32(tab, x.device)
    y, t_hi = consistency_target(target_model, teacher, z, n, seq, alphas, skip, sigma_data=sigma_data, timestep_scale=timestep_scale,
                                 t_min=t_min)
    loss = consistency_loss(student, z, t_hi, y, tab_d, huber_c)
    out = train.finish_step(student, state, loss)
    _target_update(student, target_model, state, mu)
    return out


class ConsistencyStepper(sampler.DDIMStepper):
    """``DDIMStepper`` on ``schedule.consistency_coefficients`` rows: the frame, the graph rule, ownership and ``_stale`` are the
    base class's; the update is ``cmx_consistency_update`` on the network's RAW output (the table already is that of the model's
    prediction, so there is no v conversion), and a ``NoiseStream``'s normals are drawn inside it: no noise buffer, no fill."""

    def __init__(self, model, xt, coef64, use_graph=True, noise_fn=None, slot=0, fork=True, noise=None):
        sampler._check_noise(noise, noise_fn)
        super().__init__(model, xt, coef64, use_graph=use_graph, noise_fn=noise_fn, slot=slot, fork=fork)
        self.noise = noise  # handed over behind the frame's constructor: the update draws in the kernel, so no buffer is allocated

    def _to_eps(self, out, st):
        return out

    def _update(self, out, noise, st):
        xt, ns = self.xt, self.noise
        seed, first = (ns.seed, ns.first_sample) if ns is not None else (0, 0)
        _lib.check(self.lib.cmx_consistency_update(_lib.ptr(xt), _lib.ptr(out), _lib.ptr(noise), _lib.ptr(self.x0), _lib.ptr(self.coef),
                                                   _lib.ptr(self.counter), xt.size(0), xt[0].numel(), seed, first, 0, st))


def consistency_steps(x, seq, model, alphas, select_index=None, noise=None, noise_fn=None, prediction=None, sigma_data=0.5,
                      timestep_scale=10.0, t_min=0, **kwargs):
    """Multistep consistency sampling: ``len(seq)`` evaluations of ``model``, a consistency model (``consistency_step``'s student)
    on the increasing timesteps ``seq`` (every entry > t_min).  Iteration i (from the top): x0 = f(x, seq[-1 - i]); unless it is
    the last, x <- alpha x0 + sigma z at the next lower entry of ``seq``.  Returns (xs, x0_preds) like ``generalized_steps``;
    the last xs entry is the last prediction.

    ``noise``: a ``NoiseStream`` -- z is drawn inside the update kernel from the seeded device stream (draw index = iteration), the
    step replays from one hipGraph under ``generalized_steps``' rule (``len(seq) >= 4``), and a sample depends on (seed, global
    sample index) only.  Without one, z is ``torch.randn_like`` or ``noise_fn(x_t)`` and the steps run eagerly.  A one-entry
    ``seq`` needs no noise at all.  ``prediction``: what the network's output is (None: the model's own, else ``"eps"``); it picks
    the table (``schedule.consistency_table``; ``sigma_data``, ``timestep_scale``, ``t_min`` must be those of the training).
    Refused before any launch: a ``BrownianStream`` or anything else that is no ``NoiseStream`` (TypeError), ``noise`` and
    ``noise_fn`` together, ``threshold=`` and any other keyword (ValueError / TypeError)."""
    if kwargs.get("threshold") is not None:
        raise ValueError("consistency_steps has no threshold=: x0 clipping on a consistency model is not built")
    kwargs.pop("threshold", None)
    if kwargs:
        raise TypeError(f"consistency_steps got unexpected keyword arguments {sorted(kwargs)}")
    sampler._check_noise(noise, noise_fn)
    prediction = sampler._prediction(model, prediction)
    seq = list(seq)
    coef = consistency_coefficients(seq, alphas, prediction, sigma_data=sigma_data, timestep_scale=timestep_scale, t_min=t_min)
    sampler._check_sample(x, model)
    _lib.load()
    device = sampler._device(model, x)
    host_fn = None
    if noise is None and len(seq) > 1:
        host_fn = noise_fn if noise_fn is not None else torch.randn_like
    with torch.no_grad(), torch.cuda.device(device):
        xt = sampler._as_state(x, device)
        stepper = ConsistencyStepper(model, xt, coef, use_graph=(len(seq) >= 4), noise_fn=host_fn, noise=noise)
        return sampler._run(stepper, x, select_index)
