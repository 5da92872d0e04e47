"""Progressive distillation of the sampler (Salimans & Ho 2022): a student learns to do in ONE DDIM step what its teacher does in
two, so a teacher that samples over the sequence S (2N timesteps) yields a student that samples over ``schedule.halve_seq(S)``
(N timesteps) with ``generalized_steps`` as it stands; the next round takes the student as teacher and the halved sequence.

Student step k goes t = S[2k+1] -> t'' = S[2k-1] (the data for k = 0); the teacher goes t -> t' = S[2k] -> t'', both steps at
eta = 0.  With m0 the teacher's x0 prediction at (z, t), z' = alpha' m0 + sigma' eps0 its half step and m1 its x0 prediction at
(z', t'), the x0 the student must predict for its single step to land on the teacher's z'' is

    x = m1 + omega (m0 - m1),    omega = A / (A + B) in [0, 0.5)    (``schedule.distill_coefficients``)

-- the convex form of (z'' - r z) / (alpha'' - r alpha), whose denominator cancels for short steps -- and the student's training
target is (z - alpha x) / sigma for an eps student, (alpha z - x) / sigma for a v student.  Two teacher forwards (no_grad) and two
kernels (``ddimxd_distill_half``, ``ddimxd_distill_target``, include/ddimx_distill.h; a v teacher's outputs pass ``ddimx_v_to_eps``
first); ``distill_step`` then runs ``losses.target_loss`` on the student and the tail of ``train.train_step``.  Eager only, single
rank as tested: a graphed or data-parallel distillation step is not built.
"""
import numpy as np
import torch

from . import _lib, losses, sampler, train
from .schedule import _check_teacher_seq, check_prediction, distill_coefficients, v_table


def _teacher_eps(teacher, z, t, pred, vt):
    out = teacher(z, t).float().contiguous()
    if pred == "v":
        _lib.check(_lib.load().ddimx_v_to_eps(_lib.ptr(z), _lib.ptr(out), _lib.ptr(out), _lib.ptr(vt), vt.size(0), _lib.ptr(t),
                                              z.size(0), z[0].numel(), _lib.stream()))
    return out


def _check_steps(k, n, n_steps):
    """``k`` as a host int64 array of ``n`` student step indices inside 0 .. n_steps - 1."""
    if not isinstance(k, torch.Tensor) or k.dim() != 1 or k.numel() != n or k.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"k must be an integer tensor of shape [{n}] (one student step index per sample)")
    kh = k.to("cpu", torch.int64).numpy()
    if kh.min() < 0 or kh.max() >= n_steps:
        raise ValueError(f"k entries must lie in 0..{n_steps - 1} (the teacher sequence makes {n_steps} student steps)")
    return kh


def distill_target(teacher, z, k, teacher_seq, alphas, prediction=None, student_prediction="eps", return_x0=False):
    """The student's training target at the noised samples ``z`` ([B, C, T, F]; sample b sits at t = teacher_seq[2 k[b] + 1]).

    ``teacher``: a ``Model`` in eval mode or any callable ``model(x, t)``; ``prediction`` what its output is (None: the model's
    own, else ``"eps"``); ``k``: integer [B] tensor of student step indices, read on the host (t and t' are built there from the
    coefficient rows); ``student_prediction``: what the target is a target for.  Two teacher forwards under ``no_grad``.
    Returns (target, t) -- t the int64 device tensor of the students' timesteps -- or (target, t, x0_target) with ``return_x0``.
    Invalid arguments raise ValueError before any launch."""
    pred = sampler._prediction(teacher, prediction)
    check_prediction(student_prediction)
    shape = sampler._check_sample(z, teacher)
    if isinstance(teacher, torch.nn.Module) and teacher.training:
        raise ValueError("the teacher must be in eval mode (teacher.eval()): its dropout is not part of the target")
    coef = distill_coefficients(teacher_seq, alphas, student_prediction)
    rows = coef[_check_steps(k, shape[0], coef.shape[0])]
    dev = sampler._device(teacher, z)
    lib = _lib.load()
    b, per = shape[0], z[0].numel()
    with torch.cuda.device(dev), torch.no_grad():
        zc = z.detach().to(dev, torch.float32).contiguous()
        rows_d = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(dev)
        t = torch.from_numpy(rows[:, 0].astype(np.int64)).to(dev)
        t_mid = torch.from_numpy(rows[:, 5].astype(np.int64)).to(dev)
        vt = torch.from_numpy(np.ascontiguousarray(v_table(alphas), dtype=np.float32)).to(dev) if pred == "v" else None
        eps0 = _teacher_eps(teacher, zc, t, pred, vt)
        zmid, m0 = torch.empty_like(zc), torch.empty_like(zc)
        _lib.check(lib.ddimxd_distill_half(_lib.ptr(zc), _lib.ptr(eps0), _lib.ptr(rows_d), _lib.ptr(zmid), _lib.ptr(m0), b, per,
                                           _lib.stream()))
        eps1 = _teacher_eps(teacher, zmid, t_mid, pred, vt)
        x0_target = torch.empty_like(zc) if return_x0 else None
        # in place: the target takes m0's buffer
        _lib.check(lib.ddimxd_distill_target(_lib.ptr(zc), _lib.ptr(zmid), _lib.ptr(eps1), _lib.ptr(m0), _lib.ptr(rows_d), _lib.ptr(m0),
                                             _lib.ptr(x0_target), b, per, _lib.stream()))
    return (m0, t, x0_target) if return_x0 else (m0, t)


def mirrored_steps(n, n_steps, generator=None):
    """CPU draw of ceil(n / 2) student step indices, mirrored (k, n_steps - 1 - k), truncated to n: ``antithetic_timesteps`` on
    the student's steps."""
    return train.antithetic_timesteps(n, n_steps, generator=generator)


def distill_step(student, teacher, x, state, alphas, teacher_seq, e=None, k=None):
    """One optimisation step of the student (``state``: its ``train.TrainingState``) on the data batch ``x`` [B, C, T, F]:
    z = the q-sample of x at the students' timesteps (``ddimx_qsample``), the target of ``distill_target`` in the student's own
    prediction, ``losses.target_loss(student, z, t, target, weight=state.loss_weight)`` and ``train.finish_step`` -- the tail
    ``train_step`` runs.  ``e`` / ``k`` default to fresh noise / ``mirrored_steps``.  Returns (loss, {clip group: total grad
    norm}) as device tensors.  The teacher is only read."""
    student.train()
    n = x.size(0)
    seq = _check_teacher_seq(teacher_seq, alphas.numel())
    if k is None:
        k = mirrored_steps(n, len(seq) // 2)
    if e is None:
        e = torch.randn_like(x)
    s_pred = sampler._prediction(student, None)
    kh = _check_steps(k, n, len(seq) // 2)
    t_host = torch.tensor([int(seq[2 * int(i) + 1]) for i in kh], dtype=torch.int64)
    lib = _lib.load()
    with torch.cuda.device(x.device), torch.no_grad():
        xc, ec = x.float().contiguous(), e.float().contiguous()
        ac = alphas.to(x.device, torch.float32).contiguous()
        tq = t_host.to(x.device)
        z = torch.empty_like(xc)
        _lib.check(lib.ddimx_qsample(_lib.ptr(xc), _lib.ptr(ec), _lib.ptr(ac), _lib.ptr(tq), _lib.ptr(z), n, xc.numel() // n, _lib.stream()))
    target, t = distill_target(teacher, z, k, seq, alphas, student_prediction=s_pred)
    w = state.device_loss_weight(x.device)
    loss = losses.target_loss(student, z, t, target, weight=w)
    return train.finish_step(student, state, loss)
