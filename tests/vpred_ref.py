"""CPU restatement of the v-parameterisation (test infrastructure; Salimans & Ho 2022).

With a = alphas-cumprod[t], s1 = sqrt(1 - a), s2 = sqrt(a):  x = s2 x0 + s1 e,  v = s2 e - s1 x0,  and back
e = s1 x + s2 v,  x0 = s2 x - s1 v  (s1^2 + s2^2 = 1).  Everything here works in the dtype it is handed (numpy float64 for
the identities and the closed-form model, torch for the loss that autograd differentiates through ``oracle.ref_cpu``); nothing
is shared with ``ddim_audio_amd.schedule.v_table`` or the kernels, so the two statements check each other."""
import numpy as np
import torch


def scales(alpha, t):
    """(s1, s2) of timestep ``t`` in float64 from the fp32 alphas-cumprod table."""
    a = float(torch.as_tensor(alpha).to("cpu", torch.float32)[int(t)])
    return np.sqrt(1.0 - a), np.sqrt(a)


def q_sample(x0, e, s1, s2):
    return s2 * x0 + s1 * e


def v_target(x0, e, s1, s2):
    return s2 * e - s1 * x0


def eps_from_v(x, v, s1, s2):
    return s1 * x + s2 * v


def x0_from_v(x, v, s1, s2):
    return s2 * x - s1 * v


def x0_from_eps(x, e, s1, s2):
    return (x - s1 * e) / s2


def as_eps_model(v_fn, alpha):
    """``model_fn(x, t) -> eps`` over ``v_fn(x, t) -> v``: the conversion a sampler applies to a v network.  ``t`` is an int or
    a tensor / array of equal timesteps (the samplers of ``oracle.ref_cpu`` and ``tests/solver_ref.py`` pass one level per call)."""
    def model_fn(x, t):
        s1, s2 = scales(alpha, t if np.ndim(t) == 0 else np.asarray(t).reshape(-1)[0])
        return eps_from_v(x, v_fn(x, t), s1, s2)
    return model_fn


def gaussian_v_model(alpha, var):
    """The exact v predictor of data ~ N(0, var I), the v form of ``solver_ref.gaussian_model``: with D = a var + 1 - a the
    posterior means are E[x0 | x] = s2 var x / D and E[e | x] = s1 x / D, so v = s2 E[e | x] - s1 E[x0 | x] = s1 s2 (1 - var) x / D."""
    a = torch.as_tensor(alpha).to("cpu", torch.float32).numpy().astype(np.float64)
    return lambda x, t: np.sqrt(1.0 - a[t]) * np.sqrt(a[t]) * (1.0 - var) * x / (a[t] * var + 1.0 - a[t])


def v_prediction_loss(model_fn, x0, t, e, a, keepdim=False):
    """``oracle.ref_cpu.noise_estimation_loss`` with the v target in the noise's place; ``model_fn(x, t)`` returns v."""
    at = a.index_select(0, t).view(-1, 1, 1, 1)
    x = x0 * at.sqrt() + e * (1.0 - at).sqrt()
    v = e * at.sqrt() - x0 * (1.0 - at).sqrt()
    per = (v - model_fn(x, t)).square().sum(dim=(1, 2, 3))
    return per if keepdim else per.mean(dim=0)
