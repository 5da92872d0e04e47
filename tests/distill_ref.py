"""float64 restatement of SNR loss weighting and of the progressive-distillation target (Salimans & Ho 2022), for the tests.
It shares nothing with ddim_audio_amd/schedule.py or the kernels: numpy only, and the target is the DIRECT formula -- two
reference DDIM steps of the teacher, then the x0 whose single step lands on their end point -- not the convex form the
library evaluates."""
import numpy as np


def table64(alphas):
    """The fp32 alphas-cumprod table's values as float64."""
    return np.asarray(alphas, dtype=np.float32).astype(np.float64)


def loss_weights(alphas, prediction, kind, gamma=5.0):
    """float64 [len(alphas)] weights of the squared error of ``prediction``, written from the x0-space weight: min-SNR is
    min(SNR, gamma), truncated SNR max(SNR, 1); an eps error is the x0 error times sqrt(SNR), a v error the x0 error times
    sqrt(SNR + 1)."""
    a = table64(alphas)
    snr = a / (1.0 - a)
    x0_weight = {"min_snr": np.minimum(snr, gamma), "trunc_snr": np.maximum(snr, 1.0)}[kind]
    return x0_weight / {"eps": snr, "v": snr + 1.0}[prediction]


def alpha_sigma(a, t):
    """(alpha, sigma) = (sqrt(a_t), sqrt(1 - a_t)); t = -1 is the data: (1, 0)."""
    at = 1.0 if t < 0 else float(a[t])
    return np.sqrt(at), np.sqrt(1.0 - at)


def ddim_step(z, eps, a, t, t_next):
    """One reference DDIM step at eta = 0 (functions/denoising.py:22-40 in float64): returns (x0 prediction, z at t_next)."""
    al, si = alpha_sigma(a, t)
    al_n, si_n = alpha_sigma(a, t_next)
    x0 = (z - si * eps) / al
    return x0, al_n * x0 + si_n * eps


def steps_of(teacher_seq, k):
    """(t, t', t'') of student step k."""
    return teacher_seq[2 * k + 1], teacher_seq[2 * k], (teacher_seq[2 * k - 1] if k else -1)


def direct_x0_target(z, z_end, a, t, t_end):
    """The x0 whose single DDIM step t -> t_end from z lands on z_end: z_end = alpha'' x + (sigma''/sigma)(z - alpha x)."""
    al, si = alpha_sigma(a, t)
    al_e, si_e = alpha_sigma(a, t_end)
    r = si_e / si
    return (z_end - r * z) / (al_e - r * al)


def student_target(z, x0_target, a, t, prediction):
    al, si = alpha_sigma(a, t)
    return (z - al * x0_target) / si if prediction == "eps" else (al * z - x0_target) / si


def distill_target(teacher_eps, z, k, teacher_seq, alphas, student_prediction="eps"):
    """(target, x0 target) for ONE sample z (float64 array) at student step k; ``teacher_eps(z, t)`` returns the teacher's eps in
    float64.  Two reference DDIM steps, then the direct formula."""
    a = table64(alphas)
    t, t_mid, t_end = steps_of(list(teacher_seq), k)
    _, z_mid = ddim_step(z, teacher_eps(z, t), a, t, t_mid)
    _, z_end = ddim_step(z_mid, teacher_eps(z_mid, t_mid), a, t_mid, t_end)
    x = direct_x0_target(z, z_end, a, t, t_end)
    return student_target(z, x, a, t, student_prediction), x


def direct_from_mid(z, z_mid, eps1, teacher_seq, k, alphas, student_prediction="eps"):
    """The same from a GIVEN half step: the teacher's second step from (z_mid, eps1), then the direct formula."""
    a = table64(alphas)
    t, t_mid, t_end = steps_of(list(teacher_seq), k)
    _, z_end = ddim_step(z_mid, eps1, a, t_mid, t_end)
    x = direct_x0_target(z, z_end, a, t, t_end)
    return student_target(z, x, a, t, student_prediction), x


def weighted_loss(out, target, weight=None):
    """Per-sample sum of squared error times the sample's weight, float64: ([B] values, their mean)."""
    out, target = np.asarray(out, dtype=np.float64), np.asarray(target, dtype=np.float64)
    per = ((target - out) ** 2).reshape(out.shape[0], -1).sum(axis=1)
    if weight is not None:
        per = per * np.asarray(weight, dtype=np.float64)
    return per, per.mean()
