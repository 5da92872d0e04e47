"""References of SDE-DPM-Solver++ (``dpm_solver_steps(tau > 0)``, ``ddimxs_multistep_update``; test infrastructure).

Restatements written on their own, so that they check each other, the library and the table's form (``solver_ref.table_steps``
with ``zs``: the w-form the kernel computes, in float64; its bits in fp32 are ``step_math_ref.updater32``'s):

* ``sde_steps`` -- the published update (Lu et al. 2022, appendix, SDE-DPM-Solver++(2M); the 3M SDE scheme as it circulates), with
  noise levels, half-log-SNR, the differences D1 / d1, d2 and the phi terms -- NOT the table's weights;
* ``gaussian_cov`` -- for Gaussian data and its exact noise predictor (``solver_ref.gaussian_model``) every update is linear in
  (x, m1, m2), so the covariance of the final sample follows exactly from a 3 x 3 recursion.
"""
import numpy as np
import torch

import noise_ref as N
import solver_ref as R


# ---- float64: the published form ------------------------------------------------------------------------------------------------------
def sde_steps(x, seq, model_fn, alpha, order, tau, zs):
    """The published update, iteration by iteration (lower-order start: iteration k runs at order min(order, k + 1); the final jump
    to t = -1 lands on the prediction and adds no noise):

        x_n = (sigma_n / sigma_t) e^(-tau h) x + alpha_n (1 - e^(-h_tau)) m0 + correction + sigma_n sqrt(1 - e^(-2 tau h)) z,
        h_tau = (1 + tau) h,
        order 2:  correction = 1/2 alpha_n (1 - e^(-h_tau)) D1,                         D1 = (m0 - m1) / r0
        order 3:  correction = alpha_n (phi2 d1 - phi3 d2),  d1_0 = (m0 - m1) / r0,  d1_1 = (m1 - m2) / r1,
                  d1 = d1_0 + (d1_0 - d1_1) r0 / (r0 + r1),  d2 = (d1_0 - d1_1) / (r0 + r1),
                  phi2 = expm1(-h_tau) / h_tau + 1,  phi3 = phi2 / h_tau - 1/2."""
    ts = list(reversed(list(seq)))
    al, sg, lam = R.levels(seq, alpha)
    x = np.asarray(x, dtype=np.float64)
    xs, ms = [x.copy()], []
    for k, t in enumerate(ts):
        eps = np.asarray(model_fn(x, t), dtype=np.float64)
        m0 = (x - sg[k] * eps) / al[k]
        ms.append(m0)
        p = min(order, k + 1)
        if sg[k + 1] == 0.0:
            x = m0.copy()
        else:
            h = lam[k + 1] - lam[k]
            ht = (1.0 + tau) * h
            data = -np.expm1(-ht)  # 1 - e^(-h_tau)
            x = sg[k + 1] / sg[k] * np.exp(-tau * h) * x + al[k + 1] * data * m0
            if p == 2:
                r0 = (lam[k] - lam[k - 1]) / h
                x = x + 0.5 * al[k + 1] * data * (m0 - ms[-2]) / r0
            elif p == 3:
                r0, r1 = (lam[k] - lam[k - 1]) / h, (lam[k - 1] - lam[k - 2]) / h
                d1_0, d1_1 = (m0 - ms[-2]) / r0, (ms[-2] - ms[-3]) / r1
                d1 = d1_0 + (d1_0 - d1_1) * r0 / (r0 + r1)
                d2 = (d1_0 - d1_1) / (r0 + r1)
                phi2 = np.expm1(-ht) / ht + 1.0
                phi3 = phi2 / ht - 0.5
                x = x + al[k + 1] * (phi2 * d1 - phi3 * d2)
            if tau > 0:
                x = x + sg[k + 1] * np.sqrt(-np.expm1(-2.0 * tau * h)) * np.asarray(zs(k, x.shape), dtype=np.float64)
        xs.append(x.copy())
    return xs, ms


def stream_normals(seed, first_sample):
    """``zs`` of a ``NoiseStream(seed, first_sample)``: the float64 normals of the words of draw k (tag 0) for a [B, ...] shape."""
    return lambda k, shape: N.normals64(N.words(seed, first_sample, shape, k))[0]


# ---- Gaussian data: the exact covariance of the final sample ---------------------------------------------------------------------------
def gaussian_cov(coef, alpha, var):
    """The variance of the final sample of a run over ``coef`` (float64 rows) that starts from the true marginal N(0, a var + 1 - a)
    at the first row's level, for data ~ N(0, var) and its exact noise predictor eps = g_t x.  With m0 = k_t x the update is
    x' = (s3 k + c2 g + w1 k) x - (w1 - w2) m1 - w2 m2 + c1 z, m1' = k x, m2' = m1: P' = F P F^T + c1^2 e1 e1^T on the covariance of
    (x, m1, m2)."""
    a = torch.as_tensor(alpha).to("cpu", torch.float32).numpy().astype(np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    t0 = int(coef[0, 0])
    P = np.zeros((3, 3))
    P[0, 0] = a[t0] * var + 1.0 - a[t0]
    for t, s1, s2, s3, c2, c1, w1, w2 in coef:
        at = a[int(t)]
        g = np.sqrt(1.0 - at) / (at * var + 1.0 - at)
        k = (1.0 - s1 * g) / s2
        F = np.array([[s3 * k + c2 * g + w1 * k, -(w1 - w2), -w2], [k, 0.0, 0.0], [0.0, 1.0, 0.0]])
        P = F @ P @ F.T
        P[0, 0] += c1 * c1
    return float(P[0, 0])


def variance_error(coef, alpha, var):
    """|final variance - var| / var of ``gaussian_cov``."""
    return abs(gaussian_cov(coef, alpha, var) - var) / var
