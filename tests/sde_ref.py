"""References of SDE-DPM-Solver++ (``dpm_solver_steps(tau > 0)``, ``ddimxs_multistep_update``; test infrastructure).

Four restatements, each written on its own so that they check each other and the library:

* ``table_steps_z`` -- ``solver_ref.table_steps`` plus c1 z, in the kernel's order, in float64, from a ``schedule.dpm_coefficients``
  table (the w-form the kernel computes);
* ``sde_steps`` -- the published update (Lu et al. 2022, appendix, SDE-DPM-Solver++(2M); the 3M SDE scheme as it circulates), with
  noise levels, half-log-SNR, the differences D1 / d1, d2 and the phi terms -- NOT the table's weights;
* ``updater32`` / ``update32`` -- one update of the kernel in fp32, every operation rounded once (an exact fused multiply-add: ``fma32``), the bits
  the kernel must give;
* ``gaussian_cov`` -- for Gaussian data and its exact noise predictor (``solver_ref.gaussian_model``) every update is linear in
  (x, m1, m2), so the covariance of the final sample follows exactly from a 3 x 3 recursion.
"""
import numpy as np
import torch

import noise_ref as N
import solver_ref as R

F32 = np.float32


# ---- float64: the table's form and the published form --------------------------------------------------------------------------------
def table_steps_z(x, coef, model_fn, zs):
    """Every iteration's (xs, x0_preds) from a coefficient table, ``solver_ref.table_steps`` with the noise term last:
    u = s3 m0 + c2 eps, + w1 (m0 - m1), + w2 (m1 - m2), + c1 z.  ``zs(k, shape)``: the standard normals of iteration k (asked for
    only where c1 != 0)."""
    x = np.asarray(x, dtype=np.float64)
    xs, ms = [x.copy()], []
    for k, (t, s1, s2, s3, c2, c1, w1, w2) in enumerate(np.asarray(coef, dtype=np.float64)):
        eps = np.asarray(model_fn(x, int(t)), dtype=np.float64)
        m0 = (x - s1 * eps) / s2
        u = s3 * m0 + c2 * eps
        if w1 != 0.0:
            u = u + w1 * (m0 - ms[-1])
        if w2 != 0.0:
            u = u + w2 * (ms[-1] - ms[-2])
        if c1 != 0.0:
            u = u + c1 * np.asarray(zs(k, x.shape), dtype=np.float64)
        ms.append(m0)
        x = u
        xs.append(x.copy())
    return xs, ms


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


# ---- fp32: the kernel's bits -------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """An exact fp32 fused multiply-add, element-wise: rn32(a b + c).  The product of two fp32 numbers is exact in fp64, and
    s = rn64(product + c) rounded again to fp32 is the single rounding of the exact sum unless s lies exactly half way between two
    fp32 neighbours (the 29 bits fp32 drops are 1 0...0) while the exact sum does not: only those elements, and results below the
    normal fp32 range, where the half-way pattern sits elsewhere, go the slow way -- s is re-rounded TO ODD from the error term
    of the two-sum (which says whether the sum was exact and on which side of s it lies), and that value rounds to fp32 once
    (53 >= 24 + 2 bits)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    risky = np.flatnonzero(((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000).ravel() | (np.abs(s) < 2.0 ** -126).ravel())
    if risky.size:
        pr, cr, sr = p.ravel()[risky], c.ravel()[risky], s.ravel()[risky]
        bb = sr - pr
        err = (pr - (sr - bb)) + (cr - bb)  # two-sum: p + c = s + err exactly
        even = (sr.view(np.int64) & 1) == 0
        sr = np.where((err != 0) & even, np.nextafter(sr, np.where(err > 0, np.inf, -np.inf)), sr)
        s = s.copy().ravel()
        s[risky] = sr
        s = s.reshape(p.shape)
    return s.astype(F32)


def updater32(x, e, z, m1, m2):
    """``ddimxs_multistep_update`` on fp32 arrays as a function of (row, hist): (xt, x0, hist) after the call; ``hist`` False: a null
    history buffer (no second history term, nothing kept; the third result is None).  row: (t, s1, s2, s3, c2, c1, w1, w2) fp32.
    Operation for operation ``step_math.h`` and the kernel's comment: fma and division, product and fma, subtraction and fma
    twice, fma.  Every stage is kept under the scalars it depends on, so rows that share a prefix of the chain share its cost."""
    x, e, z, m1, m2 = (np.asarray(v, dtype=F32) for v in (x, e, z, m1, m2))
    memo = {}

    def stage(key, fn):
        if key not in memo:
            memo[key] = fn()
        return memo[key]

    def update(row, hist=True):
        _, s1, s2, s3, c2, c1, w1, w2 = (F32(v) for v in row)
        key = (float(s1), float(s2))
        m0 = stage(key, lambda: (fma32(e, -s1, x) / s2).astype(F32))
        key += (float(s3), float(c2))
        u = stage(key, lambda: fma32(e, c2, (m0 * s3).astype(F32)))
        if w1 != 0:
            key += ("w1", float(w1))
            u = stage(key, lambda u=u: fma32(w1, (m0 - m1).astype(F32), u))
        if w2 != 0 and hist:
            key += ("w2", float(w2))
            u = stage(key, lambda u=u: fma32(w2, (m1 - m2).astype(F32), u))
        if c1 != 0:
            key += ("c1", float(c1))
            u = stage(key, lambda u=u: fma32(z, c1, u))
        return u, m0, (m1.copy() if hist else None)

    return update


def update32(x, e, z, m1, m2, row, hist=True):
    """One ``ddimxs_multistep_update``: ``updater32(x, e, z, m1, m2)(row, hist)``."""
    return updater32(x, e, z, m1, m2)(row, hist)


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
