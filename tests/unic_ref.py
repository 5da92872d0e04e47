"""fp64 restatement of ``ddim_audio_amd.dpm_solver_steps(corrector=True)`` (test infrastructure).

DPM-Solver++ multistep with the UniC corrector of UniPC (Zhao et al. 2023), data-prediction form with B(h) = h ("bh1"), written
the way the paper states it, in two passes: the corrected sample is KEPT, every iteration corrects it with the prediction the
network just made at the predicted sample, and the predictor (``solver_ref``'s D-form) then steps from the corrected sample.
Nothing here knows the folded weights of ``schedule.unic_coefficients``, so the two derivations check each other.  Also the
same trajectory from that 9-column table, as the kernel computes it, and one update of the kernel in fp32, every operation
rounded once."""
import math

import numpy as np

from sde_ref import F32, fma32
from solver_ref import gaussian_exact, gaussian_model, levels


def unic_rho(lam, k, q):
    """(rho [q], r [q]) of the corrector of order q at iteration k: nodes r_j = (lam[k-1-j] - lam[k-1]) / h' for j < q, r_q = 1;
    rho solves sum_j r_j^(i-1) rho_j = g_i i! / hh, hh = -h' (rho = 1/2 at q = 1)."""
    hp = lam[k] - lam[k - 1]
    hh = -hp
    r = np.array([(lam[k - 1 - j] - lam[k - 1]) / hp for j in range(1, q)] + [1.0])
    g, b = np.expm1(hh) / hh - 1.0, []
    for i in range(1, q + 1):
        b.append(g * math.factorial(i) / hh)
        g = g / hh - 1.0 / math.factorial(i + 1)
    if q == 1:
        return np.array([0.5]), r
    R = np.array([r ** (i - 1) for i in range(1, q + 1)])
    return np.linalg.solve(R, np.array(b)), r


def unic_steps(x, seq, model_fn, alpha, order):
    """Every iteration's (xs, x0_preds), xs[0] = x: ``xs`` holds the predictor's samples (what the network sees), the corrected
    sample lives between the iterations only.  Lower-order start: the corrector of iteration k runs at order min(order, k), the
    predictor at min(order, k + 1); the final jump to t = -1 is first order and lands on the prediction."""
    ts = list(reversed(list(seq)))
    al, sg, lam = levels(seq, alpha)
    x = np.asarray(x, dtype=np.float64)
    xs, ms = [x.copy()], []
    xc_prev = None
    for k, t in enumerate(ts):
        eps = np.asarray(model_fn(x, t), dtype=np.float64)
        m0 = (x - sg[k] * eps) / al[k]
        xc = x
        if k >= 1 and sg[k + 1] != 0.0:  # nothing to correct at k = 0; the final jump does not read the sample
            q = min(order, k)
            hp = lam[k] - lam[k - 1]
            rho, r = unic_rho(lam, k, q)
            m1 = ms[-1]
            acc = rho[q - 1] * (m0 - m1)
            for j in range(1, q):
                acc = acc + rho[j - 1] * (ms[-1 - j] - m1) / r[j - 1]
            xc = sg[k] / sg[k - 1] * xc_prev - al[k] * np.expm1(-hp) * m1 - al[k] * (-hp) * acc
        ms.append(m0)
        p = min(order, k + 1)
        if sg[k + 1] == 0.0:
            x = m0.copy()
        else:
            h = lam[k + 1] - lam[k]
            phi1 = np.expm1(-h)
            x = sg[k + 1] / sg[k] * xc - al[k + 1] * phi1 * m0
            if p == 2:
                r0 = (lam[k] - lam[k - 1]) / h
                x = x - 0.5 * al[k + 1] * phi1 * (m0 - ms[-2]) / r0
            elif p == 3:
                r0, r1 = (lam[k] - lam[k - 1]) / h, (lam[k - 1] - lam[k - 2]) / h
                D1_0, D1_1 = (m0 - ms[-2]) / r0, (ms[-2] - ms[-3]) / r1
                D1 = D1_0 + r0 / (r0 + r1) * (D1_0 - D1_1)
                D2 = (D1_0 - D1_1) / (r0 + r1)
                phi2 = phi1 / h + 1.0
                phi3 = phi2 / h - 0.5
                x = x + al[k + 1] * phi2 * D1 - al[k + 1] * phi3 * D2
        xc_prev = xc
        xs.append(x.copy())
    return xs, ms


def table_steps(x, coef, model_fn):
    """The same trajectory from a ``schedule.unic_coefficients`` table (the folded form the kernel computes), in float64."""
    x = np.asarray(x, dtype=np.float64)
    xs, ms = [x.copy()], []
    for t, s1, s2, s3, c2, _, w1, w2, w3 in np.asarray(coef, dtype=np.float64):
        eps = np.asarray(model_fn(x, int(t)), dtype=np.float64)
        m0 = (x - s1 * eps) / s2
        u = s3 * m0 + c2 * eps
        if w1 != 0.0:
            u = u + w1 * (m0 - ms[-1])
        if w2 != 0.0:
            u = u + w2 * (ms[-1] - ms[-2])
        if w3 != 0.0:
            u = u + w3 * (ms[-2] - ms[-3])
        ms.append(m0)
        x = u
        xs.append(x.copy())
    return xs, ms


def final_error(seq, alpha, order, var):
    """Relative error of the final sample of a corrector run that starts at x = 1 on level seq[-1] (``solver_ref.final_error``)."""
    xs, _ = unic_steps(np.ones(1), seq, gaussian_model(alpha, var), alpha, order)
    want = gaussian_exact(alpha, var, np.ones(1), seq[-1])
    return float(np.abs(xs[-1] - want).max() / np.abs(want).max())


# ---- fp32: the kernel's bits -------------------------------------------------------------------------------------------------------------
def updater32(x, e, m1, m2, m3):
    """``ddimxu_multistep_update`` on fp32 arrays as a function of (row, hist, hist2): (xt, x0) after the call; ``hist`` / ``hist2``
    False: a null buffer, whose term is not applied.  What the call leaves in the history buffers is a plain move (hist <- the old
    x0, hist2 <- the old hist) and is the caller's to compare.  row: (t, s1, s2, s3, c2, c1, w1, w2, w3) fp32; c1 is not read.
    Operation for operation ``step_math.h``: fma and division, product and fma, then subtraction and fma per history term.  Every
    stage is kept under the terms applied so far, so rows that share a prefix of the chain share its cost; m1, m2, m3 are read
    only by the terms that are applied."""
    x, e, m1, m2, m3 = (np.asarray(v, dtype=F32) for v in (x, e, m1, m2, m3))
    memo = {}

    def stage(key, fn):
        if key not in memo:
            memo[key] = fn()
        return memo[key]

    def update(row, hist=True, hist2=True):
        _, s1, s2, s3, c2, _, w1, w2, w3 = (F32(v) for v in row)
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
        if w3 != 0 and hist and hist2:
            key += ("w3", float(w3))
            u = stage(key, lambda u=u: fma32(w3, (m2 - m3).astype(F32), u))
        return u, m0

    return update
