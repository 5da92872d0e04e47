"""fp64 restatement of ``ddim_audio_amd.dpm_solver_steps(corrector=True)`` (test infrastructure).

DPM-Solver++ multistep with the UniC corrector of UniPC (Zhao et al. 2023), data-prediction form with B(h) = h ("bh1"), written
the way the paper states it, in two passes: the corrected sample is KEPT, every iteration corrects it with the prediction the
network just made at the predicted sample, and the predictor (``solver_ref``'s D-form) then steps from the corrected sample.
Nothing here knows the folded weights of ``schedule.unic_coefficients``, so the two derivations check each other
(``solver_ref.table_steps`` walks that 9-column table as the kernel computes it; ``step_math_ref.updater32`` gives one update's
bits)."""
import math

import numpy as np

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


def final_error(seq, alpha, order, var):
    """Relative error of the final sample of a corrector run that starts at x = 1 on level seq[-1] (``solver_ref.final_error``)."""
    xs, _ = unic_steps(np.ones(1), seq, gaussian_model(alpha, var), alpha, order)
    want = gaussian_exact(alpha, var, np.ones(1), seq[-1])
    return float(np.abs(xs[-1] - want).max() / np.abs(want).max())
