"""fp64 restatement of ``ddim_audio_amd.dpm_solver_steps`` (test infrastructure).

DPM-Solver++ multistep, data-prediction form, written the way the paper states it (Lu et al. 2022, Algorithm 2 and its
third-order extension): noise levels sigma, half-log-SNR lam, step sizes h, ratios r, the divided differences D1 / D2 and the
phi terms -- NOT the (w1, w2) weights of ``schedule.dpm_coefficients``, so the two derivations check each other.  Works on
numpy float64 arrays (or floats) over any ``model_fn(x, t) -> eps``.  Also the one model whose probability-flow ODE has a closed
form: Gaussian data."""
import numpy as np
import torch


def levels(seq, alpha):
    """(alpha_t, sigma_t, lam_t) in float64 for the levels of a run in execution order: reversed ``seq``, then t = -1
    (alphas-cumprod 1: alpha = 1, sigma = 0, lam = +inf)."""
    a = torch.as_tensor(alpha).to("cpu", torch.float32).numpy().astype(np.float64)
    ac = np.array([a[t] for t in reversed(list(seq))] + [1.0])
    al, sg = np.sqrt(ac), np.sqrt(1.0 - ac)
    with np.errstate(divide="ignore"):
        lam = np.log(al) - np.log(sg)
    return al, sg, lam


def dpm_solver_steps(x, seq, model_fn, alpha, order):
    """Every iteration's (xs, x0_preds), xs[0] = x.  Lower-order start (iteration k runs at order min(order, k + 1)), and the
    final jump to t = -1 at order 1."""
    seq = list(seq)
    ts = list(reversed(seq))
    al, sg, lam = levels(seq, alpha)
    x = np.asarray(x, dtype=np.float64)
    xs, ms = [x.copy()], []
    for k, t in enumerate(ts):
        eps = np.asarray(model_fn(x, t), dtype=np.float64)
        m0 = (x - sg[k] * eps) / al[k]
        ms.append(m0)
        p = min(order, k + 1)
        if sg[k + 1] == 0.0:
            x = m0.copy()  # sigma_t / sigma_s = 0, alpha_t = 1, exp(-h) = 0: the first-order step lands on the prediction
        else:
            h = lam[k + 1] - lam[k]
            phi1 = np.expm1(-h)
            x = sg[k + 1] / sg[k] * x - al[k + 1] * phi1 * m0
            if p == 2:
                r0 = (lam[k] - lam[k - 1]) / h
                D1 = (m0 - ms[-2]) / r0
                x = x - 0.5 * al[k + 1] * phi1 * D1
            elif p == 3:
                r0, r1 = (lam[k] - lam[k - 1]) / h, (lam[k - 1] - lam[k - 2]) / h
                D1_0, D1_1 = (m0 - ms[-2]) / r0, (ms[-2] - ms[-3]) / r1
                D1 = D1_0 + r0 / (r0 + r1) * (D1_0 - D1_1)
                D2 = (D1_0 - D1_1) / (r0 + r1)
                phi2 = phi1 / h + 1.0
                phi3 = phi2 / h - 0.5
                x = x + al[k + 1] * phi2 * D1 - al[k + 1] * phi3 * D2
        xs.append(x.copy())
    return xs, ms


def table_steps(x, coef, model_fn):
    """The same trajectory from a ``schedule.dpm_coefficients`` table (the w-form the kernel computes), in float64."""
    x = np.asarray(x, dtype=np.float64)
    xs, ms = [x.copy()], []
    for t, s1, s2, s3, c2, _, w1, w2 in np.asarray(coef, dtype=np.float64):
        eps = np.asarray(model_fn(x, int(t)), dtype=np.float64)
        m0 = (x - s1 * eps) / s2
        u = s3 * m0 + c2 * eps
        if w1 != 0.0:
            u = u + w1 * (m0 - ms[-1])
        if w2 != 0.0:
            u = u + w2 * (ms[-1] - ms[-2])
        ms.append(m0)
        x = u
        xs.append(x.copy())
    return xs, ms


def gaussian_model(alpha, var):
    """The exact noise predictor of data ~ N(0, var I): eps(x, t) = sqrt(1 - a_t) x / (a_t var + 1 - a_t)."""
    a = torch.as_tensor(alpha).to("cpu", torch.float32).numpy().astype(np.float64)
    return lambda x, t: np.sqrt(1.0 - a[t]) * x / (a[t] * var + 1.0 - a[t])


def gaussian_exact(alpha, var, x_start, t_start, t=-1):
    """Closed-form solution of that model's probability-flow ODE from level t_start to level t (-1: a = 1):
    x_t = x_start sqrt(v_t / v_start), v_t = a_t var + 1 - a_t."""
    a = torch.as_tensor(alpha).to("cpu", torch.float32).numpy().astype(np.float64)
    v = lambda u: 1.0 * var if u < 0 else a[u] * var + 1.0 - a[u]  # noqa: E731
    return np.asarray(x_start, dtype=np.float64) * np.sqrt(v(t) / v(t_start))


def final_error(seq, alpha, order, var, steps=dpm_solver_steps):
    """Relative error of the final sample of a run that starts at x = 1 on level seq[-1]."""
    xs, _ = steps(np.ones(1), seq, gaussian_model(alpha, var), alpha, order)
    want = gaussian_exact(alpha, var, np.ones(1), seq[-1])
    return float(np.abs(xs[-1] - want).max() / np.abs(want).max())
