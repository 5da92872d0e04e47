"""fp64 restatement of ``ddim_audio_amd.dpm_solver_steps`` (test infrastructure).

DPM-Solver++ multistep, data-prediction form, written the way the paper states it (Lu et al. 2022, Algorithm 2 and its
third-order extension): noise levels sigma, half-log-SNR lam, step sizes h, ratios r, the divided differences D1 / D2 and the
phi terms -- NOT the (w1, w2) weights of ``schedule.dpm_coefficients``, so the two derivations check each other.  Works on
numpy float64 arrays (or floats) over any ``model_fn(x, t) -> eps``.  Also the float64 walker of a coefficient table -- every
sampler's: ``table_row`` / ``table_steps`` --, the one model whose probability-flow ODE has a closed form (Gaussian data), and the
model and the sequences the CPU tests of the tables share."""
import numpy as np
import torch

from ddim_audio_amd.schedule import logsnr_seq, make_seq


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


def table_row(x, eps, m1, m2, m3, row, z=None):
    """One update in float64 on one coefficient row, the form every update kernel computes (csrc/step_math.h): (u, m0) with
    m0 = (x - s1 eps) / s2, u = s3 m0 + c2 eps, + w1 (m0 - m1), + w2 (m1 - m2), + w3 (m2 - m3), + c1 z, each term only where its
    weight is not 0 (its operand may then be None; ``z`` may be a callable that draws it).  ``row``: (t, s1, s2, s3, c2, c1) and,
    where the table has them, w1, w2 and w3 -- 6, 8 or 9 columns."""
    _, s1, s2, s3, c2, c1, w1, w2, w3 = tuple(np.asarray(row, dtype=np.float64)) + (0.0,) * (9 - len(row))
    m0 = (x - s1 * eps) / s2
    u = s3 * m0 + c2 * eps
    if w1 != 0.0:
        u = u + w1 * (m0 - m1)
    if w2 != 0.0:
        u = u + w2 * (m1 - m2)
    if w3 != 0.0:
        u = u + w3 * (m2 - m3)
    if c1 != 0.0:
        u = u + c1 * np.asarray(z() if callable(z) else z, dtype=np.float64)
    return u, m0


def table_steps(x, coef, model_fn, zs=None):
    """Every iteration's (xs, x0_preds) from a coefficient table of ``schedule.ddim_coefficients``, ``dpm_coefficients`` or
    ``unic_coefficients`` (the folded form the kernels compute), in float64: ``table_row`` row after row.  ``zs(k, shape)``: the
    standard normals of iteration k, asked for only where c1 != 0."""
    x = np.asarray(x, dtype=np.float64)
    xs, ms = [x.copy()], [None, None, None]
    for k, row in enumerate(np.asarray(coef, dtype=np.float64)):
        eps = np.asarray(model_fn(x, int(row[0])), dtype=np.float64)
        x, m0 = table_row(x, eps, ms[-1], ms[-2], ms[-3], row, lambda: zs(k, x.shape))
        ms.append(m0)
        xs.append(x.copy())
    return xs, ms[3:]


def gaussian_model(alpha, var):
    """The exact noise predictor of data ~ N(0, var I): eps(x, t) = sqrt(1 - a_t) x / (a_t var + 1 - a_t)."""
    a = torch.as_tensor(alpha).to("cpu", torch.float32).numpy().astype(np.float64)
    return lambda x, t: np.sqrt(1.0 - a[t]) * x / (a[t] * var + 1.0 - a[t])


def tanh_model(alpha):
    """A smooth model that is no Gaussian's predictor: the tests that compare two forms of one update on something nonlinear."""
    a = torch.as_tensor(alpha).numpy().astype(np.float64)
    return lambda x, t: np.tanh(1.5 * x + 0.3) * np.sqrt(1.0 - a[t]) + 0.1 * np.sin(x * (1.0 + t / 500.0))


def seqs(alpha):
    """The timestep sequences every table test walks: uniform, the log-SNR grid, a single level, and one that starts off 0."""
    return {"uniform": make_seq(1000, 10), "logsnr": logsnr_seq(alpha, 20), "single": [250], "offset": [13, 400, 999]}


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
