"""fp64 restatement of ``ddim_audio_amd.invert_steps`` and ``ddim_audio_amd.slerp`` (test infrastructure).

The inversion is written from the equations with the quantities of ``solver_ref.levels`` (alpha_t = sqrt(a_t), sigma_t =
sqrt(1 - a_t)) -- NOT from the (p, q) columns of ``schedule.invert_coefficients`` -- and in another grouping: the decoder's step
x_j = alpha_j (x_i - sigma_i e) / alpha_i + sigma_j e, solved for x_i with e held fixed, is "predict the data from the point below,
put the same noise back at the level above":

    x0hat = (x_j - sigma_j e) / alpha_j,     x_i = alpha_i x0hat + sigma_i e.

So the two derivations check each other.  Works on numpy float64 arrays [B, ...] over any ``model_fn(x, t) -> eps``."""
import numpy as np

import solver_ref as R


def _levels_up(seq, alpha):
    """(alpha, sigma) of the data level (a = 1) followed by the levels of ``seq`` upwards."""
    al, sg, _ = R.levels(seq, alpha)  # execution order of the decoder: reversed seq, then a = 1
    return al[::-1], sg[::-1]


def _per_sample_norm(v):
    v = np.asarray(v, dtype=np.float64)
    return np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(axis=1)) if v.ndim > 1 else np.abs(v)


def invert_steps(x, seq, model_fn, alpha, iters):
    """Every level's (xs, x0_preds, residual), xs[0] = x; residual [len(seq), iters, B] (B = x.shape[0]; for 1-D x every element
    is its own sample): |cand_m - cand_{m-1}| / |cand_m| per sample, 0 where the denominator is 0.  x0_preds[k] is the
    prediction of level k's last evaluation, from the point that evaluation was made at."""
    seq = list(seq)
    al, sg = _levels_up(seq, alpha)
    x = np.asarray(x, dtype=np.float64)
    xs, preds, res = [x.copy()], [], []
    for k, t in enumerate(seq):
        base, cand, lvl = x, x, []
        for _ in range(iters):
            e = np.asarray(model_fn(cand, t), dtype=np.float64)
            pred = (cand - sg[k + 1] * e) / al[k + 1]
            x0hat = (base - sg[k] * e) / al[k]
            new = al[k + 1] * x0hat + sg[k + 1] * e
            num, den = _per_sample_norm(new - cand), _per_sample_norm(new)
            lvl.append(np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0))
            cand = new
        x = cand
        xs.append(x.copy())
        preds.append(pred)
        res.append(np.stack(lvl))
    return xs, preds, np.stack(res)


def table_steps(x, coef, model_fn):
    """The same trajectory from a ``schedule.invert_coefficients`` table (the (p, q) form the kernel computes), in float64:
    one entry per ROW of the table: (xs, x0_preds, residual [rows, B])."""
    x = np.asarray(x, dtype=np.float64)
    xs, preds, res = [x.copy()], [], []
    base = None
    for t, s1, s2, p, q, first in np.asarray(coef, dtype=np.float64):
        if first != 0.0:
            base = x
        e = np.asarray(model_fn(x, int(t)), dtype=np.float64)
        preds.append((x - s1 * e) / s2)
        new = p * base + q * e
        num, den = _per_sample_norm(new - x), _per_sample_norm(new)
        res.append(np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0))
        x = new
        xs.append(x.copy())
    return xs, preds, np.stack(res)


def ddim_decode(x, seq, model_fn, alpha):
    """``generalized_steps(eta=0)`` in float64: from level seq[-1] down to the data; returns the final sample."""
    xs, _ = R.dpm_solver_steps(x, seq, model_fn, alpha, 1)
    return xs[-1]


def round_trip_error(seq, alpha, var, iters, x=None, steps=invert_steps):
    """Relative error of invert -> DDIM decode on the Gaussian model, from x (default: 1)."""
    x = np.ones(1) if x is None else np.asarray(x, dtype=np.float64)
    fn = R.gaussian_model(alpha, var)
    back = ddim_decode(steps(x, seq, fn, alpha, iters)[0][-1], seq, fn, alpha)
    return float(np.abs(back - x).max() / np.abs(x).max())


def latent_error(seq, alpha, var, iters):
    """Relative error of the latent at seq[-1] against the closed-form probability-flow solution, from x = 1 at the data."""
    xs, _, _ = invert_steps(np.ones(1), seq, R.gaussian_model(alpha, var), alpha, iters)
    want = 1.0 / R.gaussian_exact(alpha, var, np.ones(1), seq[-1])  # the flow is linear: up is the reciprocal of down
    return float(np.abs(xs[-1] - want).max() / np.abs(want).max())


def slerp_coefficients(z1, z2, weights):
    """(a [M], b [M]) in float64 for one pair: theta from the whole sample; the straight line where sin(theta) = 0 or an input is
    all zero.  ``weights``: the fp32 values the kernel reads, as float64."""
    z1, z2 = np.asarray(z1, dtype=np.float64).reshape(-1), np.asarray(z2, dtype=np.float64).reshape(-1)
    w = np.asarray(weights, dtype=np.float64)
    n1, n2 = float(z1 @ z1), float(z2 @ z2)
    st = theta = 0.0
    if n1 > 0 and n2 > 0:
        theta = float(np.arccos(np.clip(float(z1 @ z2) / np.sqrt(n1 * n2), -1.0, 1.0)))
        st = float(np.sin(theta))
    if not st > 0:
        return 1.0 - w, w.copy()
    return np.sin((1.0 - w) * theta) / st, np.sin(w * theta) / st


def slerp(z1, z2, weights):
    """[P, M, ...] float64: pair-major, like the kernel's output."""
    z1, z2 = np.asarray(z1, dtype=np.float64), np.asarray(z2, dtype=np.float64)
    out = []
    for p in range(z1.shape[0]):
        a, b = slerp_coefficients(z1[p], z2[p], weights)
        out.append(np.stack([a[m] * z1[p] + b[m] * z2[p] for m in range(len(a))]))
    return np.stack(out)
