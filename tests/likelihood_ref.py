"""float64 reference of ``ddim_audio_amd.likelihood`` (numpy; the reference project has no such code): the table restated directly,
the integrator on the levels of a grid, the probe from tests/noise_ref.py's Philox words, the closed-form Gaussian models, and an
fp32 mirror of one ``lkx_stage`` row.  Written from the formulas of Song et al. 2021, appendix D.2, in the DDIM variables:

    u = x / alpha, s = sigma / alpha, du/ds = eps(alpha u, t)
    log p_{t0}(x_0) = log N(x_T; 0, I) + D log(alpha_T / alpha_0) + integral of alpha tr J_eps ds
"""
import math

import numpy as np

import noise_ref
from step_math_ref import fma32  # the one exact fp32 fused multiply-add of the tests

TAG_PROBE = 3
SAVE, COMMIT = 1, 2


def linear_alphas(n=1000, lo=1e-4, hi=0.02):
    """audio.yml's schedule as the library forms it: linear betas in float64, the cumulative product in fp32."""
    return np.cumprod((1.0 - np.linspace(lo, hi, n, dtype=np.float64)).astype(np.float32), dtype=np.float32)


def grid(n, levels=1000):
    return list(range(0, levels, levels // n)) + [levels - 1]


def levels(seq, alphas):
    """(alpha, sigma, s) of every level of seq, float64 from the fp32 table's values."""
    ab = np.asarray(alphas, dtype=np.float32).astype(np.float64)[list(seq)]
    al, sg = np.sqrt(ab), np.sqrt(1.0 - ab)
    return al, sg, sg / al


def rows(seq, alphas, order, prediction="eps"):
    """The rows (t, wk, we, a_next, wd, flags, 0, 0) restated: Euler one per interval, Heun a predictor and a trapezoid row; for v
    every wd times s2 = alpha of its own level.  Returns (rows, trace_per_dim, logdet_per_dim)."""
    al, sg, s = levels(seq, alphas)
    out, trace = [], 0.0
    for i in range(len(seq) - 1):
        h = s[i + 1] - s[i]
        if order == 1:
            stages = [(i, 0.0, h, h * al[i], COMMIT)]
        else:
            stages = [(i, 0.0, h, h * al[i] / 2, SAVE), (i + 1, h / 2, h / 2, h * al[i + 1] / 2, COMMIT)]
        for at, wk, we, w, fl in stages:
            s1, s2 = (sg[at], al[at]) if prediction == "v" else (0.0, 1.0)
            trace += w * s1
            out.append([float(seq[at]), wk, we, al[i + 1], w * s2, float(fl), 0.0, 0.0])
    return np.asarray(out, dtype=np.float64), trace, math.log(al[-1] / al[0])


def log_normal(x):
    """log N(x; 0, I) per sample of x [B, D]."""
    return -0.5 * (x * x).sum(axis=1) - 0.5 * x.shape[1] * math.log(2.0 * math.pi)


def integrate(x, seq, alphas, order, eps_div):
    """The float64 integrator, written as the two schemes and not through the rows: x [B, D]; ``eps_div(x, t)`` returns
    (eps [B, D], the divergence estimate [B]) of an eps model.  Returns (logp [B], x_T [B, D], evaluations)."""
    al, sg, s = levels(seq, alphas)
    u, acc, n_eval = x / al[0], np.zeros(x.shape[0]), 0
    for i in range(len(seq) - 1):
        h = s[i + 1] - s[i]
        e, d = eps_div(al[i] * u, seq[i])
        n_eval += 1
        if order == 1:
            u = u + h * e
            acc += h * al[i] * d
        else:
            e2, d2 = eps_div(al[i + 1] * (u + h * e), seq[i + 1])
            n_eval += 1
            u = u + 0.5 * h * (e + e2)
            acc += 0.5 * h * (al[i] * d + al[i + 1] * d2)
    xt = al[-1] * u
    return log_normal(xt) + x.shape[1] * math.log(al[-1] / al[0]) + acc, xt, n_eval


def stage32(u, k1, e, g, r, row):
    """One ``lkx_stage`` row on fp32 arrays, each operation rounded once: returns (u', k1', xin, d) with d the float64 sum of r g
    per sample (rows of the 2-D inputs), correctly rounded."""
    wk, we, an, flags = np.float32(row[1]), np.float32(row[2]), np.float32(row[3]), int(row[5])
    base = fma32(wk, k1, u) if wk != 0 else u
    un = fma32(we, e, base)
    xin = an * un  # fp32 x fp32 in numpy: one rounding
    d = exact_sum(r.astype(np.float64) * g.astype(np.float64))
    return (un if flags & COMMIT else u), (e.copy() if flags & SAVE else k1), xin, d


def exact_sum(a):
    """The correctly rounded float64 sum of every row of a (math.fsum): a reference with no summation error of its own."""
    return np.array([math.fsum(row) for row in np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1)])


def probe(seed, first_sample, shape, k):
    """The Rademacher probe of the samples first_sample .. of a [B, ...] tensor for probe index k: +1 where bit 31 of the Philox word
    is clear (counter (group, sample, k, 3))."""
    w = noise_ref.words(seed, first_sample, shape, k, TAG_PROBE)
    return np.where((w >> np.uint32(31)) == 0, 1.0, -1.0)


# ---- closed-form models -----------------------------------------------------------------------------------------------------------------
def iso_eps_div(alphas, var=0.25):
    """Isotropic Gaussian data of variance ``var``: eps*(x, t) = sigma x / (abar var + 1 - abar) and its exact divergence
    (J is a multiple of the identity, so r . J r = tr J for every Rademacher r)."""
    ab = np.asarray(alphas, dtype=np.float32).astype(np.float64)

    def fn(x, t):
        c = math.sqrt(1.0 - ab[t]) / (ab[t] * var + 1.0 - ab[t])
        return c * x, np.full(x.shape[0], c * x.shape[1])

    return fn


def iso_logp(x, alphas, t0, var=0.25):
    """The closed form: the marginal at level t0 is N(0, (abar var + 1 - abar) I)."""
    ab = float(np.float32(alphas[t0]))
    v = ab * var + 1.0 - ab
    return -0.5 * (x * x).sum(axis=1) / v - 0.5 * x.shape[1] * math.log(2.0 * math.pi * v)


def correlated_cov(d=12, seed=0):
    """A data covariance whose eigenvectors are no coordinate axes: the Jacobian of eps* is not diagonal."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return (q * np.linspace(0.05, 1.5, d)) @ q.T


def correlated_jacobian(cov, abar):
    """J of eps*(x) = sigma (abar Cov + (1 - abar) I)^-1 x, symmetric."""
    d = cov.shape[0]
    return math.sqrt(1.0 - abar) * np.linalg.inv(abar * cov + (1.0 - abar) * np.eye(d))
