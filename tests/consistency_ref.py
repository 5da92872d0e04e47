"""Restatements of consistency distillation and consistency sampling for the tests (include/cmx_consistency.h,
ddim_audio_amd/consistency.py): float64 ones written from the method's definitions -- c_skip, c_out and the network's data
prediction, not the (p, q) table the library evaluates -- and fp32 mirrors of the four kernels, operation for operation, on
tests/step_math_ref.py (the fused multiply-add) and tests/tail_kernel_ref.py (the loss's two-stage reduction: the only Python copy
of it).  numpy only; nothing is shared with ddim_audio_amd/schedule.py or the kernels."""
import numpy as np

import step_math_ref as SM
import tail_kernel_ref as TK

F = np.float32


def table64(alphas):
    """The fp32 alphas-cumprod table's values as float64."""
    return np.asarray(alphas, dtype=np.float32).astype(np.float64)


def alpha_sigma(a, t):
    """(alpha, sigma) = (sqrt(a_t), sqrt(1 - a_t)); t = -1 is the data: (1, 0)."""
    at = 1.0 if t < 0 else float(a[t])
    return np.sqrt(at), np.sqrt(1.0 - at)


# ---- float64, from the definitions --------------------------------------------------------------------------------------------------------
def scalings(t, sigma_data=0.5, timestep_scale=10.0, t_min=0):
    """(c_skip, c_out) of Luo et al. 2023 at timestep t."""
    u = timestep_scale * max(t - t_min, 0)
    return sigma_data ** 2 / (u ** 2 + sigma_data ** 2), u / np.sqrt(u ** 2 + sigma_data ** 2)


def x0_hat(x, out, a, t, prediction):
    """The data prediction of a network whose raw output at (x, t) is ``out``."""
    al, si = alpha_sigma(a, t)
    return (x - si * out) / al if prediction == "eps" else al * x - si * out


def f64(x, out, a, t, prediction, **kw):
    """The consistency function c_skip x + c_out x0_hat, float64; the identity at t <= t_min whatever ``out`` is."""
    if t <= kw.get("t_min", 0):
        return np.asarray(x, dtype=np.float64) + 0.0 * np.asarray(out, dtype=np.float64)
    c_skip, c_out = scalings(t, **kw)
    return c_skip * np.asarray(x, dtype=np.float64) + c_out * x0_hat(np.asarray(x, np.float64), np.asarray(out, np.float64), a, t, prediction)


def pq(a, t, prediction, **kw):
    """(p, q) with f = p x + q out, read off ``f64`` at the two unit inputs."""
    return float(f64(1.0, 0.0, a, t, prediction, **kw)), float(f64(0.0, 1.0, a, t, prediction, **kw))


def distance64(S, c):
    """The distance of a per-sample sum of squares S: S itself, or the pseudo-Huber sqrt(S + c^2) - c in its DIRECT form, in
    extended precision so that its cancellation at S << c^2 stays below what the tests count."""
    if c == 0:
        return np.asarray(S, dtype=np.float64)
    S, c = np.asarray(S, dtype=np.longdouble), np.longdouble(c)
    return np.asarray(np.sqrt(S + c * c) - c, dtype=np.float64)


def loss64(f, y, c=0.0):
    """([B] distances, their mean, [B] sums of squares) of d(y_b, f_b), float64."""
    d = np.asarray(y, np.float64) - np.asarray(f, np.float64)
    S = (d * d).reshape(d.shape[0], -1).sum(axis=1)
    per = distance64(S, c)
    return per, per.mean(), S


def loss_bwd64(f, y, q, g, c=0.0):
    """d loss / d out for the upstream gradient g [B + 1] of (per-sample distances, mean): q k_b (f - y) with k_b = 2 (g[b] + g[B] /
    B), over 2 sqrt(S_b + c^2) for the pseudo-Huber."""
    f, y, g = np.asarray(f, np.float64), np.asarray(y, np.float64), np.asarray(g, np.float64)
    B = f.shape[0]
    k = 2.0 * (g[:B] + g[B] / B)
    if c:
        k = k / (2.0 * np.sqrt(loss64(f, y)[2] + c * c))
    return (np.asarray(q, np.float64) * k).reshape(B, *([1] * (f.ndim - 1))) * (f - y)


def ddim_step(z, eps, a, t, t_next):
    """One reference DDIM step at eta = 0 in float64: z at t_next."""
    al, si = alpha_sigma(a, t)
    al_n, si_n = alpha_sigma(a, t_next)
    return al_n * (z - si * eps) / al + si_n * eps


def target64(target_out, teacher_eps, z, t_hi, t_lo, alphas, target_prediction, **kw):
    """y for ONE level pair and a batch z: the teacher's DDIM step t_hi -> t_lo, then f of the target network there.
    ``teacher_eps(z, t)`` and ``target_out(z, t)`` return float64 arrays (the teacher's eps, the target's raw output)."""
    a = table64(alphas)
    z_hat = ddim_step(z, teacher_eps(z, t_hi), a, t_hi, t_lo)
    return f64(z_hat, target_out(z_hat, t_lo), a, t_lo, target_prediction, **kw)


def sample64(out_fn, x, seq, alphas, prediction, noises, **kw):
    """Multistep consistency sampling in float64: ([x after each iteration], [x0 prediction of each]); ``noises[i]`` is the z of
    iteration i (unused in the last), ``out_fn(x, t)`` the network's raw output."""
    a = table64(alphas)
    x = np.asarray(x, dtype=np.float64)
    xs, x0s = [], []
    for i, j in enumerate(reversed(range(len(seq)))):
        x0 = f64(x, out_fn(x, seq[j]), a, seq[j], prediction, **kw)
        if j:
            al, si = alpha_sigma(a, seq[j - 1])
            x = al * x0 + si * np.asarray(noises[i], dtype=np.float64)
        else:
            x = x0
        xs.append(x)
        x0s.append(x0)
    return xs, x0s


# ---- fp32 mirrors of the kernels ----------------------------------------------------------------------------------------------------------
def f32(x, out, p, q):
    """``consistency_f`` (step_math.h): fma(q, out, rn(p x)); p, q scalars or [B, 1] columns."""
    return SM.v_to_eps(x, out, p, q)


def loss32(x, out, y, p, q, c=0.0):
    """``cmx_consistency_loss``'s [B + 1] vector: the squared-error loss's reduction (``tail_kernel_ref.sqerr_mirror``) on (y, f),
    then the distance per sample and the running mean, every operation in fp32 and in the header's order."""
    with np.errstate(all="ignore"):
        S = TK.sqerr_mirror(np.asarray(y, F), f32(x, out, p, q))
        B = S.shape[0] - 1
        if not c > 0:
            return S
        c = F(c)
        loss = np.zeros(B + 1, F)
        tot = F(0)
        for b in range(B):
            loss[b] = S[b] / (np.sqrt(F(S[b] + F(c * c))) + c)
            tot = F(tot + loss[b])
        loss[B] = tot / F(B)
        return loss


def loss_bwd32(x, out, y, p, q, g, loss, c=0.0):
    """``cmx_consistency_loss_bwd``: d_out [B][per] in fp32, the header's operations in its order."""
    with np.errstate(all="ignore"):
        B = x.shape[0]
        g, loss = np.asarray(g, F), np.asarray(loss, F)
        k = F(2.0) * (g[:B] + g[B] / F(B))
        if c > 0:
            k = k / (F(2.0) * (loss[:B] + F(c)))
        cq = (np.asarray(q, F).reshape(-1) * k).astype(F)
        return cq[:, None] * (f32(x, out, p, q) - np.asarray(y, F))


def update32(xt, out, row, z=None):
    """``cmx_consistency_update`` on one row (t, p, q, a_next, 0, c1, 0, 0): (xt, x0) after the call, fp32."""
    with np.errstate(all="ignore"):
        row = np.asarray(row, F)
        m = f32(xt, out, row[1], row[2])
        u = row[3] * m
        if row[5] != 0:
            u = SM.fma32(z, row[5], u)
        return u, m


# ---- the Gaussian model: data N(0, var), exact predictor, linear students -----------------------------------------------------------------
def gaussian_ddim_factor(a, t_hi, t_lo, var):
    """x at t_lo = D x at t_hi under one eta = 0 DDIM step of the exact predictor E[x0 | x] = alpha var / (alpha^2 var + sigma^2) x."""
    (al, si), (al_n, si_n) = alpha_sigma(a, t_hi), alpha_sigma(a, t_lo)
    vt = al * al * var + si * si
    x0 = al * var / vt
    return al_n * x0 + si_n * (1.0 - al * x0) / si


def gaussian_flow(a, t_hi, t_lo, var):
    """The exact probability-flow map between two levels: the ratio of the marginals' standard deviations."""
    (al, si), (al_n, si_n) = alpha_sigma(a, t_hi), alpha_sigma(a, t_lo)
    return np.sqrt((al_n * al_n * var + si_n * si_n) / (al * al * var + si * si))


def gaussian_fixed_point(a, seq, var, prediction, skip=1, **kw):
    """The student f(x, t) = theta_t x the distillation recursion converges to on the levels ``seq``, by back-substitution: at
    level S[n + skip] the least-squares output of a linear network out = w x against the target theta_{S[n]} D x is
    w = (theta_{S[n]} D - p) / q, and theta = p + q w.  Returns {level: theta}; levels below S[skip] that no pair reaches from
    S[0] keep the identity."""
    theta = {t: 1.0 for t in seq[:skip]}
    for n in range(len(seq) - skip):
        hi, lo = seq[n + skip], seq[n]
        p, q = pq(a, hi, prediction, **kw)
        w = (theta[lo] * gaussian_ddim_factor(a, hi, lo, var) - p) / q
        theta[hi] = p + q * w
    return theta


def uniform_levels(n, top=999):
    """n levels from 0 to ``top``, as even as integers allow."""
    return sorted({int(round(top * i / (n - 1))) for i in range(n)})
