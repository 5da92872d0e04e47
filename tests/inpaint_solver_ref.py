"""Restatements of ``ddim_audio_amd.inpaint_solver_steps`` (test infrastructure).

* ``solver_steps``: steps 1-6 of the definition in plain torch ops over ``model_fn(x, t) -> eps`` (the CPU oracle, or the exact
  predictor of a Gaussian), in the dtype of ``x`` (fp64 for the studies), with the guidance gradient taken the plain way --
  ``torch.autograd.grad`` of L_b = sum (m (x0 - y))^2 w.r.t. x_t, not the k1 / k2 decomposition the kernels use.  Two switches
  restate what the function deliberately is NOT: ``known="eps"`` is ``inpaint_steps``' replacement s3 y + c2 eps, and
  ``guide="euler"`` subtracts zeta / sqrt(L) g from x_{t-1} as ``inpaint_steps`` does (``guidance`` then holds zeta); with both
  and order 1 it is ``inpaint_steps``.
* ``gaussian_case``: the committed-in-code fixture of the convergence study -- a 12-dimensional correlated Gaussian with its exact
  eps predictor, 5 known coordinates.
* ``update32``: one call of ``ddimxi_multistep_update`` on fp32 arrays, every operation rounded once and in the documented order
  (include/ddimx_inpaint_solver.h): the kernel's own body over ``step_math_ref``'s scalar operations."""
import numpy as np
import torch

from ddim_audio_amd.schedule import dpm_coefficients, logsnr_seq
import step_math_ref as SM

F32 = np.float32


def _per_iteration(v, n):
    v = np.asarray(v, dtype=np.float64)
    return np.full(n, float(v)) if v.ndim == 0 else v


def solver_steps(x, seq, model_fn, alpha, y, mask, guidance=0.0, replace=True, order=2, tau=0.0, noise_fn=None, known="exact",
                 guide="fold"):
    """Every iteration's (xs, x0_preds), xs[0] = x.  ``noise_fn(index, xt)`` gives z on rows with c1 != 0."""
    coef = dpm_coefficients(seq, alpha, order, tau)
    rho = _per_iteration(guidance, coef.shape[0])
    guided = bool((rho != 0).any())
    m = torch.broadcast_to(mask.to(x.dtype), x.shape)
    yk = torch.where(m == 0, torch.zeros((), dtype=x.dtype), torch.broadcast_to(y.to(x.dtype), x.shape))
    view = (-1,) + (1,) * (x.dim() - 1)
    xt = x.clone()
    xs, x0s, hist = [x.clone()], [], []
    for i, row in enumerate(coef):
        ti, s1, s2, s3, c2, c1, w1, w2 = [float(v) for v in row]
        t = torch.full((xt.size(0),), int(ti), dtype=torch.long)
        z = noise_fn(i, xt) if c1 != 0.0 else None
        if guided:
            xg = xt.detach().clone().requires_grad_(True)
            with torch.enable_grad():
                e = model_fn(xg, t)
                m0 = (xg - s1 * e) / s2
                L = (m * (m0 - yk)).square().flatten(1).sum(1)
                (g,) = torch.autograd.grad(L.sum(), xg)  # samples are independent: d L_b / d x_t for every b
            e, m0, L = e.detach(), m0.detach(), L.detach()
            w = torch.where(L > 0, rho[i] / L.clamp_min(torch.finfo(L.dtype).tiny).sqrt(), torch.zeros_like(L)).view(view)
        else:
            with torch.no_grad():
                e = model_fn(xt, t)
                m0 = (xt - s1 * e) / s2
            g = w = None
        cx, w0 = c2 / s1, s3 - c2 * s2 / s1
        mt = m0 - w * g if guided and guide == "fold" else m0
        u = s3 * m0 + c2 * e + w0 * (mt - m0)
        if w1 != 0.0:
            u = u + w1 * (mt - hist[-1])
        if w2 != 0.0:
            u = u + w2 * (hist[-1] - hist[-2])
        if z is not None:
            u = u + c1 * z
        if guided and guide == "euler":
            u = u - w * g
        if replace:
            k = cx * xt + w0 * yk if known == "exact" else s3 * yk + c2 * e
            if z is not None:
                k = k + c1 * z
            u = m * k + (1 - m) * u
        hist.append(mt)
        xt = u
        xs.append(xt.clone())
        x0s.append(m0.clone())
    return xs, x0s


# ---- the convergence study's fixture ---------------------------------------------------------------------------------------------------
DIM, KNOWN = 12, 5
REF_LEVELS = 734  # logsnr_seq(alpha, 734): 562 levels on audio.yml's schedule


def gaussian_case(alpha, seed=20261020):
    """(model_fn, x_T [1, 12], y [12], mask [12]) in float64 and the table M [n_table, 12, 12] of the exact eps predictor
    eps(x, t) = M[t] x of x0 ~ N(0, S): M[t] = sqrt(1 - a) (a S + (1 - a) I)^-1, S = A A^T / 12 + 0.05 I from a fixed numpy seed.
    y is a draw of N(0, S), of which the first 5 coordinates are known."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((DIM, DIM))
    S = A @ A.T / DIM + 0.05 * np.eye(DIM)
    a = torch.as_tensor(alpha).double().numpy()
    M = torch.from_numpy(np.stack([np.sqrt(1.0 - at) * np.linalg.inv(at * S + (1.0 - at) * np.eye(DIM)) for at in a]))
    y = torch.from_numpy(np.linalg.cholesky(S) @ rng.standard_normal(DIM))
    x = torch.from_numpy(rng.standard_normal((1, DIM)))
    mask = torch.zeros(DIM, dtype=torch.float64)
    mask[:KNOWN] = 1.0
    return (lambda xx, t: torch.einsum("bij,bj->bi", M[t].to(xx.dtype), xx)), x, y, mask, M


MODES = {"replace": dict(guidance=0.0, replace=True), "guided+replace": dict(guidance=0.3, replace=True),
         "guided": dict(guidance=0.3, replace=False), "eps-path replace": dict(guidance=0.0, replace=True, known="eps")}
STEPS, ORDERS = (10, 20, 50, 100), (1, 2, 3)


def study(alpha, seed=20261020, modes=MODES, steps=STEPS, orders=ORDERS, final=None):
    """{mode: {(requested steps, order): error}}: the relative L2 distance of the final sample from the mode's own order-2 run on
    logsnr_seq(alpha, REF_LEVELS), in float64.  ``final(seq, order, **mode)`` (default: ``solver_steps`` on the fixture) returns a
    run's final sample."""
    fn, x, y, mask, _ = gaussian_case(alpha, seed)

    def run(seq, order, **kw):
        return solver_steps(x, seq, fn, alpha, y, mask, order=order, **kw)[0][-1]

    out = {}
    for name, kw in modes.items():
        ref = run(logsnr_seq(alpha, REF_LEVELS), 2, **kw).double()
        out[name] = {(n, p): float(((final or run)(logsnr_seq(alpha, n), p, **kw).double() - ref).norm() / ref.norm())
                     for n in steps for p in orders}
    return out


def table(errors, steps=STEPS, orders=ORDERS):
    lines = ["steps  " + "  ".join(f"order {p}  " for p in orders)]
    lines += [f"{n:5d}  " + "  ".join(f"{errors[(n, p)]:9.2e}" for p in orders) for n in steps]
    return "\n".join(lines)


# ---- fp32: the kernel's bits -------------------------------------------------------------------------------------------------------------
def weight32(rho, L):
    """``inpaint_weight``'s rule per sample: fp32(rho / sqrt(L)), the quotient in double and rounded once; 0 when L = 0 or rho = 0."""
    L64 = np.asarray(L, dtype=F32).astype(np.float64)
    with np.errstate(divide="ignore"):
        w = np.where((L64 > 0) & (F32(rho) != 0), np.float64(F32(rho)) / np.sqrt(np.where(L64 > 0, L64, 1.0)), 0.0)
    return w.astype(F32)


def update32(row, flags, x, e, z, m0, m1, m2, y, m, d, L, h2_given):
    """One ``ddimxi_multistep_update`` on [B, per] fp32 arrays: row = (t, s1, s2, s3, c2, c1, k1, k2, rho, cx, w0, w1, w2) fp32,
    flags 1 = replace, 2 = guided; L [B] the sum of a sample's partials.  Returns (xt, x0, h1, h2): x0 is None when the kernel
    only reads it (guided), h2 None when the kernel does not store it.  An input that the row and the flags leave unread may hold
    anything (the tests poison it): it never enters a result."""
    _, s1, s2, s3, c2, c1, _, k2, rho, cx, w0, w1, w2 = (F32(v) for v in row)
    x, e, z, m0, m1, m2, y, m, d = (np.asarray(v, dtype=F32) for v in (x, e, z, m0, m1, m2, y, m, d))
    guided, replace = bool(flags & 2), bool(flags & 1)
    x0 = None
    if not guided:
        m0 = x0 = SM.ddim_x0(x, e, s1, s2)
    w = (weight32(rho, L) if guided else np.zeros(x.shape[0], dtype=F32))[:, None]
    fold = np.broadcast_to(w != 0, x.shape)
    mt = np.where(fold, SM.inpaint_guide(m0, m0, y, m, d, k2, w), m0)
    u = SM.ddim_next(m0, e, s3, c2)
    u = np.where(fold, SM.fma32(w0, SM.sub32(mt, m0), u), u)
    use1, use2, add_z = w1 != 0, w2 != 0 and h2_given, c1 != 0
    if use1:
        u = SM.fma32(w1, SM.sub32(mt, m1), u)
    if use2:
        u = SM.fma32(w2, SM.sub32(m1, m2), u)
    if add_z:
        u = SM.fma32(z, c1, u)
    if replace:
        kv = SM.inpaint_known(x, y, cx, w0, cx != 0)
        if add_z:
            kv = SM.fma32(z, c1, kv)
        u = SM.inpaint_replace(u, kv, m)
    return u, x0, mt, (m1 if h2_given and (use1 or use2) else None)
