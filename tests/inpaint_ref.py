"""CPU restatement of ``ddim_audio_amd.inpaint_steps`` (test infrastructure).

Steps 1-6 of the definition in plain torch ops over ``model_fn(x, t) -> eps`` (``oracle.ref_cpu.model_forward``), with the
guidance gradient taken the plain DPS way: ``torch.autograd.grad`` of L_b = sum (m (x0 - y))^2 w.r.t. x_t, not the k1 / k2
decomposition the kernels use.  Works in the dtype of ``x`` (fp32, or fp64 for the decomposition test)."""
import torch

from ddim_audio_amd.schedule import ddim_coefficients


def zetas(guidance, n):
    if isinstance(guidance, (int, float)):
        return [float(guidance)] * n
    return [float(v) for v in guidance]


def step(model_fn, xt, row, zeta, y, m, guided, replace, z=None):
    """One iteration: returns (x_{t-1}, x0, L_b).  ``row`` = (t, s1, s2, s3, c2, c1) of ``ddim_coefficients``."""
    ti, s1, s2, s3, c2, c1 = [float(v) for v in row]
    t = torch.full((xt.size(0),), int(ti), dtype=torch.long)
    L = None
    if guided:
        xg = xt.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            e = model_fn(xg, t)
            x0 = (xg - s1 * e) / s2
            L = (m * (x0 - y)).square().flatten(1).sum(1)
            (g,) = torch.autograd.grad(L.sum(), xg)  # samples are independent: d L_b / d x_t for every b
        e, x0, L = e.detach(), x0.detach(), L.detach()
    else:
        with torch.no_grad():
            e = model_fn(xt, t)
            x0 = (xt - s1 * e) / s2
    u = s3 * x0 + c2 * e
    if z is not None:
        u = u + c1 * z
    if guided and zeta != 0.0:
        w = torch.where(L > 0, zeta / L.clamp_min(torch.finfo(L.dtype).tiny).sqrt(), torch.zeros_like(L))
        u = u - w.view(-1, 1, 1, 1) * g
    if replace:
        k = s3 * y + c2 * e
        if z is not None:
            k = k + c1 * z
        u = m * k + (1 - m) * u
    return u, x0, L


def inpaint_steps(x, seq, model_fn, alpha, y, mask, guidance=0.0, replace=True, eta=0.0, noise_fn=None):
    """Every iteration's (xs, x0_preds), xs[0] = x.  ``noise_fn(index, xt)`` gives z when eta > 0."""
    coef = ddim_coefficients(seq, alpha, eta)
    zs = zetas(guidance, coef.shape[0])
    guided = any(v != 0.0 for v in zs)
    m = torch.broadcast_to(mask.to(x.dtype), x.shape)
    yk = torch.where(m == 0, torch.zeros((), dtype=x.dtype), torch.broadcast_to(y.to(x.dtype), x.shape))
    xt = x.clone()
    xs, x0s = [x.clone()], []
    for i, row in enumerate(coef):
        z = noise_fn(i, xt) if eta != 0.0 else None
        xt, x0, _ = step(model_fn, xt, row, zs[i], yk, m, guided, replace, z)
        xs.append(xt.clone())
        x0s.append(x0.clone())
    return xs, x0s
