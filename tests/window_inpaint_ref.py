"""CPU restatement of ``ddim_audio_amd.windowed_inpaint_steps`` (test infrastructure).

Steps 1-6 of the definition in plain torch ops over ``model_fn(window, t, j) -> the network's output`` (a real network ignores the
window's index j).  The blend is written from the definition as in tests/window_ref.py -- loop over the windows, accumulate
weight x eps and weight per canvas row, divide -- NOT from the (jfirst, cnt, wt) tables of ``schedule.window_plan``; the guidance
gradient is taken the plain DPS way, ``torch.autograd.grad`` of L_n = sum (m (x0 - y))^2 per canvas sample w.r.t. the canvas, through
gather -> per-window model -> (v to eps with the window's own input) -> blend -> loss, NOT by the k1 / k2 + weighted-seed +
overlap-add decomposition the kernels use.  Works in the dtype of ``x`` (fp32, or fp64 for the decomposition test)."""
import torch

from ddim_audio_amd.schedule import ddim_coefficients


def zetas(guidance, n):
    if isinstance(guidance, (int, float)):
        return [float(guidance)] * n
    return [float(v) for v in guidance]


def taper_weights(T, taper, dtype):
    """w(tau), tau = 0 .. T - 1."""
    tau = torch.arange(T, dtype=dtype)
    if taper == "flat":
        return torch.ones(T, dtype=dtype)
    if taper == "tri":
        return torch.minimum(tau + 1.0, T - tau)
    raise ValueError(taper)


def n_windows(L, T, H):
    assert L >= T and (L - T) % H == 0, (L, T, H)
    return (L - T) // H + 1


def blend(x, t, model_fn, T, H, taper, v_rows=None):
    """The blended noise prediction of the canvas x [N, C, L, F]: sum_j w(l - j H) eps_j(l - j H) / sum_j w(l - j H).  ``v_rows`` =
    (s1, s2): the network predicts v, and eps_j = s1 window_j + s2 v_j with the window's own input."""
    L = x.shape[-2]
    w = taper_weights(T, taper, x.dtype)[:, None]
    num, den = torch.zeros_like(x), torch.zeros((L, 1), dtype=x.dtype)
    tt = torch.full((x.size(0),), int(t), dtype=torch.long)
    for j in range(n_windows(L, T, H)):
        win = x[..., j * H:j * H + T, :]
        e = model_fn(win, tt, j)
        assert e.shape == win.shape, (e.shape, win.shape)
        if v_rows is not None:
            e = v_rows[0] * win + v_rows[1] * e
        pad = torch.zeros_like(x)
        pad[..., j * H:j * H + T, :] = w * e
        num = num + pad
        den[j * H:j * H + T] += w
    assert bool((den > 0).all())
    return num / den


def step(model_fn, xt, row, zeta, y, m, T, H, taper, guided, replace, z=None, prediction="eps"):
    """One iteration: returns (x_{t-1}, x0, L_n, g) -- g the autograd gradient of L_n w.r.t. the canvas (None when not guided).
    ``row`` = (t, s1, s2, s3, c2, c1) of ``ddim_coefficients``."""
    ti, s1, s2, s3, c2, c1 = [float(v) for v in row]
    v_rows = (s1, s2) if prediction == "v" else None
    L = g = None
    if guided:
        xg = xt.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            e = blend(xg, ti, model_fn, T, H, taper, v_rows)
            x0 = (xg - s1 * e) / s2
            L = (m * (x0 - y)).square().flatten(1).sum(1)
            (g,) = torch.autograd.grad(L.sum(), xg)  # canvas samples are independent: d L_n / d x_t for every n
        e, x0, L = e.detach(), x0.detach(), L.detach()
    else:
        with torch.no_grad():
            e = blend(xt, ti, model_fn, T, H, taper, v_rows)
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
    return u, x0, L, g


def windowed_inpaint_steps(x, seq, model_fn, alpha, T, H, taper, y, mask, guidance=0.0, replace=True, eta=0.0, noise_fn=None,
                           prediction="eps"):
    """Every iteration's (xs, x0_preds), xs[0] = x.  ``noise_fn(index, xt)`` gives the canvas-shaped z when eta > 0."""
    coef = ddim_coefficients(seq, alpha, eta)
    zs = zetas(guidance, coef.shape[0])
    guided = any(v != 0.0 for v in zs)
    m = torch.broadcast_to(mask.to(x.dtype), x.shape)
    yk = torch.where(m == 0, torch.zeros((), dtype=x.dtype), torch.broadcast_to(y.to(x.dtype), x.shape))
    xt = x.clone()
    xs, x0s = [x.clone()], []
    for i, row in enumerate(coef):
        z = noise_fn(i, xt) if eta != 0.0 else None
        xt, x0, _, _ = step(model_fn, xt, row, zs[i], yk, m, T, H, taper, guided, replace, z, prediction)
        xs.append(xt.clone())
        x0s.append(x0.clone())
    return xs, x0s
