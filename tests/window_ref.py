"""fp64 restatement of ``ddim_audio_amd.windowed_steps`` (test infrastructure).

Written from the definition -- loop over the windows, accumulate weight x eps and weight per canvas row, divide -- NOT from the
(jfirst, cnt, wt) tables of ``schedule.window_plan``, so the two derivations check each other.  Works on numpy float64 arrays
whose second-to-last axis is the canvas row axis ([..., L, F]) over any ``model_fn(window, t, j) -> eps``: the window's content
[..., T, F], the timestep and the window's index (a real network ignores j; the tests also use models that do not)."""
import numpy as np
import torch


def taper_weights(T, taper):
    """w(tau), tau = 0 .. T - 1, float64."""
    tau = np.arange(T, dtype=np.float64)
    if taper == "flat":
        return np.ones(T)
    if taper == "tri":
        return np.minimum(tau + 1.0, T - tau)
    raise ValueError(taper)


def n_windows(L, T, H):
    assert L >= T and (L - T) % H == 0, (L, T, H)
    return (L - T) // H + 1


def blend(x, t, model_fn, T, H, taper):
    """The blended noise prediction of the canvas x [..., L, F]: sum_j w(l - j H) eps_j(l - j H) / sum_j w(l - j H)."""
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[-2]
    w = taper_weights(T, taper)[:, None]
    num, den = np.zeros_like(x), np.zeros((L, 1))
    for j in range(n_windows(L, T, H)):
        rows = slice(j * H, j * H + T)
        e = np.asarray(model_fn(x[..., rows, :].copy(), t, j), dtype=np.float64)
        assert e.shape == x[..., rows, :].shape, (e.shape, x.shape)
        num[..., rows, :] += w * e
        den[rows] += w
    assert (den > 0).all()
    return num / den


def windowed_steps(x, seq, model_fn, alpha, T, H, taper, eta=0.0, noise_fn=None):
    """Every iteration's (xs, x0_preds), xs[0] = x: the eta-generalised DDIM update of the whole canvas on the blended eps,
    with a_t from the fp32 table in float64 and a_{-1} = 1; ``noise_fn(k, x)`` gives iteration k's canvas-shaped noise."""
    a = torch.as_tensor(alpha).to("cpu", torch.float32).numpy().astype(np.float64)
    seq = list(seq)
    x = np.asarray(x, dtype=np.float64)
    xs, x0s = [x.copy()], []
    for k, (t, t_next) in enumerate(zip(reversed(seq), reversed([-1] + seq[:-1]))):
        at, an = a[t], (a[t_next] if t_next >= 0 else 1.0)
        e = blend(x, t, model_fn, T, H, taper)
        x0 = (x - np.sqrt(1.0 - at) * e) / np.sqrt(at)
        c1 = eta * np.sqrt((1.0 - at / an) * (1.0 - an) / (1.0 - at))
        c2 = np.sqrt((1.0 - an) - c1 ** 2)
        x = np.sqrt(an) * x0 + c2 * e
        if c1 != 0.0:
            x = x + c1 * np.asarray(noise_fn(k, x), dtype=np.float64)
        x0s.append(x0)
        xs.append(x.copy())
    return xs, x0s
