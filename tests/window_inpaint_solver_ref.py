"""fp64 reference of ``ddim_audio_amd.windowed_inpaint_solver_steps`` (test infrastructure): the existing restatements composed,
nothing new derived -- ``inpaint_solver_ref.solver_steps`` (steps 1-6 of the multistep inpainting definition, the guidance gradient
by autograd, L per sample of what it is handed: the CANVAS sample) driven by ``window_inpaint_ref.blend`` (the blend from its
definition, differentiable; a v network's output converted per window with the window's own input).

Also the convergence experiment both test files repeat: ``window_solver_ref``'s canvas whose windows DISAGREE, with a predictor per
window whose rows are CORRELATED -- an uncorrelated one would make the guidance gradient vanish off the known rows -- and a mask that
spans several windows."""
import numpy as np
import torch

import inpaint_solver_ref as R
import window_inpaint_ref as WI
import window_solver_ref as WS


def blended(fn, T, H, taper, alpha=None, prediction="eps"):
    """``model_fn(x, t) -> eps`` of ``solver_steps`` over ``fn(window, t, j)`` of the window references: the canvas-shaped blend.
    ``prediction="v"``: ``fn`` gives v and every window is converted with the row (s1, s2) of t before the blend."""
    a = None if alpha is None else torch.as_tensor(alpha).to("cpu", torch.float32).double()

    def model_fn(x, t):
        ti = int(t[0])
        v_rows = (float((1.0 - a[ti]).sqrt()), float(a[ti].sqrt())) if prediction == "v" else None
        return WI.blend(x, ti, fn, T, H, taper, v_rows)

    return model_fn


def steps(x, seq, fn, alpha, T, H, taper, y, mask, guidance=0.0, replace=True, order=2, tau=0.0, noise_fn=None, prediction="eps"):
    """Every iteration's (xs, x0_preds) of the canvas x [N, C, L, F], in x's dtype."""
    return R.solver_steps(x, seq, blended(fn, T, H, taper, alpha, prediction), alpha, y, mask, guidance=guidance, replace=replace,
                          order=order, tau=tau, noise_fn=noise_fn)


# ---- the convergence experiment ------------------------------------------------------------------------------------------------------
CONV_MASKED = (12, 28)  # canvas rows 12..27 are unknown: they lie in windows 0-3 of the five
CONV_REF_LEVELS = 734  # logsnr_seq(a, 734): the grid of the order-2 reference run
CONV_MODES = {"replace": dict(guidance=0.0, replace=True), "guided+replace": dict(guidance=0.3, replace=True)}


def conv_matrices(alpha):
    """M [W, n_table, T, T] float64: window j's exact eps predictor of a Gaussian over its T rows with covariance
    S_j = CONV_VARS[j] (exp(-|a - b| / 4) + 0.05 I), M_j[t] = sqrt(1 - a_t) (a_t S_j + (1 - a_t) I)^-1, applied along the row axis."""
    a = torch.as_tensor(alpha).to("cpu", torch.float32).numpy().astype(np.float64)
    T = WS.CONV_T
    r = np.arange(T)
    base = np.exp(-np.abs(r[:, None] - r[None, :]) / 4.0) + 0.05 * np.eye(T)
    return np.stack([np.stack([np.sqrt(1.0 - at) * np.linalg.inv(at * (v * base) + (1.0 - at) * np.eye(T)) for at in a])
                     for v in WS.CONV_VARS])


def conv_model(alpha):
    """``fn(window [..., T, F], t, j)`` in torch, differentiable, in the window's dtype."""
    M = torch.from_numpy(conv_matrices(alpha))
    return lambda w, t, j: torch.einsum("ab,...bf->...af", M[j, int(torch.as_tensor(t).reshape(-1)[0])].to(w.dtype), w)


def conv_case():
    """(x, y, mask) float64: the start, the known content and the mask, 1 except canvas rows 12..27."""
    rng = np.random.default_rng(48)
    x = rng.standard_normal(WS.CONV_SHAPE)
    y = 0.8 * rng.standard_normal(WS.CONV_SHAPE)
    mask = torch.ones(1, 1, WS.CONV_SHAPE[2], 1, dtype=torch.float64)
    mask[:, :, CONV_MASKED[0]:CONV_MASKED[1]] = 0.0
    return torch.from_numpy(x), torch.from_numpy(y), mask


def conv_final(alpha, seq, order, fn=None, **mode):
    x, y, mask = conv_case()
    return steps(x, seq, fn or conv_model(alpha), alpha, WS.CONV_T, WS.CONV_H, WS.CONV_TAPER, y, mask, order=order, **mode)[0][-1]


def conv_study(alpha, seq_of, modes=CONV_MODES, counts=(20, 50), orders=(1, 2, 3), final=None):
    """{mode: {(order, steps): error}}: the relative L2 distance of the final canvas from the mode's own fp64 order-2 run on
    ``seq_of(CONV_REF_LEVELS)``.  ``final(seq, order, **mode)`` (default: the fp64 reference itself) returns a run's final canvas."""
    fn = conv_model(alpha)
    out = {}
    for name, kw in modes.items():
        ref = conv_final(alpha, seq_of(CONV_REF_LEVELS), 2, fn, **kw).numpy()
        run = final or (lambda seq, order, **k: conv_final(alpha, seq, order, fn, **k))
        out[name] = {(p, n): WS.rel_l2(torch.as_tensor(run(seq_of(n), p, **kw)).double().numpy().reshape(ref.shape), ref)
                     for n in counts for p in orders}
    return out


def conv_table(err, counts=(20, 50), orders=(1, 2, 3)):
    lines = ["steps  " + "  ".join(f"order {p}  " for p in orders)]
    lines += [f"{n:5d}  " + "  ".join(f"{err[(p, n)]:9.2e}" for p in orders) for n in counts]
    return "\n".join(lines)
