"""fp64 reference of ``ddim_audio_amd.windowed_solver_steps`` (test infrastructure): the existing restatements composed, nothing
new derived -- the published multistep update of tests/sde_ref.py driven by the blended noise prediction of tests/window_ref.py.

Also the convergence experiment both test files repeat: a canvas whose windows DISAGREE (window j predicts with the exact Gaussian
noise predictor of its own variance), so the blend is no formality, measured against a fine order-2 run."""
import numpy as np

import sde_ref as S
import solver_ref as R
import window_ref as WR


def blended(fn, T, H, taper):
    """``model_fn(x, t)`` of the solver references over ``fn(window, t, j)`` of the window reference: the canvas-shaped blend."""
    return lambda x, t: WR.blend(x, t, fn, T, H, taper)


def steps(x, seq, fn, alpha, T, H, taper, order, tau=0.0, zs=None):
    """Every iteration's (xs, x0_preds) of the canvas x [..., L, F], float64."""
    return S.sde_steps(x, seq, blended(fn, T, H, taper), alpha, order, tau, zs)


# ---- the convergence experiment ------------------------------------------------------------------------------------------------------
CONV_SHAPE, CONV_T, CONV_H, CONV_W, CONV_TAPER = (1, 2, 48, 4), 16, 8, 5, "tri"
CONV_VARS = [0.25, 1.0, 2.0, 0.5, 1.5]  # window j's data variance: neighbouring windows predict different eps for one canvas row
CONV_FINE = 1000  # logsnr_seq(a, 1000): the grid of the order-2 reference run


def window_gaussians(alpha):
    """``fn(window, t, j)``: window j uses the exact noise predictor of N(0, CONV_VARS[j])."""
    models = [R.gaussian_model(alpha, v) for v in CONV_VARS]
    return lambda w, t, j: models[j](w, t)


def conv_start():
    return np.random.default_rng(48).standard_normal(CONV_SHAPE)


def conv_reference(alpha, seq_of):
    """The final canvas of the fine order-2 run; ``seq_of(n)`` = ``schedule.logsnr_seq(alpha, n)``."""
    return steps(conv_start(), seq_of(CONV_FINE), window_gaussians(alpha), alpha, CONV_T, CONV_H, CONV_TAPER, 2)[0][-1]


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def conv_conditions(err):
    """The two conditions on ``err[(order, steps)]``, each with the ratio it leaves: order 2 at 20 steps is at most a quarter of
    order 1 at 20 steps (the fp64 references give an eighth) and at most order 1 at 50 steps (they give a third)."""
    return [("order 2 @ 20 <= 1/4 order 1 @ 20", err[2, 20] / err[1, 20], 0.25), ("order 2 @ 20 <= order 1 @ 50", err[2, 20] / err[1, 50], 1.0)]
