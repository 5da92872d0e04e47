"""Multistep inpainting on the CPU (ddim_audio_amd.inpaint_solver_steps): the coefficient table against the two tables it is
made of and against the closed forms of its two new columns, ``guidance_per_step`` against an fp64 restatement of
``inpaint_steps``, the fp64 convergence study on a correlated Gaussian (tests/inpaint_solver_ref.py) with its two gates,
validation before any device work, and the binding of include/ddimx_inpaint_solver.h.

The study, measured (float64, audio.yml's schedule, relative L2 distance of the final sample from the mode's own order-2 run on
logsnr_seq(alpha, 734); requested steps 10 / 20 / 50 / 100, orders 1 / 2 / 3):

    replacement only        10: 1.18e-01 3.83e-02 4.72e-02   20: 5.84e-02 1.02e-02 4.44e-03
                            50: 2.33e-02 1.49e-03 4.45e-04  100: 1.16e-02 3.50e-04 9.00e-05
    guided + replacement    10: 1.15e-01 3.64e-02 4.56e-02   20: 5.72e-02 9.77e-03 4.33e-03
                            50: 2.28e-02 1.45e-03 4.36e-04  100: 1.14e-02 3.40e-04 8.91e-05
    guided only (no gate)   10: 2.39e-01 2.17e-01 1.00e-01   20: 1.37e-01 5.72e-02 1.08e-02
                            50: 6.61e-02 8.09e-03 7.22e-04  100: 4.70e-02 1.83e-03 1.47e-03
    eps-path replacement    10: 3.07e-01 2.60e-01 2.36e-01   20: 1.95e-01 1.67e-01 1.68e-01
    (inpaint_steps')        50: 9.08e-02 8.31e-02 8.37e-02  100: 4.52e-02 4.25e-02 4.26e-02

Gates (replacement only): order 1 / order 2 at 20 steps = 5.7 (>= 3), order 2 at 20 / at 50 steps = 6.8 (>= 3)."""
import os

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib
from ddim_audio_amd.schedule import (INPAINT_SOLVER_STRIDE, dpm_coefficients, guidance_per_step, inpaint_coefficients,
                                     inpaint_solver_coefficients, logsnr_seq)

import inpaint_solver_ref as R
import model_harness as MH
import solver_ref as SR


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("tau", [0.0, 1.0])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("kind", ["uniform", "logsnr", "single", "offset"])
def test_coefficient_table(kind, order, tau, prediction):
    a = MH.alphas()
    seq = SR.seqs(a)[kind]
    rho = np.linspace(0.0, 0.7, len(seq))
    c = inpaint_solver_coefficients(seq, a, order, tau, rho, prediction)
    assert c.dtype == np.float64 and c.shape == (len(seq), 13) and INPAINT_SOLVER_STRIDE == 13
    base = dpm_coefficients(seq, a, order, tau)
    known = inpaint_coefficients(seq, a, 1.0 if tau else 0.0, rho, prediction)
    assert np.array_equal(c[:, :6], base[:, :6]) and np.array_equal(c[:, 11:], base[:, 6:]), "the solver's columns, bit for bit"
    assert np.array_equal(c[:, 6:8], known[:, 6:8]), "k1, k2"
    assert np.array_equal(c[:, 8], rho)
    s1, s2, s3, c2 = (base[:, i] for i in (1, 2, 3, 4))
    assert np.array_equal(c[:, 9], c2 / s1) and np.array_equal(c[:, 10], s3 - c2 * s2 / s1)
    # the closed forms of dpm_coefficients' docstring: (sigma_n / sigma_t) e^(-tau h) and alpha_n (1 - e^(-(1 + tau) h))
    a64 = a.double().numpy()
    lam = 0.5 * np.log(a64 / (1 - a64))
    ts = list(reversed(seq))
    for k in range(len(seq) - 1):
        i, j = ts[k], ts[k + 1]
        h = lam[j] - lam[i]
        assert abs(c[k, 9] - np.sqrt((1 - a64[j]) / (1 - a64[i])) * np.exp(-tau * h)) <= 1e-12
        assert abs(c[k, 10] - np.sqrt(a64[j]) * -np.expm1(-(1 + tau) * h)) <= 1e-12 * max(1.0, np.exp(2 * tau * h))
    assert c[-1, 9] == 0.0 and c[-1, 10] == 1.0, "the final row: cx = 0, w0 = 1"
    # one float serves every row
    assert np.array_equal(inpaint_solver_coefficients(seq, a, order, tau, 0.25, prediction)[:, 8], np.full(len(seq), 0.25))


def test_table_checks_are_those_of_the_two_tables():
    a = MH.alphas()
    for kw, msg in ((dict(order=0), "order"), (dict(order=4), "order"), (dict(order=True), "order"), (dict(tau=-1.0), "tau"),
                    (dict(tau=float("nan")), "tau"), (dict(guidance=-0.1), "guidance"), (dict(guidance=[0.1, 0.2]), "guidance"),
                    (dict(guidance=float("inf")), "guidance"), (dict(prediction="x0"), "prediction"), (dict(seq=[]), "empty"),
                    (dict(seq=[5, 5]), "increasing")):
        kw = dict(kw)
        with pytest.raises(ValueError, match=msg):
            inpaint_solver_coefficients(kw.pop("seq", [0, 300, 600]), a, **kw)


# ---- 2. rho against zeta -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.0, 1.0])
def test_guidance_per_step_is_the_order_1_guidance_of_inpaint_steps(tau):
    """Order 1 of the folded form == the fp64 restatement of inpaint_steps (guidance subtracted from x_{t-1}, eta = tau) with
    zeta_i = rho w0_i, to 1e-12, on the Gaussian fixture; without replacement, where the two functions differ by design."""
    a = MH.alphas()
    fn, x, y, mask, _ = R.gaussian_case(a)
    seq = logsnr_seq(a, 20)
    rho = np.linspace(0.5, 0.1, len(seq))
    zeta = guidance_per_step(seq, a, rho, tau)
    c = inpaint_solver_coefficients(seq, a, 1, tau, rho)
    assert np.array_equal(zeta, c[:, 8] * c[:, 10]) and zeta[-1] == rho[-1]
    assert np.array_equal(guidance_per_step(seq, a, 0.25, tau), 0.25 * c[:, 10])
    zs = torch.from_numpy(np.random.default_rng(3).standard_normal((len(seq),) + tuple(x.shape)))
    kw = dict(replace=False, order=1, tau=tau, noise_fn=lambda i, xt: zs[i])
    xs, x0 = R.solver_steps(x, seq, fn, a, y, mask, guidance=rho, **kw)
    want, want0 = R.solver_steps(x, seq, fn, a, y, mask, guidance=zeta, guide="euler", **kw)
    worst = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(xs[1:] + x0, want[1:] + want0))
    print(f"[rho vs zeta, tau {tau}] worst relative difference {worst:.2e}")
    assert worst <= 1e-12
    assert float((xs[-1] - R.solver_steps(x, seq, fn, a, y, mask, guidance=0.0, **kw)[0][-1]).abs().max()) > 1e-3, "guidance acts"


# ---- 3. the convergence study ------------------------------------------------------------------------------------------------------
def test_convergence_study_on_a_correlated_gaussian():
    """The module docstring's tables, re-measured and printed; the two gates hold for replacement only.  Guided only has no gate:
    1 / sqrt(L) is not smooth where the residual nearly vanishes, and the order-2/3 rows are erratic across seeds."""
    errors = R.study(MH.alphas())
    for name, e in errors.items():
        print(f"[inpaint solver study: {name}]\n{R.table(e)}")
    e = errors["replace"]
    r_order, r_steps = e[(20, 1)] / e[(20, 2)], e[(20, 2)] / e[(50, 2)]
    print(f"[inpaint solver study] order 1 / order 2 at 20 steps = {r_order:.2f}; order 2 at 20 / at 50 steps = {r_steps:.2f}")
    assert r_order >= 3.0, f"order 2 at 20 steps is only {r_order:.2f}x closer than order 1"
    assert r_steps >= 3.0, f"the order-2 error falls only {r_steps:.2f}x from 20 to 50 steps"


# ---- 4. validation -----------------------------------------------------------------------------------------------------------------
def _call(**kw):
    # the model is never reached: validation comes before any device work (None would fail at the first forward)
    shape = (2, 2, 16, 32)
    kw.setdefault("y", torch.zeros(shape))
    kw.setdefault("mask", torch.ones(shape))
    return D.inpaint_solver_steps(kw.pop("x", torch.zeros(shape)), kw.pop("seq", [0, 300, 600]), None, MH.alphas(), None, **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(noise=D.BrownianStream(1, 0), tau=1.0), "BrownianStream"),
    (dict(corrector=True), "corrector"),
    (dict(threshold=D.X0Clip(1.0)), "threshold"),
    (dict(noise=D.NoiseStream(1, 0), noise_fn=torch.randn_like, tau=1.0), "not both"),
    (dict(order=0), "order"),
    (dict(order=4), "order"),
    (dict(order=2.5), "order"),
    (dict(tau=-0.5), "tau"),
    (dict(tau=float("inf")), "tau"),
    (dict(y=None), "needs y="),
    (dict(mask=None), "needs y="),
    (dict(y=torch.zeros(2, 2, 16, 31)), "broadcast"),
    (dict(mask=torch.full((2, 2, 16, 32), 1.5)), r"\[0, 1\]"),
    (dict(y=torch.zeros(2, 2, 16, 32, dtype=torch.int32)), "floating"),
    (dict(guidance=-1.0), "guidance"),
    (dict(guidance=[0.1, 0.2]), "guidance"),
    (dict(prediction="x0"), "prediction"),
    (dict(seq=[]), "empty"),
    (dict(seq=[0, 300, 300]), "increasing"),
    (dict(x=torch.zeros(2, 2, 16)), "B, C, T, F"),
])
def test_invalid_arguments_raise_before_device_work(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _call(**kw)


# ---- 5. the binding ----------------------------------------------------------------------------------------------------------------
def test_ninth_header_is_bound():
    assert list(_lib.INPAINT_SOLVER_EXPORTS) == ["ddimxi_residual", "ddimxi_multistep_update"]
    assert _lib.DDIMXI_STRIDE == 13 == INPAINT_SOLVER_STRIDE
    assert (_lib.DDIMXI_REPLACE, _lib.DDIMXI_GUIDED) == (_lib.DDIMX_INPAINT_REPLACE, _lib.DDIMX_INPAINT_GUIDED)
    res, args = _lib.HEADERS["ddimx_inpaint_solver.h"].funcs["ddimxi_multistep_update"]
    assert res is _lib.c_int
    assert args == [_lib.c_void_p] * 12 + [_lib.c_int, _lib.c_longlong, _lib.c_int, _lib.c_ulonglong, _lib.c_uint, _lib.c_uint, _lib.c_void_p]
    res, args = _lib.HEADERS["ddimx_inpaint_solver.h"].funcs["ddimxi_residual"]
    assert res is _lib.c_int and args == _lib.HEADERS["ddimx.h"].funcs["ddimx_inpaint_residual"][1], "ddimx_inpaint_residual's signature"
    assert not set(_lib.INPAINT_SOLVER_EXPORTS) & set(_lib.EXPORTS), "ddimx.h's list is unchanged"
    assert not [n for n in _lib.EXPORTS if n.startswith("ddimxi_")]
    from ddim_audio_amd import build
    assert "inpaint_solver.cpp" in build.SOURCES and "inpaint_solver_kernels.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "inpaint_solver_kernels.h"))
    doc = D.inpaint_solver_steps.__doc__
    assert "guidance_per_step" in doc and "erratic" in doc and "BrownianStream" in doc
