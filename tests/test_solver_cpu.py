"""DPM-Solver++ multistep sampler, host side (no GPU, no library): the coefficient table the kernel reads against
ddim_coefficients and against the paper's form of the update (tests/solver_ref.py), the log-SNR step grid, the order of
convergence against a closed-form solution, and argument validation before any device work."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import configs
from ddim_audio_amd.schedule import ddim_coefficients, dpm_coefficients, logsnr_seq, make_seq

import model_harness as MH
import solver_ref as R

VAR = 0.25  # data variance of the Gaussian model
LOGSNR_20 = [0, 1, 4, 10, 19, 35, 61, 103, 166, 253, 353, 454, 546, 629, 704, 772, 834, 893, 947, 999]


def _seqs(a):
    return dict(R.seqs(a), quad=sorted(set(make_seq(1000, 12, "quad"))))


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("kind", ["uniform", "quad", "logsnr", "single", "offset"])
def test_coefficient_table(kind, order):
    a = MH.alphas()
    seq = _seqs(a)[kind]
    c = dpm_coefficients(seq, a, order)
    assert c.dtype == np.float64 and c.shape == (len(seq), 8)
    assert np.array_equal(c[:, :6], ddim_coefficients(seq, a, 0.0)), "columns 0-5 must be ddim_coefficients bit for bit"
    assert (c[:, 5] == 0).all()
    w = c[:, 6:]
    assert np.isfinite(w).all()
    assert (w[0] == 0).all() and (w[-1] == 0).all(), "the first row and the final jump to t = -1 are first order"
    assert (w[:2, 1] == 0).all(), "no second history term before two predictions exist"
    if order == 1:
        assert (w == 0).all()
    if order <= 2:
        assert (w[:, 1] == 0).all()
    if order >= 2 and len(seq) > 2:
        assert (w[1:-1, 0] != 0).all()
    if order == 3 and len(seq) > 3:
        assert (w[2:-1, 1] != 0).all()


def test_first_order_term_is_the_ddim_update():
    """(sigma_t / sigma_s) x - alpha_t expm1(-h) m0 = s3 m0 + c2 eps for every row but the final jump (h infinite there)."""
    a = MH.alphas()
    seq = logsnr_seq(a, 20)
    c = dpm_coefficients(seq, a, 1)
    al, sg, lam = R.levels(seq, a)
    x, eps = 0.7, -1.3
    for k in range(len(seq) - 1):
        _, s1, s2, s3, c2 = c[k, :5]
        m0 = (x - s1 * eps) / s2
        paper = sg[k + 1] / sg[k] * x - al[k + 1] * np.expm1(-(lam[k + 1] - lam[k])) * m0
        assert abs(paper - (s3 * m0 + c2 * eps)) <= 1e-14 * (abs(s3 * m0) + abs(c2 * eps))


# ---- 2. w-form = D-form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("model", ["gaussian", "tanh"])
@pytest.mark.parametrize("kind", ["uniform", "logsnr", "offset"])
def test_table_trajectory_equals_paper_form(kind, model, order):
    a = MH.alphas()
    seq = _seqs(a)[kind]
    fn = R.gaussian_model(a, VAR) if model == "gaussian" else R.tanh_model(a)
    x = np.linspace(-2.0, 2.0, 9)
    want_xs, want_ms = R.dpm_solver_steps(x, seq, fn, a, order)
    xs, ms = R.table_steps(x, dpm_coefficients(seq, a, order), fn)
    worst = 0.0
    for got, want in zip(xs[1:] + ms, want_xs[1:] + want_ms):
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print(f"[w-form vs D-form {kind} {model} order {order}] worst relative difference {worst:.2e}")
    assert worst <= 1e-12


# ---- 3. the step grid --------------------------------------------------------------------------------------------------------------
def test_logsnr_seq():
    a = MH.alphas()
    assert logsnr_seq(a, 20) == LOGSNR_20
    for n in (2, 5, 10, 20, 25, 50, 200):
        s = logsnr_seq(a, n)
        assert all(type(t) is int for t in s)
        assert all(q > p for p, q in zip(s, s[1:])) and s[0] == 0 and s[-1] == 999 and len(s) <= n
    assert len(logsnr_seq(a, 50)) == 49, "the documented shortening: two targets round to the same t near t = 0"
    assert "shorter" in logsnr_seq.__doc__.lower()
    for bad in (1, 0, 2.5):
        with pytest.raises(ValueError):
            logsnr_seq(a, bad)
    assert make_seq(1000, 20) == list(range(0, 1000, 50))


# ---- 4. convergence against the closed form ----------------------------------------------------------------------------------------
def test_convergence_conditions():
    a = MH.alphas()
    e = {(n, p): R.final_error(logsnr_seq(a, n), a, p, VAR) for n in (20, 25, 50) for p in (1, 2, 3)}
    ddim_100 = R.final_error(make_seq(1000, 100), a, 1, VAR)
    for k, v in sorted(e.items()):
        print(f"[convergence fp64] log-SNR grid, {k[0]} requested steps, order {k[1]}: {v:.3e}")
    print(f"[convergence fp64] uniform grid, 100 steps, order 1: {ddim_100:.3e}")
    assert e[20, 2] <= e[20, 1] / 5
    assert e[20, 3] <= e[20, 2]
    assert 1.6 <= e[25, 1] / e[50, 1] <= 2.5
    assert e[25, 2] / e[50, 2] >= 3
    assert e[25, 3] / e[50, 3] >= 5
    assert e[20, 2] <= ddim_100


# ---- 5. validation -----------------------------------------------------------------------------------------------------------------
def _call(**kw):
    x = kw.pop("x", torch.zeros(2, 2, 16, 32))
    seq = kw.pop("seq", [0, 300, 600])
    # the model is never reached: validation comes before any device work (None would fail at the first forward)
    return D.dpm_solver_steps(x, seq, None, MH.alphas(), None, **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(order=0), "order"),
    (dict(order=4), "order"),
    (dict(order=2.5), "order"),
    (dict(seq=[]), "empty"),
    (dict(seq=[0, 300, 300]), "increasing"),
    (dict(seq=[0, 600, 300]), "increasing"),
    (dict(seq=[0, 300, 1000]), "0..999"),
    (dict(seq=[-1, 300]), "0..999"),
    (dict(seq=[0, 300.5]), "integers"),
    (dict(x=torch.zeros(2, 16, 32)), "[B, C, T, F]"),
    (dict(x=torch.zeros(1, 1, 3, 3)), "multiple of 4"),
    (dict(x=torch.zeros(2, 1, 3, 6)), "multiple of 4"),
])
def test_invalid_arguments_raise_before_device_work(kw, msg):
    with pytest.raises(ValueError) as e:
        _call(**kw)
    assert msg in str(e.value)


@pytest.mark.parametrize("bad_order", [0, 4, 2.5, True, "2"])
def test_order_is_checked_before_anything_else(bad_order):
    with pytest.raises(ValueError, match="order"):
        dpm_coefficients([], MH.alphas(), bad_order)


def test_shape_must_match_the_model():
    m = D.Model(configs.tiny_config("torch.FloatTensor"))  # F = 32, C = 2, three levels; never leaves the CPU
    for shape, msg in (((2, 2, 16, 64), "does not match the model"), ((2, 2, 10, 32), "multiple of 4 for this model")):
        with pytest.raises(ValueError) as e:
            D.dpm_solver_steps(torch.zeros(shape), [0, 300, 600], m, MH.alphas(), None)
        assert msg in str(e.value)
