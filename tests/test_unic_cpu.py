"""The UniC corrector of DPM-Solver++, host side (no GPU, no library): the 9-column table against dpm_coefficients, the folded
update against the two-pass paper form (tests/unic_ref.py), the order of convergence against a closed-form solution, argument
validation before any device work, and the binding of include/ddimx_unic.h."""
import os

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, configs
from ddim_audio_amd.pool import request_rows
from ddim_audio_amd.schedule import UNIC_STRIDE, dpm_coefficients, logsnr_seq, unic_coefficients

import model_harness as MH
import solver_ref as R
import unic_ref as U

VAR = 0.25  # data variance of the Gaussian model


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("kind", ["uniform", "logsnr", "single", "offset"])
def test_coefficient_table(kind, order):
    a = MH.alphas()
    seq = R.seqs(a)[kind]
    n = len(seq)
    c, u = dpm_coefficients(seq, a, order), unic_coefficients(seq, a, order)
    assert u.dtype == np.float64 and u.shape == (n, 9) and UNIC_STRIDE == 9
    assert np.array_equal(u[:, :6], c[:, :6]), "columns 0-5 must be dpm_coefficients bit for bit"
    assert np.isfinite(u).all()
    for row in (0, n - 1):
        assert np.array_equal(u[row, :8], c[row]) and u[row, 8] == 0, "row 0 and the final jump are dpm_coefficients' rows, w3 = 0"
    if order <= 2:
        assert (u[:, 8] == 0).all()
    if order == 1:
        assert (u[:, 7] == 0).all()
    # the corrector exists from iteration 1 on, reaches one prediction further back per iteration, and never touches the final jump
    assert (u[1:n - 1, 6] != c[1:n - 1, 6]).all()
    assert (u[:, 7] != 0).sum() == (max(n - 3, 0) if order >= 2 else 0)
    assert (u[:, 8] != 0).sum() == (max(n - 4, 0) if order == 3 else 0)
    if order >= 2:
        assert (u[2:n - 1, 7] != 0).all()
    if order == 3:
        assert (u[3:n - 1, 8] != 0).all()


def test_nonzero_pattern_on_the_20_step_grid():
    a = MH.alphas()
    seq = logsnr_seq(a, 20)
    assert len(seq) == 20
    for order, want in ((1, (18, 0, 0)), (2, (18, 17, 0)), (3, (18, 17, 16))):
        u = unic_coefficients(seq, a, order)
        assert tuple(int((u[:, col] != 0).sum()) for col in (6, 7, 8)) == want, order


# ---- 2. fold = paper form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("model", ["gaussian", "tanh"])
@pytest.mark.parametrize("kind", ["uniform", "logsnr", "offset"])
def test_folded_table_equals_the_two_pass_paper_form(kind, model, order):
    a = MH.alphas()
    seq = R.seqs(a)[kind]
    fn = R.gaussian_model(a, VAR) if model == "gaussian" else R.tanh_model(a)
    x = np.linspace(-2.0, 2.0, 9)
    want_xs, want_ms = U.unic_steps(x, seq, fn, a, order)
    xs, ms = R.table_steps(x, unic_coefficients(seq, a, order), fn)
    plain_xs, _ = R.dpm_solver_steps(x, seq, fn, a, order)
    worst = 0.0
    for got, want in zip(xs[1:] + ms, want_xs[1:] + want_ms):
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print(f"[fold vs two-pass {kind} {model} order {order}] worst relative difference {worst:.2e}")
    assert worst <= 1e-12
    assert np.abs(want_xs[-1] - plain_xs[-1]).max() > 1e-6, "the corrector changes the run"


# ---- 3. convergence against the closed form ----------------------------------------------------------------------------------------
def test_convergence_conditions():
    """One order more: on log-SNR grids the error of every order drops, and the ratio from 25 to 50 steps goes from about
    2 / 4 / 6.5 to 4.4 / 10.6 / 19.3.  On the coarse grids of 8 and 10 steps the corrector does NOT help order 2 (printed, and
    asserted so the documents stay true)."""
    a = MH.alphas()
    steps = (8, 10, 20, 25, 50)
    e = {(n, p): R.final_error(logsnr_seq(a, n), a, p, VAR) for n in steps for p in (1, 2, 3)}
    ec = {(n, p): U.final_error(logsnr_seq(a, n), a, p, VAR) for n in steps for p in (1, 2, 3)}
    for k in sorted(e):
        print(f"[unic convergence fp64] log-SNR grid, {k[0]} requested steps, order {k[1]}: {e[k]:.4e} -> {ec[k]:.4e} "
              f"({e[k] / ec[k]:.2f} x)")
    for p in (1, 2, 3):
        print(f"[unic convergence fp64] order {p}: error ratio 25 -> 50 steps {e[25, p] / e[50, p]:.2f} -> {ec[25, p] / ec[50, p]:.2f}")
    assert ec[20, 1] <= e[20, 1] / 4
    assert ec[20, 2] <= e[20, 2] / 1.3
    assert ec[20, 3] <= e[20, 3] / 2
    assert ec[50, 2] <= e[50, 2] / 4
    assert ec[50, 3] <= e[50, 3] / 8
    for p, least in ((1, 3.5), (2, 8.0), (3, 14.0)):
        assert ec[25, p] / ec[50, p] >= least, p
    assert ec[20, 3] <= e[25, 3], "order 3 with the corrector at 20 steps beats order 3 without it at 25"
    assert ec[8, 2] > e[8, 2] and ec[10, 2] > e[10, 2], "the documented finding: no gain for order 2 on very coarse grids"


# ---- 4. validation -----------------------------------------------------------------------------------------------------------------
def _solver(**kw):
    # the model is never reached: validation comes before any device work (None would fail at the first forward)
    return D.dpm_solver_steps(kw.pop("x", torch.zeros(2, 2, 16, 32)), kw.pop("seq", [0, 300, 600]), None, MH.alphas(), None, **kw)


def _window(**kw):
    return D.windowed_solver_steps(kw.pop("x", torch.zeros(1, 2, 48, 32)), kw.pop("seq", [0, 300, 600]), None, MH.alphas(), None,
                                   window=32, hop=16, **kw)


@pytest.mark.parametrize("call", [_solver, _window], ids=["solver", "window"])
@pytest.mark.parametrize("kw,msg", [
    (dict(tau=1.0), "tau"),
    (dict(tau=0.5, noise=D.NoiseStream(1, 0)), "tau"),
    (dict(corrector=1), "corrector"),
    (dict(corrector="yes"), "corrector"),
    (dict(order=0), "order"),
    (dict(order=4), "order"),
    (dict(order=2.5), "order"),
    (dict(seq=[]), "empty"),
    (dict(seq=[0, 300, 300]), "increasing"),
    (dict(seq=[0, 300, 1000]), "0..999"),
    (dict(seq=[0, 300.5]), "integers"),
])
def test_invalid_arguments_raise_before_device_work(call, kw, msg):
    kw = dict(kw)
    kw.setdefault("corrector", True)
    with pytest.raises(ValueError) as e:
        call(**kw)
    assert msg in str(e.value)


def test_order_3_is_refused_in_the_window_and_in_the_pool():
    a = MH.alphas()
    with pytest.raises(ValueError, match="order 1 or 2"):
        _window(order=3, corrector=True)
    with pytest.raises(ValueError, match="order 1 or 2"):
        request_rows([0, 300, 600, 900], a, order=3, corrector=True)
    m = D.Model(configs.tiny_config("torch.FloatTensor"))  # never leaves the CPU
    pool = D.SamplerPool(m, a, slots=2, t_size=16, max_steps=8)
    x = torch.zeros(1, 2, 16, 32)
    for kw, msg in ((dict(order=3), "order 1 or 2"), (dict(order=2, tau=1.0, noise=D.NoiseStream(1, 0)), "tau"),
                    (dict(order=1, eta=0.5, noise=D.NoiseStream(1, 0)), "eta"), (dict(order=4), "order"), (dict(order=2, corrector=2), "corrector")):
        with pytest.raises(ValueError, match=msg):
            pool.submit(x, kw.pop("seq", [0, 300, 600, 900]), **dict(dict(corrector=True), **kw))
    with pytest.raises(ValueError, match="increasing"):
        pool.submit(x, [0, 300, 300], order=2, corrector=True)
    assert pool._stepper is None and not pool.table.queue, "nothing was queued, nothing touched the device"
    pool.close()


def test_checks_are_dpm_coefficients_own_in_its_order():
    a = MH.alphas()
    for bad_order in (0, 4, 2.5, True, "2"):
        with pytest.raises(ValueError, match="order"):
            unic_coefficients([], a, bad_order)  # the order before the empty seq
    for seq, msg in (([], "empty"), ([0, 2.5], "integers"), ([0, 1000], "0..999"), ([5, 5], "increasing")):
        with pytest.raises(ValueError, match=msg):
            unic_coefficients(seq, a, 2)


def test_pool_rows_are_the_first_eight_columns():
    a = MH.alphas()
    seq = logsnr_seq(a, 10)
    for order in (1, 2):
        u = unic_coefficients(seq, a, order)
        rows = request_rows(seq, a, order=order, corrector=True)
        assert rows.dtype == np.float32 and np.array_equal(rows, u[:, :8].astype(np.float32)) and (u[:, 8] == 0).all()
        assert not np.array_equal(rows, request_rows(seq, a, order=order))
        assert np.array_equal(request_rows(seq, a, order=order, corrector=False), request_rows(seq, a, order=order))


# ---- 5. the binding ----------------------------------------------------------------------------------------------------------------
def test_eighth_header_is_bound():
    assert list(_lib.UNIC_EXPORTS) == ["ddimxu_multistep_update"]
    assert _lib.DDIMXU_STRIDE == 9 == UNIC_STRIDE
    res, args = _lib.HEADERS["ddimx_unic.h"].funcs["ddimxu_multistep_update"]
    assert res is _lib.c_int and args == [_lib.c_void_p] * 7 + [_lib.c_longlong, _lib.c_void_p]
    assert not set(_lib.UNIC_EXPORTS) & set(_lib.EXPORTS), "ddimx.h's list is unchanged"
    from ddim_audio_amd import build
    assert "unic.cpp" in build.SOURCES and "unic_kernels.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "unic_kernels.h"))
    for doc in (D.dpm_solver_steps.__doc__,):
        assert "predictor" in doc.lower() and "never materialised" in doc and "last x0 prediction" in doc
