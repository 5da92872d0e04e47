"""SDE-DPM-Solver++ on the host (no GPU): the ``tau`` column of ``schedule.dpm_coefficients`` against its contracts, the table's
form against the published update in float64, what the noise buys on Gaussian data (an exact covariance recursion, tied to the
restatement by 2^20 sampled chains), the pool's rows, the fourth header's binding and the argument checks in front of any device
work."""
import ctypes

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, sampler
from ddim_audio_amd.pool import request_rows
from ddim_audio_amd.schedule import ddim_coefficients, dpm_coefficients, logsnr_seq, make_seq
import model_harness as MH
import sde_ref as S
import solver_ref as R

TAUS = (0.5, 1.0, 2.0)


def _grids(a):
    return {"logsnr 20": logsnr_seq(a, 20), "uniform 10": make_seq(1000, 10)}


# ---- 1. the coefficient table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3])
def test_tau_zero_is_the_table_without_the_keyword_and_tau_one_is_ddim_eta_one(order):
    a = MH.alphas()
    for what, seq in _grids(a).items():
        plain = dpm_coefficients(seq, a, order)
        assert np.array_equal(dpm_coefficients(seq, a, order, tau=0.0), plain), what
        assert np.array_equal(dpm_coefficients(seq, a, order, tau=0), plain), what
        one = dpm_coefficients(seq, a, order, tau=1.0)
        assert np.array_equal(one[:, :6], ddim_coefficients(seq, a, 1.0)), what
        assert (one[:-1, 5] > 0).all() and one.shape == plain.shape == (len(seq), 8)
        # the history weights change with tau; the order ramp does not
        assert np.array_equal(one[:, 6:] != 0, plain[:, 6:] != 0)
        if order > 1:
            assert not np.array_equal(one[:, 6:], plain[:, 6:])


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("tau", TAUS)
def test_first_order_columns_are_the_published_coefficients(tau, order):
    a = MH.alphas()
    for what, seq in _grids(a).items():
        c = dpm_coefficients(seq, a, order, tau=tau)
        al, sg, lam = R.levels(seq, a)
        t, s1, s2, s3, c2, c1 = (c[:-1, i] for i in range(6))
        assert np.array_equal(c[:, :4], ddim_coefficients(seq, a, 0.0)[:, :4])
        h = lam[1:-1] - lam[:-2]
        an = MH.alphas().double().numpy()[list(reversed(seq))[1:]]  # the levels reached, but for the final jump's
        assert np.abs(c1 ** 2 + c2 ** 2 - (1.0 - an)).max() <= 1e-14, what
        # c2 = sqrt((1 - an) - c1^2) cancels where e^(-2 tau h) is small: the difference carries the few roundings of its two
        # terms, each 2^-53 of (1 - an), so c2 -- and the x coefficient, which is proportional to it -- is good to that many
        # units of 2^-53 (1 - an) / c2^2 (schedule.dpm_coefficients' docstring).  The log-SNR grid is held to 1e-12 as it stands;
        # the uniform grid's last step (h = 3.5) is where the cancellation shows: 4.5e-10 at tau = 2
        slack = np.full(h.shape, 1e-12) if what == "logsnr 20" else 1e-12 + 8 * 2.0 ** -53 * (1.0 - an) / c2 ** 2
        x_coef, want = c2 / s1, sg[1:-1] / sg[:-2] * np.exp(-tau * h)
        assert (np.abs(x_coef / want - 1.0) <= slack).all(), what
        assert what == "logsnr 20" or slack.max() <= (2e-9 if tau == 2.0 else 1e-11)
        data, want = s3 - c2 * s2 / s1, al[1:-1] * -np.expm1(-(1.0 + tau) * h)
        assert np.abs(data / want - 1.0).max() <= 1e-12, what
        want = sg[1:-1] * np.sqrt(-np.expm1(-2.0 * tau * h))
        assert np.abs(c1 / want - 1.0).max() <= 1e-12, what
        assert (c[-1, 4:] == 0).all(), "the final row: c1 = c2 = w1 = w2 = 0"
        assert c[-1, 3] == 1.0


def test_bad_tau_raises():
    a = MH.alphas()
    seq = logsnr_seq(a, 10)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), None, "1", True):
        with pytest.raises(ValueError, match="tau"):
            dpm_coefficients(seq, a, 2, tau=bad)
    # a tau at which some step keeps less than one ulp of the sample is refused, whatever sign the cancelled difference takes;
    # the largest h of this grid decides where that begins
    lam = R.levels(seq, a)[2]
    h_max = float(np.max(lam[1:-1] - lam[:-2]))
    edge = 52 * np.log(2.0) / (2.0 * h_max)
    for bad in (1.01 * edge, 2 * edge, 1e3, 1e6, 1e300):
        with pytest.raises(ValueError, match="c2"):
            dpm_coefficients(seq, a, 2, tau=bad)
    ok = dpm_coefficients(seq, a, 2, tau=0.99 * edge)
    assert np.isfinite(ok).all() and (ok[:-1, 4] > 0).all()
    with pytest.raises(ValueError, match="order"):
        dpm_coefficients(seq, a, 4, tau=1.0)
    with pytest.raises(ValueError, match="seq"):
        dpm_coefficients([5, 5], a, 2, tau=1.0)


# ---- 2. the table's form == the published form -------------------------------------------------------------------------------------------
def _wiggly(a, var):
    """A model that is not linear in x, so the history terms do not cancel by accident."""
    g = R.gaussian_model(a, var)
    return lambda x, t: g(x, t) + 0.1 * np.sin(3.0 * x + t)


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("tau", (0.0,) + TAUS)
def test_table_form_equals_the_published_update(tau, order):
    a = MH.alphas()
    seq = logsnr_seq(a, 20)
    assert len(seq) == 20
    rng = np.random.default_rng(5)
    x = rng.standard_normal(64)
    z = rng.standard_normal((20, 64))
    zs = lambda k, shape: z[k]  # noqa: E731
    model = _wiggly(a, 0.25)
    coef = dpm_coefficients(seq, a, order, tau=tau)
    got_x, got_m = R.table_steps(x, coef, model, zs)
    want_x, want_m = S.sde_steps(x, seq, model, a, order, tau, zs)
    assert len(got_x) == 21
    for k in range(20):
        for got, want in ((got_x[k + 1], want_x[k + 1]), (got_m[k], want_m[k])):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (k, tau, order)
    if tau == 0.0:  # and both are the deterministic solver
        ode_x, _ = R.dpm_solver_steps(x, seq, model, a, order)
        assert np.abs(got_x[-1] - ode_x[-1]).max() <= 1e-12 * np.abs(ode_x[-1]).max()
    else:
        assert not np.allclose(got_x[-2], R.table_steps(x, coef, model, lambda k, shape: -z[k])[0][-2]), "the noise matters"


# ---- 3. Gaussian data --------------------------------------------------------------------------------------------------------------------
def _err(a, n, order, tau, var):
    return S.variance_error(dpm_coefficients(logsnr_seq(a, n), a, order, tau=tau), a, var)


def test_covariance_recursion_gives_the_documented_table():
    """Relative error of the final sample's variance, var = 0.25, audio schedule, ``logsnr_seq(alpha, n)``: the figures of
    INTEGRATION.md section O, to the digits shown there."""
    a = MH.alphas()
    table = {(10, 1.0): ("0.589", "0.042", "1.06"), (20, 0.5): ("0.307", "0.050", "0.044"), (20, 1.0): ("0.372", "0.070", "0.086"),
             (50, 0.5): ("0.136", "0.0084", "0.0051"), (50, 1.0): ("0.174", "0.0129", "0.0109")}
    used = {10: 10, 20: 20, 50: 49}
    for (n, tau), want in table.items():
        assert len(logsnr_seq(a, n)) == used[n]
        for order, w in zip((1, 2, 3), want):
            got = _err(a, n, order, tau, 0.25)
            digits = len(w.split(".")[1]) if not w.startswith("1.") else 2
            assert f"{got:.{digits}f}" == w, (n, tau, order, got)
    # order 3 at tau = 1 and 20 steps is where the data's variance matters most
    assert f"{_err(a, 20, 3, 1.0, 4.0):.3f}" == "0.096"
    # order 1 at tau = 1 is DDIM at eta = 1
    c6 = np.concatenate([ddim_coefficients(logsnr_seq(a, 20), a, 1.0), np.zeros((20, 2))], axis=1)
    assert S.variance_error(c6, a, 0.25) == _err(a, 20, 1, 1.0, 0.25)


@pytest.mark.parametrize("var", [0.25, 1.0, 4.0])
@pytest.mark.parametrize("n", [20, 50])
def test_second_order_with_noise_beats_first_order_with_noise(n, var):
    a = MH.alphas()
    e1, e2 = _err(a, n, 1, 1.0, var), _err(a, n, 2, 1.0, var)
    print(f"[variance error n={n} var={var}] order 1 {e1:.4f}, order 2 {e2:.4f}, ratio {e2 / e1:.3f}")
    assert e2 < e1 / 3


@pytest.mark.parametrize("order, tau, n", [(2, 1.0, 20), (3, 0.5, 20), (1, 1.0, 10)])
def test_sampled_chains_have_the_recursions_variance(order, tau, n):
    """2^20 independent scalar chains through the float64 restatement, numpy normals: the empirical variance of the final sample is
    within 4 standard errors, var sqrt(2 / N), of the recursion's."""
    a, var, N = MH.alphas(), 0.25, 1 << 20
    seq = logsnr_seq(a, n)
    coef = dpm_coefficients(seq, a, order, tau=tau)
    rng = np.random.default_rng(1234 + order)
    a_start = float(a[seq[-1]])
    x = rng.standard_normal(N) * np.sqrt(a_start * var + 1.0 - a_start)
    xs, _ = R.table_steps(x, coef, R.gaussian_model(a, var), lambda k, shape: rng.standard_normal(shape))
    got, want = float(np.mean(xs[-1] ** 2)), S.gaussian_cov(coef, a, var)
    se = var * np.sqrt(2.0 / N)
    print(f"[chains order {order} tau {tau} n {n}] empirical {got:.6f}, recursion {want:.6f}: {abs(got - want) / se:.2f} standard errors")
    assert abs(got - want) <= 4 * se
    assert abs(want - var) > 8 * se, "the recursion's own deviation from var is resolved at this N"


# ---- 4. the pool's rows and the argument checks ------------------------------------------------------------------------------------------
def test_request_rows_with_tau():
    a = MH.alphas()
    seq = logsnr_seq(a, 12)
    rows = request_rows(seq, a, order=2, tau=1)
    assert rows.dtype == np.float32 and np.array_equal(rows, dpm_coefficients(seq, a, 2, tau=1.0).astype(np.float32))
    rows = request_rows(seq, a, 0.0, 3, tau=0.5)
    assert np.array_equal(rows, dpm_coefficients(seq, a, 3, tau=0.5).astype(np.float32))
    # order 1: at tau = 1 the rows of eta = 1, bit for bit
    assert np.array_equal(request_rows(seq, a, order=1, tau=1.0), request_rows(seq, a, 1.0, 1))
    assert np.array_equal(request_rows(seq, a, 0.5, 1, tau=0.0), request_rows(seq, a, 0.5, 1))
    with pytest.raises(ValueError, match="eta must be 0"):
        request_rows(seq, a, 0.5, 2, tau=1.0)
    with pytest.raises(ValueError, match="eta must be 0"):
        request_rows(seq, a, 0.5, 1, tau=1.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            request_rows(seq, a, 0.0, 2, tau=bad)


def test_argument_errors_raise_before_the_library_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "stream", no_library)
    monkeypatch.setattr(sampler.DDIMStepper, "__init__", lambda *a, **k: pytest.fail("a stepper was built"))
    a = MH.alphas()
    model = lambda x, t: x  # noqa: E731  (never called)
    seq = list(range(0, 1000, 200))
    ns = D.NoiseStream(3)
    # the pool
    pool = D.SamplerPool(model, a, slots=4, t_size=32, max_steps=10)
    x = torch.zeros(2, 2, 32, 8)
    with pytest.raises(ValueError, match="eta must be 0"):
        pool.submit(x, seq, eta=0.5, order=2, noise=ns)
    with pytest.raises(ValueError, match="eta must be 0"):
        pool.submit(x, seq, eta=0.5, order=2, noise=ns, tau=1.0)
    with pytest.raises(ValueError, match="eta must be 0"):
        pool.submit(x, seq, eta=0.5, order=1, noise=ns, tau=1.0)
    for order in (1, 2, 3):
        with pytest.raises(ValueError, match="NoiseStream") as with_tau:
            pool.submit(x, seq, order=order, tau=1.0)
    with pytest.raises(ValueError, match="NoiseStream") as with_eta:
        pool.submit(x, seq, eta=1.0)
    assert str(with_tau.value) == str(with_eta.value)
    with pytest.raises(TypeError, match="NoiseStream"):
        pool.submit(x, seq, order=2, tau=1.0, noise=torch.Generator())
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            pool.submit(x, seq, order=2, tau=bad, noise=ns)
    with pytest.raises(ValueError, match="2\\^32"):
        pool.submit(x, seq, order=2, tau=1.0, noise=D.NoiseStream(3, first_sample=2 ** 32 - 1))
    assert pool.stats == {"steps": 0, "busy": 0, "idle": 0, "captures": 0} and not pool.table.queue
    # the solver
    x = torch.zeros(2, 2, 16, 32)
    with pytest.raises(ValueError, match="not both"):
        D.dpm_solver_steps(x, seq, model, a, None, order=2, tau=1.0, noise=ns, noise_fn=torch.randn_like)
    with pytest.raises(ValueError, match="not both"):
        D.dpm_solver_steps(x, seq, model, a, None, order=2, noise=ns, noise_fn=torch.randn_like)
    with pytest.raises(TypeError, match="NoiseStream"):
        D.dpm_solver_steps(x, seq, model, a, None, order=2, tau=1.0, noise=torch.Generator())
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            D.dpm_solver_steps(x, seq, model, a, None, order=2, tau=bad, noise=ns)
        with pytest.raises(ValueError, match="tau"):
            D.dpm_solver_steps(x, seq, model, a, None, order=2, tau=bad)


def test_fourth_header_is_bound_and_the_other_lists_are_unchanged():
    assert _lib.SDE_EXPORTS == ("ddimxs_multistep_update",)
    assert len(_lib.EXPORTS) == 151 and all(n.startswith("ddimx_") for n in _lib.EXPORTS)
    assert _lib.THRESHOLD_EXPORTS == ("ddimxq_quantile_work_bytes", "ddimxq_x0_quantile", "ddimxq_threshold_eps")
    assert _lib.DISTILL_EXPORTS == ("ddimxd_sqerr_loss_w", "ddimxd_sqerr_loss_w_bwd_mean", "ddimxd_distill_half", "ddimxd_distill_target")
    lib = _lib.load()
    P, I, L, UL, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_uint
    fn = lib.ddimxs_multistep_update  # resolves in the built library
    assert fn.restype is I and list(fn.argtypes) == [P, P, P, P, P, P, P, I, L, UL, U, U, P]
    # a refusal needs no device: every argument is checked before the launch
    p = ctypes.c_void_p(256)  # never dereferenced
    bad = [((None, p, None, p, None, p, p, 1, 4, 0, 0, 0, None), "null"), ((p, None, None, p, None, p, p, 1, 4, 0, 0, 0, None), "null"),
           ((p, p, None, None, None, p, p, 1, 4, 0, 0, 0, None), "null"), ((p, p, None, p, None, None, p, 1, 4, 0, 0, 0, None), "null"),
           ((p, p, None, p, None, p, None, 1, 4, 0, 0, 0, None), "null"),
           ((p, p, None, p, None, p, p, 0, 4, 0, 0, 0, None), "B = 0"), ((p, p, None, p, None, p, p, 65536, 4, 0, 0, 0, None), "B = 65536"),
           ((p, p, None, p, None, p, p, 1, 0, 0, 0, 0, None), "multiple of 4"), ((p, p, None, p, None, p, p, 1, 6, 0, 0, 0, None), "multiple of 4"),
           ((p, p, None, p, None, p, p, 1, -4, 0, 0, 0, None), "multiple of 4"),
           ((p, p, None, p, None, p, p, 1, 4 * (2 ** 32 + 1), 0, 0, 0, None), "groups of four"),
           ((p, p, None, p, None, p, p, 2, 4, 0, 2 ** 32 - 1, 0, None), "2^32")]
    for args, msg in bad:
        assert fn(*args) != 0, msg
        err = lib.ddimx_last_error().decode()
        assert "ddimxs_multistep_update" in err and msg in err, (msg, err)
