"""CPU tests of the log-likelihood feature (ddim_audio_amd/likelihood.py): the float64 reference's convergence on the closed-form
Gaussian, the probe estimator, ``schedule.likelihood_coefficients`` against a direct restatement, the argument checks and the
binding of include/features/lkx_likelihood.h."""
import math
import shutil
import subprocess
from ctypes import c_int, c_longlong, c_uint, c_ulonglong, c_void_p

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, schedule
from ddim_audio_amd.noise import BrownianStream, NoiseStream
import likelihood_ref as R

ALPHAS = R.linear_alphas()
LKX = ("lkx_partials_doubles", "lkx_probe_fill", "lkx_stage", "lkx_finish", "lkx_sumsq")


# ---- 1. the integrator's order -------------------------------------------------------------------------------------------------------
def _errors(order, dim=64, seed=0):
    """Signed error of logp against the closed form, in bits/dim, at n = 20, 50, 100, 200 levels."""
    x = np.random.default_rng(seed).standard_normal((1, dim)) * math.sqrt(float(ALPHAS[0]) * 0.25 + 1.0 - float(ALPHAS[0]))
    exact = R.iso_logp(x, ALPHAS, 0)
    out = {}
    for n in (20, 50, 100, 200):
        logp, _, n_eval = R.integrate(x, R.grid(n), ALPHAS, order, R.iso_eps_div(ALPHAS))
        assert n_eval == order * n  # grid(n) has n + 1 levels
        out[n] = float((logp - exact)[0]) / (dim * math.log(2.0))
    return out


def test_heun_is_second_order_and_euler_first_on_the_gaussian():
    """The isotropic Gaussian's probe estimate is exact, so the error is the integrator's alone.  Measured here (float64, D = 64,
    seed 0), bits/dim:  Euler 1.48, 0.557, 0.274, 0.136;  Heun 0.164, 0.0262, 0.00653, 0.00163  at n = 20, 50, 100, 200."""
    euler, heun = _errors(1), _errors(2)
    for n in (20, 50, 100, 200):
        print(f"[likelihood order] n = {n}: Euler {euler[n]:.4g}, Heun {heun[n]:.4g} bits/dim")
    print(f"[likelihood order] ratio 100 -> 200: Euler {euler[100] / euler[200]:.3f}, Heun {heun[100] / heun[200]:.3f}")
    assert 3.5 <= heun[100] / heun[200] <= 4.5
    assert 1.8 <= euler[100] / euler[200] <= 2.2
    assert abs(heun[100]) < 0.01


def test_the_rows_drive_the_same_integral_as_the_schemes():
    """The table read row by row (the kernels' view) is the two schemes written out (``likelihood_ref.integrate``)."""
    x = np.random.default_rng(1).standard_normal((2, 16))
    fn = R.iso_eps_div(ALPHAS)
    for order in (1, 2):
        seq = R.grid(20)
        tab = schedule.likelihood_coefficients(seq, ALPHAS, order, "eps")
        al = R.levels(seq, ALPHAS)[0]
        u, k1, xin, acc = x / al[0], None, x.copy(), np.zeros(2)
        for row, wd in zip(tab.rows, tab.wd):
            e, d = fn(xin, int(row[0]))
            un = u + row[2] * e + (row[1] * k1 if row[1] != 0 else 0.0)
            xin = row[3] * un
            if int(row[5]) & R.SAVE:
                k1 = e
            if int(row[5]) & R.COMMIT:
                u = un
            acc += wd * d
        got = R.log_normal(xin) + 16 * tab.logdet_per_dim + acc
        want, xt, _ = R.integrate(x, seq, ALPHAS, order, fn)
        assert np.allclose(got, want, rtol=0, atol=1e-9 * np.abs(want).max()) and np.allclose(xin, xt, rtol=1e-12, atol=0)


# ---- 2. the probe ---------------------------------------------------------------------------------------------------------------------
PROBE_SEED = 0  # the first of 0, 1, 2, ... at which the float64 estimate lies within 3 standard errors (asserted below)


def _probe_estimate(seed, k_probes=64, d=12):
    jac = R.correlated_jacobian(R.correlated_cov(d), float(ALPHAS[100]))
    assert np.abs(jac - np.diag(np.diag(jac))).max() > 0.05 * np.abs(np.diag(jac)).max()  # not diagonal
    r = np.stack([R.probe(seed, 0, (1, d), k)[0] for k in range(k_probes)])
    assert set(np.unique(r)) == {-1.0, 1.0}
    est = np.einsum("ki,ij,kj->k", r, jac, r)
    return float(est.mean()), float(est.std(ddof=1)) / math.sqrt(k_probes), float(np.trace(jac))


def test_probe_estimator_is_unbiased():
    first = next(s for s in range(16) if (lambda m, se, tr: abs(m - tr) <= 3 * se)(*_probe_estimate(s)))
    assert first == PROBE_SEED
    mean, se, trace = _probe_estimate(PROBE_SEED)
    print(f"[likelihood probe] seed {PROBE_SEED}: mean {mean:.5f}, trace {trace:.5f}, standard error {se:.5f}")
    assert se > 0 and abs(mean - trace) <= 4 * se


# ---- 3. the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("prediction", ["eps", "v"])
def test_rows_against_a_direct_restatement(order, prediction):
    seq = [0, 3, 40, 412, 999]
    tab = schedule.likelihood_coefficients(seq, torch.from_numpy(ALPHAS), order, prediction)
    rows, trace, logdet = R.rows(seq, ALPHAS, order, prediction)
    assert tab.rows.dtype == np.float64 and tab.rows.shape == ((len(seq) - 1) * order, schedule.LKX_STRIDE) and schedule.LKX_STRIDE == 8
    assert np.allclose(tab.rows, rows, rtol=1e-14, atol=0)
    assert np.array_equal(tab.wd, tab.rows[:, 4]) and tab.wd.dtype == np.float64
    assert math.isclose(tab.trace_per_dim, trace, rel_tol=1e-13, abs_tol=0) and math.isclose(tab.logdet_per_dim, logdet, rel_tol=1e-14)
    assert np.array_equal(tab.rows[:, 0].astype(np.float32).astype(np.float64), tab.rows[:, 0])  # t survives fp32
    assert np.all(tab.rows[:, 6:] == 0)
    flags = tab.rows[:, 5].astype(int).tolist()
    assert flags == ([_lib.LKX_COMMIT] * 4 if order == 1 else [_lib.LKX_SAVE, _lib.LKX_COMMIT] * 4)


def test_v_constant_is_s1_times_the_eps_weights():
    """eps = s1 x + s2 v: per row the v table's wd is s2 times the eps table's, and the constant is the sum of (eps wd) s1."""
    seq = [0, 100, 500, 999]
    for order in (1, 2):
        e = schedule.likelihood_coefficients(seq, ALPHAS, order, "eps")
        v = schedule.likelihood_coefficients(seq, ALPHAS, order, "v")
        vt = schedule.v_table(ALPHAS)[e.rows[:, 0].astype(int)]
        assert e.trace_per_dim == 0.0
        assert np.allclose(v.wd, e.wd * vt[:, 1], rtol=1e-15, atol=0)
        assert math.isclose(v.trace_per_dim, float((e.wd * vt[:, 0]).sum()), rel_tol=1e-13)
        assert np.array_equal(v.rows[:, :4], e.rows[:, :4])  # the state update does not know the prediction type
        d = 24
        assert math.isclose(d * v.trace_per_dim, float(sum(w * s1 * d for w, s1 in zip(e.wd, vt[:, 0]))), rel_tol=1e-13)


def test_euler_step_is_the_ddim_step_in_u():
    """A DDIM step from t_hi to t_lo moves u = x / alpha by (sigma_lo / alpha_lo - sigma_hi / alpha_hi) eps; Euler's ``we`` is
    the same difference walked upwards."""
    seq = [0, 7, 250, 999]
    tab = schedule.likelihood_coefficients(seq, ALPHAS, 1, "eps")
    for i, row in enumerate(tab.rows):
        _, s1, s2, s3, c2, _ = schedule.ddim_coefficients(seq[i:i + 2], ALPHAS)[0]
        assert math.isclose(row[2], s1 / s2 - c2 / s3, rel_tol=1e-13)
        assert row[3] == s2 and row[0] == seq[i]


@pytest.mark.parametrize("kw, msg", [
    (dict(seq=[5]), "at least 2 levels"),
    (dict(seq=[]), "must not be empty"),
    (dict(seq=[0, 5, 5]), "strictly increasing"),
    (dict(seq=[0, 1000]), r"lie in 0\.\.999"),
    (dict(seq=[0, 2.5]), "must hold integers"),
    (dict(order=3), "order must be 1"),
    (dict(order=True), "order must be 1"),
    (dict(prediction="x0"), "prediction must be"),
])
def test_table_refusals(kw, msg):
    args = dict(seq=[0, 10, 999], alphas=ALPHAS, order=2, prediction="eps")
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        schedule.likelihood_coefficients(**args)


class _Never:
    def __call__(self, x, t):
        raise AssertionError("the model was called")


@pytest.mark.parametrize("kw, exc, msg", [
    (dict(noise=BrownianStream(1)), TypeError, "noise must be a NoiseStream, got BrownianStream"),
    (dict(noise=7), TypeError, "noise must be a NoiseStream"),
    (dict(threshold=schedule.X0Clip(1.0)), ValueError, "no threshold="),
    (dict(window=16), ValueError, "no window="),
    (dict(hop=8), ValueError, "no hop="),
    (dict(eta=1.0), TypeError, "unexpected keyword"),
    (dict(probes=0), ValueError, "probes must be a positive integer"),
    (dict(probes=1.5), ValueError, "probes must be a positive integer"),
    (dict(order=4), ValueError, "order must be 1"),
    (dict(seq=[3]), ValueError, "at least 2 levels"),
    (dict(x=torch.zeros(2, 3)), ValueError, r"\[B, C, T, F\]"),
    (dict(x=torch.zeros(1, 1, 1, 3)), ValueError, "multiple of 4"),
    (dict(stats=[]), ValueError, "stats must be a dict"),
    (dict(prediction="x0"), ValueError, "prediction must be"),
])
def test_log_likelihood_refuses_before_any_device_work(kw, exc, msg):
    """CPU tensors, a model that must never be called, no GPU: every refusal comes before the library is touched."""
    args = dict(x=torch.zeros(2, 1, 4, 4), seq=[0, 500, 999], model=_Never(), alphas=ALPHAS)
    args.update(kw)
    with pytest.raises(exc, match=msg):
        D.log_likelihood(**args)


def test_public_names():
    from ddim_audio_amd import likelihood
    assert D.log_likelihood is likelihood.log_likelihood and D.Likelihood is likelihood.Likelihood
    assert D.LikelihoodStepper is likelihood.LikelihoodStepper
    assert D.Likelihood._fields == ("logp", "bpd", "stderr", "latent")
    assert isinstance(NoiseStream(3).for_rank(8, 1, 2), NoiseStream)


# ---- the third header table ----------------------------------------------------------------------------------------------------------
def test_feature_directory_table():
    assert list(_lib.FEATURES) == ["lkx_likelihood.h"]
    h = _lib.FEATURES["lkx_likelihood.h"]
    assert tuple(h.funcs) == LKX and h.structs == {}
    assert h.consts == {"LKX_STRIDE": 8, "LKX_SAVE": 1, "LKX_COMMIT": 2}
    assert (_lib.LKX_STRIDE, _lib.LKX_SAVE, _lib.LKX_COMMIT) == (8, 1, 2)
    P = c_void_p
    assert h.funcs["lkx_partials_doubles"] == (c_longlong, [c_int, c_longlong])
    assert h.funcs["lkx_probe_fill"] == (c_int, [P, c_int, c_longlong, c_ulonglong, c_uint, c_uint, P])
    assert h.funcs["lkx_stage"] == (c_int, [P, P, P, P, P, P, P, P, c_int, c_longlong, c_ulonglong, c_uint, c_uint, P])
    assert h.funcs["lkx_finish"] == (c_int, [P, P, P, P, c_int, c_int, P])
    assert h.funcs["lkx_sumsq"] == (c_int, [P, P, P, c_int, c_longlong, P])
    # kept apart from the other two tables
    assert "lkx_likelihood.h" not in _lib.HEADERS and "lkx_likelihood.h" not in _lib.FEATURE_HEADERS
    assert not set(LKX) & (set(_lib._OWNER) | set(_lib._FEATURE_OWNER))
    assert not any(name.endswith("_EXPORTS") and set(LKX) & set(getattr(_lib, name)) for name in dir(_lib))
    assert _lib.DDIMX_ABI_VERSION == 2


def test_feature_functions_are_bound_on_first_use():
    lib = _lib._Library(_lib.LIB_PATH)  # a fresh object: nothing bound yet
    assert not any(n in vars(lib) for n in LKX)
    for name in LKX:
        fn = getattr(lib, name)
        want = _lib.FEATURES["lkx_likelihood.h"].funcs[name]
        assert name in vars(lib) and (fn.restype, list(fn.argtypes)) == (want[0], want[1])
    with pytest.raises(AttributeError, match=r"no include/ddimx\*\.h declares lkx_nonesuch"):
        getattr(lib, "lkx_nonesuch")
    # the launchers' argument checks run without a GPU: refused before any launch
    assert lib.lkx_partials_doubles(3, 4 * 257) == 3 and lib.lkx_partials_doubles(1, 4 * 1024 * 5 + 4) == 6
    assert lib.lkx_partials_doubles(0, 4) == 0 and lib.lkx_partials_doubles(1, 6) == 0
    assert lib.lkx_stage(None, None, None, None, None, None, None, None, 1, 4, 0, 0, 0, None) != 0
    assert "lkx_stage: null argument" in lib.ddimx_last_error().decode()


def test_a_function_two_tables_declare_is_refused():
    with pytest.raises(RuntimeError, match="lkx_b.h: lkx_g is declared in lkx_a.h too"):
        _lib._parse_all({"lkx_a.h": "int lkx_g(int n);", "lkx_b.h": "int lkx_g(int n);"})


@pytest.mark.skipif(shutil.which("nm") is None, reason="nm (binutils) is needed to list the library's dynamic symbols")
def test_library_defines_exactly_the_declared_lkx_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.split()}
    assert {n for n in defined if n.startswith("lkx_")} == set(LKX)
