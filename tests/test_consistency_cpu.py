"""Consistency distillation and sampling, host side (ddim_audio_amd/schedule.py, consistency.py, _lib.py's feature headers), against
tests/consistency_ref.py.  No GPU: 1. the (p, q) table; 2. the teacher's rows and the sampler's rows; 3. the Gaussian study
(what the method converges to, and how far that is from the exact flow); 4. every refusal, before any device work; 5. the binding
of include/cmx_consistency.h."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, configs, schedule
from ddim_audio_amd.schedule import consistency_coefficients, consistency_pairs, consistency_table, ddim_coefficients
import consistency_ref as R
import model_harness as MH

KW = [dict(), dict(sigma_data=0.3, timestep_scale=4.0, t_min=3)]


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", KW, ids=["defaults", "other"])
@pytest.mark.parametrize("pred", ["eps", "v"])
def test_table_vs_restatement(pred, kw):
    """Row t is (p, q) of f = c_skip x + c_out x0_hat read off at the unit inputs; every row t <= t_min is (1, 0) exactly."""
    a = MH.alphas()
    a64 = R.table64(a.numpy())
    tab = consistency_table(a, pred, **kw)
    assert tab.dtype == np.float64 and tab.shape == (1000, 2)
    t_min = kw.get("t_min", 0)
    assert np.array_equal(tab[:t_min + 1], [[1.0, 0.0]] * (t_min + 1)) and not np.signbit(tab[:t_min + 1]).any()
    for t in (t_min + 1, 7, 412, 998, 999):
        p, q = R.pq(a64, t, pred, **kw)
        assert abs(tab[t, 0] - p) <= 1e-12 * abs(p) and abs(tab[t, 1] - q) <= 1e-12 * abs(q), t
    assert (tab[t_min + 1:, 1] < 0).all() and np.isfinite(tab).all()


def test_eps_and_v_tables_give_one_function():
    """For a consistent pair (eps, v) of one data prediction the two tables give the same f, to 1e-12 of its terms' size."""
    a = MH.alphas()
    a64 = R.table64(a.numpy())
    te, tv = consistency_table(a, "eps"), consistency_table(a, "v")
    rng = np.random.default_rng(7)
    for t in (1, 5, 300, 870, 999):
        al, si = R.alpha_sigma(a64, t)
        x0, e = rng.standard_normal(64), rng.standard_normal(64)
        x = al * x0 + si * e
        v = al * e - si * x0
        fe, fv = te[t, 0] * x + te[t, 1] * e, tv[t, 0] * x + tv[t, 1] * v
        size = np.abs(te[t, 0] * x) + np.abs(te[t, 1] * e)
        assert (np.abs(fe - fv) <= 1e-12 * size).all(), t
        c_skip, c_out = R.scalings(t)
        assert (np.abs(fv - (c_skip * x + c_out * x0)) <= 1e-12 * size).all(), t


def test_table_anchors_on_the_audio_schedule():
    """What the docstring quotes, recomputed from the schedule: at t = 999 an eps student's output enters f about 157 times,
    a v student's once."""
    a64 = R.table64(MH.alphas().numpy())
    al, si = R.alpha_sigma(a64, 999)
    c_skip, c_out = R.scalings(999)
    te, tv = consistency_table(MH.alphas(), "eps"), consistency_table(MH.alphas(), "v")
    assert abs(te[999, 0] - (c_skip + c_out / al)) < 1e-9 and abs(te[999, 1] + c_out * si / al) < 1e-9
    assert round(te[999, 0], 2) == 157.41 and round(te[999, 1], 2) == -157.41
    assert round(tv[999, 0], 4) == 0.0064 and round(tv[999, 1], 4) == -1.0
    print(f"[consistency table t=999] eps (p, q) = ({te[999, 0]:.2f}, {te[999, 1]:.2f}), v (p, q) = ({tv[999, 0]:.4f}, {tv[999, 1]:.4f})")


# ---- 2. the rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [1, 2])
def test_pairs_rows_are_the_teachers_ddim_rows(skip):
    a = MH.alphas()
    S = [0, 3, 500, 870, 999]
    rows, t_hi, t_lo = consistency_pairs(S, a, skip)
    assert rows.dtype == np.float64 and rows.shape == (len(S) - skip, schedule.DISTILL_STRIDE) and schedule.DISTILL_STRIDE == 12
    assert t_hi.tolist() == S[skip:] and t_lo.tolist() == S[:len(S) - skip]
    for n in range(len(S) - skip):
        want = ddim_coefficients([S[n], S[n + skip]], a, 0.0)[0]
        assert want[0] == S[n + skip] and want[5] == 0
        assert np.abs(rows[n, :5] - want[:5]).max() <= 1e-12
        assert rows[n, 5] == S[n] and np.abs(rows[n, 6:8] - [want[4], want[3]]).max() <= 1e-12 and not rows[n, 8:].any()


@pytest.mark.parametrize("pred", ["eps", "v"])
def test_sampler_rows(pred):
    a = MH.alphas()
    a64 = R.table64(a.numpy())
    seq = [100, 500, 870, 999]
    coef = consistency_coefficients(seq, a, pred)
    tab = consistency_table(a, pred)
    assert coef.dtype == np.float64 and coef.shape == (4, schedule.CONSISTENCY_STRIDE) and schedule.CONSISTENCY_STRIDE == _lib.CMX_STRIDE == 8
    assert coef[:, 0].tolist() == [999, 870, 500, 100]
    for i, row in enumerate(coef):
        t = seq[3 - i]
        assert np.array_equal(row[1:3], tab[t]) and not row[[4, 6, 7]].any()
        if i < 3:
            al, si = R.alpha_sigma(a64, seq[2 - i])
            assert abs(row[3] - al) <= 1e-12 and abs(row[5] - si) <= 1e-12 and row[5] > 0
    assert coef[-1, 3:].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]  # the last row is final: xt = x0
    one = consistency_coefficients([999], a, pred, t_min=5)
    assert one.shape == (1, 8) and one[0, 3:].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0] and np.array_equal(one[0, 1:3], consistency_table(a, pred, t_min=5)[999])


# ---- 3. the Gaussian study ------------------------------------------------------------------------------------------------------------
def test_gaussian_fixed_point_is_the_teachers_ddim_map():
    """Data N(0, 0.25), the exact predictor as teacher, students f(x, t) = theta_t x.  The fixed point of the distillation
    recursion on N levels is the product of the teacher's N - 1 DDIM factors -- the teacher's whole DDIM run in one evaluation --
    whichever prediction the student has.  Its error against the exact flow from t = 999 is first order in 1 / N:
    err(50) < 0.5 err(20) and err(200) < 0.3 err(50) (measured: ratios 0.40 and 0.25; errors 0.139, 0.0560, 0.0141, 0.0028 at 20,
    50, 200, 1000 levels)."""
    a = R.table64(MH.alphas().numpy())
    var, err = 0.25, {}
    exact = R.gaussian_flow(a, 999, 0, var)
    for n in (20, 50, 200, 1000):
        S = R.uniform_levels(n)
        assert len(S) == n and S[0] == 0 and S[-1] == 999
        prod = float(np.prod([R.gaussian_ddim_factor(a, S[i + 1], S[i], var) for i in range(n - 1)]))
        for pred in ("eps", "v"):
            theta = R.gaussian_fixed_point(a, S, var, pred)
            assert abs(theta[999] - prod) <= 1e-12 * prod, (n, pred)
        err[n] = abs(prod - exact) / exact
    print("[consistency gaussian] one-step error from t = 999 against the exact flow: " + ", ".join(f"{n} levels {e:.4f}" for n, e in err.items()))
    print(f"[consistency gaussian] ratios err(50) / err(20) = {err[50] / err[20]:.2f}, err(200) / err(50) = {err[200] / err[50]:.2f}")
    assert err[50] < 0.5 * err[20] and err[200] < 0.3 * err[50]
    assert err[1000] < err[200]
    # skip = 2: the pairs reach every second level from S[0]; the map from the top is the teacher's run on those levels
    S = R.uniform_levels(21)
    theta = R.gaussian_fixed_point(a, S, var, "v", skip=2)
    prod = float(np.prod([R.gaussian_ddim_factor(a, S[i + 2], S[i], var) for i in range(0, 19, 2)]))
    assert abs(theta[999] - prod) <= 1e-12 * prod


def test_gaussian_multistep_sampling_variance():
    """The variance of 1-, 2- and 4-evaluation consistency sampling with the fixed-point student from x_T ~ N(0, 1), against the
    variance of the data at the lowest level: re-noising does not compound the one-step error (printed; the README quotes it)."""
    a = R.table64(MH.alphas().numpy())
    var, out = 0.25, {}
    for n in (50, 200):
        S = R.uniform_levels(n)
        theta = R.gaussian_fixed_point(a, S, var, "v")
        al0, si0 = R.alpha_sigma(a, 0)
        want = al0 * al0 * var + si0 * si0
        for evals in (1, 2, 4):
            seq = [S[(n - 1) * (k + 1) // evals] for k in range(evals)]
            v = 1.0
            for j in reversed(range(evals)):
                v = theta[seq[j]] ** 2 * v
                if j:
                    al, si = R.alpha_sigma(a, seq[j - 1])
                    v = al * al * v + si * si
            out[n, evals] = abs(v - want) / want
    print("[consistency gaussian] variance error: " + ", ".join(f"{n} levels / {e} evaluations {v:.3f}" for (n, e), v in out.items()))
    assert all(out[200, e] < 0.5 * out[50, e] for e in (1, 2, 4)) and max(out.values()) < 0.2


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_schedule_functions_raise():
    a = MH.alphas()
    for kw, msg in ((dict(prediction="x0"), "prediction"), (dict(sigma_data=0.0), "sigma_data"), (dict(sigma_data=float("inf")), "sigma_data"),
                    (dict(sigma_data=float("nan")), "sigma_data"), (dict(timestep_scale=-1.0), "timestep_scale"),
                    (dict(timestep_scale=float("inf")), "timestep_scale"), (dict(t_min=-1), "t_min"), (dict(t_min=1000), "t_min"),
                    (dict(t_min=1.5), "t_min"), (dict(t_min=True), "t_min"), (dict(alphas=torch.tensor([0.5, 1.0])), "alphas"),
                    (dict(alphas=torch.tensor([])), "alphas")):
        args = dict(alphas=a, prediction="v")
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            consistency_table(**args)
    S = [0, 3, 500, 870]
    for kw, msg in ((dict(seq=[0, 500, 500]), "increasing"), (dict(seq=[0, 870, 500]), "increasing"), (dict(seq=[0, 500, 1000]), "entries"),
                    (dict(seq=[-1, 0, 5]), "entries"), (dict(seq=[0, 1.5, 3]), "integers"), (dict(seq=[]), "empty"),
                    (dict(seq=[3, 500, 870]), "t_min"), (dict(seq=S, t_min=3), "t_min"), (dict(skip=0), "skip"), (dict(skip=4), "skip"),
                    (dict(skip=1.0), "skip"), (dict(skip=True), "skip"), (dict(seq=[0]), "skip")):
        args = dict(seq=S, alphas=a, skip=1)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            consistency_pairs(**args)
    assert consistency_pairs([3, 500], a, 1, t_min=3)[1].tolist() == [500]
    for kw, msg in ((dict(seq=[5, 5]), "increasing"), (dict(seq=[0, 5]), "t_min"), (dict(seq=[3, 9], t_min=3), "t_min"),
                    (dict(seq=[5, 1000]), "entries"), (dict(seq=[]), "empty"), (dict(prediction="x"), "prediction"),
                    (dict(sigma_data=-0.5), "sigma_data")):
        args = dict(seq=[5, 999], alphas=a, prediction="eps")
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            consistency_coefficients(**args)


def _micro(**model_fields):
    d = configs.micro_dict("torch.FloatTensor")
    d["model"].update(model_fields)
    cfg = configs.dict2namespace(d)
    return cfg, D.Model(cfg)


def test_arguments_raise_before_any_device_work():
    """None of these reaches the library (there is no GPU here: a launch would raise something else)."""
    a = MH.alphas()
    z, n = torch.zeros(2, 2, 8, 16), torch.tensor([0, 2])
    model = lambda x, t: x  # noqa: E731
    S = [0, 3, 870, 999]
    bad = [(dict(teacher_prediction="x0"), "prediction"), (dict(target_prediction="x0"), "prediction"), (dict(seq=[3, 870, 999]), "t_min"),
           (dict(seq=[0, 870, 1000]), "entries"), (dict(skip=4), "skip"), (dict(skip=2, n=torch.tensor([0, 2])), "n entries"),
           (dict(n=torch.tensor([-1, 0])), "n entries"), (dict(n=torch.tensor([0])), "n must"), (dict(n=torch.tensor([0.0, 1.0])), "n must"),
           (dict(n=[0, 1]), "n must"), (dict(z=torch.zeros(2, 8, 16)), "x must"), (dict(z=torch.zeros(2, 1, 1, 3)), "multiple of 4"),
           (dict(sigma_data=0), "sigma_data")]
    for kw, msg in bad:
        args = dict(target_model=model, teacher=model, z=z, n=n, seq=S, alphas=a)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            D.consistency_target(**args)
    cfg, m = _micro()
    zm = torch.zeros(2, m.config.channels, 8, m.config.f_size)
    with pytest.raises(ValueError, match="teacher must be in eval mode"):
        D.consistency_target(model, m.train(), zm, n, S, a)
    with pytest.raises(ValueError, match="target model must be in eval mode"):
        D.consistency_target(m.train(), model, zm, n, S, a)
    # the step: its own arguments, and everything above through it
    from ddim_audio_amd import train
    student = _micro()[1]
    state = train.TrainingState(cfg, student)
    for kw, msg in ((dict(mu=1.5), "mu"), (dict(mu=float("nan")), "mu"), (dict(huber_c=-1.0), "huber_c"), (dict(huber_c=float("inf")), "huber_c"),
                    (dict(seq=[1, 5]), "t_min"), (dict(skip=3), "skip"), (dict(n=torch.tensor([0, 3])), "n entries"), (dict(target_model=student), "of its own")):
        args = dict(student=student, target_model=m.eval(), teacher=model, x=zm, state=state, alphas=a, seq=[0, 5, 9])
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            D.consistency_step(**args)
    # the sampler
    ns = D.NoiseStream(1)
    for kw, err, msg in ((dict(noise=D.BrownianStream(1)), TypeError, "NoiseStream"), (dict(noise=torch.zeros(1)), TypeError, "NoiseStream"),
                         (dict(noise=ns, noise_fn=torch.randn_like), ValueError, "not both"), (dict(threshold=D.X0Clip(1.0)), ValueError, "threshold"),
                         (dict(eta=1.0), TypeError, "eta"), (dict(prediction="x0"), ValueError, "prediction"), (dict(seq=[0, 5]), ValueError, "t_min"),
                         (dict(seq=[5, 5]), ValueError, "increasing"), (dict(seq=[]), ValueError, "empty"), (dict(t_min=5, seq=[5, 9]), ValueError, "t_min"),
                         (dict(x=torch.zeros(2, 8, 16)), ValueError, "x must"), (dict(x=torch.zeros(2, 1, 1, 3)), ValueError, "multiple of 4")):
        args = dict(x=z, seq=[5, 999], model=model, alphas=a)
        args.update(kw)
        with pytest.raises(err, match=msg):
            D.consistency_steps(**args)
    assert not torch.cuda.is_initialized()


# ---- 5. the binding ---------------------------------------------------------------------------------------------------------------------
CMX = ("cmx_consistency_out", "cmx_consistency_loss", "cmx_consistency_loss_bwd", "cmx_consistency_update")


def test_feature_header_is_found_parsed_and_kept_apart():
    assert list(_lib.FEATURE_HEADERS) == ["cmx_consistency.h"]
    h = _lib.FEATURE_HEADERS["cmx_consistency.h"]
    assert tuple(h.funcs) == CMX and h.consts == {"CMX_STRIDE": 8} and not h.structs and _lib.CMX_STRIDE == 8
    # the public table does not know it
    assert len(_lib.HEADERS) == 10 and all(name.startswith("ddimx") for name in _lib.HEADERS)
    assert not set(CMX) & set(_lib._OWNER) and not any(n.startswith("cmx") for n in _lib._OWNER)
    exports = sorted(n for n in vars(_lib) if n.endswith("EXPORTS"))
    assert len(exports) == 10 and "EXPORTS" in exports and not any("CMX" in n or "CONSISTENCY" in n for n in exports)
    assert _lib.DDIMX_ABI_VERSION == 2
    from ctypes import c_float, c_int, c_longlong, c_uint, c_ulonglong, c_void_p
    P = c_void_p
    assert h.funcs["cmx_consistency_out"] == (c_int, [P, P, P, c_int, P, P, c_int, c_longlong, P])
    assert h.funcs["cmx_consistency_loss"] == (c_int, [P, P, P, P, c_int, P, c_float, P, P, c_int, c_longlong, P])
    assert h.funcs["cmx_consistency_loss_bwd"] == (c_int, [P, P, P, P, c_int, P, c_float, P, P, P, c_int, c_longlong, P])
    assert h.funcs["cmx_consistency_update"] == (c_int, [P, P, P, P, P, P, c_int, c_longlong, c_ulonglong, c_uint, c_uint, P])


def test_feature_functions_bind_on_first_use():
    lib = _lib.load()
    assert lib.ddimx_abi_version() == 2
    for name in CMX:
        fn = getattr(lib, name)
        assert name in vars(lib) and (fn.restype, list(fn.argtypes)) == (_lib.FEATURE_HEADERS["cmx_consistency.h"].funcs[name][0],
                                                                         _lib.FEATURE_HEADERS["cmx_consistency.h"].funcs[name][1])
        assert getattr(lib, name) is fn
    with pytest.raises(AttributeError, match=r"no include/ddimx\*\.h declares cmx_nonesuch"):
        getattr(lib, "cmx_nonesuch")
    # a null argument is refused by the export itself: the call reaches the library with the header's types
    assert lib.cmx_consistency_out(None, None, None, 1, None, None, 1, 4, None) != 0
    assert "cmx_consistency_out: null argument" in lib.ddimx_last_error().decode()
    assert D.consistency_step.__module__ == D.consistency_steps.__module__ == D.consistency_target.__module__ == "ddim_audio_amd.consistency"


def test_a_function_in_both_tables_is_refused():
    """The rule of the import, on texts: a feature header that declares what a public header declares raises, naming both."""
    public, owner = _lib._parse_all({"ddimx_a.h": "int ddimxa_f(int n);"})
    feature, fowner = _lib._parse_all({"cmx_b.h": "int cmx_g(int n);\nint ddimxa_f(int n);"})
    assert owner == {"ddimxa_f": "ddimx_a.h"} and set(fowner) == {"cmx_g", "ddimxa_f"}
    with pytest.raises(RuntimeError, match="cmx_c.h: cmx_g is declared in cmx_b.h too"):
        _lib._parse_all({"cmx_b.h": "int cmx_g(int n);", "cmx_c.h": "int cmx_g(int n);"})
    # and the module's own tables do not overlap
    assert not set(_lib._FEATURE_OWNER) & set(_lib._OWNER)


def test_every_cmx_name_called_on_the_library_is_declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = [os.path.join(root, "bench.py")]
    for sub in ("ddim_audio_amd", "tools", "tests"):
        files += [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(root, sub)) for f in fs if f.endswith(".py")]
    used = {}
    for path in files:
        with open(path) as f:
            for name in re.findall(r"\.(cmx[a-z]*_\w+)\b", f.read()):
                used.setdefault(name, os.path.relpath(path, root))
    declared = {n for h in _lib.FEATURE_HEADERS.values() for n in h.funcs}
    assert len(files) > 100 and set(used) == declared, (used, declared)


@pytest.mark.skipif(shutil.which("nm") is None, reason="nm (binutils) is needed to list the library's dynamic symbols")
def test_library_defines_every_feature_function():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.split()}
    assert set(CMX) <= defined and {n for n in defined if n.startswith("cmx_")} == set(CMX)
