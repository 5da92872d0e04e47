"""SNR loss weighting and progressive distillation, host side (no GPU): the weight table against the fp64 restatement
(tests/distill_ref.py), the coefficient table -- its DDIM columns, omega, and the identity the feature rests on: the student's ONE
step with the convex-form target lands where the teacher's TWO steps land --, ``halve_seq``, every ValueError, the second header's
exports and ``TrainingState``'s configuration fields."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, configs, schedule, train
from ddim_audio_amd.schedule import ddim_coefficients, distill_coefficients, halve_seq, loss_weight_table, make_schedule

import distill_ref as R
import model_harness as MH

SEQS = {"uniform10": list(range(0, 1000, 100)), "all1000": list(range(1000)), "two": [0, 999], "ragged": [3, 870, 990, 999]}


# ---- 1. the weight table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["min_snr", "trunc_snr"])
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("gamma", [5.0, 1.0, 20.0])
def test_weight_table_vs_restatement(kind, prediction, gamma):
    """The two are written differently (the table's closed forms against x0 weight / conversion factor): they agree to a few
    float64 roundings, 1e-14 relative."""
    a = MH.alphas()
    w = loss_weight_table(a, prediction, kind, gamma)
    want = R.loss_weights(a.numpy(), prediction, kind, gamma)
    assert w.dtype == np.float64 and w.shape == (1000,)
    assert np.all(np.abs(w - want) <= 1e-14 * want) and np.all(w > 0)


def test_weight_table_anchors_on_the_audio_schedule():
    """linear beta 1e-4 -> 0.02, fp32 cumprod: SNR falls below gamma = 5 between t = 129 and t = 130, below 1 between t = 258 and
    t = 259.  min(1, gamma / SNR) is therefore < 1 for t < 130 and exactly 1 from t = 130 on (the weight caps the HIGH-SNR, small-t
    end); max(1, 1 / SNR) is exactly 1 for t < 259 and > 1 from t = 259 on."""
    a = MH.alphas()
    snr = R.table64(a.numpy()) / (1.0 - R.table64(a.numpy()))
    assert snr[129] > 5.0 > snr[130] and snr[258] > 1.0 > snr[259]
    w = loss_weight_table(a, "eps", "min_snr", 5.0)
    assert np.all(w[:130] < 1.0) and np.all(w[130:] == 1.0)
    w = loss_weight_table(a, "eps", "trunc_snr")
    assert np.all(w[:259] == 1.0) and np.all(w[259:] > 1.0)
    # v: both weights stay inside (0, 1]
    for kind in ("min_snr", "trunc_snr"):
        w = loss_weight_table(a, "v", kind)
        assert np.all(w > 0) and np.all(w <= 1.0)
    assert loss_weight_table(a, "eps", "uniform") is None and loss_weight_table(a, "v", "uniform") is None


def test_weight_table_raises():
    a = MH.alphas()
    with pytest.raises(ValueError, match="loss weight"):
        loss_weight_table(a, "eps", "snr")
    with pytest.raises(ValueError, match="prediction"):
        loss_weight_table(a, "x0", "min_snr")
    for g in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            loss_weight_table(a, "eps", "min_snr", g)
    for bad in (torch.tensor([0.5, 1.0]), torch.tensor([0.0, 0.5]), torch.tensor([0.5, -0.1]), torch.tensor([0.5, float("nan")]),
                torch.tensor([])):
        with pytest.raises(ValueError, match="alphas"):
            loss_weight_table(bad, "eps", "min_snr")
        with pytest.raises(ValueError, match="alphas"):
            loss_weight_table(bad, "eps", "uniform")


# ---- 2. halve_seq and distill_coefficients --------------------------------------------------------------------------------------------
def test_halve_seq():
    assert halve_seq([0, 999]) == [999]
    assert halve_seq([3, 870, 990, 999]) == [870, 999]
    s16 = schedule.make_seq(1000, 16)[:16]
    assert halve_seq(s16) == s16[1::2] and halve_seq(halve_seq(s16)) == s16[3::4]
    for bad in ([], [5], [1, 2, 3], [2, 2], [3, 1], [-1, 4], [0, 1.5], [True, 3]):
        with pytest.raises(ValueError):
            halve_seq(bad)


@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("name", list(SEQS))
def test_coefficient_rows(name, pred):
    a = MH.alphas()
    seq = SEQS[name]
    c = distill_coefficients(seq, a, pred)
    assert c.dtype == np.float64 and c.shape == (len(seq) // 2, 12)
    ddim = {int(r[0]): r for r in ddim_coefficients(seq, a, 0.0)}  # the teacher's own table, by timestep
    a64 = R.table64(a.numpy())
    for k in range(c.shape[0]):
        t, t_mid, t_end = R.steps_of(seq, k)
        assert np.array_equal(c[k, :5], ddim[t][:5]) and ddim[t][5] == 0.0
        assert (int(c[k, 0]), int(c[k, 5])) == (t, t_mid)
        assert np.array_equal(c[k, 6:8], ddim[t_mid][1:3])
        assert np.array_equal(np.float32(c[k, 3:5]), np.float32(c[k, [7, 6]]))  # (s3, c2) = (s2', s1'): one value, two places
        al, si = R.alpha_sigma(a64, t)
        want = (1 / si, -al / si) if pred == "eps" else (al / si, -1 / si)
        assert np.allclose(c[k, 9:11], want, rtol=1e-15, atol=0) and c[k, 11] == 0.0
        assert c[k, 8] == 0.0 if k == 0 else 0.0 < c[k, 8] < 0.5


def _teacher(a64):
    """An arbitrary nonlinear 'network': eps as a function of (z, t), float64."""
    def eps(z, t):
        return np.tanh(0.7 * z + 0.001 * t) + 0.3 * np.sin(z * z) * np.sqrt(1.0 - a64[t])
    return eps


@pytest.mark.parametrize("name", list(SEQS))
def test_one_student_step_equals_two_teacher_steps(name):
    """float64, every student step of the sequence: (1) the convex form x = m1 + omega (m0 - m1) with the table's omega equals the
    restatement's direct formula, (2) the target from the table's (cz, cx) equals the restatement's, (3) ONE reference DDIM step
    t -> t'' whose x0 prediction is x lands on the teacher's z''.  All to 1e-12, relative to the operands' size (z is O(1))."""
    a = MH.alphas()
    a64 = R.table64(a.numpy())
    seq = SEQS[name]
    teacher = _teacher(a64)
    rng = np.random.default_rng(7)
    for pred in ("eps", "v"):
        c = distill_coefficients(seq, a, pred)
        for k in range(c.shape[0]):
            t, t_mid, t_end = R.steps_of(seq, k)
            z = rng.standard_normal(64)
            _, s1, s2, s3, c2, _, s1m, s2m, omega, cz, cx, _ = c[k]
            e0 = teacher(z, t)
            m0 = (z - s1 * e0) / s2
            z_mid = s3 * m0 + c2 * e0
            m1 = (z_mid - s1m * teacher(z_mid, t_mid)) / s2m
            x = m1 + omega * (m0 - m1)
            target = cz * z + cx * x
            want_target, want_x = R.distill_target(teacher, z, k, seq, a.numpy(), pred)
            scale = 1.0 + np.abs(want_x).max()
            assert np.abs(x - want_x).max() <= 1e-12 * scale, (name, k)
            assert np.abs(target - want_target).max() <= 1e-12 * (1.0 + np.abs(want_target).max()), (name, k)
            # the student's single step from z with x0 prediction x, against the teacher's two steps
            al, si = R.alpha_sigma(a64, t)
            al_e, si_e = R.alpha_sigma(a64, t_end)
            landed = al_e * x + si_e * (z - al * x) / si
            _, zm = R.ddim_step(z, teacher(z, t), a64, t, t_mid)
            _, z_end = R.ddim_step(zm, teacher(zm, t_mid), a64, t_mid, t_end)
            assert np.abs(landed - z_end).max() <= 1e-12 * (1.0 + np.abs(z_end).max()), (name, k)


def test_coefficients_raise():
    a = MH.alphas()
    for bad in ([], [5], [1, 2, 3], [2, 2], [3, 1], [-1, 4], [0, 1000], [0, 1.5], [True, 3]):
        with pytest.raises(ValueError, match="teacher_seq"):
            distill_coefficients(bad, a)
    with pytest.raises(ValueError, match="prediction"):
        distill_coefficients([0, 999], a, "x0")


# ---- 3. the second header, the public names, the configuration -----------------------------------------------------------------------
def test_distill_exports_resolve_and_the_first_header_is_unchanged():
    assert _lib.DISTILL_EXPORTS == ("ddimxd_sqerr_loss_w", "ddimxd_sqerr_loss_w_bwd_mean", "ddimxd_distill_half", "ddimxd_distill_target")
    assert len(_lib.EXPORTS) == 151 and _lib.EXPORTS[-1] == "ddimx_adam_multi_dyn" and not set(_lib.DISTILL_EXPORTS) & set(_lib.EXPORTS)
    assert _lib.DDIMX_DISTILL_STRIDE == schedule.DISTILL_STRIDE == 12
    lib = _lib.load()
    from ctypes import c_int, c_longlong, c_void_p
    for name in _lib.DISTILL_EXPORTS:
        fn = getattr(lib, name)
        assert fn.restype is c_int and fn.argtypes[-1] is c_void_p and fn.argtypes[-2] is c_longlong and fn.argtypes[-3] is c_int
    assert list(lib.ddimxd_sqerr_loss_w.argtypes[:4]) == [c_void_p, c_void_p, c_void_p, c_int]
    assert lib.ddimx_abi_version() == _lib.DDIMX_ABI_VERSION == 2
    assert D.distill_target.__module__ == D.distill_step.__module__ == "ddim_audio_amd.distill"
    assert D.target_loss is D.losses.target_loss


def _micro(**model_fields):
    d = configs.micro_dict("torch.FloatTensor")
    d["model"].update(model_fields)
    cfg = configs.dict2namespace(d)
    return cfg, D.Model(cfg)


def test_training_state_reads_the_loss_weight():
    cfg, m = _micro()
    assert not hasattr(cfg.model, "loss_weight") and train.TrainingState(cfg, m).loss_weight is None
    cfg, m = _micro(loss_weight="uniform")
    assert train.TrainingState(cfg, m).loss_weight is None
    a = make_schedule(cfg.diffusion)[1]
    for kind, typ, gamma in (("min_snr", "simple", None), ("min_snr", "v", 2.0), ("trunc_snr", "v", None)):
        fields = dict(loss_weight=kind, type=typ)
        if gamma is not None:
            fields["loss_gamma"] = gamma
        cfg, m = _micro(**fields)
        w = train.TrainingState(cfg, m).loss_weight
        want = loss_weight_table(a, "v" if typ == "v" else "eps", kind, 5.0 if gamma is None else gamma)
        assert w.dtype == torch.float32 and w.device.type == "cpu" and np.array_equal(w.numpy(), np.float32(want))
    cfg, m = _micro(loss_weight="snr")
    with pytest.raises(ValueError, match="loss weight"):
        train.TrainingState(cfg, m)


def test_distill_arguments_raise_before_any_device_work():
    """None of these reaches the library (there is no GPU here: a launch would raise something else)."""
    a = MH.alphas()
    z = torch.zeros(2, 2, 8, 16)
    k = torch.tensor([0, 1])
    model = lambda x, t: x  # noqa: E731
    S = [3, 870, 990, 999]
    bad = [(dict(prediction="x0"), "prediction"), (dict(student_prediction="x0"), "prediction"),
           (dict(teacher_seq=[3, 870, 990]), "teacher_seq"), (dict(teacher_seq=[3, 870, 990, 1000]), "teacher_seq"),
           (dict(k=torch.tensor([0, 2])), "k entries"), (dict(k=torch.tensor([-1, 0])), "k entries"),
           (dict(k=torch.tensor([0])), "k must"), (dict(k=torch.tensor([0.0, 1.0])), "k must"), (dict(k=[0, 1]), "k must"),
           (dict(z=torch.zeros(2, 8, 16)), "x must"), (dict(z=torch.zeros(2, 1, 1, 3)), "multiple of 4")]
    for kw, msg in bad:
        args = dict(teacher=model, z=z, k=k, teacher_seq=S, alphas=a)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            D.distill_target(**args)
    teacher = _micro()[1].train()
    with pytest.raises(ValueError, match="eval mode"):
        D.distill_target(teacher, torch.zeros(2, teacher.config.channels, 8, teacher.config.f_size), k, S, a)
