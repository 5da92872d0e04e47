"""v-prediction, host side (no GPU, no library): the (s1, s2) table against every coefficient table, the inpainting table's
k1 / k2 for a v network, the fp64 restatement (tests/vpred_ref.py) -- identities, sampling the closed-form Gaussian model in its
v form against its eps form, the error amplification the feature exists for --, the registry and ``Model.prediction``, and
argument validation before any device work."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import configs, losses
from ddim_audio_amd.schedule import (ddim_coefficients, dpm_coefficients, inpaint_coefficients, invert_coefficients, logsnr_seq,
                                     make_schedule, make_seq, v_table)

import model_harness as MH
import solver_ref as R
import vpred_ref as V

VAR = 0.25  # data variance of the Gaussian model


# ---- 1. the table -------------------------------------------------------------------------------------------------------------------
def _tables(a):
    seq = make_seq(1000, 50)
    return {"ddim": ddim_coefficients(seq, a, 0.5), "dpm": dpm_coefficients(logsnr_seq(a, 20), a, 3),
            "inpaint": inpaint_coefficients(seq, a, 0.5, 0.3), "inpaint_v": inpaint_coefficients(seq, a, 0.0, 0.3, "v"),
            "invert": invert_coefficients(seq, a, iters=2)}


@pytest.mark.parametrize("kind", ["ddim", "dpm", "inpaint", "inpaint_v", "invert"])
def test_v_table_rows_are_the_coefficient_tables_columns_bit_for_bit(kind):
    a = MH.alphas()
    vt = v_table(a)
    assert vt.dtype == np.float64 and vt.shape == (1000, 2)
    v32, tab = np.float32(vt), _tables(a)[kind]
    assert tab.shape[0] >= 20
    for k in range(tab.shape[0]):
        t = int(tab[k, 0])
        assert np.array_equal(v32[t], np.float32(tab)[k, 1:3]), (kind, k, t)


def test_v_table_values():
    a = MH.alphas()
    vt = v_table(a)
    a64 = a.double().numpy()
    # (Python's pow and numpy's sqrt may differ in the last place)
    assert np.allclose(vt[:, 0], np.sqrt(1 - a64), rtol=4e-16, atol=0) and np.allclose(vt[:, 1], np.sqrt(a64), rtol=4e-16, atol=0)
    assert np.allclose(vt[:, 0] ** 2 + vt[:, 1] ** 2, 1.0, rtol=0, atol=1e-15)
    # the figures the feature is argued from: s1 / s2 at t = 999, 950, 900, 800
    ratio = vt[:, 0] / vt[:, 1]
    assert [round(float(ratio[t]), 1) for t in (999,)] == [157.4]
    assert [int(round(float(ratio[t]))) for t in (950, 900, 800)] == [97, 61, 26]
    assert abs(1.0 / float(np.float32(vt)[900, 1]) - 60.8) < 0.05


# ---- 2. inpaint_coefficients --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta,guidance", [(0.0, 0.0), (0.5, 0.3), (1.0, [0.1 * i for i in range(10)])])
def test_inpaint_coefficients_prediction(eta, guidance):
    a, seq = MH.alphas(), make_seq(1000, 10)
    base = inpaint_coefficients(seq, a, eta, guidance)
    assert np.array_equal(inpaint_coefficients(seq, a, eta, guidance, prediction="eps"), base)
    assert np.array_equal(inpaint_coefficients(seq, a, eta, guidance, "eps"), base)
    cv = inpaint_coefficients(seq, a, eta, guidance, prediction="v")
    assert cv.dtype == np.float64 and cv.shape == base.shape == (10, 9)
    assert np.array_equal(cv[:, 6], -2.0 * base[:, 1]) and np.array_equal(cv[:, 7], 2.0 * base[:, 2])
    for col in (0, 1, 2, 3, 4, 5, 8):
        assert np.array_equal(cv[:, col], base[:, col]), col
    assert not np.array_equal(cv[:, 6], base[:, 6]) and not np.array_equal(cv[:, 7], base[:, 7])


@pytest.mark.parametrize("bad", ["x0", "V", "", None, 0])
def test_inpaint_coefficients_refuses_another_prediction(bad):
    with pytest.raises(ValueError, match="prediction"):
        inpaint_coefficients([0, 500], MH.alphas(), 0.0, 0.0, bad)


def test_v_seed_decomposition_is_the_gradient():
    """k1 = -2 s1, k2 = 2 s2 for a v network: with x0 = s2 x - s1 v(x) the gradient of |m (x0 - y)|^2 w.r.t. x is
    k2 m^2 (x0 - y) + J_v^T (k1 m^2 (x0 - y)); checked in float64 against autograd on a small nonlinear map."""
    torch.manual_seed(0)
    n = 12
    W = torch.randn(n, n, dtype=torch.float64) / n ** 0.5
    net = lambda x: torch.tanh(x @ W)  # noqa: E731
    x = torch.randn(n, dtype=torch.float64, requires_grad=True)
    y, m = torch.randn(n, dtype=torch.float64), (torch.rand(n, dtype=torch.float64) > 0.4).double()
    s1, s2 = V.scales(MH.alphas(), 800)
    v = net(x)
    x0 = V.x0_from_v(x, v, s1, s2)
    (want,) = torch.autograd.grad((m * (x0 - y)).square().sum(), x, retain_graph=True)
    r = (m * m * (x0 - y)).detach()
    (jt,) = torch.autograd.grad(v, x, -2.0 * s1 * r)
    got = 2.0 * s2 * r + jt
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---- 3. the restatement in float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 412, 800, 999])
def test_identities(t):
    rng = np.random.default_rng(t)
    x0, e = rng.standard_normal(64), rng.standard_normal(64)
    s1, s2 = V.scales(MH.alphas(), t)
    assert abs(s1 * s1 + s2 * s2 - 1.0) < 1e-15
    x, v = V.q_sample(x0, e, s1, s2), V.v_target(x0, e, s1, s2)
    tol = 1e-13 * (1.0 + s1 / s2)  # recovering through the eps form divides by s2
    assert np.abs(V.eps_from_v(x, v, s1, s2) - e).max() < 1e-14
    assert np.abs(V.x0_from_v(x, v, s1, s2) - x0).max() < 1e-14
    assert np.abs(V.x0_from_eps(x, V.eps_from_v(x, v, s1, s2), s1, s2) - x0).max() < tol
    assert np.abs(V.v_target(V.x0_from_eps(x, e, s1, s2), e, s1, s2) - v).max() < tol


@pytest.mark.parametrize("order", [1, 2, 3])
def test_sampling_the_v_form_equals_sampling_the_eps_form(order):
    a = MH.alphas()
    seq = logsnr_seq(a, 12)
    x = np.random.default_rng(order).standard_normal((2, 8))
    eps_fn, v_fn = R.gaussian_model(a, VAR), V.gaussian_v_model(a, VAR)
    # the v form really is another function of x
    assert np.abs(v_fn(x, 500) - eps_fn(x, 500)).max() > 0.1
    xs_e, x0_e = R.dpm_solver_steps(x, seq, eps_fn, a, order)
    xs_v, x0_v = R.dpm_solver_steps(x, seq, V.as_eps_model(v_fn, a), a, order)
    for k in range(len(seq)):
        # eps is rebuilt as s1 x + s2 v: its fp64 rounding enters x0 divided by s2 (157 at the first level)
        assert np.abs(xs_v[k + 1] - xs_e[k + 1]).max() <= 1e-12 * np.abs(xs_e[k + 1]).max(), k
        assert np.abs(x0_v[k] - x0_e[k]).max() <= 1e-12 * np.abs(x0_e[k]).max(), k


@pytest.mark.parametrize("t", [800, 900, 950, 999])
def test_amplification_factors(t):
    """x0 error per unit error of the network output: s1 / s2 through the eps form, s1 through the v form."""
    rng = np.random.default_rng(7)
    x, out, d = rng.standard_normal(256), rng.standard_normal(256), 1e-3 * rng.standard_normal(256)
    s1, s2 = V.scales(MH.alphas(), t)
    rms = lambda u: float(np.sqrt(np.mean(u * u)))  # noqa: E731
    amp_eps = rms(V.x0_from_eps(x, out + d, s1, s2) - V.x0_from_eps(x, out, s1, s2)) / rms(d)
    amp_v = rms(V.x0_from_v(x, out + d, s1, s2) - V.x0_from_v(x, out, s1, s2)) / rms(d)
    assert abs(amp_eps - s1 / s2) <= 1e-9 * s1 / s2 and abs(amp_v - s1) <= 1e-9
    assert amp_v <= 1.0 < 25.0 <= amp_eps  # (25.7 at t = 800)
    # and through the conversion the samplers apply: an error d of v reaches x0 as s1 d, not (s1 / s2) d
    via = V.x0_from_eps(x, V.eps_from_v(x, out + d, s1, s2), s1, s2) - V.x0_from_eps(x, V.eps_from_v(x, out, s1, s2), s1, s2)
    assert abs(rms(via) / rms(d) - s1) <= 1e-6


def test_reference_loss_is_the_eps_loss_on_the_v_target():
    from oracle import ref_cpu
    a = MH.alphas()
    g = torch.Generator().manual_seed(3)
    x0, e = torch.randn(3, 2, 4, 4, generator=g, dtype=torch.float64), torch.randn(3, 2, 4, 4, generator=g, dtype=torch.float64)
    t = torch.tensor([0, 999, 412])
    net = lambda x, tt: 0.3 * x  # noqa: E731
    at = a.double().index_select(0, t).view(-1, 1, 1, 1)
    v = e * at.sqrt() - x0 * (1 - at).sqrt()
    got = V.v_prediction_loss(net, x0, t, e, a.double(), keepdim=True)
    # the eps loss with (x0, e) rotated into (x_t-preserving) v coordinates: same x_t, target v
    xt = x0 * at.sqrt() + e * (1 - at).sqrt()
    want = (v - 0.3 * xt).square().sum(dim=(1, 2, 3))
    assert torch.allclose(got, want, rtol=1e-14, atol=0)
    assert torch.allclose(V.v_prediction_loss(net, x0, t, e, a.double()), want.mean(), rtol=1e-14, atol=0)
    assert not torch.allclose(got, ref_cpu.noise_estimation_loss(net, x0, t, e, a.double(), keepdim=True))


# ---- 4. registry, Model.prediction ---------------------------------------------------------------------------------------------------
def test_registry_and_exports():
    assert set(losses.loss_registry) == {"simple", "v"}
    assert losses.loss_registry["v"] is losses.v_prediction_loss is D.v_prediction_loss
    assert losses.loss_registry["simple"] is losses.noise_estimation_loss
    from ddim_audio_amd.dropin.functions.losses import loss_registry
    assert loss_registry["v"] is losses.v_prediction_loss


def _typed_model(kind):
    d = configs.tiny_dict("torch.FloatTensor")
    if kind is None:
        del d["model"]["type"]
    else:
        d["model"]["type"] = kind
    return D.Model(configs.dict2namespace(d))  # never leaves the CPU


def test_model_prediction():
    assert _typed_model("simple").prediction == "eps"
    assert _typed_model(None).prediction == "eps"
    assert _typed_model("v").prediction == "v"
    for bad in ("x0", "V", "eps"):
        m = _typed_model(bad)  # building it is fine: the type is read when the prediction is
        with pytest.raises(ValueError, match="model.type"):
            m.prediction


# ---- 5. argument validation before any device work -----------------------------------------------------------------------------------
def _entry_points(model, x, a, bad):
    seq = [0, 300, 600]
    y, mask = torch.zeros_like(x), torch.zeros(1, 1, 1, 1)
    b = make_schedule(configs.audio_config().diffusion)[0]
    return {"generalized_steps": lambda: D.generalized_steps(x, seq, model, a, None, prediction=bad),
            "ddpm_steps": lambda: D.ddpm_steps(x, seq, model, b, None, prediction=bad),
            "dpm_solver_steps": lambda: D.dpm_solver_steps(x, seq, model, a, None, order=2, prediction=bad),
            "windowed_steps": lambda: D.windowed_steps(x, seq, model, a, None, window=16, hop=8, prediction=bad),
            "invert_steps": lambda: D.invert_steps(x, seq, model, a, None, iters=2, prediction=bad),
            "inpaint_steps": lambda: D.inpaint_steps(x, seq, model, a, None, y=y, mask=mask, prediction=bad),
            "SamplerPool": lambda: D.SamplerPool(model, a, slots=2, t_size=16, max_steps=4, prediction=bad)}


@pytest.mark.parametrize("bad", ["x0", "epsilon", 1])
@pytest.mark.parametrize("name", ["generalized_steps", "ddpm_steps", "dpm_solver_steps", "windowed_steps", "invert_steps",
                                  "inpaint_steps", "SamplerPool"])
def test_unknown_prediction_raises_before_device_work(name, bad):
    """On a CPU tensor, a CPU model and a machine without a GPU: a ValueError that names the argument, nothing else."""
    m = _typed_model("v")
    with pytest.raises(ValueError, match="prediction"):
        _entry_points(m, torch.zeros(2, 2, 32, 32), MH.alphas(), bad)[name]()


def test_a_model_of_unknown_type_is_refused_unless_told():
    m = _typed_model("x0")
    with pytest.raises(ValueError, match="model.type"):
        D.dpm_solver_steps(torch.zeros(2, 2, 16, 32), [0, 300], m, MH.alphas(), None)
