"""DDIM inversion with fixed-point refinement and latent slerp, host side (no GPU): the table the kernel reads against an
independent formation and against the restatement written from the equations (tests/invert_ref.py), the contraction of the
round-trip error with the number of iterations, the order of convergence against a closed-form solution, the slerp restatement,
and argument validation before any device work."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, configs
from ddim_audio_amd.schedule import ddim_coefficients, invert_coefficients, logsnr_seq, make_seq

import invert_ref as IR
import model_harness as MH
import solver_ref as R

VAR = 0.25  # data variance of the Gaussian model


def _seqs(a):
    return dict(R.seqs(a), quad=sorted(set(make_seq(1000, 12, "quad"))))


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 2, 5, 16])
@pytest.mark.parametrize("kind", ["uniform", "quad", "logsnr", "single", "offset"])
def test_coefficient_table(kind, iters):
    a = MH.alphas()
    seq = _seqs(a)[kind]
    c = invert_coefficients(seq, a, iters)
    assert c.dtype == np.float64 and c.shape == (len(seq) * iters, _lib.DDIMX_INVERT_STRIDE) and _lib.DDIMX_INVERT_STRIDE == 6
    assert np.isfinite(c).all()
    first = c[:, 5].reshape(len(seq), iters)
    assert (first[:, 0] == 1.0).all() and (first[:, 1:] == 0.0).all()
    lv = c.reshape(len(seq), iters, 6)
    assert (lv[:, :, :5] == lv[:, :1, :5]).all(), "the rows of a level differ in `first` only"
    assert lv[:, 0, 0].tolist() == [float(t) for t in seq], "levels upwards, the timestep of the level being solved for"
    # columns against an independent formation: alpha / sigma of solver_ref.levels (decoder order: reversed seq, then a = 1)
    al, sg, _ = R.levels(seq, a)
    al, sg = al[::-1], sg[::-1]  # the data, then seq upwards
    for k in range(len(seq)):
        _, s1, s2, p, q, _ = lv[k, 0]
        assert abs(s1 - sg[k + 1]) <= 1e-15 and abs(s2 - al[k + 1]) <= 1e-15
        assert abs(p - al[k + 1] / al[k]) <= 4e-16 * p
        assert abs(q - (sg[k + 1] - al[k + 1] / al[k] * sg[k])) <= 1e-15
    # s1, s2 are ddim_coefficients' (the x0 prediction is ddim_update's), in the opposite order
    d = ddim_coefficients(seq, a, 0.0)[::-1]
    assert np.array_equal(lv[:, 0, 1], d[:, 1]) and np.array_equal(lv[:, 0, 2], d[:, 2])
    # a level that starts from the data: p = s2, q = s1 exactly
    assert lv[0, 0, 3] == lv[0, 0, 2] and lv[0, 0, 4] == lv[0, 0, 1]


def test_row_is_the_inverse_of_the_decoder_step():
    """x_i = p x_j + q e put through the decoder's row for i -> j with the same e gives x_j back."""
    a = MH.alphas()
    seq = logsnr_seq(a, 20)
    inv = invert_coefficients(seq, a, 1)
    dec = ddim_coefficients(seq, a, 0.0)[::-1]
    xj, e = 0.7, -1.3
    for k in range(len(seq)):
        _, s1, s2, p, q, _ = inv[k]
        _, d1, d2, s3, c2, _ = dec[k]
        xi = p * xj + q * e
        back = s3 * (xi - d1 * e) / d2 + c2 * e
        assert abs(back - xj) <= 1e-14 * (abs(xj) + abs(e))


# ---- 2. table form = restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("model", ["gaussian", "tanh"])
@pytest.mark.parametrize("kind", ["uniform", "logsnr", "offset"])
def test_table_trajectory_equals_restatement(kind, model, iters):
    a = MH.alphas()
    seq = _seqs(a)[kind]
    fn = R.gaussian_model(a, VAR) if model == "gaussian" else R.tanh_model(a)
    x = np.linspace(-2.0, 2.0, 9)
    want_xs, want_p, want_r = IR.invert_steps(x, seq, fn, a, iters)
    xs, ps, rs = IR.table_steps(x, invert_coefficients(seq, a, iters), fn)
    assert len(xs) == len(seq) * iters + 1 and rs.shape == (len(seq) * iters, 9)
    worst = 0.0
    for k in range(len(seq)):
        row = (k + 1) * iters  # after the level's last iteration
        for got, want in ((xs[row], want_xs[k + 1]), (ps[row - 1], want_p[k])):
            worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    # residuals are differences of nearby iterates: relative to the iterates they come from
    rworst = float(np.abs(rs.reshape(len(seq), iters, 9) - want_r).max())
    print(f"[table vs restatement {kind} {model} iters {iters}] worst relative difference {worst:.2e}, residuals {rworst:.2e}")
    assert worst <= 1e-12 and rworst <= 1e-12


# ---- 3. the round trip contracts with iters ----------------------------------------------------------------------------------------
def test_round_trip_contracts_with_iters():
    a = MH.alphas()
    seq = make_seq(1000, 50)
    e = {k: IR.round_trip_error(seq, a, VAR, k) for k in (1, 2, 3, 4, 5, 8)}
    for k, v in sorted(e.items()):
        print(f"[round trip fp64] uniform 50 steps, iters {k}: {v:.3e}")
    for k in (1, 2, 3):
        assert e[k + 1] <= e[k] / 5, (k, e[k], e[k + 1])
    assert e[8] <= 1e-6
    coarse = make_seq(1000, 10)
    c1, c8 = IR.round_trip_error(coarse, a, VAR, 1), IR.round_trip_error(coarse, a, VAR, 8)
    print(f"[round trip fp64] uniform 10 steps, iters 1: {c1:.3e}, iters 8: {c8:.3e}")
    assert c8 <= c1 / 100
    # the table form gives the same figures
    tab = lambda x, s, fn, al, it: IR.table_steps(x, invert_coefficients(s, al, it), fn)  # noqa: E731
    assert abs(IR.round_trip_error(seq, a, VAR, 3, steps=tab) - e[3]) <= 1e-9 * e[3] + 1e-15


# ---- 4. first order against the closed form ----------------------------------------------------------------------------------------
def test_inverse_is_first_order():
    a = MH.alphas()
    grids = {"uniform": lambda n: make_seq(1000, n), "logsnr": lambda n: logsnr_seq(a, n)}
    for name, grid in grids.items():
        e = {n: IR.latent_error(grid(n), a, VAR, 8) for n in (25, 50, 100)}
        print(f"[latent vs closed form fp64] {name} grid, iters 8: " + ", ".join(f"{n}: {v:.3e}" for n, v in e.items())
              + f"; ratios {e[25] / e[50]:.3f}, {e[50] / e[100]:.3f}")
        assert 1.6 <= e[25] / e[50] <= 2.5
        assert 1.6 <= e[50] / e[100] <= 2.5


# ---- 5. slerp restatement ----------------------------------------------------------------------------------------------------------
def test_slerp_restatement():
    rng = np.random.default_rng(3)
    z1, z2 = rng.standard_normal((2, 2, 8, 16)), rng.standard_normal((2, 2, 8, 16))
    w = np.arange(0.0, 1.01, 0.1).astype(np.float32).astype(np.float64)
    w[-1] = 1.0
    out = IR.slerp(z1, z2, w)
    assert out.shape == (2, 11, 2, 8, 16)
    assert np.array_equal(out[:, 0], z1) and np.array_equal(out[:, -1], z2), "w = 0 / 1 return the inputs"
    # equal norms: the interpolant stays on the sphere
    z2n = z2 * (np.sqrt((z1 ** 2).sum(axis=(1, 2, 3))) / np.sqrt((z2 ** 2).sum(axis=(1, 2, 3))))[:, None, None, None]
    on = IR.slerp(z1, z2n, w)
    norms = np.sqrt((on ** 2).sum(axis=(2, 3, 4)))
    assert np.abs(norms / norms[:, :1] - 1.0).max() <= 1e-12
    # the straight-line fallback: identical, parallel and all-zero inputs
    for u, v in ((z1, z1), (z1, 2.0 * z1), (np.zeros_like(z1), z2), (z1, np.zeros_like(z1))):
        line = IR.slerp(u, v, w)
        assert np.isfinite(line).all()
        want = (1.0 - w)[None, :, None, None, None] * u[:, None] + w[None, :, None, None, None] * v[:, None]
        assert np.array_equal(line, want)
    # against the reference's formula where it is finite
    th = np.arccos((z1[0] * z2[0]).sum() / (np.linalg.norm(z1[0]) * np.linalg.norm(z2[0])))
    want = np.sin((1 - w[3]) * th) / np.sin(th) * z1[0] + np.sin(w[3] * th) / np.sin(th) * z2[0]
    assert np.abs(out[0, 3] - want).max() <= 1e-13


# ---- 6. validation -----------------------------------------------------------------------------------------------------------------
def _call(**kw):
    x = kw.pop("x", torch.zeros(2, 2, 16, 32))
    seq = kw.pop("seq", [0, 300, 600])
    # the model is never reached: validation comes before any device work (None would fail at the first forward)
    return D.invert_steps(x, seq, None, MH.alphas(), None, **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(iters=0), "iters"),
    (dict(iters=17), "iters"),
    (dict(iters=2.5), "iters"),
    (dict(iters=True), "iters"),
    (dict(iters="2"), "iters"),
    (dict(seq=[]), "empty"),
    (dict(seq=[0, 300, 300]), "increasing"),
    (dict(seq=[0, 600, 300]), "increasing"),
    (dict(seq=[0, 300, 1000]), "0..999"),
    (dict(seq=[-1, 300]), "0..999"),
    (dict(seq=[0, 300.5]), "integers"),
    (dict(x=torch.zeros(2, 16, 32)), "[B, C, T, F]"),
    (dict(x=torch.zeros(1, 1, 3, 3)), "multiple of 4"),
    (dict(x=torch.zeros(2, 1, 3, 6)), "multiple of 4"),
    (dict(stats=[]), "stats"),
])
def test_invalid_arguments_raise_before_device_work(kw, msg):
    with pytest.raises(ValueError) as e:
        _call(**kw)
    assert msg in str(e.value)


@pytest.mark.parametrize("bad_iters", [0, 17, 2.5, True, "2"])
def test_iters_is_checked_before_anything_else(bad_iters):
    with pytest.raises(ValueError, match="iters"):
        invert_coefficients([], MH.alphas(), bad_iters)


def test_shape_must_match_the_model():
    m = D.Model(configs.tiny_config("torch.FloatTensor"))  # F = 32, C = 2, three levels; never leaves the CPU
    for shape, msg in (((2, 2, 16, 64), "does not match the model"), ((2, 2, 10, 32), "multiple of 4 for this model")):
        with pytest.raises(ValueError) as e:
            D.invert_steps(torch.zeros(shape), [0, 300, 600], m, MH.alphas(), None)
        assert msg in str(e.value)


@pytest.mark.parametrize("z1,z2,w,msg", [
    (torch.zeros(2, 2, 8, 16), torch.zeros(2, 2, 8, 32), [0.5], "differ"),
    (torch.zeros(2, 2, 8, 16), torch.zeros(3, 2, 8, 16), [0.5], "differ"),
    (torch.zeros(2, 8, 16), torch.zeros(2, 8, 16), [0.5], "[P, C, T, F]"),
    (torch.zeros(2, 2, 8, 16), torch.zeros(2, 2, 8, 16), [], "weights"),
    (torch.zeros(2, 2, 8, 16), torch.zeros(2, 2, 8, 16), [[0.5]], "weights"),
    (torch.zeros(2, 2, 8, 16), torch.zeros(2, 2, 8, 16), [0.5, float("nan")], "finite"),
    (torch.zeros(2, 2, 8, 16), torch.zeros(2, 2, 8, 16), [float("inf")], "finite"),
    (torch.zeros(2, 1, 3, 6), torch.zeros(2, 1, 3, 6), [0.5], "multiple of 4"),
    (torch.zeros(0, 2, 8, 16), torch.zeros(0, 2, 8, 16), [0.5], "pairs"),
])
def test_slerp_invalid_arguments_raise_before_device_work(z1, z2, w, msg):
    with pytest.raises(ValueError) as e:
        D.slerp(z1, z2, w)  # CPU tensors on a box without a GPU: any device work would raise something else
    assert msg in str(e.value)
