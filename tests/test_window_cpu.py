"""Windowed long-form sampler, host side (no GPU, no library): the plan tables the kernel reads against a brute-force
enumeration, the float64 restatement (tests/window_ref.py, written from the definition and not from those tables) against plain
DDIM of the whole canvas for a model that does not know its window, against the hand-written blend for one that does, and
argument validation before any device work."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd.schedule import make_seq, window_plan

import model_harness as MH
import solver_ref as S
import window_ref as R

T = 32
HOPS = [32, 16, 12, 8, 5, 4]
TAPERS = ["flat", "tri"]
F = 4
REL = 1e-12  # float64 agreement of two orders of the same arithmetic; the margin is for other BLAS / libm builds


def _covering(L, H):
    """Brute force: for every canvas row the windows that cover it, ascending."""
    W = (L - T) // H + 1
    return [[j for j in range(W) if j * H <= row < j * H + T] for row in range(L)]


def _exact_weights(L, H, taper):
    """Per row the float64 normalised weights of its covering windows, from the taper's definition."""
    w = (lambda tau: 1.0) if taper == "flat" else (lambda tau: float(min(tau + 1, T - tau)))
    out = []
    for row, js in enumerate(_covering(L, H)):
        raw = [w(row - j * H) for j in js]
        out.append([v / sum(raw) for v in raw])
    return out


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# ---- 1. the plan ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("H", HOPS)
def test_plan_against_brute_force(H, taper):
    L = T + 3 * H
    p = window_plan(L, T, H, taper)
    cover = _covering(L, H)
    assert p.W == 4 and p.K == -(-T // H) and max(len(js) for js in cover) == min(p.K, p.W)
    assert p.jfirst.dtype == np.int32 and p.cnt.dtype == np.int32 and p.wt.dtype == np.float32
    assert p.jfirst.shape == (L,) and p.cnt.shape == (L,) and p.wt.shape == (p.K, L)
    assert p.jfirst.tolist() == [js[0] for js in cover]
    assert p.cnt.tolist() == [len(js) for js in cover]
    assert all(js == list(range(js[0], js[0] + len(js))) for js in cover), "the covering windows are consecutive"
    exact = _exact_weights(L, H, taper)
    worst = 0.0
    for row in range(L):
        n = int(p.cnt[row])
        col = p.wt[:, row]
        assert (col[n:] == 0).all(), "zero beyond cnt"
        assert np.array_equal(col[:n], np.asarray(exact[row], dtype=np.float64).astype(np.float32)), "float64, rounded once"
        s = float(col.astype(np.float64).sum())
        worst = max(worst, abs(s - 1.0))
        if n == 1:
            assert col[0] == 1.0
    print(f"[window plan T {T} H {H} {taper}] max |sum of fp32 weights - 1| = {worst / 2.0 ** -24:.3f} x 2^-24")
    assert worst <= 2.0 ** -24
    if taper == "tri":
        for row in range(L):
            n = int(p.cnt[row])
            assert p.cnt[L - 1 - row] == n
            assert np.array_equal(p.wt[:n, row], p.wt[:n, L - 1 - row][::-1]), "symmetric under l -> L - 1 - l"


def test_default_hop_is_half_a_window_and_one_window_is_all_ones():
    p = window_plan(T, T, 16, "tri")
    assert p.W == 1 and p.K == 2 and (p.cnt == 1).all() and (p.jfirst == 0).all() and (p.wt[0] == 1.0).all() and (p.wt[1] == 0).all()
    p = window_plan(3 * T, T, T, "tri")
    assert p.W == 3 and p.K == 1 and (p.cnt == 1).all() and p.jfirst.tolist() == [r // T for r in range(3 * T)] and (p.wt == 1.0).all()


@pytest.mark.parametrize("args,word", [
    ((64, 32, 0, "tri"), "hop"), ((64, 32, 33, "tri"), "hop"), ((64, 32, 3, "tri"), "hop"),    # K = 11 > 8
    ((65, 32, 16, "tri"), "L"), ((16, 32, 16, "tri"), "L"), ((64, 0, 16, "tri"), "window"),
    ((64, 32, 16, "hann"), "taper"), ((64, 32, 16.0, "tri"), "hop"), ((64, True, 16, "tri"), "window"), ((64.0, 32, 16, "tri"), "L"),
])
def test_plan_argument_errors(args, word):
    with pytest.raises(ValueError, match=word):
        window_plan(*args)


def test_windowed_steps_argument_errors_before_any_device_work():
    a = MH.alphas()
    seq = make_seq(1000, 5)
    model = lambda x, t: x  # noqa: E731  (never called: everything below raises first, on CPU tensors, without the library)
    x = torch.zeros(1, 2, 96, 256)
    ok = dict(window=32, hop=16)
    for kw, word in [(dict(window=32, hop=0), "hop"), (dict(window=32, hop=33), "hop"), (dict(window=32, hop=3), "hop"),
                     (dict(window=32, hop=20), "L"), (dict(window=128), "L"), (dict(window=0), "window"), (dict(window=32.0), "window"),
                     (dict(ok, taper="hann"), "taper"), (dict(ok, eta=-1.0), "eta"), (dict(ok, eta=float("nan")), "eta")]:
        with pytest.raises(ValueError, match=word):
            D.windowed_steps(x, seq, model, a, None, **kw)
    with pytest.raises(ValueError, match="seq"):
        D.windowed_steps(x, [], model, a, None, **ok)
    with pytest.raises(ValueError, match="x"):
        D.windowed_steps(torch.zeros(2, 96, 256), seq, model, a, None, **ok)
    with pytest.raises(ValueError, match="x"):
        D.windowed_steps(torch.zeros(1, 2, 96, 6), seq, model, a, None, **ok)
    with pytest.raises(ValueError, match="65535"):
        D.windowed_steps(torch.zeros(9363, 1, 8 + 6 * 4, 4), seq, model, a, None, window=8, hop=4)  # 9363 x 7 = 65541 windows
    with pytest.raises(TypeError):
        D.windowed_steps(x, seq, model, a, None, noise=object(), **ok)
    with pytest.raises(TypeError):
        D.windowed_steps(x, seq, model, a, None, 32)  # window is keyword-only


# ---- 2. a model that does not know its window: plain DDIM of the whole canvas -----------------------------------------------------------
@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("H", HOPS)
def test_position_independent_model_is_plain_ddim(H, taper):
    a = MH.alphas()
    seq = make_seq(1000, 20)
    L = T + 3 * H
    x = np.random.default_rng(H).standard_normal((2, L, F))
    g = S.gaussian_model(a, 0.25)
    xs, x0s = R.windowed_steps(x, seq, lambda w, t, j: g(w, t), a, T, H, taper)
    want_xs, want_x0 = S.dpm_solver_steps(x, seq, g, a, 1)
    worst = max(_rel(u, v) for u, v in zip(xs, want_xs))
    # the x0 prediction (x - s1 eps) / s2 of this model cancels almost completely at high noise (x0 is 1e-3 of x at t = 950), so
    # two float64 evaluations agree relative to the operands of that subtraction, |x| / s2, not relative to its result
    s2 = np.sqrt(torch.as_tensor(a).double().numpy()[list(reversed(seq))])
    worst0 = max(float(np.abs(u - v).max() / (np.abs(xk).max() / s)) for u, v, xk, s in zip(x0s, want_x0, want_xs, s2))
    print(f"[windowed reference vs DDIM, T {T} H {H} {taper}] max relative difference: x {worst:.2e}, x0 {worst0:.2e}")
    assert len(xs) == 21 and len(x0s) == 20 and worst <= REL and worst0 <= REL


# ---- 3. a model that does: the hand-written blend ---------------------------------------------------------------------------------------
def _gains(W):
    return [0.2 + 0.6 * ((7 * j + 3) % 11) / 11.0 for j in range(W)]  # a different scalar per window, in 0.2 .. 0.8


@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("H", HOPS)
def test_window_dependent_model_is_the_hand_written_blend(H, taper):
    a = MH.alphas()
    seq = make_seq(1000, 20)
    L = T + 3 * H
    gj = _gains(4)
    assert len(set(gj)) == 4
    x = np.random.default_rng(100 + H).standard_normal((2, L, F))
    cover, exact = _covering(L, H), _exact_weights(L, H, taper)
    row_gain = np.array([sum(w * gj[j] for w, j in zip(exact[r], cover[r])) for r in range(L)])[:, None]  # sum_j w_j g_j per row
    got = R.blend(x, 500, lambda w, t, j: gj[j] * w, T, H, taper)
    assert _rel(got, row_gain * x) <= REL
    xs, x0s = R.windowed_steps(x, seq, lambda w, t, j: gj[j] * w, a, T, H, taper)
    want_xs, want_x0 = S.dpm_solver_steps(x, seq, lambda v, t: row_gain * v, a, 1)
    worst = max(max(_rel(u, v) for u, v in zip(xs, want_xs)), max(_rel(u, v) for u, v in zip(x0s, want_x0)))
    print(f"[windowed reference vs hand-written blend, T {T} H {H} {taper}] max relative difference {worst:.2e}")
    assert worst <= REL
    if H < T:
        assert not np.allclose(row_gain[:T], gj[0]), "the overlap really blends"


@pytest.mark.parametrize("taper", TAPERS)
def test_one_window_is_ddim_and_no_overlap_is_independent_runs(taper):
    a = MH.alphas()
    seq = make_seq(1000, 20)
    gj = _gains(3)
    x = np.random.default_rng(7).standard_normal((2, 3 * T, F))
    # W = 1: the DDIM reference of the one window
    one = x[:, :T]
    xs, x0s = R.windowed_steps(one, seq, lambda w, t, j: gj[j] * w, a, T, 16, taper)
    want_xs, want_x0 = S.dpm_solver_steps(one, seq, lambda v, t: gj[0] * v, a, 1)
    assert max(_rel(u, v) for u, v in zip(xs + x0s, want_xs + want_x0)) <= REL
    # H = T: W independent runs, one per segment with its own model
    xs, x0s = R.windowed_steps(x, seq, lambda w, t, j: gj[j] * w, a, T, T, taper)
    for j in range(3):
        seg = slice(j * T, (j + 1) * T)
        want_xs, want_x0 = S.dpm_solver_steps(x[:, seg], seq, lambda v, t, g=gj[j]: g * v, a, 1)
        assert max(_rel(u[:, seg], v) for u, v in zip(xs + x0s, want_xs + want_x0)) <= REL, j


def test_reference_noise_term():
    """eta > 0 in the reference: the canvas takes c1 z on top of the deterministic update (used by the GPU tests)."""
    a = MH.alphas()
    seq = make_seq(1000, 4)
    x = np.random.default_rng(3).standard_normal((1, 2 * T, F))
    z = np.random.default_rng(4).standard_normal((4,) + x.shape)
    f = lambda w, t, j: 0.5 * w  # noqa: E731
    det, _ = R.windowed_steps(x, seq, f, a, T, 16, "tri")
    sto, _ = R.windowed_steps(x, seq, f, a, T, 16, "tri", eta=1.0, noise_fn=lambda k, ref: z[k])
    from ddim_audio_amd.schedule import ddim_coefficients
    c1 = ddim_coefficients(seq, a, 1.0)[0, 5]
    c2 = ddim_coefficients(seq, a, 1.0)[0, 4]
    c2_det = ddim_coefficients(seq, a, 0.0)[0, 4]
    assert c1 > 0
    assert _rel(sto[1], det[1] + (c2 - c2_det) * 0.5 * x + c1 * z[0]) <= REL
