"""Windowed inpainting without a GPU (ddim_audio_amd.windowed_inpaint_steps, include/ddimx_window_inpaint.h).

The seventh header: bound as WINDOW_INPAINT_EXPORTS with the signatures parsed from it, beside the unchanged lists of the six
others, and every refusal of its three functions (which needs no device).  The decomposition the kernels compute -- k1 / k2, the
seed of a window weighted with the blend's weights, the overlap-add of the windows' input gradients -- against plain autograd through
gather -> per-window model -> blend -> loss in fp64, on windows that use different nonlinear models.  The restatement
(tests/window_inpaint_ref.py) where it reduces to the two older ones.  Arguments: every check raises before the library is loaded
or a stepper's device state is built."""
import ctypes
import types

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, sampler
from ddim_audio_amd.schedule import inpaint_coefficients, window_plan
import inpaint_ref
import model_harness as MH
import window_inpaint_ref as WI
import window_ref as WR


# ---- 1. the seventh header ---------------------------------------------------------------------------------------------------------------
def test_seventh_header_is_bound_and_refuses_before_any_launch():
    assert _lib.WINDOW_INPAINT_EXPORTS == ("ddimxwi_partials_floats", "ddimxwi_residual", "ddimxwi_update")
    assert len(_lib.EXPORTS) == 151 and all(n.startswith("ddimx_") for n in _lib.EXPORTS)
    assert _lib.WINDOW_EXPORTS == ("ddimxw_multistep_update", "ddimxw_blend")
    assert _lib.SDE_EXPORTS == ("ddimxs_multistep_update",) and _lib.BROWNIAN_EXPORTS == ("ddimxb_multistep_update", "ddimxb_path_fill")
    assert _lib.DISTILL_EXPORTS == ("ddimxd_sqerr_loss_w", "ddimxd_sqerr_loss_w_bwd_mean", "ddimxd_distill_half", "ddimxd_distill_target")
    assert _lib.THRESHOLD_EXPORTS == ("ddimxq_quantile_work_bytes", "ddimxq_x0_quantile", "ddimxq_threshold_eps")
    assert _lib.DDIMX_ABI_VERSION == 2 and _lib.DDIMX_WINDOW_MAX_COVER == 8
    assert (_lib.DDIMX_INPAINT_REPLACE, _lib.DDIMX_INPAINT_GUIDED, _lib.DDIMX_INPAINT_STRIDE) == (1, 2, 9)
    lib = _lib.load()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    parts, res, upd = lib.ddimxwi_partials_floats, lib.ddimxwi_residual, lib.ddimxwi_update  # resolve in the built library
    assert parts.restype is LL and list(parts.argtypes) == [I, LL]
    assert res.restype is I and list(res.argtypes) == [P] * 13 + [I] * 7 + [P]
    assert upd.restype is I and list(upd.argtypes) == [P] * 13 + [I] * 8 + [P]
    assert D.windowed_inpaint_steps.__module__ == "ddim_audio_amd.window_inpaint"
    # the partials: inpaint_residual_kernel's count for a sample of C L F elements
    for n, per in ((1, 2 * 48 * 4), (3, 4 * 5132), (2, 4 * 256 * 3000), (65535, 8)):
        assert parts(n, per) == lib.ddimx_inpaint_partials_floats(n, per) > 0 and parts(n, per) % n == 0
    for n, per in ((0, 8), (65536, 8), (1, 0), (1, 6), (1, -4)):
        assert parts(n, per) == -1
    p = ctypes.c_void_p(256)  # never dereferenced: every argument is checked before the launch
    geometry = [({0: 0}, "N = 0"), ({1: 0}, "W = 0"), ({0: 30000}, "N W in 1..65535"), ({2: 0}, "C = 0"), ({3: 65}, "L = 65"),
                ({5: 0}, "H = 0"), ({3: 66, 5: 33}, "H = 33"), ({6: 6}, "F = 6"), ({6: 0}, "F = 0"), ({4: 0}, "T = 0"),
                ({3: 32 + 2 * 3, 5: 3}, "cover")]
    dims = [2, 3, 2, 64, 32, 16, 8]  # N, W, C, L, T, H, F
    #       x  eps y  mask x0 beps seed partials jf cnt wt coef step | dims | stream
    good = [p, p, p, p, p, p, p, p, p, p, p, p, p] + dims + [None]
    bad = ([({k: None}, "null") for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12)] + [({10: None}, "need wt")]
           + [({k + 13: v for k, v in edit.items()}, msg) for edit, msg in geometry])
    for edit, msg in bad:
        args = [edit.get(k, v) for k, v in enumerate(good)]
        assert res(*args) != 0, msg
        err = lib.ddimx_last_error().decode()
        assert "ddimxwi_residual" in err and msg in err, (msg, err)
    #       x  eps noise x0 y  mask d_win partials jf cnt wt coef step | dims | flags stream
    good = [p, p, None, p, p, p, p, p, p, p, p, p, p] + dims + [3, None]
    bad = ([({k: None}, "null") for k in (0, 1, 3, 8, 9, 11, 12)] + [({10: None}, "need wt")]
           + [({k + 13: v for k, v in edit.items()}, msg) for edit, msg in geometry]
           + [({20: 4}, "unknown flags"), ({20: -1}, "unknown flags"), ({4: None}, "need y and mask"), ({5: None, 20: 1}, "need y and mask"),
              ({4: None, 20: 2}, "need y and mask"), ({6: None}, "needs d_win and partials"), ({7: None, 20: 2}, "needs d_win and partials")])
    for edit, msg in bad:
        args = [edit.get(k, v) for k, v in enumerate(good)]
        assert upd(*args) != 0, msg
        err = lib.ddimx_last_error().decode()
        assert "ddimxwi_update" in err and msg in err, (msg, err)


# ---- 2. the decomposition against autograd ----------------------------------------------------------------------------------------------
SHAPE, T, H = (2, 2, 48, 4), 16, 8  # W = 5, K = 2


def _models(dtype=torch.float64):
    """Five windows, five different nonlinear models; each couples a window's rows and channels, so its Jacobian is not diagonal."""
    gen = torch.Generator().manual_seed(12)
    A = [0.3 * torch.randn(T, T, generator=gen, dtype=dtype) for _ in range(5)]
    gain = [0.6, -0.9, 1.3, 0.4, -1.1]

    def fn(win, t, j):
        mixed = torch.einsum("ts,ncsf->nctf", A[j], win) + 0.25 * win.flip(1)
        return gain[j] * torch.tanh(mixed + 0.1 * j) + 0.05 * win * win + 0.002 * float(t[0]) / 1000.0
    return fn


def _soft_mask(shape, dtype=torch.float64):
    n, c, length, f = shape
    m = torch.ones(n, 1, length, f, dtype=dtype)
    m[:, :, length // 4: length // 2] = 0
    m[:, :, :, -1:] *= 0.5
    m[-1, :, : length // 8] = 0.25
    return m


@pytest.mark.parametrize("table", ["double", "fp32"])
@pytest.mark.parametrize("taper", ["flat", "tri"])
@pytest.mark.parametrize("prediction", ["eps", "v"])
def test_decomposition_equals_autograd_fp64(prediction, taper, table):
    """g = k2 m r + sum over the covering windows of J_j^T (wt_j k1 m r), with k1 / k2 from the table the kernels read and the
    windows, their order and their count from the plan the kernels read, against ``torch.autograd.grad`` through the restatement.
    eps: 1e-12 relative.  v: the table's k2 = 2 s2 stands for the exact 2 (1 - s1^2) / s2 (x0 = ((1 - s1^2) x - s1 s2 v) / s2), which
    it is only as far as s1^2 + s2^2 = 1 holds for the table's doubles; the difference, per element, is
    2 |s1^2 + s2^2 - 1| / s2 |m r|, and that is the bound on top of the 1e-12.  ``table`` "fp32": s1 and s2 as the device table
    holds them, rounded to fp32, with k1 / k2 formed from them by ``inpaint_coefficients``' expressions -- s1^2 + s2^2 then misses 1
    by about 1e-7, which the bound follows."""
    a = MH.alphas()
    fn = _models()
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    y = torch.randn(SHAPE, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    m = torch.broadcast_to(_soft_mask(SHAPE), SHAPE)
    y = y * (m != 0)
    row = inpaint_coefficients([0, 300, 700], a, 0.0, 0.5, prediction)[1]
    if table == "fp32":
        row[1], row[2] = float(np.float32(row[1])), float(np.float32(row[2]))
        row[6], row[7] = (-2.0 * row[1], 2.0 * row[2]) if prediction == "v" else (-2.0 * row[1] / row[2], 2.0 / row[2])
    ti, s1, s2, k1, k2 = int(row[0]), row[1], row[2], row[6], row[7]
    _, x0_ref, L_ref, g_auto = WI.step(fn, x, row[:6], 0.5, y, m, T, H, taper, True, False, prediction=prediction)
    # the kernels' way: plan tables (the weights formed as the plan forms them, in float64 and not yet rounded to fp32)
    p = window_plan(SHAPE[2], T, H, taper)
    assert p.W == 5 and p.K == 2
    wd = WI.taper_weights(T, taper, torch.float64)
    w64 = torch.zeros(p.K, SHAPE[2], dtype=torch.float64)
    for l in range(SHAPE[2]):
        for k in range(int(p.cnt[l])):
            w64[k, l] = wd[l - (int(p.jfirst[l]) + k) * H]
    w64 = w64 / w64.sum(0)
    assert np.array_equal(w64.numpy().astype(np.float32), p.wt), "the plan's fp32 weights are these, rounded once"
    tt = torch.full((SHAPE[0],), ti, dtype=torch.long)
    wins = [x[:, :, j * H:j * H + T].clone().requires_grad_(True) for j in range(p.W)]
    outs = [fn(wins[j], tt, j) for j in range(p.W)]                                          # the network's output: eps or v
    eps = [s1 * wins[j].detach() + s2 * outs[j].detach() if prediction == "v" else outs[j].detach() for j in range(p.W)]
    e = torch.zeros(SHAPE, dtype=torch.float64)
    for l in range(SHAPE[2]):
        for k in range(int(p.cnt[l])):
            j = int(p.jfirst[l]) + k
            e[:, :, l] += w64[k, l] * eps[j][:, :, l - j * H]
    x0 = (x - s1 * e) / s2
    assert torch.allclose(x0, x0_ref, rtol=1e-13, atol=1e-13)
    r = m * (x0 - y)
    assert torch.allclose(r.square().flatten(1).sum(1), L_ref, rtol=1e-13, atol=0)
    s = k1 * (m * r)                                                                         # the canvas seed
    g = k2 * (m * r)
    d_win = []
    for j in range(p.W):
        seed = torch.zeros_like(wins[j])
        for tau in range(T):
            l = j * H + tau
            k = j - int(p.jfirst[l])
            assert 0 <= k < int(p.cnt[l]), "a window row's canvas row is covered by that window"
            seed[:, :, tau] = s[:, :, l] if int(p.cnt[l]) == 1 else w64[k, l] * s[:, :, l]
        (d,) = torch.autograd.grad(outs[j], wins[j], seed)
        d_win.append(d)
    for l in range(SHAPE[2]):
        j0 = int(p.jfirst[l])
        acc = d_win[j0][:, :, l - j0 * H]
        for k in range(1, int(p.cnt[l])):
            acc = acc + d_win[j0 + k][:, :, l - (j0 + k) * H]
        g[:, :, l] += acc
    scale = float(g_auto.abs().max())
    share = 2.0 * abs(s1 * s1 + s2 * s2 - 1.0) / s2 * (m * r).abs() if prediction == "v" else torch.zeros_like(g)
    err = (g - g_auto).abs()
    print(f"[windowed inpaint decomposition {prediction} {taper} {table}] max error {float(err.max()) / scale:.2e} of max |g|; "
          f"the table's share of the bound at most {float(share.max()) / scale:.2e}")
    assert bool((err <= 1e-12 * scale + share).all()), float((err - share).max()) / scale
    assert float(g_auto.abs().max()) > 0 and float((g - k2 * (m * r)).abs().max()) > 1e-3 * scale, "the network term matters"


# ---- 3. the restatement where it reduces to the older ones ----------------------------------------------------------------------------------
@pytest.mark.parametrize("guidance", [0.0, [0.2, 0.3, 0.0]], ids=["replace_only", "guided"])
def test_one_window_restatement_is_inpaint_ref(guidance):
    a = MH.alphas()
    fn = _models()
    shape = (2, 2, T, 4)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    y = torch.randn(shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    m = _soft_mask(shape)
    seq = [0, 400, 800]
    z = torch.randn((3,) + shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    for taper in ("flat", "tri"):
        xs, x0 = WI.windowed_inpaint_steps(x, seq, fn, a, T, T, taper, y, m, guidance, True, eta=0.5, noise_fn=lambda i, xt: z[i])
        rxs, rx0 = inpaint_ref.inpaint_steps(x, seq, lambda w, t: fn(w, t, 0), a, y, m, guidance, True, eta=0.5, noise_fn=lambda i, xt: z[i])
        for i in range(3):
            assert torch.allclose(xs[i + 1], rxs[i + 1], rtol=1e-12, atol=1e-12) and torch.allclose(x0[i], rx0[i], rtol=1e-12, atol=1e-12), i
    assert not torch.equal(xs[-1], x)


@pytest.mark.parametrize("replace", [True, False])
@pytest.mark.parametrize("taper", ["flat", "tri"])
def test_empty_mask_restatement_is_window_ref(taper, replace):
    a = MH.alphas()
    fn = _models()
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    y = torch.randn(SHAPE, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    seq = [0, 400, 800]
    z = torch.randn((3,) + SHAPE, generator=torch.Generator().manual_seed(10), dtype=torch.float64)
    xs, x0 = WI.windowed_inpaint_steps(x, seq, fn, a, T, H, taper, y, torch.zeros(1, 1, 1, 1), 0.0, replace, eta=0.5,
                                       noise_fn=lambda i, xt: z[i])
    tt = torch.zeros(SHAPE[0], dtype=torch.long)
    np_fn = lambda w, t, j: fn(torch.from_numpy(w), tt + int(t), j).numpy()  # noqa: E731
    rxs, rx0 = WR.windowed_steps(x.numpy(), seq, np_fn, a, T, H, taper, eta=0.5, noise_fn=lambda k, xx: z[k].numpy())
    for i in range(3):
        assert np.allclose(xs[i + 1].numpy(), rxs[i + 1], rtol=1e-12, atol=1e-12) and np.allclose(x0[i].numpy(), rx0[i], rtol=1e-12, atol=1e-12), i


# ---- 4. arguments ---------------------------------------------------------------------------------------------------------------------------
class _Net:
    """What the argument checks read of a ``ddim_audio_amd.Model``: its config and that it is one (``forward_slot``)."""
    prediction = "eps"
    config = types.SimpleNamespace(channels=2, f_size=32, ch=[8, 8, 8])  # T must be a multiple of 4

    def forward_slot(self, *a, **k):
        raise AssertionError("the network was called")


def test_argument_errors_raise_before_the_library_is_loaded(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "stream", no_library)
    monkeypatch.setattr(sampler.DDIMStepper, "__init__", lambda *a, **k: pytest.fail("a stepper's device state was built"))
    a = MH.alphas()
    net, fn = _Net(), (lambda x, t: x)  # noqa: E731  (never called)
    seq = list(range(0, 1000, 100))
    x = torch.zeros(2, 2, 128, 32)
    base = dict(y=torch.zeros(2, 2, 128, 32), mask=torch.ones(2, 1, 128, 1))

    def run(xx=x, s=seq, m=net, **kw):
        args = dict(base, window=64)
        args.update(kw)
        return D.windowed_inpaint_steps(xx, s, m, a, None, **args)

    # windowed_steps' checks: the canvas, the geometry, the model
    for kw, word in [(dict(hop=0), "hop"), (dict(hop=65), "hop"), (dict(hop=7), "hop"), (dict(hop=48), "L"), (dict(window=256), "L"),
                     (dict(window=66, hop=31), "window"), (dict(window=0), "window"), (dict(window=64.0), "window"),
                     (dict(window=True), "window"), (dict(hop=32.0), "hop"), (dict(hop=32, taper="cos"), "taper"),
                     (dict(eta=-0.5), "eta"), (dict(eta=float("nan")), "eta")]:
        with pytest.raises(ValueError, match=word):
            run(**kw)
    with pytest.raises(ValueError, match="model"):
        run(torch.zeros(2, 2, 128, 16))
    with pytest.raises(ValueError, match="model"):
        run(torch.zeros(2, 3, 128, 32))
    with pytest.raises(ValueError, match=r"\[N, C, L, F\]"):
        run(torch.zeros(2, 128, 32))
    with pytest.raises(ValueError, match="no canvas sample"):
        run(torch.zeros(0, 2, 128, 32))
    with pytest.raises(ValueError, match="multiple of 4"):
        run(torch.zeros(2, 2, 128, 6), m=fn)
    with pytest.raises(ValueError, match="65535"):
        run(torch.zeros(300, 1, 8 + 299 * 1, 4), m=fn, window=8, hop=1)  # N W = 300 x 300
    with pytest.raises(ValueError, match="seq is empty"):
        run(s=[])
    with pytest.raises(ValueError, match="prediction"):
        run(prediction="x0")
    for bad in (torch.Generator(), torch.randn_like, 7):
        with pytest.raises(TypeError, match="NoiseStream"):
            run(eta=1.0, noise=bad)
    # inpaint_steps' checks, against the CANVAS
    for kw, word in [(dict(mask=torch.ones(2, 2, 128, 3)), "broadcast"), (dict(mask=torch.ones(3, 1, 1, 1)), "broadcast"),
                     (dict(mask=torch.ones(2, 1, 64, 1)), "broadcast"), (dict(y=torch.zeros(2, 2, 64, 32)), "broadcast"),
                     (dict(y=torch.zeros(2, 2, 128, 32, 1)), "broadcast"), (dict(mask=torch.full((1, 1, 1, 32), 1.5)), r"\[0, 1\]"),
                     (dict(mask=torch.full((1, 1, 1, 32), float("nan"))), r"\[0, 1\]"),
                     (dict(mask=torch.full((1, 1, 1, 32), 2, dtype=torch.int64)), r"\[0, 1\]"),
                     (dict(mask=torch.ones(1, 1, 1, 1, dtype=torch.complex64)), "mask must be"),
                     (dict(y=torch.zeros(1, 1, 1, 1, dtype=torch.int32)), "floating-point"),
                     (dict(guidance=-1.0), "guidance"), (dict(guidance=float("inf")), "guidance"), (dict(guidance=[1.0, 2.0]), "guidance"),
                     (dict(mask=None), "windowed_inpaint_steps needs"), (dict(y=None), "y=")]:
        with pytest.raises(ValueError, match=word):
            run(**kw)
    for kw in (dict(y=np.zeros((2, 2, 128, 32))), dict(mask=[1.0])):
        with pytest.raises(TypeError, match="must be a tensor"):
            run(**kw)
    # guidance needs the tape-keeping forward and the data-only backward: a Model
    with pytest.raises(RuntimeError, match="needs a ddim_audio_amd.Model"):
        run(m=fn, guidance=0.3)
    with pytest.raises(RuntimeError, match="needs a ddim_audio_amd.Model"):
        run(m=fn, guidance=[0.0] * 9 + [0.1])


def test_stepper_refuses_before_its_device_state_is_built(monkeypatch):
    from ddim_audio_amd.window_inpaint import WindowInpaintStepper
    monkeypatch.setattr(sampler.DDIMStepper, "__init__", lambda *a, **k: pytest.fail("a stepper's device state was built"))
    a = MH.alphas()
    seq = list(range(0, 1000, 100))
    fn = lambda x, t: x  # noqa: E731
    x = torch.zeros(2, 2, 128, 32)
    coef = inpaint_coefficients(seq, a, 0.0, 0.3)
    with pytest.raises(ValueError, match="hop"):
        WindowInpaintStepper(fn, x, x, x, coef, False, True, 64, 7)
    with pytest.raises(ValueError, match="L"):
        WindowInpaintStepper(fn, x, x, x, coef, False, True, 96, 48)
    with pytest.raises(ValueError, match=r"\[N, C, L, F\]"):
        WindowInpaintStepper(fn, x[0], x[0], x[0], coef, False, True, 64)
    with pytest.raises(RuntimeError, match="needs a ddim_audio_amd.Model"):
        WindowInpaintStepper(fn, x, x, x, coef, True, True, 64)
    with pytest.raises(pytest.fail.Exception, match="device state"):
        WindowInpaintStepper(fn, x, x, x, coef, False, True, 64)
