"""Windowed multistep sampling without a GPU (ddim_audio_amd.windowed_solver_steps, include/ddimx_window.h).

Arguments: every check of the two parents -- windowed_steps' canvas and geometry, dpm_solver_steps' order, tau, noise, prediction
and threshold -- raises before the library is loaded or a stepper's device state is built.  The sixth header: bound as
WINDOW_EXPORTS with the signatures parsed from it, beside 147 unchanged ddimx.h exports, and every refusal of the two functions
(which needs no device).  The references: the table's form over the blend equals the published update over the blend, and the
convergence experiment on a canvas whose windows disagree gives the documented table and the two conditions the GPU test repeats."""
import ctypes
import types

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, sampler
from ddim_audio_amd.schedule import X0Clip, brownian_plan, dpm_coefficients, logsnr_seq
import model_harness as MH
import solver_ref as R
import window_ref as WR
import window_solver_ref as WS


class _Net:
    """What the argument checks read of a ``ddim_audio_amd.Model``: its config and that it is one (``forward_slot``)."""
    prediction = "eps"
    config = types.SimpleNamespace(channels=2, f_size=32, ch=[8, 8, 8])  # T must be a multiple of 4

    def forward_slot(self, *a, **k):
        raise AssertionError("the network was called")


# ---- 1. arguments ---------------------------------------------------------------------------------------------------------------------
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
    ns, bs = D.NoiseStream(3), D.BrownianStream(3)
    run = lambda xx=x, s=seq, m=net, **kw: D.windowed_solver_steps(xx, s, m, a, None, **kw)  # noqa: E731
    # windowed_steps' checks: the canvas, the geometry, the model
    for kw, word in [(dict(window=64, hop=0), "hop"), (dict(window=64, hop=65), "hop"), (dict(window=64, hop=7), "hop"),
                     (dict(window=64, hop=48), "L"), (dict(window=256), "L"), (dict(window=66, hop=31), "window"),
                     (dict(window=0), "window"), (dict(window=64.0), "window"), (dict(window=True), "window"),
                     (dict(window=64, hop=32.0), "hop"), (dict(window=64, hop=32, taper="cos"), "taper")]:
        with pytest.raises(ValueError, match=word):
            run(**kw)
    with pytest.raises(ValueError, match="model"):
        run(torch.zeros(2, 2, 128, 16), window=64)
    with pytest.raises(ValueError, match="model"):
        run(torch.zeros(2, 3, 128, 32), window=64)
    with pytest.raises(ValueError, match=r"\[N, C, L, F\]"):
        run(torch.zeros(2, 128, 32), window=64)
    with pytest.raises(ValueError, match=r"\[N, C, L, F\]"):
        run(np.zeros((2, 2, 128, 32)), window=64)
    with pytest.raises(ValueError, match="no canvas sample"):
        run(torch.zeros(0, 2, 128, 32), window=64)
    with pytest.raises(ValueError, match="multiple of 4"):
        run(torch.zeros(2, 2, 128, 6), m=fn, window=64)
    with pytest.raises(ValueError, match="65535"):
        run(torch.zeros(300, 1, 8 + 299 * 1, 4), m=fn, window=8, hop=1)  # N W = 300 x 300
    with pytest.raises(ValueError, match="seq is empty"):
        run(s=[], window=64)
    # dpm_solver_steps' checks: order, tau, seq, noise, prediction, threshold
    for bad in (0, 4, 2.0, True, None):
        with pytest.raises(ValueError, match="order"):
            run(window=64, order=bad)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            run(window=64, tau=bad)
        with pytest.raises(ValueError, match="tau"):
            run(window=64, tau=bad, noise=ns)
    for bad, word in (([5, 5, 9], "strictly increasing"), ([9, 5], "strictly increasing"), ([0, 1000], "0..999"), ([0.5, 7], "integers")):
        with pytest.raises(ValueError, match=word):
            run(s=bad, window=64)
    for stream in (ns, bs):
        for tau in (0.0, 1.0):  # also where the stream would not be used
            with pytest.raises(ValueError, match="not both"):
                run(window=64, tau=tau, noise=stream, noise_fn=torch.randn_like)
    for bad in (torch.Generator(), torch.randn_like, 7):
        with pytest.raises(TypeError, match="NoiseStream"):
            run(window=64, tau=1.0, noise=bad)
    with pytest.raises(ValueError, match="prediction"):
        run(window=64, prediction="x0")
    for bad in (1.0, "clip", (1.0,)):
        with pytest.raises(ValueError, match="threshold"):
            run(window=64, threshold=bad)


def test_stepper_refuses_what_its_parents_refuse_before_its_device_state_is_built(monkeypatch):
    from ddim_audio_amd.window import WindowSolverStepper
    monkeypatch.setattr(sampler.DDIMStepper, "__init__", lambda *a, **k: pytest.fail("a stepper's device state was built"))
    a = MH.alphas()
    seq = logsnr_seq(a, 8)
    fn = lambda x, t: x  # noqa: E731
    x = torch.zeros(2, 2, 128, 32)
    c2, c3, s2 = dpm_coefficients(seq, a, 2), dpm_coefficients(seq, a, 3), dpm_coefficients(seq, a, 2, tau=1.0)
    with pytest.raises(ValueError, match="order = 3"):  # no hist buffer at order 2: a table with w2 != 0 is refused, as MultistepStepper does
        WindowSolverStepper(fn, x, c3, 2, 64)
    with pytest.raises(ValueError, match=r"\[n_iter, 8\]"):
        WindowSolverStepper(fn, x, c2[:, :6], 2, 64)
    with pytest.raises(ValueError, match="hop"):
        WindowSolverStepper(fn, x, c2, 2, 64, 7)
    with pytest.raises(ValueError, match="L"):
        WindowSolverStepper(fn, x, c2, 2, 96, 48)
    with pytest.raises(ValueError, match=r"\[N, C, L, F\]"):
        WindowSolverStepper(fn, x[0], c2, 2, 64)
    with pytest.raises(ValueError, match="needs noise="):
        WindowSolverStepper(fn, x, s2, 2, 64)
    with pytest.raises(ValueError, match="not both"):
        WindowSolverStepper(fn, x, s2, 2, 64, noise=D.NoiseStream(1), noise_fn=torch.randn_like)
    with pytest.raises(TypeError, match="NoiseStream"):
        WindowSolverStepper(fn, x, s2, 2, 64, noise=torch.Generator())
    with pytest.raises(ValueError, match=r"2\^32"):  # N = 2 canvas samples, not N W = 6 windows, count against the stream
        WindowSolverStepper(fn, x, s2, 2, 64, noise=D.NoiseStream(1, first_sample=2 ** 32 - 1))
    with pytest.raises(ValueError, match="plan="):
        WindowSolverStepper(fn, x, s2, 2, 64, noise=D.BrownianStream(1))
    with pytest.raises(ValueError, match="plan"):
        WindowSolverStepper(fn, x, s2, 2, 64, noise=D.BrownianStream(1), plan=brownian_plan(seq, a, 1.0)[:-1])
    # and what they accept reaches the device state: N W = 6 windows above 2^32 - 4 would be refused, N = 2 samples are not
    with pytest.raises(pytest.fail.Exception, match="device state"):
        WindowSolverStepper(fn, x, s2, 2, 64, noise=D.NoiseStream(1, first_sample=2 ** 32 - 2), threshold=(X0Clip(1.0), None))


# ---- 2. the sixth header ----------------------------------------------------------------------------------------------------------------
def test_sixth_header_is_bound_and_refuses_before_any_launch():
    assert _lib.WINDOW_EXPORTS == ("ddimxw_multistep_update", "ddimxw_blend")
    assert len(_lib.EXPORTS) == 151 and all(n.startswith("ddimx_") for n in _lib.EXPORTS)
    assert _lib.SDE_EXPORTS == ("ddimxs_multistep_update",) and _lib.BROWNIAN_EXPORTS == ("ddimxb_multistep_update", "ddimxb_path_fill")
    assert _lib.DDIMX_ABI_VERSION == 2 and _lib.DDIMX_WINDOW_MAX_COVER == 8
    lib = _lib.load()
    P, I, UL, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_uint
    up, blend = lib.ddimxw_multistep_update, lib.ddimxw_blend  # resolve in the built library
    assert up.restype is I and list(up.argtypes) == [P] * 10 + [I] * 7 + [UL, U, U, P]
    assert blend.restype is I and list(blend.argtypes) == [P] * 5 + [I] * 7 + [P]
    assert D.windowed_solver_steps.__module__ == "ddim_audio_amd.window"
    p = ctypes.c_void_p(256)  # never dereferenced: every argument is checked before the launch
    #       x  eps noise x0 hist jf cnt wt coef step N  W  C  L   T   H   F  seed first base stream
    good = [p, p, None, p, None, p, p, p, p, p, 2, 3, 2, 64, 32, 16, 8, 0, 0, 0, None]
    geometry = [({10: 0}, "N = 0"), ({11: 0}, "W = 0"), ({10: 30000}, "N W in 1..65535"), ({12: 0}, "C = 0"), ({13: 65}, "L = 65"),
                ({15: 0}, "H = 0"), ({13: 66, 15: 33}, "H = 33"), ({16: 6}, "F = 6"), ({16: 0}, "F = 0"), ({14: 0}, "T = 0"),
                ({13: 32 + 2 * 3, 15: 3}, "cover"), ({7: None}, "need wt")]
    bad = [({k: None}, "null") for k in (0, 1, 3, 5, 6, 8, 9)] + geometry + [({18: 2 ** 32 - 1}, "2^32")]
    for edit, msg in bad:
        args = [edit.get(k, v) for k, v in enumerate(good)]
        assert up(*args) != 0, msg
        err = lib.ddimx_last_error().decode()
        assert "ddimxw_multistep_update" in err and msg in err, (msg, err)
    #       eps beps jf cnt wt N  W  C  L   T   H   F  stream
    good = [p, p, p, p, p, 2, 3, 2, 64, 32, 16, 8, None]
    bad = [({k: None}, "null") for k in (0, 1, 2, 3)] + [({k - 5: v for k, v in edit.items()}, msg) for edit, msg in geometry[:-1]] + [
        ({4: None}, "need wt")]
    for edit, msg in bad:
        args = [edit.get(k, v) for k, v in enumerate(good)]
        assert blend(*args) != 0, msg
        err = lib.ddimx_last_error().decode()
        assert "ddimxw_blend" in err and msg in err, (msg, err)


# ---- 3. the references --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taper", ["flat", "tri"])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("tau", [0.0, 0.5, 1.0])
def test_table_form_over_the_blend_equals_the_published_update_over_the_blend(tau, order, taper):
    """``solver_ref.table_steps`` (the w-form the kernels compute) and ``sde_steps`` (the published update), both driven by the blend of
    windows that disagree and are not linear in x, to fp64 rounding."""
    a = MH.alphas()
    seq = logsnr_seq(a, 20)
    T, H, Wn = 16, 6, 4  # K = 3
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, 2, T + (Wn - 1) * H, 4))
    z = rng.standard_normal((20,) + x.shape)
    zs = lambda k, shape: z[k]  # noqa: E731
    g = [R.gaussian_model(a, v) for v in (0.25, 1.0, 2.0, 0.5)]
    fn = lambda w, t, j: g[j](w, t) + 0.1 * np.sin(3.0 * w + t + j)  # noqa: E731
    model = WS.blended(fn, T, H, taper)
    got_x, got_m = R.table_steps(x, dpm_coefficients(seq, a, order, tau=tau), model, zs)
    want_x, want_m = WS.steps(x, seq, fn, a, T, H, taper, order, tau, zs)
    assert len(got_x) == 21 and len(got_m) == 20
    for k in range(20):
        for got, want in ((got_x[k + 1], want_x[k + 1]), (got_m[k], want_m[k])):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (k, tau, order)
    same = lambda w, t, j: g[1](w, t) + 0.1 * np.sin(3.0 * w + t)  # noqa: E731
    agree = WS.steps(x, seq, same, a, T, H, taper, order, tau, zs)[0][-1]
    assert np.abs(agree - want_x[-1]).max() > 1e-2, "the windows disagree: the blend matters"


def test_convergence_on_a_canvas_whose_windows_disagree():
    """The documented table: relative L2 distance of the final canvas from the order-2 run on logsnr_seq(a, 1000) (734 levels).
    The two conditions are the ones the device repeats in fp32."""
    a = MH.alphas()
    seq_of = lambda n: logsnr_seq(a, n)  # noqa: E731
    assert len(seq_of(WS.CONV_FINE)) == 734
    p = D.schedule.window_plan(WS.CONV_SHAPE[2], WS.CONV_T, WS.CONV_H, WS.CONV_TAPER)
    assert p.W == WS.CONV_W == len(WS.CONV_VARS) and p.K == 2
    ref = WS.conv_reference(a, seq_of)
    fn = WS.window_gaussians(a)
    err = {(o, n): WS.rel_l2(WS.steps(WS.conv_start(), seq_of(n), fn, a, WS.CONV_T, WS.CONV_H, WS.CONV_TAPER, o)[0][-1], ref)
           for o in (1, 2, 3) for n in (10, 20, 50)}
    for n in (10, 20, 50):
        print(f"[windowed solver convergence, fp64] {n} steps: " + "  ".join(f"order {o} {err[o, n]:.2e}" for o in (1, 2, 3)))
    table = {(1, 10): 2.30e-1, (2, 10): 3.79e-2, (3, 10): 7.49e-2, (1, 20): 1.16e-1, (2, 20): 1.45e-2, (3, 20): 8.12e-3,
             (1, 50): 4.70e-2, (2, 50): 2.33e-3, (3, 50): 8.37e-4}
    for key, want in table.items():
        assert abs(err[key] - want) <= 0.02 * want, (key, err[key], want)  # the table's three digits, whatever the start
    for what, ratio, bound in WS.conv_conditions(err):
        print(f"[windowed solver convergence, fp64] {what}: ratio {ratio:.3f}")
        assert ratio <= bound, (what, ratio)
    # order 1 on a grid IS the windowed DDIM run on it
    ddim = WR.windowed_steps(WS.conv_start(), seq_of(20), fn, a, WS.CONV_T, WS.CONV_H, WS.CONV_TAPER)[0][-1]
    assert abs(WS.rel_l2(ddim, ref) - err[1, 20]) <= 1e-9
    # the flat taper agrees to a few per cent (not a claim about the taper: the experiment does not hinge on it)
    flat = WS.rel_l2(WS.steps(WS.conv_start(), seq_of(20), fn, a, WS.CONV_T, WS.CONV_H, "flat", 2)[0][-1],
                     WS.steps(WS.conv_start(), seq_of(WS.CONV_FINE), fn, a, WS.CONV_T, WS.CONV_H, "flat", 2)[0][-1])
    print(f"[windowed solver convergence, fp64] flat taper, order 2 at 20 steps: {flat:.2e}")
    assert flat <= 0.25 * err[1, 20]
