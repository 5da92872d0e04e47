"""``windowed_inpaint_solver_steps`` without a GPU: the fp64 reference (tests/window_inpaint_solver_ref.py: a composition of
``inpaint_solver_ref.solver_steps`` and ``window_inpaint_ref.blend``) keeps the solver's order where the windows disagree and the
mask spans several windows; it reduces to the two references it is composed of; every refusal comes before any device work; the
header is the tenth public header, and its two functions are bound on first use like every other."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib
from ddim_audio_amd.schedule import logsnr_seq
import inpaint_solver_ref as R
import model_harness as MH
import window_inpaint_solver_ref as WIS
import window_solver_ref as WS

HEADER = "ddimx_window_inpaint_solver.h"


# ---- 1. the study --------------------------------------------------------------------------------------------------------------------
def test_convergence_study_on_disagreeing_correlated_windows():
    """Order 2 at 20 steps is at most a quarter of order 1 at 20 steps and at most order 1 at 50 steps, replacement only and guided
    (rho = 0.3) + replacement alike; the guidance is no formality."""
    a = MH.alphas()
    seq_of = lambda n: logsnr_seq(a, n)  # noqa: E731
    err = WIS.conv_study(a, seq_of)
    for mode, e in err.items():
        print(f"[windowed inpaint solver study: {mode}]\n{WIS.conv_table(e)}")
        for what, ratio, bound in WS.conv_conditions(e):
            print(f"[windowed inpaint solver study: {mode}] {what}: {ratio:.3f} (<= {bound})")
            assert ratio <= bound, (mode, what, ratio)
    guided = WIS.conv_final(a, seq_of(20), 2, **WIS.CONV_MODES["guided+replace"]).numpy()
    plain = WIS.conv_final(a, seq_of(20), 2, **WIS.CONV_MODES["replace"]).numpy()
    diff = WS.rel_l2(guided, plain)
    print(f"[windowed inpaint solver study] guided against unguided, order 2 at 20 steps: {diff:.2e}")
    assert diff > 1e-4, "the guided run is the unguided one"


# ---- 2. identities of the reference ---------------------------------------------------------------------------------------------------
def _smooth_model(alpha):
    """``fn(window, t, j)`` in torch: smooth, nonlinear, differentiable, mixing neighbouring rows (so a gradient crosses from the known
    rows into the gap) and different per window -- and well conditioned, unlike the study's matrix inverses, whose amplification
    of one rounding would say nothing about an identity."""
    a = torch.as_tensor(alpha).to("cpu", torch.float32).double()

    def fn(w, t, j):
        ti = int(torch.as_tensor(t).reshape(-1)[0])
        return (1.0 - a[ti]).sqrt().to(w.dtype) * torch.tanh(0.7 * w + 0.3 * torch.roll(w, 1, -2) + 0.1 * j)

    return fn


def _rel(got, want):
    return max(float((torch.as_tensor(u) - torch.as_tensor(v)).abs().max() / torch.as_tensor(v).abs().max()) for u, v in zip(got, want))


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("guidance", [0.0, 0.3])
def test_one_window_is_solver_steps(order, guidance):
    a = MH.alphas()
    fn = _smooth_model(a)
    x, y, mask = WIS.conv_case()
    x, y, mask = x[:, :, :WS.CONV_T], y[:, :, :WS.CONV_T], mask[:, :, :WS.CONV_T]
    seq = logsnr_seq(a, 7)
    kw = dict(guidance=guidance, replace=True, order=order)
    for taper in ("flat", "tri"):
        got = WIS.steps(x, seq, fn, a, WS.CONV_T, WS.CONV_T, taper, y, mask, **kw)
        want = R.solver_steps(x, seq, lambda xx, t: fn(xx, t, 0), a, y, mask, **kw)
        worst = _rel(got[0][1:] + got[1], want[0][1:] + want[1])
        print(f"[one window, order {order}, rho {guidance}, {taper}] worst relative difference {worst:.2e}")
        assert worst <= 1e-12


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("replace", [True, False])
def test_empty_mask_without_guidance_is_the_windowed_solver_reference(order, replace):
    a = MH.alphas()
    fn = _smooth_model(a)
    x, y, _ = WIS.conv_case()
    seq = logsnr_seq(a, 7)
    got = WIS.steps(x, seq, fn, a, WS.CONV_T, WS.CONV_H, WS.CONV_TAPER, y, torch.zeros(1, 1, 1, 1, dtype=torch.float64), guidance=0.0,
                    replace=replace, order=order)
    fn_np = lambda w, t, j: fn(torch.from_numpy(np.ascontiguousarray(w)), t, j).numpy()  # noqa: E731
    want = WS.steps(x.numpy(), seq, fn_np, a, WS.CONV_T, WS.CONV_H, WS.CONV_TAPER, order)
    worst = _rel(got[0][1:] + got[1], want[0][1:] + want[1])
    print(f"[empty mask, order {order}, replace {replace}] worst relative difference {worst:.2e}")
    assert worst <= 1e-12


# ---- 3. validation -------------------------------------------------------------------------------------------------------------------
def _call(**kw):
    # the model is never reached: validation comes before any device work (None would fail at the first forward)
    shape = (2, 2, 48, 32)
    kw.setdefault("y", torch.zeros(shape))
    kw.setdefault("mask", torch.ones(shape))
    kw.setdefault("window", 16)
    kw.setdefault("hop", 8)
    return D.windowed_inpaint_solver_steps(kw.pop("x", torch.zeros(shape)), kw.pop("seq", [0, 300, 600]), kw.pop("model", None),
                                           MH.alphas(), None, **kw)


INVALID = [
    (dict(noise=D.BrownianStream(1, 0), tau=1.0), ValueError, "BrownianStream"),
    (dict(corrector=True), ValueError, "corrector"),
    (dict(threshold=D.X0Clip(1.0)), ValueError, "threshold"),
    (dict(noise=D.NoiseStream(1, 0), noise_fn=torch.randn_like, tau=1.0), ValueError, "not both"),
    (dict(noise=object(), tau=1.0), TypeError, "NoiseStream"),
    (dict(order=0), ValueError, "order"),
    (dict(order=4), ValueError, "order"),
    (dict(tau=-0.5), ValueError, "tau"),
    (dict(tau=float("inf")), ValueError, "tau"),
    (dict(y=None), ValueError, "needs y="),
    (dict(mask=None), ValueError, "needs y="),
    (dict(y=torch.zeros(2, 2, 16, 32)), ValueError, "broadcast"),
    (dict(mask=torch.full((2, 2, 48, 32), 1.5)), ValueError, r"\[0, 1\]"),
    (dict(y=torch.zeros(2, 2, 48, 32, dtype=torch.int32)), ValueError, "floating"),
    (dict(mask="all"), TypeError, "mask"),
    (dict(guidance=-1.0), ValueError, "guidance"),
    (dict(guidance=[0.1, 0.2]), ValueError, "guidance"),
    (dict(prediction="x0"), ValueError, "prediction"),
    (dict(seq=[]), ValueError, "empty"),
    (dict(seq=[0, 300, 300]), ValueError, "increasing"),
    (dict(x=torch.zeros(2, 2, 48)), ValueError, "N, C, L, F"),
    (dict(x=torch.zeros(2, 2, 48, 30), y=torch.zeros(2, 2, 48, 30), mask=torch.ones(1)), ValueError, "multiple of 4"),
    (dict(window=0), ValueError, "window"),
    (dict(hop=0), ValueError, "hop"),
    (dict(hop=7), ValueError, "hop"),
    (dict(hop=1), ValueError, "8"),
    (dict(taper="hann"), ValueError, "taper"),
    (dict(guidance=0.3, model=lambda x, t: x), RuntimeError, "needs a ddim_audio_amd.Model"),
]


def test_invalid_arguments_raise_before_device_work():
    for kw, exc, msg in INVALID:
        with pytest.raises(exc, match=msg):
            _call(**kw)
    assert "windowed_inpaint_solver_steps" in str(pytest.raises(ValueError, _call, corrector=True).value)
    assert not torch.cuda.is_initialized()


def test_docstrings_carry_the_warning():
    import ddim_audio_amd.window_inpaint_solver as mod
    assert "erratic" in mod.__doc__ and "replace=True" in mod.__doc__
    doc = D.windowed_inpaint_solver_steps.__doc__
    assert "guidance_per_step" in doc and "erratic" in doc and "BrownianStream" in doc


# ---- 4. the binding ------------------------------------------------------------------------------------------------------------------
PUBLIC = ["ddimx.h", "ddimx_brownian.h", "ddimx_distill.h", "ddimx_inpaint_solver.h", "ddimx_sde.h", "ddimx_threshold.h", "ddimx_unic.h",
          "ddimx_window.h", "ddimx_window_inpaint.h", HEADER]


def test_header_is_found_parsed_and_in_the_public_table():
    assert list(_lib.HEADERS) == PUBLIC and len(_lib.EXPORTS) == 151
    assert sorted(_lib.HEADERS) == sorted(f for f in os.listdir(_lib._INCLUDE) if f.startswith("ddimx") and f.endswith(".h"))
    h = _lib.HEADERS[HEADER]
    assert list(h.funcs) == ["ddimxwis_residual", "ddimxwis_multistep_update"] and not h.consts and not h.structs
    P, I, U = _lib.c_void_p, _lib.c_int, _lib.c_uint
    res, args = h.funcs["ddimxwis_residual"]
    assert res is I and args == _lib.HEADERS["ddimx_window_inpaint.h"].funcs["ddimxwi_residual"][1] == [P] * 13 + [I] * 7 + [P]
    res, args = h.funcs["ddimxwis_multistep_update"]
    assert res is I and args == [P] * 15 + [I] * 8 + [_lib.c_ulonglong, U, U, P]
    # its tuple exists by the table's rule, beside its neighbours'; no name is declared twice across the headers
    assert _lib.WINDOW_INPAINT_SOLVER_EXPORTS == tuple(h.funcs)
    assert _lib.WINDOW_INPAINT_EXPORTS == ("ddimxwi_partials_floats", "ddimxwi_residual", "ddimxwi_update")
    assert _lib.INPAINT_SOLVER_EXPORTS == ("ddimxi_residual", "ddimxi_multistep_update")
    every = [n for hd in _lib.HEADERS.values() for n in hd.funcs]
    assert len(every) == len(set(every)) and [n for n in every if n.startswith("ddimxwis_")] == list(h.funcs)
    from ddim_audio_amd import build
    assert len(build.SOURCES) == 50 and os.path.exists(os.path.join(build.CSRC, "window_inpaint_kernels.h"))


class _FakeLib:
    """A library with every function of the other headers and, of this one, only those in ``has``."""

    def __init__(self, has):
        self.has, self.touched = set(has), []

    def __getattr__(self, name):
        if name.startswith("ddimxwis_") and name not in self.has:
            raise AttributeError(name)
        self.touched.append(name)
        fn = types.SimpleNamespace()
        if name == "ddimx_abi_version":
            fn = lambda: _lib.DDIMX_ABI_VERSION  # noqa: E731
        setattr(self, name, fn)
        return fn


def _fake(monkeypatch, has):
    fake = _FakeLib(has)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: fake)
    monkeypatch.setattr(_lib, "LIB_PATH", __file__)  # a file that exists; the fake CDLL never opens it
    return fake


def test_binds_on_first_use_and_names_what_an_old_library_lacks(monkeypatch):
    funcs = _lib.HEADERS[HEADER].funcs
    # an old library: it loads, nothing of this header touched; the missing function names the header, itself and the remedy
    old = _fake(monkeypatch, has=["ddimxwis_residual"])
    lib = _lib.load()
    assert old.touched == ["ddimx_abi_version"]
    with pytest.raises(RuntimeError, match=r"^ddimx_window_inpaint_solver\.h: .*ddimxwis_multistep_update.*built before this header existed: rebuild"):
        lib.ddimxwis_multistep_update
    assert __file__ in str(pytest.raises(RuntimeError, getattr, lib, "ddimxwis_multistep_update").value)  # LIB_PATH
    assert lib.ddimxwis_residual.argtypes == funcs["ddimxwis_residual"][1]  # what it has, it runs
    # the stepper's refusal, by name and in front of every allocation: the window cut is host work, the parents' __init__ is not reached
    from ddim_audio_amd.window_inpaint_solver import WindowInpaintSolverStepper
    with pytest.raises(RuntimeError, match=r"ddimx_window_inpaint_solver\.h: .*ddimxwis_multistep_update.*rebuild"):
        WindowInpaintSolverStepper(None, torch.zeros(1, 2, 48, 32), None, None, None, 2, False, True, 16, 8)
    assert not torch.cuda.is_initialized()
    # a current one: each function bound once, with the parsed types
    new = _fake(monkeypatch, has=list(funcs))
    lib = _lib.load()
    for name, (res, args) in funcs.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
        assert getattr(lib, name) is getattr(new, name)
    assert new.touched == ["ddimx_abi_version", *funcs], "bound once"


@pytest.mark.skipif(shutil.which("nm") is None, reason="nm (binutils) is needed to list the library's dynamic symbols")
def test_library_defines_the_extension_symbols():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libddimx.so is not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.split()}
    assert set(_lib.HEADERS[HEADER].funcs) <= defined
    assert {n for n in defined if n.startswith("ddimxwis_")} == set(_lib.HEADERS[HEADER].funcs)


# ---- 5. the timing tool, as far as it runs without a device ---------------------------------------------------------------------------
def test_timing_tool_imports_parses_and_refuses_without_a_gpu(monkeypatch):
    import importlib
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import timing
    mod = importlib.import_module("window_inpaint_solver_time")
    assert "usage: python tools/window_inpaint_solver_time.py [rounds=5] [wall]" in mod.__doc__
    assert (mod.N, mod.W, mod.T, mod.H, mod.L) == (1, 8, 1024, 512, 4608)
    seen = []
    parse = timing.parse_args

    def spy(argv, spec, flags=()):
        seen.append(vars(parse(argv, spec, flags)))
        return parse(argv, spec, flags)
    monkeypatch.setattr(timing, "parse_args", spy)
    for line, want in (("", dict(rounds=5, wall=False)), ("2 wall", dict(rounds=2, wall=True)), ("wall rounds=0", dict(rounds=0, wall=True))):
        with pytest.raises(RuntimeError, match="GPU"):  # main parses, then refuses: no device work
            mod.main(line.split())
        assert seen[-1] == want
    with pytest.raises(SystemExit, match="rounds"):
        mod.main(["abc"])
    assert not torch.cuda.is_initialized()
