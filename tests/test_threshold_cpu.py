"""The host side of the x0 clip / dynamic threshold: the rank, the two rule classes, the samplers' refusal before any device
work, the third header's binding, and the test reference's selection against a sort."""
import ctypes

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, pool, sampler
from ddim_audio_amd.schedule import X0Clip, X0Threshold, check_threshold, make_seq, threshold_rank
import model_harness  # noqa: F401  (tests/ on the path like every other module here)
import step_math_ref as SM
import threshold_ref as TR


def test_threshold_rank():
    assert threshold_rank(1.0, 1) == 0 and threshold_rank(0.5, 1) == 0 and threshold_rank(1e-300, 1) == 0
    for n in (2, 20, 1024, 4 * 5132, 2 ** 31 - 4):
        assert threshold_rank(1.0, n) == n - 1               # the maximum, never n
        assert threshold_rank(1e-12, n) == 0 and threshold_rank(5e-324, n) == 0
        assert threshold_rank(0.5, n) == (n - 1) // 2
        k = threshold_rank(0.995, n)
        assert 0 <= k <= n - 1 and k == int(np.floor(0.995 * (n - 1)))
    assert threshold_rank(0.995, 1024) == 1017 and threshold_rank(0.9, 11) == 9
    # numpy's "lower" quantile picks the same element
    a = np.random.default_rng(3).standard_normal(1001)
    for ratio in (0.1, 0.5, 0.9, 0.995, 1.0):
        assert np.sort(a)[threshold_rank(ratio, a.size)] == np.quantile(a, ratio, method="lower")
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            threshold_rank(0.5, bad)
    for bad in (0.0, -0.1, 1.0000001, float("nan"), float("inf"), "0.5", None):
        with pytest.raises(ValueError):
            threshold_rank(bad, 10)


def test_rule_classes_validate_and_are_immutable():
    c, t = X0Clip(), X0Threshold()
    assert c.limit == 1.0 and (t.ratio, t.floor, t.ceil) == (0.995, 1.0, None)
    assert X0Clip(limit=2.5).limit == 2.5 and X0Threshold(0.9, floor=0.5, ceil=0.5).ceil == 0.5 and X0Threshold(1.0).ratio == 1.0
    assert D.X0Clip is X0Clip and D.X0Threshold is X0Threshold
    assert c == X0Clip(1.0) and hash(t) == hash(X0Threshold(0.995, 1.0, None))
    for obj, name in ((c, "limit"), (t, "ratio"), (t, "floor"), (t, "ceil")):
        with pytest.raises(AttributeError):
            setattr(obj, name, 3.0)
        with pytest.raises(AttributeError):
            obj.other = 1
    for bad in (0.0, -1.0, float("inf"), float("nan"), None, "1", True, 1e-60, 1e60):  # the last two: 0 and inf in fp32
        with pytest.raises(ValueError):
            X0Clip(bad)
    for kw in (dict(ratio=0.0), dict(ratio=-0.5), dict(ratio=1.01), dict(ratio=float("nan")), dict(ratio=None),
               dict(floor=0.0), dict(floor=-1.0), dict(floor=float("inf")), dict(floor=None), dict(floor=1e-60),
               dict(ceil=0.5), dict(floor=2.0, ceil=1.0), dict(ceil=float("inf")), dict(ceil=float("nan")), dict(ceil="2")):
        with pytest.raises(ValueError):
            X0Threshold(**kw)
    assert check_threshold(None) is None and check_threshold(c) is c and check_threshold(t) is t
    for bad in (1.0, "clip", (0.995, 1.0, None), True, X0Clip):
        with pytest.raises(ValueError, match="threshold"):
            check_threshold(bad)


def test_samplers_refuse_an_unknown_threshold_before_any_device_work(monkeypatch):
    monkeypatch.setattr(sampler.DDIMStepper, "__init__", lambda *a, **k: pytest.fail("a stepper was built"))
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(_lib, "stream", lambda: pytest.fail("a launch was prepared"))
    a = model_harness.alphas()
    x = torch.zeros(2, 2, 16, 32)
    model = lambda xt, t: xt  # noqa: E731
    seq = make_seq(1000, 5)
    for bad in (1.0, "dynamic", (0.995, 1.0)):
        with pytest.raises(ValueError, match="threshold"):
            D.generalized_steps(x, seq, model, a, None, threshold=bad)
        with pytest.raises(ValueError, match="threshold"):
            D.dpm_solver_steps(x, seq, model, a, None, order=2, threshold=bad)
        with pytest.raises(ValueError, match="threshold"):
            D.SamplerPool(model, a, slots=2, t_size=16, max_steps=8, threshold=bad)
    assert pool.SamplerPool(model, a, slots=2, t_size=16, max_steps=8, threshold=X0Clip(2.0)).threshold == X0Clip(2.0)
    # the samplers this change leaves alone do not take the keyword
    for fn, kw in ((D.inpaint_steps, dict(y=x, mask=torch.zeros(1, 1, 1, 1))), (D.windowed_steps, dict(window=16, hop=8)),
                   (D.invert_steps, {})):
        with pytest.raises(TypeError, match="threshold"):
            fn(x, seq, model, a, None, threshold=X0Clip(), **kw)


def test_third_header_is_bound_and_the_other_two_lists_are_unchanged():
    assert _lib.THRESHOLD_EXPORTS == ("ddimxq_quantile_work_bytes", "ddimxq_x0_quantile", "ddimxq_threshold_eps")
    assert len(_lib.EXPORTS) == 151 and all(n.startswith("ddimx_") for n in _lib.EXPORTS)
    assert _lib.DISTILL_EXPORTS == ("ddimxd_sqerr_loss_w", "ddimxd_sqerr_loss_w_bwd_mean", "ddimxd_distill_half", "ddimxd_distill_target")
    assert not any(n.startswith("ddimx_") for n in _lib.THRESHOLD_EXPORTS)
    lib = _lib.load()
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    want = {"ddimxq_quantile_work_bytes": (L, [I]),
            "ddimxq_x0_quantile": (I, [P, P, P, I, P, L, F, F, P, P, I, L, P]),
            "ddimxq_threshold_eps": (I, [P, P, P, P, P, I, P, I, L, P])}
    for name, (res, args) in want.items():
        fn = getattr(lib, name)  # resolves in the built library
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.ddimxq_quantile_work_bytes(1) == 16384 and lib.ddimxq_quantile_work_bytes(3) == 3 * 16384
    assert lib.ddimxq_quantile_work_bytes(0) == -1 and lib.ddimxq_quantile_work_bytes(65536) == -1
    # a refusal needs no device: nulls are checked first
    assert lib.ddimxq_x0_quantile(None, None, None, 1, None, 0, 1.0, 2.0, None, None, 1, 4, None) != 0
    assert b"ddimxq_x0_quantile" in lib.ddimx_last_error()
    assert lib.ddimxq_threshold_eps(None, None, None, None, None, 1, None, 1, 4, None) != 0
    assert b"ddimxq_threshold_eps" in lib.ddimx_last_error()


def test_reference_selection_equals_a_sort_on_tied_data():
    rng = np.random.default_rng(11)
    vals = np.array([0.0, -0.0, 0.25, -0.25, 1.5, -3.0, 3.0, 2.0 ** -130, np.inf], dtype=np.float32)
    for n in (1, 7, 1000):
        x0 = vals[rng.integers(0, len(vals) - (n < 1000), n)]  # long runs of equal keys; the inf only in the long case
        keys = np.sort(TR.bits(x0) & TR.ABS)
        assert (np.diff(keys.astype(np.int64)) == 0).sum() >= n - len(vals)
        for rank in sorted({0, n // 3, n // 2, n - 1}):
            assert TR.select_key(TR.bits(x0) & TR.ABS, rank) == keys[rank]
            q = TR.quantile(x0, rank)
            assert TR.bits(q) == keys[rank] and not np.signbit(q)
            assert q == np.sort(np.abs(x0))[rank]  # unsigned order of the bits = order of the magnitudes
    # (s, r): every branch, and the NaN rule
    assert TR.scale_row(0.5, 1.0, None) == (1.0, 1.0) and TR.scale_row(2.0, 1.0, None) == (2.0, 0.5)
    assert TR.scale_row(8.0, 1.0, 4.0) == (4.0, 0.25) and TR.scale_row(np.nan, 1.5, 4.0) == (1.5, 1.0)
    assert TR.scale_row(np.inf, 1.0, None) == (np.float32(np.inf), 0.0)
    # the rewrite keeps eps where the clip keeps x0, and lands on the clipped prediction elsewhere
    x, e = rng.standard_normal(64).astype(np.float32), rng.standard_normal(64).astype(np.float32)
    s1, s2 = np.float32(0.6), np.float32(0.8)
    x0 = SM.ddim_x0(x, e, s1, s2)
    new, keep = TR.rewrite(x, e, s1, s2, np.float32(1.0), np.float32(1.0))
    assert keep.any() and not keep.all() and (keep == (np.abs(x0) <= 1.0)).all()
    assert (TR.bits(new)[keep] == TR.bits(e)[keep]).all()
    assert np.abs(SM.ddim_x0(x, new, s1, s2)[~keep]).max() <= 1.0 + 1e-6
    # float64 rule: Imagen's with floor 1, the identity below the floor
    m = rng.standard_normal((2, 50))
    m[1] *= 0.01
    out = TR.rule64(m, X0Threshold(0.9, 1.0))
    s = np.sort(np.abs(m[0]))[threshold_rank(0.9, 50)]
    assert s > 1 and np.allclose(out[0], np.clip(m[0], -s, s) / s) and np.array_equal(out[1], m[1])
    assert np.array_equal(TR.rule64(m, X0Clip(0.5)), np.clip(m, -0.5, 0.5)) and TR.rule64(m, None) is m
