"""The Brownian path of ``BrownianStream`` on the host (no GPU): ``schedule.brownian_plan`` against the independent plan of
tests/brownian_ref.py; the reference path over the stream's own Philox words -- unit-normal, uncorrelated, additive increments --;
strong convergence across step counts on Gaussian data, against independent per-step normals; the fifth header's binding; and the
samplers that cannot honour a path refusing one before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, sampler, schedule
from ddim_audio_amd.schedule import alphas_cumprod, brownian_plan, dpm_coefficients, get_beta_schedule, logsnr_seq, make_seq
import brownian_ref as B
import model_harness as MH
import noise_ref as N
import sde_ref as S
import solver_ref as R

TAUS = (0.5, 1.0, 2.0)
F32 = np.float32


def _table_1024():
    """A table of exactly 1024 timesteps: D = 10, and point N = 1024 is the only virtual one."""
    return alphas_cumprod(get_beta_schedule("linear", beta_start=1e-4, beta_end=0.02, num_diffusion_timesteps=1024))


def _cases():
    a, a1024 = MH.alphas(), _table_1024()
    assert len(a) == 1000 and len(a1024) == 1024
    return {"logsnr 20": (logsnr_seq(a, 20), a), "uniform 10": (make_seq(1000, 10), a), "adjacent": ([0, 1, 2, 3], a),
            "T 1024": (sorted(set(logsnr_seq(a1024, 20)) | {511, 512, 513, 1022}), a1024)}


# ---- 1. the plan ---------------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_headers():
    assert schedule.BROWNIAN_STRIDE == _lib.DDIMXB_PLAN_STRIDE == 4 + 2 * (_lib.DDIMXB_MAX_DEPTH + 1) * 4
    assert schedule.BROWNIAN_MAX_DEPTH == _lib.DDIMXB_MAX_DEPTH
    assert (schedule.ENTER_ANCHOR, schedule.ENTER_ROOT, schedule.ENTER_LEFT, schedule.ENTER_RIGHT) == (
        _lib.DDIMXB_ENTER_ANCHOR, _lib.DDIMXB_ENTER_ROOT, _lib.DDIMXB_ENTER_LEFT, _lib.DDIMXB_ENTER_RIGHT)
    from ddim_audio_amd import noise
    assert noise.TAG_PATH == _lib.DDIMXB_NOISE_TAG == B.TAG_PATH == 2 and (noise.TAG_STEP, noise.TAG_INITIAL) == (0, 1)


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("case", ["logsnr 20", "uniform 10", "adjacent", "T 1024"])
def test_plan_equals_the_independent_plan(case, tau):
    seq, a = _cases()[case]
    plan = brownian_plan(seq, a, tau)
    want = B.run_plan(seq, a, tau)
    coef = dpm_coefficients(seq, a, 2, tau)
    u, depth = B.clock(a, tau)
    assert plan.dtype == np.int32 and plan.shape == (len(seq), schedule.BROWNIAN_STRIDE) and len(want) == len(seq)
    assert depth == 10 and (u[:len(a)] > 0).all() and (np.diff(u[:len(a)]) < 0).all() and (u[len(a):] == 0).all()
    assert not plan[-1].any() and coef[-1, 5] == 0, "the final jump adds no noise: an empty row"
    levels = list(reversed(seq))
    for k, w in enumerate(want[:-1]):
        share, g, ri, rj = B.decode_row(plan[k], schedule.BROWNIAN_MAX_DEPTH)
        wi, wj, wshare, wg = w
        assert coef[k, 5] != 0 and share == wshare >= 1 and g == F32(wg) and g > 0, (k, share, wshare, g, wg)
        for got, ref, t in ((ri, wi, levels[k]), (rj, wj, levels[k + 1])):
            assert len(got) == len(ref) <= depth + 1 and len(ref) == (1 if t == 0 else 1 + depth - ((t & -t).bit_length() - 1)), (k, t)
            for r, ((node, rho, s, enter), (wnode, wrho, ws, wa, wb)) in enumerate(zip(got, ref)):
                assert node == wnode and rho == F32(wrho) and s == F32(ws), (k, t, r, node, wnode, rho, wrho, s, ws)
                assert 0 <= rho <= 1 and (s > 0) == ((wa + wb) // 2 < len(a)), "a virtual midpoint (t >= T) is W(0) = 0: rho = s = 0"
                if r == 0:
                    assert enter == schedule.ENTER_ANCHOR and node == 0 and rho == 0
                elif r == 1:
                    assert enter == schedule.ENTER_ROOT and node == 1 and (wa, wb) == (0, 1 << depth)
                else:
                    prev_m = (ref[r - 1][3] + ref[r - 1][4]) // 2
                    assert enter == (schedule.ENTER_LEFT if wb == prev_m else schedule.ENTER_RIGHT) and prev_m in (wa, wb)
                    assert node == 2 * ref[r - 1][0] + (wa == prev_m)
        # the words behind the lengths are untouched
        per = 4 * (schedule.BROWNIAN_MAX_DEPTH + 1)
        assert not plan[k, 4 + 4 * len(ri):4 + per].any() and not plan[k, 4 + per + 4 * len(rj):].any()


def test_tau_zero_gives_empty_rows_and_bad_arguments_raise():
    a = MH.alphas()
    seq = logsnr_seq(a, 20)
    assert not brownian_plan(seq, a, 0.0).any()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            brownian_plan(seq, a, bad)
    with pytest.raises(ValueError, match="strictly increasing"):
        brownian_plan([5, 5], a, 1.0)
    with pytest.raises(ValueError, match="tau > 0"):
        schedule.brownian_clock(a, 0.0)
    with pytest.raises(ValueError, match="depth"):
        schedule.brownian_clock(torch.linspace(0.999, 0.001, 2 ** 16 + 1), 1.0)
    with pytest.raises(ValueError, match="non-increasing"):
        schedule.brownian_clock(torch.tensor([0.5, 0.6]), 1.0)
    clock = schedule.brownian_clock(a, 1.0)
    for i, j in ((3, 3), (3, 5), (1000, 3), (5, -1), (5, True)):
        with pytest.raises(ValueError):
            schedule.brownian_row(clock, i, j)
    with pytest.raises(ValueError, match="fp32"):  # two levels whose clocks are one fp32 number
        schedule.brownian_row(schedule.brownian_clock(torch.tensor([0.5, 0.5 - 2.0 ** -25]), 0.01), 1, 0)


# ---- 2. the reference path over the stream's Philox words ----------------------------------------------------------------------------------
N_EL = 2 ** 20
_STEPS = {}


def _steps20():
    """(z of every noisy step of the 20-step grid at tau = 1 [19][2^20], the plans, the source of normals): float64, from the words
    of seed 0x1234, first_sample 3; computed once."""
    if not _STEPS:
        a = MH.alphas()
        seq = logsnr_seq(a, 20)
        assert len(seq) == 20
        plans = B.run_plan(seq, a, 1.0)[:-1]
        xi_r = B.words_normals(0x1234, 3, (1, N_EL))
        xi = lambda node: xi_r(node)[0]  # noqa: E731
        _STEPS.update(z=np.stack([B.increment64(p, xi).reshape(-1) for p in plans]), plans=plans, xi=xi, seq=seq, a=a)
    return _STEPS


def test_increments_are_unit_normals():
    """Each step's z over 2^20 elements, inside the six-sigma gates of test_gpu_noise.py's moments test at this N: mean 1/sqrt(N),
    variance sqrt(2/N), raw fourth moment sqrt(96/N)."""
    z = _steps20()["z"]
    n = z.shape[1]
    assert z.shape == (19, N_EL)
    for k, zk in enumerate(z):
        mean, var, m4 = zk.mean(), zk.var(), (zk ** 4).mean()
        print(f"step {k}: mean {mean:.3e} var {var:.6f} m4 {m4:.5f}")
        assert abs(mean) <= 6 / np.sqrt(n) and abs(var - 1) <= 6 * np.sqrt(2 / n) and abs(m4 - 3) <= 6 * np.sqrt(96 / n), k


def test_increments_of_different_steps_are_uncorrelated():
    z = _steps20()["z"]
    n = z.shape[1]
    c = z - z.mean(axis=1, keepdims=True)
    corr = (c @ c.T) / n / np.sqrt(np.outer(z.var(axis=1), z.var(axis=1)))
    off = np.abs(corr - np.diag(np.diag(corr)))
    print(f"largest correlation between two steps: {off.max():.3e} (gate {6 / np.sqrt(n):.3e})")
    assert off.max() <= 6 / np.sqrt(n)


def test_increments_add_up_across_a_coarse_step():
    """P(j) - P(i) over a step that spans several steps of the fine grid equals the sum of theirs, to float64 rounding (every value
    involved is at most a few sqrt(u_j); 64 ulps of that)."""
    st = _steps20()
    seq, plans, z, xi = st["seq"], st["plans"], st["z"], st["xi"]
    u, depth = B.clock(st["a"], 1.0)
    levels = list(reversed(seq))
    for lo, hi in ((0, 19), (3, 8), (17, 19), (0, 1)):
        i, j = levels[lo], levels[hi]
        coarse = B.step_plan(u, depth, i, j)
        whole = B.increment64(coarse, xi).reshape(-1) / coarse[3]
        parts = sum(z[k] / plans[k][3] for k in range(lo, hi))
        tol = 64 * 2.0 ** -53 * 6 * np.sqrt(u[j])
        assert np.abs(whole - parts).max() <= tol, (lo, hi, np.abs(whole - parts).max(), tol)
        assert whole.std() > 0.9 * np.sqrt(u[j] - u[i])


# ---- 3. strong convergence across step counts ------------------------------------------------------------------------------------------
def test_runs_of_different_step_counts_converge_to_one_sample():
    """Gaussian data (var = 0.25) and its exact noise predictor, float64, order 2, tau = 1, 8192 elements from one x_T: the final
    sample of the 20- and 50-step runs against the 200-step run, rms distance over the sample's std.  On the path: (20, 200) at
    most a quarter of what independent per-step normals give (they give sqrt 2: unrelated samples), and (50, 200) at most half of
    (20, 200).  A float64 prototype on numpy's generator gave 0.185 against 1.44, and 0.074."""
    a, var, seed, shape = MH.alphas(), 0.25, 0x5EED, (1, 8192)
    model = R.gaussian_model(a, var)
    x_t = N.normals64(N.words(seed, 0, shape, 0, N.TAG_INITIAL))[0]
    xi_r = B.words_normals(seed, 0, shape)
    xi = lambda node: xi_r(node)[0]  # noqa: E731

    def final(n, brownian):
        seq = logsnr_seq(a, n)
        if brownian:
            plans = B.run_plan(seq, a, 1.0)
            zs = lambda k, shp: B.increment64(plans[k], xi)  # noqa: E731
        else:
            zs = S.stream_normals(seed, 0)
        return R.table_steps(x_t, dpm_coefficients(seq, a, 2, 1.0), model, zs)[0][-1]

    ref = final(200, True)
    dist = lambda x, y: float(np.sqrt(np.mean((x - y) ** 2)) / y.std())  # noqa: E731
    b20, b50, b100 = (dist(final(n, True), ref) for n in (20, 50, 100))
    i20 = dist(final(20, False), final(200, False))
    print(f"distance to the 200-step run / std: on the path 20 steps {b20:.4f}, 50 steps {b50:.4f}, 100 steps {b100:.4f}; "
          f"independent normals 20 steps {i20:.4f}; final std {ref.std():.4f} (data std {np.sqrt(var):.4f})")
    assert abs(ref.std() / np.sqrt(var) - 1) <= 0.05
    assert b20 <= 0.25 * i20
    assert b50 <= 0.5 * b20


# ---- 4. the stream object, the binding, the refusals ---------------------------------------------------------------------------------------
def test_stream_object():
    bs = D.BrownianStream(0x1234, 3)
    assert not isinstance(bs, D.NoiseStream) and (bs.seed, bs.first_sample) == (0x1234, 3)
    assert "BrownianStream" in repr(bs)
    sh = bs.shard(5)
    assert type(sh) is D.BrownianStream and (sh.seed, sh.first_sample) == (0x1234, 8)
    ns = D.NoiseStream(0x1234, 3)
    for n, rank, world in ((8, 0, 3), (8, 1, 3), (8, 2, 3), (5, 1, 2)):
        got = bs.for_rank(n, rank, world)
        assert type(got) is D.BrownianStream and got.first_sample == ns.for_rank(n, rank, world).first_sample
    for bad in (-1, 2 ** 64, 1.0, True):
        with pytest.raises(ValueError):
            D.BrownianStream(bad)
    with pytest.raises(ValueError):
        D.BrownianStream(0, 2 ** 32)


def test_samplers_that_cannot_follow_a_path_refuse_it_before_any_device_work(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "stream", no_library)
    monkeypatch.setattr(sampler.DDIMStepper, "__init__", lambda *a, **k: pytest.fail("a stepper was built"))
    a = MH.alphas()
    b = schedule.make_schedule(D.configs.audio_config().diffusion)[0]
    model = lambda x, t: x  # noqa: E731  (never called)
    seq = list(range(0, 1000, 200))
    bs = D.BrownianStream(3)
    x = torch.zeros(2, 2, 16, 32)
    with pytest.raises(TypeError, match="NoiseStream"):
        D.generalized_steps(x, seq, model, a, None, eta=1.0, noise=bs)
    with pytest.raises(TypeError, match="NoiseStream"):
        D.ddpm_steps(x, seq, model, b, None, noise=bs)
    with pytest.raises(TypeError, match="NoiseStream"):
        D.inpaint_steps(x, seq, model, a, None, y=x, mask=torch.ones(2, 1, 16, 32), eta=1.0, noise=bs)
    pool = D.SamplerPool(model, a, slots=4, t_size=32, max_steps=10)
    with pytest.raises(TypeError, match="NoiseStream"):
        pool.submit(torch.zeros(2, 2, 32, 8), seq, order=2, tau=1.0, noise=bs)
    assert pool.stats == {"steps": 0, "busy": 0, "idle": 0, "captures": 0} and not pool.table.queue
    # the solver takes it, and still checks what it checked
    with pytest.raises(ValueError, match="not both"):
        D.dpm_solver_steps(x, seq, model, a, None, order=2, tau=1.0, noise=bs, noise_fn=torch.randn_like)
    with pytest.raises(TypeError, match="NoiseStream"):
        D.dpm_solver_steps(x, seq, model, a, None, order=2, tau=1.0, noise=torch.Generator())
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            D.dpm_solver_steps(x, seq, model, a, None, order=2, tau=bad, noise=bs)


def test_fifth_header_is_bound_and_refuses_before_any_launch():
    assert _lib.BROWNIAN_EXPORTS == ("ddimxb_multistep_update", "ddimxb_path_fill")
    assert _lib.SDE_EXPORTS == ("ddimxs_multistep_update",) and len(_lib.EXPORTS) == 151
    assert not any(n.startswith("ddimx_") for n in _lib.BROWNIAN_EXPORTS)
    lib = _lib.load()
    P, I, L, UL, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_uint
    up, fill = lib.ddimxb_multistep_update, lib.ddimxb_path_fill  # resolve in the built library
    assert up.restype is I and list(up.argtypes) == [P, P, P, P, P, P, P, I, L, UL, U, P]
    assert fill.restype is I and list(fill.argtypes) == [P, I, L, UL, U, P, I, P]
    p = ctypes.c_void_p(256)  # never dereferenced
    good = [p, p, p, None, p, p, p, 1, 4, 0, 0, None]
    bad = [({k: None}, "null") for k in (0, 1, 2, 4, 5, 6)] + [({7: 0}, "B = 0"), ({7: 65536}, "B = 65536"), ({8: 0}, "multiple of 4"),
                                                                ({8: 6}, "multiple of 4"), ({8: -4}, "multiple of 4"),
                                                                ({8: 4 * (2 ** 32 + 1)}, "groups of four"), ({7: 2, 10: 2 ** 32 - 1}, "2^32")]
    for edit, msg in bad:
        args = [edit.get(k, v) for k, v in enumerate(good)]
        assert up(*args) != 0, msg
        err = lib.ddimx_last_error().decode()
        assert "ddimxb_multistep_update" in err and msg in err, (msg, err)
    good = [p, 1, 4, 0, 0, p, _lib.DDIMXB_PATH, None]
    bad = [({0: None}, "null"), ({5: None}, "null"), ({1: 0}, "B = 0"), ({2: 6}, "multiple of 4"), ({1: 2, 4: 2 ** 32 - 1}, "2^32"),
           ({6: 2}, "kind = 2"), ({6: -1}, "kind = -1")]
    for edit, msg in bad:
        args = [edit.get(k, v) for k, v in enumerate(good)]
        assert fill(*args) != 0, msg
        err = lib.ddimx_last_error().decode()
        assert "ddimxb_path_fill" in err and msg in err, (msg, err)
