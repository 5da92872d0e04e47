"""Windowed long-form sampling on the GPU (ddim_audio_amd.windowed_steps, ddimx_window_gather / ddimx_window_update).

Bit for bit against the samplers that existed before (one window = generalized_steps; no overlap = generalized_steps over the
segments as a batch; K = 1 update = ddimx_ddim_update); the overlap against the float64 restatement (tests/window_ref.py) driving
the CPU oracle's forward, at the project's gates; the blend kernel alone against the float64 sum inside the textbook bound of a
fused-multiply-add chain; replayed = eager; canvas-batch invariance; validation and graph ownership."""
import functools
import gc

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, synth
from ddim_audio_amd.noise import NoiseStream
from ddim_audio_amd.schedule import ddim_coefficients, window_plan
from ddim_audio_amd.window import WindowStepper
import gpu_util as G
import model_harness as MH
from model_harness import MODES, MODE_IDS, U
import window_ref as R

pytestmark = pytest.mark.gpu
TAPERS = ["flat", "tri"]
P = _lib.ptr


# ---- 1. one window is generalized_steps -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_one_window_is_generalized_steps(mode, eta, taper):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = list(range(0, 1000, 100))
    x = synth.gaussian("window.one", (4, 2, 32, 32))
    ns = lambda: NoiseStream(0xABCD, 1) if eta else None  # noqa: E731  (the same seed on both sides)
    want_xs, want_x0 = D.generalized_steps(x.cuda(), seq, m, a, None, eta=eta, noise=ns())
    xs, x0 = D.windowed_steps(x.cuda(), seq, m, a, None, window=32, taper=taper, eta=eta, noise=ns())
    assert len(xs) == 11 and len(x0) == 10 and xs[1].shape == x.shape and torch.isfinite(xs[-1]).all()
    MH.same_list(xs[1:], want_xs[1:], "xs")
    MH.same_list(x0, want_x0, "x0_preds")
    if eta:
        assert not torch.equal(xs[1], D.windowed_steps(x.cuda(), seq, m, a, [0], window=32, taper=taper)[0][1]), "the noise entered"
    # the conventions of generalized_steps: xs[0] is the caller's tensor, updated in place; select_index
    xc = x.cuda()
    sxs, sx0 = D.windowed_steps(xc, seq, m, a, [2, -1], window=32, hop=32, taper=taper, eta=eta, noise=ns())
    assert sxs[0] is xc and torch.equal(xc.cpu(), xs[-1]) and len(sxs) == 3 and len(sx0) == 2
    MH.same_list(sxs[1:], [xs[3], xs[10]], "selected xs")
    MH.same_list(sx0, [x0[2], x0[9]], "selected x0")


# ---- 2. no overlap is a batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_no_overlap_is_a_batch_of_segments(mode, taper):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = list(range(0, 1000, 100))
    T, W, N = 32, 3, 2
    x = synth.gaussian("window.segments", (N, 2, W * T, 32))
    segs = torch.stack([x[n, :, j * T:(j + 1) * T] for n in range(N) for j in range(W)])  # sample 3 n + j
    want_xs, want_x0 = D.generalized_steps(segs.cuda(), seq, m, a, None, eta=0.0)
    xs, x0 = D.windowed_steps(x.cuda(), seq, m, a, None, window=T, hop=T, taper=taper)
    assert len(xs) == 11 and len(x0) == 10
    for got, want in ((xs[1:], want_xs[1:]), (x0, want_x0)):
        for i, (u, v) in enumerate(zip(got, want)):
            for n in range(N):
                for j in range(W):
                    assert torch.equal(u[n, :, j * T:(j + 1) * T], v[W * n + j]), (i, n, j)


# ---- 3. overlap, against the reference ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_reference(H, taper):
    """The float64 reference over the oracle's fp32 forward: the same for both activation dtypes of the GPU model."""
    cfg, m = MH.build("tiny", MODES[0][0], 5, mode="eval")
    T = 64
    L = T + 4 * H  # W = 5: every hop reaches its full K-fold cover
    x = synth.gaussian(f"window.overlap.{H}", (2, 2, L, 32))
    seq = list(range(0, 1000, 100))
    xs, x0 = R.windowed_steps(x.double().numpy(), seq, MH.oracle_eps_np(m, "tiny"), MH.alphas(cfg), T, H, taper)
    return x, seq, xs, x0


@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("H", [32, 16, 24])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_overlap_matches_the_reference(mode, H, taper):
    """The final x0 prediction and every selected x within the trajectory gates (x 10): fp32 max <= 1e-3 sigma,
    rms <= 2e-4 sigma; bf16 1.5, 0.2."""
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    x, seq, rxs, rx0 = _tiny_reference(H, taper)
    p = window_plan(x.size(2), 64, H, taper)
    assert p.W == 5 and p.K == {32: 2, 16: 4, 24: 3}[H] and int(p.cnt.max()) == p.K
    sel = [0, 4, -1]
    xs, x0 = D.windowed_steps(x.cuda(), seq, m, MH.alphas(cfg), sel, window=64, hop=H, taper=taper)
    assert len(xs) == 4 and len(x0) == 3
    for k, i in enumerate(sel):
        mx, rms = G.check_close(xs[k + 1], rxs[i % 10 + 1], mode[1], f"x at iteration {i}", scale=10.0)
        print(f"[windowed vs reference {MODE_IDS[mode[1]]} H {H} {taper}] x at iteration {i}: max {mx:.3e} rms {rms:.3e} of sigma")
    mx, rms = G.check_close(x0[-1], rx0[-1], mode[1], "final x0 prediction", scale=10.0)
    print(f"[windowed vs reference {MODE_IDS[mode[1]]} H {H} {taper}] final x0: max {mx:.3e} rms {rms:.3e} of sigma")


@functools.lru_cache(maxsize=None)
def _audio_reference():
    cfg, m = MH.build("audio", MODES[0][0], 5, mode="eval")
    x = synth.gaussian("window.audio", (1, 2, 2048, 256))
    seq = [400, 900]
    xs, x0 = R.windowed_steps(x.double().numpy(), seq, MH.oracle_eps_np(m, "audio"), MH.alphas(cfg), 1024, 512, "tri")
    return x, seq, xs, x0


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_overlap_at_the_audio_widths_matches_the_oracle(mode):
    """T = 1024, H = 512, W = 3 over a 2-step schedule (the CPU oracle needs about a second per T = 1024 forward)."""
    cfg, m = MH.build("audio", mode[0], 5, mode="eval")
    x, seq, rxs, rx0 = _audio_reference()
    xs, x0 = D.windowed_steps(x.cuda(), seq, m, MH.alphas(cfg), None, window=1024, hop=512, taper="tri")
    assert len(xs) == 3 and len(x0) == 2
    for i in range(2):
        mx, rms = G.check_close(xs[i + 1], rxs[i + 1], mode[1], f"x after iteration {i}", scale=10.0)
        print(f"[windowed vs oracle, audio {MODE_IDS[mode[1]]}] x after iteration {i}: max {mx:.3e} rms {rms:.3e} of sigma")
    mx, rms = G.check_close(x0[-1], rx0[-1], mode[1], "final x0 prediction", scale=10.0)
    print(f"[windowed vs oracle, audio {MODE_IDS[mode[1]]}] final x0: max {mx:.3e} rms {rms:.3e} of sigma")


@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("H", [32, 16, 24, 9])
def test_callable_model_that_knows_its_window(H, eta):
    """Any callable ``model(x, t)`` on the window batch: eps = g_j x with a gain per window (sample b of the batch is window b % W),
    against the reference with the same gains and, for eta = 1, the same NoiseStream draws; allclose at 2e-5 like the stream sampler's
    oracle test (fp32 arithmetic on both sides of a 10-step trajectory)."""
    a = MH.alphas()
    seq = list(range(0, 1000, 100))
    T, Wn, N = 64, 5, 2
    L = T + (Wn - 1) * H
    gj = [0.15 + 0.1 * ((3 * j + 1) % 5) for j in range(Wn)]
    gains = torch.tensor(gj * N, device=G.dev()).view(-1, 1, 1, 1)
    x = synth.gaussian(f"window.callable.{H}", (N, 2, L, 16))
    ns = NoiseStream(2718, 3)
    for taper in TAPERS:
        xs, x0 = D.windowed_steps(x.cuda(), seq, lambda w, t: gains * w, a, None, window=T, hop=H, taper=taper, eta=eta,
                                  noise=ns if eta else None)
        rxs, rx0 = R.windowed_steps(x.double().numpy(), seq, lambda w, t, j: gj[j] * w, a, T, H, taper, eta=eta,
                                    noise_fn=lambda k, ref: ns.step_noise(x.shape, k, G.dev()).cpu().double().numpy())
        for k in range(10):
            assert torch.allclose(xs[k + 1].double(), torch.from_numpy(rxs[k + 1]), rtol=2e-5, atol=2e-5), (taper, k)
            assert torch.allclose(x0[k].double(), torch.from_numpy(rx0[k]), rtol=2e-5, atol=2e-5), (taper, k)


# ---- 4. the kernels alone, through the C ABI --------------------------------------------------------------------------------------------
# (N, C, T, H, W, F): K = 1, 2, 3, 7, 8; one canvas large enough for more than 1024 blocks (2 x 2080 x 256 / 4 / 256 = 1040);
# canvases whose element count is not a multiple of 1024
KERNEL_CASES = [(2, 2, 32, 32, 3, 32), (2, 2, 32, 16, 4, 32), (3, 2, 32, 12, 4, 12), (2, 1, 32, 5, 9, 8), (2, 2, 32, 4, 10, 4),
                (1, 2, 32, 16, 129, 256), (5, 3, 8, 3, 6, 20),
                (2, 1, 8, 2, 5, 4), (2, 1, 10, 2, 6, 4), (2, 1, 12, 2, 7, 4)]  # the last three: K = 4, 5, 6


def _case_tensors(case, seed):
    N, C, T, H, W, F = case
    L = T + (W - 1) * H
    g = torch.Generator().manual_seed(seed)
    canvas = torch.randn((N, C, L, F), generator=g)
    eps = torch.randn((N * W, C, T, F), generator=g)
    noise = torch.randn((N, C, L, F), generator=g)
    return L, canvas.to(G.dev()), eps.to(G.dev()), noise.to(G.dev())


def _plan_tensors(L, T, H, taper):
    p = window_plan(L, T, H, taper)
    return p, torch.from_numpy(p.jfirst).to(G.dev()), torch.from_numpy(p.cnt).to(G.dev()), torch.from_numpy(p.wt.copy()).to(G.dev())


def _update(x, eps, noise, x0, jf, cn, wt, coef, ctr, geom):
    _lib.check(_lib.load().ddimx_window_update(P(x), P(eps), P(noise), P(x0), P(jf), P(cn), P(wt), P(coef), P(ctr), *geom, _lib.stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", KERNEL_CASES, ids=str)
def test_gather_equals_the_slices(case):
    N, C, T, H, W, F = case
    L, canvas, _, _ = _case_tensors(case, 1)
    win = torch.full((N * W, C, T, F), float("nan"), device=G.dev())
    _lib.check(_lib.load().ddimx_window_gather(P(canvas), P(win), N, W, C, L, T, H, F, _lib.stream()))
    torch.cuda.synchronize()
    want = torch.stack([canvas[n, :, j * H:j * H + T] for n in range(N) for j in range(W)])
    assert torch.equal(win, want)


@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=str)
def test_blend_within_the_fma_chain_bound(case, taper):
    """Coefficient row (s1, s2) = (-1, 1) and x = 0: the kernel's x0 IS the blended eps.  Where one window covers the row it is
    that window's eps bit for bit; elsewhere it differs from the float64 sum of fp32 weights x fp32 values by at most
    cnt * 2^-24 * sum_k |w_k eps_k|: the textbook bound of a cnt-term fused-multiply-add chain (term k passes through at most cnt
    roundings, each at most 2^-24 relative).  Derived, not tuned; the largest share of it is printed before the assertion."""
    N, C, T, H, W, F = case
    L, _, eps, _ = _case_tensors(case, 2)
    p, jf, cn, wt = _plan_tensors(L, T, H, taper)
    x = torch.zeros((N, C, L, F), device=G.dev())
    x0 = torch.full_like(x, float("nan"))
    coef = torch.tensor([[7.0, -1.0, 1.0, 0.5, 0.25, 0.0]], device=G.dev())
    ctr = torch.zeros(1, dtype=torch.int32, device=G.dev())
    _update(x, eps, None, x0, jf, cn, wt, coef, ctr, (N, W, C, L, T, H, F))
    assert torch.isfinite(x0).all() and torch.isfinite(x).all(), "every element must be written"
    got = x0.cpu().double().numpy()
    e = eps.cpu().double().numpy().reshape(N, W, C, T, F)
    total, mag = np.zeros((N, C, L, F)), np.zeros((N, C, L, F))
    single = np.zeros((N, C, L, F))
    for row in range(L):
        for k in range(int(p.cnt[row])):
            j = int(p.jfirst[row]) + k
            term = float(p.wt[k, row]) * e[:, j, :, row - j * H, :]
            total[:, :, row], mag[:, :, row] = total[:, :, row] + term, mag[:, :, row] + np.abs(term)
        single[:, :, row] = e[:, int(p.jfirst[row]), :, row - int(p.jfirst[row]) * H, :]
    one = p.cnt == 1
    assert np.array_equal(got[:, :, one], single[:, :, one]), "cnt == 1: a select, no multiply"
    bound = p.cnt.astype(np.float64)[None, None, :, None] * U * mag
    err = np.abs(got - total)
    many = ~one
    if many.any():
        worst = float((err[:, :, many] / bound[:, :, many]).max())
        print(f"[blend {case} {taper}] K {p.K}: max error / bound {worst:.3f}")
        assert (err[:, :, many] <= bound[:, :, many]).all(), worst
    # x_{t-1} = s3 x0 + c2 e on the same blended value, ddim_update's two roundings
    eb = x0.double()
    want_x = (eb * 0.5).float().double() + 0.25 * eb  # fmaf(e, c2, fmul(x0, s3)): the product rounded, the fma rounded once
    assert torch.equal(x, want_x.float())


@pytest.mark.parametrize("with_noise", [False, True], ids=["eta0", "noise"])
@pytest.mark.parametrize("case", [(2, 2, 32, 32, 3, 32), (1, 2, 1040, 1040, 2, 256), (5, 3, 8, 8, 6, 20)], ids=str)
def test_update_without_overlap_is_ddim_update(case, with_noise):
    N, C, T, H, W, F = case
    L, canvas, eps, noise = _case_tensors(case, 3)
    assert H == T
    _, jf, cn, wt = _plan_tensors(L, T, H, "tri")
    a = MH.alphas()
    coef = torch.from_numpy(ddim_coefficients(list(range(0, 1000, 100)), a, 1.0 if with_noise else 0.0).astype(np.float32)).to(G.dev())
    ctr = torch.full((1,), 3, dtype=torch.int32, device=G.dev())
    nz = noise if with_noise else None
    x, x0 = canvas.clone(), torch.full_like(canvas, float("nan"))
    _update(x, eps, nz, x0, jf, cn, None, coef, ctr, (N, W, C, L, T, H, F))  # K = 1 reads no weights
    # the window batch laid out as the canvas: eps_canvas[n][c][j T + tau] = eps[n W + j][c][tau]
    ec = eps.view(N, W, C, T, F).permute(0, 2, 1, 3, 4).reshape(N, C, L, F).contiguous()
    wx, wx0 = canvas.clone(), torch.full_like(canvas, float("nan"))
    _lib.check(_lib.load().ddimx_ddim_update(P(wx), P(ec), P(nz), P(wx0), P(coef), P(ctr), wx.numel(), _lib.stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(x0).all() and torch.equal(x, wx) and torch.equal(x0, wx0)
    assert not torch.equal(x, canvas)


def test_kernels_validate_before_the_launch():
    lib, dev = _lib.load(), G.dev()
    buf = torch.zeros(1 << 16, device=dev)
    ints = torch.zeros(1 << 10, dtype=torch.int32, device=dev)
    coef = torch.tensor([[7.0, 0.6, 0.8, 0.9, 0.4, 0.0]], device=dev)
    good = (2, 3, 2, 64, 32, 16, 8)  # N, W, C, L, T, H, F
    upd = lambda g, wt=buf: lib.ddimx_window_update(P(buf), P(buf), None, P(buf), P(ints), P(ints), P(wt), P(coef), P(ints), *g,  # noqa: E731
                                                    _lib.stream())
    gat = lambda g: lib.ddimx_window_gather(P(buf), P(buf), *g, _lib.stream())  # noqa: E731
    for bad in ((0, 3, 2, 64, 32, 16, 8), (2, 0, 2, 64, 32, 16, 8), (30000, 3, 2, 64, 32, 16, 8), (2, 3, 0, 64, 32, 16, 8),
                (2, 3, 2, 65, 32, 16, 8), (2, 3, 2, 64, 32, 0, 8), (2, 3, 2, 64 + 2, 32, 33, 8), (2, 3, 2, 64, 32, 16, 6),
                (2, 3, 2, 64, 32, 16, 0), (2, 3, 2, 64, 0, 16, 8)):
        assert gat(bad) != 0, bad
        assert b"ddimx_window_gather" in lib.ddimx_last_error()
        assert upd(bad) != 0, bad
        assert b"ddimx_window_update" in lib.ddimx_last_error()
    assert upd((2, 3, 2, 32 + 2 * 3, 32, 3, 8)) != 0 and b"cover" in lib.ddimx_last_error(), "K = 11"
    assert upd(good, None) != 0, "overlap needs the weights"
    assert lib.ddimx_window_gather(None, P(buf), *good, _lib.stream()) != 0
    assert lib.ddimx_window_update(P(buf), None, None, P(buf), P(ints), P(ints), P(buf), P(coef), P(ints), *good, _lib.stream()) != 0
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0, "nothing was launched"
    assert lib.ddimx_abi_version() == 2


# ---- 5. replayed = eager ----------------------------------------------------------------------------------------------------------------
def _run(m, x, coef, n_steps, use_graph, noise, disturb=None, **kw):
    """``MH.stepper_run`` of a WindowStepper on a clone of x (an eager stepper stays on one stream, fork=False: the same bits --
    DESIGN section 9a)."""
    return MH.stepper_run(lambda: WindowStepper(m, x.clone(), coef, 64, 32, "tri", use_graph=use_graph, fork=use_graph, noise=noise, **kw),
                          n_steps, disturb)


@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_replayed_equals_eager(mode, eta):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = list(range(0, 1000, 84))
    assert len(seq) == 12
    coef = ddim_coefficients(seq, a, eta)
    x = synth.gaussian("window.replay", (2, 2, 64 + 2 * 32, 32)).cuda()  # W = 3: six windows, the captured forward forks
    ns = NoiseStream(0xFEED, 5) if eta else None
    eager, c0, g0 = _run(m, x, coef, 12, False, ns)
    graph, c1, g1 = _run(m, x, coef, 12, True, ns)
    assert (c0, g0) == (0, False) and (c1, g1) == (1, True)
    for i in range(12):
        assert torch.equal(eager[i][0], graph[i][0]) and torch.equal(eager[i][1], graph[i][1]), i
    xs, x0 = D.windowed_steps(x.clone(), seq, m, a, None, window=64, hop=32, eta=eta, noise=ns)
    MH.same_list(xs[1:], [o[0] for o in graph], "windowed_steps xs")
    MH.same_list(x0, [o[1] for o in graph], "windowed_steps x0")
    if eta:
        assert not torch.equal(graph[0][0], _run(m, x, ddim_coefficients(seq, a, 0.0), 1, False, None)[0][0][0])


def test_live_graph_sees_load_state_dict():
    """As test_gpu_configs.test_live_graph_sees_load_state_dict_and_in_place_parameter_writes: new weights under the live graph
    are used by the next replay, one capture throughout."""
    cfg, m = MH.build("tiny", MODES[1][0], 3, mode="eval")
    other = synth.fill_module(D.Model(cfg), 11).eval().state_dict()
    first = {k: v.clone() for k, v in m.state_dict().items()}
    a = MH.alphas(cfg)
    seq = list(range(0, 1000, 100))
    coef = ddim_coefficients(seq, a, 0.0)
    x = synth.gaussian("window.live", (2, 2, 128, 32)).cuda()

    def disturb(i):
        if i == 4:
            m.load_state_dict(other)
        if i == 7:
            with torch.no_grad():
                pb = dict(m.named_parameters())["temb.weight.2.bias"]
                pb.copy_(pb * 0.5 + 0.1)

    outs = []
    for graph in (False, True):
        m.load_state_dict(first)
        o, captures, has = _run(m, x, coef, 10, graph, None, disturb)
        assert (captures, has) == ((1, True) if graph else (0, False))
        outs.append(o[-1])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    m.load_state_dict(first)
    plain, _, _ = _run(m, x, coef, 10, False, None)
    assert not torch.equal(plain[-1][0], outs[0][0]), "the updates really changed the trajectory"


# ---- 6. canvas-batch invariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_canvas_does_not_depend_on_its_batch(mode, eta):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = list(range(0, 1000, 125))
    x = synth.gaussian("window.batch", (3, 2, 64 + 3 * 16, 32))
    kw = dict(window=64, hop=16, taper="tri", eta=eta)
    xs, x0 = D.windowed_steps(x.cuda(), seq, m, a, None, noise=NoiseStream(99) if eta else None, **kw)
    for n in range(3):
        sxs, sx0 = D.windowed_steps(x[n:n + 1].cuda(), seq, m, a, None, noise=NoiseStream(99, first_sample=n) if eta else None, **kw)
        for i in range(len(seq)):
            assert torch.equal(xs[i + 1][n:n + 1], sxs[i + 1]) and torch.equal(x0[i][n:n + 1], sx0[i]), (n, i)


# ---- 7. arguments and ownership ---------------------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_anything_is_launched(monkeypatch):
    cfg, m = MH.build("tiny", MODES[0][0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = list(range(0, 1000, 100))
    x = synth.gaussian("window.args", (2, 2, 128, 32)).cuda()
    before = x.clone()
    lib = _lib.load()
    launched = []
    for name in ("ddimx_step_begin", "ddimx_step_begin_ex", "ddimx_window_gather", "ddimx_window_update", "ddimx_unet_fwd", "ddimx_unet_fwd_forked"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *args, _n=name, _r=real: (launched.append(_n), _r(*args))[1])
    for kw, word in [(dict(window=64, hop=0), "hop"), (dict(window=64, hop=65), "hop"), (dict(window=64, hop=7), "hop"),
                     (dict(window=64, hop=48), "L"), (dict(window=256), "L"), (dict(window=66, hop=31), "window"),
                     (dict(window=64, hop=32, taper="cos"), "taper"), (dict(window=64, hop=32, eta=-0.5), "eta")]:
        with pytest.raises(ValueError, match=word):
            D.windowed_steps(x, seq, m, a, None, **kw)
    with pytest.raises(ValueError, match="model"):
        D.windowed_steps(torch.zeros(2, 2, 128, 16, device=G.dev()), seq, m, a, None, window=64)
    with pytest.raises(TypeError):
        D.windowed_steps(x, seq, m, a, None, window=64, noise=torch.randn_like)
    with pytest.raises(ValueError, match="hop"):
        WindowStepper(m, x, ddim_coefficients(seq, a, 0.0), 64, 7)
    torch.cuda.synchronize()
    assert not launched and torch.equal(x, before)
    D.windowed_steps(x, seq[:2], m, a, [-1], window=64)
    assert "ddimx_window_update" in launched and not torch.equal(x, before), "the probe works"


def test_a_dropped_stepper_does_not_disturb_the_next_capture():
    cfg, m = MH.build("tiny", MODES[1][0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = list(range(0, 1000, 100))
    coef = ddim_coefficients(seq, a, 0.0)
    x = synth.gaussian("window.drop", (2, 2, 128, 32)).cuda()
    want, _, _ = _run(m, x, coef, 10, False, None)
    with torch.no_grad():
        st = WindowStepper(m, x.clone(), coef, 64, 32, "tri")
        for _ in range(5):
            st.step()
        assert st.captures == 1 and st.graph is not None
        del st  # no close(): __del__ destroys the graph first, then what it referenced
        gc.collect()
    got, captures, has = _run(m, x, coef, 10, True, None)
    assert (captures, has) == (1, True)
    assert torch.equal(got[-1][0], want[-1][0]) and torch.equal(got[-1][1], want[-1][1])
