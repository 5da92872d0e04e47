"""Windowed multistep sampling on the GPU (ddim_audio_amd.windowed_solver_steps, ddimxw_multistep_update, ddimxw_blend).

The kernels alone through guarded buffers: the blend against the float64 sum inside the bound of its fused-multiply-add chain (a
row one window covers: that window's eps bit for bit); the fused update's bits against tests/step_math_ref.py's fp32 update on the eps
the blend wrote, for every zero / non-zero combination of the row's (c1, w1, w2), with and without a history buffer, noise from a
buffer and drawn in the kernel, and against ddimxw_blend followed by ddimxs_multistep_update; refusals.  The sampler: the
trajectory against the composed float64 reference (tests/window_solver_ref.py) driving the CPU oracle at model_harness's gate; the
convergence conditions of tests/test_window_solver_cpu.py in fp32; the identities with dpm_solver_steps and windowed_steps bit
for bit; replayed == eager; canvas-batch invariance; a BrownianStream against noise_fn fed its increments; clips and the dynamic
threshold on the canvas; graph ownership."""
import functools
import gc

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, synth
from ddim_audio_amd.schedule import X0Clip, X0Threshold, dpm_coefficients, logsnr_seq, v_table, window_plan
from ddim_audio_amd.window import WindowSolverStepper
import gpu_util as G
import kernel_harness as KH
import model_harness as MH
from model_harness import MODES, MODE_IDS, U
import sde_ref as S
import step_math_ref as SM
import threshold_ref as TR
import window_solver_ref as WS

pytestmark = pytest.mark.gpu
TAPERS = ["flat", "tri"]
SEED, FIRST, BASE = 0xDEADBEEF12345678, 4000000000, 3  # a seed above 2^32, a sample index above 2^31, a draw base


# ---- 1. the kernels through the C ABI ---------------------------------------------------------------------------------------------------
# (N, C, T, H, W, F): K = 1, 2, 3, 7, 8; an element count that is no multiple of 1024; a canvas sample that needs 416 blocks where the
# grid gives 409 (2048 / 5), so its last float4s are a second grid-stride pass
KERNEL_CASES = [(2, 2, 32, 32, 3, 32), (2, 2, 32, 16, 4, 32), (3, 2, 32, 12, 4, 12), (2, 1, 32, 5, 9, 8), (2, 2, 32, 4, 10, 4),
                (5, 3, 8, 3, 6, 20), (5, 2, 32, 16, 51, 256),
                (2, 1, 8, 2, 5, 4), (2, 1, 10, 2, 6, 4), (2, 1, 12, 2, 7, 4)]  # the last three: K = 4, 5, 6
# (row, with a history buffer, z drawn in the kernel): row k has c1 / w1 / w2 zeroed unless bit 0 / 1 / 2 of k is set
COMBOS = [(k, h, d) for k in range(8) for h in (True, False) for d in ((False, True) if k & 1 else (False,))]
BIG_COMBOS = [(7, True, True), (1, False, False), (6, True, False), (0, False, False), (3, True, False)]


def _rows():
    a = MH.alphas()
    row = dpm_coefficients(logsnr_seq(a, 20), a, 3, tau=1.0)[5].astype(np.float32)
    assert (row[5:] != 0).all()
    rows = np.tile(row, (8, 1))
    for k in range(8):
        for bit, col in enumerate((5, 6, 7)):
            if not k >> bit & 1:
                rows[k, col] = 0.0
    return rows


class _Case:
    """The tensors of one kernel case: the window batch's eps, the canvas-shaped x, z, m1, m2 and the plan on the device."""

    def __init__(self, case, taper):
        N, C, T, H, W, F = case
        self.L = L = T + (W - 1) * H
        self.geom = (N, W, C, L, T, H, F)
        self.shape, self.n = (N, C, L, F), N * C * L * F
        g = torch.Generator().manual_seed(1 + sum(case))
        self.eps = torch.randn((N * W, C, T, F), generator=g)
        self.x, self.z, self.m1, self.m2 = (torch.randn(self.shape, generator=g) for _ in range(4))
        self.plan = p = window_plan(L, T, H, taper)
        assert p.W == W and p.K == -(-T // H)
        self.epsd = KH.Ro(self.eps)
        self.jf, self.cn, self.wt = KH.Ro(p.jfirst, torch.int32), KH.Ro(p.cnt, torch.int32), KH.Ro(p.wt.copy())

    def blend(self):
        out = KH.Out(self.n)
        _lib.check(KH.lib().ddimxw_blend(self.epsd.ptr, out.ptr, self.jf.ptr, self.cn.ptr, self.wt.ptr, *self.geom, _lib.stream()))
        KH.sync()
        return out.read("ddimxw_blend").view(self.shape)

    def fused(self, xt, noise, x0, hist, coef, ctr, seed=0, first=0, base=0):
        rc = KH.lib().ddimxw_multistep_update(xt.ptr, self.epsd.ptr, None if noise is None else noise.ptr, x0.ptr,
                                              None if hist is None else hist.ptr, self.jf.ptr, self.cn.ptr, self.wt.ptr, coef.ptr, ctr.ptr,
                                              *self.geom, seed, first, base, _lib.stream())
        _lib.check(rc)
        KH.sync()

    def check_inputs(self, what):
        for r in (self.epsd, self.jf, self.cn, self.wt):
            r.check(what)


@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=str)
def test_blend_carries_single_windows_and_stays_inside_the_fma_chain_bound(case, taper):
    """Where one window covers a row the blended eps is that window's eps bit for bit; elsewhere it differs from the float64 sum of
    fp32 weights x fp32 values by at most cnt * 2^-24 * sum_k |w_k eps_k| -- the bound of a cnt-term fused-multiply-add chain that
    tests/test_gpu_window.py derives for ddimx_window_update's blend (term k passes through at most cnt roundings of 2^-24 each)."""
    N, C, T, H, W, F = case
    c = _Case(case, taper)
    p, L = c.plan, c.L
    got = c.blend().double().numpy()
    c.check_inputs("ddimxw_blend")
    e = c.eps.double().numpy().reshape(N, W, C, T, F)
    total, mag, single = np.zeros(c.shape), np.zeros(c.shape), np.zeros(c.shape)
    for row in range(L):
        for k in range(int(p.cnt[row])):
            j = int(p.jfirst[row]) + k
            term = float(p.wt[k, row]) * e[:, j, :, row - j * H, :]
            total[:, :, row], mag[:, :, row] = total[:, :, row] + term, mag[:, :, row] + np.abs(term)
        single[:, :, row] = e[:, int(p.jfirst[row]), :, row - int(p.jfirst[row]) * H, :]
    one = p.cnt == 1
    assert one.any() and np.array_equal(got[:, :, one], single[:, :, one]), "cnt == 1: a select, no multiply"
    many = ~one
    assert many.any() == (H < T)
    if many.any():
        bound = p.cnt.astype(np.float64)[None, None, :, None] * U * mag
        err = np.abs(got - total)
        worst = float((err[:, :, many] / bound[:, :, many]).max())
        print(f"[ddimxw_blend {case} {taper}] K {p.K}: max error / bound {worst:.3f}")
        assert (err[:, :, many] <= bound[:, :, many]).all(), worst


@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=str)
def test_fused_update_has_the_fp32_updates_bits_on_the_blended_eps_and_equals_blend_then_sde_update(case, taper):
    lib = KH.lib()
    c = _Case(case, taper)
    N, n = case[0], c.n
    per = n // N
    rows = _rows()
    coef, zd = KH.Ro(rows), KH.Ro(c.z)
    beps = c.blend()
    bd = KH.Ro(beps)
    x, m1, m2 = (v.numpy().reshape(-1) for v in (c.x, c.m1, c.m2))
    fed = SM.updater32(x, beps.numpy().reshape(-1), m1, m2, z=c.z.numpy().reshape(-1))
    ns = D.NoiseStream(SEED, FIRST)
    nan = np.full(n, np.nan, dtype=np.float32)
    for k, with_hist, drawn in (BIG_COMBOS if n > 1 << 20 else COMBOS):
        what = f"row {k} (c1, w1, w2 = {rows[k, 5:]}), hist {with_hist}, {'drawn' if drawn else 'buffer'}"
        ctr = KH.Ro([k], torch.int32)
        first_iteration = not k & 6  # w1 = w2 = 0: what x0 and hist hold must not enter the result
        ref = fed
        if drawn:  # the buffer ddimx_noise_fill writes for this canvas shape, sample and draw
            zbuf = torch.zeros(c.shape, device=G.dev())
            ns.fill(zbuf, ctr.t, BASE)
            KH.sync()
            ref = SM.updater32(x, beps.numpy().reshape(-1), m1, m2, z=zbuf.cpu().numpy().reshape(-1))
        want_x, want_0 = ref(rows[k], with_hist)
        xt, x0 = KH.Out(n, init=c.x), KH.Out(n, init=nan if first_iteration else c.m1)
        hist = KH.Out(n, init=nan if first_iteration else c.m2) if with_hist else None
        c.fused(xt, None if drawn else zd, x0, hist, coef, ctr, *((SEED, FIRST, BASE) if drawn else (0, 0, 0)))
        got = [xt.read(f"x, {what}"), x0.read(f"x0, {what}")] + ([hist.read(f"hist, {what}")] if with_hist else [])
        KH.same(got[0], want_x, f"x, {what}")
        KH.same(got[1], want_0, f"x0, {what}")
        assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all()), what
        if with_hist:
            KH.same(got[2], nan if first_iteration else m1, f"hist <- the old x0, {what}")
        # the same call in two: ddimxw_blend's canvas eps, then ddimxs_multistep_update on it
        o = [KH.Out(n, init=c.x), KH.Out(n, init=nan if first_iteration else c.m1),
             (KH.Out(n, init=nan if first_iteration else c.m2) if with_hist else None)]
        _lib.check(lib.ddimxs_multistep_update(o[0].ptr, bd.ptr, None if drawn else zd.ptr, o[1].ptr, None if o[2] is None else o[2].ptr,
                                               coef.ptr, ctr.ptr, N, per, *((SEED, FIRST, BASE) if drawn else (0, 0, 0)), _lib.stream()))
        KH.sync()
        for g, w in zip(got, [v.read(what) for v in o if v is not None]):
            KH.same(g, w, f"fused == blend + ddimxs_multistep_update, {what}")
        if k & 1:  # the noise term is there
            assert not np.array_equal(want_x, ref(rows[k & 6], with_hist)[0])
        for r in (coef, zd, bd, ctr):
            r.check(what)
        c.check_inputs(what)


def test_kernels_refuse_bad_arguments_and_write_nothing():
    lib, st = KH.lib(), _lib.stream()
    c = _Case((2, 2, 32, 16, 3, 8), "tri")
    coef, ctr, zd = KH.Ro(_rows()), KH.Ro([7], torch.int32), KH.Ro(c.z)
    xt, x0, hist, be = (KH.Out(c.n) for _ in range(4))
    good = dict(x=xt.ptr, eps=c.epsd.ptr, noise=zd.ptr, x0=x0.ptr, hist=hist.ptr, jf=c.jf.ptr, cn=c.cn.ptr, wt=c.wt.ptr, coef=coef.ptr,
                step=ctr.ptr, N=2, W=3, C=2, L=64, T=32, H=16, F=8, seed=SEED, first=0, base=0)
    shapes = [dict(N=0), dict(W=0), dict(N=30000), dict(C=0), dict(L=65), dict(H=0), dict(L=66, H=33), dict(F=6), dict(F=0), dict(T=0),
              dict(L=32 + 2 * 3, H=3), dict(wt=None)]
    for edit in [dict(x=None), dict(eps=None), dict(x0=None), dict(jf=None), dict(cn=None), dict(coef=None), dict(step=None)] + shapes + [
            dict(first=2 ** 32 - 1), dict(first=2 ** 32 - 1, noise=None)]:
        a = dict(good, **edit)
        rc = lib.ddimxw_multistep_update(a["x"], a["eps"], a["noise"], a["x0"], a["hist"], a["jf"], a["cn"], a["wt"], a["coef"], a["step"],
                                         a["N"], a["W"], a["C"], a["L"], a["T"], a["H"], a["F"], a["seed"], a["first"], a["base"], st)
        KH.refused(rc, xt, x0, hist, who="ddimxw_multistep_update")
    for edit in [dict(eps=None), dict(x=None), dict(jf=None), dict(cn=None)] + shapes:
        a = dict(good, x=be.ptr)
        a.update(edit)
        rc = lib.ddimxw_blend(a["eps"], a["x"], a["jf"], a["cn"], a["wt"], a["N"], a["W"], a["C"], a["L"], a["T"], a["H"], a["F"], st)
        KH.refused(rc, be, who="ddimxw_blend")
    # and the same arguments, unedited, are accepted: the last sample index a stream can hold included
    xt, x0, hist = KH.Out(c.n, init=c.x), KH.Out(c.n, init=c.m1), KH.Out(c.n, init=c.m2)
    c.fused(xt, None, x0, hist, coef, ctr, SEED, 2 ** 32 - 2, 2 ** 32 - 1)
    assert bool(torch.isfinite(xt.read("x")).all()) and lib.ddimx_abi_version() == 2
    for r in (coef, ctr, zd):
        r.check("refusals")
    c.check_inputs("refusals")


# ---- 2. the trajectory against the composed reference -------------------------------------------------------------------------------------
LEGS = {"order2": (2, 0.0), "order3": (3, 0.0), "order2_tau1": (2, 1.0)}
REF_SEED, REF_FIRST = 0x0123456789ABCDEF, 100


@functools.lru_cache(maxsize=None)
def _tiny_reference(H, leg):
    """The float64 reference over the oracle's fp32 forward, once: the same for both activation dtypes of the GPU model."""
    cfg, m = MH.build("tiny", MODES[0][0], 5, mode="eval")
    a = MH.alphas(cfg)
    order, tau = LEGS[leg]
    x = synth.gaussian(f"wsolver.overlap.{H}", (2, 2, 64 + 4 * H, 32))
    seq = logsnr_seq(a, 7)
    assert len(seq) == 7
    xs, x0 = WS.steps(x.double().numpy(), seq, MH.oracle_eps_np(m), a, 64, H, "tri", order, tau, S.stream_normals(REF_SEED, REF_FIRST))
    return x, seq, xs, x0


@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("H", [32, 16, 24])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_trajectory_matches_the_composed_reference_on_the_cpu_oracle(mode, H, leg):
    """Seven logsnr_seq steps on a canvas of five windows against sde_ref.sde_steps over window_ref.blend over the CPU oracle, every
    x and every x0 prediction at model_harness's gate -- the one test_gpu_solver.py and test_gpu_sde.py put on their trajectories."""
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 5, mode="eval")
    a = MH.alphas(cfg)
    order, tau = LEGS[leg]
    x, seq, rxs, rx0 = _tiny_reference(H, leg)
    p = window_plan(x.size(2), 64, H, "tri")
    assert p.W == 5 and p.K == {32: 2, 16: 4, 24: 3}[H]
    xs, x0 = D.windowed_solver_steps(x.cuda(), seq, m, a, None, window=64, hop=H, taper="tri", order=order, tau=tau,
                                     noise=D.NoiseStream(REF_SEED, REF_FIRST) if tau else None)
    assert len(xs) == 8 and len(x0) == 7
    worst = (0.0, 0.0)
    for i in range(7):
        worst = max(worst, MH.gate(xs[i + 1], torch.from_numpy(rxs[i + 1]), dt, f"xs[{i + 1}] {leg} H {H}"))
        worst = max(worst, MH.gate(x0[i], torch.from_numpy(rx0[i]), dt, f"x0[{i}] {leg} H {H}"))
    lim = (2e-3, float("inf")) if dt == G.F32 else (0.6, 5e-2)
    print(f"[windowed solver vs reference {leg} H {H} {MODE_IDS[dt]}] worst max {worst[0]:.3e} rms err {worst[1]:.3e} x rms: "
          f"{worst[0] / lim[0]:.3f} / {worst[1] / lim[1]:.3f} of the gate")


# ---- 3. the convergence conditions on the device ------------------------------------------------------------------------------------------
def _window_gaussians(a, n_windows, n_canvas):
    """The callable of window_solver_ref.window_gaussians on the GPU: sample b of the window batch is window b % W, and window j
    uses the exact Gaussian predictor of variance CONV_VARS[j]: eps = gain[j][t] x."""
    a64 = a.double()
    tab = torch.stack([(1.0 - a64).sqrt() / (a64 * v + 1.0 - a64) for v in WS.CONV_VARS[:n_windows]]).float().to(G.dev())
    j = (torch.arange(n_canvas * n_windows) % n_windows).to(G.dev())
    return lambda x, t: x * tab[j, t].view(-1, 1, 1, 1)


def test_device_repeats_the_convergence_conditions_in_fp32():
    """tests/test_window_solver_cpu.py's experiment with the blend and the update running in the kernels: a [1, 2, 48, 4] canvas,
    T = 16, H = 8, five windows that disagree, against the float64 order-2 run on logsnr_seq(a, 1000).  Errors of 1e-2 sit four
    orders above the fp32 floor."""
    a = MH.alphas()
    seq_of = lambda n: logsnr_seq(a, n)  # noqa: E731
    ref = WS.conv_reference(a, seq_of)
    model = _window_gaussians(a, WS.CONV_W, 1)
    x = torch.from_numpy(WS.conv_start()).float()
    err = {}
    for order, n in ((1, 20), (1, 50), (2, 20), (3, 20)):
        xs, _ = D.windowed_solver_steps(x.cuda(), seq_of(n), model, a, [-1], window=WS.CONV_T, hop=WS.CONV_H, taper=WS.CONV_TAPER,
                                        order=order)
        err[order, n] = WS.rel_l2(xs[-1].double().numpy(), ref)
    print("[windowed solver convergence, gpu fp32] " + "  ".join(f"order {o} at {n} steps {e:.3e}" for (o, n), e in err.items()))
    for what, ratio, bound in WS.conv_conditions(err):
        print(f"[windowed solver convergence, gpu fp32] {what}: ratio {ratio:.3f}")
        assert ratio <= bound, (what, ratio)
    # order 1 is the windowed DDIM run on that grid
    xs, _ = D.windowed_steps(x.cuda(), seq_of(20), model, a, [-1], window=WS.CONV_T, hop=WS.CONV_H, taper=WS.CONV_TAPER)
    assert WS.rel_l2(xs[-1].double().numpy(), ref) == err[1, 20]


# ---- 4. the identities ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_one_window_is_dpm_solver_steps(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = logsnr_seq(a, 8)
    x = synth.gaussian("wsolver.one", (4, 2, 32, 32))
    for order in (1, 2, 3):
        for tau in (0.0, 1.0):
            ns = D.NoiseStream(0xABCD, 1) if tau else None
            want = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=tau, noise=ns)
            for taper in TAPERS:
                got = D.windowed_solver_steps(x.cuda(), seq, m, a, None, window=32, taper=taper, order=order, tau=tau, noise=ns)
                assert len(got[0]) == 9 and len(got[1]) == 8 and got[0][1].shape == x.shape
                MH.same_run(got, want, f"order {order} tau {tau} {taper}")
    # the conventions: xs[0] is the caller's tensor, updated in place; select_index
    xc = x.cuda()
    sel = D.windowed_solver_steps(xc, seq, m, a, [2, -1], window=32, hop=32, order=3, tau=1.0, noise=ns)
    assert sel[0][0] is xc and torch.equal(xc.cpu(), want[0][-1]) and len(sel[0]) == 3 and len(sel[1]) == 2
    assert torch.equal(sel[0][1], want[0][3]) and torch.equal(sel[1][0], want[1][2]) and torch.equal(sel[1][1], want[1][7])
    # the v model
    cfg, mv, ms, a = MH.pair("tiny", mode[0])
    for tau in (0.0, 1.0):
        ns = D.NoiseStream(0xABCD, 1) if tau else None
        want = D.dpm_solver_steps(x.cuda(), seq, mv, a, None, order=2, tau=tau, noise=ns)
        MH.same_run(D.windowed_solver_steps(x.cuda(), seq, mv, a, None, window=32, order=2, tau=tau, noise=ns), want, f"v model tau {tau}")
    assert MH.differs(want, D.windowed_solver_steps(x.cuda(), seq, ms, a, None, window=32, order=2, tau=1.0, noise=ns))


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_no_overlap_is_dpm_solver_steps_over_the_segments_as_a_batch(mode, order):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = logsnr_seq(a, 8)
    T, W, N = 32, 3, 2
    x = synth.gaussian("wsolver.segments", (N, 2, W * T, 32))
    segs = torch.stack([x[n, :, j * T:(j + 1) * T] for n in range(N) for j in range(W)])  # sample 3 n + j
    want_xs, want_x0 = D.dpm_solver_steps(segs.cuda(), seq, m, a, None, order=order)
    for taper in TAPERS:
        xs, x0 = D.windowed_solver_steps(x.cuda(), seq, m, a, None, window=T, hop=T, taper=taper, order=order)
        assert len(xs) == 9 and len(x0) == 8
        for got, want in ((xs[1:], want_xs[1:]), (x0, want_x0)):
            for i, (u, v) in enumerate(zip(got, want)):
                for n in range(N):
                    for j in range(W):
                        assert torch.equal(u[n, :, j * T:(j + 1) * T], v[W * n + j]), (taper, i, n, j)


def _canvas(tag, n=3):
    return synth.gaussian(f"wsolver.{tag}", (n, 2, 96, 32))  # T = 32, H = 16: five windows, K = 2


KW = dict(window=32, hop=16, taper="tri")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_order_one_is_windowed_steps(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    x = _canvas("o1")
    for seq in (list(range(0, 1000, 100)), logsnr_seq(a, 3)):  # replayed, eager
        want = D.windowed_steps(x.cuda(), seq, m, a, None, eta=0.0, **KW)
        MH.same_run(D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=1, **KW), want, "tau 0")
        want = D.windowed_steps(x.cuda(), seq, m, a, None, eta=1.0, noise=D.NoiseStream(SEED, FIRST), **KW)
        MH.same_run(D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=1, tau=1.0, noise=D.NoiseStream(SEED, FIRST), **KW), want, "tau 1")


@pytest.mark.parametrize("leg", ["order2", "order3_tau1", "order3_path", "order2_threshold"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_replayed_equals_eager(mode, leg):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq, x = logsnr_seq(a, 8), _canvas("replay")
    kw = {"order2": dict(order=2), "order3_tau1": dict(order=3, tau=1.0, noise=D.NoiseStream(41, 7)),
          "order3_path": dict(order=3, tau=1.0, noise=D.BrownianStream(41, 7)),
          "order2_threshold": dict(order=2, tau=1.0, noise=D.NoiseStream(41, 7), threshold=X0Threshold(0.9, floor=0.5))}[leg]
    got = D.windowed_solver_steps(x.cuda(), seq, m, a, None, **kw, **KW)
    assert len(got[0]) == 9 and len(got[1]) == 8 and bool(torch.isfinite(got[0][-1]).all())
    with MH.eager_steps():
        want = D.windowed_solver_steps(x.cuda(), seq, m, a, None, **kw, **KW)
    MH.same_run(got, want, leg)
    if "noise" in kw:  # the noise matters, and tau = 0 ignores the stream
        plain = D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=kw["order"], threshold=kw.get("threshold"), **KW)
        assert MH.differs(got, plain)
        MH.same_run(D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=kw["order"], tau=0.0, noise=kw["noise"], threshold=kw.get("threshold"),
                                      **KW), plain, "tau 0 with a stream")


@pytest.mark.parametrize("path", [False, True], ids=["stream", "path"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_canvas_does_not_depend_on_its_batch(mode, path):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq, x = logsnr_seq(a, 6), _canvas("batch")
    make = D.BrownianStream if path else D.NoiseStream
    f = 2 ** 32 - 3  # the last three sample indices a stream holds
    whole = D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=1.0, noise=make(99, f), **KW)
    for n in range(3):
        part = D.windowed_solver_steps(x[n:n + 1].cuda(), seq, m, a, None, order=3, tau=1.0, noise=make(99, f + n), **KW)
        MH.same_run(part, ([v[n:n + 1] for v in whole[0]], [v[n:n + 1] for v in whole[1]]), f"canvas {n}")
    assert not torch.equal(whole[0][-2][0], whole[0][-2][1])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_brownian_run_is_noise_fn_fed_the_paths_increments(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq, x = logsnr_seq(a, 7), _canvas("fn", 2)
    levels = list(reversed(seq))
    bs = D.BrownianStream(45, 9)
    got = D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=0.5, noise=bs, **KW)
    calls = []

    def noise_fn(xt):
        k = len(calls)
        calls.append(tuple(xt.shape))
        if k + 1 == len(levels):
            return torch.zeros_like(xt)  # the final jump adds none
        return bs.increment(xt.shape, levels[k], levels[k + 1], a, 0.5, xt.device)

    MH.same_run(D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=0.5, noise_fn=noise_fn, **KW), got, "noise_fn")
    assert calls == [tuple(x.shape)] * len(seq), "every step asks the host for one canvas-shaped draw: the run is eager"
    # a NoiseStream likewise: the fused kernel's own draw is the stream's canvas-shaped step noise
    ns = D.NoiseStream(45, 9)
    calls.clear()
    got = D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=0.5, noise=ns, **KW)
    fed = D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=0.5,
                                  noise_fn=lambda xt: (calls.append(0), ns.step_noise(xt.shape, len(calls) - 1, xt.device))[1], **KW)
    MH.same_run(fed, got, "noise_fn fed the stream's draws")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_v_model_equals_the_wrapped_eps_callable(mode):
    """Every window's v is converted with the window's own input before the blend: the run equals the one over a callable that
    converts its own output."""
    cfg, mv, ms, a = MH.pair("tiny", mode[0])
    seq, x = logsnr_seq(a, 8), _canvas("v")
    ns = D.NoiseStream(43, 2)
    got = D.windowed_solver_steps(x.cuda(), seq, mv, a, None, order=2, tau=1.0, noise=ns, **KW)
    with MH.eager_steps():  # the callable allocates
        want = D.windowed_solver_steps(x.cuda(), seq, MH.v_wrapped(ms, v_table(a)), a, None, order=2, tau=1.0, noise=ns, prediction="eps", **KW)
    MH.same_run(got, want, "v model")
    assert MH.differs(got, D.windowed_solver_steps(x.cuda(), seq, ms, a, None, order=2, tau=1.0, noise=ns, **KW)), "the twin reads the output as eps"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_clip_above_every_prediction_is_the_plain_run_and_one_below_is_kept_in_the_history(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq, x = logsnr_seq(a, 8), _canvas("clip")
    ns = D.NoiseStream(44, 0)
    run = lambda **kw: D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=1.0, noise=ns, **kw, **KW)  # noqa: E731
    plain = run()
    top = max(float(p.abs().max()) for p in plain[1])
    MH.same_run(run(threshold=X0Clip(2 * top)), plain, "a clip that never engages (the materialised path == the fused one)")
    MH.same_run(run(threshold=X0Threshold(0.5, floor=2 * top)), plain, "a threshold whose floor is above every prediction")
    limit = float(plain[1][0].abs().flatten().median())
    low = run(threshold=X0Clip(limit))
    assert MH.differs(low, plain) and not torch.equal(low[1][0], plain[1][0])
    # what comes back is the clipped prediction of the BLENDED eps up to the rewrite's and ddim_x0's roundings: |p| - limit <=
    # u (3 |x| / s2 + 5 limit) + 4 * 2^-126, the bound test_gpu_threshold.py derives for an engaged clip
    coef, lim32 = dpm_coefficients(seq, a, 3, tau=1.0), float(np.float32(limit))
    for i, p in enumerate(low[1]):
        xi = (low[0][i] if i else x).double().abs()
        bound = U * (3 * xi / float(np.float32(coef[i, 2])) + 5 * lim32) + 4 * MH.TINY
        assert bool((p.double().abs() - lim32 <= bound).all()), f"x0_preds[{i}] exceeds the clip by more than its roundings"
    assert int((low[1][0].double().abs() >= lim32 * (1 - 1e-6)).sum()) >= low[1][0].numel() // 4, "half of the first prediction sits on the limit"
    # the clipped prediction is what the history holds: the run by hand over the exports, x0 / hist never rewritten outside them
    with torch.no_grad():
        st = WindowSolverStepper(m, x.cuda(), coef, 3, 32, 16, "tri", noise=ns, threshold=(X0Clip(limit), v_table(a)))
        try:
            assert st.ceps is not None and st.scale.shape == (3, 2) and st.hist is not None
            for i in range(3):
                before = st.x0.clone()
                st.step()
                assert torch.equal(st.x0.cpu(), low[1][i]) and (i == 0 or torch.equal(st.hist, before)), i
        finally:
            st.close()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_dynamic_threshold_acts_on_the_canvas(mode):
    """X0Threshold against tests/threshold_ref.py's float64 rule -- per canvas sample, on the x0 prediction of the blended eps, the
    rank from the canvas sample's element count -- inside the composed reference over the CPU oracle, at model_harness's gate."""
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 5, mode="eval")
    a = MH.alphas(cfg)
    seq, x = logsnr_seq(a, 7), _canvas("threshold", 2)
    plain = D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=2, **KW)
    rule = X0Threshold(0.9, floor=float(plain[1][0].abs().flatten().median()))
    got = D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=2, threshold=rule, **KW)
    assert MH.differs(got, plain) and not torch.equal(got[1][0], plain[1][0]), "the rule acted"
    rxs, rx0 = TR.dpm_solver_steps(x.double().numpy(), seq, WS.blended(MH.oracle_eps_np(m), 32, 16, "tri"), a, 2, rule)
    worst = (0.0, 0.0)
    for i in range(7):
        worst = max(worst, MH.gate(got[0][i + 1], torch.from_numpy(rxs[i + 1]), dt, f"xs[{i + 1}]"))
        worst = max(worst, MH.gate(got[1][i], torch.from_numpy(rx0[i]), dt, f"x0[{i}]"))
    print(f"[windowed solver, threshold on the canvas {MODE_IDS[dt]}] worst max {worst[0]:.3e} rms err {worst[1]:.3e} x rms")
    # sized from the canvas, not from the window batch
    with torch.no_grad():
        st = WindowSolverStepper(m, x.cuda(), dpm_coefficients(seq, a, 2), 2, 32, 16, "tri", threshold=(rule, v_table(a)))
        try:
            assert st.scale.shape == (2, 2) and st.t.numel() == 10 and st.rank == D.schedule.threshold_rank(0.9, 2 * 96 * 32)
        finally:
            st.close()


# ---- 5. graphs and the Brownian path --------------------------------------------------------------------------------------------------------
def _run(m, x, coef, order, n_steps, use_graph, disturb=None, **kw):
    """``MH.stepper_run`` of a WindowSolverStepper on a clone of x."""
    return MH.stepper_run(lambda: WindowSolverStepper(m, x.clone(), coef, order, 32, 16, "tri", use_graph=use_graph, fork=use_graph, **kw),
                          n_steps, disturb)


@pytest.mark.parametrize("tau", [0.0, 1.0])
def test_one_graph_is_captured_and_replayed_and_nothing_extra_is_allocated(tau):
    cfg, m = MH.build("tiny", MODES[1][0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq, x = logsnr_seq(a, 10), _canvas("cap").cuda()
    ns = D.NoiseStream(41, 7)
    want = D.windowed_solver_steps(x.clone(), seq, m, a, [-1], order=3, tau=tau, noise=ns, **KW)
    coef = dpm_coefficients(seq, a, 3, tau=tau)
    with torch.no_grad():
        st = WindowSolverStepper(m, x.clone(), coef, 3, 32, 16, "tri", noise=ns if tau else None)
        assert st.use_graph and st.graph is None and st.captures == 0
        assert st.noise_buf is None and st.ceps is None and st.plan is None and st.hist is not None and st.stochastic == (tau > 0)
        assert st.win.shape == (15, 2, 32, 32) and st.t.numel() == 15 and st.x0.shape == x.shape
        st.step()
        assert st.graph is not None and st.captures == 1, "captured behind the first, eager step"
        for _ in seq[1:]:
            st.step()
        torch.cuda.synchronize()
        assert st.graph is not None and st.captures == 1 and st.done == len(seq)
        assert torch.equal(st.xt.cpu(), want[0][-1])
        st.close()
        st = WindowSolverStepper(m, x.clone(), dpm_coefficients(seq, a, 2, tau=tau), 2, 32, 16, "tri", noise=ns if tau else None)
        assert st.hist is None and st.ceps is None
        st.close()
    eager, c0, g0 = _run(m, x, coef, 3, 10, False, noise=ns if tau else None)
    graph, c1, g1 = _run(m, x, coef, 3, 10, True, noise=ns if tau else None)
    assert (c0, g0) == (0, False) and (c1, g1) == (1, True)
    for i in range(10):
        assert torch.equal(eager[i][0], graph[i][0]) and torch.equal(eager[i][1], graph[i][1]), i


def test_a_dropped_stepper_does_not_disturb_the_next_capture():
    cfg, m = MH.build("tiny", MODES[1][0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq, x = logsnr_seq(a, 10), _canvas("drop", 2).cuda()
    coef = dpm_coefficients(seq, a, 2, tau=1.0)
    bs = D.BrownianStream(5, 1)
    plan = D.schedule.brownian_plan(seq, a, 1.0)
    want, _, _ = _run(m, x, coef, 2, 10, False, noise=bs, plan=plan)
    with torch.no_grad():
        st = WindowSolverStepper(m, x.clone(), coef, 2, 32, 16, "tri", noise=bs, plan=plan)
        for _ in range(5):
            st.step()
        assert st.captures == 1 and st.graph is not None and st.ceps is not None and st.plan is not None
        del st  # no close(): __del__ destroys the graph first, then what it referenced
        gc.collect()
    got, captures, has = _run(m, x, coef, 2, 10, True, noise=bs, plan=plan)
    assert (captures, has) == (1, True)
    assert torch.equal(got[-1][0], want[-1][0]) and torch.equal(got[-1][1], want[-1][1])


def test_live_graph_sees_load_state_dict():
    cfg, m = MH.build("tiny", MODES[1][0], 3, mode="eval")
    other = synth.fill_module(D.Model(cfg), 11).eval().state_dict()
    first = {k: v.clone() for k, v in m.state_dict().items()}
    a = MH.alphas(cfg)
    seq, x = logsnr_seq(a, 10), _canvas("live", 2).cuda()
    coef = dpm_coefficients(seq, a, 2)

    def disturb(i):
        if i == 4:
            m.load_state_dict(other)

    outs = []
    for graph in (False, True):
        m.load_state_dict(first)
        o, captures, has = _run(m, x, coef, 2, 10, graph, disturb)
        assert (captures, has) == ((1, True) if graph else (0, False))
        outs.append(o[-1])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    m.load_state_dict(first)
    plain, _, _ = _run(m, x, coef, 2, 10, False)
    assert not torch.equal(plain[-1][0], outs[0][0]), "the new weights really changed the trajectory"


def test_runs_of_20_and_50_steps_are_closer_on_the_path_than_on_a_noise_stream():
    """Order 2 at tau = 1 over the windows that disagree: with a BrownianStream the 20- and 50-step runs follow one path and end
    near each other; two NoiseStream runs of different step counts draw unrelated noise."""
    a, seed, shape = MH.alphas(), 0x5EED, (2, 2, 48, 32)
    model = _window_gaussians(a, WS.CONV_W, 2)
    bs, ns = D.BrownianStream(seed), D.NoiseStream(seed)
    x_t = bs.initial(shape, G.dev())

    def final(n, noise):
        xs, _ = D.windowed_solver_steps(x_t.clone(), logsnr_seq(a, n), model, a, [-1], window=WS.CONV_T, hop=WS.CONV_H,
                                        taper=WS.CONV_TAPER, order=2, tau=1.0, noise=noise)
        return xs[-1].double()

    dist = lambda p, q: float((p - q).square().mean().sqrt() / q.std())  # noqa: E731
    on_path, on_stream = dist(final(20, bs), final(50, bs)), dist(final(20, ns), final(50, ns))
    print(f"[windowed solver, brownian] distance of the 20-step final from the 50-step final / std: on the path {on_path:.4f}, "
          f"NoiseStream {on_stream:.4f}: ratio {on_path / on_stream:.4f}")
    assert on_path < on_stream
