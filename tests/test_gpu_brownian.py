"""The Brownian path on the GPU (ddim_audio_amd.BrownianStream, ddimxb_path_fill, ddimxb_multistep_update,
dpm_solver_steps(tau > 0, noise=BrownianStream)).

The path alone: P(t) and the increments of single steps bit for bit against the fp32 restatement of tests/brownian_ref.py fed the
device's own tag-2 normals, and inside that module's running bound against float64 from the Philox words.  The update kernel
through guarded buffers: its bits against tests/step_math_ref.py's update fed the materialised increment, for every zero / non-zero
combination of the row's (c1, w1, w2); rows without noise against ddimxs_multistep_update; refusals.  The sampler: replayed ==
eager, shards, noise_fn fed the materialised increments, a v model, an engaged clip; runs of 20 and 50 steps approach the 200-step
run where a NoiseStream's do not; and the runs that take no path are what the untouched exports give."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, schedule, synth
from ddim_audio_amd.schedule import X0Clip, brownian_clock, brownian_plan, brownian_row, dpm_coefficients, logsnr_seq, v_table
from ddim_audio_amd.solver import MultistepStepper
import brownian_ref as B
import gpu_util as G
import kernel_harness as KH
import model_harness as MH
from model_harness import MODES, MODE_IDS
import step_math_ref as SM

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 8, 16), (5, 2, 32, 256), (8, 1, 1, 4), (3, 2, 37, 4)]
BIG = (8, 2, 1024, 256)  # 131072 float4s a sample, 256 blocks of 256 threads: the grid-stride loop takes two trips
SEEDS = [0, 0x1234, 2 ** 64 - 1]
FIRSTS = [0, 3, 2 ** 32 - 9]
TS = [0, 1, 511, 512, 513, 998, 999]
STEPS = [(999, 950), (1, 0), (512, 511)]
TAU = 1.0
# every (shape, seed, first) of the small shapes; the large one once, with the seed and the first sample that use all 64 / 32 bits
CASES = [(sh, sd, fs) for sh in SHAPES for sd in SEEDS for fs in FIRSTS] + [(BIG, 2 ** 64 - 1, 2 ** 32 - 9)]
CASE_IDS = [f"{'x'.join(map(str, sh))}-{sd:#x}-{fs}" for sh, sd, fs in CASES]


def _gpu_normals(seed, first, shape):
    """``xi(node)``: the fp32 normals the device's own fill writes for counter (., ., node, tag 2), cached per node."""
    ns, memo = D.NoiseStream(seed, first), {}

    def xi(node):
        if node not in memo:
            memo[node] = ns._make(shape, G.dev(), torch.float32, k=node, tag=B.TAG_PATH).cpu().numpy()
        return memo[node]

    return xi


def _points(shape):
    """(timesteps, steps) tested at a shape: all of them, but on the large shape one of the longest descents and the step that ends
    there (what the shape adds is the second trip of the grid-stride loop, not another point)."""
    return (TS, STEPS) if shape != BIG else ([511], [(512, 511)])


def _fill(shape, seed, first, row, kind):
    """ddimxb_path_fill into a guarded buffer."""
    b, per = shape[0], int(np.prod(shape[1:]))
    out, rowd = KH.Out(b * per), KH.Ro(row, torch.int32)
    _lib.check(KH.lib().ddimxb_path_fill(out.ptr, b, per, seed, first, rowd.ptr, kind, _lib.stream()))
    KH.sync()
    rowd.check("the plan row")
    return out.read("ddimxb_path_fill").view(shape).numpy()


# ---- 1. path and increment, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, seed, first", CASES, ids=CASE_IDS)
def test_path_and_increment_have_the_fp32_restatements_bits(shape, seed, first):
    a = MH.alphas()
    u, depth = B.clock(a, TAU)
    clock = brownian_clock(a, TAU)
    xi = _gpu_normals(seed, first, shape)
    bs = D.BrownianStream(seed, first)
    ts, steps = _points(shape)
    memo = {}
    for t in ts:
        got = _fill(shape, seed, first, brownian_row(clock, None, t), _lib.DDIMXB_PATH)
        KH.same(got, B.path32(B.descent(u, depth, t), xi, memo), f"P({t})")
    for i, j in steps:
        got = _fill(shape, seed, first, brownian_row(clock, i, j), _lib.DDIMXB_INCREMENT)
        KH.same(got, B.increment32(B.step_plan(u, depth, i, j), xi, memo), f"z of {i} -> {j}")
        assert got.std() > 0.5 or got.size < 64
    # the object's two methods are that export
    t, (i, j) = ts[-1], steps[-1]
    KH.same(bs.path(shape, t, a, TAU, G.dev()).cpu().numpy(), _fill(shape, seed, first, brownian_row(clock, None, t), _lib.DDIMXB_PATH))
    KH.same(bs.increment(shape, i, j, a, TAU, G.dev()).cpu().numpy(),
            _fill(shape, seed, first, brownian_row(clock, i, j), _lib.DDIMXB_INCREMENT))


def test_path_depends_on_every_word_of_its_identity_and_shards_are_rows():
    a, shape, dev = MH.alphas(), (5, 2, 32, 256), G.dev()
    bs = D.BrownianStream(0x1234, 3)
    p = bs.path(shape, 513, a, TAU, dev)
    for other in (D.BrownianStream(0x1235, 3), D.BrownianStream(0x1234, 4)):
        assert not torch.equal(other.path(shape, 513, a, TAU, dev), p)
    assert not torch.equal(bs.path(shape, 512, a, TAU, dev), p) and not torch.equal(bs.path(shape, 513, a, 0.5, dev), p)
    assert torch.equal(bs.shard(2).path((3,) + shape[1:], 513, a, TAU, dev), p[2:])
    assert torch.equal(bs.shard(2).increment((3,) + shape[1:], 999, 950, a, TAU, dev), bs.increment(shape, 999, 950, a, TAU, dev)[2:])
    assert torch.equal(bs.initial(shape, dev), D.NoiseStream(0x1234, 3).initial(shape, dev)), "the same seed starts from the same x_T"
    # increments of adjacent steps add up to the increment across them, up to the fp32 roundings of the three z
    u, _ = B.clock(a, TAU)
    whole = bs.increment(shape, 999, 900, a, TAU, dev).double() * np.sqrt(u[900] - u[999])
    parts = sum(bs.increment(shape, i, j, a, TAU, dev).double() * np.sqrt(u[j] - u[i]) for i, j in ((999, 950), (950, 900)))
    assert float((whole - parts).abs().max()) <= 64 * MH.U * 6 * np.sqrt(u[900])


# ---- 2. against float64 from the words, inside the running bound ------------------------------------------------------------------------
@pytest.mark.parametrize("shape, seed, first", CASES[:-1], ids=CASE_IDS[:-1])
def test_path_and_increment_stay_inside_the_running_bound(shape, seed, first):
    """|fp32 P(t) - float64 P(t)| <= brownian_ref.path_bound's err, the float64 path taken from the Philox words of the reference;
    the increments likewise (increment_bound).  Prints the worst share of the bound before it asserts."""
    a = MH.alphas()
    u, depth = B.clock(a, TAU)
    xi_r = B.words_normals(seed, first, shape)
    bs = D.BrownianStream(seed, first)
    worst = 0.0
    for t in TS:
        want, bound = B.path_bound(B.descent(u, depth, t), xi_r)
        got = bs.path(shape, t, a, TAU, G.dev()).cpu().numpy().astype(np.float64)
        share = float((np.abs(got - want) / bound).max())
        print(f"P({t}): worst {share:.3f} of the bound")
        worst = max(worst, share)
    for i, j in STEPS:
        want, bound = B.increment_bound(B.step_plan(u, depth, i, j), xi_r)
        got = bs.increment(shape, i, j, a, TAU, G.dev()).cpu().numpy().astype(np.float64)
        share = float((np.abs(got - want) / bound).max())
        print(f"z of {i} -> {j}: worst {share:.3f} of the bound, rms error {np.sqrt(np.mean((got - want) ** 2)):.3e}")
        worst = max(worst, share)
    print(f"[brownian vs float64 {shape} seed {seed:#x} first {first}] worst {worst:.3f} of the bound")
    assert worst <= 1.0


# ---- 3. the update kernel ------------------------------------------------------------------------------------------------------------------
def _rows():
    """Eight fp32 coefficient rows (test_gpu_sde.py's construction, re-stated): row k is a third-order tau = 1 row of a real table with
    c1 / w1 / w2 zeroed unless bit 0 / 1 / 2 of k is set; and the plan beside them: the step STEPS[k mod 3] where c1 != 0, else empty."""
    a = MH.alphas()
    row = dpm_coefficients(logsnr_seq(a, 20), a, 3, tau=TAU)[5].astype(np.float32)
    assert (row[5:] != 0).all()
    rows = np.tile(row, (8, 1))
    plan = np.zeros((8, schedule.BROWNIAN_STRIDE), dtype=np.int32)
    clock = brownian_clock(a, TAU)
    for k in range(8):
        for bit, col in enumerate((5, 6, 7)):
            if not k >> bit & 1:
                rows[k, col] = 0.0
        if k & 1:
            plan[k] = brownian_row(clock, *STEPS[k % 3])
    return rows, plan


COMBOS = [(k, h) for k in range(8) for h in (True, False)]
KSHAPES = [(sh[0], int(np.prod(sh[1:]))) for sh in SHAPES + [BIG]]
SEED, FIRST = 0xDEADBEEF12345678, 4000000000


def _inputs(b, per):
    return [synth.gaussian(f"brownian.k.{s}.{b}.{per}", (b, per)) for s in "xepq"]


def _outs(x, m1, m2, with_hist):
    return KH.Out(x.numel(), init=x), KH.Out(x.numel(), init=m1), (KH.Out(x.numel(), init=m2) if with_hist else None)


def _update(xt, e, x0, hist, coef, plan, ctr, b, per, seed=SEED, first=FIRST):
    _lib.check(KH.lib().ddimxb_multistep_update(xt.ptr, e.ptr, x0.ptr, None if hist is None else hist.ptr, coef.ptr, plan.ptr, ctr.ptr, b,
                                                per, seed, first, _lib.stream()))
    KH.sync()


@pytest.mark.parametrize("b, per", KSHAPES, ids=[f"{b}x{per}" for b, per in KSHAPES])
def test_update_kernel_has_the_fp32_updates_bits_on_the_materialised_increment(b, per):
    lib = KH.lib()
    rows, plan = _rows()
    a = MH.alphas()
    x, e, m1, m2 = _inputs(b, per)
    ed, coef, pland = KH.Ro(e), KH.Ro(rows), KH.Ro(plan, torch.int32)
    bs = D.BrownianStream(SEED, FIRST)
    zs = {k: bs.increment((b, per), *STEPS[k % 3], a, TAU, G.dev()) for k in (1, 3, 5, 7)}
    big = b * per > 1 << 20
    for k, with_hist in ([(7, True), (1, False), (6, True)] if big else COMBOS):
        ctr = KH.Ro([k], torch.int32)
        xt, x0, hist = _outs(x, m1, m2, with_hist)
        _update(xt, ed, x0, hist, coef, pland, ctr, b, per)
        what = f"row {k} (c1, w1, w2 = {rows[k, 5:]}), hist {with_hist}"
        got = [o.read(what).view(b, per) for o in (xt, x0, hist) if o is not None]
        if k & 1:  # c1 != 0: the fp32 update on the increment ddimxb_path_fill materialises
            ref = SM.updater32(x.numpy(), e.numpy(), m1.numpy(), m2.numpy(), z=zs[k].cpu().numpy())
            want_x, want_0 = ref(rows[k], with_hist)
            KH.same(got[0], want_x, f"xt, {what}")
            KH.same(got[1], want_0, f"x0, {what}")
            if with_hist:
                KH.same(got[2], m1, f"hist <- the old x0, {what}")
            assert not np.array_equal(want_x, ref(rows[k & 6], with_hist)[0])
        else:  # c1 = 0, an empty plan row: ddimxs_multistep_update on that row
            o = _outs(x, m1, m2, with_hist)
            _lib.check(lib.ddimxs_multistep_update(o[0].ptr, ed.ptr, None, o[1].ptr, None if o[2] is None else o[2].ptr, coef.ptr, ctr.ptr,
                                                   b, per, SEED, FIRST, 0, _lib.stream()))
            KH.sync()
            want = [v.read(what).view(b, per) for v in o if v is not None]
            assert all(torch.equal(g, w) for g, w in zip(got, want)), f"{what}: not ddimxs_multistep_update's bits"
        for r in (ed, coef, pland, ctr):
            r.check(what)


def test_update_kernel_depends_on_the_noise_identity_and_refuses_bad_arguments():
    lib, st = KH.lib(), _lib.stream()
    b, per = 2, 16
    rows, plan = _rows()
    x, e, m1, m2 = _inputs(b, per)
    ed, coef, pland, ctr = KH.Ro(e), KH.Ro(rows), KH.Ro(plan, torch.int32), KH.Ro([7], torch.int32)

    def run(seed, first):
        o = _outs(x, m1, m2, True)
        _update(*o[:1], ed, *o[1:], coef, pland, ctr, b, per, seed, first)
        return [v.read("identity") for v in o]

    base = run(SEED, FIRST)
    for other in ((SEED + 1, FIRST), (SEED, FIRST + 1)):
        got = run(*other)
        assert not torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]) and torch.equal(got[2], base[2]), other
    xt, x0, hist = _outs(x, m1, m2, True)
    keep = [o.t.clone() for o in (xt, x0, hist)]
    good = dict(xt=xt.ptr, eps=ed.ptr, x0=x0.ptr, hist=hist.ptr, coef=coef.ptr, plan=pland.ptr, step=ctr.ptr, B=b, per=per, first=0)
    bad = [dict(xt=None), dict(eps=None), dict(x0=None), dict(coef=None), dict(plan=None), dict(step=None), dict(B=0), dict(B=-1),
           dict(B=65536), dict(per=0), dict(per=-16), dict(per=14), dict(per=4 * (2 ** 32 + 1)), dict(first=2 ** 32 - 1)]
    for edit in bad:
        g = dict(good, **edit)
        rc = lib.ddimxb_multistep_update(g["xt"], g["eps"], g["x0"], g["hist"], g["coef"], g["plan"], g["step"], g["B"], g["per"], SEED,
                                         g["first"], st)
        KH.sync()
        msg = lib.ddimx_last_error().decode(errors="replace")
        assert rc != 0 and "ddimxb_multistep_update" in msg, (edit, rc, msg)
        assert all(torch.equal(o.t, k) for o, k in zip((xt, x0, hist), keep)), f"{edit}: a refused call wrote"
    fresh = KH.Out(b * per)
    KH.refused(lib.ddimxb_path_fill(fresh.ptr, b, per, SEED, 0, pland.ptr, 2, st), fresh, who="ddimxb_path_fill")
    KH.refused(lib.ddimxb_path_fill(fresh.ptr, b, 14, SEED, 0, pland.ptr, 0, st), fresh, who="ddimxb_path_fill")
    KH.refused(lib.ddimxb_path_fill(fresh.ptr, b, per, SEED, 2 ** 32 - 1, pland.ptr, 0, st), fresh, who="ddimxb_path_fill")
    KH.refused(lib.ddimxb_path_fill(fresh.ptr, b, per, SEED, 0, None, 0, st), fresh, who="ddimxb_path_fill")
    # and the same arguments, unedited, are accepted: the last sample index a stream can hold included
    _update(xt, ed, x0, hist, coef, pland, ctr, b, per, SEED, 2 ** 32 - b)
    for r in (ed, coef, pland, ctr):
        r.check("refusals")


# ---- 4. the sampler ------------------------------------------------------------------------------------------------------------------------
def _x(tag, cfg, b=4):
    return synth.gaussian(f"brownian.{tag}", (b, 2, 32, cfg.model.f_size))


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_replayed_equals_eager_and_one_graph_serves_the_run(mode, order):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, x = MH.alphas(cfg), _x("run", cfg)
    seq = logsnr_seq(a, 10)
    bs = D.BrownianStream(41, 7)
    got = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=TAU, noise=bs)
    assert len(got[0]) == len(seq) + 1 and len(got[1]) == len(seq)
    with MH.eager_steps():
        want = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=TAU, noise=bs)
    MH.same_run(got, want, f"order {order}")
    assert MH.differs(got, D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order)), "the noise matters"
    assert MH.differs(got, D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=TAU, noise=D.BrownianStream(42, 7)))
    assert MH.differs(got, D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=TAU, noise=D.NoiseStream(41, 7)))
    with torch.no_grad():
        st = MultistepStepper(m, x.cuda(), dpm_coefficients(seq, a, order, tau=TAU), order, noise=bs, plan=brownian_plan(seq, a, TAU))
        assert st.use_graph and st.graph is None and st.plan is not None and st.plan.dtype == torch.int32 and st.noise_buf is None
        for _ in seq:
            st.step()
        torch.cuda.synchronize()
        assert st.graph is not None and st.captures == 1 and st.done == len(seq)
        assert torch.equal(st.xt.cpu(), got[0][-1])
        st.close()
        for bad in (None, brownian_plan(seq[1:], a, TAU), brownian_plan(seq, a, 0.0)):
            with pytest.raises(ValueError, match="plan"):
                MultistepStepper(m, x.cuda(), dpm_coefficients(seq, a, order, tau=TAU), order, noise=bs, plan=bad)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_eight_samples_equal_their_shards(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, x = MH.alphas(cfg), _x("shard", cfg, 8)
    seq = logsnr_seq(a, 8)
    bs = D.BrownianStream(SEED, 2 ** 32 - 8)
    whole = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=TAU, noise=bs)
    for bounds in ((0, 4, 8), (0, 3, 6, 8)):
        for lo, hi in zip(bounds, bounds[1:]):
            part = D.dpm_solver_steps(x[lo:hi].cuda(), seq, m, a, None, order=3, tau=TAU, noise=bs.shard(lo))
            MH.same_run(part, ([v[lo:hi] for v in whole[0]], [v[lo:hi] for v in whole[1]]), f"samples {lo}..{hi}")
    assert not torch.equal(whole[0][-2][0], whole[0][-2][2])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_noise_fn_fed_the_materialised_increments_is_the_in_kernel_run(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, x = MH.alphas(cfg), _x("fn", cfg)
    seq = logsnr_seq(a, 7)
    levels = list(reversed(seq))
    bs = D.BrownianStream(45, 9)
    got = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=0.5, noise=bs)
    calls = []

    def noise_fn(xt):
        k = len(calls)
        calls.append(xt.shape)
        if k + 1 == len(levels):
            return torch.zeros_like(xt)  # the final jump adds none
        return bs.increment(xt.shape, levels[k], levels[k + 1], a, 0.5, xt.device)

    MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=0.5, noise_fn=noise_fn), got, "noise_fn")
    assert len(calls) == len(seq)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_v_model_equals_the_wrapped_eps_callable(mode):
    cfg, mv, ms, a = MH.pair("tiny", mode[0])
    seq, x = logsnr_seq(a, 8), _x("v", cfg)
    bs = D.BrownianStream(43, 2)
    got = D.dpm_solver_steps(x.cuda(), seq, mv, a, None, order=2, tau=TAU, noise=bs)
    with MH.eager_steps():  # the callable allocates
        want = D.dpm_solver_steps(x.cuda(), seq, MH.v_wrapped(ms, v_table(a)), a, None, order=2, tau=TAU, noise=bs, prediction="eps")
    MH.same_run(got, want, "v model")
    assert MH.differs(got, D.dpm_solver_steps(x.cuda(), seq, ms, a, None, order=2, tau=TAU, noise=bs)), "the twin reads the output as eps"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_an_engaged_clip_matches_its_own_eager_run(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, x = MH.alphas(cfg), _x("clip", cfg)
    seq = logsnr_seq(a, 8)
    bs = D.BrownianStream(44, 0)
    plain = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=TAU, noise=bs)
    limit = float(plain[1][0].abs().flatten().median())
    low = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=TAU, noise=bs, threshold=X0Clip(limit))
    assert MH.differs(low, plain), "the clip engages"
    with MH.eager_steps():
        MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=TAU, noise=bs, threshold=X0Clip(limit)), low, "clip, eager")


# ---- 5. step-count convergence on the device ----------------------------------------------------------------------------------------------
def test_runs_of_20_and_50_steps_approach_the_200_step_run_on_the_path_and_not_on_a_noise_stream():
    """tests/test_brownian_cpu.py's two gates with the update running in the kernel: the Gaussian model (var 0.25) as a GPU callable,
    order 2, tau = 1, 32768 elements from the seed's x_T.  (20, 200) on the path at most a quarter of (20, 200) with a NoiseStream;
    (50, 200) at most half of (20, 200).  A NoiseStream's 20-step run is unrelated to its 200-step run: above 1 (independent samples
    are sqrt 2 apart), so it fails the first gate against itself by more than the factor four."""
    a, var, seed, shape = MH.alphas(), 0.25, 0x5EED, (2, 2, 32, 256)
    a64 = a.double()
    gain = ((1.0 - a64).sqrt() / (a64 * var + 1.0 - a64)).float().cuda()  # eps(x, t) = gain[t] x
    model = lambda x, t: x * gain[t].view(-1, 1, 1, 1)  # noqa: E731
    bs, ns = D.BrownianStream(seed), D.NoiseStream(seed)
    x_t = bs.initial(shape, G.dev())

    def final(n, noise):
        xs, _ = D.dpm_solver_steps(x_t.clone(), logsnr_seq(a, n), model, a, [-1], order=2, tau=TAU, noise=noise)
        return xs[-1].double()

    dist = lambda p, q: float((p - q).square().mean().sqrt() / q.std())  # noqa: E731
    ref = final(200, bs)
    b20, b50 = dist(final(20, bs), ref), dist(final(50, bs), ref)
    i20 = dist(final(20, ns), final(200, ns))
    print(f"[brownian convergence gpu] distance to the 200-step run / std: on the path 20 steps {b20:.4f}, 50 steps {b50:.4f}; "
          f"NoiseStream 20 steps {i20:.4f}; final std {float(ref.std()):.4f}")
    assert b20 <= 0.25 * i20
    assert b50 <= 0.5 * b20
    assert i20 > 1.0 and not i20 <= 0.25 * i20


# ---- 6. the runs that take no path are what they were -------------------------------------------------------------------------------------
def _by_hand(x, seq, model, a, order, tau, update):
    """The run as a loop over the exports that existed before the path: eps from ``model``, then ``update(xt, eps, x0, hist, coef,
    ctr, k)``; returns (xs, x0_preds) like the sampler."""
    dev = G.dev()
    coef = torch.from_numpy(dpm_coefficients(seq, a, order, tau).astype(np.float32)).to(dev)
    xt = x.to(dev).clone()
    x0, hist = torch.empty_like(xt), (torch.empty_like(xt) if order >= 3 else None)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    xs, x0s = [x], []
    with torch.no_grad():
        for k, t in enumerate(reversed(seq)):
            eps = model(xt, torch.full((xt.size(0),), t, dtype=torch.int64, device=dev))
            update(xt, eps, x0, hist, coef, ctr, k)
            ctr += 1
            xs.append(xt.cpu())
            x0s.append(x0.cpu())
    return xs, x0s


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_runs_without_a_path_are_what_the_untouched_exports_give(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, x = MH.alphas(cfg), _x("old", cfg)
    seq = logsnr_seq(a, 7)
    lib, P = _lib.load(), _lib.ptr
    model = lambda xt, t: m(xt, t, _fork=False).clone()  # noqa: E731
    ns = D.NoiseStream(46, 5)
    b, per = x.size(0), x[0].numel()

    def sde(noise_of):
        def update(xt, eps, x0, hist, coef, ctr, k):
            _lib.check(lib.ddimxs_multistep_update(P(xt), P(eps), P(noise_of(k, xt)), P(x0), P(hist), P(coef), P(ctr), b, per, ns.seed,
                                                   ns.first_sample, 0, _lib.stream()))
        return update

    def ode(xt, eps, x0, hist, coef, ctr, k):
        _lib.check(lib.ddimx_multistep_update(P(xt), P(eps), P(x0), P(hist), P(coef), P(ctr), xt.numel(), _lib.stream()))

    zs = [synth.gaussian(f"brownian.old.z{k}", tuple(x.shape)).cuda() for k in range(len(seq))]
    calls = []

    def noise_fn(xt):
        calls.append(1)
        return zs[len(calls) - 1]

    for order in (2, 3):
        MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=TAU, noise=ns),
              _by_hand(x, seq, model, a, order, TAU, sde(lambda k, xt: None)), f"NoiseStream, order {order}")
        del calls[:]
        MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=TAU, noise_fn=noise_fn),
              _by_hand(x, seq, model, a, order, TAU, sde(lambda k, xt: zs[k])), f"noise_fn, order {order}")
        want = _by_hand(x, seq, model, a, order, 0.0, ode)
        MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order), want, f"tau = 0, order {order}")
        MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=0.0, noise=D.BrownianStream(46, 5)), want,
              f"tau = 0 with a BrownianStream, order {order}")
    with torch.no_grad():  # a path that is given and unused allocates nothing
        st = MultistepStepper(m, x.cuda(), dpm_coefficients(seq, a, 2, tau=0.0), 2, noise=D.BrownianStream(46, 5))
        assert st.plan is None and st.noise_buf is None and not st.stochastic
        st.close()
