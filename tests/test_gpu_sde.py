"""SDE-DPM-Solver++ on the GPU (ddim_audio_amd.dpm_solver_steps(tau > 0), SamplerPool.submit(tau=), ddimxs_multistep_update).

The kernel alone through guarded buffers: its bits against the fp32 mirror of step_math.h (tests/step_math_ref.py) for every combination of the
row's (c1, w1, w2) being zero or not, with and without a history buffer; the draw inside the kernel against the same call fed the
buffer ddimx_noise_fill writes; the rows it shares with ddimx_multistep_update and ddimx_ddim_update against those; refusals.  The
sampler: replayed == eager, order 1 at tau = 1 == generalized_steps(eta=1), tau = 0 == the run without the keyword, shards, a v
model, a clip that never engages, noise_fn, and the trajectory against the published update driving the CPU oracle under
model_harness's gate.  The pool: stochastic solver requests beside DDIM and deterministic ones, each == the request run alone."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, synth
from ddim_audio_amd.schedule import X0Clip, dpm_coefficients, logsnr_seq, v_table
from ddim_audio_amd.solver import MultistepStepper
from oracle import ref_cpu
import kernel_harness as KH
import model_harness as MH
from model_harness import KERNEL_CASES, KERNEL_IDS, MODES, MODE_IDS
import sde_ref as S
import step_math_ref as SM

pytestmark = pytest.mark.gpu

SEED, FIRST, BASE = 0xDEADBEEF12345678, 4000000000, 3  # a seed above 2^32, a sample index above 2^31, a draw base


# ---- the kernel through the C ABI --------------------------------------------------------------------------------------------------------
def _rows():
    """Eight fp32 rows, row k = a third-order tau = 1 row of a real table with c1 / w1 / w2 zeroed unless bit 0 / 1 / 2 of k is set."""
    a = MH.alphas()
    row = dpm_coefficients(logsnr_seq(a, 20), a, 3, tau=1.0)[5].astype(np.float32)
    assert (row[5:] != 0).all()
    rows = np.tile(row, (8, 1))
    for k in range(8):
        for bit, col in enumerate((5, 6, 7)):
            if not k >> bit & 1:
                rows[k, col] = 0.0
    return rows


COMBOS = [(k, h) for k in range(8) for h in (True, False)]  # (row, with a history buffer): all sixteen, at every size


def _inputs(b, per):
    return [synth.gaussian(f"sde.k.{s}.{b}.{per}", (b, per)) for s in "xezpq"]


def _call(xt, e, z, x0, hist, coef, ctr, b, per, seed=0, first=0, base=0):
    rc = KH.lib().ddimxs_multistep_update(xt.ptr, e.ptr, None if z is None else z.ptr, x0.ptr, None if hist is None else hist.ptr,
                                          coef.ptr, ctr.ptr, b, per, seed, first, base, _lib.stream())
    _lib.check(rc)
    KH.sync()


def _outs(x, m1, m2, with_hist):
    return KH.Out(x.numel(), init=x), KH.Out(x.numel(), init=m1), (KH.Out(x.numel(), init=m2) if with_hist else None)


@pytest.mark.parametrize("b, per", KERNEL_CASES, ids=KERNEL_IDS)
def test_kernel_with_a_noise_buffer_gives_the_fp32_restatements_bits(b, per):
    rows = _rows()
    x, e, z, m1, m2 = _inputs(b, per)
    ed, zd, coef = KH.Ro(e), KH.Ro(z), KH.Ro(rows)
    ref = SM.updater32(x.numpy(), e.numpy(), m1.numpy(), m2.numpy(), z=z.numpy())
    for k, with_hist in COMBOS:
        ctr = KH.Ro([k], torch.int32)
        xt, x0, hist = _outs(x, m1, m2, with_hist)
        _call(xt, ed, zd, x0, hist, coef, ctr, b, per)
        want_x, want_0 = ref(rows[k], with_hist)
        what = f"row {k} (c1, w1, w2 = {rows[k, 5:]}), hist {with_hist}"
        KH.same(xt.read("xt").view(b, per), want_x, f"xt, {what}")
        KH.same(x0.read("x0").view(b, per), want_0, f"x0, {what}")
        if with_hist:
            KH.same(hist.read("hist").view(b, per), m1, f"hist <- the old x0, {what}")
        for r in (ed, zd, coef, ctr):
            r.check(what)
        # the terms are really there: the row without this one's noise term gives other bits
        if k & 1:
            assert not np.array_equal(want_x, ref(rows[k & 6], with_hist)[0])


@pytest.mark.parametrize("b, per", KERNEL_CASES, ids=KERNEL_IDS)
def test_kernel_draw_equals_the_noise_fill_and_shared_rows_equal_the_other_update_kernels(b, per):
    lib = KH.lib()
    rows = _rows()
    x, e, _, m1, m2 = _inputs(b, per)
    ed, coef, coef6 = KH.Ro(e), KH.Ro(rows), KH.Ro(rows[:, :6].copy())
    ns = D.NoiseStream(SEED, FIRST)
    n = b * per
    for k, with_hist in COMBOS:
        ctr = KH.Ro([k], torch.int32)
        zbuf = KH.Ro(torch.zeros(b, per))
        ns.fill(zbuf.t, ctr.t, BASE)  # draw index BASE + k
        KH.sync()
        zbuf.keep.copy_(zbuf.t)
        fed = _outs(x, m1, m2, with_hist)
        _call(fed[0], ed, zbuf, fed[1], fed[2], coef, ctr, b, per)
        drawn = _outs(x, m1, m2, with_hist)
        _call(drawn[0], ed, None, drawn[1], drawn[2], coef, ctr, b, per, SEED, FIRST, BASE)
        what = f"row {k}, hist {with_hist}"
        got = [o.read(what) for o in drawn if o is not None]
        want = [o.read(what) for o in fed if o is not None]
        assert all(torch.equal(g, w) for g, w in zip(got, want)), f"{what}: the draw inside the kernel is not the fill's"
        if k & 1:  # and it depends on each word of the noise identity
            for other in ((SEED + 1, FIRST, BASE), (SEED, FIRST + 1, BASE), (SEED, FIRST, BASE + 1)):
                o = _outs(x, m1, m2, with_hist)
                _call(o[0], ed, None, o[1], o[2], coef, ctr, b, per, *other)
                assert not torch.equal(o[0].read(what), got[0]) and torch.equal(o[1].read(what), got[1]), (what, other)
        if not k & 1:  # c1 = 0: ddimx_multistep_update
            o = _outs(x, m1, m2, with_hist)
            _lib.check(lib.ddimx_multistep_update(o[0].ptr, ed.ptr, o[1].ptr, None if o[2] is None else o[2].ptr, coef.ptr, ctr.ptr, n,
                                                  _lib.stream()))
            KH.sync()
            assert all(torch.equal(p.read(what), g) for p, g in zip([v for v in o if v is not None], got)), f"{what}: multistep_update"
        if not k & 6:  # w1 = w2 = 0: ddimx_ddim_update on that noise
            o = _outs(x, m1, m2, False)
            _lib.check(lib.ddimx_ddim_update(o[0].ptr, ed.ptr, zbuf.ptr if k & 1 else None, o[1].ptr, coef6.ptr, ctr.ptr, n, _lib.stream()))
            KH.sync()
            assert torch.equal(o[0].read(what), got[0]) and torch.equal(o[1].read(what), got[1]), f"{what}: ddim_update"
        for r in (ed, zbuf, coef, coef6, ctr):
            r.check(what)


def test_kernel_refuses_bad_arguments_and_writes_nothing():
    lib, st = KH.lib(), _lib.stream()
    b, per = 2, 16
    x, e, z, m1, m2 = _inputs(b, per)
    ed, zd, coef, ctr = KH.Ro(e), KH.Ro(z), KH.Ro(_rows()), KH.Ro([7], torch.int32)
    xt, x0, hist = _outs(x, m1, m2, True)
    keep = [o.t.clone() for o in (xt, x0, hist)]
    good = dict(xt=xt.ptr, eps=ed.ptr, noise=zd.ptr, x0=x0.ptr, hist=hist.ptr, coef=coef.ptr, step=ctr.ptr, B=b, per=per, seed=SEED,
                first=0, base=0)
    bad = [dict(xt=None), dict(eps=None), dict(x0=None), dict(coef=None), dict(step=None), dict(B=0), dict(B=-1), dict(B=65536),
           dict(per=0), dict(per=-16), dict(per=14), dict(per=4 * (2 ** 32 + 1)), dict(first=2 ** 32 - 1), dict(first=2 ** 32 - 1, noise=None)]
    for edit in bad:
        a = dict(good, **edit)
        rc = lib.ddimxs_multistep_update(a["xt"], a["eps"], a["noise"], a["x0"], a["hist"], a["coef"], a["step"], a["B"], a["per"], a["seed"],
                                         a["first"], a["base"], st)
        KH.sync()
        msg = lib.ddimx_last_error().decode(errors="replace")
        assert rc != 0 and "ddimxs_multistep_update" in msg, (edit, rc, msg)
        assert all(torch.equal(o.t, k) for o, k in zip((xt, x0, hist), keep)), f"{edit}: a refused call wrote"
    fresh = KH.Out(b * per), KH.Out(b * per)
    KH.refused(lib.ddimxs_multistep_update(fresh[0].ptr, ed.ptr, None, fresh[1].ptr, None, coef.ptr, ctr.ptr, b, 14, SEED, 0, 0, st), *fresh,
               who="ddimxs_multistep_update")
    # and the same arguments, unedited, are accepted: the last sample index a stream can hold included
    _call(xt, ed, None, x0, hist, coef, ctr, b, per, SEED, 2 ** 32 - b, 2 ** 32 - 1)
    for r in (ed, zd, coef, ctr):
        r.check("refusals")


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------
def _x(tag, cfg, b=4):
    return synth.gaussian(f"sde.{tag}", (b, 2, 32, cfg.model.f_size))  # B = 4: the captured graph forks into two shards


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_replayed_equals_eager(mode, order):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, seq, x = MH.alphas(cfg), MH.spread(10), _x("run", cfg)
    ns = D.NoiseStream(41, 7)
    got = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=1.0, noise=ns)
    assert len(got[0]) == 11 and len(got[1]) == 10
    with MH.eager_steps():
        want = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=1.0, noise=ns)
    MH.same_run(got, want, f"order {order}")
    assert MH.differs(got, D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order)), "the noise matters"
    assert MH.differs(got, D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=1.0, noise=D.NoiseStream(42, 7)))
    assert MH.differs(got, D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=0.5, noise=ns))
    xin = x.cuda()
    again = D.dpm_solver_steps(xin, seq, m, a, [-1], order=order, tau=1.0, noise=ns)
    assert again[0][0] is xin and torch.equal(xin.cpu(), got[0][-1]) and torch.equal(again[0][-1], got[0][-1]), "reproducible, in place"


@pytest.mark.parametrize("n", [3, 10], ids=["eager", "replayed"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_order1_at_tau_one_equals_generalized_steps_at_eta_one(mode, n):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, x = MH.alphas(cfg), _x("o1", cfg)
    seq = list(range(0, 1000, 1000 // n))[:n]
    ns = D.NoiseStream(SEED, FIRST)
    want = D.generalized_steps(x.cuda(), seq, m, a, None, eta=1.0, noise=ns)
    MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=1, tau=1.0, noise=ns), want, "order 1, tau 1")


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_tau_zero_with_a_stream_is_the_run_without_one_and_no_stepper_allocates_a_fill_buffer(mode, order):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, seq, x = MH.alphas(cfg), MH.spread(10), _x("tau0", cfg)
    ns = D.NoiseStream(41, 7)
    want = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order)
    MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=0.0, noise=ns), want, "tau 0")
    with torch.no_grad():
        for tau in (0.0, 1.0):
            st = MultistepStepper(m, x.cuda(), dpm_coefficients(seq, a, order, tau=tau), order, noise=ns)
            assert st.noise_buf is None and st.noise is ns and st.noise_fn is None and st.stochastic == (tau > 0)
            assert (st.hist is not None) == (order == 3)
            st.close()
        with pytest.raises(ValueError, match="noise"):
            MultistepStepper(m, x.cuda(), dpm_coefficients(seq, a, order, tau=1.0), order)


@pytest.mark.parametrize("order", [2, 3])
def test_stochastic_stepper_captures_one_graph_and_replays_it(order):
    """The hot-path claim itself: with a ``NoiseStream`` the tau > 0 step is captured once, after its first eager step, and every
    later step is a replay of that graph -- on the trajectory ``dpm_solver_steps`` returns."""
    cfg, m = MH.build("tiny", MODES[1][0], 5, mode="eval")
    a, seq, x = MH.alphas(cfg), MH.spread(10), _x("cap", cfg)
    ns = D.NoiseStream(41, 7)
    want = D.dpm_solver_steps(x.cuda(), seq, m, a, [-1], order=order, tau=1.0, noise=ns)
    with torch.no_grad():
        st = MultistepStepper(m, x.cuda(), dpm_coefficients(seq, a, order, tau=1.0), order, noise=ns)
        assert st.use_graph and st.graph is None and st.captures == 0
        st.step()
        assert st.graph is not None and st.captures == 1, "captured behind the first, eager step"
        for _ in seq[1:]:
            st.step()
        torch.cuda.synchronize()
        assert st.graph is not None and st.captures == 1 and st.done == len(seq) and st.noise_buf is None
        assert torch.equal(st.xt.cpu(), want[0][-1])
        st.close()
    with MH.eager_steps(), torch.no_grad():
        st = MultistepStepper(m, x.cuda(), dpm_coefficients(seq, a, order, tau=1.0), order, noise=ns)
        st.step()
        st.step()
        assert st.graph is None and st.captures == 0 and not st.use_graph
        st.close()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_four_samples_equal_two_shards_of_two(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, seq, x = MH.alphas(cfg), MH.spread(10), _x("shard", cfg)
    ns = D.NoiseStream(SEED, 2 ** 32 - 4)
    whole = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=1.0, noise=ns)
    for lo in (0, 2):
        part = D.dpm_solver_steps(x[lo:lo + 2].cuda(), seq, m, a, None, order=3, tau=1.0, noise=ns.shard(lo))
        MH.same_run(part, ([v[lo:lo + 2] for v in whole[0]], [v[lo:lo + 2] for v in whole[1]]), f"shard {lo}")
    assert not torch.equal(whole[0][-2][0], whole[0][-2][2])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_v_model_equals_the_wrapped_eps_callable(mode):
    cfg, mv, ms, a = MH.pair("tiny", mode[0])
    seq, x = logsnr_seq(a, 8), _x("v", cfg)
    ns = D.NoiseStream(43, 2)
    got = D.dpm_solver_steps(x.cuda(), seq, mv, a, None, order=2, tau=1.0, noise=ns)
    with MH.eager_steps():  # the callable allocates
        want = D.dpm_solver_steps(x.cuda(), seq, MH.v_wrapped(ms, v_table(a)), a, None, order=2, tau=1.0, noise=ns, prediction="eps")
    MH.same_run(got, want, "v model")
    assert MH.differs(got, D.dpm_solver_steps(x.cuda(), seq, ms, a, None, order=2, tau=1.0, noise=ns)), "the twin reads the output as eps"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_clip_above_every_prediction_is_the_plain_run_and_one_below_is_kept_in_the_history(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, x = MH.alphas(cfg), _x("clip", cfg)
    seq = logsnr_seq(a, 8)
    ns = D.NoiseStream(44, 0)
    plain = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=1.0, noise=ns)
    top = max(float(p.abs().max()) for p in plain[1])
    MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=1.0, noise=ns, threshold=X0Clip(2 * top)), plain, "a high clip")
    limit = float(plain[1][0].abs().flatten().median())
    low = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=1.0, noise=ns, threshold=X0Clip(limit))
    assert MH.differs(low, plain)
    # what comes back is the clipped prediction up to the rewrite's and ddim_x0's roundings: |p| - limit <= u (3 |x| / s2 + 5 limit)
    # + 4 * 2^-126 (the bound test_gpu_threshold.py derives for an engaged clip; the noise does not enter it)
    coef, lim32 = dpm_coefficients(seq, a, 3, tau=1.0), float(np.float32(limit))
    for i, p in enumerate(low[1]):
        xi = (low[0][i] if i else x).double().abs()
        bound = MH.U * (3 * xi / float(np.float32(coef[i, 2])) + 5 * lim32) + 4 * MH.TINY
        assert bool((p.double().abs() - lim32 <= bound).all()), f"x0_preds[{i}] exceeds the clip by more than its roundings"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_noise_fn_returning_the_streams_noise_is_the_in_kernel_run(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, seq, x = MH.alphas(cfg), MH.spread(6), _x("fn", cfg)
    ns = D.NoiseStream(45, 9)
    got = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=1.0, noise=ns)
    calls = []

    def noise_fn(xt):
        calls.append(xt.shape)
        return ns.step_noise(xt.shape, len(calls) - 1, xt.device)

    MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=1.0, noise_fn=noise_fn), got, "noise_fn")
    assert len(calls) == len(seq), "every step asks the host: the run is eager"
    # without either the noise is torch.randn_like from torch's generator
    torch.manual_seed(7)
    default = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=1.0)
    torch.manual_seed(7)
    MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, tau=1.0, noise_fn=torch.randn_like), default, "randn_like")
    assert MH.differs(default, got)


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_trajectory_vs_the_published_update_on_the_cpu_oracle(mode, order):
    """Seven steps at tau = 1 against tests/sde_ref.py's transcription of the published update in float64, over the CPU oracle and
    the float64 normals of the stream's own words, at the gate test_gpu_solver.py puts on its own trajectories."""
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 5, mode="eval")
    a = MH.alphas(cfg)
    seq = logsnr_seq(a, 7)
    assert len(seq) == 7
    live, ocfg = MH.oracle(m, "tiny")
    sd = {k: v.detach() for k, v in live.items()}

    def ref_fn(xn, t):
        with torch.no_grad():
            xt = torch.from_numpy(xn).float()
            return ref_cpu.model_forward(sd, ocfg, xt, torch.full((xt.size(0),), int(t), dtype=torch.long)).double().numpy()

    x = synth.gaussian("sde.ref", (2, 2, 16, 32))
    seed, first = 0x0123456789ABCDEF, 100
    xs, x0 = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=1.0, noise=D.NoiseStream(seed, first))
    rxs, rx0 = S.sde_steps(x.double().numpy(), seq, ref_fn, a, order, 1.0, S.stream_normals(seed, first))
    det, _ = S.sde_steps(x.double().numpy(), seq, ref_fn, a, order, 0.0, None)
    assert np.abs(rxs[-2] - det[-2]).max() > 0.1, "the reference's noise is no small term"
    worst = (0.0, 0.0)
    for i in range(len(seq)):
        mx, er = MH.gate(xs[i + 1], torch.from_numpy(rxs[i + 1]), dt, f"xs[{i + 1}] order {order}")
        worst = max(worst, (mx, er))
        worst = max(worst, MH.gate(x0[i], torch.from_numpy(rx0[i]), dt, f"x0[{i}] order {order}"))
    print(f"[sde vs reference order {order} {MODE_IDS[dt]}] worst max {worst[0]:.3e} rms err {worst[1]:.3e} x rms; "
          f"final max {mx:.3e} rms err {er:.3e} x rms")


# ---- the pool ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_pool_serves_stochastic_solver_requests_beside_the_others_each_as_if_alone(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    reqs = [  # four slots: the first three requests fill them; the others enter slots that these leave
        dict(name="ddim eta 1", steps=5, order=1, eta=1.0, tau=0.0, n=1, seed=0x5EED, first=7),
        dict(name="2m sde", steps=9, order=2, eta=0.0, tau=1.0, n=2, seed=SEED, first=FIRST),
        dict(name="3m sde tau 0.5", steps=12, order=3, eta=0.0, tau=0.5, n=1, seed=0x0123456789ABCDEF, first=100),
        dict(name="ode", steps=7, order=2, eta=0.0, tau=0.0, n=1, seed=None, first=0),
        dict(name="late 3m sde", steps=6, order=3, eta=0.0, tau=1.0, n=1, seed=0x5EED, first=3),
        dict(name="late sde order 1", steps=4, order=1, eta=0.0, tau=2.0, n=1, seed=0x5EED, first=4)]
    pool = D.SamplerPool(m, a, slots=4, t_size=32, max_steps=12)
    tickets, solo = {}, {}
    for r in reqs:
        seq = MH.spread(r["steps"])
        assert len(seq) == r["steps"]
        x = synth.gaussian(f"sde.pool.{r['name']}", (r["n"], 2, 32, cfg.model.f_size))
        ns = D.NoiseStream(r["seed"], r["first"]) if r["seed"] is not None else None
        tickets[r["name"]] = pool.submit(x, seq, eta=r["eta"], order=r["order"], noise=ns, tau=r["tau"])
        rows = []
        for j in range(r["n"]):
            nj = D.NoiseStream(r["seed"], r["first"] + j) if r["seed"] is not None else None
            if r["eta"] > 0:
                out, _ = D.generalized_steps(x[j:j + 1].cuda(), seq, m, a, [-1], eta=r["eta"], noise=nj)
            else:
                out, _ = D.dpm_solver_steps(x[j:j + 1].cuda(), seq, m, a, [-1], order=r["order"], tau=r["tau"], noise=nj)
            rows.append(out[-1][0])
        solo[r["name"]] = torch.stack(rows)
    pool.drain()
    assert pool.stats["captures"] == 1 and pool.stats["busy"] == sum(r["n"] * r["steps"] for r in reqs)
    assert sum(r["n"] for r in reqs) > 4 and pool.stats["steps"] > 12, "the late requests waited for a slot and entered a used one"
    for r in reqs:
        got = tickets[r["name"]].result().cpu()
        for j in range(r["n"]):
            assert torch.equal(got[j], solo[r["name"]][j]), f"request {r['name']!r} sample {j} differs from its run alone"
    pool.close()
    # the stochastic requests really drew: two samples of one request from the same start differ
    x = synth.gaussian("sde.pool.twice", (1, 2, 32, cfg.model.f_size)).repeat(2, 1, 1, 1)
    out, _ = D.dpm_solver_steps(x.cuda(), MH.spread(9), m, a, [-1], order=2, tau=1.0, noise=D.NoiseStream(SEED, FIRST))
    assert not torch.equal(out[-1][0], out[-1][1])
