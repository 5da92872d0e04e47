"""The UniC corrector of DPM-Solver++ on the GPU (ddim_audio_amd.dpm_solver_steps(corrector=True), SamplerPool.submit(corrector=),
windowed_solver_steps(corrector=), ddimxu_multistep_update).

The kernel alone through guarded buffers: its bits against the fp32 mirror of step_math.h (tests/step_math_ref.py) for every combination of the
row's (w1, w2, w3) being zero or not, with no history buffer, one or two -- every buffer whose term is off poisoned, so that a
read of it shows --; the rows it shares with ddimx_multistep_update against that kernel; refusals.  The sampler: replayed ==
eager, one captured graph, the trajectory against the two-pass paper form driving the CPU oracle under model_harness's gate, a v
model, clips.  The pool and the window: a corrector request == the same request run alone / on one window.  corrector=False ==
the run without the keyword."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, synth
from ddim_audio_amd.schedule import X0Clip, dpm_coefficients, logsnr_seq, unic_coefficients, v_table
from ddim_audio_amd.solver import MultistepStepper
import kernel_harness as KH
import model_harness as MH
from model_harness import KERNEL_CASES, KERNEL_IDS, MODES, MODE_IDS
import step_math_ref as SM
import unic_ref as U

pytestmark = pytest.mark.gpu


# ---- the kernel through the C ABI --------------------------------------------------------------------------------------------------------
def _rows():
    """Eight fp32 rows, row k = a third-order corrector row of a real table with w1 / w2 / w3 zeroed unless bit 0 / 1 / 2 of k is
    set."""
    a = MH.alphas()
    row = unic_coefficients(logsnr_seq(a, 20), a, 3)[5].astype(np.float32)
    assert (row[6:] != 0).all() and row[5] == 0
    rows = np.tile(row, (8, 1))
    for k in range(8):
        for bit, col in enumerate((6, 7, 8)):
            if not k >> bit & 1:
                rows[k, col] = 0.0
    return rows


BUFFERS = [(False, False), (True, False), (True, True)]  # (hist, hist2) given
COMBOS = [(k, h, h2) for k in range(8) for h, h2 in BUFFERS]  # all twenty-four, at every size


def _inputs(b, per):
    return [synth.gaussian(f"unic.k.{s}.{b}.{per}", (b, per)) for s in "xepqr"]


def _terms(row, h, h2):
    """Which of (m1, m2, m3) enter u for this row and these buffers."""
    t1, t2, t3 = bool(row[6] != 0), bool(row[7] != 0 and h), bool(row[8] != 0 and h2)
    return t1 or t2, t2 or t3, t3


def _outs(x, m1, m2, m3, row, h, h2):
    """(xt, x0, hist, hist2) as the call finds them, and the bits the history buffers hold on entry: a buffer that no term of this
    row reads is all PATTERN."""
    n = x.numel()
    use = _terms(row, h, h2)
    init = [v if u else MH.sentinel(*x.shape).cpu() for v, u in zip((m1, m2, m3), use)]
    return (KH.Out(n, init=x), KH.Out(n, init=init[0]), KH.Out(n, init=init[1]) if h else None, KH.Out(n, init=init[2]) if h2 else None), init


def _call(outs, e, coef, ctr, n):
    xt, x0, hist, hist2 = outs
    rc = KH.lib().ddimxu_multistep_update(xt.ptr, e.ptr, x0.ptr, None if hist is None else hist.ptr, None if hist2 is None else hist2.ptr,
                                          coef.ptr, ctr.ptr, n, _lib.stream())
    _lib.check(rc)
    KH.sync()


@pytest.mark.parametrize("b, per", KERNEL_CASES, ids=KERNEL_IDS)
def test_kernel_gives_the_fp32_restatements_bits_and_never_reads_a_buffer_whose_term_is_off(b, per):
    rows = _rows()
    x, e, m1, m2, m3 = _inputs(b, per)
    ed, coef = KH.Ro(e), KH.Ro(rows)
    ref = SM.updater32(*(v.numpy() for v in (x, e, m1, m2, m3)))
    for k, h, h2 in COMBOS:
        ctr = KH.Ro([k], torch.int32)
        outs, init = _outs(x, m1, m2, m3, rows[k], h, h2)
        _call(outs, ed, coef, ctr, b * per)
        want_x, want_0 = ref(rows[k], h, h2)
        what = f"row {k} (w1, w2, w3 = {rows[k, 6:]}), hist {h}, hist2 {h2}"
        got_x = outs[0].read("xt").view(b, per)
        assert bool(torch.isfinite(got_x).all()), f"{what}: a poisoned history buffer reached xt"
        KH.same(got_x, want_x, f"xt, {what}")
        KH.same(outs[1].read("x0").view(b, per), want_0, f"x0, {what}")
        if h:
            KH.same(outs[2].read("hist").view(b, per), init[0].view(b, per), f"hist <- the old x0, {what}")
        if h2:
            KH.same(outs[3].read("hist2").view(b, per), init[1].view(b, per), f"hist2 <- the old hist, {what}")
        for r in (ed, coef, ctr):
            r.check(what)
        # the terms are really there: the row without this one's third term gives other bits
        if k & 4 and h2:
            assert not np.array_equal(want_x, ref(rows[k & 3], h, h2)[0])


@pytest.mark.parametrize("b, per", KERNEL_CASES, ids=KERNEL_IDS)
def test_rows_without_a_third_term_equal_multistep_update(b, per):
    """w3 = 0, or no hist2 to take it from: ddimx_multistep_update's bits on the first eight columns, in every buffer."""
    lib = KH.lib()
    rows = _rows()
    x, e, m1, m2, m3 = _inputs(b, per)
    ed, coef, coef8 = KH.Ro(e), KH.Ro(rows), KH.Ro(rows[:, :8].copy())
    for k in range(8):
        for h in (False, True):
            ctr = KH.Ro([k], torch.int32)
            got, _ = _outs(x, m1, m2, m3, rows[k], h, False)
            _call(got, ed, coef, ctr, b * per)
            want, _ = _outs(x, m1, m2, m3, rows[k], h, False)
            _lib.check(lib.ddimx_multistep_update(want[0].ptr, ed.ptr, want[1].ptr, None if want[2] is None else want[2].ptr, coef8.ptr,
                                                  ctr.ptr, b * per, _lib.stream()))
            KH.sync()
            what = f"row {k}, hist {h}"
            for g, w in zip(got[:3], want[:3]):
                if g is not None:
                    KH.same(g.read(what), w.read(what), what)
            for r in (ed, coef, coef8, ctr):
                r.check(what)


def test_kernel_refuses_bad_arguments_and_writes_nothing():
    lib, st = KH.lib(), _lib.stream()
    b, per = 2, 16
    n = b * per
    x, e, m1, m2, m3 = _inputs(b, per)
    rows = _rows()
    ed, coef, ctr = KH.Ro(e), KH.Ro(rows), KH.Ro([7], torch.int32)
    (xt, x0, hist, hist2), _ = _outs(x, m1, m2, m3, rows[7], True, True)
    keep = [o.t.clone() for o in (xt, x0, hist, hist2)]
    good = dict(xt=xt.ptr, eps=ed.ptr, x0=x0.ptr, hist=hist.ptr, hist2=hist2.ptr, coef=coef.ptr, step=ctr.ptr, n=n)
    bad = [dict(xt=None), dict(eps=None), dict(x0=None), dict(coef=None), dict(step=None), dict(n=0), dict(n=-16), dict(n=14), dict(n=n + 2),
           dict(hist=None)]  # the last: hist2 without hist
    for edit in bad:
        a = dict(good, **edit)
        rc = lib.ddimxu_multistep_update(a["xt"], a["eps"], a["x0"], a["hist"], a["hist2"], a["coef"], a["step"], a["n"], st)
        KH.sync()
        msg = lib.ddimx_last_error().decode(errors="replace")
        assert rc != 0 and "ddimxu_multistep_update" in msg, (edit, rc, msg)
        assert all(torch.equal(o.t, k) for o, k in zip((xt, x0, hist, hist2), keep)), f"{edit}: a refused call wrote"
    fresh = KH.Out(n), KH.Out(n), KH.Out(n), KH.Out(n)
    KH.refused(lib.ddimxu_multistep_update(fresh[0].ptr, ed.ptr, fresh[1].ptr, fresh[2].ptr, fresh[3].ptr, coef.ptr, ctr.ptr, 14, st), *fresh,
               who="ddimxu_multistep_update")
    # and the same arguments, unedited, are accepted -- with both history buffers, with one and with none
    _call((xt, x0, hist, hist2), ed, coef, ctr, n)
    _call((xt, x0, hist, None), ed, coef, ctr, n)
    _call((xt, x0, None, None), ed, coef, ctr, n)
    for r in (ed, coef, ctr):
        r.check("refusals")


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------
def _x(tag, cfg, b=4):
    return synth.gaussian(f"unic.{tag}", (b, 2, 32, cfg.model.f_size))  # B = 4: the captured graph forks into two shards


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_replayed_equals_eager(mode, order):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, seq, x = MH.alphas(cfg), MH.spread(10), _x("run", cfg)
    got = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, corrector=True)
    assert len(got[0]) == 11 and len(got[1]) == 10
    with MH.eager_steps():
        want = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, corrector=True)
    MH.same_run(got, want, f"order {order}")
    plain = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order)
    assert MH.differs(got, plain), "the corrector matters"
    assert torch.equal(got[0][1], plain[0][1]) and torch.equal(got[1][0], plain[1][0]), "iteration 0 has nothing to correct"
    assert torch.equal(got[0][-1], got[1][-1]), "the final sample is the last x0 prediction"
    xin = x.cuda()
    again = D.dpm_solver_steps(xin, seq, m, a, [-1], order=order, corrector=True)
    assert again[0][0] is xin and torch.equal(xin.cpu(), got[0][-1]) and torch.equal(again[0][-1], got[0][-1]), "reproducible, in place"


@pytest.mark.parametrize("order", [1, 2, 3])
def test_stepper_captures_one_graph_replays_it_and_owns_a_history_as_deep_as_its_weights(order):
    cfg, m = MH.build("tiny", MODES[1][0], 5, mode="eval")
    a, seq, x = MH.alphas(cfg), MH.spread(10), _x("cap", cfg)
    want = D.dpm_solver_steps(x.cuda(), seq, m, a, [-1], order=order, corrector=True)
    coef = unic_coefficients(seq, a, order)
    with torch.no_grad():
        st = MultistepStepper(m, x.cuda(), coef, order)
        assert st.corrector and not st.stochastic and st.noise_buf is None and st.plan is None
        assert (st.hist is not None) == (order >= 2) and (st.hist2 is not None) == (order == 3)
        assert st.use_graph and st.graph is None and st.captures == 0
        st.step()
        assert st.graph is not None and st.captures == 1, "captured behind the first, eager step"
        for _ in seq[1:]:
            st.step()
        torch.cuda.synchronize()
        assert st.graph is not None and st.captures == 1 and st.done == len(seq)
        assert torch.equal(st.xt.cpu(), want[0][-1])
        st.close()
        if order < 3:  # a weight beyond the order, and a table with noise, are refused
            with pytest.raises(ValueError, match="beyond its order"):
                MultistepStepper(m, x.cuda(), unic_coefficients(seq, a, order + 1), order)
        noisy = coef.copy()
        noisy[2, 5] = 0.1
        with pytest.raises(ValueError, match="no noise"):
            MultistepStepper(m, x.cuda(), noisy, order)


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_trajectory_vs_the_two_pass_paper_form_on_the_cpu_oracle(mode, order):
    """Seven steps against tests/unic_ref.py's two-pass corrector in float64 over the CPU oracle, at the gate test_gpu_solver.py
    puts on its own trajectories of this shape."""
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 5, mode="eval")
    a = MH.alphas(cfg)
    seq = logsnr_seq(a, 7)
    assert len(seq) == 7
    w = np.abs(unic_coefficients(seq, a, order)[:, 6:])
    assert (w[3:6, order - 1] != 0).all(), "the deepest term of the order is at work"
    ref_fn = MH.oracle_eps_np(m)
    x = synth.gaussian("unic.ref", (2, 2, 16, 32))
    xs, x0 = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, corrector=True)
    rxs, rx0 = U.unic_steps(x.double().numpy(), seq, ref_fn, a, order)
    plain, _ = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order)
    worst = (0.0, 0.0)
    for i in range(len(seq)):
        mx, er = MH.gate(xs[i + 1], torch.from_numpy(rxs[i + 1]), dt, f"xs[{i + 1}] order {order}")
        worst = max(worst, (mx, er))
        worst = max(worst, MH.gate(x0[i], torch.from_numpy(rx0[i]), dt, f"x0[{i}] order {order}"))
    moved = float((plain[-2].double() - xs[-2].double()).abs().max() / xs[-2].double().square().mean().sqrt())
    print(f"[unic vs two-pass reference order {order} {MODE_IDS[dt]}] worst max {worst[0]:.3e} rms err {worst[1]:.3e} x rms; "
          f"final max {mx:.3e} rms err {er:.3e} x rms; history weights up to {w.sum(1).max():.3f}; the corrector moves xs[-2] by "
          f"{moved:.3e} x rms")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_v_model_equals_the_wrapped_eps_callable(mode):
    cfg, mv, ms, a = MH.pair("tiny", mode[0])
    seq, x = logsnr_seq(a, 8), _x("v", cfg)
    got = D.dpm_solver_steps(x.cuda(), seq, mv, a, None, order=3, corrector=True)
    with MH.eager_steps():  # the callable allocates
        want = D.dpm_solver_steps(x.cuda(), seq, MH.v_wrapped(ms, v_table(a)), a, None, order=3, corrector=True, prediction="eps")
    MH.same_run(got, want, "v model")
    assert MH.differs(got, D.dpm_solver_steps(x.cuda(), seq, ms, a, None, order=3, corrector=True)), "the twin reads the output as eps"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_clip_above_every_prediction_is_the_plain_corrector_run_and_one_below_is_kept_in_the_history(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, x = MH.alphas(cfg), _x("clip", cfg)
    seq = logsnr_seq(a, 8)
    plain = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, corrector=True)
    top = max(float(p.abs().max()) for p in plain[1])
    MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, corrector=True, threshold=X0Clip(2 * top)), plain, "a high clip")
    limit = float(plain[1][0].abs().flatten().median())
    low = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3, corrector=True, threshold=X0Clip(limit))
    assert MH.differs(low, plain)
    # what comes back is the clipped prediction up to the rewrite's and ddim_x0's roundings: |p| - limit <= u (3 |x| / s2 + 5 limit)
    # + 4 * 2^-126 (the bound test_gpu_threshold.py derives for an engaged clip)
    coef, lim32 = unic_coefficients(seq, a, 3), float(np.float32(limit))
    for i, p in enumerate(low[1]):
        xi = (low[0][i] if i else x).double().abs()
        bound = MH.U * (3 * xi / float(np.float32(coef[i, 2])) + 5 * lim32) + 4 * MH.TINY
        assert bool((p.double().abs() - lim32 <= bound).all()), f"x0_preds[{i}] exceeds the clip by more than its roundings"
    # and the history holds the clipped predictions: every step is the kernel's update of the clipped m0, m1, m2, m3 the run returned
    c32 = coef.astype(np.float32)
    for i in range(3, len(seq) - 1):
        m0, m1, m2, m3 = (low[1][i - j].numpy() for j in range(4))
        s1, s2, s3, c2 = c32[i, 1:5]
        e = ((low[0][i].numpy().astype(np.float64) - np.float64(s2) * m0) / np.float64(s1))  # the eps whose prediction is m0
        u = np.float64(s3) * m0 + np.float64(c2) * e + c32[i, 6] * (m0.astype(np.float64) - m1) + c32[i, 7] * (m1.astype(np.float64) - m2) \
            + c32[i, 8] * (m2.astype(np.float64) - m3)
        err = np.abs(low[0][i + 1].numpy() - u).max()
        assert err <= 1e-4 * max(1.0, np.abs(u).max()), f"xs[{i + 1}] is not the update of the clipped history: {err:.3e}"


# ---- the pool ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_pool_serves_corrector_requests_beside_the_others_each_as_if_alone(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    reqs = [  # four slots: the first three requests fill them; the others enter slots that these leave
        dict(name="ddim eta 1", steps=5, order=1, eta=1.0, corrector=False, n=1, seed=0x5EED, first=7),
        dict(name="unic 2", steps=9, order=2, eta=0.0, corrector=True, n=2, seed=None, first=0),
        dict(name="ode 3", steps=12, order=3, eta=0.0, corrector=False, n=1, seed=None, first=0),
        dict(name="unic 1", steps=7, order=1, eta=0.0, corrector=True, n=1, seed=None, first=0),
        dict(name="late unic 2", steps=6, order=2, eta=0.0, corrector=True, n=1, seed=None, first=0)]
    pool = D.SamplerPool(m, a, slots=4, t_size=32, max_steps=12)
    tickets, solo = {}, {}
    for r in reqs:
        seq = MH.spread(r["steps"])
        assert len(seq) == r["steps"]
        x = synth.gaussian(f"unic.pool.{r['name']}", (r["n"], 2, 32, cfg.model.f_size))
        ns = D.NoiseStream(r["seed"], r["first"]) if r["seed"] is not None else None
        tickets[r["name"]] = pool.submit(x, seq, eta=r["eta"], order=r["order"], noise=ns, corrector=r["corrector"])
        rows = []
        for j in range(r["n"]):
            if r["eta"] > 0:
                out, _ = D.generalized_steps(x[j:j + 1].cuda(), seq, m, a, [-1], eta=r["eta"], noise=D.NoiseStream(r["seed"], r["first"] + j))
            else:
                out, _ = D.dpm_solver_steps(x[j:j + 1].cuda(), seq, m, a, [-1], order=r["order"], corrector=r["corrector"])
            rows.append(out[-1][0])
        solo[r["name"]] = torch.stack(rows)
    pool.drain()
    assert pool.stats["captures"] == 1 and pool.stats["busy"] == sum(r["n"] * r["steps"] for r in reqs)
    assert sum(r["n"] for r in reqs) > 4, "the late requests waited for a slot and entered a used one"
    for r in reqs:
        got = tickets[r["name"]].result().cpu()
        for j in range(r["n"]):
            assert torch.equal(got[j], solo[r["name"]][j]), f"request {r['name']!r} sample {j} differs from its run alone"
    pool.close()
    x = synth.gaussian("unic.pool.unic 2", (2, 2, 32, cfg.model.f_size))
    plain, _ = D.dpm_solver_steps(x[:1].cuda(), MH.spread(9), m, a, [-1], order=2)
    assert not torch.equal(plain[-1][0], solo["unic 2"][0]), "the corrector request is not the plain one"


# ---- the window --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_one_window_is_dpm_solver_steps_with_the_corrector(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = logsnr_seq(a, 8)
    x = synth.gaussian("unic.window.one", (4, 2, 32, 32))
    for order in (1, 2):
        want = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, corrector=True)
        for taper in ("flat", "tri"):
            got = D.windowed_solver_steps(x.cuda(), seq, m, a, None, window=32, taper=taper, order=order, corrector=True)
            assert len(got[0]) == 9 and len(got[1]) == 8 and got[0][1].shape == x.shape
            MH.same_run(got, want, f"order {order} {taper}")
        # the materialised path (a clip that never engages forces the blend into a buffer) runs the same table
        top = max(float(p.abs().max()) for p in want[1])
        MH.same_run(D.windowed_solver_steps(x.cuda(), seq, m, a, None, window=32, order=order, corrector=True, threshold=X0Clip(2 * top)), want,
              f"order {order}, materialised")
    # overlapping windows: replayed == eager, and the corrector matters on the canvas
    canvas = synth.gaussian("unic.window.canvas", (2, 2, 64, 32))
    got = D.windowed_solver_steps(canvas.cuda(), seq, m, a, None, window=32, hop=16, order=2, corrector=True)
    with MH.eager_steps():
        want = D.windowed_solver_steps(canvas.cuda(), seq, m, a, None, window=32, hop=16, order=2, corrector=True)
    MH.same_run(got, want, "overlapping windows")
    assert MH.differs(got, D.windowed_solver_steps(canvas.cuda(), seq, m, a, None, window=32, hop=16, order=2))


# ---- corrector off -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_corrector_false_is_the_run_without_the_keyword_and_allocates_no_second_history(mode, order):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, seq, x = MH.alphas(cfg), MH.spread(10), _x("off", cfg)
    want = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order)
    MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, corrector=False), want, "corrector=False")
    ns = D.NoiseStream(41, 7)
    want = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=1.0, noise=ns)
    MH.same_run(D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=1.0, noise=ns, corrector=False), want, "corrector=False, tau 1")
    with torch.no_grad():
        st = MultistepStepper(m, x.cuda(), dpm_coefficients(seq, a, order), order)
        assert not st.corrector and st.hist2 is None and (st.hist is not None) == (order == 3)
        st.close()
