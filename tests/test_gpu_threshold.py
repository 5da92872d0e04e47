"""x0 clipping and dynamic thresholding on the GPU (ddimxq_x0_quantile, ddimxq_threshold_eps, ``threshold=`` in
``generalized_steps``, ``dpm_solver_steps`` and ``SamplerPool``).

The two exports through the C ABI against tests/threshold_ref.py bit for bit, on guarded outputs: Gaussian data on real table rows
and the data classes that break a radix select; the work buffer across consecutive calls; batch independence; the refusals.  The
samplers: a clip that never engages is the plain run bit for bit, one that engages bounds every returned prediction, the fp32 and
bf16 runs against the float64 restatement driving the CPU oracle, replayed == eager, and the identities order 1 == DDIM, v model ==
wrapped eps callable, pool == alone, all with a threshold on both sides."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, synth
from ddim_audio_amd.schedule import (X0Clip, X0Threshold, ddim_coefficients, dpm_coefficients, logsnr_seq, make_seq, threshold_rank,
                                     v_table)
import gpu_util as G
import kernel_harness as KH
import model_harness as MH
from model_harness import KERNEL_CASES, KERNEL_IDS, MODES, MODE_IDS, ROWS, TINY, U
import step_math_ref as SM
import threshold_ref as TR

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = float("inf")
OWN = 1000  # the test-owned row behind the real table: (s1, s2) = (0, 1), so x0 = x exactly


def _table():
    """(fp32 [1001, 2] on the host, the same on the device): ``v_table`` of the schedule and the row OWN."""
    t32 = np.concatenate([F32(v_table(MH.alphas())), np.array([[0.0, 1.0]], dtype=F32)])
    return t32, KH.Ro(t32)


def _gauss(tag, b, per):
    return synth.gaussian(f"thr.{tag}.x.{b}.{per}", (b, per)).numpy(), synth.gaussian(f"thr.{tag}.e.{b}.{per}", (b, per)).numpy()


def _work(b):
    return torch.zeros(int(KH.lib().ddimxq_quantile_work_bytes(b)), dtype=torch.uint8, device=G.dev())


def _quantile(x, e, tab, rows, rank, floor, ceil, work=None):
    """One ddimxq_x0_quantile call on x, e [b, per] (host arrays, or ``Ro`` inputs already on the device); returns the [b, 2] rows
    read from a guarded output, after checking that the inputs were left alone and that the work buffer is all zeros again."""
    xd, ed = (v if isinstance(v, KH.Ro) else KH.Ro(v) for v in (x, e))
    b, per = xd.t.shape
    td = KH.Ro(np.asarray(rows, dtype=np.int64), torch.int64)
    work = _work(b) if work is None else work
    scale = KH.Out(2 * b)
    _lib.check(KH.lib().ddimxq_x0_quantile(xd.ptr, ed.ptr, tab.ptr, tab.t.size(0), td.ptr, rank, floor, ceil, _lib.ptr(work), scale.ptr,
                                           b, per, _lib.stream()))
    KH.sync()
    got = scale.read("scale").view(b, 2)
    for ro in (xd, ed, td, tab):
        ro.check("ddimxq_x0_quantile")
    assert not bool(work.any()), "the work buffer is not all zeros after the call"
    return got.numpy()


def _want(x, e, t32, rows, rank, floor, ceil):
    return TR.scale_rows(x, e, [t32[r] for r in rows], rank, floor, ceil)


def _ranks(n):
    return sorted({0, n - 1, int(np.floor(0.995 * (n - 1))), int(np.floor(0.5 * (n - 1)))})


# ---- 1. ddimxq_x0_quantile bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,per", KERNEL_CASES, ids=KERNEL_IDS)
def test_quantile_gaussian_on_real_rows(b, per):
    """Gaussian (x, eps) on the table rows ROWS, every rank of the issue, and floor / ceil above, below and between the data so
    that s is the floor, the ceiling and the quantile itself."""
    t32, tab = _table()
    rows = ROWS[:b][::-1] if b < 3 else ROWS
    x, e = _gauss("g", b, per)
    xd, ed = KH.Ro(x), KH.Ro(e)
    x0 = [SM.ddim_x0(x[i], e[i], *t32[row]) for i, row in enumerate(rows)]  # once: the reference of every call below
    seen = set()
    for rank in _ranks(per):
        q = np.array([TR.quantile(p, rank) for p in x0])
        assert np.isfinite(q).all() and (q > 0).all()
        lo, hi = float(q.min()), float(q.max())
        for floor, ceil in ((lo / 4, INF), (hi * 2, INF), (lo / 4, lo / 2), (lo / 4, (lo + hi) / 2 if b > 1 else hi * 2)):
            want = np.array([TR.scale_row(v, floor, None if ceil == INF else ceil) for v in q], dtype=F32)
            KH.same(_quantile(xd, ed, tab, rows, rank, floor, ceil), want, f"rank {rank} floor {floor} ceil {ceil}")
            seen |= {"q" if s == v else ("floor" if s == F32(floor) else "ceil") for (s, _), v in zip(want, q)}
            assert (want[want[:, 0] == F32(floor), 1] == 1.0).all()  # s = floor: r is exactly 1
    assert seen == {"q", "floor", "ceil"}  # every branch of (s, r) was taken


def _classes(n):
    """{name: ([3, n] x with x0 = x on the row OWN, ranks)}: every sample of a batch has other data."""
    rng = np.random.default_rng(2022)
    out = {}
    # five distinct magnitudes, +0 and -0 among them; ranks at the first, an inner and the last index of a tie run
    mags = np.array([0.0, 0.25, 0.5, 1.5, 3.0], dtype=F32)
    xs, ranks = [], set()
    for i in range(3):
        pick = rng.choice(5, size=n, p=np.roll([0.3, 0.1, 0.35, 0.05, 0.2], i))
        pick[:6] = [0, 0, 1, 2, 3, 4]  # every magnitude occurs, the zero with either sign
        sign = rng.choice([-1.0, 1.0], size=n)
        sign[:2] = [1.0, -1.0]
        xs.append((mags[pick] * sign).astype(F32))
    assert all(np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all() for v in xs)
    edges = np.cumsum(np.bincount(np.searchsorted(mags, np.abs(xs[0])), minlength=5))  # sample 0's runs
    for m in range(5):
        first, last = (0 if m == 0 else int(edges[m - 1])), int(edges[m]) - 1
        ranks |= {first, (first + last) // 2, last}
    out["ties"] = (np.stack(xs), sorted(ranks))
    out["all_equal"] = (np.stack([np.full(n, v, dtype=F32) for v in (-1.25, 2.0 ** -140, 7.0)]), [0, n // 2, n - 1])
    # keys base + j: only the last digit differs; (base + j << 10): only the middle one; both with repeats and mixed signs
    j = np.arange(n, dtype=np.uint32)
    for name, shift in (("last_digit", 0), ("middle_digit", 10)):
        keys = [np.uint32(base) + ((rng.permutation(j) % np.uint32(1000 - 7 * i)) << np.uint32(shift))
                for i, base in enumerate((0x3F800000, 0x00000000 if shift else 0x41234400, 0x7F000000))]
        sign = (rng.integers(0, 2, size=(3, n)).astype(np.uint32) << np.uint32(31))
        out[name] = ((np.stack(keys) | sign).view(F32), _ranks(n) + [1, n // 3])
    # denormals, and one +inf: rank n - 1 is the inf
    keys = np.stack([np.uint32(1) + (rng.permutation(j) % np.uint32(5000 + i)) for i in range(3)])
    den = keys.view(F32).copy()
    assert (np.abs(den) < 2.0 ** -126).all() and (den != 0).all()
    den[:, n // 2] = np.inf
    out["denormals_inf"] = (den, [0, n // 2, n - 2, n - 1])
    return out


@pytest.mark.parametrize("n", [20, 4 * 5132], ids=["sub_block", "ragged"])
def test_quantile_on_the_data_that_breaks_a_radix_select(n):
    t32, tab = _table()
    e = _gauss("cls", 3, n)[1]
    for name, (x, ranks) in _classes(n).items():
        assert np.array_equal(TR.bits(SM.ddim_x0(x, e, *t32[OWN])) & TR.ABS, TR.bits(x) & TR.ABS)  # |x0| = |x|, bit for bit
        for rank in ranks:
            for floor, ceil in ((2.0 ** -149, INF), (1.0, INF), (2.0 ** -149, 2.0)):
                got = _quantile(x, e, tab, [OWN] * 3, rank, floor, ceil)
                KH.same(got, _want(x, e, t32, [OWN] * 3, rank, floor, None if ceil == INF else ceil), f"{name} rank {rank} floor {floor}")
        if name == "denormals_inf":
            got = _quantile(x, e, tab, [OWN] * 3, n - 1, 1.0, INF)
            assert np.isinf(got[:, 0]).all() and (got[:, 1] == 0).all()
            got = _quantile(x, e, tab, [OWN] * 3, 0, 2.0 ** -149, INF)
            assert (got[:, 0] < 2.0 ** -126).all() and (got[:, 0] > 0).all()  # a denormal came through


def test_quantile_leaves_the_row_of_a_sample_outside_the_table_alone():
    t32, tab = _table()
    b, per = 3, 4 * 5132
    x, e = _gauss("oob", b, per)
    rank = threshold_rank(0.995, per)
    want = _want(x, e, t32, ROWS, rank, 0.5, None)
    for bad_at, bad_t in ((0, -1), (1, 1001), (2, 2 ** 40)):
        rows = list(ROWS)
        rows[bad_at] = bad_t
        xd, ed, td = KH.Ro(x), KH.Ro(e), KH.Ro(np.asarray(rows, dtype=np.int64), torch.int64)
        work, scale = _work(b), KH.Out(2 * b)
        _lib.check(KH.lib().ddimxq_x0_quantile(xd.ptr, ed.ptr, tab.ptr, 1001, td.ptr, rank, 0.5, INF, _lib.ptr(work), scale.ptr, b, per,
                                               _lib.stream()))
        KH.sync()
        raw = scale.body.view(torch.int32).view(b, 2).cpu()
        for i in range(b):
            if i == bad_at:
                assert bool((raw[i] == -1).all()), f"t = {bad_t}: the row was written"  # four sentinel bytes are the word -1
            else:
                KH.same(raw[i].view(torch.float32), want[i], f"t = {bad_t}: sample {i}")
        assert not bool(work.any())


# ---- 2. one work buffer, consecutive calls ----------------------------------------------------------------------------------------------
def test_one_work_buffer_serves_consecutive_calls():
    t32, tab = _table()
    b, per = 3, 4 * 5132
    work = _work(b)
    for call, rank in enumerate((threshold_rank(0.995, per), 0, per // 2)):
        x, e = _gauss(f"again{call}", b, per)
        got = _quantile(x, e, tab, ROWS, rank, 2.0 ** -100, INF, work=work)
        KH.same(got, _want(x, e, t32, ROWS, rank, 2.0 ** -100, None), f"call {call}")


# ---- 3. a sample alone and as a member of a batch ---------------------------------------------------------------------------------------
def _rewrite(x, e, scale, tab, rows, alias):
    """One ddimxq_threshold_eps call; returns eps_out [b, per] (read from a guarded buffer)."""
    b, per = x.shape
    xd, sd, td = KH.Ro(x), KH.Ro(scale), KH.Ro(np.asarray(rows, dtype=np.int64), torch.int64)
    if alias:
        out = KH.Out(b * per, init=torch.from_numpy(e))
        src = out.ptr
    else:
        out, ed = KH.Out(b * per), KH.Ro(e)
        src = ed.ptr
    _lib.check(KH.lib().ddimxq_threshold_eps(xd.ptr, src, out.ptr, sd.ptr, tab.ptr, tab.t.size(0), td.ptr, b, per, _lib.stream()))
    KH.sync()
    for ro in (xd, sd, td, tab) + (() if alias else (ed,)):
        ro.check("ddimxq_threshold_eps")
    return out


def test_a_sample_is_the_same_alone_and_in_any_place_of_a_batch():
    t32, tab = _table()
    per = 4 * 5132
    x, e = _gauss("member", 3, per)
    rank = threshold_rank(0.9, per)
    solo_s = _quantile(x[:1], e[:1], tab, [412], rank, 0.25, INF)
    solo_e = _rewrite(x[:1], e[:1], solo_s, tab, [412], False).read("eps").numpy()
    assert solo_s[0, 0] > 0.25 and not np.array_equal(TR.bits(solo_e), TR.bits(e[:1].reshape(-1)))  # the threshold engaged
    for place in range(3):
        order = [1, 2]
        order.insert(place, 0)
        rows = [999, 0]
        rows.insert(place, 412)
        xb, eb = x[order], e[order]
        s = _quantile(xb, eb, tab, rows, rank, 0.25, INF)
        KH.same(s[place], solo_s[0], f"(s, r) as member {place}")
        got = _rewrite(xb, eb, s, tab, rows, False).read("eps").view(3, per).numpy()
        KH.same(got[place], solo_e, f"eps' as member {place}")


# ---- 4. ddimxq_threshold_eps bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alias", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("b,per", KERNEL_CASES, ids=KERNEL_IDS)
def test_threshold_eps(b, per, alias):
    """Sample 0: s = floor (r exactly 1), the median of |x0| -- the elements below it keep their eps bits; the others: r < 1."""
    t32, tab = _table()
    rows = ROWS[:b][::-1] if b < 3 else ROWS
    x, e = _gauss("rw", b, per)
    scale = np.empty((b, 2), dtype=F32)
    for i, row in enumerate(rows):
        med = TR.quantile(SM.ddim_x0(x[i], e[i], *t32[row]), per // 2)
        scale[i] = TR.scale_row(med, med if i == 0 else med / 3, None)
    assert scale[0, 1] == 1.0 and (scale[1:, 1] < 1.0).all()
    got = _rewrite(x, e, scale, tab, rows, alias).read("eps").view(b, per).numpy()
    for i, row in enumerate(rows):
        want, keep = TR.rewrite(x[i], e[i], *t32[row], *scale[i])
        KH.same(got[i], want, f"sample {i} (t = {row})")
        if i == 0:
            assert 0.3 * per <= keep.sum() <= 0.7 * per
            assert np.array_equal(TR.bits(got[i])[keep], TR.bits(e[i])[keep]) and (TR.bits(got[i])[~keep] != TR.bits(e[i])[~keep]).any()
            back = SM.ddim_x0(x[i], got[i], *t32[row])
            assert np.isfinite(back).all()


@pytest.mark.parametrize("alias", [False, True], ids=["out_of_place", "in_place"])
def test_threshold_eps_leaves_a_sample_outside_the_table_alone(alias):
    t32, tab = _table()
    b, per = 3, 4 * 5132
    x, e = _gauss("rwoob", b, per)
    scale = np.tile(np.array([[0.5, 1.0]], dtype=F32), (b, 1))
    for bad_at, bad_t in ((0, -1), (1, 1001), (2, -(2 ** 40))):
        rows = list(ROWS)
        rows[bad_at] = bad_t
        out = _rewrite(x, e, scale, tab, rows, alias)
        body = out.body.view(torch.int32).view(b, per).cpu().numpy()
        out.read("eps")  # guards
        for i in range(b):
            if i != bad_at:
                KH.same(body[i].view(F32), TR.rewrite(x[i], e[i], *t32[rows[i]], *scale[i])[0], f"t = {bad_t}: sample {i}")
            elif alias:
                assert np.array_equal(body[i].view(np.uint32), TR.bits(e[i])), f"t = {bad_t}: the sample was written"
            else:
                assert (body[i] == -1).all(), f"t = {bad_t}: the sample was written"


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_exports_validate_before_any_launch():
    lib = KH.lib()
    b, per = 2, 16
    x, e, tab = KH.Ro(np.zeros((b, per), F32)), KH.Ro(np.ones((b, per), F32)), KH.Ro(np.ones((4, 2), F32))
    t, sc_in = KH.Ro(np.zeros(b, np.int64), torch.int64), KH.Ro(np.ones((b, 2), F32))
    st = _lib.stream()

    def quantile(**kw):
        work, scale = KH.Out(int(lib.ddimxq_quantile_work_bytes(b)), torch.uint8), KH.Out(2 * b)
        a = dict(x=x.ptr, eps=e.ptr, tab=tab.ptr, n_table=4, t=t.ptr, rank=3, floor=1.0, ceil=2.0, work=work.ptr, scale=scale.ptr, B=b,
                 per=per)
        a.update(kw)
        rc = lib.ddimxq_x0_quantile(a["x"], a["eps"], a["tab"], a["n_table"], a["t"], a["rank"], a["floor"], a["ceil"], a["work"],
                                    a["scale"], a["B"], a["per"], st)
        KH.refused(rc, work, scale, who="ddimxq_x0_quantile")

    for kw in (dict(x=None), dict(eps=None), dict(tab=None), dict(t=None), dict(work=None), dict(scale=None), dict(B=0), dict(B=65536),
               dict(per=0), dict(per=14), dict(per=-4), dict(per=2 ** 31), dict(rank=-1), dict(rank=per), dict(n_table=0),
               dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(floor=3.0), dict(ceil=float("nan"))):
        quantile(**kw)

    def rewrite(**kw):
        out = KH.Out(b * per)
        a = dict(x=x.ptr, eps_in=e.ptr, eps_out=out.ptr, scale=sc_in.ptr, tab=tab.ptr, n_table=4, t=t.ptr, B=b, per=per)
        a.update(kw)
        rc = lib.ddimxq_threshold_eps(a["x"], a["eps_in"], a["eps_out"], a["scale"], a["tab"], a["n_table"], a["t"], a["B"], a["per"], st)
        KH.refused(rc, out, who="ddimxq_threshold_eps")

    for kw in (dict(x=None), dict(eps_in=None), dict(eps_out=None), dict(scale=None), dict(tab=None), dict(t=None), dict(B=0),
               dict(B=65536), dict(per=0), dict(per=18), dict(per=2 ** 31), dict(n_table=0)):
        rewrite(**kw)
    for ro in (x, e, tab, t, sc_in):
        ro.check("a refused call")


# ---- the samplers ----------------------------------------------------------------------------------------------------------------------
T_LEN = 16
SEQ7 = [0, 140, 290, 450, 620, 800, 999]  # 7 steps: the captured step replays five times


_MODELS = {}


def _model(dtype_str=MODES[0][0]):
    """(cfg, model, alphas) of the tiny network, eval mode, once per mode and process."""
    if dtype_str not in _MODELS:
        cfg, m = MH.build("tiny", dtype_str, 5, mode="eval")
        _MODELS[dtype_str] = (cfg, m, MH.alphas(cfg))
    return _MODELS[dtype_str]


def _x(tag, b, cfg):
    return synth.gaussian(f"thr.{tag}", (b, 2, T_LEN, cfg.model.f_size))


_PLAIN = {}


def _plain(b):
    """The un-thresholded fp32 runs of batch b, once: (x, ddim (xs, x0_preds), solver order 2 (xs, x0_preds), seq of the solver)."""
    if b not in _PLAIN:
        cfg, m, a = _model()
        x, seq2 = _x(f"plain{b}", b, cfg), logsnr_seq(a, 7)
        assert len(seq2) == 7
        _PLAIN[b] = (x, D.generalized_steps(x.cuda(), SEQ7, m, a, None, eta=0.0), D.dpm_solver_steps(x.cuda(), seq2, m, a, None, order=2),
                     seq2)
    return _PLAIN[b]


def _median_limit(b):
    """The median |x0| of the plain DDIM run's first prediction."""
    return float(_plain(b)[1][1][0].abs().flatten().median())


# ---- 6. a clip that never engages ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [3, 5])
def test_a_clip_above_every_prediction_is_the_plain_run(b):
    cfg, m, a = _model()
    x, ddim, dpm, seq2 = _plain(b)
    top = max(float(p.abs().max()) for p in ddim[1] + dpm[1])
    clip = X0Clip(2 * top)
    MH.same_run(D.generalized_steps(x.cuda(), SEQ7, m, a, None, eta=0.0, threshold=clip), ddim, "ddim")
    MH.same_run(D.dpm_solver_steps(x.cuda(), seq2, m, a, None, order=2, threshold=clip), dpm, "solver order 2")
    # the dynamic rule below its floor: s = floor, r = 1, nothing moves
    MH.same_run(D.generalized_steps(x.cuda(), SEQ7, m, a, None, eta=0.0, threshold=X0Threshold(1.0, floor=2 * top)), ddim, "ddim, dynamic")


# ---- 7. a clip that engages -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [3, 5])
def test_an_engaged_clip_bounds_every_returned_prediction(b):
    """What the sampler returns as x0_pred is p = ddim_x0(x, e', s1, s2) with e' = rn(rn(x - s2 c) / s1) for an element the clip
    changed, |c| <= limit (unchanged elements return their own prediction, <= limit as it stands).  With u = 2^-24 and d_i the four
    roundings (the fma and the division of the rewrite, the fma and the division of ddim_x0): s1 e' = (x - s2 c)(1 + d1)(1 + d2),
    so x - s1 e' = s2 c - (x - s2 c)(d1 + d2) to first order, and p = [c - (x / s2 - c)(d1 + d2)](1 + d3 + d4), hence
    |p - c| <= u (2 |x| / s2 + 2 |c| + 2 |c|) = u (2 |x| / s2 + 4 limit).  One more unit on either term covers the second-order
    products, 2^-126 per rounding an underflow: bound = u (3 |x| / s2 + 5 limit) + 4 * 2^-126."""
    cfg, m, a = _model()
    x, ddim, dpm, seq2 = _plain(b)
    limit = _median_limit(b)
    assert limit > 0
    clip = X0Clip(limit)
    lim32 = float(F32(limit))
    for what, plain, got, coef in (("ddim", ddim, D.generalized_steps(x.cuda(), SEQ7, m, a, None, eta=0.0, threshold=clip),
                                    ddim_coefficients(SEQ7, a, 0.0)),
                                   ("solver", dpm, D.dpm_solver_steps(x.cuda(), seq2, m, a, None, order=2, threshold=clip),
                                    dpm_coefficients(seq2, a, 2))):
        assert MH.differs_anywhere(got, plain) and not torch.equal(got[1][0], plain[1][0]), what
        xs, x0 = got
        assert len(x0) == 7
        worst = 0.0
        for i, p in enumerate(x0):
            s2 = float(F32(coef[i, 2]))
            xi = (xs[i] if i else x).double().abs()
            bound = U * (3 * xi / s2 + 5 * lim32) + 4 * TINY
            over = p.double().abs() - lim32
            assert bool((over <= bound).all()), f"{what} x0_preds[{i}]: {float((over / bound).max()):.3f} x the bound over the limit"
            worst = max(worst, float((over / bound).max()))
            if i == 0:  # half of the first prediction sits on the limit, up to the same roundings
                assert float(over.max()) >= -float(bound.max()) and int((over.abs() <= bound).sum()) >= p.numel() // 4
        print(f"[clip {what} B {b}] limit {limit:.4e}, worst excess {worst:.3f} x the rounding bound")


# ---- 8 / 13. against the float64 restatement driving the oracle --------------------------------------------------------------------------
def _gated(got, ref, dt, what):
    (xs, x0), (rxs, rx0) = got, ref
    assert len(xs) == len(rxs) and len(x0) == len(rx0)
    for i in range(len(x0)):
        mx, er = MH.gate(xs[i + 1], torch.from_numpy(rxs[i + 1]), dt, f"{what} xs[{i + 1}]")
        MH.gate(x0[i], torch.from_numpy(rx0[i]), dt, f"{what} x0[{i}]")
    fmx, frms = G.check_close(x0[-1], rx0[-1], dt, f"{what}: the final x0", scale=10.0)  # trajectories x10
    print(f"[threshold vs oracle {what} {MODE_IDS[dt]}] final max {mx:.3e} rms err {er:.3e} x rms; final x0 max {fmx:.3e} rms {frms:.3e} of std")


def _oracle_legs(mode, legs):
    dtype_str, dt = mode
    cfg, m, a = _model(dtype_str)
    rule = X0Threshold(0.9, floor=_median_limit(3))
    x = _x("oracle", 3, cfg)
    ref_fn = MH.oracle_eps_np(m)
    if "ddim0" in legs:
        got = D.generalized_steps(x.cuda(), SEQ7, m, a, None, eta=0.0, threshold=rule)
        ref = TR.generalized_steps(x.double().numpy(), SEQ7, ref_fn, a, 0.0, rule)
        _gated(got, ref, dt, "ddim eta 0")
        assert MH.differs_anywhere(got, D.generalized_steps(x.cuda(), SEQ7, m, a, None, eta=0.0))  # the rule acted
    if "ddim1" in legs:
        ns = D.NoiseStream(2022, 5)
        got = D.generalized_steps(x.cuda(), SEQ7, m, a, None, eta=1.0, noise=ns, threshold=rule)
        ref = TR.generalized_steps(x.double().numpy(), SEQ7, ref_fn, a, 1.0, rule,
                                   noise_fn=lambda k, shape: ns.step_noise(shape, k, G.dev()).cpu().double().numpy())
        _gated(got, ref, dt, "ddim eta 1")
    if "dpm2" in legs:
        seq2 = logsnr_seq(a, 7)
        got = D.dpm_solver_steps(x.cuda(), seq2, m, a, None, order=2, threshold=rule)
        ref = TR.dpm_solver_steps(x.double().numpy(), seq2, ref_fn, a, 2, rule)
        _gated(got, ref, dt, "solver order 2")


@pytest.mark.parametrize("leg", ["ddim0", "ddim1", "dpm2"])
def test_fp32_samplers_vs_the_float64_restatement(leg):
    _oracle_legs(MODES[0], [leg])


def test_bf16_ddim_vs_the_float64_restatement():
    _oracle_legs(MODES[1], ["ddim0"])


# ---- 9. replayed == eager -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [3, 5])
@pytest.mark.parametrize("kind", ["static", "dynamic"])
def test_replayed_equals_eager_and_a_second_run(kind, b):
    cfg, m, a = _model()
    x, _, _, seq2 = _plain(b)
    limit = _median_limit(b)
    rule = X0Clip(limit) if kind == "static" else X0Threshold(0.9, floor=limit)
    runs = {"ddim": lambda: D.generalized_steps(x.cuda(), SEQ7, m, a, None, eta=0.0, threshold=rule),
            "ddim eta 1": lambda: D.generalized_steps(x.cuda(), SEQ7, m, a, None, eta=1.0, noise=D.NoiseStream(7, 3), threshold=rule),
            "solver": lambda: D.dpm_solver_steps(x.cuda(), seq2, m, a, None, order=2, threshold=rule)}
    for what, run in runs.items():
        got = run()
        MH.same_run(run(), got, f"{what}: a second run")
        with MH.eager_steps():
            MH.same_run(run(), got, f"{what}: eager")


# ---- 10. order 1 == DDIM --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["static", "dynamic"])
def test_solver_order_1_is_generalized_steps_with_the_same_threshold(kind):
    cfg, m, a = _model()
    x = _plain(3)[0]
    limit = _median_limit(3)
    rule = X0Clip(limit) if kind == "static" else X0Threshold(0.9, floor=limit)
    got = D.dpm_solver_steps(x.cuda(), SEQ7, m, a, None, order=1, threshold=rule)
    MH.same_run(got, D.generalized_steps(x.cuda(), SEQ7, m, a, None, eta=0.0, threshold=rule), "order 1")
    assert MH.differs_anywhere(got, _plain(3)[1])


# ---- 11. a v model == the eps callable over the same weights -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["static", "dynamic"])
def test_v_model_equals_the_wrapped_eps_callable(kind):
    cfg, mv, ms, a = MH.pair("tiny", MODES[0][0])
    w = MH.v_wrapped(ms, v_table(a), record=True)
    x = _x("v", 5, cfg)
    plain = D.generalized_steps(x.cuda(), SEQ7, mv, a, None, eta=0.0)
    limit = float(plain[1][0].abs().flatten().median())
    rule = X0Clip(limit) if kind == "static" else X0Threshold(0.9, floor=limit)
    got = D.generalized_steps(x.cuda(), SEQ7, mv, a, None, eta=0.0, threshold=rule)
    assert MH.differs_anywhere(got, plain)
    with MH.eager_steps():  # the callable allocates
        want = D.generalized_steps(x.cuda(), SEQ7, w, a, None, eta=0.0, prediction="eps", threshold=rule)
    MH.same_run(got, want, "ddim")
    # the callable's own tensors were read, never rewritten
    assert len(w.outputs) == 7 and all(torch.equal(o, keep) for o, keep in w.outputs)
    seq2 = logsnr_seq(a, 7)
    got = D.dpm_solver_steps(x.cuda(), seq2, mv, a, None, order=2, threshold=rule)
    with MH.eager_steps():
        want = D.dpm_solver_steps(x.cuda(), seq2, w, a, None, order=2, prediction="eps", threshold=rule)
    MH.same_run(got, want, "solver order 2")


# ---- 12. the pool ---------------------------------------------------------------------------------------------------------------------------
def test_pool_request_equals_the_request_alone_with_the_same_threshold():
    cfg, m, a = _model()
    rule = X0Threshold(0.9, floor=_median_limit(3))
    seq2 = logsnr_seq(a, 7)
    reqs = [dict(name="ddim7", n=2, seq=SEQ7, order=1), dict(name="short", n=1, seq=make_seq(1000, 4), order=1),
            dict(name="dpm7", n=2, seq=seq2, order=2)]
    xs = [_x(f"pool.{r['name']}", r["n"], cfg) for r in reqs]
    pool = D.SamplerPool(m, a, slots=4, t_size=T_LEN, max_steps=8, threshold=rule)  # five samples, four slots: slots idle at the end
    tickets = [pool.submit(x, r["seq"], order=r["order"]) for r, x in zip(reqs, xs)]
    pool.drain()
    assert pool.stats["captures"] == 1 and pool.stats["idle"] > 0
    results = [tk.result().cpu() for tk in tickets]
    pool.close()
    for r, x, res in zip(reqs, xs, results):
        for j in range(r["n"]):
            xj = x[j:j + 1].cuda()
            if r["order"] == 1:
                out, _ = D.generalized_steps(xj, r["seq"], m, a, [-1], eta=0.0, threshold=rule)
                off, _ = D.generalized_steps(x[j:j + 1].cuda(), r["seq"], m, a, [-1], eta=0.0)
            else:
                out, _ = D.dpm_solver_steps(xj, r["seq"], m, a, [-1], order=2, threshold=rule)
                off, _ = D.dpm_solver_steps(x[j:j + 1].cuda(), r["seq"], m, a, [-1], order=2)
            assert torch.equal(res[j], out[-1][0]), (r["name"], j)
            assert not torch.equal(res[j], off[-1][0]), (r["name"], j, "the rule did not act")
