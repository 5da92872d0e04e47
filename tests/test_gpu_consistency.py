"""Consistency distillation and consistency sampling on the GPU (include/cmx_consistency.h, ddim_audio_amd/consistency.py).

1. the four kernels through the C ABI; 2. the loss and every parameter gradient against the oracle; 3. ``consistency_target``;
4. ``consistency_step``; 5. ``consistency_steps``.

No tolerance is invented here: bit equality against the fp32 mirrors of tests/consistency_ref.py, rounding bounds counted in the
docstrings, or the project's gates imported from where they live (model_harness.gate, model_harness.backward_case)."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, configs, consistency, synth, train
from ddim_audio_amd.schedule import consistency_coefficients, consistency_pairs, consistency_table, v_table
import consistency_ref as R
import gpu_util as G
import kernel_harness as KH
import model_harness as MH
from model_harness import KERNEL_CASES, KERNEL_IDS, MODES, MODE_IDS, ROWS, TINY, U

pytestmark = pytest.mark.gpu
P, chk = _lib.ptr, _lib.check
F = np.float32
GRID = [0, 3, 500, 870]  # student levels: t_min, one step above the data, mid-schedule, high noise
SEED = 0xC0515


def _dev32(a64):
    return torch.from_numpy(np.ascontiguousarray(a64, dtype=np.float32)).to(G.dev())


def _operand(tag, b, per):
    return synth.gaussian(f"consistency.{tag}.{b}.{per}", (b, per)).numpy()


def _table(pred):
    """(fp32 table on the host, the same on the device): 1000 rows (p, q) of the audio schedule."""
    tab = F(consistency_table(MH.alphas(), pred))
    return tab, _dev32(tab)


def _pq(tab, rows):
    """The rows' (p, q) as [B, 1] fp32 columns."""
    return tab[rows, 0].reshape(-1, 1), tab[rows, 1].reshape(-1, 1)


def _t(rows):
    return torch.tensor(rows, dtype=torch.int64, device=G.dev())


def _upstream(b):
    """An upstream gradient of the [B + 1] loss vector with every entry in use."""
    return np.array([0.25 * (i + 1) for i in range(b)] + [1.0], dtype=F)


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------------
def _out(x, out, tab_d, t, f=None, n_table=None):
    b, per = x.t.shape
    f = KH.Out(b * per) if f is None else f
    chk(KH.lib().cmx_consistency_out(x.ptr, out.ptr, P(tab_d), tab_d.size(0) if n_table is None else n_table, P(t), f.ptr, b, per,
                                     _lib.stream()))
    return f


def _loss(x, out, y, tab_d, t, c=0.0, n_table=None):
    b, per = x.t.shape
    partial, loss = KH.Out(b * 64), KH.Out(b + 1)
    chk(KH.lib().cmx_consistency_loss(x.ptr, out.ptr, y.ptr, P(tab_d), tab_d.size(0) if n_table is None else n_table, P(t), c,
                                      partial.ptr, loss.ptr, b, per, _lib.stream()))
    return loss, partial


def _loss_bwd(x, out, y, tab_d, t, loss, g, c=0.0, n_table=None):
    b, per = x.t.shape
    d = KH.Out(b * per)
    chk(KH.lib().cmx_consistency_loss_bwd(x.ptr, out.ptr, y.ptr, P(tab_d), tab_d.size(0) if n_table is None else n_table, P(t), c,
                                          loss.ptr, g.ptr, d.ptr, b, per, _lib.stream()))
    return d


@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("b,per", KERNEL_CASES, ids=KERNEL_IDS)
def test_out_kernel(b, per, pred):
    """f = fma(q, out, rn(p x)) with the rows of t = [0, 412, 999][:B], bit for bit; row 0 is (1, 0): f is x; f aliasing out gives
    the same bits; the inputs are only read."""
    tab, tab_d = _table(pred)
    rows = ROWS[:b]
    xh, oh = _operand("o.x", b, per), _operand("o.out", b, per)
    x, out, t = KH.Ro(xh), KH.Ro(oh), _t(rows)
    want = R.f32(xh, oh, *_pq(tab, rows))
    got = _out(x, out, tab_d, t).read("f").view(b, per)
    KH.same(got, want, "cmx_consistency_out")
    assert np.isfinite(want).all() and np.array_equal(want[0], xh[0])
    x.check("x")
    out.check("out")
    alias = KH.Out(b * per, init=oh)
    _out(x, alias, tab_d, t, f=alias)
    KH.same(alias.read("f aliasing out").view(b, per), want, "in place")


@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("b,per", KERNEL_CASES, ids=KERNEL_IDS)
def test_loss_kernels(b, per, pred):
    """The loss vector and d_out against the fp32 mirror (the squared-error loss's partition on y - f, then the distance and the
    header's backward scalars), bit for bit, with huber_c = 0 and 0.5; the scratch holds the 64 parts per sample; inputs only read."""
    tab, tab_d = _table(pred)
    rows = ROWS[:b]
    p, q = _pq(tab, rows)
    xh, oh, yh = _operand("l.x", b, per), _operand("l.out", b, per), _operand("l.y", b, per)
    gh = _upstream(b)
    x, out, y, g, t = KH.Ro(xh), KH.Ro(oh), KH.Ro(yh), KH.Ro(gh), _t(rows)
    for c in (0.0, 0.5):
        loss, partial = _loss(x, out, y, tab_d, t, c)
        d = _loss_bwd(x, out, y, tab_d, t, loss, g, c)
        got = loss.read(f"loss c={c}")
        want = R.loss32(xh, oh, yh, p, q, c)
        KH.same(got, want, f"cmx_consistency_loss c={c}")
        assert np.isfinite(want).all() and bool(torch.isfinite(partial.read("partial")).all())
        KH.same(d.read(f"d_out c={c}").view(b, per), R.loss_bwd32(xh, oh, yh, p, q, gh, want, c), f"cmx_consistency_loss_bwd c={c}")
    for ro in (x, out, y, g):
        ro.check("an input")


@pytest.mark.parametrize("b,per", KERNEL_CASES, ids=KERNEL_IDS)
def test_identity_table_gives_the_squared_error_kernels(b, per):
    """With rows (0, 1) and huber_c = 0, f is out: loss and backward are ddimx_sqerr_loss(y, out) / ddimx_sqerr_loss_bwd_mean."""
    lib, dev = KH.lib(), G.dev()
    xh, oh, yh = _operand("i.x", b, per), _operand("i.out", b, per), _operand("i.y", b, per)
    x, out, y, g, t = KH.Ro(xh), KH.Ro(oh), KH.Ro(yh), KH.Ro(_upstream(b)), _t(ROWS[:b])
    ident = torch.tensor([[0.0, 1.0]] * 1000, device=dev)
    loss, _ = _loss(x, out, y, ident, t)
    d = _loss_bwd(x, out, y, ident, t, loss, g)
    partial = torch.empty(b * 64, device=dev)
    want_loss, want_d = MH.sentinel(1, b + 1)[0], MH.sentinel(b, per)
    chk(lib.ddimx_sqerr_loss(y.ptr, out.ptr, P(partial), P(want_loss), b, per, _lib.stream()))
    chk(lib.ddimx_sqerr_loss_bwd_mean(y.ptr, out.ptr, g.ptr, P(want_d), b, per, _lib.stream()))
    torch.cuda.synchronize()
    assert torch.equal(loss.read("loss"), want_loss.cpu()) and torch.equal(d.read("d").view(b, per), want_d.cpu())
    assert bool(torch.isfinite(want_loss).all()) and bool(torch.isfinite(want_d).all())


@pytest.mark.parametrize("near", [False, True], ids=["S>>c2", "S<<c2"])
@pytest.mark.parametrize("b,per", KERNEL_CASES[:2], ids=KERNEL_IDS[:2])
def test_pseudo_huber_against_float64(b, per, near):
    """huber_c = 0.5 against float64 on the kernel's own fp32 sums S_b (the huber_c = 0 output: that path is bit-checked above), for
    ordinary operands (S >= 10 c^2) and for y within 1e-4 of f (S <= c^2 / 100, where sqrt(S + c^2) - c would cancel).

    Forward, L = S / (sqrt(S + c^2) + c): c^2 and S + c^2 are rounded (relative error of the sum <= 2 u), the root halves that and
    rounds (2 u), adding c rounds (the denominator: <= 3 u), the division rounds (4 u): |L - L64| <= 5 (u L + 2^-126), one unit spare.
    Backward, d = cq (f - y), cq = rn(q k), k = rn(c0 / rn(2 rn(L + c))), c0 recomputed here with the kernel's fp32 operations:
    L + c stands for sqrt(S + c^2) with L's 4 u and its own rounding (5 u; L <= the root), the doubling is exact, the division
    and the product q k round (7 u on cq).  f = fma(q, out, rn(p x)) errs by u (|p x| + |f|), the difference by u |f - y|, the last
    product by u |d|: |d - d64| <= |cq| u (|p x| + |f| + |f - y|) + 8 u |d| <= 10 (u |cq| (|p x| + |f| + |f - y|) + 2^-126)."""
    c = 0.5
    tab, tab_d = _table("v")
    rows = ROWS[:b]
    p, q = _pq(tab, rows)
    xh, oh = _operand("h.x", b, per), _operand("h.out", b, per)
    yh = _operand("h.y", b, per)
    if near:
        yh = (R.f32(xh, oh, p, q) + F(1e-4) * yh).astype(F)
    gh = _upstream(b)
    x, out, y, g, t = KH.Ro(xh), KH.Ro(oh), KH.Ro(yh), KH.Ro(gh), _t(rows)
    S = _loss(x, out, y, tab_d, t, 0.0)[0].read("S").double().numpy()[:b]
    loss, _ = _loss(x, out, y, tab_d, t, c)
    got = loss.read("loss").double().numpy()
    assert ((S < 1e-2 * c * c) if near else (S > 10 * c * c)).all(), S
    want = R.distance64(S, c)
    err, bound = np.abs(got[:b] - want), 5 * (U * want + TINY)
    assert (err <= bound).all(), f"forward: {np.max(err / bound):.3f} x bound"
    if near:  # the form the header forbids, in fp32, does not pass here
        naive = np.sqrt(F(S) + F(c * c), dtype=F) - F(c)
        assert (np.abs(naive - want) > bound).all()
    d = _loss_bwd(x, out, y, tab_d, t, loss, g, c).read("d").view(b, per).double().numpy()
    x64, o64, y64 = (v.astype(np.float64) for v in (xh, oh, yh))
    p64, q64 = p.astype(np.float64), q.astype(np.float64)
    f64 = p64 * x64 + q64 * o64
    c0 = F(2.0) * (gh[:b] + gh[b] / F(b))
    cq = q64[:, 0] * c0.astype(np.float64) / (2.0 * np.sqrt(S + c * c))
    want_d = cq[:, None] * (f64 - y64)
    bd = 10 * (U * np.abs(cq)[:, None] * (np.abs(p64 * x64) + np.abs(f64) + np.abs(f64 - y64)) + TINY)
    ed = np.abs(d - want_d)
    rows_on = np.abs(q64[:, 0]) > 0  # t = 0: q = 0, d_out is zero
    assert (ed <= bd).all() and (d[~rows_on] == 0).all(), f"backward: {np.max(ed / bd):.3f} x bound"
    print(f"[pseudo-Huber B {b} per_sample {per} {'S<<c2' if near else 'S>>c2'}] forward {np.max(err / bound):.3f}, backward "
          f"{np.max(ed[rows_on] / bd[rows_on]) if rows_on.any() else 0.0:.3f} x the rounding bound")


def test_a_timestep_outside_the_table_gives_nan():
    """NaN for that sample (f, its loss, the mean, its d_out), the other samples' bits untouched.  No row is read: behind a short
    table stand rows of 7.0, which a read would turn into a finite value."""
    b, per = 3, 4 * 5132
    tab, tab_d = _table("v")
    xh, oh, yh = _operand("n.x", b, per), _operand("n.out", b, per), _operand("n.y", b, per)
    x, out, y, g = KH.Ro(xh), KH.Ro(oh), KH.Ro(yh), KH.Ro(_upstream(b))
    t_ok = _t(ROWS)
    want_l, _ = _loss(x, out, y, tab_d, t_ok, 0.5)
    want_f, want_d = _out(x, out, tab_d, t_ok).read("f").view(b, per), _loss_bwd(x, out, y, tab_d, t_ok, want_l, g, 0.5).read("d").view(b, per)
    want_l = want_l.read("loss")
    for bad_at, bad_t in ((0, -1), (1, 1000), (2, -(2 ** 40)), (1, 2 ** 40)):
        t = t_ok.clone()
        t[bad_at] = bad_t
        loss, _ = _loss(x, out, y, tab_d, t, 0.5)
        f, d = _out(x, out, tab_d, t).read("f").view(b, per), _loss_bwd(x, out, y, tab_d, t, loss, g, 0.5).read("d").view(b, per)
        loss = loss.read("loss")
        for i in range(b):
            if i == bad_at:
                assert bool(torch.isnan(loss[i])) and bool(torch.isnan(d[i]).all()) and bool(torch.isnan(f[i]).all())
            else:
                KH.same(loss[i], want_l[i])
                KH.same(d[i], want_d[i])
                KH.same(f[i], want_f[i])
        assert bool(torch.isnan(loss[b]))
    short = torch.cat([tab_d[:400], torch.full((600, 2), 7.0, device=G.dev())])
    loss, _ = _loss(x, out, y, short, t_ok, 0.5, n_table=400)
    f = _out(x, out, short, t_ok, n_table=400).read("f").view(b, per)
    d = _loss_bwd(x, out, y, short, t_ok, loss, g, 0.5, n_table=400).read("d").view(b, per)
    loss = loss.read("loss")
    KH.same(loss[0], want_l[0])
    KH.same(f[0], want_f[0])
    assert bool(torch.isnan(loss[1:]).all()) and bool(torch.isnan(d[1:]).all()) and bool(torch.isnan(f[1:]).all())


def _update(xt, out, x0, coef_d, pos, noise=None, seed=0, first=0, base=0):
    b, per = out.t.shape
    step = torch.tensor([pos], dtype=torch.int32, device=G.dev())
    chk(KH.lib().cmx_consistency_update(xt.ptr, out.ptr, None if noise is None else noise.ptr, x0.ptr, P(coef_d), P(step), b, per, seed,
                                        first, base, _lib.stream()))


@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("b,per", KERNEL_CASES, ids=KERNEL_IDS)
def test_update_kernel(b, per, pred):
    """One sampling step on each row of a three-level run (999 -> 500 -> 100 -> data), bit for bit against the fp32 mirror: with a
    noise buffer; with the noise drawn in the kernel (= ddimx_noise_fill for the same seed, first sample, row and draw base, then
    the buffer); on the final row xt is x0, and neither a buffer of NaN nor the seed is read."""
    coef = consistency_coefficients([100, 500, 999], MH.alphas(), pred)
    coef32, coef_d = F(coef), _dev32(coef)
    xh, oh, zh = _operand("u.x", b, per), _operand("u.out", b, per), _operand("u.z", b, per)
    out, z = KH.Ro(oh), KH.Ro(zh)
    for pos in (0, 1):
        xt, x0 = KH.Out(b * per, init=xh), KH.Out(b * per)
        _update(xt, out, x0, coef_d, pos, noise=z)
        want_x, want_m = R.update32(xh, oh, coef32[pos], zh)
        KH.same(xt.read("xt").view(b, per), want_x, f"xt, row {pos}")
        KH.same(x0.read("x0").view(b, per), want_m, f"x0, row {pos}")
        assert np.isfinite(want_x).all() and coef32[pos, 5] > 0 and not np.array_equal(want_x, want_m)
        # drawn in the kernel
        first, base = 5, 3
        zbuf = torch.empty(b, per, device=G.dev())
        D.NoiseStream(SEED, first).fill(zbuf, torch.tensor([pos], dtype=torch.int32, device=G.dev()), base)
        via_buf_x, via_buf_m = KH.Out(b * per, init=xh), KH.Out(b * per)
        _update(via_buf_x, out, via_buf_m, coef_d, pos, noise=KH.Ro(zbuf))
        drawn_x, drawn_m = KH.Out(b * per, init=xh), KH.Out(b * per)
        _update(drawn_x, out, drawn_m, coef_d, pos, seed=SEED, first=first, base=base)
        KH.same(drawn_x.read("xt drawn"), via_buf_x.read("xt via buffer"), f"in-kernel draw, row {pos}")
        KH.same(drawn_m.read("x0 drawn"), via_buf_m.read("x0 via buffer"))
        assert not torch.equal(drawn_x.read("xt"), xt.read("xt")) and bool(torch.isfinite(drawn_x.read("xt")).all())
    # the final row: c1 = 0, a_next = 1
    assert coef32[2, 3:].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    poison = KH.Ro(np.full((b, per), np.nan, dtype=F))
    want_x, want_m = R.update32(xh, oh, coef32[2])
    for noise, seed in ((poison, 0), (None, SEED)):
        xt, x0 = KH.Out(b * per, init=xh), KH.Out(b * per)
        _update(xt, out, x0, coef_d, 2, noise=noise, seed=seed)
        KH.same(xt.read("xt").view(b, per), want_x, "xt, final row")
        KH.same(x0.read("x0").view(b, per), want_m, "x0, final row")
    assert np.array_equal(want_x, want_m) and np.isfinite(want_m).all()
    out.check("out")
    z.check("noise")


def test_a_samples_result_does_not_depend_on_the_batch():
    """Sample b of a batch of three (first_sample = 7) is the batch of one at first_sample = 7 + b, for all four kernels -- the
    backward with g[B] = 0, whose share g[B] / B is the only place B enters."""
    b, per = 3, 4 * 5132
    tab, tab_d = _table("eps")
    coef_d = _dev32(consistency_coefficients([100, 500, 999], MH.alphas(), "eps"))
    xh, oh, yh = _operand("b.x", b, per), _operand("b.out", b, per), _operand("b.y", b, per)
    gh = np.array([0.5, -1.0, 2.0, 0.0], dtype=F)

    def run(sl, first):
        n = xh[sl].shape[0]
        x, out, y, t = KH.Ro(xh[sl]), KH.Ro(oh[sl]), KH.Ro(yh[sl]), _t(ROWS[sl])
        g = KH.Ro(np.concatenate([gh[sl], [0.0]]).astype(F))
        loss, _ = _loss(x, out, y, tab_d, t, 0.5)
        d = _loss_bwd(x, out, y, tab_d, t, loss, g, 0.5).read("d").view(n, per)
        xt, x0 = KH.Out(n * per, init=xh[sl]), KH.Out(n * per)
        _update(xt, out, x0, coef_d, 1, seed=SEED, first=first)
        return _out(x, out, tab_d, t).read("f").view(n, per), loss.read("loss")[:n], d, xt.read("xt").view(n, per), x0.read("x0").view(n, per)

    whole = run(slice(0, 3), 7)
    for i in range(b):
        for got, want in zip(run(slice(i, i + 1), 7 + i), whole):
            KH.same(got[0], want[i], f"sample {i}")


def test_kernels_validate_before_the_launch():
    lib, dev = KH.lib(), G.dev()
    x = torch.zeros(2, 16, device=dev)
    tab, coef = torch.ones(4, 2, device=dev), torch.zeros(2, 8, device=dev)
    t, g, step = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(3, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    pt = torch.zeros(128, device=dev)
    s = _lib.stream()
    co, cl, cb, cu = lib.cmx_consistency_out, lib.cmx_consistency_loss, lib.cmx_consistency_loss_bwd, lib.cmx_consistency_update
    X, T, TB, G_, PT, C, ST = P(x), P(t), P(tab), P(g), P(pt), P(coef), P(step)
    bad = [(lambda: co(None, X, TB, 4, T, X, 2, 16, s), "cmx_consistency_out: null"), (lambda: co(X, None, TB, 4, T, X, 2, 16, s), "cmx_consistency_out: null"),
           (lambda: co(X, X, None, 4, T, X, 2, 16, s), "cmx_consistency_out: null"), (lambda: co(X, X, TB, 4, None, X, 2, 16, s), "cmx_consistency_out: null"),
           (lambda: co(X, X, TB, 4, T, None, 2, 16, s), "cmx_consistency_out: null"), (lambda: co(X, X, TB, 0, T, X, 2, 16, s), "cmx_consistency_out: n_table = 0"),
           (lambda: co(X, X, TB, 4, T, X, 0, 16, s), "cmx_consistency_out: B = 0"), (lambda: co(X, X, TB, 4, T, X, 65536, 16, s), "cmx_consistency_out: B = 65536"),
           (lambda: co(X, X, TB, 4, T, X, 2, 14, s), "cmx_consistency_out: per_sample = 14"), (lambda: co(X, X, TB, 4, T, X, 2, 0, s), "cmx_consistency_out: per_sample = 0"),
           (lambda: cl(None, X, X, TB, 4, T, 0.0, PT, G_, 2, 16, s), "cmx_consistency_loss: null"), (lambda: cl(X, X, None, TB, 4, T, 0.0, PT, G_, 2, 16, s), "cmx_consistency_loss: null"),
           (lambda: cl(X, X, X, TB, 4, T, 0.0, None, G_, 2, 16, s), "cmx_consistency_loss: null"), (lambda: cl(X, X, X, TB, 4, T, 0.0, PT, None, 2, 16, s), "cmx_consistency_loss: null"),
           (lambda: cl(X, X, X, TB, -1, T, 0.0, PT, G_, 2, 16, s), "cmx_consistency_loss: n_table = -1"), (lambda: cl(X, X, X, TB, 4, T, -0.5, PT, G_, 2, 16, s), "cmx_consistency_loss: huber_c"),
           (lambda: cl(X, X, X, TB, 4, T, float("nan"), PT, G_, 2, 16, s), "cmx_consistency_loss: huber_c"), (lambda: cl(X, X, X, TB, 4, T, float("inf"), PT, G_, 2, 16, s), "cmx_consistency_loss: huber_c"),
           (lambda: cl(X, X, X, TB, 4, T, 0.0, PT, G_, 2, 18, s), "cmx_consistency_loss: per_sample = 18"), (lambda: cl(X, X, X, TB, 4, T, 0.0, PT, G_, -1, 16, s), "cmx_consistency_loss: B = -1"),
           (lambda: cb(X, None, X, TB, 4, T, 0.0, G_, G_, X, 2, 16, s), "cmx_consistency_loss_bwd: null"), (lambda: cb(X, X, X, TB, 4, T, 0.0, None, G_, X, 2, 16, s), "cmx_consistency_loss_bwd: null"),
           (lambda: cb(X, X, X, TB, 4, T, 0.0, G_, None, X, 2, 16, s), "cmx_consistency_loss_bwd: null"), (lambda: cb(X, X, X, TB, 4, T, 0.0, G_, G_, None, 2, 16, s), "cmx_consistency_loss_bwd: null"),
           (lambda: cb(X, X, X, TB, 0, T, 0.0, G_, G_, X, 2, 16, s), "cmx_consistency_loss_bwd: n_table = 0"), (lambda: cb(X, X, X, TB, 4, T, -1.0, G_, G_, X, 2, 16, s), "cmx_consistency_loss_bwd: huber_c"),
           (lambda: cb(X, X, X, TB, 4, T, 0.0, G_, G_, X, 2, -4, s), "cmx_consistency_loss_bwd: per_sample = -4"), (lambda: cb(X, X, X, TB, 4, T, 0.0, G_, G_, X, 65536, 16, s), "cmx_consistency_loss_bwd: B = 65536"),
           (lambda: cu(None, X, None, X, C, ST, 2, 16, 0, 0, 0, s), "cmx_consistency_update: null"), (lambda: cu(X, None, None, X, C, ST, 2, 16, 0, 0, 0, s), "cmx_consistency_update: null"),
           (lambda: cu(X, X, None, None, C, ST, 2, 16, 0, 0, 0, s), "cmx_consistency_update: null"), (lambda: cu(X, X, None, X, None, ST, 2, 16, 0, 0, 0, s), "cmx_consistency_update: null"),
           (lambda: cu(X, X, None, X, C, None, 2, 16, 0, 0, 0, s), "cmx_consistency_update: null"), (lambda: cu(X, X, None, X, C, ST, 0, 16, 0, 0, 0, s), "cmx_consistency_update: B = 0"),
           (lambda: cu(X, X, None, X, C, ST, 2, 6, 0, 0, 0, s), "cmx_consistency_update: per_sample = 6"),
           (lambda: cu(X, X, None, X, C, ST, 2, 16, 0, 2 ** 32 - 1, 0, s), "cmx_consistency_update: first_sample + B")]
    for call, msg in bad:
        assert call() != 0
        assert msg in lib.ddimx_last_error().decode(), (msg, lib.ddimx_last_error().decode())
    xt, x0 = torch.ones(2, 16, device=dev), torch.ones(2, 16, device=dev)
    assert cu(P(xt), X, None, P(x0), C, ST, 2, 16, 0, 2 ** 32 - 2, 0, s) == 0  # first_sample + B = 2^32: the last sample index there is
    torch.cuda.synchronize()
    assert bool((x == 0).all()) and bool((xt == 0).all()) and bool((x0 == 0).all())  # the row of zeros was applied


# ---- 2. the loss and its gradients ------------------------------------------------------------------------------------------------------
def _qsample(x0, e, a, t):
    z = torch.empty_like(x0)
    chk(_lib.load().ddimx_qsample(P(x0), P(e), P(a), P(t), P(z), x0.size(0), x0[0].numel(), _lib.stream()))
    return z


def _teacher_model(dtype_str):
    return MH.pair("tiny", dtype_str)[2]  # type simple, eval mode


def _target_model(dtype_str):
    return MH.pair("tiny", dtype_str)[1]  # type v, eval mode


@pytest.mark.parametrize("huber_c", [0.0, 0.5], ids=["sq", "huber"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape,nn", [((2, 2, 16, 32), [2, 0]), ((3, 2, 24, 32), [1, 2, 0])], ids=["tiny", "ragged"])
def test_loss_and_parameter_gradients_vs_oracle(mode, shape, nn, huber_c):
    """The loss ``consistency_step`` differentiates -- the q-sample at t_hi, the GPU-computed target y of an eps teacher and a v target
    network, d(y, p z + q student(z, t_hi)) of a v student -- and every parameter gradient against autograd through the ORACLE
    student on that y, under ``model_harness.backward_case``'s gates unchanged.  Levels [0, 3, 500, 870], mixed indices."""
    dtype_str, dt = mode
    teacher, target = _teacher_model(dtype_str), _target_model(dtype_str)
    tt = [GRID[n + 1] for n in nn]
    made = {}

    def model(name, dtype_str, seed):
        return MH.build(name, dtype_str, seed, mode="train", kind="v", dropout=0.0, optimizer="Adam")

    def loss(m, x0, t, e, a):
        assert t.tolist() == tt
        z = _qsample(x0, e, a, t)
        y, t2 = D.consistency_target(target, teacher, z, torch.tensor(nn), GRID, a)
        assert torch.equal(t2, t) and bool(torch.isfinite(y).all())
        made["z"], made["y"] = z.cpu(), y.cpu()
        return consistency.consistency_loss(m, z, t, y, _dev32(consistency_table(a, "v")), huber_c)

    def ref_loss(model_fn, x0, t, e, a):
        tab = torch.from_numpy(F(consistency_table(a, "v")))[t]
        p, q = tab[:, 0].view(-1, 1, 1, 1), tab[:, 1].view(-1, 1, 1, 1)
        S = (made["y"] - (p * made["z"] + q * model_fn(made["z"], t))).square().sum(dim=(1, 2, 3))
        return (S / ((S + huber_c ** 2).sqrt() + huber_c) if huber_c else S).mean()

    MH.backward_case(mode, shape, tt, build_model=model, loss=loss, ref_loss=ref_loss)


# ---- 3. consistency_target ---------------------------------------------------------------------------------------------------------------
NN = [2, 0, 1]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_consistency_target_vs_oracle(mode):
    """y of an eps teacher and a v target network (the tiny pair) against the float64 restatement -- the teacher's reference DDIM
    step, then c_skip z_hat + c_out x0_hat -- over the CPU oracle's forwards, under ``model_harness.gate``.  Sample 1 has
    t_lo = t_min: its y is z_hat itself.  (An eps target multiplies its network's bf16 error by sigma / alpha; the composition test
    below covers it bit for bit.)"""
    dtype_str, dt = mode
    cfg, mv, ms, a = MH.pair("tiny", dtype_str)
    z = synth.gaussian("consistency.target.z", (3, 2, 16, 32))
    y, t_hi = D.consistency_target(mv, ms, z.to(G.dev()), torch.tensor(NN), GRID, a)
    assert t_hi.tolist() == [870, 3, 500] and t_hi.dtype == torch.int64 and t_hi.is_cuda and y.shape == z.shape
    teacher_eps, target_out = MH.oracle_eps_np(ms), MH.oracle_eps_np(mv)
    want = np.concatenate([R.target64(target_out, teacher_eps, z[i:i + 1].double().numpy(), GRID[n + 1], GRID[n], a.numpy(), "v")
                           for i, n in enumerate(NN)])
    mx, er = MH.gate(y, torch.from_numpy(want), dt, "consistency target")
    print(f"[consistency_target tiny {MODE_IDS[MODES.index(mode)]} eps->v] max {mx:.2e} rms {er:.2e}")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_consistency_target_is_the_composition_of_the_c_calls(mode):
    """All four teacher / target combinations of eps and v: bit for bit the forwards, ddimx_v_to_eps, ddimxd_distill_half on
    ``consistency_pairs`` rows and cmx_consistency_out applied by hand; skip = 2 takes the pairs two levels apart."""
    dtype_str, dt = mode
    lib, dev = _lib.load(), G.dev()
    cfg, mv, ms, a = MH.pair("tiny", dtype_str)
    z = synth.gaussian("consistency.target.z", (3, 2, 16, 32)).to(dev)
    b, per = z.size(0), z[0].numel()
    vt = _dev32(v_table(a))
    for teacher, t_pred in ((ms, "eps"), (mv, "v")):
        for target, y_pred in ((ms, "eps"), (mv, "v")):
            for skip, nn in ((1, NN), (2, [1, 0, 1])):
                y, t_hi = D.consistency_target(target, teacher, z, torch.tensor(nn), GRID, a, skip=skip)
                rows, hi, lo = consistency_pairs(GRID, a, skip)
                assert t_hi.tolist() == hi[nn].tolist() == [GRID[n + skip] for n in nn]
                rows_d, tab_d = _dev32(rows[nn]), _dev32(consistency_table(a, y_pred))
                thi, tlo = torch.from_numpy(hi[nn]).to(dev), torch.from_numpy(lo[nn]).to(dev)
                with torch.no_grad():
                    e0 = teacher(z, thi).clone()
                    if t_pred == "v":
                        chk(lib.ddimx_v_to_eps(P(z), P(e0), P(e0), P(vt), 1000, P(thi), b, per, _lib.stream()))
                    zhat, m0 = MH.sentinel(b, per), MH.sentinel(b, per)
                    chk(lib.ddimxd_distill_half(P(z), P(e0), P(rows_d), P(zhat), P(m0), b, per, _lib.stream()))
                    out = target(zhat.view_as(z), tlo).clone()
                    want = MH.sentinel(b, per)
                    chk(lib.cmx_consistency_out(P(zhat), P(out), P(tab_d), 1000, P(tlo), P(want), b, per, _lib.stream()))
                torch.cuda.synchronize()
                assert torch.equal(MH.bits(y.view(b, per)), MH.bits(want)), (t_pred, y_pred, skip)
                assert bool(torch.isfinite(y).all())
                at_min = [i for i, n in enumerate(nn) if GRID[n] == 0]
                assert at_min and all(torch.equal(y[i].view(-1), zhat[i]) for i in at_min)  # f(x, t_min) = x


# ---- 4. consistency_step ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("huber_c", [0.0, 0.5], ids=["sq", "huber"])
def test_consistency_step_is_the_composition_by_hand(huber_c):
    """Loss, norms and every student parameter after one ``consistency_step`` are ``torch.equal`` to ddimx_qsample ->
    ``consistency_target`` -> ``consistency_loss`` -> ``train.finish_step`` by hand on a twin; every target parameter is
    fp32(1 - mu) theta + fp32(mu) theta- on the UPDATED student, the three operations rounded separately (``EMAHelper``'s rounding),
    in one launch; the teacher is bit-unchanged; the default ``n`` is a mirrored draw; a second step runs.  bf16 mode, dropout 0.1,
    v student and target of an eps teacher."""
    dtype_str, mu = "torch.cuda.BFloat16Tensor", 0.95
    dev = G.dev()
    d = MH.config_dict("tiny", dtype_str, kind="v", optimizer="AdamW")
    cfg = configs.dict2namespace(d)
    a = MH.alphas(cfg).to(dev)
    teacher = _teacher_model(dtype_str)
    before = {k: v.clone() for k, v in teacher.state_dict().items()}
    x, e = synth.gaussian("cstep.x", (4, 2, 32, 32)).to(dev), synth.gaussian("cstep.e", (4, 2, 32, 32)).to(dev)
    n = torch.tensor([2, 0, 1, 2])

    def fresh():
        torch.manual_seed(77)
        m = synth.fill_module(D.Model(cfg), 11)
        tg = synth.fill_module(D.Model(cfg), 12).eval()
        return m, tg, train.TrainingState(cfg, m)

    calls = {"ema": 0}
    lib = _lib.load()
    real = lib.ddimx_ema_update_multi_coef

    def spy(*args):
        calls["ema"] += 1
        return real(*args)

    ma, ta, sa = fresh()
    has_ema = sa.ema_helper is not None
    lib.ddimx_ema_update_multi_coef = spy
    try:
        loss_a, norms_a = D.consistency_step(ma, ta, teacher, x, sa, a, GRID, huber_c=huber_c, mu=mu, e=e, n=n)
    finally:
        lib.ddimx_ema_update_multi_coef = real
    assert calls["ema"] == 1 + int(has_ema)  # the target update is one launch (beside the state's own EMA)
    mb, tb, sb = fresh()
    mb.train()
    t = torch.tensor([870, 3, 500, 870], device=dev)
    z = _qsample(x, e, a, t)
    y, t2 = D.consistency_target(tb, teacher, z, n, GRID, a)
    assert torch.equal(t2, t)
    loss_b = consistency.consistency_loss(mb, z, t2, y, _dev32(consistency_table(a, "v")), huber_c)
    loss_b, norms_b = train.finish_step(mb, sb, loss_b)
    assert torch.equal(loss_a, loss_b) and bool(torch.isfinite(loss_a)) and norms_a.keys() == norms_b.keys() and len(norms_a) >= 1
    assert all(torch.equal(norms_a[k], norms_b[k]) for k in norms_a)
    start_m, start_t, _ = fresh()
    start, start_tg = dict(start_m.named_parameters()), dict(start_t.named_parameters())
    for (name, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(pa, pb), name
    assert any(not torch.equal(pa, start[name]) for name, pa in ma.named_parameters())  # the step trained
    c_p, c_s = torch.tensor(F(1.0 - mu), device=dev), torch.tensor(F(mu), device=dev)
    moved = 0
    for name, pt in ta.named_parameters():
        want = (c_p * dict(ma.named_parameters())[name].detach()) + (c_s * start_tg[name].detach())
        assert torch.equal(pt.detach(), want), name
        moved += int(not torch.equal(pt.detach(), start_tg[name].detach()))
        assert torch.equal(dict(tb.named_parameters())[name], start_tg[name]), name  # the twin's target was only read
    assert moved > 0 and not ta.training
    for name, v in teacher.state_dict().items():
        assert torch.equal(v, before[name]), name
    assert not teacher.training
    # the target's next forward sees the new weights: its packed copy was invalidated
    with torch.no_grad():
        assert not torch.equal(ta(z, t), tb(z, t))
    nd = consistency.mirrored_indices(5, 3, generator=torch.Generator().manual_seed(3))
    assert nd.shape == (5,) and torch.equal(nd[3:], 2 - nd[:2]) and int(nd.min()) >= 0 and int(nd.max()) <= 2
    tables = sa._consistency_tables
    loss_c, _ = D.consistency_step(ma, ta, teacher, x, sa, a, GRID, huber_c=huber_c, mu=mu)
    assert bool(torch.isfinite(loss_c)) and sa._consistency_tables is tables  # the pointer tables are kept


# ---- 5. consistency_steps ----------------------------------------------------------------------------------------------------------------
SEQ4 = [100, 500, 870, 999]


def _x(b=2, tag="x"):
    return synth.gaussian(f"consistency.sample.{tag}", (b, 2, 16, 32))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_one_evaluation_is_the_consistency_function_of_one_forward(mode):
    dtype_str, dt = mode
    lib, dev = _lib.load(), G.dev()
    cfg, mv, ms, a = MH.pair("tiny", dtype_str)
    for m, pred in ((mv, "v"), (ms, "eps")):
        x = _x().to(dev)
        keep = x.clone()
        xs, x0s = D.consistency_steps(x, [870], m, a)
        t = torch.full((2,), 870, dtype=torch.int64, device=dev)
        with torch.no_grad():
            out = m(keep, t).clone()
        want, tab_d = torch.empty_like(keep), _dev32(consistency_table(a, pred))
        chk(lib.cmx_consistency_out(P(keep), P(out), P(tab_d), 1000, P(t), P(want), 2, keep[0].numel(), _lib.stream()))
        torch.cuda.synchronize()
        assert len(xs) == 2 and len(x0s) == 1 and xs[0] is x
        assert torch.equal(x0s[0], want.cpu()) and torch.equal(xs[1], want.cpu()) and torch.equal(x, want)  # in place, like generalized_steps
        assert bool(torch.isfinite(want).all())


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_trajectory_vs_oracle(mode):
    """Four levels with handed noise against the float64 restatement over the CPU oracle, every x0 prediction and every sample
    under ``model_harness.gate``; v model (|q| <= 1: the network's error is not amplified)."""
    dtype_str, dt = mode
    cfg, mv, ms, a = MH.pair("tiny", dtype_str)
    x = _x()
    zs = [synth.gaussian(f"consistency.traj.z{i}", tuple(x.shape)) for i in range(4)]
    handed = iter(zs)
    xs, x0s = D.consistency_steps(x.to(G.dev()), SEQ4, mv, a, noise_fn=lambda xt: next(handed).to(xt.device))
    assert len(xs) == 5 and len(x0s) == 4
    wxs, wx0s = R.sample64(MH.oracle_eps_np(mv), x.double().numpy(), SEQ4, a.numpy(), "v", [z.double().numpy() for z in zs])
    worst = 0.0
    for i in range(4):
        worst = max(worst, MH.gate(x0s[i], torch.from_numpy(wx0s[i]), dt, f"x0 prediction {i}")[0],
                    MH.gate(xs[i + 1], torch.from_numpy(wxs[i]), dt, f"sample {i}")[0])
    assert torch.equal(xs[-1], x0s[-1]) and not torch.equal(xs[-2], x0s[-2])
    print(f"[consistency_steps trajectory tiny {MODE_IDS[MODES.index(mode)]}] worst max {worst:.2e} x rms")


def _stepper(m, a, x, ns):
    return consistency.ConsistencyStepper(m, x.clone(), consistency_coefficients(SEQ4, a, m.prediction), use_graph=True, noise=ns)


def test_replayed_equals_eager_with_one_capture():
    """With a ``NoiseStream`` the step replays from one hipGraph: four steps, one capture, no noise buffer, and the bits of the
    eager run; ``consistency_steps`` gives the same; another seed gives another run."""
    cfg, mv, ms, a = MH.pair("tiny", "torch.cuda.BFloat16Tensor")
    x = _x().to(G.dev())
    ns = D.NoiseStream(SEED)
    outs, captures, has_graph, buf = MH.stepper_run(lambda: _stepper(mv, a, x, ns), 4, keep=lambda st: st.noise_buf)
    assert captures == 1 and has_graph and buf is None
    with MH.eager_steps():
        eager, ecaptures, egraph = MH.stepper_run(lambda: _stepper(mv, a, x, ns), 4)
    assert ecaptures == 0 and not egraph
    for i, ((xt, x0), (ext, ex0)) in enumerate(zip(outs, eager)):
        assert torch.equal(xt, ext) and torch.equal(x0, ex0), i
    run = D.consistency_steps(x.clone(), SEQ4, mv, a, noise=ns)
    MH.same_list(run[0][1:], [o[0] for o in outs], "xs")
    MH.same_list(run[1], [o[1] for o in outs], "x0_preds")
    assert bool(torch.isfinite(outs[-1][0]).all()) and torch.equal(outs[-1][0], outs[-1][1])
    other = D.consistency_steps(x.clone(), SEQ4, mv, a, noise=D.NoiseStream(SEED + 1))
    assert torch.equal(other[1][0], run[1][0]) and MH.differs(other, run)
    sel = D.consistency_steps(x.clone(), SEQ4, mv, a, select_index=[0, -1], noise=ns)
    MH.same_list(sel[1], [run[1][0], run[1][-1]], "select_index")


def test_a_batch_of_eight_is_two_shards_of_four():
    cfg, mv, ms, a = MH.pair("tiny", "torch.cuda.BFloat16Tensor")
    x = _x(8, "x8").to(G.dev())
    ns = D.NoiseStream(SEED)
    whole = D.consistency_steps(x.clone(), SEQ4, mv, a, noise=ns)
    for rank in range(2):
        part = D.consistency_steps(x[4 * rank:4 * rank + 4].clone(), SEQ4, mv, a, noise=ns.for_rank(8, rank, 2))
        MH.same_list(part[0][1:], [v[4 * rank:4 * rank + 4] for v in whole[0][1:]], f"xs of rank {rank}")
        MH.same_list(part[1], [v[4 * rank:4 * rank + 4] for v in whole[1]], f"x0_preds of rank {rank}")
    assert not torch.equal(whole[0][-1][:4], whole[0][-1][4:])


def test_noise_fn_fed_the_streams_normals_is_the_in_kernel_draw():
    cfg, mv, ms, a = MH.pair("tiny", "torch.cuda.BFloat16Tensor")
    x = _x().to(G.dev())
    ns = D.NoiseStream(SEED, 3)
    drawn = D.consistency_steps(x.clone(), SEQ4, mv, a, noise=ns)
    calls = []

    def noise_fn(xt):
        calls.append(len(calls))
        return ns.step_noise(tuple(xt.shape), calls[-1], xt.device)

    fed = D.consistency_steps(x.clone(), SEQ4, mv, a, noise_fn=noise_fn)
    MH.same_run(fed, drawn, "noise_fn against the in-kernel draw")
    assert calls == [0, 1, 2, 3]


@pytest.mark.parametrize("t", [500, 999])
def test_v_model_against_the_eps_callable_over_the_same_weights(t):
    """One evaluation at t of the v model (v table) against the callable that returns the eps of the same network's output read as
    v (``model_harness.v_wrapped``; eps table): the same function, two roundings apart -- not bit-equal.  With v the network's
    output (the same bits on both sides), eps = fma(v, s2, rn(x s1)) on fp32 (s1, s2) errs by at most 3 u (|x s1| + |v s2|) (two
    table roundings, two operations), which enters f_eps times |q_e|; each side adds its table's roundings and its two operations:
    u (2 |p x| + |q out| + |f|) in its own (p, q, out).  Every term is covered by
        4 (u (|q_e| (|x s1| + |v s2|) + |p_e x| + |q_e eps| + |p_v x| + |q_v v| + |f|) + 2^-126)."""
    cfg, mv, ms, a = MH.pair("tiny", "torch.cuda.FloatTensor")
    dev = G.dev()
    x = _x().to(dev)
    wrapped = MH.v_wrapped(ms, v_table(a))
    got_v = D.consistency_steps(x.clone(), [t], mv, a)[1][0].double().numpy()
    got_e = D.consistency_steps(x.clone(), [t], wrapped, a, prediction="eps")[1][0].double().numpy()
    with torch.no_grad():
        v = ms(x, torch.full((2,), t, dtype=torch.int64, device=dev), _fork=False).cpu().double().numpy()
    x64 = x.cpu().double().numpy()
    s1, s2 = v_table(a)[t]
    (pe, qe), (pv, qv) = consistency_table(a, "eps")[t], consistency_table(a, "v")[t]
    eps = s1 * x64 + s2 * v
    f = pv * x64 + qv * v
    bound = 4 * (U * (abs(qe) * (np.abs(x64 * s1) + np.abs(v * s2)) + np.abs(pe * x64) + np.abs(qe * eps) + np.abs(pv * x64) + np.abs(qv * v)
                      + np.abs(f)) + TINY)
    err = np.abs(got_v - got_e)
    assert (err <= bound).all(), f"{np.max(err / bound):.3f} x bound"
    assert (np.abs(got_v - f) <= bound).all() and not np.array_equal(got_v, got_e)
    print(f"[consistency v model vs eps callable t {t}] worst {np.max(err / bound):.3f} x the rounding bound, |q_eps| = {abs(qe):.2f}")
