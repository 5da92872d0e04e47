"""SNR loss weighting and progressive distillation on the GPU (include/ddimx_distill.h, ddim_audio_amd/losses.py, distill.py).

1. the weighted loss kernels through the C ABI; 2. ddimxd_distill_half / ddimxd_distill_target through the C ABI; 3. ``distill_target``
end to end; 4. training: ``target_loss``, the weighted loss's gradients, ``distill_step``, the graphed step with a weight, and
that a configuration without a weight launches what it launched before.

No tolerance is invented here: bit equality, rounding bounds counted in the docstrings, or the project's gates imported from
where they live (model_harness.gate, model_harness.backward_case)."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, configs, distill, losses, synth, train
from ddim_audio_amd.schedule import ddim_coefficients, distill_coefficients, halve_seq, loss_weight_table, v_table
from oracle import ref_cpu
import distill_ref as R
import gpu_util as G
import model_harness as MH
from model_harness import KERNEL_CASES, KERNEL_IDS, MODES, MODE_IDS, ROWS, TINY, U
import solver_ref
import vpred_ref as V

pytestmark = pytest.mark.gpu
NAMES = ["tiny", "audio"]
SEQS = [[0, 300, 600, 999], [3, 870, 990, 999]]
P, chk = _lib.ptr, _lib.check


def _dev32(a64):
    return torch.from_numpy(np.ascontiguousarray(a64, dtype=np.float32)).to(G.dev())


def _operand(tag, b, per):
    x = synth.gaussian(f"distill.{tag}.{b}.{per}", (b, per))
    return x, x.to(G.dev())


# ---- 1. the weighted loss kernels ----------------------------------------------------------------------------------------------------
def _loss_w(target, out, w, t, n_table=None):
    lib, b = _lib.load(), out.size(0)
    partial = torch.empty(b * 64, dtype=torch.float32, device=out.device)
    loss = MH.sentinel(1, b + 1)[0]
    chk(lib.ddimxd_sqerr_loss_w(P(target), P(out), P(w), w.numel() if n_table is None else n_table, P(t), P(partial), P(loss), b,
                               out[0].numel(), _lib.stream()))
    return loss


def _loss_w_bwd(target, out, g, w, t, n_table=None):
    lib, b = _lib.load(), out.size(0)
    d = MH.sentinel(b, out[0].numel())
    chk(lib.ddimxd_sqerr_loss_w_bwd_mean(P(target), P(out), P(g), P(w), w.numel() if n_table is None else n_table, P(t), P(d), b,
                                        out[0].numel(), _lib.stream()))
    return d


def _loss_plain(target, out, g):
    lib, b, per = _lib.load(), out.size(0), out[0].numel()
    partial = torch.empty(b * 64, dtype=torch.float32, device=out.device)
    loss, d = MH.sentinel(1, b + 1)[0], MH.sentinel(b, per)
    chk(lib.ddimx_sqerr_loss(P(target), P(out), P(partial), P(loss), b, per, _lib.stream()))
    chk(lib.ddimx_sqerr_loss_bwd_mean(P(target), P(out), P(g), P(d), b, per, _lib.stream()))
    return loss, d


def _upstream(b):
    """An upstream gradient of the [B + 1] loss vector with every entry in use."""
    return torch.tensor([0.25 * (i + 1) for i in range(b)] + [1.0], dtype=torch.float32, device=G.dev())


@pytest.mark.parametrize("b,per", KERNEL_CASES, ids=KERNEL_IDS)
def test_weighted_loss_kernels(b, per):
    """(1) A table of ones: loss, mean and d_out are the unweighted kernels' bits.

    (2) The min_snr table (eps, gamma 5) at t = [0, 412, 999][:B]: loss[b] is the fp32 product of the table entry and the unweighted
    value, and loss[B] the fp32 sum of those in b order divided by B.  d_out = c (out - target) with c = rn(w c0), c0 =
    rn(2 rn(g[b] + rn(g[B] / B))): c0 is recomputed here with the same fp32 operations (numpy), so what is left to count against
    fp64 is the product w c0 (one rounding), the difference out - target (one) and the product c (out - target) (one): each errs
    by 2^-24 of its result, all three results scale the final value, so |error| <= 3 * 2^-24 |d| to first order; one more unit
    covers the second-order terms, 2^-126 per rounding an underflow: 4 (2^-24 |c (out - target)| + 2^-126)."""
    dev = G.dev()
    (tg, tgd), (o, od) = _operand("lw.target", b, per), _operand("lw.out", b, per)
    g = _upstream(b)
    rows = ROWS[:b]
    t = torch.tensor(rows, dtype=torch.int64, device=dev)
    want_loss, want_d = _loss_plain(tgd, od, g)
    ones = torch.ones(1000, device=dev)
    loss, d = _loss_w(tgd, od, ones, t), _loss_w_bwd(tgd, od, g, ones, t)
    torch.cuda.synchronize()
    assert torch.equal(MH.bits(loss), MH.bits(want_loss)) and torch.equal(MH.bits(d), MH.bits(want_d))
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(d).all())
    # the min_snr table
    w64 = loss_weight_table(MH.alphas(), "eps", "min_snr", 5.0)
    w32 = np.float32(w64)
    assert w32[0] < 1 and w32[412] == 1 and w32[999] == 1 and len({float(v) for v in w32[:130]}) > 100
    wd = _dev32(w64)
    loss, d = _loss_w(tgd, od, wd, t), _loss_w_bwd(tgd, od, g, wd, t)
    torch.cuda.synchronize()
    plain, got = want_loss.cpu().numpy(), loss.cpu().numpy()
    per_w = np.array([np.float32(w32[r]) * np.float32(plain[i]) for i, r in enumerate(rows)], dtype=np.float32)
    tot = np.float32(0.0)
    for v in per_w:
        tot = np.float32(tot + v)
    assert np.array_equal(got[:b], per_w) and got[b] == np.float32(tot / np.float32(b))
    # the v table, where every weight is below 1: the mean sums the ROUNDED products (no product is fused into the sum)
    v32 = np.float32(loss_weight_table(MH.alphas(), "v", "min_snr", 5.0))
    got = _loss_w(tgd, od, _dev32(v32), t).cpu().numpy()
    tot = np.float32(0.0)
    for i, r in enumerate(rows):
        assert v32[r] < 1 and got[i] == np.float32(v32[r] * plain[i])
        tot = np.float32(tot + got[i])
    assert got[b] == np.float32(tot / np.float32(b))
    gh, dh = g.cpu().numpy(), d.cpu().double().numpy()
    worst = 0.0
    for i, r in enumerate(rows):
        c0 = np.float32(2.0) * np.float32(gh[i] + np.float32(gh[b] / np.float32(b)))
        want = float(w32[r]) * float(c0) * (o[i].double().numpy() - tg[i].double().numpy())
        bound = 4 * (U * np.abs(want) + TINY)
        err = np.abs(dh[i] - want)
        assert (err <= bound).all(), f"sample {i} (t = {r}): worst {np.max(err / bound):.3f} x bound"
        worst = max(worst, float(np.max(err / bound)))
    print(f"[sqerr_loss_w_bwd B {b} per_sample {per}] worst error {worst:.3f} x the rounding bound")
    if b > 1:  # sample 0 carries a weight below 1: its row is not the unweighted one
        assert not torch.equal(d[0], want_d[0]) and torch.equal(d[1], want_d[1])


def test_weighted_loss_with_a_timestep_outside_the_table():
    """NaN for that sample (and the mean), the other samples' values untouched.  No row is read: behind a short table stand NaN
    rows, then -- since a NaN read there could not be told from the NaN of a sample outside -- rows of 7.0, which a read would
    turn into a finite value."""
    dev, b, per = G.dev(), 3, 4 * 5132
    (tg, tgd), (o, od) = _operand("oob.target", b, per), _operand("oob.out", b, per)
    g = _upstream(b)
    wd = _dev32(loss_weight_table(MH.alphas(), "eps", "min_snr", 5.0))
    t_ok = torch.tensor(ROWS, dtype=torch.int64, device=dev)
    want, want_d = _loss_w(tgd, od, wd, t_ok), _loss_w_bwd(tgd, od, g, wd, t_ok)
    for bad_at, bad_t in ((0, -1), (1, 1000), (2, -(2 ** 40)), (1, 2 ** 40)):
        t = t_ok.clone()
        t[bad_at] = bad_t
        loss, d = _loss_w(tgd, od, wd, t), _loss_w_bwd(tgd, od, g, wd, t)
        torch.cuda.synchronize()
        for i in range(b):
            if i == bad_at:
                assert bool(torch.isnan(loss[i])) and bool(torch.isnan(d[i]).all())
            else:
                assert torch.equal(MH.bits(loss[i]), MH.bits(want[i])) and torch.equal(MH.bits(d[i]), MH.bits(want_d[i])), (bad_t, i)
        assert bool(torch.isnan(loss[b]))
    # a shorter table, 400 rows: t = 412 and 999 are outside
    for behind in (float("nan"), 7.0):
        short = torch.cat([wd[:400], torch.full((600,), behind, device=dev)])
        loss, d = _loss_w(tgd, od, short, t_ok, n_table=400), _loss_w_bwd(tgd, od, g, short, t_ok, n_table=400)
        torch.cuda.synchronize()
        assert torch.equal(MH.bits(loss[0]), MH.bits(want[0])) and torch.equal(MH.bits(d[0]), MH.bits(want_d[0]))
        assert bool(torch.isnan(loss[1:]).all()) and bool(torch.isnan(d[1:]).all())


def test_kernels_validate_before_the_launch():
    lib, dev = _lib.load(), G.dev()
    x = torch.zeros(2, 16, device=dev)
    w, rows = torch.ones(4, device=dev), torch.zeros(2, 12, device=dev)
    t, g = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(3, device=dev)
    pt = torch.zeros(128, device=dev)
    s = _lib.stream()
    lw, lb, dh, dt_ = lib.ddimxd_sqerr_loss_w, lib.ddimxd_sqerr_loss_w_bwd_mean, lib.ddimxd_distill_half, lib.ddimxd_distill_target
    bad = [(lambda: lw(None, P(x), P(w), 4, P(t), P(pt), P(g), 2, 16, s), "ddimxd_sqerr_loss_w: null"),
           (lambda: lw(P(x), P(x), None, 4, P(t), P(pt), P(g), 2, 16, s), "ddimxd_sqerr_loss_w: null"),
           (lambda: lw(P(x), P(x), P(w), 4, None, P(pt), P(g), 2, 16, s), "ddimxd_sqerr_loss_w: null"),
           (lambda: lw(P(x), P(x), P(w), 4, P(t), P(pt), None, 2, 16, s), "ddimxd_sqerr_loss_w: null"),
           (lambda: lw(P(x), P(x), P(w), 0, P(t), P(pt), P(g), 2, 16, s), "ddimxd_sqerr_loss_w: n_table = 0"),
           (lambda: lw(P(x), P(x), P(w), 4, P(t), P(pt), P(g), 0, 16, s), "ddimxd_sqerr_loss_w: B = 0"),
           (lambda: lw(P(x), P(x), P(w), 4, P(t), P(pt), P(g), 65536, 16, s), "ddimxd_sqerr_loss_w: B = 65536"),
           (lambda: lw(P(x), P(x), P(w), 4, P(t), P(pt), P(g), 2, 0, s), "ddimxd_sqerr_loss_w: per_sample = 0"),
           (lambda: lb(P(x), None, P(g), P(w), 4, P(t), P(x), 2, 16, s), "ddimxd_sqerr_loss_w_bwd_mean: null"),
           (lambda: lb(P(x), P(x), None, P(w), 4, P(t), P(x), 2, 16, s), "ddimxd_sqerr_loss_w_bwd_mean: null"),
           (lambda: lb(P(x), P(x), P(g), P(w), 4, P(t), None, 2, 16, s), "ddimxd_sqerr_loss_w_bwd_mean: null"),
           (lambda: lb(P(x), P(x), P(g), P(w), -1, P(t), P(x), 2, 16, s), "ddimxd_sqerr_loss_w_bwd_mean: n_table = -1"),
           (lambda: lb(P(x), P(x), P(g), P(w), 4, P(t), P(x), 2, -4, s), "ddimxd_sqerr_loss_w_bwd_mean: per_sample = -4"),
           (lambda: dh(None, P(x), P(rows), P(x), P(x), 2, 16, s), "ddimxd_distill_half: null"),
           (lambda: dh(P(x), P(x), None, P(x), P(x), 2, 16, s), "ddimxd_distill_half: null"),
           (lambda: dh(P(x), P(x), P(rows), P(x), None, 2, 16, s), "ddimxd_distill_half: null"),
           (lambda: dh(P(x), P(x), P(rows), P(x), P(x), 0, 16, s), "ddimxd_distill_half: B = 0"),
           (lambda: dh(P(x), P(x), P(rows), P(x), P(x), 2, 14, s), "ddimxd_distill_half: per_sample = 14"),
           (lambda: dt_(P(x), P(x), P(x), P(x), P(rows), None, None, 2, 16, s), "ddimxd_distill_target: null"),
           (lambda: dt_(P(x), None, P(x), P(x), P(rows), P(x), None, 2, 16, s), "ddimxd_distill_target: null"),
           (lambda: dt_(P(x), P(x), P(x), P(x), P(rows), P(x), None, 65536, 16, s), "ddimxd_distill_target: B = 65536"),
           (lambda: dt_(P(x), P(x), P(x), P(x), P(rows), P(x), None, 2, 0, s), "ddimxd_distill_target: per_sample = 0")]
    for call, msg in bad:
        assert call() != 0
        assert msg in lib.ddimx_last_error().decode(), (msg, lib.ddimx_last_error().decode())


# ---- 2. the target kernels --------------------------------------------------------------------------------------------------------------
def _rows(pred):
    """(coefficient rows float64 [4, 12], their (teacher_seq, k)): the two student steps of each of SEQS -- k = 0, where omega = 0
    and the step ends at the data, included."""
    a = MH.alphas()
    coef = np.concatenate([distill_coefficients(s, a, pred) for s in SEQS])
    return coef, [(s, k) for s in SEQS for k in range(2)]


PICK = {3: [3, 0, 1], 2: [2, 3], 1: [3]}  # which of the four rows the samples of a batch take


def _half(z, e0, rows_d):
    lib, (b, per) = _lib.load(), z.shape
    zmid, m0 = MH.sentinel(b, per), MH.sentinel(b, per)
    chk(lib.ddimxd_distill_half(P(z), P(e0), P(rows_d), P(zmid), P(m0), b, per, _lib.stream()))
    return zmid, m0


def _target(z, zmid, e1, m0, rows_d, target=None, want_x0=True):
    lib, (b, per) = _lib.load(), z.shape
    target = MH.sentinel(b, per) if target is None else target
    x0 = MH.sentinel(b, per) if want_x0 else None
    chk(lib.ddimxd_distill_target(P(z), P(zmid), P(e1), P(m0), P(rows_d), P(target), P(x0), b, per, _lib.stream()))
    return target, x0


def x0_bound(zmid, e1, m0, s1m, s2m):
    """|x - fp64(x)| for x = fma(omega, m0 - m1, m1), m1 = rn(rn(zmid - s1' e1) / s2'), on given fp32 operands, 0 <= omega < 0.5.
    With M1 = (|zmid| + s1' |e1|) / s2' >= |m1| and X = M1 + |m0|: the fma and the division leave m1 with at most 2 * 2^-24 M1; the
    difference m0 - m1 adds 2^-24 |m0 - m1| <= 2^-24 X, weighted by omega < 0.5; m1's error reaches x with weight 1 - omega <= 1;
    the last fma adds 2^-24 |x| <= 2^-24 X.  Sum: 2^-24 (2 M1 + 0.5 X + X) <= 3.5 * 2^-24 X; half a unit more for the second order,
    2^-126 per rounding for an underflow: 4 (2^-24 X + 2^-126).  Returns (bound, X)."""
    X = (np.abs(zmid) + s1m * np.abs(e1)) / s2m + np.abs(m0)
    return 4 * (U * X + TINY), X


def target_bound(z, X, cz, cx):
    """|target - fp64(target)| for target = fma(x, cx, rn(z cz)): x's error (3.5 * 2^-24 X, above) times |cx|, the product z cz
    (2^-24 |z cz|) and the fma (2^-24 |target| <= 2^-24 (|z cz| + |cx| X)): 2^-24 (4.5 |cx| X + 2 |z cz|), rounded up to
    5 (2^-24 (|cx| X + |z cz|) + 2^-126)."""
    return 5 * (U * (np.abs(cx) * X + np.abs(z * cz)) + TINY)


def direct_bounds(z, e0, zmid, e1, m0, row64, a64, seq, k):
    """Bounds for kernel against tests/distill_ref.py's DIRECT formula in fp64 with fp64 coefficients, fed the kernel's own
    fp32 zmid and the same z, eps1: (bound on x, bound on target).

    The direct formula never sees m0: x_D = (z'' - r z) / (alpha'' - r alpha) with z'' the teacher's second step from zmid.
    Writing z = alpha m0* + sigma e0 (m0* the exact first prediction) and zmid = alpha' m0* + sigma' e0 + dz', it is
    x_D = omega m0* + (1 - omega) m1(zmid) + G dz', G = (sigma''/sigma') / (alpha'' - (sigma''/sigma) alpha): the half step's
    rounding error dz', which the convex form ignores, comes back divided by the cancelling denominator.  That is the direct
    form's own conditioning term.  Term by term, in units of u = 2^-24, with M0 = (|z| + sigma |e0|) / alpha, M1 and X as in
    ``x0_bound``, Zm = alpha' |m0| + sigma' |e0|:
      the kernel's arithmetic (x0_bound)                                          3.5 X
      omega rounded to fp32, times |m0 - m1| <= X, omega < 0.5                    0.5 X
      m0: s1, s2 rounded to fp32 (2 M0) and its two roundings (2 M0), weight omega < 0.5   2 M0
      m1: s1', s2' rounded to fp32                                                2 M1 <= 2 X
      dz': alpha' times m0's error (4 alpha' M0), s3, c2 rounded to fp32 (Zm), the product and the fma (2 Zm), times G
    so |x - x_D| <= u (6 X + 2 M0) + G u (4 alpha' M0 + 3 Zm); one unit more on the first term for the second order:
    7 (u (X + M0) + 2^-126) + G u (4 alpha' M0 + 3 Zm).  The target adds cz, cx rounded to fp32 and its own two roundings:
    |cx| (bound on x) + u (3 |z cz| + 2 |cx| X) + 2^-126."""
    t, t_mid, t_end = R.steps_of(seq, k)
    (al, si), (alm, sim), (ale, sie) = R.alpha_sigma(a64, t), R.alpha_sigma(a64, t_mid), R.alpha_sigma(a64, t_end)
    G_ = (sie / sim) / (ale - (sie / si) * al)
    M0 = (np.abs(z) + si * np.abs(e0)) / al
    _, X = x0_bound(zmid, e1, m0, sim, alm)
    Zm = alm * np.abs(m0) + sim * np.abs(e0)
    bx = 7 * (U * (X + M0) + TINY) + G_ * U * (4 * alm * M0 + 3 * Zm)
    cz, cx = row64[9], row64[10]
    return bx, np.abs(cx) * bx + U * (3 * np.abs(z * cz) + 2 * np.abs(cx) * X) + TINY


@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("b,per", KERNEL_CASES, ids=KERNEL_IDS)
def test_distill_kernels(b, per, pred):
    """zmid and m0 are ddimx_ddim_update's bits (run per sample on a copy, with the teacher's own eta = 0 table); the target and the
    x0 target against fp64 on the same fp32 operands (``x0_bound``, ``target_bound``) and against the restatement's direct formula
    (``direct_bounds``); in place (target is m0) equals out of place; omega = 0 rows return m1 itself."""
    lib, dev = _lib.load(), G.dev()
    a = MH.alphas()
    a64 = R.table64(a.numpy())
    coef, where = _rows(pred)
    pick = PICK[b]
    rows64 = coef[pick]
    rows32 = np.float32(rows64)
    rows_d = _dev32(rows64)
    (z, zd), (e0, e0d), (e1, e1d) = _operand("k.z", b, per), _operand("k.e0", b, per), _operand("k.e1", b, per)
    zmid, m0 = _half(zd, e0d, rows_d)
    z_before = zd.clone()
    target, x0 = _target(zd, zmid, e1d, m0, rows_d)
    torch.cuda.synchronize()
    assert torch.equal(zd, z_before)
    # the half step: ddimx_ddim_update with the teacher's coefficient table, one sample at a time
    for i, r in enumerate(pick):
        seq, k = where[r]
        table = ddim_coefficients(seq, a, 0.0)
        at = [int(row[0]) for row in table].index(int(rows64[i, 0]))
        step, table_d = torch.tensor([at], dtype=torch.int32, device=dev), _dev32(table)
        xt, p0, ei = zd[i].clone(), MH.sentinel(1, per)[0], e0d[i].contiguous()
        chk(lib.ddimx_ddim_update(P(xt), P(ei), None, P(p0), P(table_d), P(step), per, _lib.stream()))
        torch.cuda.synchronize()
        assert torch.equal(MH.bits(xt), MH.bits(zmid[i])) and torch.equal(MH.bits(p0), MH.bits(m0[i])), i
    assert bool(torch.isfinite(zmid).all()) and bool(torch.isfinite(m0).all())
    # fp64 on the same fp32 operands
    zm, mm = zmid.cpu().double().numpy(), m0.cpu().double().numpy()
    got_t, got_x = target.cpu().double().numpy(), x0.cpu().double().numpy()
    assert np.isfinite(got_t).all() and np.isfinite(got_x).all()
    worst = [0.0] * 4
    for i, r in enumerate(pick):
        seq, k = where[r]
        s1m, s2m, om, cz, cx = (float(v) for v in rows32[i, 6:11])
        zi, e0i, e1i = z[i].double().numpy(), e0[i].double().numpy(), e1[i].double().numpy()
        m1 = (zm[i] - s1m * e1i) / s2m
        want_x = m1 + om * (mm[i] - m1)
        want_t = cz * zi + cx * want_x
        bx, X = x0_bound(zm[i], e1i, mm[i], s1m, s2m)
        bt = target_bound(zi, X, cz, cx)
        ex, et = np.abs(got_x[i] - want_x), np.abs(got_t[i] - want_t)
        assert (ex <= bx).all() and (et <= bt).all(), f"sample {i} (row {r}): {np.max(ex / bx):.3f}, {np.max(et / bt):.3f} x bound"
        assert (om == 0.0) == (k == 0)
        # the direct formula, fp64 coefficients
        dir_t, dir_x = R.direct_from_mid(zi, zm[i], e1i, seq, k, a.numpy(), pred)
        dbx, dbt = direct_bounds(zi, e0i, zm[i], e1i, mm[i], rows64[i], a64, seq, k)
        dx, dt_ = np.abs(got_x[i] - dir_x), np.abs(got_t[i] - dir_t)
        assert (dx <= dbx).all() and (dt_ <= dbt).all(), f"direct, sample {i} (row {r}): {np.max(dx / dbx):.3f}, {np.max(dt_ / dbt):.3f}"
        worst = [max(w, float(np.max(v))) for w, v in zip(worst, (ex / bx, et / bt, dx / dbx, dt_ / dbt))]
    print(f"[distill kernels {pred} B {b} per_sample {per}] worst error / bound: x {worst[0]:.3f}, target {worst[1]:.3f}, "
          f"direct x {worst[2]:.3f}, direct target {worst[3]:.3f}")
    # negative control: another row's scalars do not pass the fp64 bound
    other = np.float32(coef[(pick[0] + 1) % 4])
    s1m, s2m, om, cz, cx = (float(v) for v in other[6:11])
    m1 = (zm[0] - s1m * e1[0].double().numpy()) / s2m
    wrong = cz * z[0].double().numpy() + cx * (m1 + om * (mm[0] - m1))
    assert (np.abs(got_t[0] - wrong) > target_bound(z[0].double().numpy(), x0_bound(zm[0], e1[0].double().numpy(), mm[0], s1m, s2m)[1], cz, cx)).any()
    # in place (target is m0) = out of place; a null x0_target writes the same target
    inplace = m0.clone()
    t2, none = _target(zd, zmid, e1d, inplace, rows_d, target=inplace, want_x0=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(MH.bits(t2), MH.bits(target))


def test_distill_kernels_sample_result_does_not_depend_on_the_batch():
    b, per = 3, 4 * 5132
    coef, _ = _rows("v")
    rows_d = _dev32(coef[PICK[3]])
    (_, zd), (_, e0d), (_, e1d) = _operand("ind.z", b, per), _operand("ind.e0", b, per), _operand("ind.e1", b, per)
    zmid, m0 = _half(zd, e0d, rows_d)
    target, x0 = _target(zd, zmid, e1d, m0, rows_d)
    for i in range(b):
        one = slice(i, i + 1)
        r1 = rows_d[one].contiguous()
        zm1, m1 = _half(zd[one].contiguous(), e0d[one].contiguous(), r1)
        t1, x1 = _target(zd[one].contiguous(), zm1, e1d[one].contiguous(), m1, r1)
        for solo, full in ((zm1, zmid), (m1, m0), (t1, target), (x1, x0)):
            assert torch.equal(MH.bits(solo[0]), MH.bits(full[i])), i


# ---- 3. distill_target end to end --------------------------------------------------------------------------------------------------------
SEQ = [3, 870, 990, 999]
K = [0, 1]  # t = 870 -> 3 -> data, and 999 -> 990 -> 870


def _z(name, cfg):
    shape = (2, 2, 16, 32) if name == "tiny" else (2, cfg.model.channels, 32, cfg.model.f_size)
    return synth.gaussian(f"distill.e2e.{name}", shape)


_REFS = {}


def _oracle_reference(name, dtype_str, pred):
    """(target, x0 target) of the restatement over the CPU oracle for the same-prediction pair ``pred`` -> ``pred``, once per
    (network, prediction): float64 chain, the oracle's fp32 forward as the teacher."""
    key = (name, pred)
    if key not in _REFS:
        cfg, mv, ms, a = MH.pair(name, dtype_str)
        live, ocfg = MH.oracle(mv, name)
        sd = {k: v.detach() for k, v in live.items()}
        z = _z(name, cfg)

        def teacher(zz, t):
            with torch.no_grad():
                out = ref_cpu.model_forward(sd, ocfg, torch.from_numpy(zz).float()[None], torch.tensor([t]))[0].double().numpy()
            if pred == "v":
                s1, s2 = V.scales(a, t)
                out = V.eps_from_v(zz, out, s1, s2)
            return out

        out = [R.distill_target(teacher, z[i].double().numpy(), K[i], SEQ, a.numpy(), pred) for i in range(2)]
        _REFS[key] = (torch.from_numpy(np.stack([o[0] for o in out])), torch.from_numpy(np.stack([o[1] for o in out])))
    return _REFS[key]


@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_distill_target_same_prediction_vs_oracle(name, mode, pred):
    """eps teacher -> eps student and v teacher -> v student: the target and the x0 target against the restatement (direct formula,
    two reference DDIM steps) over the CPU oracle, under the whole-network gate of model_harness."""
    dtype_str, dt = mode
    cfg, mv, ms, a = MH.pair(name, dtype_str)
    teacher = mv if pred == "v" else ms
    z = _z(name, cfg).to(G.dev())
    target, t, x0 = D.distill_target(teacher, z, torch.tensor(K), SEQ, a, student_prediction=pred, return_x0=True)
    assert t.tolist() == [870, 999] and t.dtype == torch.int64 and t.is_cuda
    want_t, want_x = _oracle_reference(name, dtype_str, pred)
    mx, er = MH.gate(target, want_t, dt, f"target {name} {pred}")
    mx2, er2 = MH.gate(x0, want_x, dt, f"x0 target {name} {pred}")
    print(f"[distill_target {name} {MODE_IDS[MODES.index(mode)]} {pred}->{pred}] target max {mx:.2e} rms {er:.2e}; x0 max {mx2:.2e} rms {er2:.2e}")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_distill_target_cross_prediction_is_the_composition_of_the_c_calls(name, mode):
    """eps teacher -> v student and v teacher -> eps student: bit for bit the forwards, ddimx_v_to_eps, ddimxd_distill_half and
    ddimxd_distill_target applied by hand (out of place).  No oracle gate: the bf16 error of a cross pair is legitimately amplified
    by sigma / alpha or 1 / alpha (test_gpu_vpred's amplification test)."""
    dtype_str, dt = mode
    lib, dev = _lib.load(), G.dev()
    cfg, mv, ms, a = MH.pair(name, dtype_str)
    z = _z(name, cfg).to(dev)
    b, per = z.size(0), z[0].numel()
    vt = _dev32(v_table(a))
    for teacher, t_pred, s_pred in ((ms, "eps", "v"), (mv, "v", "eps")):
        target, t, x0 = D.distill_target(teacher, z, torch.tensor(K), SEQ, a, student_prediction=s_pred, return_x0=True)
        rows64 = distill_coefficients(SEQ, a, s_pred)[K]
        rows_d = _dev32(rows64)
        tt, tm = torch.tensor([870, 999], device=dev), torch.tensor([3, 990], device=dev)
        with torch.no_grad():
            e0 = teacher(z, tt).clone()
            if t_pred == "v":
                chk(lib.ddimx_v_to_eps(P(z), P(e0), P(e0), P(vt), 1000, P(tt), b, per, _lib.stream()))
            zmid, m0 = _half(z.view(b, per), e0.view(b, per), rows_d)
            e1 = teacher(zmid.view_as(z), tm).clone()
            if t_pred == "v":
                chk(lib.ddimx_v_to_eps(P(zmid), P(e1), P(e1), P(vt), 1000, P(tm), b, per, _lib.stream()))
            want_t, want_x = _target(z.view(b, per), zmid, e1.view(b, per), m0, rows_d)
        torch.cuda.synchronize()
        assert torch.equal(MH.bits(target.view(b, per)), MH.bits(want_t)) and torch.equal(MH.bits(x0.view(b, per)), MH.bits(want_x)), (t_pred, s_pred)
        assert bool(torch.isfinite(target).all())
        only_t, _ = D.distill_target(teacher, z, torch.tensor(K), SEQ, a, student_prediction=s_pred)
        assert torch.equal(only_t, target)


def closed_form_bound(z, a64, var, row64, seq, k):
    """|x - fp64| and |target - fp64| when the teacher is eps = c_t z with c_t given to the GPU as an fp32 scalar, against the fp64
    chain with fp64 c_t.  In units of u = 2^-24, M0, M1, X, Zm as in ``direct_bounds`` but from the fp64 chain:
      eps0: c_t rounded, one product                                              2 |e0|
      m0: eps0's error (2 sigma |e0| / alpha <= 2 M0), s1, s2 rounded (2 M0), two roundings (2 M0)          6 M0
      z': alpha' times that, eps0's error (2 sigma' |e0|), s3, c2 rounded (Zm), two roundings (2 Zm)         dz' = 6 alpha' M0 + 5 Zm
      eps1 = c_t' z': c_t' dz' + 2 |e1|
      m1 = (z' - sigma' eps1) / alpha': |1 - sigma' c_t'| / alpha' = D1 times dz', eps1's own 2 sigma' |e1| / alpha' <= 2 M1,
           s1', s2' rounded (2 M1), two roundings (2 M1)                          D1 dz' + 6 M1
      x: omega < 0.5 times m0's error (3 M0), m1's error, omega rounded and the difference (X), the fma (X)
    so |x - x64| <= u (3 M0 + 6 M1 + 2 X) + D1 u (6 alpha' M0 + 5 Zm) <= 8 u (X + M0) + D1 u (6 alpha' M0 + 5 Zm), one unit of the
    first term standing for the second order; the target as in ``direct_bounds``."""
    t, t_mid, _ = R.steps_of(seq, k)
    (al, si), (alm, sim) = R.alpha_sigma(a64, t), R.alpha_sigma(a64, t_mid)
    c0, c1 = si / (a64[t] * var + 1 - a64[t]), sim / (a64[t_mid] * var + 1 - a64[t_mid])
    e0 = c0 * z
    m0 = (z - si * e0) / al
    zm = alm * m0 + sim * e0
    e1 = c1 * zm
    M0, M1 = (np.abs(z) + si * np.abs(e0)) / al, (np.abs(zm) + sim * np.abs(e1)) / alm
    X, Zm = M1 + np.abs(m0), alm * np.abs(m0) + sim * np.abs(e0)
    D1 = abs(1 - sim * c1) / alm
    bx = 8 * (U * (X + M0) + TINY) + D1 * U * (6 * alm * M0 + 5 * Zm)
    cz, cx = row64[9], row64[10]
    return bx, np.abs(cx) * bx + U * (3 * np.abs(z * cz) + 2 * np.abs(cx) * X) + TINY


@pytest.mark.parametrize("pred,s_pred", [("eps", "eps"), ("v", "v"), ("eps", "v"), ("v", "eps")])
def test_distill_target_of_a_callable_teacher_in_closed_form(pred, s_pred):
    """The exact predictors of Gaussian data (solver_ref.gaussian_model, vpred_ref.gaussian_v_model) are linear in z, so the target
    is too: the GPU result with the teacher as a plain callable -- one fp32 scalar per timestep times z -- against the fp64 chain
    of tests/distill_ref.py over the fp64 predictor (``closed_form_bound``; a v teacher adds ddimx_v_to_eps: see below)."""
    dev, var = G.dev(), 0.25
    a = MH.alphas()
    a64 = R.table64(a.numpy())
    fn64 = solver_ref.gaussian_model(a, var)
    net64 = fn64 if pred == "eps" else V.gaussian_v_model(a, var)
    coefs = _dev32(np.array([net64(1.0, t) for t in range(1000)]))
    calls = []

    def teacher(x, t):
        calls.append(t.tolist())
        return x * coefs[t].view(-1, 1, 1, 1)

    z = synth.gaussian("distill.closed", (2, 2, 8, 16))
    args = (teacher, z.to(dev), torch.tensor(K), SEQ, a)
    target, t, x0 = D.distill_target(*args, prediction=pred, student_prediction=s_pred, return_x0=True)
    assert calls == [[870, 999], [3, 990]]
    rows64 = distill_coefficients(SEQ, a, s_pred)[K]
    worst = 0.0
    for i in range(2):
        zi = z[i].double().numpy()
        want_t, want_x = R.distill_target(fn64, zi, K[i], SEQ, a.numpy(), s_pred)
        bx, bt = closed_form_bound(zi, a64, var, rows64[i], SEQ, K[i])
        if pred == "v":
            # eps = fma(v, s2, rn(z s1)) of an fp32 v = c z: v's error 2 u |v| times s2, s2 and s1 rounded (u |v s2| + u |z s1|), the
            # product (u |z s1|) and the fma (u |eps| <= u (|z s1| + |v s2|)): at most 4 u (|z s1| + |v s2|).  For this model, with
            # D = a var + 1 - a <= 1, |z s1| = D |eps| and |v s2| = a (1 - var) |eps| <= 0.75 |eps|: at most 7 u |eps| where the eps
            # teacher has 2 u |eps| -- under 4 times its term, wherever that term enters.  Both bounds scale by 4.
            bx, bt = 4 * bx, 4 * bt
        ex, et = np.abs(x0[i].cpu().double().numpy() - want_x), np.abs(target[i].cpu().double().numpy() - want_t)
        assert (ex <= bx).all() and (et <= bt).all(), f"sample {i}: {np.max(ex / bx):.3f}, {np.max(et / bt):.3f} x bound"
        worst = max(worst, float(np.max(ex / bx)), float(np.max(et / bt)))
    print(f"[distill_target closed form {pred}->{s_pred}] worst error {worst:.3f} x bound")


# ---- 4. training --------------------------------------------------------------------------------------------------------------------------
def _weighted_v_model(name, dtype_str, seed, dropout=0.0):
    return MH.build(name, dtype_str, seed, mode="train", kind="v", dropout=dropout, optimizer="Adam", loss_weight="min_snr")


def _qsample(x0, e, a, t):
    z = torch.empty_like(x0)
    chk(_lib.load().ddimx_qsample(P(x0), P(e), P(a), P(t), P(z), x0.size(0), x0[0].numel(), _lib.stream()))
    return z


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_target_loss_with_the_noise_as_target_is_noise_estimation_loss(mode):
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 5, mode="train", dropout=0.0, optimizer="Adam")
    dev = G.dev()
    a = MH.alphas(cfg).to(dev)
    x0, e = synth.gaussian("ragged.x0", (3, 2, 24, 32)).to(dev), synth.gaussian("ragged.e", (3, 2, 24, 32)).to(dev)
    t = torch.tensor([0, 999, 412], device=dev)
    z = _qsample(x0, e, a, t)
    want, got = losses.noise_estimation_loss(m, x0, t, e, a, keepdim=True), losses.target_loss(m, z, t, e, keepdim=True)
    assert torch.equal(got, want) and got.shape == (3,)
    # the mean and its gradients: one forward and backward after the other
    want_mean = losses.noise_estimation_loss(m, x0, t, e, a)
    want_mean.backward()
    ga = [p.grad.clone() for p in m.parameters()]
    m.zero_grad()
    got_mean = D.target_loss(m, z, t, e)
    assert got_mean.grad_fn is not None
    got_mean.backward()
    assert torch.equal(got_mean, want_mean) and all(torch.equal(x, p.grad) for x, p in zip(ga, m.parameters()))
    with pytest.raises(ValueError, match="weight"):
        losses.target_loss(m, z, t, e, weight=torch.ones(1000))  # a host table
    with pytest.raises(ValueError, match="weight"):
        losses.noise_estimation_loss(m, x0, t, e, a, weight=torch.ones(1000, dtype=torch.float64, device=dev))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape,tt", [((2, 2, 16, 32), [3, 870]), ((3, 2, 24, 32), [0, 999, 412])], ids=["tiny", "ragged"])
def test_weighted_loss_and_parameter_gradients_vs_oracle(mode, shape, tt):
    """A v model with ``loss_weight: min_snr``: the weighted loss and every parameter gradient against autograd through the oracle,
    under the gates of test_gpu_train.py -- ``model_harness.backward_case`` with this feature's collaborators, as in test_gpu_vpred.py: the
    model, the loss under test (``v_prediction_loss`` with the state's table) and the reference loss (vpred_ref's per-sample
    values times the fp64 table's entries, then the mean)."""
    made = {}

    def model(name, dtype_str, seed, dropout=0.0):
        made["cfg"], made["m"] = _weighted_v_model(name, dtype_str, seed, dropout)
        return made["cfg"], made["m"]

    def loss(m, x0, t, e, a):
        st = train.TrainingState(made["cfg"], m)
        assert st.loss_weight is not None and not st.loss_weight.is_cuda
        return losses.loss_registry["v"](m, x0, t, e, a, weight=st.device_loss_weight(x0.device))

    def ref_loss(model_fn, x0, t, e, a):
        w = torch.from_numpy(loss_weight_table(a, "v", "min_snr", 5.0))[t]
        return (V.v_prediction_loss(model_fn, x0, t, e, a, keepdim=True) * w.to(torch.float32)).mean()

    MH.backward_case(mode, shape, tt, build_model=model, loss=loss, ref_loss=ref_loss)


DSEQ = [0, 3, 500, 870]  # student steps: k = 0 at t = 3 (ends at the data), k = 1 at t = 870


def _teacher_model(dtype_str):
    return MH.pair("tiny", dtype_str)[2]  # type simple, eval mode


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape,kk", [((2, 2, 16, 32), [0, 1]), ((3, 2, 24, 32), [1, 0, 1])], ids=["tiny", "ragged"])
def test_distillation_loss_and_parameter_gradients_vs_oracle(mode, shape, kk):
    """The loss ``distill_step`` differentiates -- the q-sample, the target of an eps teacher in the v student's prediction, the
    min_snr-weighted squared error -- and every parameter gradient against autograd through the ORACLE student on the
    GPU-computed target, under the gates of test_gpu_train.py (``model_harness.backward_case`` with this feature's collaborators)."""
    dtype_str, dt = mode
    teacher = _teacher_model(dtype_str)
    tt = [DSEQ[2 * k + 1] for k in kk]
    made = {}

    def model(name, dtype_str, seed, dropout=0.0):
        made["cfg"], made["m"] = _weighted_v_model(name, dtype_str, seed, dropout)
        return made["cfg"], made["m"]

    def loss(m, x0, t, e, a):
        assert t.tolist() == tt
        st = train.TrainingState(made["cfg"], m)
        z = _qsample(x0, e, a, t)
        target, t2 = D.distill_target(teacher, z, torch.tensor(kk), DSEQ, a, student_prediction="v")
        assert torch.equal(t2, t)
        made["z"], made["target"] = z.cpu(), target.cpu()
        return losses.target_loss(m, z, t, target, weight=st.device_loss_weight(z.device))

    def ref_loss(model_fn, x0, t, e, a):
        w = torch.from_numpy(loss_weight_table(a, "v", "min_snr", 5.0))[t].to(torch.float32)
        per = (made["target"] - model_fn(made["z"], t)).square().sum(dim=(1, 2, 3))
        return (per * w).mean()

    MH.backward_case(mode, shape, tt, build_model=model, loss=loss, ref_loss=ref_loss)


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "min_snr"])
def test_distill_step_is_the_composition_by_hand(weighted):
    """Loss, norms and every parameter after one ``distill_step`` are ``torch.equal`` to ddimx_qsample -> ``distill_target`` ->
    ``target_loss`` -> ``train.finish_step`` by hand on a twin; the teacher's parameters and buffers are bit-unchanged; and the
    default ``k`` is a mirrored draw.  bf16 mode, dropout 0.1, v student of an eps teacher."""
    dtype_str = "torch.cuda.BFloat16Tensor"
    dev = G.dev()
    d = MH.config_dict("tiny", dtype_str, kind="v", optimizer="AdamW", loss_weight="min_snr" if weighted else None)
    cfg = configs.dict2namespace(d)
    a = MH.alphas(cfg).to(dev)
    teacher = _teacher_model(dtype_str)
    before = {k: v.clone() for k, v in teacher.state_dict().items()}
    x, e = synth.gaussian("dstep.x", (4, 2, 32, 32)).to(dev), synth.gaussian("dstep.e", (4, 2, 32, 32)).to(dev)
    k = torch.tensor([0, 1, 1, 0])
    seq16 = list(range(40, 1000, 60))
    assert len(seq16) == 16

    def fresh():
        torch.manual_seed(77)
        m = synth.fill_module(D.Model(cfg), 11)
        return m, train.TrainingState(cfg, m)

    ma, sa = fresh()
    loss_a, norms_a = D.distill_step(ma, teacher, x, sa, a, DSEQ, e=e, k=k)
    mb, sb = fresh()
    mb.train()
    t = torch.tensor([3, 870, 870, 3], device=dev)
    z = _qsample(x, e, a, t)
    target, t2 = D.distill_target(teacher, z, k, DSEQ, a, student_prediction="v")
    loss_b = losses.target_loss(mb, z, t2, target, weight=sb.device_loss_weight(dev))
    loss_b, norms_b = train.finish_step(mb, sb, loss_b)
    assert torch.equal(loss_a, loss_b) and bool(torch.isfinite(loss_a)) and norms_a.keys() == norms_b.keys() and len(norms_a) >= 1
    assert all(torch.equal(norms_a[n], norms_b[n]) for n in norms_a)
    start = dict(fresh()[0].named_parameters())
    for (name, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(pa, pb), name
        assert torch.equal(sa.ema_helper.shadow[name], sb.ema_helper.shadow[name]), name
    assert any(not torch.equal(pa, start[name]) for name, pa in ma.named_parameters())  # the step trained
    assert (sa.loss_weight is not None) == weighted
    for name, v in teacher.state_dict().items():
        assert torch.equal(v, before[name]), name
    assert not teacher.training
    # the default draw: mirrored, inside the student's steps; a second step on a 16 -> 8 round runs
    kd = distill.mirrored_steps(5, 8, generator=torch.Generator().manual_seed(3))
    assert kd.shape == (5,) and torch.equal(kd[3:], 7 - kd[:2]) and int(kd.min()) >= 0 and int(kd.max()) <= 7
    loss_c, _ = D.distill_step(ma, teacher, x, sa, a, seq16)
    assert bool(torch.isfinite(loss_c)) and halve_seq(seq16) == seq16[1::2]


def test_graphed_train_step_with_a_loss_weight_is_bit_identical_to_eager():
    """As test_gpu_vpred's graphed-equals-eager test, with ``loss_weight: min_snr`` on the v model: two eager warm-up steps, one
    capture, three replays leave what five eager ``train_step``s leave -- the captured weighted loss reads its timesteps when it
    runs.  The first loss differs from the uniform one."""
    d = MH.config_dict("tiny", "torch.cuda.BFloat16Tensor", kind="v", optimizer="AdamW", loss_weight="min_snr")
    d["optimization"]["optimizer"]["default"]["warmup"] = 3
    cfg = configs.dict2namespace(d)
    alphas = MH.alphas(cfg).cuda()
    n = 5
    xs = [synth.gaussian(f"vgraphed.x{i}", (4, 2, 32, 32)).cuda() for i in range(n)]
    es = [synth.gaussian(f"vgraphed.e{i}", (4, 2, 32, 32)).cuda() for i in range(n)]
    ts = [torch.tensor([10 + i, 500, 989 - i, 250]) for i in range(n)]  # the weight is below 1 at t = 10 + i and 989 - i

    def run(graphed, c=cfg):
        torch.manual_seed(77)
        m = synth.fill_module(D.Model(c), 11)
        st = train.TrainingState(c, m)
        step = train.GraphedTrainStep(m, st, alphas, warmup=2) if graphed else None
        out = []
        for i in range(n if c is cfg else 1):
            if graphed:
                loss, norms = step(xs[i], e=es[i], t=ts[i])
            else:
                loss, norms = train.train_step(m, xs[i], st, alphas, e=es[i], t=ts[i])
            out.append((float(loss), {k: float(v) for k, v in norms.items()}))
        if graphed:
            assert step.graph is not None
            step.close()
        return m, st, out

    ma, sa, oa = run(False)
    mb, sb, ob = run(True)
    assert oa == ob, (oa, ob)
    assert all(np.isfinite(l) for l, _ in oa) and len(oa[0][1]) >= 1
    assert sa.loss_weight.is_cuda and sb.loss_weight.is_cuda
    for (name, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(pa, pb), name
        assert torch.equal(sa.ema_helper.shadow[name], sb.ema_helper.shadow[name]), name
    d_u = dict(d, model={k: v for k, v in d["model"].items() if k != "loss_weight"})
    _, su, ou = run(False, configs.dict2namespace(d_u))
    assert su.loss_weight is None and abs(ou[0][0] - oa[0][0]) > 1e-2 * oa[0][0]


def test_a_configuration_without_a_weight_never_reaches_the_weighted_kernels(monkeypatch):
    """``train_step`` on a config without ``loss_weight`` (and with ``uniform``) makes the launches it made before: a spy in
    ``ddimxd_sqerr_loss_w``'s place is never called, while the unweighted kernel is; with ``min_snr`` the spy IS called."""
    lib, dev = _lib.load(), G.dev()
    seen = {"w": 0, "plain": 0}
    real_w, real_plain = lib.ddimxd_sqerr_loss_w, lib.ddimx_sqerr_loss

    def spy_w(*args):
        seen["w"] += 1
        return real_w(*args)

    def spy_plain(*args):
        seen["plain"] += 1
        return real_plain(*args)

    monkeypatch.setattr(lib, "ddimxd_sqerr_loss_w", spy_w)
    monkeypatch.setattr(lib, "ddimx_sqerr_loss", spy_plain)
    x, e = synth.gaussian("spy.x", (2, 2, 16, 32)).to(dev), synth.gaussian("spy.e", (2, 2, 16, 32)).to(dev)
    t = torch.tensor([3, 870])
    out = {}
    for kind in (None, "uniform", "min_snr"):
        d = MH.config_dict("tiny", "torch.cuda.FloatTensor", kind="v", dropout=0.0, loss_weight=kind)
        cfg = configs.dict2namespace(d)
        m = synth.fill_module(D.Model(cfg), 5)
        seen.update(w=0, plain=0)
        loss, _ = train.train_step(m, x, train.TrainingState(cfg, m), MH.alphas(cfg).to(dev), e=e, t=t)
        out[kind] = float(loss)
        assert (seen["w"], seen["plain"]) == ((1, 0) if kind == "min_snr" else (0, 1)), (kind, seen)
    assert out[None] == out["uniform"] and out["min_snr"] < out[None]  # t = 3 carries a weight below 1
