"""The kernels that run after the backward pass, one by one through their own C-ABI entry points, against the references of
tests/tail_kernel_ref.py: qsample, sqerr_part / sqerr_final, sqerr_bwd (both forms), ema_multi, sqnorm_multi / sqnorm_final, scale_multi
and adam_multi (by-value and device scalars, with and without the in-register clip).

Every tensor a kernel writes lives inside a sentinel-filled allocation with guard bands (``Out`` of tests/kernel_harness.py: every
byte 0xFF, a NaN in fp32) whose other bytes must still be 0xFF afterwards; scratch (``partial``) is NaN before each call; every
read-only input (``Ro``, same module) must be bitwise unchanged.  qsample, scale and EMA are
compared bit for bit; integer-valued losses bit for bit; the rest at the gates derived in tail_kernel_ref.py, every element of every
output.  The gated tests print the measured worst errors in units of their gate."""
import ctypes

import numpy as np
import pytest
import torch

from ddim_audio_amd import _lib
import gpu_util as G
from kernel_harness import NAN, Out, Ro, lib as L, refused, report, same, sync
import tail_kernel_ref as R

pytestmark = pytest.mark.gpu
F = np.float32


class Table:
    """Device pointer / size / block tables over lists of Out / Ro (one entry per tensor each), built by the reference's builder."""

    def __init__(self, sizes, *lists):
        bt, bo = R.tables(sizes)
        mk = lambda v, dt: torch.tensor(v, dtype=dt, device=G.dev())  # noqa: E731
        self.sizes, self.bt, self.bo, self.nblk = mk(list(sizes), torch.int64), mk(bt, torch.int32), mk(bo, torch.int64), len(bt)
        self.ptrs = [mk([x.addr for x in xs], torch.int64) for xs in lists]

    def args(self):
        return _lib.ptr(self.sizes), _lib.ptr(self.bt), _lib.ptr(self.bo), self.nblk


# ---- q-sample ----------------------------------------------------------------------------------------------------------------------------
ALPHAS = R.alphas()


@pytest.mark.parametrize("B", sorted(R.QS_T))
@pytest.mark.parametrize("per", R.QS_PER)
def test_qsample(per, B):
    """qsample_kernel against the reference expression in fp32, bit for bit: t at both ends of the table and repeated in the batch, lengths
    around one block and one that needs a second grid-stride trip under the 1024-block cap."""
    x0, e, al = Ro(R.gauss(f"qs.x0.{per}.{B}", (B, per))), Ro(R.gauss(f"qs.e.{per}.{B}", (B, per))), Ro(ALPHAS)
    for tl in R.QS_T[B]:
        t, x = Ro(tl, torch.int64), Out(B * per)
        _lib.check(L().ddimx_qsample(x0.ptr, e.ptr, al.ptr, t.ptr, x.ptr, B, per, _lib.stream()))
        sync()
        got = x.read("qsample").numpy().reshape(B, per)
        same(got, R.qsample(x0.keep.cpu().numpy(), e.keep.cpu().numpy(), ALPHAS, tl), (per, B, tl))
        for r in (x0, e, al, t):
            r.check("qsample")


# ---- loss --------------------------------------------------------------------------------------------------------------------------------
def run_sqerr(e, out):
    B, per = e.shape
    ed, od, partial, loss = Ro(e), Ro(out), Out(B * R.SQ_PARTS), Out(B + 1)
    _lib.check(L().ddimx_sqerr_loss(ed.ptr, od.ptr, partial.ptr, loss.ptr, B, per, _lib.stream()))
    sync()
    ed.check("sqerr_loss"), od.check("sqerr_loss")
    parts = partial.read("sqerr partial").numpy()
    assert not np.isnan(parts).any(), "every part writes its slot, the ones past the end of the sample too"
    return loss.read("sqerr loss").numpy(), parts.reshape(B, R.SQ_PARTS)


@pytest.mark.parametrize("B", R.SQ_B)
@pytest.mark.parametrize("per", R.SQ_PER)
def test_sqerr_loss(per, B):
    """sqerr_part_kernel + sqerr_final_kernel.  Integer differences: every sum is exact, so loss[b] -- and loss[B] where B is a power of
    two -- equal the fp64 sums bit for bit, and the parts past the end of the sample hold 0.  Gaussian: within k 2^-24 loss.
    Measured on MI355X: at most 0.17 of the gate."""
    e, out = R.loss_inputs(B, per, integer=True)
    want = R.sqerr(e, out)
    got, parts = run_sqerr(e, out)
    assert np.array_equal(got[:B].astype(np.float64), want[:B]), (got, want)
    chunk = -(-per // R.SQ_PARTS)
    d2 = np.zeros((B, R.SQ_PARTS * chunk))
    d2[:, :per] = (e.astype(np.float64) - out) ** 2
    assert np.array_equal(parts.astype(np.float64), d2.reshape(B, R.SQ_PARTS, chunk).sum(2))
    if B & (B - 1) == 0:
        assert float(got[B]) == want[B]
    else:
        assert abs(float(got[B]) - want[B]) <= R.U * want[B]  # one division
    e, out = R.loss_inputs(B, per)
    want = R.sqerr(e, out)
    got, _ = run_sqerr(e, out)
    w = R.worst(got - want, R.sqerr_gate(want, per))
    report(f"sqerr_loss per={per} B={B}", w)
    assert w <= 1.0


@pytest.mark.parametrize("B", R.BWD_B)
@pytest.mark.parametrize("per", R.SQ_PER)
def test_sqerr_loss_bwd(per, B):
    """sqerr_bwd_kernel in both forms: the per-sample gradient alone (which must not read g[B]: it is NaN here) and with the gradient
    of the batch mean; Gaussian and one-hot upstream gradients.  Measured on MI355X: at most 0.44 of the gate."""
    e, out = R.loss_inputs(B, per)
    ed, od = Ro(e), Ro(out)
    worst = 0.0
    grads = [R.loss_grads(B)] + [R.loss_grads(B, onehot=b) for b in range(B + 1)]
    for g in grads:
        for with_mean in (0, 1):
            gh = g.copy()
            if not with_mean:
                gh[B] = NAN
            gd, d = Ro(gh), Out(B * per)
            fn = L().ddimx_sqerr_loss_bwd_mean if with_mean else L().ddimx_sqerr_loss_bwd
            _lib.check(fn(ed.ptr, od.ptr, gd.ptr, d.ptr, B, per, _lib.stream()))
            sync()
            got = d.read("sqerr_bwd").numpy().reshape(B, per)
            want = R.sqerr_bwd(e, out, g, with_mean)
            worst = max(worst, R.worst(got - want, R.sqerr_bwd_gate(want)))
            for r in (ed, od, gd):
                r.check("sqerr_bwd")
    report(f"sqerr_loss_bwd per={per} B={B}", worst)
    assert worst <= 1.0


# ---- EMA ---------------------------------------------------------------------------------------------------------------------------------
def ema_launch(tb, c_param, c_shadow):
    _lib.check(L().ddimx_ema_update_multi_coef(_lib.ptr(tb.ptrs[0]), _lib.ptr(tb.ptrs[1]), *tb.args(), c_param, c_shadow, _lib.stream()))


@pytest.mark.parametrize("mu", R.MUS)
def test_ema(mu):
    """ema_multi_kernel through ddimx_ema_update_multi_coef with the coefficients as EMAHelper.update passes them (1.0 - mu and mu as
    doubles): two updates in a row equal the reference's (1.0 - mu) * p + mu * shadow bit for bit; updating every tensor in a launch of
    its own gives the same bits.  The first export, which can only form 1 - fp32(mu), equals the reference evaluated with THAT
    coefficient -- and for mu = 0.9999 / 0.999 misses the true one on 6 529 / 5 153 of these 32 781 elements (printed)."""
    params = [R.gauss(f"ema.p.{n}", n) for n in R.SIZES]
    shadows = [(F(0.99) * p - F(0.003)).astype(F) for p in params]
    P, S = [Ro(p) for p in params], [Out(n, init=s) for n, s in zip(R.SIZES, shadows)]
    tb = Table(R.SIZES, S, P)
    want = shadows
    for _ in range(2):
        ema_launch(tb, 1.0 - mu, mu)
        sync()
        want = [R.ema(s, p, mu) for s, p in zip(want, params)]
        for s, w in zip(S, want):
            same(s.read("ema shadow"), w, "ema shadow")
    for p in P:
        p.check("ema")
    # one tensor per launch
    S1 = [Out(n, init=s) for n, s in zip(R.SIZES, shadows)]
    for s, p, n in zip(S1, P, R.SIZES):
        ema_launch(Table([n], [s], [p]), 1.0 - mu, mu)
    sync()
    one = [R.ema(s, p, mu) for s, p in zip(shadows, params)]
    for s, w in zip(S1, one):
        same(s.read("ema shadow, one tensor"), w, "ema shadow, one tensor")
    # the first export: the coefficient of the rounded mu
    S2 = [Out(n, init=s) for n, s in zip(R.SIZES, shadows)]
    tb2 = Table(R.SIZES, S2, P)
    _lib.check(L().ddimx_ema_update_multi(_lib.ptr(tb2.ptrs[0]), _lib.ptr(tb2.ptrs[1]), *tb2.args(), mu, _lib.stream()))
    sync()
    old = [s.read("ema shadow, first export").numpy() for s in S2]
    for a, s, p in zip(old, shadows, params):
        same(a, R.ema(s, p, mu, c_param=R.ema_old_coef(mu)), "ema shadow, first export")
    diff = sum(int((a.view(np.int32) != b.view(np.int32)).sum()) for a, b in zip(old, one))
    print(f"[ema mu={mu}] the first export differs from the reference on {diff} of {sum(R.SIZES)} elements")
    assert (diff > 0) == (mu != 0.5)


# ---- gradient norm, clip coefficient, scaling --------------------------------------------------------------------------------------------------
def run_scale(gs, coef_dev):
    Gb = [Out(g.size, init=g) for g in gs]
    tb = Table([g.size for g in gs], Gb)
    _lib.check(L().ddimx_scale_multi(_lib.ptr(tb.ptrs[0]), *tb.args(), coef_dev.ptr, _lib.stream()))
    sync()
    coef_dev.check("scale_multi")
    return [b.read("scale_multi").numpy() for b in Gb], Gb


@pytest.mark.parametrize("case", R.norm_cases(), ids=lambda c: c[0])
def test_grad_norm_and_scale(case):
    """sqnorm_multi_kernel + sqnorm_final_kernel: out[0] within 13 2^-24 of the fp64 norm, out[1] the fp32 formula applied to the kernel's
    own out[0] bit for bit.  scale_multi_kernel with that coefficient (read from out + 1, as clip_grad_norm_ passes it), with 0.37 and
    with 1: g * c bit for bit, bitwise untouched for 1.  Measured on MI355X: out[0] at most 0.07 of the gate."""
    name, gs = case
    Gr = [Ro(g) for g in gs]
    tb = Table(R.SIZES, Gr)
    partial, out = Out(tb.nblk), Out(2)
    _lib.check(L().ddimx_grad_norm_multi(_lib.ptr(tb.ptrs[0]), *tb.args(), R.MAX_NORM, partial.ptr, out.ptr, _lib.stream()))
    sync()
    for r in Gr:
        r.check("grad_norm_multi")
    assert not np.isnan(partial.read("grad_norm partial").numpy()).any()
    got = out.read("grad_norm out").numpy()
    want, coef = R.grad_norm(gs, R.MAX_NORM)
    w = abs(float(got[0]) - want) / R.grad_norm_gate(want)
    report(f"grad_norm_multi {name}", w)
    assert w <= 1.0
    same(got[1], R.clip_coef32(got[0], R.MAX_NORM), "the clip coefficient")
    assert (got[1] == 1.0) == (name == "below") and abs(float(got[1]) - coef) <= 16 * R.U * coef
    for c in (got[1], F(0.37), F(1.0)):
        cd = Ro(np.array([NAN, c], F))
        cd.t = cd.t[1:]  # the coefficient is read from where the caller points
        cd.keep = cd.keep[1:]
        res, _ = run_scale(gs, cd)
        for a, g in zip(res, gs):
            same(a, R.scale(g, c), f"scale_multi by {c}")
            if c == 1.0:
                same(a, g, "scale_multi by 1")


# ---- Adam / AdamW / AdaBelief ----------------------------------------------------------------------------------------------------------------
class AdamRun:
    """One launch set over fresh copies of a state: p, m, v in guarded buffers, g read-only (or a guarded copy when it is to be scaled)."""

    def __init__(self, tensors, scaled_g=False):
        self.sizes = [t[0].size for t in tensors]
        self.P, self.M, self.V = ([Out(t[0].size, init=t[k]) for t in tensors] for k in (0, 2, 3))
        self.Gd = [Out(t[1].size, init=t[1]) if scaled_g else Ro(t[1]) for t in tensors]
        self.scaled_g = scaled_g

    def table(self, idx=None):
        idx = range(len(self.sizes)) if idx is None else idx
        pick = lambda xs: [xs[i] for i in idx]  # noqa: E731
        return Table(pick(self.sizes), pick(self.P), pick(self.Gd), pick(self.M), pick(self.V))

    def launch(self, tb, hp, wd, decoupled, step, clip=None, dyn=None):
        b1, b2 = hp["betas"]
        head = [_lib.ptr(p) for p in tb.ptrs] + list(tb.args()) + [None if clip is None else clip.ptr]
        if dyn is None:
            rc = L().ddimx_adam_multi(*head, hp["lr"], b1, b2, hp["eps"], wd, step, decoupled, _lib.stream())
        else:
            rc = L().ddimx_adam_multi_dyn(*head, dyn.ptr, b1, b2, hp["eps"], wd, decoupled, _lib.stream())
        _lib.check(rc)

    def result(self, what):
        sync()
        if not self.scaled_g:
            for g in self.Gd:
                g.check(what)
        return [[b.read(what).numpy() for b in bs] for bs in (self.P, self.M, self.V)]


def assert_same_runs(a, b, what):
    for xs, ys in zip(a, b):
        for x, y in zip(xs, ys):
            same(x, y, what)


@pytest.mark.parametrize("cfg", R.adam_configs(), ids=R.adam_id)
def test_adam_multi(cfg):
    """adam_multi_kernel over every (step, gradient scale) of one (mode, weight decay, hyperparameter set): p, m and v of every element
    against the fp64 update at the gates of tail_kernel_ref.py, and with torch.equal-strength equalities: the device-scalar export with
    dyn_scalars(step), one tensor per launch, and the in-register clip coefficient (clip[1]; clip[0] is NaN) against scale_multi
    followed by an unclipped step.  Where g = 0 meets the zero state (step 1) and wd = 0 the parameter keeps its bits.
    Measured on MI355X: p at most 0.47, m 0.24, v 0.48 of their gates."""
    decoupled, wd, hi = cfg
    hp = R.HYPER[hi]
    wp = wm = wv = 0.0
    for step, gscale, tensors in R.adam_cases(cfg):
        what = f"adam {R.adam_id(cfg)} step {step} g {gscale:g}"
        a = AdamRun(tensors)
        a.launch(a.table(), hp, wd, decoupled, step)
        got = a.result(what)
        for i, (p, g, m, v) in enumerate(tensors):
            w = R.adam(p, g, m, v, step, hp, wd, decoupled)
            gp, gm, gv = R.adam_gates(w)
            wp = max(wp, R.worst(got[0][i] - w["p"], gp))
            wm = max(wm, R.worst(got[1][i] - w["m"], gm))
            wv = max(wv, R.worst(got[2][i] - w["v"], gv))
            if step == 1 and wd == 0:
                z = g == 0
                assert z.any()
                same(got[0][i][z], p[z], f"{what}: a zero gradient on the zero state moved the parameter")
        assert wp <= 1.0 and wm <= 1.0 and wv <= 1.0, f"{what}: p {wp:.3f} m {wm:.3f} v {wv:.3f} of the gates"
        # device scalars
        b = AdamRun(tensors)
        dyn = Ro(np.array(R.dyn_scalars(hp, step), F))
        b.launch(b.table(), hp, wd, decoupled, step, dyn=dyn)
        assert_same_runs(b.result(what + " dyn"), got, what + " dyn")
        dyn.check(what)
        # one tensor per launch
        c = AdamRun(tensors)
        for i in range(len(tensors)):
            c.launch(c.table([i]), hp, wd, decoupled, step)
        assert_same_runs(c.result(what + " single"), got, what + " single")
        # the clip coefficient in registers == scale_multi, then no clip
        for coef in (F(1.0), F(0.37)):
            clip = Ro(np.array([NAN, coef], F))
            d = AdamRun(tensors)
            d.launch(d.table(), hp, wd, decoupled, step, clip=clip)
            s = AdamRun(tensors, scaled_g=True)
            tb = s.table()
            _lib.check(L().ddimx_scale_multi(_lib.ptr(tb.ptrs[1]), *tb.args(), ctypes.c_void_p(clip.addr + 4), _lib.stream()))
            s.launch(tb, hp, wd, decoupled, step)
            res = s.result(what + " scaled")
            for gb, t in zip(s.Gd, tensors):
                same(gb.read("scaled g"), R.scale(t[1], coef), "scaled g")
            assert_same_runs(d.result(what + " clip"), res, what + f" clip {coef}")
            clip.check(what)
            if coef == 1.0:
                assert_same_runs(res, got, what + " clip 1")
    report(f"adam_multi {R.adam_id(cfg)}", max(wp, wm, wv), f"of the gates (p {wp:.3f} m {wm:.3f} v {wv:.3f})")


# ---- refused arguments -------------------------------------------------------------------------------------------------------------------
def test_rejections_loss_and_qsample():
    B, per = 2, 64
    x0, e, al, t = Ro(R.gauss("rej.x0", (B, per))), Ro(R.gauss("rej.e", (B, per))), Ro(ALPHAS), Ro([0, 999], torch.int64)
    s = _lib.stream()
    x = Out(B * per)
    q = L().ddimx_qsample
    for bad in range(5):
        a = [x0.ptr, e.ptr, al.ptr, t.ptr, x.ptr]
        a[bad] = None
        refused(q(*a, B, per, s), x, who="ddimx_qsample")
    for b_, p_ in ((0, per), (65536, per), (-1, per), (B, 0), (B, -4)):
        refused(q(x0.ptr, e.ptr, al.ptr, t.ptr, x.ptr, b_, p_, s), x, who="ddimx_qsample")
    partial, loss = Out(B * R.SQ_PARTS), Out(B + 1)
    f = L().ddimx_sqerr_loss
    for bad in range(4):
        a = [x0.ptr, e.ptr, partial.ptr, loss.ptr]
        a[bad] = None
        refused(f(*a, B, per, s), partial, loss, who="ddimx_sqerr_loss")
    for b_, p_ in ((0, per), (65536, per), (B, 0)):
        refused(f(x0.ptr, e.ptr, partial.ptr, loss.ptr, b_, p_, s), partial, loss, who="ddimx_sqerr_loss")
    g, d = Ro(R.loss_grads(B)), Out(B * per)
    for name in ("ddimx_sqerr_loss_bwd", "ddimx_sqerr_loss_bwd_mean"):
        f = getattr(L(), name)
        for bad in range(4):
            a = [x0.ptr, e.ptr, g.ptr, d.ptr]
            a[bad] = None
            refused(f(*a, B, per, s), d, who=name)
        for b_, p_ in ((0, per), (65536, per), (B, 0)):
            refused(f(x0.ptr, e.ptr, g.ptr, d.ptr, b_, p_, s), d, who=name)


def test_rejections_multi_tensor():
    """Nulls, a negative block count, step 0 and an unknown mode are refused before any launch; an empty table (nblocks = 0) returns 0
    without one."""
    sizes = (5, R.BLOCK + 1)
    st = [R.adam_state("rej", n, 2, 1.0) for n in sizes]
    a = AdamRun(st, scaled_g=True)
    outs = a.P + a.M + a.V + a.Gd
    before = [o.t.clone() for o in outs]
    tb = a.table()
    s = _lib.stream()
    sizes_, bt, bo, nblk = tb.args()
    pp, gp, mp, vp = (_lib.ptr(p) for p in tb.ptrs)
    partial, out, coef = Out(nblk), Out(2), Ro(np.array([0.5], F))
    hp = (5e-4, 0.9, 0.998, 1e-6, 0.0)
    dyn = Ro(np.array(R.dyn_scalars(R.HYPER[0], 2), F))
    calls = {
        "ddimx_ema_update_multi_coef": lambda t, n: L().ddimx_ema_update_multi_coef(*t[:2], *t[4:7], n, 0.1, 0.9, s),
        "ddimx_ema_update_multi": lambda t, n: L().ddimx_ema_update_multi(*t[:2], *t[4:7], n, 0.9, s),
        "ddimx_grad_norm_multi": lambda t, n: L().ddimx_grad_norm_multi(t[1], *t[4:7], n, 1.0, t[7], t[8], s),
        "ddimx_scale_multi": lambda t, n: L().ddimx_scale_multi(t[1], *t[4:7], n, t[9], s),
        "ddimx_adam_multi": lambda t, n, step=2, mode=1: L().ddimx_adam_multi(*t[:7], n, None, *hp, step, mode, s),
        "ddimx_adam_multi_dyn": lambda t, n, mode=1: L().ddimx_adam_multi_dyn(*t[:7], n, None, t[10], *hp[1:], mode, s),
    }
    used = {"ddimx_ema_update_multi_coef": (0, 1, 4, 5, 6), "ddimx_ema_update_multi": (0, 1, 4, 5, 6), "ddimx_grad_norm_multi": (1, 4, 5, 6, 7, 8),
            "ddimx_scale_multi": (1, 4, 5, 6, 9), "ddimx_adam_multi": (0, 1, 2, 3, 4, 5, 6), "ddimx_adam_multi_dyn": (0, 1, 2, 3, 4, 5, 6, 10)}
    full = [pp, gp, mp, vp, sizes_, bt, bo, partial.ptr, out.ptr, coef.ptr, dyn.ptr]

    def unchanged(who):
        sync()
        assert all(torch.equal(o.t, b) for o, b in zip(outs, before)), f"{who}: a refused call wrote"
        assert partial.untouched() and out.untouched()

    for name, call in calls.items():
        msg_name = "ddimx_ema_update_multi" if name.startswith("ddimx_ema") else name
        for bad in used[name]:
            t = list(full)
            t[bad] = None
            refused(call(t, nblk), who=msg_name)
            unchanged(name)
        refused(call(full, -1), who=msg_name)
        unchanged(name)
        assert call(full, 0) == 0, name
        unchanged(name)
    refused(calls["ddimx_adam_multi"](full, nblk, step=0), who="ddimx_adam_multi")
    refused(calls["ddimx_adam_multi"](full, nblk, mode=3), who="ddimx_adam_multi")
    refused(calls["ddimx_adam_multi"](full, nblk, mode=-1), who="ddimx_adam_multi")
    refused(calls["ddimx_adam_multi_dyn"](full, nblk, mode=3), who="ddimx_adam_multi_dyn")
    unchanged("adam modes")
    coef.check("rejections"), dyn.check("rejections")
