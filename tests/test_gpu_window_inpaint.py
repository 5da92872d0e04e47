"""Windowed inpainting on the GPU (ddim_audio_amd.windowed_inpaint_steps, ddimxwi_residual / ddimxwi_update).

Bit for bit where the definition reduces to a sampler that existed before: one window = inpaint_steps; an empty mask without
guidance = windowed_steps; no overlap without guidance = inpaint_steps over the segments as a batch.  The two kernels on their own
operands through the C ABI against an fp32 restatement, in guarded buffers.  The sampler against the CPU restatement
(tests/window_inpaint_ref.py: the blend from its definition, the gradient by autograd) over the CPU oracle's forward, at
model_harness's gates.  Replayed against eager steps, canvas-batch invariance, the v model, no side effects, graph ownership."""
import functools

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, synth
from ddim_audio_amd.noise import NoiseStream
from ddim_audio_amd.schedule import inpaint_coefficients, v_table, window_plan
from ddim_audio_amd.window_inpaint import WindowInpaintStepper
from oracle import ref_cpu
import kernel_harness as KH
import model_harness as MH
from model_harness import MODES, MODE_IDS, U
import step_math_ref as SM
import window_inpaint_ref as WI

pytestmark = pytest.mark.gpu
DROPOUT = 0.1  # every model here is built with it, in eval mode: must never be applied
TAPERS = ["flat", "tri"]
ZETA4 = [0.2, 0.3, 0.0, 0.25]
F32 = np.float32


def _mask(kind, shape):
    """test_gpu_inpaint.py's masks, on the canvas."""
    b, c, t, f = shape
    if kind == "gap":    # a time gap (packet loss): [N, 1, L, 1]
        m = torch.ones(b, 1, t, 1)
        m[:, :, t // 4: t // 2] = 0
    elif kind == "band":  # missing high bands (bandwidth extension): [1, 1, 1, F]
        m = torch.ones(1, 1, 1, f)
        m[..., f // 2:] = 0
    else:                 # a time gap with a soft (0.5) edge band, per sample
        m = torch.ones(b, 1, t, f)
        m[:, :, t // 4: t // 2] = 0
        m[:, :, :, -f // 4:] *= 0.5
        m[-1, :, : t // 8] = 0
    return m


def _zeta(n):
    return [ZETA4[i % 4] for i in range(n)]


def _seq(n):
    return list(range(0, 1000, 1000 // n))[:n]


# ---- 1. one window is inpaint_steps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "replace_only"])
@pytest.mark.parametrize("n", [3, 10], ids=["eager", "replayed"])
@pytest.mark.parametrize("name,T", [("tiny", 16), ("audio", 32)])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_one_window_is_inpaint_steps(mode, name, T, n, guided):
    """L = T: the blend is a select, the seed is the canvas seed, the overlap-add one term, and the norm's partials have
    inpaint_residual_kernel's block count and order for a sample of C L F elements."""
    cfg, m = MH.build(name, mode[0], 5, mode="eval", dropout=DROPOUT)
    shape = (2, 2, T, cfg.model.f_size)
    x, y = MH.pair_data("winp.one", shape)
    mask = _mask("soft", shape)
    seq, a = _seq(n), MH.alphas(cfg)
    kw = dict(y=y, mask=mask, guidance=_zeta(n) if guided else 0.0, replace=True)
    want_xs, want_x0 = D.inpaint_steps(x.cuda(), seq, m, a, None, **kw)
    for taper in TAPERS:
        xs, x0 = D.windowed_inpaint_steps(x.cuda(), seq, m, a, None, window=T, taper=taper, **kw)
        assert len(xs) == n + 1 and len(x0) == n and bool(torch.isfinite(xs[-1]).all())
        MH.same_list(xs[1:], want_xs[1:], "xs")
        MH.same_list(x0, want_x0, "x0_preds")
    if guided:
        free = D.windowed_inpaint_steps(x.cuda(), seq, m, a, [0], window=T, y=y, mask=mask, guidance=0.0)
        assert not torch.equal(free[0][1], xs[1]), "the guidance acted"
    # the conventions of generalized_steps: xs[0] is the caller's tensor, updated in place; select_index
    xc = x.cuda()
    sxs, sx0 = D.windowed_inpaint_steps(xc, seq, m, a, [1, -1], window=T, hop=T, **kw)
    assert sxs[0] is xc and torch.equal(xc.cpu(), xs[-1]) and len(sxs) == 3 and len(sx0) == 2
    MH.same_list(sxs[1:], [xs[2], xs[n]], "selected xs")
    MH.same_list(sx0, [x0[1], x0[n - 1]], "selected x0")


# ---- 2. an empty mask without guidance is windowed_steps ------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("replace", [True, False], ids=["replace", "plain"])
@pytest.mark.parametrize("n", [3, 10], ids=["eager", "replayed"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_empty_mask_is_windowed_steps(mode, n, replace, eta):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval", dropout=DROPOUT)
    shape = (2, 2, 48, 32)  # W = 5 windows of 16 at hop 8: ten windows, the captured forward forks
    x, y = MH.pair_data("winp.empty", shape)
    seq, a = _seq(n), MH.alphas(cfg)
    ns = lambda: NoiseStream(0xABCD, 1) if eta else None  # noqa: E731  (the same seed on both sides)
    kw = dict(window=16, hop=8, taper="tri", eta=eta)
    want_xs, want_x0 = D.windowed_steps(x.cuda(), seq, m, a, None, noise=ns(), **kw)
    xs, x0 = D.windowed_inpaint_steps(x.cuda(), seq, m, a, None, y=y, mask=torch.zeros(1, 1, 1, 1), guidance=0.0, replace=replace,
                                      noise=ns(), **kw)
    MH.same_list(xs[1:], want_xs[1:], "xs")
    MH.same_list(x0, want_x0, "x0_preds")
    if eta:
        assert not torch.equal(xs[1], D.windowed_steps(x.cuda(), seq, m, a, [0], window=16, hop=8)[0][1]), "the noise entered"


# ---- 3. no overlap, replacement only, is a batch of segments --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_no_overlap_is_inpaint_steps_over_the_segments_as_a_batch(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval", dropout=DROPOUT)
    T, W, N = 16, 3, 2
    shape = (N, 2, W * T, 32)
    x, y = MH.pair_data("winp.segments", shape)
    mask = torch.broadcast_to(_mask("soft", shape), shape).contiguous()
    seg = lambda v: torch.stack([v[n, :, j * T:(j + 1) * T] for n in range(N) for j in range(W)])  # noqa: E731  (sample 3 n + j)
    seq, a = _seq(10), MH.alphas(cfg)
    want_xs, want_x0 = D.inpaint_steps(seg(x).cuda(), seq, m, a, None, y=seg(y), mask=seg(mask), guidance=0.0, replace=True)
    xs, x0 = D.windowed_inpaint_steps(x.cuda(), seq, m, a, None, window=T, hop=T, y=y, mask=mask, guidance=0.0, replace=True)
    for got, want in ((xs[1:], want_xs[1:]), (x0, want_x0)):
        for i, (u, v) in enumerate(zip(got, want)):
            assert torch.equal(seg(u), v), i
    # guided, the norm belongs to the canvas sample and not to the segment: the two runs are different samplers
    gseg, _ = D.inpaint_steps(seg(x).cuda(), seq, m, a, [-1], y=seg(y), mask=seg(mask), guidance=0.3, replace=True)
    gxs, gx0 = D.windowed_inpaint_steps(x.cuda(), seq, m, a, [-1], window=T, hop=T, y=y, mask=mask, guidance=0.3, replace=True)
    assert bool(torch.isfinite(gxs[-1]).all()) and bool(torch.isfinite(gx0[-1]).all())
    assert not torch.equal(seg(gxs[-1]), gseg[-1]) and not torch.equal(gxs[-1], xs[-1])


# ---- 4. the kernels on their own operands ---------------------------------------------------------------------------------------------------
# (N, C, T, H, W, F): K = 1, 2, 3, 7, 8; one canvas sample of 655360 float4s, more than the 1024 x 256 threads of its grid
KERNEL_CASES = [(2, 2, 32, 32, 3, 32), (2, 2, 32, 16, 4, 32), (3, 2, 32, 12, 4, 12), (2, 1, 32, 5, 9, 8), (2, 2, 32, 4, 10, 4),
                (1, 1, 4096, 2048, 4, 256),
                (2, 1, 8, 2, 5, 4), (2, 1, 10, 2, 6, 4), (2, 1, 12, 2, 7, 4)]  # the last three: K = 4, 5, 6


def _row():
    """One coefficient row with every scalar set (eta = 0.5: c1 != 0), as fp32."""
    row = inpaint_coefficients([0, 300, 700], MH.alphas(), 0.5, 0.4)[1].astype(F32)
    assert (row[1:] != 0).all()
    return row


class _Case:
    """The tensors of one kernel case and its fp32 restatement (operation for operation step_math.h and the kernels' comments)."""

    def __init__(self, case, taper):
        N, C, T, H, W, F = case
        self.case, self.L = case, T + (W - 1) * H
        L = self.L
        self.geom = (N, W, C, L, T, H, F)
        self.shape, self.n, self.nwin = (N, C, L, F), N * C * L * F, N * W * C * T * F
        g = torch.Generator().manual_seed(1 + sum(case))
        self.eps, self.dwin = torch.randn((N * W, C, T, F), generator=g), torch.randn((N * W, C, T, F), generator=g)
        self.x, self.z, self.y = (torch.randn(self.shape, generator=g) for _ in range(3))
        m = torch.rand(self.shape, generator=g)
        pick = torch.rand(self.shape, generator=g)
        m = torch.where(pick < 0.3, torch.zeros(()), torch.where(pick < 0.6, torch.ones(()), torch.where(pick < 0.7, torch.full((), 0.5), m)))
        if N > 1:
            m[-1] = 0.0  # L_n = 0: no guidance term for this canvas sample
        self.m = m
        self.y = self.y * (m != 0)
        self.plan = p = window_plan(L, T, H, taper)
        assert p.W == W and p.K == -(-T // H)
        self.row = _row()
        self.coef, self.ctr = KH.Ro(np.stack([np.zeros(9, F32), self.row])), KH.Ro([1], torch.int32)
        self.epsd, self.dwd = KH.Ro(self.eps), KH.Ro(self.dwin)
        self.xd, self.zd, self.yd, self.md = KH.Ro(self.x), KH.Ro(self.z), KH.Ro(self.y), KH.Ro(self.m)
        self.jf, self.cn, self.wt = KH.Ro(p.jfirst, torch.int32), KH.Ro(p.cnt, torch.int32), KH.Ro(p.wt.copy())
        self.nparts = int(KH.lib().ddimxwi_partials_floats(N, C * L * F))
        assert self.nparts > 0 and self.nparts % N == 0

    def plan_ptrs(self):
        return self.jf.ptr, self.cn.ptr, self.wt.ptr

    def blend(self):
        out = KH.Out(self.n)
        _lib.check(KH.lib().ddimxw_blend(self.epsd.ptr, out.ptr, *self.plan_ptrs(), *self.geom, _lib.stream()))
        KH.sync()
        return out.read("ddimxw_blend").view(self.shape)

    def check_inputs(self, what):
        for r in (self.coef, self.ctr, self.epsd, self.dwd, self.xd, self.zd, self.yd, self.md, self.jf, self.cn, self.wt):
            r.check(what)

    # ---- the restatement, on numpy fp32 arrays
    def residual32(self, beps):
        """(x0, r, the seed batch) from the blended eps."""
        _, s1, s2, _, _, _, k1, _, _ = self.row
        N, C, T, H, W, F = self.case
        x, y, m = (v.numpy() for v in (self.x, self.y, self.m))
        x0 = SM.ddim_x0(x, beps, s1, s2)
        r = SM.inpaint_residual(x0, y, m)
        s = SM.inpaint_seed(r, m, k1)
        p = self.plan
        seed = np.empty((N, W, C, T, F), F32)
        for j in range(W):
            rows = np.arange(j * H, j * H + T)
            k = j - p.jfirst[rows]
            assert (k >= 0).all() and (k < p.cnt[rows]).all()
            wk = p.wt[k, rows][None, None, :, None]
            one = (p.cnt[rows] == 1)[None, None, :, None]
            seed[:, j] = np.where(one, s[:, :, rows], (wk * s[:, :, rows]).astype(F32))
        return x0, r, seed.reshape(N * W, C, T, F)

    def overlap_add32(self):
        """((d[j0] + d[j1]) + d[j2]) ... per canvas row, every sum rounded to fp32."""
        N, C, T, H, W, F = self.case
        d = self.dwin.numpy().reshape(N, W, C, T, F)
        p = self.plan
        out = np.empty(self.shape, F32)
        for l in range(self.L):
            j0 = int(p.jfirst[l])
            acc = d[:, j0, :, l - j0 * H]
            for k in range(1, int(p.cnt[l])):
                acc = (acc + d[:, j0 + k, :, l - (j0 + k) * H]).astype(F32)
            out[:, :, l] = acc
        return out

    def update32(self, e, x0, gsum, w, flags, noise):
        """x after ddimxwi_update: e the blended eps, x0 the prediction, gsum the overlap-added d_win, w [N] the guidance factor."""
        _, s1, s2, s3, c2, c1, _, k2, _ = self.row
        y, m, z = self.y.numpy(), self.m.numpy(), self.z.numpy()
        u = SM.ddim_next(x0, e, s3, c2)
        if noise:
            u = SM.fma32(z, c1, u)
        if flags & 2:
            wn = w.astype(F32)[:, None, None, None]
            u = np.where(wn != 0, SM.inpaint_guide(u, x0, y, m, gsum, k2, wn), u)
        if flags & 1:
            kv = SM.ddim_next(y, e, s3, c2)
            if noise:
                kv = SM.fma32(z, c1, kv)
            u = SM.inpaint_replace(u, kv, m)
        return u


def _norm32(partials):
    """The canvas sample's norm as ddimxwi_update adds its partials [nb]: thread i adds partials i, i + 256, ... in order, then
    block_sum -- the xor butterfly over each wave of 64, then ((w0 + w1) + w2) + w3 -- all in fp32."""
    v = np.zeros(256, F32)
    for p0 in range(0, len(partials), 256):
        chunk = partials[p0:p0 + 256]
        v[:len(chunk)] = (v[:len(chunk)] + chunk).astype(F32)
    v = v.reshape(4, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lanes ^ o]).astype(F32)
    return F32(F32(F32(v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0])


@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=str)
def test_residual_kernel_matches_the_fp32_restatement(case, taper):
    """x0, the blended eps and every seed bit for bit; no seed element keeps the sentinel (each is written exactly once, nothing is
    zeroed first: the guards and the body start as 0xFF bytes); the partials add up to the sum of r^2 inside the bound of their own
    additions: a thread's chain of fused multiply-adds over its 4 ceil(n4 / threads) elements, the 6 + 3 additions of block_sum, each
    at most 2^-24 relative on non-negative terms -- gamma_n = n u / (1 - n u) of the exact sum."""
    N, C, T, H, W, F = case
    c = _Case(case, taper)
    beps = c.blend()
    x0, be, seed, parts = KH.Out(c.n), KH.Out(c.n), KH.Out(c.nwin), KH.Out(c.nparts)
    _lib.check(KH.lib().ddimxwi_residual(c.xd.ptr, c.epsd.ptr, c.yd.ptr, c.md.ptr, x0.ptr, be.ptr, seed.ptr, parts.ptr, *c.plan_ptrs(),
                                         c.coef.ptr, c.ctr.ptr, *c.geom, _lib.stream()))
    KH.sync()
    c.check_inputs("ddimxwi_residual")
    want_x0, r, want_seed = c.residual32(beps.numpy())
    KH.same(be.read("beps").view(c.shape), beps, "the blended eps is ddimxw_blend's")
    KH.same(x0.read("x0").view(c.shape), want_x0, "x0")
    got_seed = seed.read("seed")
    assert not bool((got_seed.view(torch.int32) == -1).any()), "a seed element was never written"
    KH.same(got_seed.view(N * W, C, T, F), want_seed, "seed")
    got = parts.read("partials").double().view(N, -1).sum(1).numpy()
    exact = (r.astype(np.float64) ** 2).reshape(N, -1).sum(1)
    nb = c.nparts // N
    n4 = C * c.L * F // 4
    terms = 4 * -(-n4 // (nb * 256)) + 9
    bound = terms * U / (1 - terms * U) * exact
    print(f"[ddimxwi_residual {case} {taper}] partials: {nb} per sample, worst error / bound "
          f"{float(np.max(np.abs(got - exact) / np.maximum(bound, 1e-300))):.3f}")
    assert (np.abs(got - exact) <= bound).all(), (got, exact, bound)
    if N > 1:
        assert exact[-1] == 0.0 and got[-1] == 0.0 and exact[0] > 0


@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=str)
def test_update_kernel_matches_the_fp32_restatement(case, taper):
    """All four flag combinations, with and without noise, bit for bit given the norm the restatement forms from the partials in
    the kernel's order (one ulp of slack for the device's double sqrt in zeta / sqrt(L_n), the same for every element of a canvas
    sample, as in test_gpu_inpaint.py); a canvas sample whose norm is 0 takes no guidance term; not guided, the call equals
    ddimxw_blend followed by ddimx_inpaint_update."""
    N, C, T, H, W, F = case
    lib, st = KH.lib(), _lib.stream()
    c = _Case(case, taper)
    per = C * c.L * F
    beps = c.blend()
    x0_32, r, _ = c.residual32(beps.numpy())
    gsum = c.overlap_add32()
    # the residual kernel's own outputs feed the guided calls
    x0r, ber, seed, parts = KH.Out(c.n), KH.Out(c.n), KH.Out(c.nwin), KH.Out(c.nparts)
    _lib.check(lib.ddimxwi_residual(c.xd.ptr, c.epsd.ptr, c.yd.ptr, c.md.ptr, x0r.ptr, ber.ptr, seed.ptr, parts.ptr, *c.plan_ptrs(),
                                    c.coef.ptr, c.ctr.ptr, *c.geom, st))
    KH.sync()
    pd, bd = KH.Ro(parts.read("partials")), KH.Ro(beps)
    Ln = np.array([_norm32(v) for v in pd.t.cpu().numpy().reshape(N, -1)], F32)
    zeta = float(c.row[8])
    w_rn = np.where(Ln > 0, zeta / np.sqrt(np.maximum(Ln.astype(np.float64), 1e-300)), 0.0).astype(F32)  # in double, rounded once
    assert w_rn[0] != 0 and (N == 1 or w_rn[-1] == 0)
    for flags in (0, 1, 2, 3):
        for noise in (False, True):
            what = f"flags {flags}, noise {noise}"
            xt = KH.Out(c.n, init=c.x)
            x0 = KH.Out(c.n, init=x0_32) if flags & 2 else KH.Out(c.n)
            _lib.check(lib.ddimxwi_update(xt.ptr, bd.ptr if flags & 2 else c.epsd.ptr, c.zd.ptr if noise else None, x0.ptr, c.yd.ptr, c.md.ptr,
                                          c.dwd.ptr, pd.ptr, *c.plan_ptrs(), c.coef.ptr, c.ctr.ptr, *c.geom, flags, st))
            KH.sync()
            KH.same(x0.read("x0, " + what).view(c.shape), x0_32, "x0, " + what)
            got = xt.read("x, " + what).view(c.shape)
            assert bool(torch.isfinite(got).all()), what
            if not flags & 2:
                KH.same(got, c.update32(beps.numpy(), x0_32, gsum, w_rn, flags, noise), "x, " + what)
                # the same call in two: ddimxw_blend's canvas eps, then ddimx_inpaint_update on it
                o, o0 = KH.Out(c.n, init=c.x), KH.Out(c.n)
                _lib.check(lib.ddimx_inpaint_update(o.ptr, bd.ptr, c.zd.ptr if noise else None, o0.ptr, c.yd.ptr, c.md.ptr, None, None,
                                                    c.coef.ptr, c.ctr.ptr, N, per, flags, st))
                KH.sync()
                KH.same(got, o.read(what).view(c.shape), "blend + ddimx_inpaint_update, x, " + what)
                KH.same(x0.read(what), o0.read(what), "blend + ddimx_inpaint_update, x0, " + what)
                continue
            got = got.numpy().view(np.int32)
            cands = [np.nextafter(w_rn, F32(-np.inf)), w_rn, np.nextafter(w_rn, F32(np.inf))]
            wants = [c.update32(beps.numpy(), x0_32, gsum, np.where(w_rn != 0, w, w_rn).astype(F32), flags, noise).view(np.int32) for w in cands]
            for n in range(N):
                ok = [np.array_equal(got[n], w[n]) for w in wants]
                bad = got[n] != wants[1][n]
                assert any(ok), f"{what}, canvas sample {n}: {int(bad.sum())} of {bad.size} elements differ"
            if N > 1:  # the canvas sample without a norm: no guidance term at all
                assert np.array_equal(got[-1], c.update32(beps.numpy(), x0_32, gsum, w_rn, flags & 1, noise).view(np.int32)[-1])
            assert not np.array_equal(got[0], c.update32(beps.numpy(), x0_32, gsum, w_rn, flags & 1, noise).view(np.int32)[0]), "the term is there"
    for r_ in (pd, bd):
        r_.check("ddimxwi_update")
    c.check_inputs("ddimxwi_update")


def test_kernels_refuse_bad_arguments_and_write_nothing():
    lib, st = KH.lib(), _lib.stream()
    c = _Case((2, 2, 32, 16, 3, 8), "tri")
    xt, x0, be, seed, parts = KH.Out(c.n), KH.Out(c.n), KH.Out(c.n), KH.Out(c.nwin), KH.Out(c.nparts)
    good = dict(x=xt.ptr, eps=c.epsd.ptr, noise=c.zd.ptr, x0=x0.ptr, y=c.yd.ptr, mask=c.md.ptr, beps=be.ptr, seed=seed.ptr, dwin=c.dwd.ptr,
                parts=parts.ptr, jf=c.jf.ptr, cn=c.cn.ptr, wt=c.wt.ptr, coef=c.coef.ptr, step=c.ctr.ptr, N=2, W=3, C=2, L=64, T=32, H=16, F=8,
                flags=3)
    shapes = [dict(N=0), dict(W=0), dict(N=30000), dict(C=0), dict(L=65), dict(H=0), dict(L=66, H=33), dict(F=6), dict(F=0), dict(T=0),
              dict(L=32 + 2 * 3, H=3), dict(wt=None)]
    nulls = [dict(x=None), dict(eps=None), dict(x0=None), dict(jf=None), dict(cn=None), dict(coef=None), dict(step=None)]
    for edit in nulls + [dict(y=None), dict(mask=None), dict(beps=None), dict(seed=None), dict(parts=None)] + shapes:
        a = dict(good, **edit)
        rc = lib.ddimxwi_residual(a["x"], a["eps"], a["y"], a["mask"], a["x0"], a["beps"], a["seed"], a["parts"], a["jf"], a["cn"], a["wt"],
                                  a["coef"], a["step"], a["N"], a["W"], a["C"], a["L"], a["T"], a["H"], a["F"], st)
        KH.refused(rc, xt, x0, be, seed, parts, who="ddimxwi_residual")
    for edit in nulls + [dict(y=None), dict(mask=None, flags=1), dict(dwin=None), dict(parts=None, flags=2), dict(flags=4), dict(flags=-1)] + shapes:
        a = dict(good, **edit)
        rc = lib.ddimxwi_update(a["x"], a["eps"], a["noise"], a["x0"], a["y"], a["mask"], a["dwin"], a["parts"], a["jf"], a["cn"], a["wt"],
                                a["coef"], a["step"], a["N"], a["W"], a["C"], a["L"], a["T"], a["H"], a["F"], a["flags"], st)
        KH.refused(rc, xt, x0, who="ddimxwi_update")
    assert lib.ddimxwi_partials_floats(2, 2 * 64 * 8 + 2) == -1 and lib.ddimx_abi_version() == 2
    c.check_inputs("refusals")


# ---- 5. the sampler against the oracle ------------------------------------------------------------------------------------------------------
# name, canvas shape, window, hop
ORACLE_CASES = {"tiny": ("tiny", (2, 2, 48, 32), 16, 8), "audio": ("audio", (1, 2, 64, 256), 32, 16), "ragged": ("tiny", (3, 2, 40, 32), 16, 12)}
ORACLE_SEQ = [0, 250, 500, 750]  # 4 steps: the replayed path


@functools.lru_cache(maxsize=None)
def _reference(case, kind, prediction="eps"):
    """The fp32 restatement over the oracle's fp32 forward, once for both activation dtypes of the GPU model.  ``kind``: "guided"
    (the soft mask, zeta per iteration) or the mask of a replacement-only run."""
    name, shape, T, H = ORACLE_CASES[case]
    cfg, m = MH.build(name, MODES[0][0], 5, mode="eval", dropout=DROPOUT, kind="v" if prediction == "v" else None)
    x, y = MH.pair_data("winp.oracle." + case, shape)
    mask = _mask("soft" if kind == "guided" else kind, shape)
    zeta = ZETA4 if kind == "guided" else 0.0
    rxs, rx0 = WI.windowed_inpaint_steps(x, ORACLE_SEQ, MH.oracle_eps(m, name), MH.alphas(cfg), T, H, "tri", y, mask, zeta, True,
                                         prediction=prediction)
    return x, y, mask, zeta, rxs, rx0


@pytest.mark.parametrize("kind", ["guided", "gap", "band"])
@pytest.mark.parametrize("case", list(ORACLE_CASES))
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_sampler_vs_reference(mode, case, kind):
    dtype_str, dt = mode
    name, shape, T, H = ORACLE_CASES[case]
    cfg, m = MH.build(name, dtype_str, 5, mode="eval", dropout=DROPOUT)
    x, y, mask, zeta, rxs, rx0 = _reference(case, kind)
    xs, x0 = D.windowed_inpaint_steps(x.cuda(), ORACLE_SEQ, m, MH.alphas(cfg), None, window=T, hop=H, taper="tri", y=y,
                                      mask=mask if kind == "guided" else mask.bool(), guidance=zeta, replace=True)
    for i in range(len(ORACLE_SEQ)):
        mx, er = MH.gate(xs[i + 1], rxs[i + 1], dt, f"xs[{i + 1}] {case} {kind}")
        MH.gate(x0[i], rx0[i], dt, f"x0[{i}] {case} {kind}")
    print(f"[windowed inpaint {kind} {case} {MODE_IDS[dt]}] final max {mx:.3e} rms err {er:.3e} x rms")
    assert ORACLE_SEQ[0] == 0
    MH.known_exact(xs[-1], y, mask)
    if kind == "guided":
        free = D.windowed_inpaint_steps(x.cuda(), ORACLE_SEQ, m, MH.alphas(cfg), [0], window=T, hop=H, y=y, mask=mask, guidance=0.0)
        assert not torch.equal(free[0][1], xs[1]), "the guidance acted"


# ---- 6. replayed = eager, canvas-batch invariance, the v model ------------------------------------------------------------------------------
KW = dict(window=16, hop=8, taper="tri")


def _canvas(tag, n=3):
    shape = (n, 2, 48, 32)
    x, y = MH.pair_data("winp." + tag, shape)
    return x, y, _mask("soft", shape)


@pytest.mark.parametrize("leg", ["guided", "replace_only", "guided_eta"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_replayed_equals_eager(mode, leg):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval", dropout=DROPOUT)
    x, y, mask = _canvas("replay", 2)
    seq, a = _seq(5), MH.alphas(cfg)
    kw = dict(KW, y=y, mask=mask, guidance=0.0 if leg == "replace_only" else _zeta(5), replace=True)
    if leg == "guided_eta":
        kw.update(eta=0.5, noise=NoiseStream(0xFEED, 5))
    g_xs, g_x0 = D.windowed_inpaint_steps(x.cuda(), seq, m, a, None, **kw)
    with MH.eager_steps():
        e_xs, e_x0 = D.windowed_inpaint_steps(x.cuda(), seq, m, a, None, **kw)
    MH.same_list(g_xs[1:], e_xs[1:], "xs")
    MH.same_list(g_x0, e_x0, "x0_preds")


@pytest.mark.parametrize("guided", [True, False], ids=["guided", "replace_only"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_canvas_does_not_depend_on_its_batch(mode, guided):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval", dropout=DROPOUT)
    x, y, mask = _canvas("batch")
    mask[-1, :, :6] = 1.0  # (the soft mask empties the last sample's start; every sample keeps a norm)
    seq, a = _seq(4), MH.alphas(cfg)
    kw = dict(KW, guidance=ZETA4 if guided else 0.0, replace=True, eta=0.5)
    xs, x0 = D.windowed_inpaint_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, noise=NoiseStream(99), **kw)
    for n in range(3):
        sxs, sx0 = D.windowed_inpaint_steps(x[n:n + 1].cuda(), seq, m, a, None, y=y[n:n + 1], mask=mask[n:n + 1],
                                            noise=NoiseStream(99, first_sample=n), **kw)
        for i in range(len(seq)):
            assert torch.equal(xs[i + 1][n:n + 1], sxs[i + 1]) and torch.equal(x0[i][n:n + 1], sx0[i]), (n, i)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_v_model_equals_the_wrapped_eps_callable(mode):
    """Replacement only: every window's v is converted with the window's own input before the blend, so the run equals the one over
    a callable that converts its own output.  (A guided run takes no plain callable: the guided v model is held to the oracle in
    test_guided_v_model_vs_reference.)"""
    cfg, mv, ms, a = MH.pair("tiny", mode[0])
    x, y, mask = _canvas("v")
    seq = _seq(5)
    kw = dict(KW, y=y, mask=mask, guidance=0.0, replace=True)
    got = D.windowed_inpaint_steps(x.cuda(), seq, mv, a, None, **kw)
    with MH.eager_steps():  # the callable allocates
        want = D.windowed_inpaint_steps(x.cuda(), seq, MH.v_wrapped(ms, v_table(a)), a, None, prediction="eps", **kw)
    MH.same_list(got[0][1:], want[0][1:], "xs")
    MH.same_list(got[1], want[1], "x0_preds")
    twin = D.windowed_inpaint_steps(x.cuda(), seq, ms, a, [-1], **kw)
    assert not torch.equal(twin[0][-1], got[0][-1]), "the twin reads the output as eps"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_guided_v_model_vs_reference(mode):
    """A guided run on a v model -- k1 = -2 s1, k2 = 2 s2 and the per-window conversion in front of the residual -- against the
    restatement, whose autograd runs through the conversion and the blend, over the oracle's v; and guided, a v model given
    ``prediction="v"`` explicitly is the same run."""
    dtype_str, dt = mode
    name, shape, T, H = ORACLE_CASES["tiny"]
    cfg, mv, _, a = MH.pair("tiny", dtype_str)
    live, ocfg = MH.oracle(mv, "tiny")
    sd = {k: v.detach() for k, v in live.items()}
    x, y = MH.pair_data("winp.v.guided", shape)
    mask = _mask("soft", shape)
    kw = dict(window=T, hop=H, y=y, mask=mask, guidance=ZETA4, replace=True)
    xs, x0 = D.windowed_inpaint_steps(x.cuda(), ORACLE_SEQ, mv, a, None, **kw)
    rxs, rx0 = WI.windowed_inpaint_steps(x, ORACLE_SEQ, lambda w, t, j: ref_cpu.model_forward(sd, ocfg, w, t), a, T, H, "tri", y, mask, ZETA4, True,
                                         prediction="v")
    for i in range(len(ORACLE_SEQ)):
        MH.gate(xs[i + 1], rxs[i + 1], dt, f"xs[{i + 1}]")
        MH.gate(x0[i], rx0[i], dt, f"x0[{i}]")
    again = D.windowed_inpaint_steps(x.cuda(), ORACLE_SEQ, mv, a, None, prediction="v", **kw)
    MH.same_list(again[0][1:], xs[1:], "prediction='v' given")
    as_eps = D.windowed_inpaint_steps(x.cuda(), ORACLE_SEQ, mv, a, [-1], prediction="eps", **kw)
    assert not torch.equal(as_eps[0][-1], xs[-1])


# ---- 7. no side effects -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_no_side_effects(mode, train):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval", dropout=DROPOUT)
    assert all(p.requires_grad for p in m.parameters())
    shape = (2, 2, 48, 32)
    x, y = MH.pair_data("winp.side", shape)
    mask = _mask("gap", shape)
    seq, a = [0, 300, 600, 900], MH.alphas(cfg)
    kw = dict(KW, y=y, mask=mask, guidance=0.3)
    before = D.windowed_steps(x.cuda(), seq, m, a, None, **KW)
    ref_xs, _ = D.windowed_inpaint_steps(x.cuda(), seq, m, a, None, **kw)
    m._dropout_calls = 17
    m.train(train)
    xs, _ = D.windowed_inpaint_steps(x.cuda(), seq, m, a, None, **kw)
    assert m._dropout_calls == 17
    assert all(p.grad is None for p in m.parameters())
    assert getattr(m, "_flat_grad", None) is None
    for i in range(1, len(seq) + 1):
        assert torch.equal(xs[i], ref_xs[i]), f"train={train}: xs[{i}] differs from the eval-mode run"
    m.eval()
    after = D.windowed_steps(x.cuda(), seq, m, a, None, **KW)
    for u, v in zip(before[0][1:] + before[1], after[0][1:] + after[1]):
        assert torch.equal(u, v)


# ---- 8. ownership -----------------------------------------------------------------------------------------------------------------------------
def _run(m, x, y, mask, coef, n_steps, use_graph, disturb=None):
    """``MH.stepper_run`` of a guided, replacing WindowInpaintStepper on a clone of x; the fourth result: the buffers it owned."""
    return MH.stepper_run(lambda: WindowInpaintStepper(m, x.clone(), y, mask, coef, True, True, 16, 8, "tri", use_graph=use_graph), n_steps,
                          disturb, keep=lambda st: dict(win=st.win, seed=st.seed, d_x=st.d_x, beps=st.beps, partials=st.partials,
                                                        tape=st.tape, ws=st.ws, x0=st.x0))


def test_stepper_owns_what_its_graph_references_and_sees_load_state_dict():
    """One capture; the buffers of a guided step are this object's, window-batch-shaped where the network reads or writes them and
    canvas-shaped elsewhere; new weights under the live graph are used by the next replay; a re-allocated backward packing makes
    the graph stale and the step re-captures (test_gpu_inpaint.py's, on the canvas)."""
    cfg, m = MH.build("tiny", MODES[1][0], 3, mode="eval", dropout=DROPOUT)
    other = synth.fill_module(D.Model(cfg), 11).eval().state_dict()
    first = {k: v.clone() for k, v in m.state_dict().items()}
    a = MH.alphas(cfg)
    coef = inpaint_coefficients(_seq(10), a, 0.0, 0.3)
    x, y, mask = (v.cuda() for v in _canvas("own", 2))
    mask = torch.broadcast_to(mask, x.shape).contiguous()

    def disturb(i):
        if i == 4:
            m.load_state_dict(other)

    outs = []
    for graph in (False, True):
        m.load_state_dict(first)
        o, captures, has, own = _run(m, x, y, mask, coef, 10, graph, disturb)
        assert (captures, has) == ((1, True) if graph else (0, False))
        outs.append(o[-1])
        assert own["win"].shape == own["seed"].shape == own["d_x"].shape == (10, 2, 16, 32)
        assert own["beps"].shape == own["x0"].shape == x.shape and own["partials"].numel() % 2 == 0
        assert own["tape"].numel() == _lib.load().ddimx_train_tape_bytes(m._handle, 10, 16)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    m.load_state_dict(first)
    plain, _, _, _ = _run(m, x, y, mask, coef, 10, False)
    assert not torch.equal(plain[-1][0], outs[0][0]), "the new weights really changed the trajectory"
    with torch.no_grad():
        st = WindowInpaintStepper(m, x.clone(), y, mask, coef, True, True, 16, 8, "tri")
        try:
            for _ in range(5):
                st.step()
            assert st.captures == 1 and st.graph is not None
            refs = {r.data_ptr() for r in st._refs}
            assert m._packed_bwd.data_ptr() in refs and m._packed.data_ptr() in refs, "captured_refs(backward=True)"
            st.rewind()
            m.invalidate()  # new packed values in place: the graph stays
            st.step()
            assert st.captures == 1
            m._packed_bwd = None  # a re-allocated backward packing does not bump Model._gen: still stale
            st.step()
            assert st.captures == 2
        finally:
            st.close()
