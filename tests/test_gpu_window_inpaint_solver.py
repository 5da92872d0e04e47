"""Windowed multistep inpainting on the GPU (ddim_audio_amd.windowed_inpaint_solver_steps, ddimxwis_residual /
ddimxwis_multistep_update of include/ddimx_window_inpaint_solver.h).

The two exports on their own operands through the C ABI, in guarded buffers: the residual against ddimxwi_residual on the narrow
row; the update against ddimxw_blend followed by ddimxi_multistep_update on [N, C L F] (guided: with d_x the fp32 overlap-add of
d_win, written in numpy) and against the fp32 restatement of the documented operation order (inpaint_solver_ref.update32) with
every unread buffer poisoned; the final row; refusals.  The sampler, bit for bit where the definition reduces to one that existed:
one window = inpaint_solver_steps, an empty mask with rho = 0 = windowed_solver_steps, no overlap without guidance =
inpaint_solver_steps over the segments as a batch; order 1 against windowed_inpaint_steps; the trajectory against the fp64
restatement (tests/window_inpaint_solver_ref.py) over the CPU oracle at model_harness's gate; the stepper; canvas-batch invariance;
a v model; and the convergence study with the update running in the kernel in fp32."""
import functools

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, synth
from ddim_audio_amd.noise import NoiseStream
from ddim_audio_amd.schedule import guidance_per_step, inpaint_solver_coefficients, logsnr_seq, v_table, window_plan
from ddim_audio_amd.window_inpaint_solver import WindowInpaintSolverStepper
from oracle import ref_cpu
import gpu_util as G
import kernel_harness as KH
import model_harness as MH
from model_harness import MODES, MODE_IDS
import inpaint_solver_ref as R
import window_inpaint_solver_ref as WIS
import window_solver_ref as WS

pytestmark = pytest.mark.gpu
SEED, FIRST, DRAW_BASE = 0x0123456789ABCDEF, 100, 5
TAPERS = ["flat", "tri"]
F32 = np.float32
RHO5 = [0.3, 0.2, 0.0, 0.25, 0.3]


# ---- 1. the exports on their own operands -------------------------------------------------------------------------------------------
# test_gpu_window_inpaint.py's cases, (N, C, T, H, W, F): K = 1, 2, 3, 7, 8; one canvas sample of 655360 float4s, more than the
# 1024 x 256 threads of its grid; K = 4, 5, 6
KERNEL_CASES = [(2, 2, 32, 32, 3, 32), (2, 2, 32, 16, 4, 32), (3, 2, 32, 12, 4, 12), (2, 1, 32, 5, 9, 8), (2, 2, 32, 4, 10, 4),
                (1, 1, 4096, 2048, 4, 256),
                (2, 1, 8, 2, 5, 4), (2, 1, 10, 2, 6, 4), (2, 1, 12, 2, 7, 4)]
BIG = KERNEL_CASES[5]


def _rows():
    """test_gpu_inpaint_solver.py's ten fp32 rows.  Row k < 8: a third-order row of a real table at tau = 1, guided, with w1 / w2 /
    c1 zeroed unless bit 0 / 1 / 2 of k is set; row 8: the table's final row; row 9: row 7 with rho = 0."""
    a = MH.alphas()
    tab = inpaint_solver_coefficients(logsnr_seq(a, 20), a, 3, 1.0, 0.4).astype(F32)
    row = tab[5]
    assert (row[[5, 8, 9, 10, 11, 12]] != 0).all()
    rows = np.tile(row, (10, 1))
    for k in range(8):
        for bit, col in enumerate((11, 12, 5)):
            if not k >> bit & 1:
                rows[k, col] = 0.0
    rows[8] = tab[-1]
    assert rows[8, 4] == 0 and rows[8, 5] == 0 and rows[8, 3] == 1 and rows[8, 9] == 0 and rows[8, 10] == 1 and rows[8, 8] != 0
    rows[9, 8] = 0.0
    return rows


def _nan(*shape):
    return torch.full(shape, KH.NAN)


class _Case:
    """The tensors of one kernel case: the window batch's eps and d_win, canvas-shaped x, z, y, m0, m1, m2 and a mask with 0, 1, 0.5
    and other fractions; L [N] -- the last canvas sample of a batch has L = 0 -- and partials [N, nb] that add up to it exactly in
    any order (units of 0.25 spread over the blocks)."""

    def __init__(self, case, taper):
        N, C, T, H, W, F = case
        self.case, self.L = case, T + (W - 1) * H
        self.geom = (N, W, C, self.L, T, H, F)
        self.shape, self.per = (N, C, self.L, F), C * self.L * F
        self.n, self.nwin = N * self.per, N * W * C * T * F
        g = torch.Generator().manual_seed(7 + sum(case))
        self.eps, self.dwin = (torch.randn((N * W, C, T, F), generator=g) for _ in range(2))
        self.v = {s: torch.randn(self.shape, generator=g).numpy() for s in ("x", "z", "y", "m0", "m1", "m2")}
        pick, frac = torch.rand(self.shape, generator=g), torch.rand(self.shape, generator=g)
        m = torch.where(pick < 0.3, torch.zeros(()), torch.where(pick < 0.6, torch.ones(()), torch.where(pick < 0.7, torch.full((), 0.5), frac)))
        self.v["m"] = m.numpy()
        self.v["y"] = (self.v["y"] * (self.v["m"] != 0)).astype(F32)
        self.plan = p = window_plan(self.L, T, H, taper)
        assert p.W == W and p.K == -(-T // H)
        self.rows = _rows()
        self.coef = KH.Ro(self.rows)
        self.epsd = KH.Ro(self.eps)
        self.jf, self.cn, self.wt = KH.Ro(p.jfirst, torch.int32), KH.Ro(p.cnt, torch.int32), KH.Ro(p.wt.copy())
        nparts = int(KH.lib().ddimxwi_partials_floats(N, self.per))
        assert nparts > 0 and nparts % N == 0 and nparts == int(KH.lib().ddimx_inpaint_partials_floats(N, self.per))
        self.nb = nparts // N
        self.Ln = np.array({1: [7.0], 2: [7.0, 0.0], 3: [7.0, 2.25, 0.0]}[N], dtype=F32)
        self.parts = np.zeros((N, self.nb), dtype=F32)
        for s in range(N):
            for j in range(int(self.Ln[s] * 4)):
                self.parts[s, (j * 5) % self.nb] += 0.25
        assert np.array_equal(self.parts.astype(np.float64).sum(1), self.Ln.astype(np.float64))
        out = KH.Out(self.n)
        _lib.check(KH.lib().ddimxw_blend(self.epsd.ptr, out.ptr, *self.plan_ptrs(), *self.geom, _lib.stream()))
        KH.sync()
        self.beps = out.read("ddimxw_blend").view(self.shape).numpy()
        self.gsum = self.overlap_add32()

    def plan_ptrs(self):
        return self.jf.ptr, self.cn.ptr, self.wt.ptr

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

    def flat(self, s):
        return self.v[s].reshape(self.shape[0], self.per)

    def call(self, k, flags, h2_given, noise_given, x_init=None):
        """One ddimxwis_multistep_update on row k with whatever the row and the flags leave unread poisoned (NaN in every word, an
        output's sentinel bytes are NaNs too); the same step in two launches on [N, C L F] -- ddimxw_blend's canvas eps (guided: the
        overlap-added d_win) into ddimxi_multistep_update -- and update32's results.  Returns (outs, pair, want)."""
        N, W = self.geom[0], self.geom[1]
        lib, st = KH.lib(), _lib.stream()
        row = self.rows[k]
        guided, replace = bool(flags & 2), bool(flags & 1)
        use1, use2, add_z = row[11] != 0, bool(row[12] != 0 and h2_given), row[5] != 0
        load1 = use1 or use2
        x = self.v["x"] if x_init is None else x_init
        ctr = KH.Ro([k], torch.int32)
        noise = KH.Ro(self.v["z"] if add_z else _nan(*self.shape)) if noise_given else None
        y, m = (KH.Ro(self.v[s] if flags else _nan(*self.shape)) for s in ("y", "m"))
        dead = torch.as_tensor(self.Ln == 0) | (not guided) | bool(row[8] == 0)  # per canvas sample: d_win is read only where wq != 0
        dwin = self.dwin.clone().view(N, W, -1)
        dwin[dead] = KH.NAN
        dsum = torch.as_tensor(self.gsum).clone()
        dsum[dead] = KH.NAN
        dwin, dsum = KH.Ro(dwin), KH.Ro(dsum)
        part = KH.Ro(self.parts if guided else _nan(*self.parts.shape))
        eps = KH.Ro(self.beps) if guided else self.epsd  # guided: the canvas-shaped beps of the residual pass
        beps = KH.Ro(self.beps)
        both = []
        for canvas in (True, False):
            xt = KH.Out(self.n, init=x if (replace or not guided) else None)
            x0 = KH.Out(self.n, init=self.v["m0"] if guided else None)
            h1 = KH.Out(self.n, init=self.v["m1"] if load1 else None)
            h2 = KH.Out(self.n, init=self.v["m2"] if use2 else None) if h2_given else None
            head = (xt.ptr, (eps if canvas else beps).ptr, None if noise is None else noise.ptr, x0.ptr, h1.ptr, None if h2 is None else h2.ptr,
                    y.ptr, m.ptr)
            if canvas:
                rc = KH.lib().ddimxwis_multistep_update(*head, dwin.ptr, part.ptr, *self.plan_ptrs(), self.coef.ptr, ctr.ptr, *self.geom, flags,
                                                        SEED, FIRST, DRAW_BASE, st)
            else:
                rc = lib.ddimxi_multistep_update(*head, dsum.ptr, part.ptr, self.coef.ptr, ctr.ptr, N, self.per, flags, SEED, FIRST, DRAW_BASE, st)
            _lib.check(rc)
            KH.sync()
            both.append((xt, x0, h1, h2))
        what = f"row {k} flags {flags}"
        for r in (self.coef, self.epsd, self.jf, self.cn, self.wt, ctr, y, m, dwin, dsum, part, eps, beps) + (() if noise is None else (noise,)):
            r.check(what)
        z = self.flat("z")
        if add_z and not noise_given:  # what ddimx_noise_fill writes for this draw: the group of four counts within the canvas sample
            z = D.NoiseStream(SEED, FIRST).step_noise((N, self.per), DRAW_BASE + k, G.dev()).cpu().numpy()
        want = R.update32(row, flags, x.reshape(N, self.per), self.beps.reshape(N, self.per), z, self.flat("m0"), self.flat("m1"), self.flat("m2"),
                          self.flat("y"), self.flat("m"), self.gsum.reshape(N, self.per), self.Ln, h2_given)
        return both[0], both[1], want

    def compare(self, outs, pair, want, what):
        N = self.geom[0]
        got = [None if o is None else o.read(what) for o in outs]
        assert bool(torch.isfinite(got[0]).all()), f"{what}: a poisoned buffer reached x"
        for g, o, name in zip(got, pair, ("x", "x0", "h1", "h2")):
            if g is not None:
                KH.same(g, o.read(what), f"{name}: blend + ddimxi_multistep_update, {what}")
        if want is None:
            return got[0]
        KH.same(got[0].view(N, self.per), want[0], f"x, {what}")
        KH.same(got[1].view(N, self.per), self.flat("m0") if want[1] is None else want[1], f"x0, {what}")
        KH.same(got[2].view(N, self.per), want[2], f"h1 <- the guided prediction, {what}")
        if outs[3] is not None:
            if want[3] is None:
                assert outs[3].untouched(), f"h2 was written though h1 was not read, {what}"
            else:
                KH.same(got[3].view(N, self.per), want[3], f"h2 <- the old h1, {what}")
        return got[0]


@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=str)
def test_residual_on_the_wide_row_is_ddimxwi_residual(case, taper):
    """The same kernel on a 13-float row gives the 9-float row's bits in x0, beps, every seed and every partial."""
    c = _Case(case, taper)
    ins = [KH.Ro(c.v[s]) for s in ("x",)] + [c.epsd] + [KH.Ro(c.v[s]) for s in ("y", "m")]
    ctr = KH.Ro([3], torch.int32)
    res = []
    for fn, tab in ((KH.lib().ddimxwis_residual, c.rows), (KH.lib().ddimxwi_residual, c.rows[:, :9].copy())):
        coef = KH.Ro(tab)
        outs = [KH.Out(c.n), KH.Out(c.n), KH.Out(c.nwin), KH.Out(c.nb * case[0])]
        _lib.check(fn(*(i.ptr for i in ins), *(o.ptr for o in outs), *c.plan_ptrs(), coef.ptr, ctr.ptr, *c.geom, _lib.stream()))
        KH.sync()
        res.append([o.read("residual") for o in outs])
        for r in ins + [coef, ctr]:
            r.check("residual")
    for g, w, what in zip(res[0], res[1], ("x0", "beps", "seed", "partials")):
        KH.same(g, w, what)
    KH.same(res[0][1].view(c.shape), c.beps, "beps is ddimxw_blend's")
    assert not bool((res[0][2].view(torch.int32) == -1).any()), "a seed element was never written"


@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("case", [c for c in KERNEL_CASES if c != BIG], ids=str)
def test_update_is_blend_then_the_multistep_update_and_the_fp32_restatement(case, taper):
    """All four flag combinations (guided: d_x the numpy overlap-add), every zero / non-zero (w1, w2, c1), h2 null and given, z
    handed and drawn: x, x0, h1 and h2 bit for bit the two-launch form's and update32's; what a row leaves unread is poisoned."""
    c = _Case(case, taper)
    seen = {}
    for flags in range(4):
        for k in range(8):
            for h2_given in (False, True):
                for noise_given in (True, False):
                    what = f"flags {flags}, row {k}, h2 {h2_given}, noise {'given' if noise_given else 'drawn'}"
                    outs, pair, want = c.call(k, flags, h2_given, noise_given)
                    seen[(flags, k, h2_given, noise_given)] = c.compare(outs, pair, want, what).numpy()
    # the terms are really there: the flags, every weight, the drawn noise and the guidance each change the bits
    full = seen[(3, 7, True, True)]
    assert not np.array_equal(full, seen[(1, 7, True, True)]), "guided"
    assert not np.array_equal(full, seen[(2, 7, True, True)]), "replace"
    assert not np.array_equal(full, seen[(3, 7, True, False)]), "the drawn noise is not the buffer's"
    for bit in range(3):
        assert not np.array_equal(full, seen[(3, 7 & ~(1 << bit), True, True)]), f"term {bit}"
    assert not np.array_equal(seen[(3, 3, True, True)], seen[(3, 3, False, True)]), "h2 null: no w2 term"
    # the canvas sample with L_n = 0 has no guidance term: the bits of the row with rho = 0; the others have one
    N = case[0]
    unguided = R.update32(c.rows[9], 3, c.flat("x"), c.beps.reshape(N, -1), c.flat("z"), c.flat("m0"), c.flat("m1"), c.flat("m2"), c.flat("y"),
                          c.flat("m"), c.gsum.reshape(N, -1), c.Ln, True)[0]
    full = full.reshape(N, -1)
    assert np.array_equal(full[-1], unguided[-1]) and not np.array_equal(full[0], unguided[0])


@pytest.mark.parametrize("flags, k, h2_given, noise_given", [(3, 7, True, False), (1, 6, False, True), (0, 3, True, True), (2, 5, True, False)])
def test_update_on_a_canvas_sample_longer_than_the_grid(flags, k, h2_given, noise_given):
    c = _Case(BIG, "tri")
    outs, pair, want = c.call(k, flags, h2_given, noise_given)
    c.compare(outs, pair, want, f"grid stride, flags {flags}, row {k}")


@pytest.mark.parametrize("case", [KERNEL_CASES[1], KERNEL_CASES[3]], ids=str)
def test_final_row_returns_y_where_the_mask_is_one(case):
    c = _Case(case, "tri")
    x_bad = c.v["x"].copy()
    x_bad[..., ::3] = np.inf  # cx = 0: x_t does not reach the known region (guided: nor the prediction, which is read)
    for flags in (1, 3):
        outs, pair, want = c.call(8, flags, True, True, x_init=x_bad if flags == 3 else None)
        got = c.compare(outs, pair, want, f"final row, flags {flags}").view(c.shape)
        KH.same(got[torch.as_tensor(c.v["m"] == 1)], torch.as_tensor(c.v["y"][c.v["m"] == 1]), "the known region is y")


def test_exports_refuse_bad_arguments_and_write_nothing():
    st = _lib.stream()
    c = _Case((2, 2, 32, 16, 3, 8), "tri")
    ro = {s: KH.Ro(c.v[s]) for s in ("z", "y", "m")}
    dwin, part, ctr = KH.Ro(c.dwin), KH.Ro(c.parts), KH.Ro([7], torch.int32)
    outs = {s: KH.Out(c.n) for s in ("x", "x0", "h1", "h2", "beps")}
    seed_out, part_out = KH.Out(c.nwin), KH.Out(c.parts.size)
    good = dict(x=outs["x"].ptr, eps=c.epsd.ptr, noise=ro["z"].ptr, x0=outs["x0"].ptr, h1=outs["h1"].ptr, h2=outs["h2"].ptr, y=ro["y"].ptr,
                mask=ro["m"].ptr, dwin=dwin.ptr, parts=part.ptr, jf=c.jf.ptr, cn=c.cn.ptr, wt=c.wt.ptr, coef=c.coef.ptr, step=ctr.ptr, N=2, W=3,
                C=2, L=64, T=32, H=16, F=8, flags=3, first=0, beps=outs["beps"].ptr, seed=seed_out.ptr, pout=part_out.ptr)
    shapes = [dict(N=0), dict(W=0), dict(N=30000), dict(C=0), dict(L=65), dict(H=0), dict(L=66, H=33), dict(F=6), dict(F=0), dict(T=0),
              dict(L=32 + 2 * 3, H=3), dict(wt=None)]
    nulls = [dict(x=None), dict(eps=None), dict(x0=None), dict(jf=None), dict(cn=None), dict(coef=None), dict(step=None)]
    update_only = [dict(h1=None), dict(y=None), dict(mask=None, flags=1), dict(dwin=None), dict(parts=None, flags=2), dict(flags=4), dict(flags=-1),
                   dict(first=2 ** 32 - 1)]
    for edit in nulls + update_only + shapes:
        a = dict(good, **edit)
        rc = KH.lib().ddimxwis_multistep_update(a["x"], a["eps"], a["noise"], a["x0"], a["h1"], a["h2"], a["y"], a["mask"], a["dwin"], a["parts"],
                                                a["jf"], a["cn"], a["wt"], a["coef"], a["step"], a["N"], a["W"], a["C"], a["L"], a["T"], a["H"],
                                                a["F"], a["flags"], SEED, a["first"], 0, st)
        KH.refused(rc, outs["x"], outs["x0"], outs["h1"], outs["h2"], who="ddimxwis_multistep_update")
    for edit in nulls + [dict(y=None), dict(mask=None), dict(beps=None), dict(seed=None), dict(pout=None)] + shapes:
        a = dict(good, **edit)
        rc = KH.lib().ddimxwis_residual(a["x"], a["eps"], a["y"], a["mask"], a["x0"], a["beps"], a["seed"], a["pout"], a["jf"], a["cn"], a["wt"],
                                        a["coef"], a["step"], a["N"], a["W"], a["C"], a["L"], a["T"], a["H"], a["F"], st)
        KH.refused(rc, outs["x"], outs["x0"], outs["beps"], seed_out, part_out, who="ddimxwis_residual")
    for r in list(ro.values()) + [dwin, part, ctr, c.epsd, c.coef, c.jf, c.cn, c.wt]:
        r.check("refusals")
    assert KH.lib().ddimx_abi_version() == 2


# ---- the sampler on the tiny model ------------------------------------------------------------------------------------------------------
CANVAS = (2, 2, 48, 32)  # W = 5 windows of 16 at hop 8, K = 2
KW = dict(window=16, hop=8, taper="tri")


def _soft_mask(shape):
    b, c, t, f = shape
    m = torch.ones(b, 1, t, f)
    m[:, :, t // 4: t // 2] = 0
    m[:, :, :, -f // 4:] *= 0.5
    m[-1, :, : t // 8] = 0
    return m


def _stream(tau, seed=41, first=3):
    return NoiseStream(seed, first) if tau else None


# ---- 2. one window is inpaint_solver_steps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.0, 1.0])
@pytest.mark.parametrize("n", [3, 10], ids=["eager", "replayed"])
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "replace_only"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_one_window_is_inpaint_solver_steps(mode, guided, order, n, tau):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, shape = MH.alphas(cfg), (2, 2, 16, 32)
    x, y = MH.pair_data("wisolve.one", shape)
    seq = logsnr_seq(a, n)
    assert len(seq) == n
    kw = dict(y=y, mask=_soft_mask(shape), guidance=0.3 if guided else 0.0, replace=True, order=order, tau=tau)
    want = D.inpaint_solver_steps(x.cuda(), seq, m, a, None, noise=_stream(tau), **kw)
    for taper in TAPERS:
        got = D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, window=16, taper=taper, noise=_stream(tau), **kw)
        assert bool(torch.isfinite(got[0][-1]).all())
        MH.same_run(got, want, taper)
    if guided:
        free = D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, window=16, noise=_stream(tau), **dict(kw, guidance=0.0))
        assert MH.differs_anywhere(free, got), "the guidance acted"


# ---- 3. an empty mask with rho = 0 is windowed_solver_steps ----------------------------------------------------------------------------------
@pytest.mark.parametrize("replace", [True, False], ids=["replace", "plain"])
@pytest.mark.parametrize("tau", [0.0, 1.0])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_empty_mask_without_guidance_is_windowed_solver_steps(mode, order, tau, replace):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    x, y = MH.pair_data("wisolve.empty", CANVAS)
    seq = logsnr_seq(a, 6)
    want = D.windowed_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=tau, noise=_stream(tau), **KW)
    got = D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y, mask=torch.zeros(1, 1, 1, 1), guidance=0.0, replace=replace,
                                          order=order, tau=tau, noise=_stream(tau), **KW)
    MH.same_run(got, want, f"order {order}, tau {tau}, replace {replace}")


# ---- 4. no overlap, no guidance, is a batch of segments -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_no_overlap_is_inpaint_solver_steps_over_the_segments_as_a_batch(mode, order):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    T, W, N = 16, 3, 2
    shape = (N, 2, W * T, 32)
    x, y = MH.pair_data("wisolve.segments", shape)
    mask = torch.broadcast_to(_soft_mask(shape), shape).contiguous()
    seg = lambda v: torch.stack([v[n, :, j * T:(j + 1) * T] for n in range(N) for j in range(W)])  # noqa: E731  (sample 3 n + j)
    a = MH.alphas(cfg)
    seq = logsnr_seq(a, 6)
    kw = dict(guidance=0.0, replace=True, order=order)
    want = D.inpaint_solver_steps(seg(x).cuda(), seq, m, a, None, y=seg(y), mask=seg(mask), **kw)
    got = D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, window=T, hop=T, y=y, mask=mask, **kw)
    MH.same_run(([got[0][0]] + [seg(u) for u in got[0][1:]], [seg(u) for u in got[1]]), want, "segments")
    # guided, the norm belongs to the canvas sample and not to the segment: the two runs are different samplers
    gseg = D.inpaint_solver_steps(seg(x).cuda(), seq, m, a, None, y=seg(y), mask=seg(mask), **dict(kw, guidance=0.3))
    gcan = D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, window=T, hop=T, y=y, mask=mask, **dict(kw, guidance=0.3))
    assert all(bool(torch.isfinite(u).all()) for u in gcan[0][1:] + gcan[1])
    assert not torch.equal(seg(gcan[0][-2]), gseg[0][-2]) and MH.differs_anywhere(gcan, got)


# ---- 5. order 1 without replacement is windowed_inpaint_steps with guidance_per_step --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(tag, order, guidance, replace, prediction="eps"):
    """The fp64 restatement over the CPU oracle's forward, once for both activation dtypes of the GPU model (the weights are the
    same).  ``guidance``: a float or a tuple, one value per iteration."""
    cfg, m = (MH.build("tiny", MODES[0][0], 5, mode="eval") if prediction == "eps" else MH.pair("tiny", MODES[0][0])[:2])
    a = MH.alphas(cfg)
    x, y = MH.pair_data("wisolve." + tag, CANVAS)
    mask = _soft_mask(CANVAS)
    seq = [0, 250, 500, 750] if order == 1 else logsnr_seq(a, 5)
    if prediction == "v":
        live, ocfg = MH.oracle(m, "tiny")
        sd = {k: v.detach() for k, v in live.items()}
        fn = lambda w, t, j: ref_cpu.model_forward(sd, ocfg, w.float(), t).to(w.dtype)  # noqa: E731
    else:
        fn = MH.oracle_eps(m)
    rho = list(guidance) if isinstance(guidance, tuple) else guidance
    ref = WIS.steps(x.double(), seq, fn, a, 16, 8, "tri", y, mask, guidance=rho, replace=replace, order=order, prediction=prediction)
    return x, y, mask, seq, rho, ref


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_order_1_guided_is_windowed_inpaint_steps_with_guidance_per_step(mode):
    """Both functions against the fp64 restatement of the folded form over the CPU oracle, each inside model_harness's gate."""
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 5, mode="eval")
    a = MH.alphas(cfg)
    x, y, mask, seq, rho, ref = _reference("o1", 1, 0.3, False)
    new = D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=rho, replace=False, order=1, **KW)
    old = D.windowed_inpaint_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=list(guidance_per_step(seq, a, rho)), replace=False, **KW)
    worst = 0.0
    for i in range(len(seq)):
        for got, name in ((new, "windowed_inpaint_solver_steps"), (old, "windowed_inpaint_steps")):
            worst = max(worst, MH.gate(got[0][i + 1], ref[0][i + 1], dt, f"{name} xs[{i + 1}]")[0])
            MH.gate(got[1][i], ref[1][i], dt, f"{name} x0[{i}]")
    assert torch.equal(new[1][0], old[1][0]), "the first prediction sees no guidance yet"
    unguided = D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=0.0, replace=False, order=1, **KW)
    assert MH.differs_anywhere(new, unguided)
    print(f"[windowed inpaint solver order 1 vs windowed_inpaint_steps {MODE_IDS[dt]}] worst max {worst:.3e} x rms")


# ---- 6. the trajectory against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True], ids=["replace_only", "guided"])
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_trajectory_vs_the_restatement_on_the_cpu_oracle(mode, order, guided):
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 5, mode="eval")
    a = MH.alphas(cfg)
    x, y, mask, seq, rho, (rxs, rx0) = _reference("traj", order, tuple(RHO5) if guided else 0.0, True)
    assert len(seq) == 5
    xs, x0 = D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=rho, replace=True, order=order, **KW)
    worst = (0.0, 0.0)
    for i in range(len(seq)):
        worst = max(worst, MH.gate(xs[i + 1], rxs[i + 1], dt, f"xs[{i + 1}]"))
        worst = max(worst, MH.gate(x0[i], rx0[i], dt, f"x0[{i}]"))
    print(f"[windowed inpaint solver vs restatement order {order} {'guided' if guided else 'replace'} {MODE_IDS[dt]}] worst max "
          f"{worst[0]:.3e} rms err {worst[1]:.3e} x rms")
    MH.known_exact(xs[-1], y, mask)
    if guided:
        plain = _reference("traj", order, 0.0, True)[5][0]
        assert float((plain[-2] - rxs[-2]).abs().max()) > 1e-3, "the reference's guidance is no small term"


# ---- 7. the stepper ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "replace_only"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_replayed_equals_eager(mode, guided):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    x, y = MH.pair_data("wisolve.replay", CANVAS)
    kw = dict(KW, y=y, mask=_soft_mask(CANVAS), guidance=0.3 if guided else 0.0, order=3, tau=1.0, noise=NoiseStream(42, 1))
    seq = logsnr_seq(a, 6)
    got = D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, **kw)
    with MH.eager_steps():
        MH.same_run(D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, **kw), got, "eager")
    assert MH.differs_anywhere(got, D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, **dict(kw, tau=0.0))), "the noise is no small term"


@pytest.mark.parametrize("guided", [True, False], ids=["guided", "replace_only"])
def test_stepper_captures_one_graph_and_owns_its_history(guided):
    cfg, m = MH.build("tiny", "torch.cuda.FloatTensor", 5, mode="eval")
    a = MH.alphas(cfg)
    x = synth.gaussian("wisolve.own", CANVAS).cuda()
    seq = logsnr_seq(a, 6)
    coef = inpaint_solver_coefficients(seq, a, 3, 1.0, 0.3 if guided else 0.0)
    make = lambda c, order, g, **kw: WindowInpaintSolverStepper(m, x, torch.zeros_like(x), torch.ones_like(x), c, order, g, True, 16, 8, "tri", **kw)  # noqa: E731
    with torch.no_grad():
        st = make(coef, 3, guided, noise=NoiseStream(1, 0))
        try:
            for _ in range(len(seq)):
                st.step()
            assert st.captures == 1 and st.graph is not None
            assert st.h1.shape == st.h2.shape == st.x0.shape == x.shape and st.noise_buf is None
            assert st.win.shape == (10, 2, 16, 32) and st.t.numel() == 10
            if guided:
                assert st.beps.shape == x.shape and st.seed.shape == st.d_x.shape == st.win.shape
                assert st.partials.numel() == _lib.load().ddimxwi_partials_floats(2, x[0].numel())
                refs = {r.data_ptr() for r in st._refs}
                assert m._packed_bwd.data_ptr() in refs and m._packed.data_ptr() in refs, "captured_refs(backward=True)"
            else:
                assert st.beps is None and st.seed is None and st.partials is None
            st.rewind()
            m.invalidate()  # new packed values in place: the graph stays
            st.step()
            assert st.captures == 1
        finally:
            st.close()
        st = make(inpaint_solver_coefficients(seq, a, 2, 0.0, 0.0), 2, False)
        assert st.h2 is None and st.seed is None and st.beps is None
        st.close()
        with pytest.raises(ValueError, match="beyond its order"):
            make(coef, 2, guided, noise=NoiseStream(1, 0))


def test_callers_tensors_and_select_index():
    cfg, m = MH.build("tiny", "torch.cuda.FloatTensor", 5, mode="eval")
    a = MH.alphas(cfg)
    x, y = MH.pair_data("wisolve.conv", CANVAS)
    mask = _soft_mask(CANVAS)
    seq = logsnr_seq(a, 6)
    kw = dict(KW, guidance=0.3, order=2)
    xs, x0 = D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, **kw)
    assert len(xs) == 7 and len(x0) == 6 and all(u.shape == CANVAS and not u.is_cuda for u in xs[1:] + x0)
    xc, yc, mc = x.cuda(), y.cuda(), mask.cuda()
    y_keep, m_keep = yc.clone(), mc.clone()
    sxs, sx0 = D.windowed_inpaint_solver_steps(xc, seq, m, a, [1, -1], y=yc, mask=mc, **kw)
    assert sxs[0] is xc and torch.equal(xc.cpu(), xs[-1]), "the caller's x is the state, updated in place"
    assert torch.equal(yc, y_keep) and torch.equal(mc, m_keep), "y and mask are the caller's, untouched"
    MH.same_list(sxs[1:], [xs[2], xs[6]], "selected xs")
    MH.same_list(sx0, [x0[1], x0[5]], "selected x0")
    xh = x.clone()  # a CPU tensor: copied, not updated
    hxs, _ = D.windowed_inpaint_solver_steps(xh, seq, m, a, [-1], y=y, mask=mask, **dict(kw, guidance=0.0))
    assert hxs[0] is xh and torch.equal(xh, x)


# ---- 8. a canvas does not depend on its batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "replace_only"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_two_canvas_samples_equal_two_runs_of_one(mode, guided):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    x, y = MH.pair_data("wisolve.batch", CANVAS)
    mask = _soft_mask(CANVAS)
    mask[-1, :, :6] = 1.0  # (the soft mask empties the last sample's start; every sample keeps a norm)
    seq = logsnr_seq(a, 5)
    kw = dict(KW, guidance=0.3 if guided else 0.0, replace=True, order=3, tau=1.0)
    both = D.windowed_inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, noise=NoiseStream(99, 4), **kw)
    for n in range(2):
        one = D.windowed_inpaint_solver_steps(x[n:n + 1].cuda(), seq, m, a, None, y=y[n:n + 1], mask=mask[n:n + 1],
                                              noise=NoiseStream(99, 4 + n), **kw)
        MH.same_run(one, ([u[n:n + 1] for u in both[0]], [u[n:n + 1] for u in both[1]]), f"canvas sample {n}")
    assert not torch.equal(both[0][-2][0], both[0][-2][1])


# ---- 9. a v model ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_v_model_equals_the_wrapped_eps_callable(mode):
    """Replacement only: every window's v is converted with the window's own input before the blend, so the run equals the one over
    a callable that converts its own output.  Guided (a Model only): against the restatement, whose autograd runs through the
    conversion and the blend, over the oracle's v."""
    dtype_str, dt = mode
    cfg, mv, ms, a = MH.pair("tiny", dtype_str)
    x, y = MH.pair_data("wisolve.v", CANVAS)
    mask = _soft_mask(CANVAS)
    kw = dict(KW, y=y, mask=mask, order=2, tau=1.0, noise=NoiseStream(44, 2))
    seq = logsnr_seq(a, 6)
    got = D.windowed_inpaint_solver_steps(x.cuda(), seq, mv, a, None, **kw)
    with MH.eager_steps():  # the callable allocates
        want = D.windowed_inpaint_solver_steps(x.cuda(), seq, MH.v_wrapped(ms, v_table(a)), a, None, prediction="eps", **kw)
    MH.same_run(got, want, "v model")
    assert MH.differs_anywhere(got, D.windowed_inpaint_solver_steps(x.cuda(), seq, ms, a, None, **kw)), "the twin reads the output as eps"
    MH.known_exact(got[0][-1], y, mask)
    x, y, mask, seq, rho, (rxs, rx0) = _reference("v.guided", 2, tuple(RHO5), True, "v")
    xs, x0 = D.windowed_inpaint_solver_steps(x.cuda(), seq, mv, a, None, y=y, mask=mask, guidance=rho, order=2, **KW)
    for i in range(len(seq)):
        MH.gate(xs[i + 1], rxs[i + 1], dt, f"guided v xs[{i + 1}]")
        MH.gate(x0[i], rx0[i], dt, f"guided v x0[{i}]")
    MH.known_exact(xs[-1], y, mask)
    again = D.windowed_inpaint_solver_steps(x.cuda(), seq, mv, a, None, y=y, mask=mask, guidance=rho, order=2, prediction="v", **KW)
    MH.same_run(again, (xs, x0), "prediction='v' given")


# ---- 10. the study on the device ---------------------------------------------------------------------------------------------------------------
def test_device_repeats_the_replacement_only_study_in_fp32():
    """tests/test_window_inpaint_solver_cpu.py's study with blend and update running in the kernel in fp32: the callable is the
    per-window correlated Gaussian's exact predictor, window j = batch index mod W, against the float64 order-2 run on
    logsnr_seq(a, 734).  Errors of 1e-2 sit far above the fp32 floor."""
    a = MH.alphas()
    Md = torch.from_numpy(WIS.conv_matrices(a)).float().to(G.dev())  # [W, n_table, T, T]
    j = (torch.arange(WS.CONV_W) % WS.CONV_W).to(G.dev())  # one canvas sample: sample b of the window batch is window b % W

    def model(xw, t):  # [W, C, T, F]; eps[b, c, r, f] = sum_s M[j_b][t_b][r, s] x[b, c, s, f]: no host read, no library call
        return (Md[j, t][:, None, :, :, None] * xw[:, :, None, :, :]).sum(3)

    x, y, mask = WIS.conv_case()

    def final(seq, order, **kw):
        with MH.eager_steps():  # the callable allocates
            xs, _ = D.windowed_inpaint_solver_steps(x.float().cuda(), seq, model, a, [-1], window=WS.CONV_T, hop=WS.CONV_H,
                                                    taper=WS.CONV_TAPER, y=y.float(), mask=mask, order=order, **kw)
        return xs[-1]

    err = WIS.conv_study(a, lambda n: logsnr_seq(a, n), modes={"replace": WIS.CONV_MODES["replace"]}, orders=(1, 2), final=final)["replace"]
    print(f"[windowed inpaint solver study on the device]\n{WIS.conv_table(err, orders=(1, 2))}")
    for what, ratio, bound in WS.conv_conditions(err):
        print(f"[windowed inpaint solver study on the device] {what}: {ratio:.3f} (<= {bound})")
        assert ratio <= bound, (what, ratio)
