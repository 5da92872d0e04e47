"""The GroupNorm kernel family one by one (tensor_stats, gn_finalize, gn_finalize_groups and the in-kernel finalisation, resid in
all its modes, gn_bwd_stats / gn_bwd_finalize / gn_bwd_apply, partsum, partsum_multi, colsum_multi and the statistics epilogue of the
data-gradient convs) through their own C-ABI entry points, against the fp64 references of tests/gn_kernel_ref.py.

Every output lives inside a sentinel-filled allocation with guard bands (``Out`` of tests/kernel_harness.py: every byte 0xFF, a NaN
in fp32 and bf16, compared byte by byte afterwards); statistics slabs and workspaces are NaN before each
call, so a slab that is read without having been written, or written where it should not be, shows.  Sums of dyadic operands are
compared bit for bit; sums through SiLU or products at n 2^-24 sum |terms|; element-wise outputs at the fp32 gate of
tests/gpu_util.py (bf16: one ulp on top); and what the source promises "bit for bit" with torch.equal.  The gated tests print the
measured worst errors in units of their gate."""
import ctypes

import pytest
import torch

from ddim_audio_amd import _lib
import exact_util as X
import gn_kernel_ref as R
import gpu_util as G
from kernel_harness import NAN, Out, dev, dev32, lib as load_lib, refused, report, same

pytestmark = pytest.mark.gpu


def act(t, dt):
    """An activation [B][HW][C] (fp64, already on the dtype's grid) on the device in the case's dtype."""
    return dev(t, R.tdt(dt))


def shape(c):
    return R.B, c["H"] * c["W"], c["C"]


# ---- launch wrappers ---------------------------------------------------------------------------------------------------------------------
def run_tensor_stats(c, x, groups, Bn=R.B):
    """x: device tensor [Bn][HW][C].  Returns the slabs [Bn][np][C][2] (groups: [Bn][np][32]) on the CPU."""
    geo = R.geometry(c["dt"], c["C"], c["H"], c["W"])
    per = R.SLAB if groups else 2 * c["C"]
    st = Out(Bn * geo["nparts"] * per)
    _lib.check(load_lib().ddimx_tensor_stats(c["dt"], _lib.ptr(x), st.ptr, Bn, c["H"], c["W"], c["C"], groups, _lib.stream()))
    torch.cuda.synchronize()
    out = st.read("tensor_stats")
    return out.view(Bn, geo["nparts"], R.SLAB) if groups else out.view(Bn, geo["nparts"], c["C"], 2)


def run_resid(c, x, h, mode, scale=None, shift=None, gn=None, groups=0, want_stats=True, Bn=R.B, expect_fail=False):
    """ddimx_resid_ex.  x, h, scale, shift: device tensors; gn = (slabs [Bn][np][32] device, np, gamma, beta or None, count).
    Returns (y as stored, slabs or None) on the CPU."""
    dt, C = c["dt"], c["C"]
    geo = R.geometry(dt, C, c["H"], c["W"])
    y = Out(Bn * geo["HW"] * C, R.tdt(dt))
    st = Out(Bn * geo["nparts"] * (R.SLAB if groups else 2 * C))
    g = gn or (None, 0, None, None, 1.0)
    rc = load_lib().ddimx_resid_ex(dt, C, _lib.ptr(x), _lib.ptr(h), mode, _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(g[0]), g[1], _lib.ptr(g[2]),
                                _lib.ptr(g[3]), g[4], R.EPS, y.ptr, st.ptr if want_stats else None, groups, Bn, c["H"], c["W"], _lib.stream())
    torch.cuda.synchronize()
    if expect_fail:
        refused(rc, y, st)
        return None, None
    _lib.check(rc)
    yv = y.read("resid y").view(Bn, geo["HW"], C)
    if not want_stats:
        assert st.untouched()
        return yv, None
    sv = st.read("resid statistics")
    return yv, sv.view(Bn, geo["nparts"], R.SLAB) if groups else sv.view(Bn, geo["nparts"], C, 2)


def run_bwd_stats(c, mode, g, u, scale=None, shift=None, Bn=R.B):
    geo = R.geometry(c["dt"], c["C"], c["H"], c["W"])
    st = Out(Bn * geo["nparts"] * 2 * c["C"])
    _lib.check(load_lib().ddimx_gn_bwd_stats(c["dt"], mode, _lib.ptr(g), _lib.ptr(u), _lib.ptr(scale), _lib.ptr(shift), st.ptr, Bn, c["H"],
                                          c["W"], c["C"], _lib.stream()))
    torch.cuda.synchronize()
    return st.read("gn_bwd_stats").view(Bn, geo["nparts"], c["C"], 2)


def run_bwd_finalize(slabs, C, count, gamma, mr):
    """slabs [B][np][C][2] fp32 (CPU) -> (coef [B][3][C], dgb [B][2][C])."""
    Bn, nparts = slabs.shape[:2]
    sd, gd, md = dev32(slabs), dev32(gamma), dev32(mr)
    coef, dgb = Out(Bn * 3 * C), Out(Bn * 2 * C)
    _lib.check(load_lib().ddimx_gn_bwd_finalize(_lib.ptr(sd), nparts, C, count, _lib.ptr(gd), _lib.ptr(md), coef.ptr, dgb.ptr, Bn, _lib.stream()))
    torch.cuda.synchronize()
    return coef.read("coef").view(Bn, 3, C), dgb.read("dgb").view(Bn, 2, C)


def run_bwd_apply(c, mode, g, u, coef, scale=None, shift=None, gy=None, extra=None, nu=None, want_sums=False, want_nstats=False, Bn=R.B):
    """Returns (out as stored, sums [Bn][np][C] or None, nstats [Bn][np][C][2] or None) on the CPU."""
    dt, C = c["dt"], c["C"]
    geo = R.geometry(dt, C, c["H"], c["W"])
    out = Out(Bn * geo["HW"] * C, R.tdt(dt))
    sums, nst = Out(Bn * geo["nparts"] * C), Out(Bn * geo["nparts"] * 2 * C)
    _lib.check(load_lib().ddimx_gn_bwd_apply(dt, mode, _lib.ptr(g), _lib.ptr(u), _lib.ptr(gy), _lib.ptr(extra), _lib.ptr(coef), _lib.ptr(scale),
                                          _lib.ptr(shift), out.ptr, sums.ptr if want_sums else None, _lib.ptr(nu) if want_nstats else None,
                                          nst.ptr if want_nstats else None, Bn, c["H"], c["W"], C, _lib.stream()))
    torch.cuda.synchronize()
    o = out.read("gn_bwd_apply out").view(Bn, geo["HW"], C)
    s = sums.read("sums").view(Bn, geo["nparts"], C) if want_sums else None
    n = nst.read("nstats").view(Bn, geo["nparts"], C, 2) if want_nstats else None
    assert want_sums or sums.untouched()
    assert want_nstats or nst.untouched()
    return o, s, n


# ---- tensor_stats ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_tensor_stats(c):
    """tensor_stats_kernel in both slab formats.  Dyadic x (k / 8): every slab equals the fp64 sums of its pixels bit for bit, the
    group format's 16 padding floats are zero.  Gaussian x: within chain * 2^-24 * sum |terms| of fp64.
    Measured on MI355X: Gaussian sums at most 0.59 of the bound (fp32; bf16 0.23)."""
    dt = c["dt"]
    geo = R.geometry(dt, c["C"], c["H"], c["W"])
    x = R.dyadic_x("ts." + c["id"], shape(c))
    want = R.chan_stats(x, geo["rpp"])
    xd = act(x, dt)
    assert torch.equal(run_tensor_stats(c, xd, 0).double(), want)
    assert torch.equal(run_tensor_stats(c, xd, 1).double(), R.group_slabs(want))
    x = R.rnd(R.gauss("ts.g." + c["id"], shape(c)) + 0.5, dt)
    want = R.chan_stats(x, geo["rpp"])
    ab = torch.stack([R.part_sums(x.abs(), geo["rpp"]), want[..., 1]], -1)
    xd = act(x, dt)
    w0 = R.gate_sum(run_tensor_stats(c, xd, 0), want, ab, R.chain(geo), "channel slabs")
    gs = run_tensor_stats(c, xd, 1)
    assert not bool(gs[..., 16:].any()), "padding of the group slabs must be written as zero"
    w1 = R.gate_sum(gs, R.group_slabs(want), R.group_slabs(ab), R.chain(geo, True), "group slabs")
    report(f"tensor_stats {c['id']}", max(w0, w1), "of the summation bound")


# ---- gn_finalize -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mr", [False, True], ids=["", "mr"])
@pytest.mark.parametrize("has_beta", [False, True], ids=["nobeta", "beta"])
@pytest.mark.parametrize("nparts", R.FINALIZE_NPARTS)
@pytest.mark.parametrize("reps", R.FINALIZE_REPS)
def test_gn_finalize(reps, nparts, has_beta, mr):
    """gn_finalize_kernel at C = 96 (groups of 12), slabs of Cs = C and 2 C channels, 1 .. 1025 parts, values of mean 2 and std 1:
    scale, shift, mean and rstd against fp64 on the same fp32 slabs, fp32 gate.  Measured on MI355X: at most 2.3e-3 of the gate."""
    C, m = 96, 4
    Cs = reps * C
    st = R.synthetic_slabs(f"fin.{reps}.{nparts}", nparts, Cs, m, offset=2.0)
    gamma, beta = R.gamma_beta("fin", C)
    if not has_beta:
        beta = None
    count = float(nparts * m * reps * (C // R.GROUPS))
    tot = R.fold_groups(st.sum(1).view(R.B, reps, C, 2).sum(1))
    want = R.gn_fold(tot[..., 0], tot[..., 1], count, gamma, beta)
    sd, gd, bd = dev32(st), dev32(gamma), None if beta is None else dev32(beta)
    scale, shift, mro = Out(R.B * C), Out(R.B * C), Out(R.B * R.GROUPS * 2)
    _lib.check(load_lib().ddimx_gn_finalize(_lib.ptr(sd), nparts, Cs, C, count, _lib.ptr(gd), _lib.ptr(bd), R.EPS, scale.ptr, shift.ptr,
                                         mro.ptr if mr else None, R.B, _lib.stream()))
    torch.cuda.synchronize()
    mv = mro.read("mean / rstd").view(R.B, R.GROUPS, 2) if mr else None
    assert mr or mro.untouched()
    worst = R.gate_stats_of_norm(scale.read("scale").view(R.B, C), shift.read("shift").view(R.B, C), None if mv is None else mv[..., 0],
                                 None if mv is None else mv[..., 1], want, "gn_finalize")
    report(f"gn_finalize reps={reps} nparts={nparts}", worst / G.TOL[G.F32]["mx"])


def _group_slabs(tag, np_, nan_padding=True):
    """Group-format slabs [B][np][32] (fp32 numbers as fp64) of 16 Gaussian values of mean 1 per (part, group), and the values'
    count per group.  The 16 floats no consumer reads hold NaN."""
    st = R.synthetic_slabs(tag, np_, R.GROUPS, 16, offset=1.0)  # [B][np][8][2]
    pad = torch.full((R.B, np_, 16), NAN if nan_padding else 0.0, dtype=torch.float64)
    return torch.cat([st.reshape(R.B, np_, 16), pad], -1), st, float(np_ * 16)


def run_finalize_groups(slabs_d, np_, gamma_d, beta_d, count, C, nthreads, expect_fail=False):
    scale, shift = Out(R.B * C), Out(R.B * C)
    rc = load_lib().ddimx_gn_finalize_groups(_lib.ptr(slabs_d), np_, _lib.ptr(gamma_d), _lib.ptr(beta_d), count, R.EPS, C, scale.ptr, shift.ptr,
                                          R.B, nthreads, _lib.stream())
    torch.cuda.synchronize()
    if expect_fail:
        refused(rc, scale, shift)
        return None, None
    _lib.check(rc)
    return scale.read("scale").view(R.B, C), shift.read("shift").view(R.B, C)


@pytest.mark.parametrize("nthreads", R.GROUPS_NTHREADS)
def test_gn_finalize_groups(nthreads):
    """gn_finalize_groups_kernel (gn_in_issue / gn_in_reduce / gn_in_group) with 64 .. 1024 threads over np = 1, 7, exactly one round
    (nthreads partials), one more (the further-rounds loop), 256 and 600 partials, beta null for odd np: scale and shift against
    fp64 on the same slabs, fp32 gate.  Block sizes the launcher cannot take are refused.
    Measured on MI355X: at most 5.1e-3 of the gate."""
    C = 96
    gamma, beta = R.gamma_beta("fg", C)
    gd, bd = dev32(gamma), dev32(beta)
    worst = 0.0
    for np_ in R.groups_np(nthreads):
        slabs, st, count = _group_slabs(f"fg.{nthreads}.{np_}", np_)
        b = None if np_ % 2 else beta
        tot = st.sum(1)
        want = R.gn_fold(tot[..., 0], tot[..., 1], count, gamma, b)
        scale, shift = run_finalize_groups(dev32(slabs), np_, gd, None if b is None else bd, count, C, nthreads)
        worst = max(worst, R.gate_stats_of_norm(scale, shift, None, None, want, f"gn_finalize_groups nthreads={nthreads} np={np_}"))
    report(f"gn_finalize_groups nthreads={nthreads}", worst / G.TOL[G.F32]["mx"])
    slabs, _, count = _group_slabs("fg.bad", 7)
    for bad in (32, 96, 1088):
        run_finalize_groups(dev32(slabs), 7, gd, bd, count, C, bad, expect_fail=True)


# ---- resid -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_resid_modes(c, mode):
    """resid_kernel with scale / shift from memory: y = x + h s + t (mode 0), x + h with h fp32 (1), x + SiLU(h) s + t (2) on Gaussian
    operands against fp64 (fp32 gate; bf16: one ulp on top, reference on the rounded inputs); the statistics of y in both slab
    formats against the fp64 sums of the y that was stored, within chain * 2^-24 * sum |terms|; a null stats pointer changes nothing.
    Measured on MI355X, of the gate: fp32 y 3.3e-3 (mode 0), 1.7e-3 (1), 1.2e-2 (2); bf16 y 0.99 (the ulp term: the fp32 slack is
    not used); statistics at most 0.65 of the bound."""
    dt, C = c["dt"], c["C"]
    geo = R.geometry(dt, C, c["H"], c["W"])
    tag = f"resid.{c['id']}"
    x = R.rnd(R.gauss(tag + ".x", shape(c)), dt)
    h = R.gauss(tag + ".h", shape(c))
    h = h.float().double() if mode == 1 else R.rnd(h, dt)
    gamma, beta = R.gamma_beta(tag, C)
    scale, shift, _, _ = (t.float().double() for t in R.group_norm_fold(R.silu(h) if mode == 2 else h, gamma, beta))
    want = R.resid(x, h, mode, scale, shift)
    xd, hd = act(x, dt), dev32(h) if mode == 1 else act(h, dt)
    sd, td = (None, None) if mode == 1 else (dev32(scale), dev32(shift))
    y, st = run_resid(c, xd, hd, mode, sd, td)
    wy = R.gate_elementwise(y, want, dt, f"resid mode {mode}")
    yd = y.double()
    ref = R.chan_stats(yd, geo["rpp"])
    ab = torch.stack([R.part_sums(yd.abs(), geo["rpp"]), ref[..., 1]], -1)
    ws = R.gate_sum(st, ref, ab, R.chain(geo), "channel statistics")
    y2, gs = run_resid(c, xd, hd, mode, sd, td, groups=1)
    same(y2, y)
    assert not bool(gs[..., 16:].any())
    ws = max(ws, R.gate_sum(gs, R.group_slabs(ref), R.group_slabs(ab), R.chain(geo, True), "group statistics"))
    y3, _ = run_resid(c, xd, hd, mode, sd, td, want_stats=False)
    same(y3, y)
    report(f"resid mode {mode} {c['id']} y", wy)
    report(f"resid mode {mode} {c['id']} statistics", ws, "of the summation bound")


FUSED_CASES = [c for c in R.SMALL if c["H"] == 7 and c["C"] in (32, 96, 192)]


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("c", FUSED_CASES, ids=R.case_id)
def test_resid_fused_finalisation_is_the_launched_one(c, mode):
    """The GroupNorm finished inside resid_kernel (gn_fused.h) against gn_finalize_groups with resid's block size followed by resid
    with scale / shift from memory: y and the statistics of y carry the same bits, in both slab formats -- for 1, 7, one full round
    (the block size), one partial more where that is still <= 256 (192-thread blocks: the further-rounds loop inside resid) and 256
    partials, beta null and non-null."""
    dt, C = c["dt"], c["C"]
    nthreads = load_lib().ddimx_resid_threads(dt, C)
    tag = f"fused.{c['id']}"
    x, h = R.rnd(R.gauss(tag + ".x", shape(c)), dt), R.rnd(R.gauss(tag + ".h", shape(c)) + 1.0, dt)
    xd, hd = act(x, dt), act(h, dt)
    gamma, beta = R.gamma_beta(tag, C)
    gd, bd = dev32(gamma), dev32(beta)
    for np_ in sorted({1, 7, nthreads, min(nthreads + 1, R.FUSE_MAX_PARTS), R.FUSE_MAX_PARTS}):
        slabs, _, count = _group_slabs(f"{tag}.{np_}", np_)
        sl = dev32(slabs)
        for b in (None, bd):
            scale, shift = run_finalize_groups(sl, np_, gd, b, count, C, nthreads)
            for groups in (0, 1):
                y0, s0 = run_resid(c, xd, hd, mode, dev32(scale), dev32(shift), groups=groups)
                y1, s1 = run_resid(c, xd, hd, mode, gn=(sl, np_, gd, b, count), groups=groups)
                same(y1, y0, (np_, b is not None, groups))
                same(s1, s0, (np_, b is not None, groups))


def test_resid_refuses_what_it_cannot_fuse():
    """More than 256 partials, and an fp32 h (mode 1) with in-kernel statistics, come back as errors before any launch."""
    c = FUSED_CASES[0]
    x = act(R.rnd(R.gauss("refuse.x", shape(c)), c["dt"]), c["dt"])
    gamma = dev32(R.gamma_beta("refuse", c["C"])[0])
    slabs, _, count = _group_slabs("refuse", R.FUSE_MAX_PARTS + 1, nan_padding=False)
    sl = dev32(slabs)
    run_resid(c, x, x, 0, gn=(sl, R.FUSE_MAX_PARTS + 1, gamma, None, count), expect_fail=True)
    assert b"resid_launch" in load_lib().ddimx_last_error()
    hf = torch.zeros(shape(c), device=G.dev())
    run_resid(c, x, hf, 1, gn=(sl, 7, gamma, None, count), expect_fail=True)


@pytest.mark.parametrize("dt", R.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("ratio", R.MEAN_OVER_STD)
def test_forward_numerics(ratio, dt):
    """Group means of 0, 4 and 32 standard deviations and one constant group (variance exactly 0, rstd = 1 / sqrt(eps)), gamma with
    mixed signs and a zero, at C = 64, 7 x 11 and C = 32, 104 x 100: tensor_stats -> gn_finalize (channel slabs) and tensor_stats ->
    gn_finalize_groups / the fused resid (group slabs) against fp64 GroupNorm statistics of the tensor itself.  scale, shift at the fp32
    gate, mean in units of the group's std, rstd relative and widened by 1 + mean^2 / var.
    Measured on MI355X (worst over both shapes, of the gate): ratio 0: 1.8e-3, 4: 2.5e-3, 32: 7.7e-2."""
    worst = 0.0
    for c in (R.case(dt, 64, 7, 11, "num"), R.case(dt, 32, 104, 100, "num")):
        C, HW = c["C"], c["H"] * c["W"]
        geo = R.geometry(dt, C, c["H"], c["W"])
        x = R.numerics_x(f"num.{ratio}.{c['id']}", dt, C, HW, ratio)
        gamma, beta = R.gamma_beta("num", C)
        want = R.group_norm_fold(x, gamma, beta)
        count = float(HW * geo["GS"])
        xd, gd, bd = act(x, dt), dev32(gamma), dev32(beta)
        st = dev32(run_tensor_stats(c, xd, 0))
        scale, shift, mro = Out(R.B * C), Out(R.B * C), Out(R.B * 16)
        _lib.check(load_lib().ddimx_gn_finalize(_lib.ptr(st), geo["nparts"], C, C, count, _lib.ptr(gd), _lib.ptr(bd), R.EPS, scale.ptr, shift.ptr,
                                             mro.ptr, R.B, _lib.stream()))
        torch.cuda.synchronize()
        mv = mro.read("mr").view(R.B, R.GROUPS, 2)
        worst = max(worst, R.gate_stats_of_norm(scale.read("scale").view(R.B, C), shift.read("shift").view(R.B, C), mv[..., 0], mv[..., 1], want,
                                                f"gn_finalize ratio {ratio}"))
        assert bool((mv[:, R.CONST_GROUP, 0] == R.CONST_VALUE).all()), "the constant group's mean is exact"
        gs = dev32(run_tensor_stats(c, xd, 1))
        nthreads = load_lib().ddimx_resid_threads(dt, C)
        s2, h2 = run_finalize_groups(gs, geo["nparts"], gd, bd, count, C, nthreads)
        worst = max(worst, R.gate_stats_of_norm(s2, h2, None, None, want, f"gn_finalize_groups ratio {ratio}"))
        if geo["nparts"] <= R.FUSE_MAX_PARTS:
            y0, _ = run_resid(c, xd, xd, 0, dev32(s2), dev32(h2))
            y1, _ = run_resid(c, xd, xd, 0, gn=(gs, geo["nparts"], gd, bd, count))
            same(y1, y0)
            if ratio == 0:
                live = R.group_of(C) != R.CONST_GROUP  # (the constant group's y is a difference of two numbers of size 1 / sqrt(eps))
                wy = R.resid(x, x, 0, want[0], want[1])
                R.gate_elementwise(y1[:, :, live], wy[:, :, live], dt, "fused resid y")
    report(f"forward numerics ratio={ratio}", worst / G.TOL[G.F32]["mx"])


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
_BWD = {}


def _bwd(c, mode):
    """Inputs and fp64 reference of one backward case, computed once."""
    key = (c["id"], mode)
    if key not in _BWD:
        d = R.bwd_inputs(c, mode)
        geo = R.geometry(c["dt"], c["C"], c["H"], c["W"])
        d["PQ"], d["coef"], d["dgb"], _ = R.bwd_reference(d, mode, geo["rpp"])
        d["geo"] = geo
        _BWD[key] = d
    return _BWD[key]


def _sc_sh(d, mode):
    return (dev32(d["scale"]), dev32(d["shift"])) if mode == 1 else (None, None)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_gn_bwd_stats(c, mode):
    """gn_bwd_stats_kernel, mode 0 (P = sum g, Q = sum g SiLU(u)) and mode 1 (g' = g SiLU'(s u + t), P = sum g', Q = sum g' u), on
    g = a_c + b_c vhat + 0.3 noise: every slab within (chain + SILU_OPS) * 2^-24 * sum |terms| of fp64; with a dyadic g, P of mode 0
    equals the fp64 sum bit for bit.  Measured on MI355X: at most 0.18 (mode 0) and 0.29 (mode 1) of the bound."""
    dt = c["dt"]
    d = _bwd(c, mode)
    geo = d["geo"]
    sc, sh = _sc_sh(d, mode)
    gd, ud = act(d["g"], dt), act(d["u"], dt)
    got = run_bwd_stats(c, mode, gd, ud, sc, sh)
    ab = R.bwd_abs_slabs(d["g"], d["u"], mode, geo["rpp"], d["scale"] if mode else None, d["shift"] if mode else None)
    worst = R.gate_sum(got, d["PQ"], ab, R.chain(geo) + R.SILU_OPS, f"gn_bwd_stats mode {mode}")
    if mode == 0:
        g2 = R.dyadic_x("bs." + c["id"], shape(c))
        got = run_bwd_stats(c, 0, act(g2, dt), ud)
        assert torch.equal(got[..., 0].double(), R.part_sums(g2, geo["rpp"]))
    report(f"gn_bwd_stats mode {mode} {c['id']}", worst, "of the summation bound")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", R.GEOM_CASES, ids=R.case_id)
def test_gn_bwd_finalize(c, mode):
    """gn_bwd_finalize_kernel on the fp32-rounded reference slabs of the case (1 .. 65 slabs: the second round of eight partials on
    eight lanes; groups of 4, 12 and 32 channels), a non-zero group mean and the upstream gradient that makes S1, S2 large: ca, cb,
    cc and the per-sample dgamma / dbeta terms each at the fp32 gate against fp64 on the same slabs.
    Measured on MI355X: at most 6.6e-3 of the gate."""
    d = _bwd(c, mode)
    C = c["C"]
    slabs = d["PQ"].float()
    mr = torch.stack([d["mean"], d["rstd"]], -1).float()
    coef, dgb = run_bwd_finalize(slabs, C, d["count"], d["gamma"], mr)
    wc, wg = R.bwd_coef(slabs.double().sum(1), d["count"], d["gamma"], d["mean"], d["rstd"])
    e = [R.gate(coef[:, i], wc[:, i], f"{n} mode {mode}")[0] for i, n in enumerate(("ca", "cb", "cc"))]
    e += [R.gate(dgb[:, i], wg[:, i], f"{n} mode {mode}")[0] for i, n in enumerate(("dgamma terms", "dbeta terms"))]
    report(f"gn_bwd_finalize mode {mode} {c['id']}", max(e) / G.TOL[G.F32]["mx"])


@pytest.mark.parametrize("nparts", [8, 64, 130])
def test_gn_bwd_finalize_slab_counts(nparts):
    """... and on synthetic slabs of 8 (one load per lane), 64 (one full round) and 130 (three rounds) parts at C = 96."""
    C = 96
    slabs = R.gauss(f"bf.{nparts}", (R.B, nparts, C, 2)).float()
    gamma, _ = R.gamma_beta("bf", C)
    mean, rstd = (0.3 * R.gauss("bf.m", (R.B, 8))).float().double(), (1.0 + 0.2 * R.gauss("bf.r", (R.B, 8)).abs()).float().double()
    coef, dgb = run_bwd_finalize(slabs, C, 1000.0, gamma, torch.stack([mean, rstd], -1).float())
    wc, wg = R.bwd_coef(slabs.double().sum(1), 1000.0, gamma, mean, rstd)
    for i in range(3):
        R.gate(coef[:, i], wc[:, i], f"coef {i}")
    for i in range(2):
        R.gate(dgb[:, i], wg[:, i], f"dgb {i}")


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_gn_bwd_apply_mode0(c):
    """gn_bwd_apply_kernel mode 0, du = (ca g + cb SiLU(u) + cc) SiLU'(u), coefficients = the fp32-rounded reference ones: du against
    fp64 (fp32 gate; bf16: one ulp on top); the per-slab channel sums against the fp64 sums of the du that was stored, within
    chain * 2^-24 * sum |terms|; a null sums pointer changes nothing.
    Measured on MI355X: du at most 7.3e-2 of the gate in fp32, 0.98 in bf16 (the ulp term); sums at most 0.44 of the bound."""
    dt = c["dt"]
    d = _bwd(c, 0)
    geo = d["geo"]
    coef = d["coef"].float()
    want = R.bwd_apply(d["g"], d["u"], 0, coef.double())
    gd, ud, cd = act(d["g"], dt), act(d["u"], dt), dev32(coef)
    out, sums, _ = run_bwd_apply(c, 0, gd, ud, cd, want_sums=True)
    wo = R.gate_elementwise(out, want, dt, "du")
    od = out.double()
    ws = R.gate_sum(sums, R.part_sums(od, geo["rpp"]), R.part_sums(od.abs(), geo["rpp"]), R.chain(geo), "sums of du")
    out2, _, _ = run_bwd_apply(c, 0, gd, ud, cd)
    same(out2, out)
    report(f"gn_bwd_apply mode 0 {c['id']} du", wo)
    report(f"gn_bwd_apply mode 0 {c['id']} sums", ws, "of the summation bound")


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_gn_bwd_apply_mode1(c):
    """gn_bwd_apply_kernel mode 1, dx = gy + ca g' + cb x + cc (+ extra), with and without `extra`, with and without the chained
    statistics: dx against fp64 (fp32 gate; bf16: one ulp on top), written to a buffer that aliases no input.  The chained slabs
    equal gn_bwd_stats mode 0 over the stored dx and nu bit for bit -- fp32 and bf16 -- and asking for them does not change dx.
    Measured on MI355X: dx at most 3.2e-2 of the gate in fp32, 0.98 in bf16 (the ulp term)."""
    dt = c["dt"]
    d = _bwd(c, 1)
    coef = d["coef"].float()
    sc, sh = _sc_sh(d, 1)
    gd, ud, yd, ed, nd = (act(d[k], dt) for k in ("g", "u", "gy", "extra", "nu"))
    cd = dev32(coef)
    worst = 0.0
    for extra in (None, ed):
        want = R.bwd_apply(d["g"], d["u"], 1, coef.double(), d["scale"], d["shift"], d["gy"], None if extra is None else d["extra"])
        out, _, _ = run_bwd_apply(c, 1, gd, ud, cd, sc, sh, yd, extra)
        worst = max(worst, R.gate_elementwise(out, want, dt, f"dx extra={extra is not None}"))
        out2, _, nst = run_bwd_apply(c, 1, gd, ud, cd, sc, sh, yd, extra, nd, want_nstats=True)
        same(out2, out, "the chained statistics must not change dx")
        alone = run_bwd_stats(c, 0, dev(out2, out2.dtype), nd)
        same(nst, alone, "chained statistics differ from gn_bwd_stats over the stored dx")
    report(f"gn_bwd_apply mode 1 {c['id']} dx", worst)


def test_gn_bwd_apply_refuses_half_a_chain():
    """nstats without nu, and nstats in mode 0, come back as errors before any launch."""
    c = R.SMALL[1]
    d = _bwd(c, 1)
    dt = c["dt"]
    sc, sh = _sc_sh(d, 1)
    gd, ud, yd, cd = act(d["g"], dt), act(d["u"], dt), act(d["gy"], dt), dev32(d["coef"].float())
    out, nst = Out(gd.numel(), R.tdt(dt)), Out(R.B * d["geo"]["nparts"] * 2 * c["C"])
    for mode, nu in ((1, None), (0, ud)):
        rc = load_lib().ddimx_gn_bwd_apply(dt, mode, _lib.ptr(gd), _lib.ptr(ud), _lib.ptr(yd), None, _lib.ptr(cd), _lib.ptr(sc), _lib.ptr(sh),
                                        out.ptr, None, _lib.ptr(nu), nst.ptr, R.B, c["H"], c["W"], c["C"], _lib.stream())
        refused(rc, out, nst)


@pytest.mark.parametrize("c", R.GEOM_CASES, ids=R.case_id)
def test_every_slab_producer_reduces_in_one_order(c):
    """Every kernel that writes a slab over the sample partition adds a thread's pieces, and then the block's rows, in one order, so
    sums of the same values carry the same bits whoever produced them (Gaussian values: another order would show).  resid in mode 1
    with an fp32 h of zeros stores y = x and writes the slabs of tensor_stats(x), in the channel and in the group format; P of
    gn_bwd_stats(mode 0, g = x) is the `sum` half of tensor_stats(x); the sums of gn_bwd_apply mode 0 are the `sum` half of
    tensor_stats over the du it stored."""
    dt = c["dt"]
    d = _bwd(c, 0)
    x, u = d["g"], act(d["u"], dt)
    xd = act(x, dt)
    hz = torch.zeros(shape(c), device=G.dev())
    ts = run_tensor_stats(c, xd, 0)
    for groups, want in ((0, ts), (1, run_tensor_stats(c, xd, 1))):
        y, st = run_resid(c, xd, hz, 1, groups=groups)
        same(y, xd.cpu(), "resid with h = 0 must store x")
        same(st, want, f"resid statistics differ from tensor_stats (groups = {groups})")
    same(run_bwd_stats(c, 0, xd, u)[..., 0].contiguous(), ts[..., 0].contiguous(), "P of gn_bwd_stats differs from tensor_stats")
    du, sums, _ = run_bwd_apply(c, 0, xd, u, dev32(d["coef"].float()), want_sums=True)
    same(sums, run_tensor_stats(c, dev(du, du.dtype), 0)[..., 0].contiguous(), "sums of gn_bwd_apply differ from tensor_stats over du")


# ---- reductions --------------------------------------------------------------------------------------------------------------------------
def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _partsum_entries():
    """(B, nparts, C) of the multi-reduction entries: unequal C (32, 200), B (1, 3, 19) and slab counts (1, 65)."""
    return [(Bn, np_, C) for C in R.MULTI_C for Bn in R.MULTI_B for np_ in R.MULTI_NPARTS]


def test_partsum_and_partsum_multi():
    """partsum_kernel: sums over 1 and 65 slabs (the second round) of C = 32 and 200 channels (the last block of 32 columns ragged),
    B = 1, 3, 19, with src_step 1 and 2 (the `sum` half of (sum, sumsq) slabs, the other half NaN) and rows of dst 7 floats apart
    from C: dyadic slabs bit for bit against fp64, Gaussian slabs equal to float32(fp64 sum).  partsum_multi_kernel over all twelve
    entries at once: every entry carries the bits of partsum alone, and nothing between the rows of dst is written."""
    lib = load_lib()
    ents = _partsum_entries()
    for kind in ("dyadic", "gauss"):
        singles, srcs, dsts = [], [], []
        for Bn, np_, C in ents:
            tag = f"ps.{kind}.{Bn}.{np_}.{C}"
            src = (R.dyadic_x(tag, (Bn, np_, C)) * 8 if kind == "dyadic" else R.gauss(tag, (Bn, np_, C))).float()
            if kind == "dyadic":
                assert torch.equal(R.partsum(src).double(), src.double().sum(1))
            stride = C + 7
            idx = torch.arange(Bn)[:, None] * stride + torch.arange(C)[None, :]
            for step in (1, 2):
                sd = torch.full((Bn, np_, C * step), NAN, device=G.dev())
                sd[..., ::step] = dev32(src)
                dst = Out(idx=idx)
                _lib.check(lib.ddimx_partsum(_lib.ptr(sd), Bn, np_, C, dst.ptr, stride, step, _lib.stream()))
                torch.cuda.synchronize()
                got = dst.read("partsum")
                same(got, R.partsum(src), (kind, Bn, np_, C, step))
            singles.append(got)
            srcs.append(dev32(src))
            dsts.append(Out(idx=idx))
        n = len(ents)
        _lib.check(lib.ddimx_partsum_multi(_arr(ctypes.c_void_p, [s.data_ptr() for s in srcs]), _arr(ctypes.c_void_p, [d.ptr.value for d in dsts]),
                                           _arr(ctypes.c_longlong, [C + 7 for _, _, C in ents]), _arr(ctypes.c_int, [p for _, p, _ in ents]),
                                           _arr(ctypes.c_int, [C for _, _, C in ents]), _arr(ctypes.c_int, [b for b, _, _ in ents]), n,
                                           _lib.stream()))
        torch.cuda.synchronize()
        for (Bn, np_, C), dst, one in zip(ents, dsts, singles):
            same(dst.read("partsum_multi"), one, (kind, Bn, np_, C))


def test_colsum_multi():
    """colsum_multi_kernel over entries of C = 32 and 200, B = 1, 3, 19, rows 2 C floats apart: one entry per half of every source (the
    dgamma half and the dbeta half of a [B][2][C] slot).  Dyadic values bit for bit against fp64, Gaussian values equal to
    float32(fp64 sum)."""
    lib = load_lib()
    for kind in ("dyadic", "gauss"):
        srcs, ents, dsts, wants = [], [], [], []
        for C in R.MULTI_C:
            for Bn in R.MULTI_B:
                tag = f"cm.{kind}.{Bn}.{C}"
                src = (R.dyadic_x(tag, (Bn, 2 * C)) * 8 if kind == "dyadic" else R.gauss(tag, (Bn, 2 * C))).float()
                sd = dev32(src)
                srcs.append(sd)
                for half in (0, 1):
                    want = R.colsum(src, C, half * C)
                    if kind == "dyadic":
                        assert torch.equal(want.double(), src.double()[:, half * C:(half + 1) * C].sum(0))
                    ents.append((sd.data_ptr() + 4 * half * C, Bn, C))
                    dsts.append(Out(C))
                    wants.append(want)
        _lib.check(lib.ddimx_colsum_multi(_arr(ctypes.c_void_p, [p for p, _, _ in ents]), _arr(ctypes.c_void_p, [d.ptr.value for d in dsts]),
                                          _arr(ctypes.c_longlong, [2 * C for _, _, C in ents]), _arr(ctypes.c_int, [b for _, b, _ in ents]),
                                          _arr(ctypes.c_int, [C for _, _, C in ents]), len(ents), _lib.stream()))
        torch.cuda.synchronize()
        for (p, Bn, C), dst, want in zip(ents, dsts, wants):
            same(dst.read("colsum_multi"), want, (kind, Bn, C))


def test_multi_reductions_refuse_bad_batches():
    lib = load_lib()
    z = _arr(ctypes.c_void_p, [0])
    one = _arr(ctypes.c_int, [1])
    ll = _arr(ctypes.c_longlong, [1])
    assert lib.ddimx_partsum_multi(z, z, ll, one, one, one, 1, _lib.stream()) != 0
    assert lib.ddimx_colsum_multi(z, z, ll, one, one, 0, _lib.stream()) != 0
    assert lib.ddimx_colsum_multi(z, z, ll, one, one, 1000, _lib.stream()) != 0


# ---- a sample's result does not depend on its batch ------------------------------------------------------------------------------------------
ALONE_CASES = [c for c in R.SMALL if c["H"] == 7 and c["C"] in (32, 96, 256)] + [R.ROUNDS65]


@pytest.mark.parametrize("c", ALONE_CASES, ids=R.case_id)
def test_sample_alone_equals_sample_in_batch(c):
    """Sample 1 of the batch of three run alone (B = 1): tensor_stats, resid (mode 2, with statistics), gn_bwd_stats and gn_bwd_apply
    (both modes, chained statistics included) give the bits it got inside the batch."""
    dt = c["dt"]
    one = slice(1, 2)
    d0, d1 = _bwd(c, 0), _bwd(c, 1)
    x = act(d1["u"], dt)
    for groups in (0, 1):
        same(run_tensor_stats(c, x, groups)[one], run_tensor_stats(c, x[one].contiguous(), groups, Bn=1))
    sc, sh = _sc_sh(d1, 1)
    h = act(d1["g"], dt)
    yb, sb = run_resid(c, x, h, 2, sc, sh)
    ya, sa = run_resid(c, x[one].contiguous(), h[one].contiguous(), 2, sc[one].contiguous(), sh[one].contiguous(), Bn=1)
    same(yb[one], ya)
    same(sb[one], sa)
    for mode, d in ((0, d0), (1, d1)):
        s_, t_ = _sc_sh(d, mode)
        s1, t1 = (None, None) if s_ is None else (s_[one].contiguous(), t_[one].contiguous())
        g, u, coef = act(d["g"], dt), act(d["u"], dt), dev32(d["coef"].float())
        g1, u1, c1 = g[one].contiguous(), u[one].contiguous(), coef[one].contiguous()
        same(run_bwd_stats(c, mode, g, u, s_, t_)[one], run_bwd_stats(c, mode, g1, u1, s1, t1, Bn=1))
        if mode == 0:
            ob, sb, _ = run_bwd_apply(c, 0, g, u, coef, want_sums=True)
            oa, sa, _ = run_bwd_apply(c, 0, g1, u1, c1, want_sums=True, Bn=1)
            same(ob[one], oa)
            same(sb[one], sa)
        else:
            gy, nu = act(d["gy"], dt), act(d["nu"], dt)
            ob, _, nb = run_bwd_apply(c, 1, g, u, coef, s_, t_, gy, None, nu, want_nstats=True)
            oa, _, na = run_bwd_apply(c, 1, g1, u1, c1, s1, t1, gy[one].contiguous(), None, nu[one].contiguous(), want_nstats=True, Bn=1)
            same(ob[one], oa)
            same(nb[one], na)


def test_non_temporal_path_equals_cached_path():
    """resid (mode 2, group statistics) and gn_bwd_apply mode 1 (with `extra` and the chained statistics) on a bf16 batch of 33 samples
    of 128 x 128 x 256 -- 264 MiB, past the 256 MiB above which the kernels use non-temporal loads and stores -- against the same
    samples in three batches of 11: same bits.  The samples are one Gaussian base tensor rolled by a different offset each."""
    dt, C, H, W, Bn, sub = G.BF16, 256, 128, 128, 33, 11
    c = R.case(dt, C, H, W, "nt")
    HW = H * W
    assert Bn * HW * C * 2 > R.NT_BYTES >= sub * HW * C * 2
    lib = load_lib()
    geo = R.geometry(dt, C, H, W)
    base = {k: synth_dev(f"nt.{k}", HW * C) for k in ("x", "h", "gy", "ex", "nu")}

    def batch(k, first, n):
        return torch.stack([torch.roll(base[k], 4099 * (first + i)) for i in range(n)]).view(n, HW, C).contiguous()

    gamma, _ = R.gamma_beta("nt", C)
    scale = dev32((0.5 + R.gauss("nt.s", (Bn, C)).abs()).float())
    shift = dev32((0.2 * R.gauss("nt.t", (Bn, C))).float())
    coef = dev32((0.5 * R.gauss("nt.c", (Bn, 3, C))).float())

    def run(first, n):
        x, h, gy, ex, nu = (batch(k, first, n) for k in ("x", "h", "gy", "ex", "nu"))
        sc, sh, cf = (t[first:first + n].contiguous() for t in (scale, shift, coef))
        y = torch.full((n, HW, C), NAN, dtype=torch.bfloat16, device=G.dev())
        st = torch.full((n, geo["nparts"], R.SLAB), NAN, device=G.dev())
        _lib.check(lib.ddimx_resid_ex(dt, C, _lib.ptr(x), _lib.ptr(h), 2, _lib.ptr(sc), _lib.ptr(sh), None, 0, None, None, 1.0, R.EPS,
                                      _lib.ptr(y), _lib.ptr(st), 1, n, H, W, _lib.stream()))
        out = torch.full((n, HW, C), NAN, dtype=torch.bfloat16, device=G.dev())
        nst = torch.full((n, geo["nparts"], C, 2), NAN, device=G.dev())
        _lib.check(lib.ddimx_gn_bwd_apply(dt, 1, _lib.ptr(h), _lib.ptr(x), _lib.ptr(gy), _lib.ptr(ex), _lib.ptr(cf), _lib.ptr(sc), _lib.ptr(sh),
                                          _lib.ptr(out), None, _lib.ptr(nu), _lib.ptr(nst), n, H, W, C, _lib.stream()))
        torch.cuda.synchronize()
        return y, st, out, nst

    big = run(0, Bn)
    for t in big:
        assert bool(torch.isfinite(t).all())
    for first in range(0, Bn, sub):
        small = run(first, sub)
        for a, b, what in zip(big, small, ("resid y", "resid statistics", "apply dx", "apply chained statistics")):
            same(a[first:first + sub], b, f"{what}: samples {first} .. {first + sub - 1} differ between the two paths")


def synth_dev(tag, n):
    """n Gaussian bf16 values on the device."""
    from ddim_audio_amd import synth
    return synth.gaussian(tag, (n,)).to(G.dev(), torch.bfloat16)


# ---- the data-gradient conv's statistics epilogue ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("bwd_mode", [1, 2])
@pytest.mark.parametrize("C,H,W", [(32, 16, 32), (128, 16, 24)])
def test_dgrad_conv_statistics_epilogue(C, H, W, bwd_mode, dt):
    """One data-gradient 3x3 conv as ddimx_resblock_bwd builds it, with ConvCfg::BWD's epilogue: its (P, Q) slabs, summed over the
    slabs in fp64, against the fp64 sums over the dg it stored and the same aux -- bwd_mode 1: P = sum dg, Q = sum dg SiLU(aux);
    2: g' = dg SiLU'(s aux + t), P = sum g', Q = sum g' aux -- within (HW + SILU_OPS) * 2^-24 * sum |terms| (HW: no chain of the
    conv's partition is longer than a sample), and against gn_bwd_stats over the same two tensors within the two bounds added (the
    partitions differ, so the bits do).  Slabs past the count the conv reports stay NaN.
    Measured on MI355X: at most 1.1e-3 of the bound."""
    lib = load_lib()
    c = R.case(dt, C, H, W, "dgrad")
    HW = H * W
    geo = R.geometry(dt, C, H, W)
    tag = f"dgrad.{C}.{bwd_mode}"
    du = R.rnd(R.gauss(tag + ".du", (R.B, HW, C)), dt)
    aux = R.rnd(R.gauss(tag + ".aux", (R.B, HW, C)) + 0.3, dt)
    w = (R.gauss(tag + ".w", (C, C, 3, 3)) / (3.0 * C ** 0.5)).float()
    gamma, beta = R.gamma_beta(tag, C)
    scale, shift, _, _ = (t.float().double() for t in R.group_norm_fold(aux, gamma, beta))
    wd = G.pack_conv_dgrad(w, dt)
    dud, auxd, sd, td = act(du, dt), act(aux, dt), dev32(scale), dev32(shift)
    dg = Out(R.B * HW * C, R.tdt(dt))
    st = Out(R.B * geo["nparts"] * C * 2)
    npc = ctypes.c_int(-1)
    _lib.check(lib.ddimx_conv3x3_dgrad_stats(dt, C, _lib.ptr(dud), _lib.ptr(wd), _lib.ptr(auxd), _lib.ptr(sd) if bwd_mode == 2 else None,
                                             _lib.ptr(td) if bwd_mode == 2 else None, bwd_mode, dg.ptr, st.ptr, ctypes.byref(npc), R.B, H, W,
                                             _lib.stream()))
    torch.cuda.synchronize()
    nparts = npc.value
    assert 0 < nparts <= geo["nparts"], "the block takes these statistics from the conv at this shape"
    slabs = st.read("conv statistics", used=R.B * nparts * C * 2).view(R.B, nparts, C, 2)
    dgv = dg.read("dg").view(R.B, HW, C)
    assert bool(torch.isfinite(dgv).all()) and float(dgv.float().std()) > 0.1
    mode = bwd_mode - 1
    s_, t_ = (scale, shift) if mode else (None, None)
    want = R.bwd_stats(dgv.double(), aux, mode, HW, s_, t_)[:, 0]
    ab = R.bwd_abs_slabs(dgv.double(), aux, mode, HW, s_, t_)[:, 0]
    got = slabs.double().sum(1)
    worst = R.gate_sum(got, want, ab, HW + R.SILU_OPS, f"conv epilogue bwd_mode {bwd_mode}")
    alone = run_bwd_stats(c, mode, dev(dgv, dgv.dtype), auxd, sd if mode else None, td if mode else None).double().sum(1)
    R.gate_sum(got, alone, ab, HW + R.chain(geo) + 2 * R.SILU_OPS, "conv epilogue against gn_bwd_stats")
    report(f"dgrad epilogue C={C} bwd_mode={bwd_mode} dt={dt}", worst, "of the summation bound")


# ---- conv_in's group-format statistics --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c0", [32, 64])
def test_conv_in_group_statistics(c0, dt):
    """The group-format slabs of conv_in (the first GroupNorm input of the inference walk) at 30 x 40 -- two parts of 1024 pixels, the
    second ragged -- on dyadic operands small enough that every sum of y and y^2 over a sample's group is below 2^24 grid units (checked
    on the data): the slabs equal the channel-format slabs of ddimx_conv_in_fwd folded to the groups bit for bit, both equal fp64, the
    16 padding floats are zero and y is the same."""
    lib = load_lib()
    Bn, cin, H, W = R.B, 2, 30, 40
    tag = f"cing.{c0}.{dt}"
    x = X.dyadic(tag + ".x", (Bn, cin, H, W), 4, 2)
    w = X.dyadic(tag + ".w", (c0, cin, 3, 3), 2, 2)
    bias = X.dyadic(tag + ".b", (c0,), 16, 4)
    exact = X.conv3(x.permute(0, 2, 3, 1).contiguous(), w, bias).reshape(Bn, H * W, c0)
    assert torch.equal(R.rnd(exact, dt), exact), "y must be exact in the output dtype"
    tot = R.fold_groups(torch.stack([exact.abs().sum(1), (exact * exact).sum(1)], -1))
    assert float(tot[..., 0].max()) * 16 < 2 ** 24 and float(tot[..., 1].max()) * 256 < 2 ** 24
    nf = int(lib.ddimx_conv_in_stats_floats(Bn, c0, H, W))
    nparts = nf // (Bn * c0 * 2)
    assert nparts == 2
    xg, wg, bg = dev32(x), dev32(w), dev32(bias)
    y0, y1 = Out(Bn * H * W * c0, R.tdt(dt)), Out(Bn * H * W * c0, R.tdt(dt))
    s0, s1 = Out(nf), Out(Bn * nparts * R.SLAB)
    _lib.check(lib.ddimx_conv_in_fwd(dt, _lib.ptr(xg), _lib.ptr(wg), _lib.ptr(bg), y0.ptr, s0.ptr, Bn, cin, c0, H, W, _lib.stream()))
    _lib.check(lib.ddimx_conv_in_fwd_groups(dt, _lib.ptr(xg), _lib.ptr(wg), _lib.ptr(bg), y1.ptr, s1.ptr, Bn, cin, c0, H, W, _lib.stream()))
    torch.cuda.synchronize()
    ya, yb = y0.read("y"), y1.read("y")
    same(ya, yb)
    assert torch.equal(ya.double().view(Bn, H * W, c0), exact)
    chan = s0.read("channel slabs").view(Bn, nparts, c0, 2).double()
    want = R.chan_stats(exact, 1024)
    assert torch.equal(chan, want)
    assert torch.equal(s1.read("group slabs").view(Bn, nparts, R.SLAB).double(), R.group_slabs(want))
