"""fp64 references and case tables of the GroupNorm kernel family, one by one (test infrastructure; no GPU).

tests/test_gn_kernels_cpu.py checks this file against torch (F.group_norm, autograd) and against itself evaluated in fp32;
tests/test_gpu_gn_kernels.py parametrizes over the tables below and compares the kernels behind ddimx_tensor_stats /
ddimx_gn_finalize / ddimx_gn_finalize_groups / ddimx_resid_ex / ddimx_gn_bwd_stats / ddimx_gn_bwd_finalize / ddimx_gn_bwd_apply /
ddimx_partsum[_multi] / ddimx_colsum_multi / ddimx_conv3x3_dgrad_stats with these functions.

Activations are [B][HW][C] (NHWC with the pixels flattened).  Every reference takes ``dt`` (default fp64): the CPU tests run the
same code in fp32 to show that each gate is one a sound fp32 implementation meets.

The element-wise passes (tensor_stats, resid, gn_bwd_stats, gn_bwd_apply) share one partition, ``geometry``: a block of `threads`
threads owns `rows` = threads / (C / EPB) pixels per iteration and `iters` iterations, so slab `p` of a sample covers the pixels
[p * rows * iters, (p + 1) * rows * iters).  A thread adds `iters` terms in fp32, the block then `rows` of those; the group
format adds up to ceil(GS / 4) + 2 more.  That is the longest fp32 accumulation chain, ``chain``.

Gates (tests/test_gpu_gn_kernels.py):

* exact -- sums of dyadic operands equal the fp64 sum bit for bit (``dyadic_x``: every partial sum is below 2^24 grid units);
* sum -- |got - want| <= n * 2^-24 * sum |terms| with n the number of fp32 roundings between the stored operands and the slab:
  ``chain`` for the accumulation, plus ``SILU_OPS`` where SiLU or SiLU' is formed on the way (see there);
* fp32 -- ``gpu_util.TOL[F32]`` (max 1e-4, rms 2e-5) in units of the std of the expected tensor; for rstd under a non-zero mean
  widened by 1 + mean^2 / var, the cancellation factor of Q / n - mean^2;
* bf16 -- against fp64 on the bf16-rounded inputs: |got - want| <= 2^-8 |want| + TOL[F32].mx * std.
"""
import math

import torch

import exact_util as X
import gpu_util as G
from ddim_audio_amd import _lib, synth
from fnet_kernel_ref import gate  # the fp32 gate with its unit made explicit

GROUPS = 8
EPS = 1e-6
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))  # the kernels take eps as a float
SLAB = 32             # floats of one group-format slab: [8][2] then 16 zeros
FUSE_MAX_PARTS = 256  # above this resid refuses to finish the GroupNorm itself
CHANNELS = (32, 64, 96, 128, 192, 256)
DTYPES = (G.F32, G.BF16)
B = 3
# fp32 roundings inside one SiLU(v) = v * rcp(1 + exp2(-log2e * v)) or SiLU'(v) term for |v| <= 12: the product with log2e (its
# relative rounding 2^-24 becomes a relative error |v| log2e ln2 2^-24 = |v| 2^-24 of the exponential: 12), exp2, the add, rcp and
# two to four products / fmas around them (8 covers SiLU' and the affine in front of it)
SILU_ARG_MAX = 12.0
SILU_OPS = 20
NT_BYTES = 256 << 20  # tensors above this take the non-temporal loads and stores


def epb(dt):
    return 8 if dt == G.BF16 else 4


def tdt(dt):
    return G.TORCH_DT[dt]


def rnd(t, dt):
    """t rounded to the activation dtype, as fp64."""
    return t.to(tdt(dt)).double()


def geometry(dt, C, H, W):
    """The partition of the element-wise passes from the library's own helpers."""
    lib = _lib.load()
    threads, iters = lib.ddimx_resid_threads(dt, C), lib.ddimx_resid_iters(dt, C, H, W)
    cpp = C // epb(dt)
    rows = threads // cpp
    return dict(threads=threads, iters=iters, rows=rows, rpp=rows * iters, nparts=X.gn_plan(dt, C, 1, H, W, 1)["y_np"], cpp=cpp,
                GS=C // GROUPS, HW=H * W)


def chain(geo, groups=False):
    return geo["iters"] + geo["rows"] + ((geo["GS"] + 3) // 4 + 2 if groups else 0)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def case(dt, C, H, W, name):
    return dict(dt=dt, C=C, H=H, W=W, id=f"{name}-C{C}-{'bf16' if dt == G.BF16 else 'f32'}")


# 3x5: one ragged part (C <= 64; up to four parts of few rows above), most threads idle.  7x11: iters = 1, several parts, the last one ragged.
SMALL = [case(dt, C, h, w, n) for dt in DTYPES for C in CHANNELS for h, w, n in ((3, 5, "tiny"), (7, 11, "ragged"))]
ROUNDS65 = case(G.F32, 32, 104, 100, "rounds65")   # iters = 5 (tails of the 4- and 2-wide unrolls), 65 slabs
ITERS16 = case(G.F32, 64, 128, 130, "iters16")     # iters = 16, 65 slabs
CASES = SMALL + [ROUNDS65, ITERS16]
# where only the partition matters (the reductions of slabs): one small case per block geometry and the two-round cases
GEOM_CASES = [c for c in SMALL if c["H"] == 7 and c["C"] in (32, 96, 256)] + [ROUNDS65, ITERS16]


def case_id(c):
    return c["id"]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def gauss(tag, shape):
    return synth.gaussian(tag, shape).double()


def dyadic_x(tag, shape):
    """k / 8, |k| <= 8: x and x^2 are multiples of 2^-6 below 1, so a sum of up to 2^18 squares is exact in fp32."""
    return X.dyadic(tag, shape, 8, 3)


def dyadic_budget_bits(n_terms):
    return math.log2(n_terms * 64.0)


def gamma_beta(tag, C):
    """gamma of order one with mixed signs and gamma[1] = 0; beta of order 0.2."""
    g = 1.0 + 0.3 * gauss(tag + ".gamma", (C,))
    g = g * torch.where(torch.arange(C) % 3 == 2, -1.0, 1.0).double()
    g[1] = 0.0
    return g.float().double(), (0.2 * gauss(tag + ".beta", (C,))).float().double()


def group_of(C):
    return torch.arange(C) // (C // GROUPS)


# ---- forward references ---------------------------------------------------------------------------------------------------------------
def part_sums(t, rpp, dt=torch.float64):
    """t [B][HW][C] -> [B][np][C]: sums over the pixels of each slab, accumulated in `dt`."""
    Bn, HW, C = t.shape
    npart = -(-HW // rpp)
    pad = torch.zeros(Bn, npart * rpp, C, dtype=dt)
    pad[:, :HW] = t.to(dt)
    return pad.view(Bn, npart, rpp, C).sum(2, dtype=dt)


def chan_stats(x, rpp, dt=torch.float64):
    """(sum, sumsq) slabs [B][np][C][2] of x [B][HW][C]."""
    x = x.to(dt)
    return torch.stack([part_sums(x, rpp, dt), part_sums(x * x, rpp, dt)], -1)


def fold_groups(st):
    """[..][C][2] -> [..][8][2]."""
    C = st.shape[-2]
    return st.reshape(*st.shape[:-2], GROUPS, C // GROUPS, 2).sum(-2)


def group_slabs(st):
    """channel slabs [B][np][C][2] -> group-format slabs [B][np][32]: [8][2], then zeros."""
    g = fold_groups(st).reshape(*st.shape[:2], 2 * GROUPS)
    return torch.cat([g, torch.zeros_like(g)], -1)


def gn_fold(S, Q, count, gamma, beta, eps=EPS32):
    """Group totals S, Q [B][8] -> (scale [B][C], shift [B][C], mean [B][8], rstd [B][8]); biased variance, beta nullable."""
    dt = S.dtype
    mean = S / count
    var = (Q / count - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=dt))
    grp = group_of(gamma.shape[0])
    scale = rstd[:, grp] * gamma.to(dt)
    shift = -mean[:, grp] * scale
    if beta is not None:
        shift = shift + beta.to(dt)
    return scale, shift, mean, rstd


def group_norm_fold(x, gamma, beta, eps=EPS32, dt=torch.float64):
    """The same from the tensor itself, x [B][HW][C]."""
    x = x.to(dt)
    st = fold_groups(torch.stack([x.sum(1), (x * x).sum(1)], -1))
    return gn_fold(st[..., 0], st[..., 1], float(x.shape[1] * (x.shape[2] // GROUPS)), gamma, beta, eps)


def silu(v):
    return v * torch.sigmoid(v)


def dsilu(v):
    s = torch.sigmoid(v)
    return s * (1.0 + v * (1.0 - s))


def resid(x, h, mode, scale=None, shift=None, dt=torch.float64):
    """mode 0: x + h * scale + shift; 1: x + h; 2: x + SiLU(h) * scale + shift.  scale / shift [B][C]."""
    x, h = x.to(dt), h.to(dt)
    if mode == 1:
        return x + h
    v = silu(h) if mode == 2 else h
    return x + v * scale.to(dt)[:, None, :] + shift.to(dt)[:, None, :]


# ---- backward references --------------------------------------------------------------------------------------------------------------
def bwd_terms(g, u, mode, scale=None, shift=None, dt=torch.float64):
    """(g', v): mode 0 (norm fed by SiLU(u)) g' = g, v = SiLU(u); mode 1 (norm followed by SiLU) g' = g SiLU'(scale u + shift), v = u."""
    g, u = g.to(dt), u.to(dt)
    if mode == 0:
        return g, silu(u)
    return g * dsilu(u * scale.to(dt)[:, None, :] + shift.to(dt)[:, None, :]), u


def bwd_abs_terms(g, u, mode, scale=None, shift=None):
    """What the sum gate of (P, Q) multiplies n 2^-24 with, per element: |g'| and |g' v| -- with SiLU'(a) = s + s a (1 - s) taken as
    s + |s a (1 - s)|: near a = -1.28 the two addends cancel, and the rounding of their sum is relative to them, not to the result."""
    g, u = g.double(), u.double()
    if mode == 0:
        return g.abs(), (g * silu(u)).abs()
    a = u * scale.double()[:, None, :] + shift.double()[:, None, :]
    s = torch.sigmoid(a)
    t = g.abs() * s * (1.0 + a.abs() * (1.0 - s))
    return t, t * u.abs()


def bwd_abs_slabs(g, u, mode, rpp, scale=None, shift=None):
    p, q = bwd_abs_terms(g, u, mode, scale, shift)
    return torch.stack([part_sums(p, rpp), part_sums(q, rpp)], -1)


def bwd_stats(g, u, mode, rpp, scale=None, shift=None, dt=torch.float64):
    """(P, Q) slabs [B][np][C][2]."""
    gp, v = bwd_terms(g, u, mode, scale, shift, dt)
    return torch.stack([part_sums(gp, rpp, dt), part_sums(gp * v, rpp, dt)], -1)


def bwd_coef(PQ, count, gamma, mean, rstd):
    """Totals PQ [B][C][2], mean / rstd [B][8] -> (coef [B][3][C] = ca, cb, cc; dgb [B][2][C] = per-sample dgamma, dbeta terms):
    S1 = sum_group gamma P, S2 = sum_group gamma rstd (Q - mean P), ca = gamma rstd, cb = -rstd^2 S2 / N,
    cc = -rstd S1 / N + mean rstd^2 S2 / N."""
    dt = PQ.dtype
    C = gamma.shape[0]
    grp = group_of(C)
    P, Q = PQ[..., 0], PQ[..., 1]
    m, r, gm = mean.to(dt)[:, grp], rstd.to(dt)[:, grp], gamma.to(dt)
    dg = r * (Q - m * P)
    fold = lambda t: t.reshape(-1, GROUPS, C // GROUPS).sum(-1)[:, grp]  # noqa: E731
    s1, s2 = fold(gm * P), fold(gm * dg)
    ca = gm * r
    cb = -r * r * s2 / count
    cc = -r * s1 / count + m * r * r * s2 / count
    return torch.stack([ca, cb, cc], 1), torch.stack([dg, P], 1)


def bwd_apply(g, u, mode, coef, scale=None, shift=None, gy=None, extra=None, dt=torch.float64):
    """mode 0: (ca g + cb SiLU(u) + cc) SiLU'(u); mode 1: gy + ca g' + cb u + cc (+ extra)."""
    gp, v = bwd_terms(g, u, mode, scale, shift, dt)
    ca, cb, cc = (coef.to(dt)[:, i, None, :] for i in range(3))
    if mode == 0:
        return (ca * gp + cb * v + cc) * dsilu(u.to(dt))
    out = gy.to(dt) + ca * gp + cb * v + cc
    return out if extra is None else out + extra.to(dt)


def projection_part(g, u, mode, coef, scale=None, shift=None):
    """The cb v + cc part of bwd_apply alone (times SiLU'(u) in mode 0)."""
    _, v = bwd_terms(g, u, mode, scale, shift)
    t = coef[:, 1, None, :] * v + coef[:, 2, None, :]
    return t * dsilu(u.double()) if mode == 0 else t


def bwd_inputs(c, mode):
    """The operands of one backward pass on case c, rounded to the case's dtype where they are activations (fp64 tensors):
    u (the saved tensor; mode 1: the block's input x, with a mean), gamma, beta, the norm's constants (mean, rstd as fp32 numbers,
    scale / shift likewise) and the upstream gradient g = a_c + b_c * vhat + 0.3 noise with a_c, b_c of order one and the sign of
    gamma_c, so that the group sums S1, S2 -- hence cb, cc -- are as large as ca g; gy / extra / nu for mode 1."""
    dt, C, HW = c["dt"], c["C"], c["H"] * c["W"]
    tag = f"gnb.{c['id']}.{mode}"
    u = gauss(tag + ".u", (B, HW, C)) * 1.5
    if mode == 1:
        u = u + 0.5
    u = rnd(u, dt)
    gamma, beta = gamma_beta(tag, C)
    v = silu(u) if mode == 0 else u
    scale, shift, mean, rstd = (t.float().double() for t in group_norm_fold(v, gamma, beta))
    grp = group_of(C)
    vhat = (v - mean[:, None, grp]) * rstd[:, None, grp]
    sgn = torch.where(gamma < 0, -1.0, 1.0).double()
    a = sgn * (0.75 + 0.25 * torch.from_numpy(synth.uniform_pm1(tag + ".a", C)).double())
    b = sgn * (0.75 + 0.25 * torch.from_numpy(synth.uniform_pm1(tag + ".b", C)).double())
    g = rnd(a + b * vhat + 0.3 * gauss(tag + ".n", (B, HW, C)), dt)
    d = dict(u=u, g=g, gamma=gamma, beta=beta, scale=scale, shift=shift, mean=mean, rstd=rstd, count=float(HW * (C // GROUPS)))
    if mode == 1:
        d["gy"] = rnd(0.5 * gauss(tag + ".gy", (B, HW, C)), dt)
        d["extra"] = rnd(0.5 * gauss(tag + ".ex", (B, HW, C)), dt)
        d["nu"] = rnd(1.5 * gauss(tag + ".nu", (B, HW, C)), dt)
    return d


def bwd_reference(d, mode, rpp):
    """fp64 (PQ slabs, coef, dgb, out) of the three passes chained: coef from the exact totals."""
    sc, sh = (d["scale"], d["shift"]) if mode == 1 else (None, None)
    PQ = bwd_stats(d["g"], d["u"], mode, rpp, sc, sh)
    coef, dgb = bwd_coef(PQ.sum(1), d["count"], d["gamma"], d["mean"], d["rstd"])
    return PQ, coef, dgb, bwd_apply(d["g"], d["u"], mode, coef, sc, sh, d.get("gy"))


# ---- gates ---------------------------------------------------------------------------------------------------------------------------
def gate_bf16(got, want, what, std=None):
    """|got - want| <= 2^-8 |want| + TOL[F32].mx * std: one bf16 ulp plus the fp32 slack of the value that was rounded."""
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    s = float(want.std()) if std is None else float(std)
    excess = (got - want).abs() - (2.0 ** -8 * want.abs() + G.TOL[G.F32]["mx"] * s)
    assert float(excess.max()) <= 0.0, f"{what}: {int((excess > 0).sum())} elements past the bf16 gate, worst by {float(excess.max()):.3e}"
    return float(((got - want).abs() / (2.0 ** -8 * want.abs() + G.TOL[G.F32]["mx"] * s)).max())


def gate_elementwise(got, want, dt, what, std=None):
    """The fp32 or the bf16 gate by the output's dtype; returns the worst error in the gate's units."""
    if dt == G.BF16:
        return gate_bf16(got, want, what, std)
    return gate(got, want, what, std=std)[0] / G.TOL[G.F32]["mx"]


def gate_sum(got, want, abs_terms, n, what):
    """|got - want| <= n 2^-24 sum |terms| element by element; returns the worst ratio to the bound."""
    got, want, bound = got.double(), want.double(), n * 2.0 ** -24 * abs_terms.double()
    assert got.shape == want.shape == bound.shape, (what, got.shape, want.shape, bound.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite sums"
    d = (got - want).abs()
    bad = d > bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} sums past n 2^-24 sum|terms| (n = {n}), worst ratio " \
                                f"{float((d / bound.clamp_min(1e-300)).max()):.3f}"
    return float((d / bound.clamp_min(1e-300)).max())


def gate_stats_of_norm(scale, shift, mean, rstd, want, what):
    """The four outputs of a finalisation against (scale, shift, mean, rstd) fp64: scale and shift at the fp32 gate in units of their
    own std; mean in units of the group's std (1 / rstd); rstd relative, widened by 1 + mean^2 / var."""
    ws, wh, wm, wr = want
    e = [gate(scale, ws, what + " scale")[0], gate(shift, wh, what + " shift")[0]]
    if mean is not None:
        e.append(gate((mean.double() - wm) * wr, torch.zeros_like(wm), what + " mean", std=1.0)[0])
        var = 1.0 / (wr * wr)  # (+ eps: what the kernel inverts)
        widen = 1.0 + wm * wm / var
        e.append(gate((rstd.double() / wr - 1.0) / widen, torch.zeros_like(wr), what + " rstd", std=1.0)[0])
    return max(e)


# ---- finalisation cases -----------------------------------------------------------------------------------------------------------------
FINALIZE_NPARTS = (1, 5, 256, 1025)
FINALIZE_REPS = (1, 2)  # Cs / C
GROUPS_NTHREADS = (64, 192, 256, 1024)


def groups_np(nthreads):
    """One partial; seven; exactly one round (eight partials for each of nthreads / 8 slices); one more; the fused limit; past it."""
    return sorted({1, 7, nthreads, nthreads + 1, FUSE_MAX_PARTS, 600})


def synthetic_slabs(tag, nparts, Cs, m=4, offset=0.0):
    """Channel slabs [B][nparts][Cs][2] as fp32 numbers (returned as fp64), each the (sum, sumsq) of m Gaussian values; count per
    (sample, group) is then nparts * m * Cs / 8."""
    v = gauss(tag, (B, nparts, m, Cs)) + offset
    return torch.stack([v.sum(2), (v * v).sum(2)], -1).float().double()


# ---- reductions -----------------------------------------------------------------------------------------------------------------------
MULTI_C = (32, 200)
MULTI_B = (1, 3, 19)
MULTI_NPARTS = (1, 65)


def partsum(src, src_step=1):
    """src [B][nparts][C * src_step] -> float32(fp64 sums over the parts of every src_step-th float) [B][C]."""
    return src.double()[..., ::src_step].sum(1).float()


def colsum(src, C, off=0):
    """src [B][stride] -> float32(fp64 column sums of columns off .. off + C - 1)."""
    return src.double()[:, off:off + C].sum(0).float()


# ---- numerics -------------------------------------------------------------------------------------------------------------------------
MEAN_OVER_STD = (0, 4, 32)
CONST_GROUP, CONST_VALUE = 3, 1.5


def numerics_x(tag, dt, C, HW, ratio):
    """x [B][HW][C] of unit std with group means +-ratio (alternating by group) and group 3 constant at 1.5 (exact in bf16: its
    variance is exactly zero and rstd = 1 / sqrt(eps)), rounded to dt."""
    grp = group_of(C)
    x = gauss(tag, (B, HW, C)) + ratio * torch.where(grp % 2 == 0, 1.0, -1.0).double()
    x[:, :, grp == CONST_GROUP] = CONST_VALUE
    return rnd(x, dt)
