"""Exact-operand checking of the convolution kernels (tests/test_gpu_exact.py, tests/test_exact_cpu.py).

Operands are small integers times a power of two, sized from the case's K (terms per output) so that every partial sum any kernel
can form is a multiple of the product grid and below 2^24 of it: any fp32 summation order then gives the exact sum.  The
reference is fp64 on the same operands, and two criteria replace the sigma gates:

* E (exact), linear outputs: a bf16 output equals RNE(exact value) (the kernels convert with v_cvt_pk_bf16_f32); an fp32 output
  equals the exact value bit for bit.
* S (SiLU), where silu_f (approximate exp2 / rcp) enters: within 1 output ulp (+ a summation bound where the SiLU feeds a sum), and
  exactly RNE where the fp64 value is farther than 2^-18 (relative) from a bf16 rounding midpoint.

No HIP here: the plan helpers call the library's host-only ddimx_debug_* exports, the rest is torch on any device.
"""
import ctypes
import zlib

import torch
import torch.nn.functional as F

from ddim_audio_amd import _lib

F32, BF16 = _lib.DDIMX_F32, _lib.DDIMX_BF16
CONV3, DOWN4, UP4 = 0, 1, 2
RING, WREG, PIPE = _lib.DDIMX_FAMILY_RING, _lib.DDIMX_FAMILY_WREG, _lib.DDIMX_FAMILY_PIPE
FAMILY = {RING: "ring", WREG: "wreg", PIPE: "pipe"}
XF_NONE, XF_AFFINE, XF_AFFINE_SILU, XF_SILU_AFFINE = 0, 1, 2, 3
# ddimx_debug_conv_plan flags (include/ddimx.h DDIMX_PLAN_*)
P_WFRAG, P_SKIP, P_STATS, P_GROUPS = _lib.DDIMX_PLAN_WFRAG, _lib.DDIMX_PLAN_SKIP, _lib.DDIMX_PLAN_STATS, _lib.DDIMX_PLAN_GROUPS
P_BATCH, P_BWD = _lib.DDIMX_PLAN_BATCH, _lib.DDIMX_PLAN_BWD


def P_XF(xf):
    return xf << 8


def P_ACT(act):
    return act << 12


def P_PREF(p):
    return p << 16


REDUCE = {0: "ks4", 1: "ks16", 2: "quad"}
MID_REL = 2.0 ** -18  # S: elements this close (relative) to a bf16 rounding midpoint may round either way


# ---- launch plans (the library's own conv_plan / wgrad_plan / GroupNorm rule, host only) -------------------------------------------
def conv_plan(dt, mode, cin, cout, B, H, W, flags):
    out = (ctypes.c_int * 12)()
    _lib.check(_lib.load().ddimx_debug_conv_plan(dt, mode, cin, cout, B, H, W, flags, out))
    keys = ("family", "var", "tiles_x", "tiles_y", "tiles_per_wg", "wgs_per_sample", "rounds", "th", "tw", "nthreads", "Hv", "Wv")
    p = dict(zip(keys, list(out)))
    tiles = p["tiles_x"] * p["tiles_y"]
    p["ragged_h"], p["ragged_w"] = p["Hv"] % p["th"] != 0, p["Wv"] % p["tw"] != 0
    p["ragged"] = p["ragged_h"] or p["ragged_w"]
    p["multi"] = p["tiles_per_wg"] > 1
    p["short_last"] = tiles % p["tiles_per_wg"] != 0
    return p


def wgrad_plan(dt, mode, ci, co, B, Hd, Wd):
    out = (ctypes.c_int * 8)()
    _lib.check(_lib.load().ddimx_debug_wgrad_plan(dt, mode, ci, co, B, Hd, Wd, out))
    p = dict(zip(("tiles_x", "tiles_y", "nsplit", "per", "reduce", "th", "tw", "ntaps"), list(out)))
    p["reduce"] = REDUCE[p["reduce"]]
    return p


REDUCE_KS = {"ks4": 4, "ks16": 16, "quad": 16}  # threads that share one output (wgrad_reduce_kernel<KS>, wgrad_reduce4_kernel)


def wgrad_ranges(p, B):
    """[(first tile, end tile)] of every workgroup of wgrad_mfma_kernel under plan p, tiles numbered sample-major."""
    total = B * p["tiles_x"] * p["tiles_y"]
    return [(t, min(t + p["per"], total)) for t in range(0, total, p["per"])]


def wgrad_key(dt, mode, ci, co, B, Hd, Wd, xf):
    """(kernel key, reduce key) of one weight-gradient launch, from the library's wgrad_plan alone.

    kernel key: (mode, ci, co, dt, xf, ragged_h, ragged_w, multi, crossing, short_last) -- the template instance, the runtime branch
    of its input transform, tiles cut by the image's lower / right edge, more than one tile per workgroup, some workgroup whose tile
    range runs from one sample into the next (it reloads the GroupNorm scale / shift), a last workgroup with fewer tiles.
    reduce key: (kind, unrolled, tail, disagree) -- the reduce kernel, the most 8-deep unrolled iterations any thread runs (0, 1,
    2 = two or more), whether any thread runs the tail loop, whether the threads that share an output run different numbers of
    unrolled iterations (thread q sums the splits q, q + KS, ...)."""
    p = wgrad_plan(dt, mode, ci, co, B, Hd, Wd)
    ts = p["tiles_x"] * p["tiles_y"]
    ranges = wgrad_ranges(p, B)
    assert len(ranges) == p["nsplit"], (p, B)
    crossing = any(t0 // ts != (t1 - 1) // ts for t0, t1 in ranges)
    short_last = ranges[-1][1] - ranges[-1][0] != p["per"]
    kernel = (mode, ci, co, dt, xf, Hd % p["th"] != 0, Wd % p["tw"] != 0, p["per"] > 1, crossing, short_last)
    ks, ns = REDUCE_KS[p["reduce"]], p["nsplit"]
    unrolled = [max(0, -(-(ns - q - 7 * ks) // (8 * ks))) for q in range(ks)]
    tail = [max(0, -(-(ns - q - 8 * ks * u) // ks)) for q, u in enumerate(unrolled)]
    reduce = (p["reduce"], min(max(unrolled), 2), any(tail), len(set(unrolled)) > 1)
    return kernel, reduce


EDGE_IN, EDGE_OUT, EDGE_OUT_BWD_DATA = _lib.DDIMX_EDGE_CONV_IN, _lib.DDIMX_EDGE_CONV_OUT, _lib.DDIMX_EDGE_CONV_OUT_BWD_DATA
EDGE_IN_BWD_DATA, EDGE_WGRAD = _lib.DDIMX_EDGE_CONV_IN_BWD_DATA, _lib.DDIMX_EDGE_WGRAD
EDGE_KEYS = ("variant", "grid_x", "grid_y", "threads", "lds", "trips", "tiles_x", "tiles_y", "partial_blocks", "reduce_blocks",
             "reduce_unrolled", "reduce_tail")


def edge_plan(op, dt, B, C0, Cio, H, W, groups=0):
    """Plan of one edge-conv launcher (ddimx_debug_edge_plan); raises RuntimeError with the launcher's reason where it refuses."""
    out = (ctypes.c_int * 12)()
    _lib.check(_lib.load().ddimx_debug_edge_plan(op, dt, B, C0, Cio, H, W, groups, out))
    return dict(zip(EDGE_KEYS, list(out)))


def gn_plan(dt, C, B, H, W, x_nparts):
    out = (ctypes.c_int * 9)()
    _lib.check(_lib.load().ddimx_debug_gn_plan(dt, C, B, H, W, x_nparts, out))
    v = list(out)
    return {"conv0": bool(v[1]), "conv1": bool(v[4]), "resid": bool(v[7]), "conv0_np": v[0], "conv1_np": v[3], "resid_np": v[6],
            "y_np": v[8]}


# ---- dyadic operands -----------------------------------------------------------------------------------------------------------
def dyadic(tag, shape, k, p, nonzero=False):
    """Integers uniform in [-k, k] (or without 0) times 2^-p, fp64, deterministic in `tag`."""
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    v = torch.randint(-k, k + 1, shape, generator=g, dtype=torch.int64)
    if nonzero:
        v = torch.where(v == 0, torch.ones_like(v), v)
    return v.double() * 2.0 ** -p


def scales(tag, shape):
    """GroupNorm scale on {0.5, 1, 1.5, 2}: x * s + h stays exact in bf16 for x on k/8, |k| <= 8 and h on k/16, |h| <= 1."""
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    return (torch.randint(1, 5, shape, generator=g).double() * 0.5)


def budget_bits(K, amax, pa, wmax, pw, extra=0.0):
    """log2 of the largest |partial sum| in units of the product grid 2^-(pa+pw): < 24 makes every fp32 summation order exact."""
    import math
    return math.log2((K * amax * wmax + extra) * 2.0 ** (pa + pw))


# ---- rounding ------------------------------------------------------------------------------------------------------------------
def rne(x, bits=8):
    """Round fp64 to `bits` significant bits, nearest-even (bits=8: bf16, 24: fp32); exact in fp64, no overflow handling."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 2.0 ** bits), e - bits)


def ulp(x, bits=8):
    """Spacing of the `bits`-significant-bit grid at |x| (bf16: 8)."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -100))
    return torch.ldexp(torch.ones_like(x), e - bits)


def near_midpoint(x, bits=8, rel=MID_REL):
    """True where x lies within rel * |x| of a rounding midpoint of the `bits` grid."""
    u = ulp(x, bits)
    r = torch.remainder(x, u) - u / 2
    return r.abs() <= rel * x.abs()


def silu64(x):
    return x * torch.sigmoid(x)


def xf64(a, scale, shift, xf):
    """The input transform of the conv / wgrad prologues on NHWC a, per-(sample, channel) scale / shift [B][C], in fp64."""
    s, h = scale[:, None, None, :], shift[:, None, None, :]
    if xf == XF_NONE:
        return a
    if xf == XF_AFFINE:
        return a * s + h
    if xf == XF_AFFINE_SILU:
        return silu64(a * s + h)
    return silu64(a) * s + h


# ---- fp64 references, NHWC (tap loops of dense products: exact in fp64 on these operands on any device) ------------------------
def conv3(x, w, bias=None, add=None):
    """x [B][H][W][Ci], w [Co][Ci][3][3] -> [B][H][W][Co] (+ bias [Co] + add [B][Co])."""
    B, H, W, _ = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros(B, H, W, w.shape[0], dtype=x.dtype, device=x.device)
    for kh in range(3):
        for kw in range(3):
            out += (xp[:, kh:kh + H, kw:kw + W, :].reshape(-1, x.shape[-1]) @ w[:, :, kh, kw].T).view(out.shape)  # one 2-D product
    if bias is not None:
        out += bias
    if add is not None:
        out += add[:, None, None, :]
    return out


def down4(x, w, bias=None):
    """Conv2d(k4, s2, p1): x [B][H][W][Ci], w [Co][Ci][4][4] -> [B][H/2][W/2][Co]."""
    B, H, W, _ = x.shape
    Ho, Wo = H // 2, W // 2
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros(B, Ho, Wo, w.shape[0], dtype=x.dtype, device=x.device)
    for kh in range(4):
        for kw in range(4):
            out += (xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :].reshape(-1, x.shape[-1]) @ w[:, :, kh, kw].T).view(out.shape)
    return out if bias is None else out + bias


def up4(x, w, bias=None, skip=None):
    """ConvTranspose2d(k4, s2, p1): x [B][H][W][Ci], w [Ci][Co][4][4] -> [B][2H][2W][Co] (+ skip)."""
    B, H, W, _ = x.shape
    full = torch.zeros(B, 2 * H + 2, 2 * W + 2, w.shape[1], dtype=x.dtype, device=x.device)
    for kh in range(4):
        for kw in range(4):
            full[:, kh:kh + 2 * H:2, kw:kw + 2 * W:2, :] += (x.reshape(-1, x.shape[-1]) @ w[:, :, kh, kw]).view(B, H, W, -1)
    out = full[:, 1:2 * H + 1, 1:2 * W + 1, :]
    if bias is not None:
        out = out + bias
    return out if skip is None else out + skip


def wgrad3(a, du):
    """dW [Co][Ci][3][3] of a 3x3 conv: a [B][H][W][Ci] (after the input transform), du [B][H][W][Co]."""
    B, H, W, ci = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    dw = torch.zeros(du.shape[-1], ci, 3, 3, dtype=a.dtype, device=a.device)
    d2 = du.reshape(-1, du.shape[-1])
    for kh in range(3):
        for kw in range(3):
            dw[:, :, kh, kw] = d2.T @ ap[:, kh:kh + H, kw:kw + W, :].reshape(-1, ci)
    return dw


def wgrad_down4(x, dy):
    """dW [Co][Ci][4][4] of Conv2d(k4, s2, p1): x [B][H][W][Ci], dy [B][H/2][W/2][Co]."""
    B, Ho, Wo, co = dy.shape
    ci = x.shape[-1]
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    dw = torch.zeros(co, ci, 4, 4, dtype=x.dtype, device=x.device)
    d2 = dy.reshape(-1, co)
    for kh in range(4):
        for kw in range(4):
            dw[:, :, kh, kw] = d2.T @ xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :].reshape(-1, ci)
    return dw


# ---- criteria ------------------------------------------------------------------------------------------------------------------
def locate(idx, shape, plan=None, layout="nhwc"):
    """(n, c, h, w) of flat index idx in an NHWC / NCHW tensor, with its tile and workgroup under `plan`."""
    if layout == "nhwc":
        B, H, W, C = shape
        n, r = divmod(idx, H * W * C)
        h, r = divmod(r, W * C)
        w, c = divmod(r, C)
    else:
        B, C, H, W = shape
        n, r = divmod(idx, C * H * W)
        c, r = divmod(r, H * W)
        h, w = divmod(r, W)
    s = f"(n={n}, c={c}, h={h}, w={w})"
    if plan is not None:
        ty, tx = h // plan["th"], w // plan["tw"]
        t = ty * plan["tiles_x"] + tx
        s += f" tile ({ty}, {tx}) of {plan['tiles_y']}x{plan['tiles_x']}, workgroup {t // plan['tiles_per_wg']} of sample {n}"
    return s


def mismatches(got, exact, dt, approx=False, delta=None):
    """Boolean mask of the elements that violate the criterion.  got: the kernel's output (any float dtype); exact: fp64 value of
    the operation (for approx=True: its argument's fp64 SiLU already applied); dt: the output's storage type; delta: fp64 bound of
    the kernel's inexact summation (tensor or float), or None."""
    g = got.detach().double().cpu()
    exact = exact.double().cpu()
    if delta is not None and torch.is_tensor(delta):
        delta = delta.double().cpu()
    bits = 8 if dt == BF16 else 24
    bad = ~torch.isfinite(g)
    if not approx and delta is None:
        want = rne(exact, bits)
        if dt == F32:
            assert torch.equal(want, exact), "fp32 output whose exact value is not an fp32 number: the case's ranges are wrong"
        return bad | (g != want)
    d = (g - exact).abs()
    # fp32 outputs of silu_f: exp2's argument carries the fp32 log2(e), so the relative error grows with |x| (4 ulp + 2^-18 covers
    # |x| <= 20; a missing term is orders of magnitude larger)
    tol = ulp(exact, bits) if dt == BF16 else 4.0 * ulp(exact, bits) + 2.0 ** -18 * exact.abs()
    if delta is not None:
        tol = tol + delta
    bad |= d > tol
    if delta is None and dt == BF16:
        sure = ~near_midpoint(exact, bits)
        bad |= sure & (g != rne(exact, bits))
    return bad


def check(got, exact, dt, what, plan=None, layout="nhwc", approx=False, delta=None):
    bad = mismatches(got, exact, dt, approx, delta)
    nbad = int(bad.sum())
    got = got.detach().cpu()
    if nbad:
        i = int(bad.reshape(-1).nonzero()[0])
        g, e = float(got.reshape(-1)[i]), float(exact.reshape(-1)[i])
        raise AssertionError(f"{what}: {nbad} of {bad.numel()} elements violate {'S' if approx or delta is not None else 'E'}; first "
                             f"{locate(i, tuple(got.shape), plan, layout)}: got {g!r}, exact {e!r}")


def sum_bound(v, m):
    """Rigorous bound of an fp32 sum of at most m terms per partial (then summed in fp64) of the values v, per channel (last dim)."""
    return m * 2.0 ** -24 * v.abs().reshape(-1, v.shape[-1]).sum(0)
