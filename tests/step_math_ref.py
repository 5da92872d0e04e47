"""The fp32 mirror of ``csrc/step_math.h`` (test infrastructure; CPU only, the library is not imported): the only Python copy
of the sampler update arithmetic.  Function for function under the header's names, on numpy arrays, one numpy operation per
rounding and in the header's order, so the results are the bits every update kernel must give.  The fused multiply-add is exact
(``fma32``).  Operands are taken as fp32 whatever they arrive as; NaN and inf are values here as they are on the device (no
numpy warning), because the kernel tests poison what a kernel must not read."""
import numpy as np

F32 = np.float32
_quiet = np.errstate(all="ignore")


def _f(*vs):
    return [np.asarray(v, dtype=F32) for v in vs]


@_quiet
def fma32(a, b, c):
    """An exact fp32 fused multiply-add, element-wise: rn32(a b + c).  The product of two fp32 numbers is exact in fp64, and
    s = rn64(product + c) rounded again to fp32 is the single rounding of the exact sum unless s lies exactly half way between two
    fp32 neighbours (the 29 bits fp32 drops are 1 0...0) while the exact sum does not: only those elements, and results below the
    normal fp32 range, where the half-way pattern sits elsewhere, go the slow way -- s is re-rounded TO ODD from the error term
    of the two-sum (which says whether the sum was exact and on which side of s it lies), and that value rounds to fp32 once
    (53 >= 24 + 2 bits)."""
    a, b, c = np.broadcast_arrays(*_f(a, b, c))
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    risky = np.flatnonzero(((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000).ravel() | (np.abs(s) < 2.0 ** -126).ravel())
    if risky.size:
        pr, cr, sr = p.ravel()[risky], c.ravel()[risky], s.ravel()[risky]
        bb = sr - pr
        err = (pr - (sr - bb)) + (cr - bb)  # two-sum: p + c = s + err exactly
        even = (sr.view(np.int64) & 1) == 0
        sr = np.where((err != 0) & even, np.nextafter(sr, np.where(err > 0, np.inf, -np.inf)), sr)
        s = s.copy().ravel()
        s[risky] = sr
        s = s.reshape(p.shape)
    return s.astype(F32)


@_quiet
def sub32(a, b):
    """``__fsub_rn``: rn32(a - b)."""
    a, b = _f(a, b)
    return a - b


# ---- the scalar operations ----------------------------------------------------------------------------------------------------------------
@_quiet
def ddim_x0(x, e, s1, s2):
    x, e, s1, s2 = _f(x, e, s1, s2)
    return fma32(e, -s1, x) / s2


@_quiet
def ddim_next(x0, e, s3, c2):
    x0, e, s3, c2 = _f(x0, e, s3, c2)
    return fma32(e, c2, x0 * s3)


@_quiet
def v_to_eps(x, v, s1, s2):
    x, v, s1, s2 = _f(x, v, s1, s2)
    return fma32(v, s2, x * s1)


def x0_scale(q, floor, ceil):
    """Comparisons only: a NaN q gives floor."""
    q, floor, ceil = _f(q, floor, ceil)
    s = np.where(q > floor, q, floor)
    return np.where(s < ceil, s, ceil)


@_quiet
def x0_clip(x0, s, r):
    x0, s, r = _f(x0, s, r)
    lo = np.where(x0 < -s, -s, x0)
    return np.where(lo > s, s, lo) * r


@_quiet
def x0_to_eps(x, e, x0, c, s1, s2):
    x, e, x0, c, s1, s2 = _f(x, e, x0, c, s1, s2)
    return np.where(np.ascontiguousarray(c).view(np.uint32) == np.ascontiguousarray(x0).view(np.uint32), e, fma32(c, -s2, x) / s1)


@_quiet
def inpaint_residual(x0, y, m):
    x0, y, m = _f(x0, y, m)
    return m * (x0 - y)


@_quiet
def inpaint_seed(r, m, k1):
    r, m, k1 = _f(r, m, k1)
    return k1 * (m * r)


@_quiet
def inpaint_guide(u, x0, y, m, d, k2, w):
    u, x0, y, m, d, k2, w = _f(u, x0, y, m, d, k2, w)
    q = m * (m * (x0 - y))
    return fma32(-w, fma32(k2, q, d), u)


@_quiet
def inpaint_replace(u, kv, m):
    u, kv, m = _f(u, kv, m)
    return np.where(m == 1, kv, np.where(m == 0, u, fma32(m, kv, (F32(1) - m) * u)))


@_quiet
def inpaint_known(x, y, cx, w0, use_x):
    x, y, cx, w0 = _f(x, y, cx, w0)
    k = w0 * y
    return fma32(cx, x, k) if use_x else k


# ---- one update on one coefficient row ----------------------------------------------------------------------------------------------------
def load_row(row):
    """``load_row`` / ``load_row3``: (s1, s2, s3, c2, c1, w1, w2, w3) as fp32 from a row of 6 columns (t .. c1: a DDIM row), 8
    (.. w2: a solver row) or 9 (.. w3: a corrector row); a column the row does not have is 0."""
    row = np.asarray(row, dtype=F32)
    assert row.shape in ((6,), (8,), (9,)), row.shape
    return tuple(row[1:]) + (F32(0),) * (9 - row.size)


def update_core3(x, e, m1, m2, m3, row, use1, use2, use3, add_z, z, stage=lambda key, fn: fn()):
    """``update4_core3`` on arrays: (u, m0) from x, e, the history m1, m2, m3 and z under ``row`` (``load_row``'s) and the caller's
    flags.  A term whose flag is off is not applied, and its input is not touched (it may be None).  ``stage(key, fn)`` computes
    one stage of the chain; ``key`` names the scalars applied so far, for a caller that keeps stages (``updater32``)."""
    s1, s2, s3, c2, c1, w1, w2, w3 = row
    key = (float(s1), float(s2))
    m0 = stage(key, lambda: ddim_x0(x, e, s1, s2))
    key += (float(s3), float(c2))
    u = stage(key, lambda: ddim_next(m0, e, s3, c2))
    for name, on, w, a, b in (("w1", use1, w1, m0, m1), ("w2", use2, w2, m1, m2), ("w3", use3, w3, m2, m3)):
        if on:
            key += (name, float(w))
            u = stage(key, lambda u=u, w=w, a=a, b=b: fma32(w, sub32(a, b), u))
    if add_z:
        key += ("c1", float(c1))
        u = stage(key, lambda u=u: fma32(z, c1, u))
    return u, m0


def updater32(x, e, m1=None, m2=None, m3=None, z=None):
    """One call of an update kernel on one row (``update4h``) as a function of (row, hist, hist2): (xt, x0) after the call, with the
    flags formed as the kernels form them -- use1 = w1 != 0, use2 = w2 != 0 and a hist buffer, use3 = w3 != 0 and a hist2 buffer,
    add_z = c1 != 0 where there is a z (the corrector's kernel has none and does not read c1).  ``hist`` / ``hist2`` False: a null
    buffer, whose term is not applied.  What the call leaves in the history buffers is a plain move (hist <- the old x0, hist2 <-
    the old hist) and is the caller's to compare.  Every stage is kept under the scalars applied so far, so rows that share a
    prefix of the chain share its cost."""
    memo = {}

    def stage(key, fn):
        if key not in memo:
            memo[key] = fn()
        return memo[key]

    def update(row, hist=True, hist2=True):
        r = load_row(row)
        c1, w1, w2, w3 = r[4:]
        return update_core3(x, e, m1, m2, m3, r, w1 != 0, w2 != 0 and hist, w3 != 0 and hist and hist2, z is not None and c1 != 0, z,
                            stage)

    return update
