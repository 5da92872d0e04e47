"""Restatements of the restoring pool's update kernel (``csrc/restore_pool_kernels.hip``; test infrastructure, CPU only).

``update32`` is ``rpx_pool_update_kernel`` on one active slot in float32: every operation is ``step_math_ref``'s (the fp32
mirror of ``step_math.h``), in the kernel's order, so its results are the bits the kernel must give for the same z.
``known64`` is the known region's path in float64 -- what the fp32 path is checked against, and y exactly at a final row."""
import numpy as np

import step_math_ref as S

KNOWN = 1  # RPX_KNOWN


def flags_of(row):
    """(use1, use2, add_z) as the kernel forms them from a pool row (t, s1, s2, s3, c2, c1, w1, w2)."""
    row = np.asarray(row, dtype=np.float32)
    return bool(row[6] != 0), bool(row[7] != 0), bool(row[5] != 0)


def update32(x, e, m1, m2, y, m, row, known, flags, z=None):
    """One active slot: (xt, x0, hist) after the launch from x, e, the history m1 = x0 and m2 = hist, the clip y and the mask m
    under the pool row ``row``, the companion row ``known`` = (cx, w0) and the slot's ``flags``.  A term whose weight is 0 is not
    applied and its operand is not touched (it may be None); y, m and ``known`` are not touched without ``KNOWN``."""
    use1, use2, add_z = flags_of(row)
    r = S.load_row(row)
    u, m0 = S.update_core3(x, e, m1, m2, None, r, use1, use2, False, add_z, z)
    if flags & KNOWN:
        cx, w0 = (np.float32(v) for v in known)
        kv = S.inpaint_known(x, y, cx, w0, cx != 0)
        if add_z:
            kv = S.fma32(z, r[4], kv)
        u = S.inpaint_replace(u, kv, m)
    return u, m0, m1


def known64(x, y, cx, w0, c1=0.0, z=None):
    """The exact path of the known region in float64: cx x + w0 y (+ c1 z)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    kv = float(w0) * y + (float(cx) * x if cx != 0 else 0.0)
    return kv + float(c1) * np.asarray(z, dtype=np.float64) if c1 != 0 else kv
