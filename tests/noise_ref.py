"""Reference of the seeded noise stream, version 1 (csrc/noise.h), in numpy.

Philox4x32-10 written from the paper (Salmon, Moraes, Dror, Shaw: "Parallel Random Numbers: As Easy as 1, 2, 3", SC'11) on
uint64 arithmetic, and the transform of its words into normals in float64 (the yardstick) and in float32 (the same operation
order as the kernel, with numpy's functions).  The reference project has no such code."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # key increments
MASK = np.uint64(0xFFFFFFFF)
TAG_STEP, TAG_INITIAL = 0, 1


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds.  Counter words: integer arrays (broadcast together) or ints; key words: ints.  Returns four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def words(seed, first_sample, shape, k, tag=TAG_STEP):
    """The uint32 words of draw ``k`` for a [B, ...] tensor: element 4 q + j of sample b is word j of the call with counter
    (q, first_sample + b, k, tag) and key (seed & 0xffffffff, seed >> 32)."""
    shape = tuple(shape)
    b, per = shape[0], int(np.prod(shape[1:]))
    assert per % 4 == 0
    q = np.arange(per // 4, dtype=np.uint64)[None, :]
    s = (np.uint64(first_sample) + np.arange(b, dtype=np.uint64))[:, None]
    w = philox4x32_10(q, s, k, tag, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=-1).reshape(shape)


def normals64(w):
    """float64 normals of a words array and the float64 radius of each element's pair.  u and v are exact in either format."""
    flat = w.reshape(-1, 2).astype(np.uint64)
    u = ((flat[:, 0] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    v = (flat[:, 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u))
    # cos(pi v), sin(pi v) with the argument reduced exactly (v is a multiple of 2^-23 in [0, 2)): v = h + f, h in {0, 1}
    h = np.floor(v)
    f = v - h
    sign = 1.0 - 2.0 * h
    z = np.stack([r * sign * np.cos(np.pi * f), r * sign * np.sin(np.pi * f)], axis=-1)
    return z.reshape(w.shape), np.repeat(r, 2).reshape(w.shape)


def normals32(w):
    """The kernel's operation order in float32 with numpy's functions (the angle pi * v is rounded: coarser than sincospif)."""
    flat = w.reshape(-1, 2)
    u = ((flat[:, 0] >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)
    v = (flat[:, 1] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23)
    r = np.sqrt(np.float32(-2.0) * np.log(u))
    a = np.float32(np.pi) * v
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=-1).astype(np.float32).reshape(w.shape)
