"""Reference of the Brownian path of ``BrownianStream`` (include/ddimx_brownian.h; test infrastructure).

Written from the contract and not from ``schedule.brownian_plan``: the tree is addressed by the binary digits of t (the node that
holds t at level l is 2^(l-1) + t // w, w = N / 2^(l-1) its width), where the product code walks intervals down from the root, so the
two check each other.  Three restatements over any source of the nodes' normals ``xi(node) -> array``:

* ``path64`` -- P(t) in float64;
* ``path32`` -- the kernel's operation order in fp32 with an exact fused multiply-add (``step_math_ref.fma32``): the bits it must give;
* ``path_bound`` -- float64 P(t) from float64 normals together with a running bound on what the fp32 evaluation may differ by,
  carried down the descent.
"""
import numpy as np
import torch

import noise_ref as N
from step_math_ref import fma32

F32 = np.float32
U = 2.0 ** -24  # unit roundoff of fp32
TAG_PATH = 2


# ---- the clock and the tree, float64 ------------------------------------------------------------------------------------------------------
def clock(alpha, tau):
    """(u [N + 1], D): u[t] = exp(2 tau lam[t]) for t < T, 0 for T <= t <= N = 2^D, D = max(1, ceil(log2 T))."""
    a = torch.as_tensor(alpha).to("cpu", torch.float32).numpy().astype(np.float64)
    depth = 1
    while (1 << depth) < a.size:
        depth += 1
    lam = 0.5 * np.log(a / (1.0 - a))
    u = np.zeros((1 << depth) + 1)
    u[:a.size] = np.exp(2.0 * tau * lam)
    return u, depth


def descent(u, depth, t):
    """[(node, rho, s, a, b)] of the draws that make P(t), the anchor first (node 0, rho = 0, s = sqrt(u0), [a, b] = [0, N]); float64.
    1 + (D - trailing zeros of t) records for t > 0, one for t = 0."""
    n = 1 << depth
    recs = [(0, 0.0, float(np.sqrt(u[0])), 0, n)]
    if t == 0:
        return recs
    stop = depth - ((t & -t).bit_length() - 1)  # the level whose midpoint is t
    for level in range(1, stop + 1):
        w = n >> (level - 1)
        a = (t // w) * w
        b, m = a + w, a + w // 2
        span = u[a] - u[b]
        rho = (u[m] - u[b]) / span if span > 0 else 0.0
        s = np.sqrt((u[a] - u[m]) * (u[m] - u[b]) / span) if span > 0 else 0.0
        recs.append(((1 << (level - 1)) + t // w, float(rho), float(s), a, b))
    assert (recs[-1][3] + recs[-1][4]) // 2 == t and len(recs) == 1 + stop
    return recs


def step_plan(u, depth, i, j):
    """The logical plan of the step i -> j: (records of the descent to i, records of the descent to j, the number of leading
    records they share, g = 1 / sqrt(u_j - u_i))."""
    ri, rj = descent(u, depth, i), descent(u, depth, j)
    share = 0
    while share < min(len(ri), len(rj)) and ri[share][0] == rj[share][0]:
        share += 1
    return ri, rj, share, float(1.0 / np.sqrt(u[j] - u[i]))


def run_plan(seq, alpha, tau):
    """Per iteration of a run over ``seq`` (execution order) its ``step_plan``, None for the final jump to t = -1 and for tau = 0."""
    levels = list(reversed(list(seq)))
    if tau == 0:
        return [None] * len(levels)
    u, depth = clock(alpha, tau)
    return [step_plan(u, depth, i, j) for i, j in zip(levels, levels[1:])] + [None]


def decode_row(row, max_depth):
    """A row of ``schedule.brownian_plan`` as (share, g, records of i, records of j), a record (node, rho, s, enter) with fp32 rho, s."""
    row = np.ascontiguousarray(row, dtype=np.int32)
    f = row.view(F32)
    per = max_depth + 1

    def recs(base, n):
        return [(int(row[base + 4 * r]), f[base + 4 * r + 1], f[base + 4 * r + 2], int(row[base + 4 * r + 3])) for r in range(n)]

    return int(row[0]), f[3], recs(4, int(row[1])), recs(4 + 4 * per, int(row[2]))


# ---- the path over a source of normals ---------------------------------------------------------------------------------------------------
def _ends(recs, r, pa, pb, pm):
    """(P(a), P(b)) of record r >= 1 from those of the record before and its midpoint value."""
    if r == 1:
        return pa, pb  # the root: [0, N] as the anchor left it
    prev_m = (recs[r - 1][3] + recs[r - 1][4]) // 2
    if recs[r][4] == prev_m:
        return pa, pm
    assert recs[r][3] == prev_m
    return pm, pb


def path64(recs, xi):
    """P(t) of ``descent``'s records in float64; ``xi(node)``: the float64 normals of a node."""
    pa = pb = pm = None
    for r, (node, rho, s, _, _) in enumerate(recs):
        z = np.asarray(xi(node), dtype=np.float64)
        if r == 0:
            pm = s * z
            pa, pb = pm, np.zeros_like(pm)
        else:
            pa, pb = _ends(recs, r, pa, pb, pm)
            pm = pb + rho * (pa - pb) + s * z
    return pm


def path32(recs, xi, memo=None):
    """The kernel's bits: rho, s rounded to fp32; d = P(a) - P(b); v = fma(rho, d, P(b)); P(m) = fma(s, xi, v); P(0) = sqrt(u0) xi_0;
    every operation rounded once.  ``xi(node)``: the fp32 normals of a node.  ``memo`` (a dict the caller keeps for one clock and one
    source of normals) holds what each node left, so descents that share a prefix share its cost: a node's value is one value."""
    pa = pb = pm = None
    for r, (node, rho, s, _, _) in enumerate(recs):
        if memo is not None and node in memo:
            pa, pb, pm = memo[node]
            continue
        z = np.asarray(xi(node), dtype=F32)
        if r == 0:
            pm = (F32(s) * z).astype(F32)
            pa, pb = pm, np.zeros_like(pm)
        else:
            pa, pb = _ends(recs, r, pa, pb, pm)
            d = (pa - pb).astype(F32)
            pm = fma32(F32(s), z, fma32(F32(rho), d, pb))
        if memo is not None:
            memo[node] = (pa, pb, pm)
    return pm


def increment32(plan, xi, memo=None):
    """z = (P(j) - P(i)) g in fp32 of a ``step_plan``."""
    ri, rj, _, g = plan
    return ((path32(rj, xi, memo) - path32(ri, xi, memo)).astype(F32) * F32(g)).astype(F32)


def increment64(plan, xi):
    ri, rj, _, g = plan
    return (path64(rj, xi) - path64(ri, xi)) * g


def path_bound(recs, xi_r):
    """(P(t) in float64, a bound on |fp32 P(t) - it|).  ``xi_r(node)``: (float64 normals, the float64 radius of each element's pair:
    ``noise_ref.normals64``).  The fp32 normal is within 8 U r of the float64 one (the counted bound of the noise stream); down the
    descent, with err_a, err_b the bounds of the ends,
        err_m = err_b + rho (err_a + err_b) + s 8 U r + 3 U (|P_b| + rho |d| + s |xi|):
    the ends' errors through the interpolation (rho err_a + (1 - rho) err_b at most), the normal's error times s, and the roundings,
    each at most U times what it rounds: rho and s themselves, d, the inner fma (|P_b| + rho |d|) and the outer one (all three
    magnitudes).  Counted one by one that is U (2 |P_b| + 4 rho |d| + 2 s |xi|); the line charges every magnitude three times
    instead, which is the larger figure wherever |P_b| + s |xi| >= rho |d| and gives one U rho |d| away elsewhere -- against
    worst cases that would need every rounding at its limit and of one sign.  The anchor is the same line with P_b = rho = 0."""
    pa = pb = pm = ea = eb = em = None
    for r, (node, rho, s, _, _) in enumerate(recs):
        z, rad = xi_r(node)
        if r == 0:
            pm = s * z
            em = s * 8 * U * rad + 3 * U * np.abs(pm)
            pa, pb, ea, eb = pm, np.zeros_like(pm), em, np.zeros_like(pm)
        else:
            (pa, pb), (ea, eb) = _ends(recs, r, pa, pb, pm), _ends(recs, r, ea, eb, em)
            d = pa - pb
            pm = pb + rho * d + s * z
            em = eb + rho * (ea + eb) + s * 8 * U * rad + 3 * U * (np.abs(pb) + rho * np.abs(d) + s * np.abs(z))
    return pm, em


def increment_bound(plan, xi_r):
    """(z in float64, a bound on |fp32 z - it|): g times the two ends' bounds, and 3 U |z| for the subtraction, g's own rounding and
    the product."""
    ri, rj, _, g = plan
    (pi, ei), (pj, ej) = path_bound(ri, xi_r), path_bound(rj, xi_r)
    z = (pj - pi) * g
    return z, g * (ei + ej) + 3 * U * np.abs(z)


def words_normals(seed, first_sample, shape):
    """``xi_r`` over the Philox words of the stream's own counters (node, tag 2), cached per node."""
    memo = {}

    def xi_r(node):
        if node not in memo:
            memo[node] = N.normals64(N.words(seed, first_sample, shape, node, TAG_PATH))
        return memo[node]

    return xi_r
