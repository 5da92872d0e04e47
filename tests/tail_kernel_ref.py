"""References, case tables and gates for the kernels that run after the backward pass: qsample_kernel, sqerr_part / sqerr_final,
sqerr_bwd, ema_multi, sqnorm_multi / sqnorm_final, scale_multi and adam_multi (csrc/tail_kernels.hip).

The references are plain functions written from the documented formulas -- the comments above each kernel, the reference's
functions/losses.py:12-18 and models/ema.py:16-23, torch's Adam / AdamW and oracle/ref_cpu.adabelief_step -- in numpy on the CPU; the
library is not imported.  Three operations are defined by their fp32 roundings and have fp32 references that the kernels must
reproduce bit for bit (qsample, scale, ema); the others have fp64 references and a gate derived below from the roundings on the
kernel's longest chain.  No gate is measured from the GPU code: the one constant that cannot be derived (ADAM_P_C) is measured here,
on the CPU, from an fp32 mirror in numpy.  tests/test_tail_kernels_cpu.py proves the references against torch and the oracle and
keeps every mirror within half of its gate."""
import math
import zlib

import numpy as np

from step_math_ref import fma32

F = np.float32
U = 2.0 ** -24          # unit roundoff of fp32
BLOCK = 4096            # elements of one block-table entry (ddimx_ema_block_elems)
SQ_PARTS = 64           # parts of one sample in sqerr_part_kernel
THREADS = 256
N_STEPS = 1000


# ---- data --------------------------------------------------------------------------------------------------------------------------------
def rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def gauss(tag, shape):
    return rng(tag).standard_normal(shape).astype(F)


def alphas():
    """The cumulative products of the linear schedule (beta 1e-4 .. 0.02 over 1000 steps) as an fp32 table."""
    return np.cumprod(1.0 - np.linspace(1e-4, 0.02, N_STEPS, dtype=np.float64)).astype(F)


# ---- case tables -------------------------------------------------------------------------------------------------------------------------
# q-sample: one block, the last thread of a block, one past it, and a length that the 1024-block cap sends round the grid-stride loop twice
QS_PER = (1, 255, 256, 257, 1024 * 256 + 5)
QS_T = {1: ([0], [999]), 3: ([0, 999, 0], [999, 412, 999])}  # t per batch size: both ends of the table and a repeat
# loss: fewer elements than parts (parts past the end), one per part, one more (the `hi` clamp), the tiny model's length, 256 per part
# (every thread once), one more (a second trip for thread 0 alone; chunk 257), three trips and a ragged last part
SQ_PER = (1, 63, 64, 65, 1024, 16384, 16385, 3 * 16384 + 17)
SQ_B = (1, 2, 7)
BWD_B = (1, 3)
# multi-tensor kernels: one element, a few, one below / at / above a block, two blocks, three blocks and a tail -- in shuffled order so
# that the block table does not run through the tensors by size
SIZES = (4097, 1, 8192, 7, 3 * 4096 + 5, 4096, 4095)
MUS = (0.9999, 0.999, 0.5)
# both optimizer groups of ddim_audio_amd/configs.py
HYPER = (dict(lr=5e-4, betas=(0.9, 0.998), eps=1e-6), dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8))
WDS = (0.0, 1e-2)
STEPS = (1, 2, 10, 1000)
GSCALES = (1e-8, 1.0, 1e4)
MAX_NORM = 1.0


def tables(sizes, block=BLOCK):
    """The block table of the multi-tensor kernels: entry k is workgroup k, elements blk_off[k] .. + block - 1 of tensor blk_tensor[k]."""
    bt, bo = [], []
    for i, n in enumerate(sizes):
        for off in range(0, n, block):
            bt.append(i)
            bo.append(off)
    return bt, bo


# ---- q-sample (functions/losses.py:12-13) ------------------------------------------------------------------------------------------------
def qsample(x0, e, alphas_, t):
    """x0 * a.sqrt() + e * (1.0 - a).sqrt() as torch evaluates it in fp32: sa = sqrt32(a), sb = sqrt32(rn(1 - a)),
    x = rn(rn(x0 sa) + rn(e sb)).  x0, e: fp32 [B][per]; t: B in-range timesteps.  GATE: bit for bit."""
    a = np.asarray(alphas_, F)[np.asarray(t)]
    sa, sb = np.sqrt(a), np.sqrt(F(1.0) - a)
    return (x0 * sa[:, None]) + (e * sb[:, None])


# ---- loss (functions/losses.py:15-18) ----------------------------------------------------------------------------------------------------
def sqerr(e, out):
    """fp64 [B + 1]: loss[b] = sum over the sample of (e - out)^2, loss[B] = their mean."""
    d = np.asarray(e, np.float64) - np.asarray(out, np.float64)
    per = (d * d).sum(axis=1)
    return np.concatenate([per, [per.mean()]])


def sqerr_trips(per):
    chunk = -(-per // SQ_PARTS)
    return -(-chunk // THREADS)


def sqerr_k(per, B):
    """Roundings on the longest chain of sqerr_part_kernel + sqerr_final_kernel, (per-sample k, k of the mean).  A thread makes
    ceil(ceil(per / 64) / 256) trips of two roundings each (the subtraction and the fma); the wave sum adds 6 and the block sum 2
    ((r0 + r1) + (r2 + r3)); the final wave sum over the 64 parts adds 6.  The mean then adds B sums and one division.  All addends
    are positive, so each rounding costs at most 2^-24 of the result: GATE k 2^-24 loss[b]."""
    k = 2 * sqerr_trips(per) + (6 + 2) + 6
    return k, k + B + 1


def sqerr_gate(want, per):
    B = want.shape[0] - 1
    k, km = sqerr_k(per, B)
    return np.concatenate([k * U * want[:B], [km * U * want[B]]])


def wave_sum32(s):
    """fp32 butterfly over 64 lanes (rows of s): every lane ends with the same sum; returns lane 0's."""
    s = np.asarray(s, F).reshape(-1, 64).copy()
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, idx ^ o]
    return s[:, 0]


def sqerr_mirror(e, out):
    """The kernels' partition in fp32: 64 parts of ceil(per / 64) elements, 256 threads striding through a part with one fma per trip,
    a wave sum, (r0 + r1) + (r2 + r3), the wave sum of the parts, the running total and one division."""
    B, per = e.shape
    chunk = -(-per // SQ_PARTS)
    trips = sqerr_trips(per)
    loss = np.zeros(B + 1, F)
    tot = F(0)
    for b in range(B):
        parts = np.zeros(SQ_PARTS, F)
        for part in range(SQ_PARTS):
            lo, hi = part * chunk, min(part * chunk + chunk, per)
            d = np.zeros(trips * THREADS, F)
            if hi > lo:
                d[:hi - lo] = e[b, lo:hi] - out[b, lo:hi]
            d = d.reshape(trips, THREADS)
            s = np.zeros(THREADS, F)
            for k in range(trips):
                s = fma32(d[k], d[k], s)
            r = wave_sum32(s)
            parts[part] = (r[0] + r[1]) + (r[2] + r[3])
        loss[b] = wave_sum32(parts)[0]
        tot = tot + loss[b]
    loss[B] = tot / F(B)
    return loss


def loss_inputs(B, per, integer=False):
    """(e, out) fp32 [B][per].  integer: e - out is a non-zero integer with |d| <= 4 on integer e, so d^2 <= 16 and every partial sum of
    the largest case (7 x 49 169 elements) stays below 2^24: the fp32 sums are exact whatever their order."""
    r = rng(f"loss.{B}.{per}.{int(integer)}")
    if not integer:
        return r.standard_normal((B, per)).astype(F), r.standard_normal((B, per)).astype(F)
    e = r.integers(-8, 9, (B, per))
    d = r.integers(1, 5, (B, per)) * r.choice([-1, 1], (B, per))
    return e.astype(F), (e - d).astype(F)


def loss_grads(B, onehot=None):
    """Upstream gradient [B + 1]: Gaussian with a non-zero g[B], or (onehot = b) 1 at sample b and 0 elsewhere, g[B] included."""
    if onehot is not None:
        g = np.zeros(B + 1, F)
        g[onehot] = 1
        return g
    r = rng(f"loss.g.{B}")
    # Redrawn until (a) no g[b] + g[B] / B cancels by more than a factor of two, which SQERR_BWD_K assumes, and (b) the fp32
    # coefficient is within 1 u of the exact one.  Its two roundings (division, sum) are shared by every element of a sample, so an
    # unlucky draw spends up to 3 u on all of them at once and the mirror's margin would say nothing about the per-element roundings.
    while True:
        g = r.standard_normal(B + 1).astype(F)
        s, a = g[:B] + g[B] / F(B), np.abs(g[:B]) + np.abs(g[B]) / F(B)
        exact = g[:B].astype(np.float64) + float(g[B]) / B
        if g[B] != 0 and np.all(np.abs(s) >= 0.5 * a) and np.all(np.abs(s - exact) <= U * np.abs(exact)):
            return g


def sqerr_bwd(e, out, g, with_mean):
    """fp64 [B][per]: d = 2 (g[b] + [with_mean] g[B] / B) (out - e).  g has B (+ 1 with the mean) entries."""
    B = e.shape[0]
    g = np.asarray(g, np.float64)
    c = 2.0 * (g[:B] + (g[B] / B if with_mean else 0.0))
    return c[:, None] * (np.asarray(out, np.float64) - np.asarray(e, np.float64))


# c = 2 (g[b] + g[B] / B) and d = c (out - e): the division costs u |g[B] / B|, which is at most 2 u |sum| while the sum does not cancel
# by more than a factor of two (loss_grads sees to that); the sum, the difference out - e and the product cost u each (the doubling
# and the int -> float conversion of B are exact): five roundings against |d|, and one spare
SQERR_BWD_K = 6


def sqerr_bwd_gate(want):
    return SQERR_BWD_K * U * np.abs(want)


def sqerr_bwd_mirror(e, out, g, with_mean):
    B = e.shape[0]
    c = F(2.0) * (g[:B] + (g[B] / F(B) if with_mean else F(0)))
    return c[:, None] * (out - e)


# ---- EMA (models/ema.py:16-23) -----------------------------------------------------------------------------------------------------------
def ema(shadow, p, mu, c_param=None):
    """(1.0 - mu) * p + mu * shadow with mu a Python double, as torch evaluates it on fp32 tensors: both scalars are rounded to fp32
    (c_param = fp32(1.0 - mu) from the DOUBLE, c_shadow = fp32(mu)) and the three operations are rounded separately.  c_param overrides
    the parameter's weight (the finding this replaced: fp32(1 - fp32(mu))).  GATE: bit for bit."""
    cp = F(1.0 - mu) if c_param is None else F(c_param)
    return (cp * p) + (F(mu) * shadow)


def ema_old_coef(mu):
    """What the first export forms from its float argument: fp32(1 - fp32(mu))."""
    return F(1.0 - float(F(mu)))


# ---- gradient norm and clip (torch.nn.utils.clip_grad_norm_) -----------------------------------------------------------------------------
def grad_norm(gs, max_norm):
    """fp64 (L2 norm over all tensors, min(1, max_norm / (norm + 1e-6)))."""
    n = math.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in gs))
    return n, min(1.0, max_norm / (n + 1e-6))


def norm_cases():
    """(name, gradients per tensor of SIZES) with the norm far below MAX_NORM (coefficient exactly 1), 2 % above it (the only range in
    which the 1e-6 of the denominator reaches the coefficient's bits while the coefficient is below 1) and far above it."""
    unit = [gauss(f"norm.{n}", n) for n in SIZES]
    n0 = grad_norm(unit, MAX_NORM)[0]
    return [(name, [(g * F(sc)).astype(F) for g in unit]) for name, sc in (("below", 1e-4), ("about", 1.02 * MAX_NORM / n0), ("above", 10.0))]


def clip_coef32(norm32, max_norm):
    """out[1] from the kernel's own out[0], in fp32: the division, the sum and the constant 1e-6f are each rounded once.  GATE: bit for bit."""
    c = F(max_norm) / (F(norm32) + F(1e-6))
    return c if c < F(1.0) else F(1.0)


# sqnorm_multi_kernel: a thread makes 4096 / 256 = 16 fma (the squares are exact inside them), then 6 wave and 2 block additions, all on
# positive numbers: 24 roundings of the sum of squares.  sqnorm_final_kernel adds the partials in double (2^-53 each: nothing against
# 2^-24) and takes a double square root, which halves the relative error; the conversion to fp32 is one more rounding.
NORM_K = (BLOCK // THREADS + 6 + 2) / 2 + 1  # = 13


def grad_norm_gate(want_norm):
    return NORM_K * U * want_norm


def grad_norm_mirror(gs):
    tot = 0.0
    for g in gs:
        for off in range(0, g.size, BLOCK):
            blk = np.zeros(BLOCK, F)
            blk[:min(BLOCK, g.size - off)] = g[off:off + BLOCK]
            blk = blk.reshape(BLOCK // THREADS, THREADS)
            s = np.zeros(THREADS, F)
            for k in range(BLOCK // THREADS):
                s = fma32(blk[k], blk[k], s)
            r = wave_sum32(s)
            tot += float((r[0] + r[1]) + (r[2] + r[3]))
    return F(math.sqrt(tot))


def scale(g, c):
    """g * c in fp32.  GATE: bit for bit (and bitwise untouched for c = 1)."""
    return g * F(c)


# ---- Adam / AdamW / AdaBelief ------------------------------------------------------------------------------------------------------------
def f32v(x):
    """The value a C float argument carries."""
    return float(F(x))


def dyn_scalars(hp, step):
    """{lr, 1 - beta1^step, sqrt(1 - beta2^step)} as fp32: what ddimx_adam_multi derives from its float arguments."""
    b1, b2 = f32v(hp["betas"][0]), f32v(hp["betas"][1])
    return F(hp["lr"]), F(1.0 - b1 ** step), F(math.sqrt(1.0 - b2 ** step))


def adam(p, g, m, v, step, hp, wd, decoupled, clip=None):
    """One step in real arithmetic (fp64) on the float-valued arguments the export receives.  decoupled 0: torch.optim.Adam (L2 term in
    the gradient), 1: AdamW, 2: AdaBelief (decoupled decay, eps added to v, no rectification).  clip: optional coefficient on g.
    Returns a dict with the new (p, m, v) and the ingredients of the gates."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = f32v(hp["lr"]), f32v(hp["betas"][0]), f32v(hp["betas"][1]), f32v(hp["eps"]), f32v(wd)
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    gc = g * (1.0 if clip is None else f32v(clip))
    if decoupled:
        p1, gp, gabs = p * (1.0 - lr * wd), gc, np.abs(gc)
    else:
        p1, gp, gabs = p, gc + wd * p, np.abs(gc) + wd * np.abs(p)
    mn = m + (1.0 - b1) * (gp - m)
    r = gp - mn
    vn = b2 * v + (1.0 - b2) * r * r + eps if decoupled == 2 else b2 * v + (1.0 - b2) * gp * gp
    denom = np.sqrt(vn) / bc2s + eps
    step_size = lr / bc1
    return dict(p=p1 - step_size * mn / denom, m=mn, v=vn, gabs=gabs, m_old=np.abs(m), r=np.abs(r), denom=denom, step_size=step_size,
                one_minus_b2=1.0 - b2, decoupled=decoupled)


# m = fma(1 - b1, rn(g' - m), m), g' = rn(g c) [+ fma(wd, p, .) for Adam's L2 term]: the two roundings of g' cost 2 u |g'|, the
# difference u |g' - m|, the fma u |m_new|, and |m_new| <= max(|g'|, |m|): at most 4 u (|g'| + |m_old|).  (1 - b1 is exact for b1 >= 0.5.)
ADAM_M_K = 4
# v = fma(rn(g'^2), 1 - b2, rn(v b2)): g' carries 2 u, its square 4 u and one more for the squaring; rn(v b2) one; the fma one.  All
# terms are positive: at most 7 u v_new; one spare.  AdaBelief adds eps (one more rounding, inside the spare) and squares
# r = rn(g' - m_new) instead: |r| <= |g'| + |m_old|, and its absolute error dr <= 2 u |g'| (g') + 4 u (|g'| + |m_old|) (m_new)
# + u |r| <= 7 u (|g'| + |m_old|) does not shrink with r, so (r + dr)^2 adds the cancellation term (1 - b2) (2 |r| dr + dr^2).
ADAM_V_K = 8
ADAM_R_K = 7
# p: the quotient m / denom carries the errors of m and of sqrt(v) through a division, which has no clean constant; the form
#   c 2^-24 (|p_ref| + step_size (|g'| + |m_old|) / denom_ref)
# scales with the two things that are rounded (the parameter, and the update at the size m's own error has).  c is measured HERE: the
# fp32 mirror below against `adam` on every case of adam_cases() gave at most 2.285 of that unit (test_tail_kernels_cpu.py prints it
# and fails if it exceeds half of c); twice that, rounded up.
ADAM_P_C = 5


def adam_gates(w):
    """(gate p, gate m, gate v) for a result of `adam`."""
    gm = ADAM_M_K * U * (w["gabs"] + w["m_old"])
    gv = ADAM_V_K * U * w["v"]
    if w["decoupled"] == 2:
        dr = ADAM_R_K * U * (w["gabs"] + w["m_old"])
        gv = gv + w["one_minus_b2"] * (2.0 * w["r"] * dr + dr * dr)
    gp = ADAM_P_C * U * (np.abs(w["p"]) + w["step_size"] * (w["gabs"] + w["m_old"]) / w["denom"])
    return gp, gm, gv


def adam_mirror(p, g, m, v, step, hp, wd, decoupled, clip=None):
    """The update in fp32 with one rounding per operation, in the kernel's order."""
    lr, bc1, bc2s = dyn_scalars(hp, step)
    b1, b2, eps, wd = F(hp["betas"][0]), F(hp["betas"][1]), F(hp["eps"]), F(wd)
    step_size = lr / bc1
    gk = g * (F(1.0) if clip is None else F(clip))
    pk = p
    if decoupled:
        pk = pk * (F(1.0) - lr * wd)
    else:
        gk = fma32(wd, pk, gk)
    mk = fma32(F(1.0) - b1, gk - m, m)
    if decoupled == 2:
        r = gk - mk
        vk = fma32(r * r, F(1.0) - b2, v * b2) + eps
    else:
        vk = fma32(gk * gk, F(1.0) - b2, v * b2)
    denom = np.sqrt(vk) / bc2s + eps
    return fma32(-step_size, mk / denom, pk), mk, vk


def adam_state(tag, n, step, gscale):
    """(p, g, m, v) of one tensor, fp32.  |g| is at least 1e-3 gscale, so g^2 (1 - b2) stays far above the subnormals.  step 1 starts
    from the zero state and has g = 0 exactly on every fifth element: there the denominator is eps alone and the update must be 0.
    Later steps start from a given state of the gradient's size (m mixed in sign, v positive)."""
    r = rng(f"adam.{tag}.{n}.{step}.{gscale}")
    z = r.standard_normal(n)
    g = (np.sign(z) * np.maximum(np.abs(z), 1e-3) * gscale).astype(F)
    p = (0.5 * r.standard_normal(n)).astype(F)
    if step == 1:
        g[::5] = 0
        return p, g, np.zeros(n, F), np.zeros(n, F)
    m = (0.5 * gscale * r.standard_normal(n)).astype(F)
    v = (gscale * gscale * (0.25 + r.random(n))).astype(F)
    return p, g, m, v


def adam_configs():
    """(decoupled, wd, index into HYPER): one GPU test each; every one runs all STEPS x GSCALES."""
    return [(d, wd, h) for d in (0, 1, 2) for wd in WDS for h in range(len(HYPER))]


def adam_id(c):
    return f"mode{c[0]}-wd{c[1]:g}-hp{c[2]}"


def adam_cases(cfg):
    """Every (step, gscale, [(p, g, m, v) per tensor of SIZES]) of one configuration."""
    for step in STEPS:
        for gs in GSCALES:
            yield step, gs, [adam_state(adam_id(cfg), n, step, gs) for n in SIZES]


def worst(err, gate):
    """max |err| / gate over all elements; a zero gate admits only a zero error."""
    err, gate = np.abs(np.asarray(err, np.float64)).reshape(-1), np.asarray(gate, np.float64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(gate > 0, err / gate, np.where(err > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0
