"""CPU restatements of the x0 clip / dynamic threshold (test infrastructure; the library is not imported).

Bit-exact fp32, on ``step_math_ref``'s operations (the x0 prediction, the clip, the rewritten eps): the selection on the
prediction's bit patterns by ``np.partition`` (no radix, no histogram: another algorithm than the kernels'), (s, r), and one
sample's rewrite.

Float64: ``generalized_steps`` from the reference's formulas and ``dpm_solver_steps`` in the paper's form (``solver_ref``'s, with
the rule between the prediction and its use), over any ``model_fn(x, t) -> eps`` on [B, ...] arrays."""
import numpy as np
import torch

from ddim_audio_amd.schedule import X0Clip, X0Threshold, threshold_rank
import solver_ref as R
import step_math_ref as SM

F32 = np.float32
ABS = np.uint32(0x7FFFFFFF)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- fp32, bit for bit ------------------------------------------------------------------------------------------------------------------
def select_key(keys, rank):
    """The key of 0-based rank ``rank`` in ascending order."""
    keys = np.asarray(keys, dtype=np.uint32).reshape(-1)
    return np.partition(keys, rank)[rank]


def quantile(x0, rank):
    """The order statistic of |x0| at ``rank`` by its bit pattern (NaN and inf sort above every finite value), as fp32."""
    return np.array([select_key(bits(x0).reshape(-1) & ABS, rank)], dtype=np.uint32).view(F32)[0]


def scale_row(q, floor, ceil):
    """(s, r): s = ``x0_scale`` (no ceiling: +inf), r = rn(floor / s)."""
    s = F32(SM.x0_scale(q, floor, np.inf if ceil is None else ceil))
    with np.errstate(all="ignore"):
        return s, F32(F32(floor) / s)


def scale_rows(x, e, rows, rank, floor, ceil):
    """[B, 2] fp32: ``ddimxq_x0_quantile`` for a batch x, e [B, n] with sample b on the table row ``rows[b]`` = (s1, s2)."""
    return np.array([scale_row(quantile(SM.ddim_x0(x[b], e[b], *rows[b]), rank), floor, ceil) for b in range(len(x))], dtype=F32)


def rewrite(x, e, s1, s2, s, r):
    """``ddimxq_threshold_eps`` for one sample: (eps', keep) -- keep marks the elements whose c has x0's bits (they keep e)."""
    x0 = SM.ddim_x0(x, e, s1, s2)
    c = SM.x0_clip(x0, s, r)
    return SM.x0_to_eps(x, e, x0, c, s1, s2), bits(c) == bits(x0)


# ---- float64 ------------------------------------------------------------------------------------------------------------------------------
def rule64(m0, rule):
    """The clipped prediction of a batch m0 [B, ...] under ``rule`` (None, X0Clip, X0Threshold), per sample."""
    if rule is None:
        return m0
    out = np.empty_like(m0)
    for b in range(m0.shape[0]):
        if isinstance(rule, X0Clip):
            s, r = rule.limit, 1.0
        else:
            a = np.abs(m0[b]).reshape(-1)
            k = threshold_rank(rule.ratio, a.size)
            s = min(max(float(np.partition(a, k)[k]), rule.floor), np.inf if rule.ceil is None else rule.ceil)
            r = rule.floor / s
        out[b] = np.clip(m0[b], -s, s) * r
    return out


def generalized_steps(x, seq, model_fn, alpha, eta, rule, noise_fn=None):
    """functions/denoising.py:10-52 in float64 with the rule on x0_t: (xs, x0_preds) of every iteration, xs[0] = x.
    ``noise_fn(k, shape)``: the noise of iteration k."""
    a = np.concatenate([[1.0], torch.as_tensor(alpha).to("cpu", torch.float32).numpy().astype(np.float64)])
    seq = list(seq)
    x = np.asarray(x, dtype=np.float64)
    xs, x0s = [x.copy()], []
    for k, (i, j) in enumerate(zip(reversed(seq), reversed([-1] + seq[:-1]))):
        at, an = a[i + 1], a[j + 1]
        et = np.asarray(model_fn(x, i), dtype=np.float64)
        x0 = rule64((x - et * np.sqrt(1 - at)) / np.sqrt(at), rule)
        et = (x - np.sqrt(at) * x0) / np.sqrt(1 - at)  # the eps whose prediction is the clipped one
        c1 = eta * np.sqrt((1 - at / an) * (1 - an) / (1 - at))
        c2 = np.sqrt((1 - an) - c1 ** 2)
        x = np.sqrt(an) * x0 + c2 * et
        if c1 != 0.0:
            x = x + c1 * np.asarray(noise_fn(k, x.shape), dtype=np.float64)
        x0s.append(x0)
        xs.append(x.copy())
    return xs, x0s


def dpm_solver_steps(x, seq, model_fn, alpha, order, rule):
    """``solver_ref.dpm_solver_steps`` (orders 1-2) with the rule on m0 before it enters the step and the history."""
    assert order in (1, 2)
    ts = list(reversed(list(seq)))
    al, sg, lam = R.levels(seq, alpha)
    x = np.asarray(x, dtype=np.float64)
    xs, ms = [x.copy()], []
    for k, t in enumerate(ts):
        eps = np.asarray(model_fn(x, t), dtype=np.float64)
        m0 = rule64((x - sg[k] * eps) / al[k], rule)
        ms.append(m0)
        if sg[k + 1] == 0.0:
            x = m0.copy()
        else:
            h = lam[k + 1] - lam[k]
            phi1 = np.expm1(-h)
            x = sg[k + 1] / sg[k] * x - al[k + 1] * phi1 * m0
            if min(order, k + 1) == 2:
                x = x - 0.5 * al[k + 1] * phi1 * (m0 - ms[-2]) / ((lam[k] - lam[k - 1]) / h)
        xs.append(x.copy())
    return xs, ms
