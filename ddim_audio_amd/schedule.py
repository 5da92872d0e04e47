"""Diffusion schedule tables and sampler step sequences (host side, numpy/float64 -> fp32).

Mirrors the pieces of the reference runner that sit on the hot path's boundary:
``get_beta_schedule`` (reference ``runners/diffusion.py:32-62``), the fp32 cumulative product of
``Diffusion.__init__`` (``:90-128``) and the ``seq`` construction of ``sample_image`` (``:475-500``).
"""
import collections

import numpy as np
import torch

from . import _lib  # the ABI's constants, parsed from the headers: no library is loaded


def get_beta_schedule(beta_schedule, *, beta_start, beta_end, num_diffusion_timesteps):
    n = num_diffusion_timesteps
    if beta_schedule == "linear":
        betas = np.linspace(beta_start, beta_end, n, dtype=np.float64)
    elif beta_schedule == "quad":
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=np.float64) ** 2
    elif beta_schedule == "const":
        betas = beta_end * np.ones(n, dtype=np.float64)
    elif beta_schedule == "jsd":
        betas = 1.0 / np.linspace(n, 1, n, dtype=np.float64)
    elif beta_schedule == "sigmoid":
        x = np.linspace(-6, 6, n)
        betas = 1.0 / (np.exp(-x) + 1.0) * (beta_end - beta_start) + beta_start
    else:
        raise NotImplementedError(beta_schedule)
    assert betas.shape == (n,)
    return betas


def alphas_cumprod(betas):
    """fp32 cumprod of [1, 1-beta] without the leading 1: the ``self.alphas`` table the reference
    runner hands to ``generalized_steps`` (``runners/diffusion.py:109-115,497-499``).  The product is
    taken in fp32, sequentially, exactly as ``torch.cumprod`` on a float tensor does."""
    a = torch.from_numpy(np.concatenate([[1.0], 1.0 - np.asarray(betas, dtype=np.float64)])).to(torch.float32)
    return a.cumprod(dim=0)[1:].contiguous()


def make_schedule(diffusion_cfg):
    betas = get_beta_schedule(
        diffusion_cfg.beta_schedule,
        beta_start=diffusion_cfg.beta_start,
        beta_end=diffusion_cfg.beta_end,
        num_diffusion_timesteps=diffusion_cfg.num_diffusion_timesteps,
    )
    return torch.from_numpy(betas).to(torch.float32), alphas_cumprod(betas)


def make_seq(num_timesteps, timesteps, skip_type="uniform"):
    """Timestep subsequence of ``sample_image`` (reference ``runners/diffusion.py:482-494``)."""
    if skip_type == "uniform":
        skip = num_timesteps // timesteps
        return list(range(0, num_timesteps, skip))
    if skip_type == "quad":
        seq = np.linspace(0, np.sqrt(num_timesteps * 0.8), timesteps) ** 2
        return [int(s) for s in list(seq)]
    raise NotImplementedError(skip_type)


def ddim_coefficients(seq, alpha, eta=0.0):
    """Per-iteration scalars of ``generalized_steps`` (reference ``functions/denoising.py:12-40``).

    ``alpha`` is the fp32 alphas-cumprod table; like the reference, the scalars are formed in
    Python double precision from the fp32 table values.  Returns a float64 array [n_iter, 6] in
    execution order (reversed ``seq``): columns (t, sqrt(1-at), sqrt(at), sqrt(at_next), c2, c1).
    """
    a = [1.0] + torch.as_tensor(alpha).to("cpu", torch.float32).numpy().tolist()
    seq = list(seq)
    seq_next = [-1] + seq[:-1]
    rows = []
    for i, j in zip(reversed(seq), reversed(seq_next)):
        at = a[int(i) + 1]
        at_next = a[int(j) + 1]
        c1 = eta * ((1 - at / at_next) * (1 - at_next) / (1 - at)) ** 0.5
        c2 = ((1 - at_next) - c1 ** 2) ** 0.5
        rows.append((float(int(i)), (1 - at) ** 0.5, at ** 0.5, at_next ** 0.5, c2, c1))
    return np.asarray(rows, dtype=np.float64).reshape(-1, 6)


def ddpm_coefficients(seq, betas):
    """Per-iteration scalars of ``ddpm_steps`` (reference ``functions/denoising.py:4-7,64-88``), formed with the
    reference's fp32 *tensor* arithmetic (it works on [n,1,1,1] fp32 tensors, not Python doubles).  Returns a float32
    array [n_iter, 7] in execution order: (t, (1/at).sqrt(), (1/at-1).sqrt(), atm1.sqrt()*beta_t,
    (1-beta_t).sqrt()*(1-atm1), 1-at, mask*exp(0.5*log(beta_t)))."""
    b = torch.as_tensor(betas).to("cpu", torch.float32)
    acp = (1 - torch.cat([torch.zeros(1), b], dim=0)).cumprod(dim=0)  # compute_alpha's table, index t+1
    seq = list(seq)
    seq_next = [-1] + seq[:-1]
    rows = []
    for i, j in zip(reversed(seq), reversed(seq_next)):
        at, atm1 = acp[int(i) + 1], acp[int(j) + 1]
        beta_t = 1 - at / atm1
        mask = 1.0 - float(int(i) == 0)
        rows.append(torch.stack([torch.tensor(float(int(i))), (1.0 / at).sqrt(), (1.0 / at - 1).sqrt(), atm1.sqrt() * beta_t,
                                 (1 - beta_t).sqrt() * (1 - atm1), 1.0 - at, mask * torch.exp(0.5 * beta_t.log())]))
    return torch.stack(rows).to(torch.float32).numpy()


PREDICTIONS = ("eps", "v")  # what the network's output is: the noise, or v = sqrt(at) eps - sqrt(1-at) x0 (Salimans & Ho 2022)


def check_prediction(prediction):
    """``prediction`` if it is one of ``PREDICTIONS``, else ValueError."""
    if prediction not in PREDICTIONS:
        raise ValueError(f"prediction must be 'eps' or 'v', got {prediction!r}")
    return prediction


def v_table(alpha):
    """The table of ``ddimx_v_to_eps``: float64 [len(alpha), 2], row t = (s1, s2) = (sqrt(1-at), sqrt(at)), formed exactly as
    ``ddim_coefficients`` forms its columns 1-2 (Python doubles from the fp32 table's values), so after rounding to fp32 row t
    equals those columns of the row with timestep t in every coefficient table.  eps = s1 x + s2 v, x0 = s2 x - s1 v."""
    a = torch.as_tensor(alpha).to("cpu", torch.float32).numpy().tolist()
    return np.asarray([((1 - at) ** 0.5, at ** 0.5) for at in a], dtype=np.float64).reshape(-1, 2)


def _finite(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def _positive32(v):
    """v is positive and finite once rounded to fp32, which is what the kernels receive."""
    with np.errstate(over="ignore"):
        f = np.float32(v)
    return bool(f > 0 and np.isfinite(f))


class X0Clip(collections.namedtuple("X0Clip", "limit")):
    """Static clipping of the x0 prediction in ``generalized_steps`` / ``dpm_solver_steps`` / ``SamplerPool``: every iteration,
    between the network's eps and the update, x0 = (x - s1 eps) / s2 is clamped to [-limit, limit] and eps is replaced by the
    eps whose prediction is the clamped value; an element the clamp leaves alone keeps its eps bit for bit.  ``limit`` is finite
    and positive (1.0: the range of the spectrograms).  Immutable."""
    __slots__ = ()

    def __new__(cls, limit=1.0):
        limit = _finite("limit", limit)
        if not _positive32(limit):
            raise ValueError(f"limit must be positive (and finite in fp32), got {limit!r}")
        return super().__new__(cls, limit)


class X0Threshold(collections.namedtuple("X0Threshold", "ratio floor ceil")):
    """Dynamic thresholding of the x0 prediction (Saharia et al. 2022, section 2.3), per sample and iteration: q is the order
    statistic of |x0| over the sample's n elements at rank ``threshold_rank(ratio, n)`` (the ``interpolation="lower"`` quantile,
    exact), s = min(max(q, floor), ceil), and x0 is clamped to [-s, s] and multiplied by r = floor / s; eps is replaced by the eps
    whose prediction is that value, and an element it leaves alone keeps its eps bit for bit.  With ``floor`` = 1 this is Imagen's
    rule (clamp to +-s, divide by s).  ``ratio`` in (0, 1]; 0 < ``floor`` <= ``ceil``, finite, ``ceil`` None for no upper limit.
    Immutable."""
    __slots__ = ()

    def __new__(cls, ratio=0.995, floor=1.0, ceil=None):
        ratio, floor = _finite("ratio", ratio), _finite("floor", floor)
        if not 0 < ratio <= 1:
            raise ValueError(f"ratio must be in (0, 1], got {ratio!r}")
        if not _positive32(floor):
            raise ValueError(f"floor must be positive (and finite in fp32), got {floor!r}")
        if ceil is not None:
            ceil = _finite("ceil", ceil)
            if not _positive32(ceil) or np.float32(ceil) < np.float32(floor):
                raise ValueError(f"ceil must be None or finite and >= floor = {floor!r}, got {ceil!r}")
        return super().__new__(cls, ratio, floor, ceil)


def check_threshold(threshold):
    """``threshold`` if it is None, an ``X0Clip`` or an ``X0Threshold``, else ValueError."""
    if threshold is not None and not isinstance(threshold, (X0Clip, X0Threshold)):
        raise ValueError(f"threshold must be None, an X0Clip or an X0Threshold, got {type(threshold).__name__}")
    return threshold


def threshold_rank(ratio, n):
    """The 0-based rank floor(ratio (n - 1)) of the ``interpolation="lower"`` quantile among n values, formed here in double
    precision: the device receives an integer rank and never a ratio."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"n must be a positive integer, got {n!r}")
    ratio = _finite("ratio", ratio)
    if not 0 < ratio <= 1:
        raise ValueError(f"ratio must be in (0, 1], got {ratio!r}")
    return min(int(np.floor(ratio * (int(n) - 1))), int(n) - 1)


def inpaint_coefficients(seq, alpha, eta=0.0, guidance=0.0, prediction="eps"):
    """Per-iteration scalars of ``inpaint_steps``: float64 [n_iter, 9] in execution order (reversed ``seq``), columns
    (t, s1 = sqrt(1-at), s2 = sqrt(at), s3 = sqrt(at_next), c2, c1, k1, k2, zeta).  Columns 0-5 are ``ddim_coefficients``;
    k1 = -2 s1/s2 and k2 = 2/s2 split the gradient of the masked residual norm through the x0 prediction (k1 scales the
    backward's seed, k2 the direct term), formed in double precision like the other columns; zeta is ``guidance`` -- one float
    for every iteration or one value per iteration in execution order, each finite and >= 0.  ``prediction="v"``: the network
    predicts v and x0 = s2 x - s1 v, so k1 = -2 s1 (the seed is then the gradient w.r.t. the network's output v) and k2 = 2 s2;
    every other column is unchanged."""
    check_prediction(prediction)
    base = ddim_coefficients(seq, alpha, eta)
    n = base.shape[0]
    z = np.asarray(guidance, dtype=np.float64)
    if z.ndim == 0:
        z = np.full(n, float(z))
    elif z.ndim != 1 or z.shape[0] != n:
        raise ValueError(f"guidance: one float or one value per iteration ({n}), got shape {tuple(z.shape)}")
    if not np.isfinite(z).all() or (z < 0).any():
        raise ValueError("guidance values must be finite and >= 0")
    s1, s2 = base[:, 1], base[:, 2]
    k1, k2 = (-2.0 * s1, 2.0 * s2) if prediction == "v" else (-2.0 * s1 / s2, 2.0 / s2)
    return np.concatenate([base, k1[:, None], k2[:, None], z[:, None]], axis=1)


def _table64(alpha):
    return torch.as_tensor(alpha).to("cpu", torch.float32).numpy().astype(np.float64)


def logsnr_seq(alpha, timesteps):
    """Timestep subsequence spaced uniformly in half-log-SNR, lam[t] = 0.5 log(a_t / (1 - a_t)) (float64 from the fp32 table):
    for each of ``timesteps`` targets between lam[T-1] and lam[0] the t whose lam is nearest (ties: the smaller t); the distinct
    values in increasing order, as Python ints.  0 and T-1 are always present.  Near t = 0 neighbouring targets can round to the
    same t, so the result may be SHORTER than ``timesteps`` (audio.yml: 50 -> 49).  The step grid for ``dpm_coefficients``: on
    ``make_seq``'s uniform grid the last steps are huge in log-SNR and a higher order loses to DDIM."""
    a = _table64(alpha)
    if isinstance(timesteps, bool) or not isinstance(timesteps, (int, np.integer)) or timesteps < 2:
        raise ValueError(f"timesteps must be an integer >= 2, got {timesteps!r}")
    if a.ndim != 1 or a.size < 2 or not ((a > 0) & (a < 1)).all():
        raise ValueError("alpha must be a 1-D alphas-cumprod table with at least two entries inside (0, 1)")
    lam = 0.5 * np.log(a / (1.0 - a))
    targets = np.linspace(lam[-1], lam[0], int(timesteps))
    return sorted({int(np.argmin(np.abs(lam - v))) for v in targets})  # argmin: the first (smallest t) of equal distances


def dpm_coefficients(seq, alpha, order=2, tau=0.0):
    """Per-iteration scalars of ``dpm_solver_steps``: float64 [n_iter, 8] in execution order (reversed ``seq``), columns
    (t, s1, s2, s3, c2, c1, w1, w2).  With ``tau`` = 0 columns 0-5 are ``ddim_coefficients(seq, alpha, 0.0)`` bit for bit (c1 = 0);
    w1, w2 weight the history of x0 predictions (m0 this iteration's, m1 and m2 those of the two before):

        x_next = [s3 m0 + c2 eps] + w1 (m0 - m1) + w2 (m1 - m2) + c1 z,    m0 = (x - s1 eps) / s2.

    DPM-Solver++ multistep, data-prediction form (Lu et al. 2022), regrouped around the DDIM update, which is its first-order
    term: with lam the half-log-SNR, h = lam_next - lam_cur, h0 and h1 the two previous step sizes, r0 = h0 / h, r1 = h1 / h,
    phi1 = expm1(-h), phi2 = phi1 / h + 1, phi3 = phi2 / h - 1/2, A = s3:
      order 2:  w1 = -A phi1 / (2 r0), w2 = 0;
      order 3:  w1 = [A phi2 (1 + r0 / (r0 + r1)) - A phi3 / (r0 + r1)] / r0,  w2 = [-A phi2 r0 / (r0 + r1) + A phi3 / (r0 + r1)] / r1.
    Iteration k (0-based) runs at order min(order, k + 1); a final row that ends at a_next = 1 (the jump to t = -1, h infinite) is
    always order 1, so the last sample is the network's x0 prediction as in ``generalized_steps``.  Rows of lower order carry
    w = 0.

    ``tau`` > 0 is SDE-DPM-Solver++ (the same paper's appendix; "DPM++ 2M SDE" / "3M SDE"): every step but the final jump adds
    c1 z, z a standard normal, and contracts the sample by e^(-tau h) more.  The first-order term is the DDIM update with a
    per-step eta, ``ddim_coefficients``' own expressions (at the level left, an the level reached):
      eta_k = sqrt(expm1(-2 tau h) / expm1(-2 h))                    exactly 0 at tau = 0 and exactly 1 at tau = 1
      c1 = eta_k sqrt((1 - at / an) (1 - an) / (1 - at))             = sigma_n sqrt(1 - e^(-2 tau h))
      c2 = sqrt((1 - an) - c1^2)                                     = sigma_n e^(-tau h)
    so at tau = 1 columns 0-5 are ``ddim_coefficients(seq, alpha, 1.0)`` bit for bit, and the x coefficient c2 / s1 is
    (sigma_n / sigma_t) e^(-tau h), the data coefficient s3 - c2 s2 / s1 is alpha_n (1 - e^(-(1 + tau) h)).  The history weights
    are the formulas above with h replaced by (1 + tau) h inside phi1, phi2, phi3 only (r0, r1 stay ratios of plain h).  The
    final row has c1 = c2 = w1 = w2 = 0 for every tau.  Order 3 with noise is unstable on coarse grids: use about 20 steps or more.

    c2 is formed as that difference because the bit contracts need it; it cancels where e^(-2 tau h) is small, so c2 carries a
    relative error of a few 2^-53 e^(2 tau h): below 1e-12 on ``logsnr_seq`` grids at tau <= 2, about 5e-10 on the last step (h = 3.5)
    of ``make_seq(1000, 10)`` at tau = 2 -- far inside fp32, which is what the kernels receive.

    Raises ValueError for ``tau`` not a finite number >= 0 (checked first), an order outside {1, 2, 3}, a ``seq`` that is empty,
    not integers, not strictly increasing or outside the table, or a ``tau`` so large that for some step e^(-2 tau h) is below
    2^-52 (one ulp of 1: c2 would be rounding error only) or c2 does not come out finite."""
    tau = _finite("tau", tau)
    if tau < 0:
        raise ValueError(f"tau must be >= 0, got {tau!r}")
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or order not in (1, 2, 3):
        raise ValueError(f"order must be 1, 2 or 3, got {order!r}")
    a = _table64(alpha)
    seq = list(seq)
    if not seq:
        raise ValueError("seq is empty")
    if any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) for t in seq):
        raise ValueError("seq must hold integers")
    if seq[0] < 0 or seq[-1] >= a.size:
        raise ValueError(f"seq entries must lie in 0..{a.size - 1}")
    if any(q <= p for p, q in zip(seq, seq[1:])):
        raise ValueError("seq must be strictly increasing")
    base = ddim_coefficients(seq, alpha, 0.0)
    af = a.tolist()  # Python doubles, as ``ddim_coefficients`` takes them from the table
    seq_next = [-1] + seq[:-1]
    w = np.zeros((len(seq), 2), dtype=np.float64)
    lams = []  # half-log-SNR of the levels visited so far
    for k, (i, j) in enumerate(zip(reversed(seq), reversed(seq_next))):
        lam_s = 0.5 * np.log(a[i] / (1.0 - a[i]))
        p = 1 if j < 0 else min(int(order), k + 1)
        if j >= 0 and (tau > 0 or p >= 2):
            lam_t = 0.5 * np.log(a[j] / (1.0 - a[j]))
            h = lam_t - lam_s
        if j >= 0 and tau > 0:
            at, an = af[i], af[j]
            if not np.exp(-2.0 * tau * h) >= 2.0 ** -52:  # below one ulp of 1: 1 - e^(-2 tau h) is 1, c2 only rounding error
                raise ValueError(f"tau = {tau!r}: e^(-2 tau h) is below 2^-52 for the step {i} -> {j}, so c2 would keep nothing "
                                 "of the sample but rounding error")
            eta_k = float((np.expm1(-2.0 * tau * h) / np.expm1(-2.0 * h)) ** 0.5)
            c1 = eta_k * ((1 - at / an) * (1 - an) / (1 - at)) ** 0.5
            c2 = ((1 - an) - c1 ** 2) ** 0.5
            if isinstance(c2, complex) or not np.isfinite(c2) or not np.isfinite(c1):
                raise ValueError(f"tau = {tau!r}: c2 is not finite for the step {i} -> {j}")
            base[k, 4], base[k, 5] = c2, c1
        if p >= 2:
            ht = (1.0 + tau) * h  # inside the phi functions only
            r0 = (lam_s - lams[-1]) / h
            A, phi1 = base[k, 3], np.expm1(-ht)
            if p == 2:
                w[k, 0] = -0.5 * A * phi1 / r0
            else:
                r1 = (lams[-1] - lams[-2]) / h
                phi2 = phi1 / ht + 1.0
                phi3 = phi2 / ht - 0.5
                w[k, 0] = (A * phi2 * (1.0 + r0 / (r0 + r1)) - A * phi3 / (r0 + r1)) / r0
                w[k, 1] = (-A * phi2 * r0 / (r0 + r1) + A * phi3 / (r0 + r1)) / r1
        lams.append(lam_s)
    return np.concatenate([base, w], axis=1)


UNIC_STRIDE = _lib.DDIMXU_STRIDE  # floats per row of ``unic_coefficients``


def unic_coefficients(seq, alpha, order=2):
    """Per-iteration scalars of ``dpm_solver_steps(corrector=True)``: float64 [n_iter, 9] in execution order, columns
    (t, s1, s2, s3, c2, c1, w1', w2', w3).  Columns 0-5 are ``dpm_coefficients(seq, alpha, order, 0.0)`` bit for bit; the update is

        x_next = [s3 m0 + c2 eps] + w1' (m0 - m1) + w2' (m1 - m2) + w3 (m2 - m3),    m0 = (x - s1 eps) / s2.

    DPM-Solver++ with the UniC corrector of UniPC (Zhao et al. 2023), data-prediction form, B(h) = h ("bh1"), folded into one
    update.  UniC takes the prediction m0 the next step needs anyway, made at the predicted sample x, and corrects x with it:
    with lam[k] the half-log-SNR of iteration k's level, h' = lam[k] - lam[k-1] the step that produced x, hh = -h',
    q = min(order, k) the corrector's order, nodes r_j = (lam[k-1-j] - lam[k-1]) / h' for j < q and r_q = 1,
    g_1 = expm1(hh) / hh - 1, g_{i+1} = g_i / hh - 1 / (i+1)!, b_i = g_i i! / hh and rho the solution of
    sum_j r_j^(i-1) rho_j = b_i, i = 1..q (rho = 1/2 at q = 1),

        x_c = (sigma_k / sigma_{k-1}) x_c,prev - alpha_k expm1(-h') m1
              - alpha_k hh [sum_{j<q} rho_j (m_{1+j} - m1) / r_j + rho_q (m0 - m1)].

    x is the predictor's step from x_c,prev, so x_c - x is linear in the differences d0 = m0 - m1, d1 = m1 - m2, d2 = m2 - m3:
    with A = s2[k] h', a0 = A rho_q; each j < q adds -A rho_j / r_j to a_1 .. a_j; and a1, a2 lose the history weights w1, w2
    the previous predictor step had added (``dpm_coefficients``' row k - 1).  The predictor is linear in its sample with the
    coefficient g = c2 / s1, so predicting from x_c instead of x is the plain row plus g (x_c - x):

        w1' = w1 + g a0,    w2' = w2 + g a1,    w3 = g a2.

    The corrected sample is never formed, the network still sees the predictor's sample, and each evaluation is used twice: the
    order of accuracy goes up by one at no extra forward.  Order 1 has w1' only, order 2 w1' and w2', order 3 all three.  Row 0
    (nothing to correct yet) and the final jump to t = -1 (g = 0: the last sample is the network's x0 prediction) are
    ``dpm_coefficients``' rows with w3 = 0.  Raises what ``dpm_coefficients(seq, alpha, order)`` raises, in its order."""
    c = dpm_coefficients(seq, alpha, order, 0.0)
    a = _table64(alpha)
    levels = list(reversed(list(seq)))
    lam = [0.5 * np.log(a[t] / (1.0 - a[t])) for t in levels]
    out = np.concatenate([c, np.zeros((c.shape[0], 1), dtype=np.float64)], axis=1)
    for k in range(1, len(levels) - 1):  # the last row is the jump to t = -1
        q = min(int(order), k)
        hp = lam[k] - lam[k - 1]
        hh = -hp
        r = np.array([(lam[k - 1 - j] - lam[k - 1]) / hp for j in range(1, q)] + [1.0])
        b, gi, fact = [], np.expm1(hh) / hh - 1.0, 1.0
        for i in range(1, q + 1):
            fact *= i
            b.append(gi * fact / hh)
            gi = gi / hh - 1.0 / (fact * (i + 1))
        rho = np.array([0.5]) if q == 1 else np.linalg.solve(np.vander(r, q, increasing=True).T, np.array(b))
        A = c[k, 2] * hp
        d = np.zeros(3, dtype=np.float64)
        d[0] = A * rho[q - 1]
        for j in range(1, q):
            d[1:j + 1] += -A * rho[j - 1] / r[j - 1]
        d[1] -= c[k - 1, 6]
        d[2] -= c[k - 1, 7]
        g = c[k, 4] / c[k, 1]
        out[k, 6] = c[k, 6] + g * d[0]
        out[k, 7] = c[k, 7] + g * d[1]
        out[k, 8] = g * d[2]
    return out


INPAINT_SOLVER_STRIDE = _lib.DDIMXI_STRIDE  # floats per row of ``inpaint_solver_coefficients``


def inpaint_solver_coefficients(seq, alpha, order=2, tau=0.0, guidance=0.0, prediction="eps"):
    """Per-iteration scalars of ``inpaint_solver_steps``: float64 [n_iter, 13] in execution order (reversed ``seq``), columns
    (t, s1, s2, s3, c2, c1, k1, k2, rho, cx, w0, w1, w2).  Columns 0-5, w1 and w2 are ``dpm_coefficients(seq, alpha, order, tau)``
    bit for bit; k1 and k2 are ``inpaint_coefficients``' for ``prediction`` (they split the gradient of the masked residual norm
    through the data prediction); rho is ``guidance`` -- one float for every iteration or one value per iteration in execution
    order, each finite and >= 0.  cx = c2 / s1 and w0 = s3 - c2 s2 / s1 are the coefficients of x_t and of the data prediction in
    the step's first-order term once eps is eliminated,

        s3 m + c2 eps = cx x_t + w0 m,    eps = (x_t - s2 m) / s1,

    which is the exact solution of the sampler's ODE / SDE over the step for a constant data prediction m: cx =
    (sigma_n / sigma_t) e^(-tau h), w0 = alpha_n (1 - e^(-(1 + tau) h)) (``dpm_coefficients``).  The sampler moves the known region
    along it with m = y, and w0 is what a change of the prediction -- the guidance's -- is worth in x_{t-1}.  The final row
    (c2 = 0, s3 = 1) has cx = 0 and w0 = 1.  Every column is formed in float64.  Raises what ``dpm_coefficients`` and
    ``inpaint_coefficients`` raise."""
    base = dpm_coefficients(seq, alpha, order, tau)
    known = inpaint_coefficients(seq, alpha, 0.0, guidance, prediction)  # k1, k2 depend on (s1, s2) alone: any eta
    s1, s2, s3, c2 = base[:, 1], base[:, 2], base[:, 3], base[:, 4]
    cx = c2 / s1
    w0 = s3 - c2 * s2 / s1
    return np.concatenate([base[:, :6], known[:, 6:9], cx[:, None], w0[:, None], base[:, 6:8]], axis=1)


def guidance_per_step(seq, alpha, rho, tau=0.0):
    """The ``inpaint_steps(guidance=[...])`` list that applies the guidance ``inpaint_solver_steps(guidance=rho)`` applies at order
    1: rho w0_i per iteration in execution order, float64 (``rho``: one float or one value per iteration).  The folded form moves
    the data prediction by -(rho / sqrt(L)) g, which moves x_{t-1} by w0 times that; ``inpaint_steps`` subtracts (zeta / sqrt(L)) g
    from x_{t-1} directly.  At ``tau`` > 0 the list belongs to the first-order sampler with the same per-step noise
    (``dpm_coefficients``' c1, c2), which ``inpaint_steps``' one eta does not express unless tau = 1 (eta = 1)."""
    c = inpaint_solver_coefficients(seq, alpha, 1, tau, rho)
    return c[:, 8] * c[:, 10]


BROWNIAN_MAX_DEPTH = _lib.DDIMXB_MAX_DEPTH  # the deepest tree a plan row holds: tables of up to 2^16 timesteps
BROWNIAN_STRIDE = _lib.DDIMXB_PLAN_STRIDE  # 32-bit words per row of ``brownian_plan``: 4 + 2 * (BROWNIAN_MAX_DEPTH + 1) * 4
ENTER_ANCHOR, ENTER_ROOT, ENTER_LEFT, ENTER_RIGHT = (_lib.DDIMXB_ENTER_ANCHOR, _lib.DDIMXB_ENTER_ROOT, _lib.DDIMXB_ENTER_LEFT,
                                                     _lib.DDIMXB_ENTER_RIGHT)  # a record's ``enter``


def brownian_clock(alpha, tau):
    """(u, D, T) of the Brownian path of ``noise.BrownianStream``: with T = len(alpha), D = max(1, ceil(log2 T))
    and N = 2^D, u is float64 [N + 1]: u[t] = exp(2 tau lam[t]) = (a_t / (1 - a_t))^tau for t < T (lam the half-log-SNR, float64 from
    the fp32 table) and 0 for T <= t <= N.  The noise a sampler accumulates from level i to level j is sigma_j u_j^(-1/2)
    [W(u_j) - W(u_i)] for one Brownian motion W on this clock.  ValueError for a ``tau`` that is not finite and > 0, a table that is
    not 1-D inside (0, 1) and non-increasing, or one longer than 2^BROWNIAN_MAX_DEPTH."""
    tau = _finite("tau", tau)
    if tau <= 0:
        raise ValueError(f"the Brownian path needs tau > 0, got {tau!r}")
    a = _table64(alpha)
    if a.ndim != 1 or a.size < 1 or not ((a > 0) & (a < 1)).all() or (np.diff(a) > 0).any():
        raise ValueError("alpha must be a non-increasing 1-D alphas-cumprod table inside (0, 1)")
    depth = max(1, int(a.size - 1).bit_length())
    if depth > BROWNIAN_MAX_DEPTH:
        raise ValueError(f"a table of {a.size} timesteps needs a tree of depth {depth} > {BROWNIAN_MAX_DEPTH}")
    u = np.zeros((1 << depth) + 1, dtype=np.float64)
    u[:a.size] = np.exp(2.0 * tau * (0.5 * np.log(a / (1.0 - a))))
    if not np.isfinite(u).all():
        raise ValueError(f"tau = {tau!r}: the clock (a / (1 - a))^tau is not finite")
    return u, depth, int(a.size)


def brownian_descent(u, depth, t):
    """The records [(node id, rho, s, enter)] (float64 rho, s) of the descent to point t, 0 <= t < 2^depth, of the tree over
    ``brownian_clock``'s u: the anchor (node 0: P(0) = sqrt(u[0]) xi_0, P(N) = 0), then from the root (node 1, [0, N]) the nodes
    whose interval [a, b] holds t, each giving its midpoint m = (a + b) / 2 as the Brownian bridge
    P(m) = P(b) + rho (P(a) - P(b)) + s xi_node,  rho = (u_m - u_b) / (u_a - u_b),  s = sqrt((u_a - u_m)(u_m - u_b) / (u_a - u_b))
    (both 0 where u_a = u_b), down to the node with m = t; the children of node n are 2n: [a, m] and 2n + 1: [m, b]."""
    recs = [(0, 0.0, float(np.sqrt(u[0])), ENTER_ANCHOR)]
    a, b, node, enter = 0, 1 << depth, 1, ENTER_ROOT
    while t != 0:
        m = (a + b) // 2
        ua, um, ub = float(u[a]), float(u[m]), float(u[b])
        span = ua - ub
        rho, s = ((um - ub) / span, float(np.sqrt((ua - um) * (um - ub) / span))) if span > 0 else (0.0, 0.0)
        recs.append((node, rho, s, enter))
        if t == m:
            break
        a, b, node, enter = (a, m, 2 * node, ENTER_LEFT) if t < m else (m, b, 2 * node + 1, ENTER_RIGHT)
    return recs


def brownian_row(clock, i, j):
    """One plan row (int32 [BROWNIAN_STRIDE], the fp32 fields as their bits; include/ddimx_brownian.h) of the step from level i to
    level j < i on ``clock`` (``brownian_clock``'s result): the number of leading records the two descents share, their lengths, g = 1 / sqrt(u_j - u_i), the records of the
    descent to i, then of the descent to j.  ``i`` None: the descent to j alone (what ``BrownianStream.path`` evaluates), g = 0.
    ValueError unless 0 <= j < i < T and u_j - u_i > 0 in fp32."""
    u, depth, n_real = clock
    ints = [v for v in (i, j) if v is not None]
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in ints) or any(not 0 <= v < n_real for v in ints):
        raise ValueError(f"timesteps must be integers in 0..{n_real - 1}, got {ints!r}")
    row = np.zeros(BROWNIAN_STRIDE, dtype=np.int32)
    f32 = row.view(np.float32)
    rj = brownian_descent(u, depth, int(j))
    ri = []
    if i is not None:
        if not j < i:
            raise ValueError(f"the step {i} -> {j} does not go down")
        with np.errstate(divide="ignore"):
            g = np.float32(1.0 / np.sqrt(u[j] - u[i]))
        if not np.float32(u[j]) - np.float32(u[i]) > 0 or not np.isfinite(g):
            raise ValueError(f"u_j - u_i is not positive in fp32 for the step {i} -> {j}")
        ri = brownian_descent(u, depth, int(i))
        f32[3] = g
    share = 0
    while share < min(len(ri), len(rj)) and ri[share][0] == rj[share][0]:
        share += 1
    row[0], row[1], row[2] = share, len(ri), len(rj)
    for base, recs in ((4, ri), (4 + 4 * (BROWNIAN_MAX_DEPTH + 1), rj)):
        for r, (node, rho, s, enter) in enumerate(recs):
            k = base + 4 * r
            row[k], f32[k + 1], f32[k + 2], row[k + 3] = node, rho, s, enter
    return row


def brownian_plan(seq, alpha, tau):
    """What ``ddimxb_multistep_update`` walks beside ``dpm_coefficients(seq, alpha, order, tau)``: int32 [n_iter, BROWNIAN_STRIDE],
    row k the ``brownian_row`` of iteration k's step from level i = reversed(seq)[k] to the level j it reaches.  A row whose c1 is 0
    -- the final jump to t = -1, and every row at ``tau`` = 0 -- is empty (all zero): no noise.  With these rows the z of a step is
    [W(u_j) - W(u_i)] / sqrt(u_j - u_i): a unit normal, independent of the z of every other step of the run, and the increments of
    adjacent steps add up to the increment of the step across them -- so runs of any step count follow one path.
    Validation is ``dpm_coefficients``' own, then ``brownian_clock``'s and ``brownian_row``'s (u_j - u_i > 0 in fp32)."""
    coef = dpm_coefficients(seq, alpha, 1, tau)
    plan = np.zeros((coef.shape[0], BROWNIAN_STRIDE), dtype=np.int32)
    if float(tau) > 0:
        clock = brownian_clock(alpha, tau)
        levels = list(reversed(list(seq)))
        for k, (i, j) in enumerate(zip(levels, levels[1:])):
            if coef[k, 5] != 0:
                plan[k] = brownian_row(clock, int(i), int(j))
    return plan


INVERT_MAX_ITERS = 16 # fixed-point iterations per level of ``invert_coefficients``


def invert_coefficients(seq, alpha, iters=1):
    """Per-evaluation scalars of ``invert_steps``: float64 [len(seq) * iters, 6], one row per network evaluation in execution
    order (``seq`` upwards, ``iters`` rows per level), columns (t, s1_i, s2_i, p, q, first).  Level i = seq[k], the level below
    it j = seq[k-1], and j = -1 (alphas-cumprod 1, the data) for k = 0.  The decoder's step from i down to j
    (``ddim_coefficients``, eta = 0) is

        x_j = s3_j (x_i - s1_i e) / s2_i + c2_j e,    s1 = sqrt(1-a_i), s2 = sqrt(a_i), s3_j = sqrt(a_j), c2_j = sqrt(1-a_j);

    solved for x_i with e held fixed it is x_i = p x_j + q e with p = s2_i / s3_j = sqrt(a_i / a_j) and q = s1_i - p c2_j, formed
    in Python double precision from the fp32 table like the other tables (a level that starts from the data has p = s2_i,
    q = s1_i exactly).  The ``iters`` rows of a level are equal but for ``first``: 1.0 on the first of them (the update keeps its
    input as the level's base point then), 0.0 on the others.  Raises ValueError for ``iters`` not an integer in 1..16 (checked
    before anything else) or a ``seq`` that is empty, not integers, not strictly increasing or outside the table."""
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 1 <= iters <= INVERT_MAX_ITERS:
        raise ValueError(f"iters must be an integer in 1..{INVERT_MAX_ITERS}, got {iters!r}")
    a = [1.0] + torch.as_tensor(alpha).to("cpu", torch.float32).numpy().tolist()
    seq = list(seq)
    if not seq:
        raise ValueError("seq is empty")
    if any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) for t in seq):
        raise ValueError("seq must hold integers")
    if seq[0] < 0 or seq[-1] >= len(a) - 1:
        raise ValueError(f"seq entries must lie in 0..{len(a) - 2}")
    if any(q <= p for p, q in zip(seq, seq[1:])):
        raise ValueError("seq must be strictly increasing")
    rows = []
    for i, j in zip(seq, [-1] + seq[:-1]):
        at, at_below = a[int(i) + 1], a[int(j) + 1]
        s1, s2 = (1 - at) ** 0.5, at ** 0.5
        p = s2 / at_below ** 0.5
        q = s1 - p * (1 - at_below) ** 0.5
        for m in range(int(iters)):
            rows.append((float(int(i)), s1, s2, p, q, 1.0 if m == 0 else 0.0))
    return np.asarray(rows, dtype=np.float64).reshape(-1, 6)


WINDOW_MAX_COVER = _lib.DDIMX_WINDOW_MAX_COVER  # the most windows that may cover one canvas row (the update kernel's unrolled loads)
WindowPlan = collections.namedtuple("WindowPlan", "W K jfirst cnt wt")


def _window_int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return int(v)


def window_plan(L, T, H, taper="tri"):
    """Host plan of ``windowed_steps``: a canvas of ``L`` rows cut into W = (L - T) / H + 1 windows of ``T`` rows at hop ``H``,
    window j covering the rows [j H, j H + T).  Returns ``WindowPlan(W, K, jfirst, cnt, wt)``: K = ceil(T / H), the most windows
    that cover one row; per canvas row l the first covering window ``jfirst[l]`` and the number of covering windows ``cnt[l]``
    (int32 [L]); and their normalised weights ``wt[k][l]`` (float32 [K, L], k = 0 .. cnt - 1 in ascending window order, zero
    beyond): w(l - j H) / sum over the covering windows j' of w(l - j' H), formed in float64 and rounded once to fp32, with the
    taper w(tau) = 1 (``"flat"``) or min(tau + 1, T - tau) (``"tri"``).  A row that one window covers carries exactly 1.0.
    Raises ValueError naming the argument for a non-integer or non-positive size, H outside 1..T, L < T or (L - T) % H != 0,
    K > 8 or an unknown taper."""
    L, T, H = _window_int("L", L), _window_int("window", T), _window_int("hop", H)
    if T < 1:
        raise ValueError(f"window = {T} must be positive")
    if not 1 <= H <= T:
        raise ValueError(f"hop = {H} outside 1..window ({T})")
    K = -(-T // H)
    if K > WINDOW_MAX_COVER:
        raise ValueError(f"hop = {H}: ceil(window / hop) = {K} windows would cover one row (at most {WINDOW_MAX_COVER})")
    if L < T or (L - T) % H:
        raise ValueError(f"L = {L}: the canvas must hold whole windows, L = window + (W - 1) hop ({T} + (W - 1) {H})")
    if taper not in ("flat", "tri"):
        raise ValueError(f"taper must be 'flat' or 'tri', got {taper!r}")
    W = (L - T) // H + 1
    rows = np.arange(L, dtype=np.int64)
    jfirst = np.maximum(0, -(-(rows - T + 1) // H))  # the smallest j with j H + T > l
    jlast = np.minimum(W - 1, rows // H)             # the largest j with j H <= l
    cnt = jlast - jfirst + 1
    raw = np.zeros((K, L), dtype=np.float64)
    for k in range(K):
        tau = rows - (jfirst + k) * H
        w = np.ones(L) if taper == "flat" else np.minimum(tau + 1, T - tau).astype(np.float64)
        raw[k] = np.where(k < cnt, w, 0.0)
    wt = (raw / raw.sum(axis=0)).astype(np.float32)
    return WindowPlan(W, K, jfirst.astype(np.int32), cnt.astype(np.int32), wt)


LOSS_WEIGHTS = ("uniform", "min_snr", "trunc_snr")


def loss_weight_table(alphas, prediction, kind, gamma=5.0):
    """Per-timestep weight of the squared-error loss: float64 [len(alphas)], or None for ``"uniform"``.  Formed like ``v_table``,
    from the fp32 table's values taken as Python doubles; SNR = a / (1 - a).

        kind          prediction="eps"       prediction="v"
        "min_snr"     min(1, gamma / SNR)    min(SNR, gamma) / (SNR + 1)      (Hang et al. 2023)
        "trunc_snr"   max(1, 1 / SNR)        max(SNR, 1) / (SNR + 1)          (max(SNR, 1) in x0 space: Salimans & Ho 2022)

    Each column is the x0-space weight divided by the factor that turns the squared x0 error into the squared error of that
    prediction (SNR for eps, SNR + 1 for v).  Raises ValueError for an unknown kind or prediction, for ``gamma`` not finite or
    <= 0, and for a table entry outside (0, 1)."""
    check_prediction(prediction)
    if kind not in LOSS_WEIGHTS:
        raise ValueError(f"loss weight must be one of {LOSS_WEIGHTS}, got {kind!r}")
    gamma = float(gamma)
    if not np.isfinite(gamma) or gamma <= 0:
        raise ValueError(f"gamma must be finite and > 0, got {gamma!r}")
    a = torch.as_tensor(alphas).to("cpu", torch.float32).reshape(-1).numpy().tolist()
    if not a or not all(0.0 < at < 1.0 for at in a):
        raise ValueError("alphas must be a non-empty alphas-cumprod table with every entry inside (0, 1)")
    if kind == "uniform":
        return None
    w = []
    for at in a:
        snr = at / (1 - at)
        if prediction == "eps":
            w.append(min(1.0, gamma / snr) if kind == "min_snr" else max(1.0, 1.0 / snr))
        else:
            w.append((min(snr, gamma) if kind == "min_snr" else max(snr, 1.0)) / (snr + 1))
    return np.asarray(w, dtype=np.float64)


DISTILL_STRIDE = _lib.DDIMX_DISTILL_STRIDE  # floats per row of ``distill_coefficients``


def _check_teacher_seq(teacher_seq, n_table):
    seq = list(teacher_seq)
    if len(seq) < 2 or len(seq) % 2:
        raise ValueError(f"teacher_seq must have an even length >= 2, got {len(seq)}")
    if any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) for t in seq):
        raise ValueError("teacher_seq must hold integers")
    if n_table is not None and (seq[0] < 0 or seq[-1] >= n_table):
        raise ValueError(f"teacher_seq entries must lie in 0..{n_table - 1}")
    if seq[0] < 0:
        raise ValueError("teacher_seq entries must not be negative")
    if any(q <= p for p, q in zip(seq, seq[1:])):
        raise ValueError("teacher_seq must be strictly increasing")
    return [int(t) for t in seq]


def halve_seq(teacher_seq):
    """The student's timestep sequence of one round of progressive distillation: ``teacher_seq[1::2]``.  Student step k goes
    S[2k+1] -> S[2k-1] (-1, the data, for k = 0) where the teacher goes S[2k+1] -> S[2k] -> S[2k-1].  ``teacher_seq``: an even
    number >= 2 of strictly increasing non-negative ints, else ValueError."""
    return _check_teacher_seq(teacher_seq, None)[1::2]


def distill_coefficients(teacher_seq, alphas, student_prediction="eps"):
    """Per-student-step scalars of ``distill_target``: float64 [N, 12] for a teacher sequence S of length 2N, row k (student step
    k: t = S[2k+1], t' = S[2k], t'' = S[2k-1] or the data) =

        (t, s1, s2, s3, c2, t', s1', s2', omega, cz, cx, 0)

    with alpha = sqrt(a), sigma = sqrt(1 - a): s1 = sigma_t, s2 = alpha_t, s3 = alpha_t', c2 = sigma_t' -- the first five are the
    eta = 0 row of ``ddim_coefficients`` for t -> t', formed the same way (Python doubles from the fp32 table) -- s1' = sigma_t',
    s2' = alpha_t'; omega = A / (A + B) with A = (sigma''/sigma') alpha' - (sigma''/sigma) alpha and B = alpha'' - (sigma''/sigma')
    alpha', the weight of the teacher's first x0 prediction in the student's x0 target x = m1 + omega (m0 - m1) (0 <= omega < 0.5,
    and 0 at k = 0 where sigma'' = 0); and (cz, cx), which turn x into the student's training target cz z + cx x:
    (1/sigma, -alpha/sigma) for an eps student, (alpha/sigma, -1/sigma) for a v student.  Raises ValueError for a sequence that is
    not an even number >= 2 of strictly increasing ints inside the table, or an unknown prediction."""
    check_prediction(student_prediction)
    a = [1.0] + torch.as_tensor(alphas).to("cpu", torch.float32).reshape(-1).numpy().tolist()
    seq = _check_teacher_seq(teacher_seq, len(a) - 1)
    rows = []
    for k in range(len(seq) // 2):
        t, tm, tl = seq[2 * k + 1], seq[2 * k], (seq[2 * k - 1] if k else -1)
        at, am, al = a[t + 1], a[tm + 1], a[tl + 1]
        s1, s2 = (1 - at) ** 0.5, at ** 0.5
        s3, c2 = am ** 0.5, ((1 - am) - 0.0 ** 2) ** 0.5  # ddim_coefficients with c1 = 0
        s1m, s2m = (1 - am) ** 0.5, am ** 0.5
        sl, xl = (1 - al) ** 0.5, al ** 0.5
        A = (sl / s1m) * s2m - (sl / s1) * s2
        B = xl - (sl / s1m) * s2m
        omega = A / (A + B)
        cz, cx = (1.0 / s1, -s2 / s1) if student_prediction == "eps" else (s2 / s1, -1.0 / s1)
        rows.append((float(t), s1, s2, s3, c2, float(tm), s1m, s2m, omega, cz, cx, 0.0))
    return np.asarray(rows, dtype=np.float64).reshape(-1, DISTILL_STRIDE)


CONSISTENCY_STRIDE = _lib.CMX_STRIDE  # floats per row of ``consistency_coefficients``


def _consistency_alphas(alphas):
    a = torch.as_tensor(alphas).to("cpu", torch.float32).reshape(-1).numpy().tolist()
    if not a or not all(0.0 < at < 1.0 for at in a):
        raise ValueError("alphas must be a non-empty alphas-cumprod table with every entry inside (0, 1)")
    return a


def _check_consistency_seq(seq, n_table, what="seq"):
    """``seq`` as a list of strictly increasing ints inside 0 .. n_table - 1, at least one."""
    seq = list(seq)
    if not seq:
        raise ValueError(f"{what} must not be empty")
    if any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) for t in seq):
        raise ValueError(f"{what} must hold integers")
    if seq[0] < 0 or seq[-1] >= n_table:
        raise ValueError(f"{what} entries must lie in 0..{n_table - 1}")
    if any(q <= p for p, q in zip(seq, seq[1:])):
        raise ValueError(f"{what} must be strictly increasing")
    return [int(t) for t in seq]


def consistency_table(alphas, prediction, sigma_data=0.5, timestep_scale=10.0, t_min=0):
    """The table of the consistency kernels (include/cmx_consistency.h): float64 [len(alphas), 2], row t = (p, q) with
    f(x, t) = p x + q out the consistency function of a network whose raw output is ``out``; the callers round it to fp32.

    The parametrisation is the discrete-time one of Luo et al. 2023 (latent consistency models) of Song et al. 2023: with
    u = timestep_scale max(t - t_min, 0), c_skip = sigma_data^2 / (u^2 + sigma_data^2) and c_out = u / sqrt(u^2 + sigma_data^2),
    f = c_skip x + c_out x0_hat, x0_hat the network's data prediction.  With a = sqrt(abar_t), sigma = sqrt(1 - abar_t) (Python
    doubles from the fp32 table, as ``v_table`` forms them):

        prediction="eps"   x0_hat = (x - sigma out) / a     p = c_skip + c_out / a     q = -c_out sigma / a
        prediction="v"     x0_hat = a x - sigma out         p = c_skip + c_out a       q = -c_out sigma

    Every row t <= t_min is (1, 0): f(x, t_min) = x, the boundary condition.  An eps student amplifies its output error at high
    noise by sigma / a -- on the audio schedule (p, q) = (157.41, -157.41) at t = 999 against (0.0064, -1.0000) for v -- so a v
    student is the one to distil for 1-2 step sampling.  ValueError for an unknown prediction, ``sigma_data`` or
    ``timestep_scale`` not positive and finite, ``t_min`` no integer inside the table, or a table entry outside (0, 1)."""
    check_prediction(prediction)
    a = _consistency_alphas(alphas)
    sd, ks = _finite("sigma_data", sigma_data), _finite("timestep_scale", timestep_scale)
    if sd <= 0 or ks <= 0:
        raise ValueError(f"sigma_data and timestep_scale must be positive, got {sigma_data!r} and {timestep_scale!r}")
    if isinstance(t_min, bool) or not isinstance(t_min, (int, np.integer)) or not 0 <= t_min < len(a):
        raise ValueError(f"t_min must be an integer in 0..{len(a) - 1}, got {t_min!r}")
    rows = []
    for t, at in enumerate(a):
        if t <= t_min:
            rows.append((1.0, 0.0))
            continue
        u = ks * (t - int(t_min))
        c_skip, c_out = sd * sd / (u * u + sd * sd), u / (u * u + sd * sd) ** 0.5
        al, sg = at ** 0.5, (1 - at) ** 0.5
        rows.append((c_skip + c_out / al, -c_out * sg / al) if prediction == "eps" else (c_skip + c_out * al, -c_out * sg))
    return np.asarray(rows, dtype=np.float64).reshape(-1, 2)


def consistency_pairs(seq, alphas, skip=1, t_min=0):
    """The teacher's steps of consistency distillation on the student levels ``seq`` = S[0..N-1] (strictly increasing ints,
    S[0] = ``t_min``): (rows, t_hi, t_lo) with rows float64 [N - skip, DISTILL_STRIDE] in ``ddimxd_distill_half``'s layout, row n
    the eta = 0 DDIM step t_hi = S[n + skip] -> t_lo = S[n],

        (t_hi, sigma_hi, alpha_hi, alpha_lo, sigma_lo, t_lo, sigma_lo, alpha_lo, 0, 0, 0, 0)

    -- columns 0-4 are the row of ``ddim_coefficients((t_lo, t_hi), alphas)`` for t_hi, formed the same way -- and t_hi, t_lo the
    int64 arrays of the two levels per index n.  ValueError for a sequence that is not strictly increasing ints inside the table,
    ``seq[0] != t_min``, or ``skip`` outside 1..N-1."""
    a = _consistency_alphas(alphas)
    seq = _check_consistency_seq(seq, len(a))
    if seq[0] != t_min:
        raise ValueError(f"seq[0] = {seq[0]} must be t_min = {t_min!r}: the level at which the consistency function is the identity")
    if isinstance(skip, bool) or not isinstance(skip, (int, np.integer)) or not 1 <= skip <= len(seq) - 1:
        raise ValueError(f"skip must be an integer in 1..{len(seq) - 1} (N - 1), got {skip!r}")
    rows = []
    for n in range(len(seq) - skip):
        at, al = a[seq[n + skip]], a[seq[n]]
        s1, s2, s3, c2 = (1 - at) ** 0.5, at ** 0.5, al ** 0.5, ((1 - al) - 0.0 ** 2) ** 0.5  # ddim_coefficients with c1 = 0
        rows.append((float(seq[n + skip]), s1, s2, s3, c2, float(seq[n]), (1 - al) ** 0.5, al ** 0.5, 0.0, 0.0, 0.0, 0.0))
    return (np.asarray(rows, dtype=np.float64).reshape(-1, DISTILL_STRIDE), np.asarray(seq[skip:], dtype=np.int64),
            np.asarray(seq[:len(seq) - skip], dtype=np.int64))


def consistency_coefficients(seq, alphas, prediction, **table_kw):
    """Per-iteration rows of ``consistency_steps`` (``cmx_consistency_update``): float64 [len(seq), CONSISTENCY_STRIDE] in execution
    order (reversed ``seq``), the row of seq[i] =

        (t, p, q, alpha_next, 0, sigma_next, 0, 0)

    with (p, q) = ``consistency_table(alphas, prediction, **table_kw)[t]`` and (alpha_next, sigma_next) those of seq[i - 1], the
    level the step re-noises its data prediction to; the row of seq[0], the last one, is final: (t, p, q, 1, 0, 0, 0, 0).  Columns
    0 and 5 sit where ``DDIMStepper`` looks for the timestep and the noise coefficient.  ``seq``: strictly increasing ints inside
    the table, every entry > t_min; else ValueError (and ``consistency_table``'s)."""
    tab = consistency_table(alphas, prediction, **table_kw)
    a = _consistency_alphas(alphas)
    seq = _check_consistency_seq(seq, len(a))
    t_min = table_kw.get("t_min", 0)
    if seq[0] <= t_min:
        raise ValueError(f"every seq entry must be > t_min = {t_min} (the consistency function is the identity there)")
    rows = []
    for i in reversed(range(len(seq))):
        t = seq[i]
        an, sn = (a[seq[i - 1]] ** 0.5, (1 - a[seq[i - 1]]) ** 0.5) if i else (1.0, 0.0)
        rows.append((float(t), tab[t, 0], tab[t, 1], an, 0.0, sn, 0.0, 0.0))
    return np.asarray(rows, dtype=np.float64).reshape(-1, CONSISTENCY_STRIDE)


LKX_STRIDE = _lib.LKX_STRIDE  # floats per row of ``likelihood_coefficients``
LIKELIHOOD_ORDERS = (1, 2)

LikelihoodTable = collections.namedtuple("LikelihoodTable", "rows wd trace_per_dim logdet_per_dim")


def likelihood_coefficients(seq, alphas, order=2, prediction="eps"):
    """The rows of ``likelihood.log_likelihood`` (include/features/lkx_likelihood.h): one per network evaluation of the
    probability-flow ODE du/ds = eps(alpha u, t) in u = x / alpha, s = sigma / alpha, walked UP the increasing levels ``seq``
    from seq[0] to seq[-1].  With (alpha_i, sigma_i) = (sqrt(abar), sqrt(1 - abar)) of level seq[i] (Python doubles from the
    fp32 table, as ``v_table`` forms them), s_i = sigma_i / alpha_i and h = s_{i+1} - s_i, interval i gives

        order=1 (Euler)   (t_i,     0,   h,   alpha_{i+1}, h alpha_i,       COMMIT)
        order=2 (Heun)    (t_i,     0,   h,   alpha_{i+1}, h alpha_i / 2,   SAVE)            the predictor, k1 <- e
                          (t_{i+1}, h/2, h/2, alpha_{i+1}, h alpha_{i+1}/2, COMMIT)          the trapezoid on (k1, e)

    as float64 rows (t, wk, we, a_next, wd, flags, 0, 0) of ``LKX_STRIDE``; the callers round them to fp32 (t < 2^24 is exact).
    For ``prediction="v"`` the backward is seeded with the gradient w.r.t. v, eps = s1 x + s2 v, so r . J_eps^T r =
    s1 D + s2 (r . g): every wd carries the factor s2 of its row's t and the s1 part is a constant of the table.

    Returns ``LikelihoodTable(rows, wd, trace_per_dim, logdet_per_dim)``: ``wd`` the float64 column 4, which ``lkx_finish`` reads
    instead of the fp32 row; ``trace_per_dim`` = the sum over the rows of (wd without its s2) s1 -- times D it is what the v
    network's identity part adds to the integral, 0.0 for eps; ``logdet_per_dim`` = log(alpha_T / alpha_0) -- times D the
    change-of-variables term.  ValueError for ``seq`` not strictly increasing ints inside the table or shorter than 2, an order
    outside (1, 2), an unknown prediction, a table entry outside (0, 1)."""
    check_prediction(prediction)
    if isinstance(order, bool) or order not in LIKELIHOOD_ORDERS:
        raise ValueError(f"order must be 1 (Euler) or 2 (Heun), got {order!r}")
    a = _consistency_alphas(alphas)
    seq = _check_consistency_seq(seq, len(a))
    if len(seq) < 2:
        raise ValueError("seq needs at least 2 levels: the ODE runs from seq[0] to seq[-1]")
    if seq[-1] >= 1 << 24:
        raise ValueError("seq entries must lie below 2^24 (a row stores t as fp32)")
    al = [a[t] ** 0.5 for t in seq]
    sg = [(1 - a[t]) ** 0.5 for t in seq]
    s = [q / p for p, q in zip(al, sg)]
    s1s2 = (lambda i: (sg[i], al[i])) if prediction == "v" else (lambda i: (0.0, 1.0))
    rows, trace = [], 0.0
    for i in range(len(seq) - 1):
        h = s[i + 1] - s[i]
        stages = [(i, 0.0, h, h * al[i], float(_lib.LKX_COMMIT))] if order == 1 else \
            [(i, 0.0, h, 0.5 * h * al[i], float(_lib.LKX_SAVE)), (i + 1, 0.5 * h, 0.5 * h, 0.5 * h * al[i + 1], float(_lib.LKX_COMMIT))]
        for at, wk, we, w, flags in stages:
            s1, s2 = s1s2(at)
            trace += w * s1
            rows.append((float(seq[at]), wk, we, al[i + 1], w * s2, flags, 0.0, 0.0))
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, LKX_STRIDE)
    return LikelihoodTable(rows, rows[:, 4].copy(), trace, float(np.log(al[-1] / al[0])))
