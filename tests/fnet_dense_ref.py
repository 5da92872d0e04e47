"""fp64 references, layouts and case tables of the fused dense path of the FNet inference walk (csrc/fnet_dense.hip:
fnet_fold_kernel, fnet_table_kernel, fnet_dense_kernel, fnet_mix2_kernel), one kernel at a time (test infrastructure; no GPU, no
library).  Written from the layouts and formulas the kernel file documents in its comments, not from the kernels' code.

tests/test_fnet_dense_cpu.py checks this file against itself, torch.fft and oracle/ref_cpu.py; tests/test_gpu_fnet_dense.py
compares the kernels behind ddimx_fnet_fold / ddimx_fnet_table / ddimx_fnet_dense / ddimx_fnet_mix2 with these functions.

Layouts (a sample owns 32 row slots; rows >= S are padding, never written and never used):
  fragment order  bf16 [n / 32][k / 16][lane = 32 h + n % 32][8], k = 16 g + 8 h + i;  fp32 [n / 32][k / 8][lane][4], k = 8 g + 4 h + i
  chunk-major     fp32 [b][k / 4][32 rows][4];  bf16 [b][k / 8][32 rows][8]
  statistics      [b][part / 2][32 rows][(sum, m2) x 2]: per part of n_part consecutive elements its sum and CENTRED sum of squares

Two kinds of comparison, as in fnet_kernel_ref.py: exact (integers |v| <= 3, dyadic statistics, eps = 0: every intermediate is an
integer multiple of a power of two below 2^24 of it, so any fp32 or bf16-operand order gives the fp64 result bit for bit) and
gated (Gaussian operands: the fp32 gate, or in bf16 mode the yardstick of `bf16_yardstick`)."""
import math

import numpy as np
import torch

import exact_util as X
import gpu_util as G
from fnet_kernel_ref import LN_EPS, OPERAND_MAX, gaussian, gate, gelu_new, ints, layernorm, offset_gate  # noqa: F401

HID = 512                    # the only hidden size fnet_mix2 takes
S_EXACT = (1, 7, 8, 31, 32)  # tokens per sample of the dense cases: one, ragged, the mix kernel's minimum, one short of full, full
S_MIX = (8, 16, 24, 32)
MEAN_MAX = 2                 # |m| of the hand-made row means
OFFSET = 32.0                # mean of the offset rows (std 1)


def _ar(n):
    return torch.arange(n, dtype=torch.int64)


# ---- index maps (flat element positions) -----------------------------------------------------------------------------------------------
def frag_index(N, K, bf16):
    """Position of W[n][k] in fragment order; [N][K]."""
    E = 8 if bf16 else 4
    n, k = _ar(N)[:, None], _ar(K)[None, :]
    g, h, i = k // (2 * E), (k % (2 * E)) // E, k % E
    return (((n // 32) * (K // (2 * E)) + g) * 64 + 32 * h + n % 32) * E + i


def chunk_index(B, S, K, ch):
    """Position of x[b][s][k] in the chunk-major layout of `ch`-element chunks (4: fp32, 8: bf16); [B][S][K]."""
    b, s, k = _ar(B)[:, None, None], _ar(S)[None, :, None], _ar(K)[None, None, :]
    return b * 32 * K + ((k // ch) * 32 + s) * ch + k % ch


def rows_index(B, S, K):
    """Row-major [B*S][K]."""
    b, s, k = _ar(B)[:, None, None], _ar(S)[None, :, None], _ar(K)[None, None, :]
    return (b * S + s) * K + k


def stats_index(B, S, nparts):
    """Position of (sum, m2)[c] of part p of row s of sample b; [B][S][nparts][2]."""
    b, s, p, c = _ar(B)[:, None, None, None], _ar(S)[None, :, None, None], _ar(nparts)[None, None, :, None], _ar(2)[None, None, None, :]
    return b * nparts * 64 + ((p // 2) * 32 + s) * 4 + (p % 2) * 2 + c


def layout_index(layout, B, S, K):
    return {"row": rows_index(B, S, K), "c4": chunk_index(B, S, K, 4), "c8": chunk_index(B, S, K, 8)}[layout]


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
def part_stats(rows, nparts):
    """(sum, centred sum of squares) of `nparts` equal parts of the last dimension: [..., nparts, 2], in the dtype of `rows`."""
    v = rows.reshape(*rows.shape[:-1], nparts, rows.shape[-1] // nparts)
    s = v.sum(-1)
    m2 = (v - s[..., None] / v.shape[-1]).square().sum(-1)
    return torch.stack([s, m2], -1)


def fold(parts, n_part, eps=0.0):
    """Chan's combination of [..., nparts, 2] parts of n_part elements each: (mean, rstd) of the whole rows, in the dtype of `parts`."""
    s, pm = parts[..., 0], parts[..., 1]
    n_row = parts.shape[-2] * n_part
    mean = s.sum(-1) / n_row
    d = s / n_part - mean[..., None]
    m2 = (n_part * d * d + pm).sum(-1)
    return mean, 1.0 / torch.sqrt(m2 / n_row + eps)


def fold2(parts, n_part, eps=0.0):
    """The fold with the mean kept in two parts, as fnet_mix2 takes it: hi = the mean of part 0, lo = the mean of the parts'
    differences from part 0; (hi, lo, rstd) with mean = hi + lo, in the dtype of `parts`."""
    s, pm = parts[..., 0], parts[..., 1]
    n_row = parts.shape[-2] * n_part
    hi = s[..., 0] / n_part
    lo = (s - s[..., :1]).sum(-1) / n_row
    d = (s / n_part - hi[..., None]) - lo[..., None]
    m2 = (n_part * d * d + pm).sum(-1)
    return hi, lo, 1.0 / torch.sqrt(m2 / n_row + eps)


def dyadic_stats(tag, B, S, nparts, n_part, kind):
    """Hand-made statistics [B][S][nparts][2] (fp64) whose fold is exactly (mean m, rstd 2^-k), m an integer |m| <= 2, k in {0, +-1}.
    'uniform': every part is (n_part m, n_part 4^k).  'between': k in {0, 1}, the parts of the first half of the row have mean
    m + a, those of the second half m - a, a = 2^(k-1), so the sums cancel around m and the between-part term n_part d^2 carries
    a^2 of the variance 4^k = a^2 + c; the within-part term carries the rest, pm = n_part c with c = 3 a^2.
    Returns (stats, mean [B][S], rstd [B][S])."""
    m = X.dyadic(tag + ".m", (B, S), MEAN_MAX, 0)
    if kind == "uniform":
        k = X.dyadic(tag + ".k", (B, S), 1, 0)
        st = torch.stack([n_part * m, n_part * 4.0 ** k], -1)[:, :, None, :].expand(B, S, nparts, 2).clone()
    else:
        k = X.dyadic(tag + ".k", (B, S), 1, 0).abs()
        a = 2.0 ** (k - 1)
        sign = torch.where(_ar(nparts) < nparts // 2, 1.0, -1.0).double()
        mp = m[..., None] + a[..., None] * sign
        st = torch.stack([n_part * mp, (n_part * 3.0 * a * a)[..., None].expand(B, S, nparts)], -1)
    return st, m, 2.0 ** -k


# ---- the operations --------------------------------------------------------------------------------------------------------------------
def bf16r(v):
    """fp64 -> nearest-even bf16 value, kept in fp64 (0 stays 0)."""
    return torch.where(v == 0, v, X.rne(v.double(), 8))


def dense(W, bias, x, stats=None, act=0, R=None, rstats=None, rgamma=None, rbeta=None, bf16=False, round_tokens=True):
    """out[b][t][n] = act(sum_k W[n][k] xf(x[b][t][k]) + bias[n]) (+ LN(R)[b][t][n] rgamma[n] + rbeta[n]) in fp64.
    stats / rstats: (mean, rstd) [B][S] of the rows of x / R, or None (xf = identity).  bf16: W and (round_tokens) the operand
    xf(x) are rounded to bf16 before the product; everything else stays fp64."""
    v = x.double()
    if stats is not None:
        v = (v - stats[0].double()[..., None]) * stats[1].double()[..., None]
    w = W.double()
    if bf16:
        w = bf16r(w)
        if round_tokens:
            v = bf16r(v)
    o = torch.einsum("bsk,nk->bsn", v, w) + bias.double()
    if act:
        o = gelu_new(o)
    if R is not None:
        o = o + (R.double() - rstats[0].double()[..., None]) * rstats[1].double()[..., None] * rgamma.double() + rbeta.double()
    return o


def _mix_input(V, stats, gamma, beta):
    v = V.double()
    if stats is None:
        return v, v
    n = (v - stats[0].double()[..., None]) * stats[1].double()[..., None]
    return n, n * gamma.double() + beta.double()


def mix2_fft(V, stats=None, gamma=None, beta=None):
    """Re(FFT2(X)) + X over [B][S][H], X = LN(V) gamma + beta from (mean, rstd) `stats`, or V."""
    _, x = _mix_input(V, stats, gamma, beta)
    return torch.fft.fftn(x, dim=(1, 2)).real + x


def mix2_table(V, tab, dseq, stats=None, gamma=None, beta=None, bc=None):
    """The same in the two-stage table form: U = T N^T with T [2H][H] (row 2j: cos_j gamma, 2j + 1: sin_j gamma) and N the
    normalised rows of V (or V), then [C | -S] U with dseq [S][2S], + S bc on row 0, + X.  Any tables (integer ones too)."""
    n, x = _mix_input(V, stats, gamma, beta)
    S = V.shape[1]
    U = torch.einsum("rh,bsh->brs", tab.double(), n)             # [B][2H][S]
    d = dseq.double()
    t = torch.einsum("ps,bjs->bpj", d[:, :S], U[:, 0::2]) + torch.einsum("ps,bjs->bpj", d[:, S:], U[:, 1::2])
    if stats is not None:
        t[:, 0, :] += S * bc.double()
    return t + x


def _trig(n, round32):
    k = np.arange(n, dtype=np.int64)
    ang = 2.0 * np.pi * ((k[:, None] * k[None, :]) % n).astype(np.float64) / n
    c, s = np.cos(ang), np.sin(ang)
    if round32:
        c, s = c.astype(np.float32).astype(np.float64), s.astype(np.float32).astype(np.float64)
    return torch.from_numpy(c), torch.from_numpy(s)


def table(gamma, beta, H, round32=True):
    """(tab [2H][H], bc [H] or None): row 2j = cos(2 pi j h / H) gamma[h], row 2j + 1 = sin(2 pi j h / H) gamma[h] (gamma None: 1),
    bc[j] = sum_h cos(2 pi j h / H) beta[h]; the argument reduced exactly mod H, fp64 trigonometry rounded once to fp32 (round32)
    as model.py::_dft_tables does, the products and sums in fp64."""
    c, s = _trig(H, round32)
    tab = torch.stack([c, s], 1).reshape(2 * H, H)
    if gamma is not None:
        tab = tab * gamma.double()
    return tab, None if beta is None else c @ beta.double()


def dft_seq(S, round32=True):
    """[S][2S] = [cos | -sin]."""
    c, s = _trig(S, round32)
    return torch.cat([c, -s], 1)


def fold_weights(W, gamma, beta, bias):
    """(W diag(gamma), bias + W beta) in fp64; gamma None: W, beta None: no bias."""
    w = W.double()
    return (w if gamma is None else w * gamma.double()), (None if beta is None else bias.double() + w @ beta.double())


# ---- the launcher's acceptance rules ---------------------------------------------------------------------------------------------------
def fnet_dense_supported(S, K, N):
    return 1 <= S <= 32 and K % 512 == 0 and N % 64 == 0 and K >= 512


def dense_args(S, K, N, x="c4", xnp=0, xn=0, rnp=0, rn=0, out="c4", ostats=False, **_):
    """The launcher-relevant fields of an argument block from a case's description."""
    return dict(S=S, K=K, N=N, xstats=xnp > 0, xnp=xnp, xn=xn, x_chunk=x != "row", x_bf16=x == "c8", out_chunk=out != "row",
                out_bf16=out == "c8", res=rnp > 0, rnp=rnp, rn=rn, ostats=ostats)


def dense_dispatch(a, bf16):
    """The kernel instantiation (PREC, TXB, TOB, WF, KS, XF, XL, GP, RES) fnet_dense_launch picks for `a` (dense_args), or None
    where it returns an error."""
    if not fnet_dense_supported(a["S"], a["K"], a["N"]):
        return None
    if a["xstats"] and (a["xnp"] > 32 or a["xnp"] % 4 or a["xn"] < 1 or not a["x_chunk"]):
        return None
    deep = a["K"] >= 4 * a["N"] or a["K"] > 1024
    KS = 8 if deep else 4
    if a["res"] and (a["rnp"] % 8 or not 1 <= a["rnp"] // 8 <= 4):
        return None
    if a["ostats"] and (a["N"] // 32) % 2:
        return None
    if (a["x_bf16"] and not a["x_chunk"]) or (a["out_bf16"] and not a["out_chunk"]):
        return None
    kw = a["K"] // KS

    def inst(prec, txb, tob, xf, xl, gp, res):
        return None if (kw // (16 if prec else 8)) % gp else (prec, txb, tob, 1, KS, xf, xl, gp, res)

    xf, res = a["xstats"], a["res"]
    if bf16:
        if not deep:
            if not xf or a["x_bf16"] or res:
                return None
            return inst(1, False, a["out_bf16"], 1, 1, 8, False)
        if a["out_bf16"] or xf:
            return None
        if a["x_bf16"]:
            return inst(1, True, False, 0, 1, 16, res)
        if not a["x_chunk"] and not res:
            return inst(1, False, False, 0, 0, 8, False)
        return None if res else inst(1, False, False, 0, 1, 8, False)
    if a["out_bf16"] or a["x_bf16"]:
        return None
    if not deep:
        return None if (not xf or res) else inst(0, False, False, 1, 1, 16, False)
    if xf:
        return None
    if a["x_chunk"]:
        return inst(0, False, False, 0, 1, 16, res)
    return None if res else inst(0, False, False, 0, 0, 16, False)


def mix2_accepts(S, hid):
    return hid == 512 and 8 <= S <= 32 and S % 8 == 0


def run_fnet_args(S, bf, hid=512, inter=2048, width=2048):
    """The argument sets run_fnet builds: projection, ffn1, ffn2, compute_out (bf: the walk's bf16 mode)."""
    c8 = "c8" if bf else "c4"
    return {
        "projection": dense_args(S, width, hid, x="c4", out="c4"),
        "ffn1": dense_args(S, hid, inter, x="c4", xnp=hid // 16, xn=16, out=c8),
        "ffn2": dense_args(S, inter, hid, x=c8, rnp=hid // 16, rn=16, out="c4", ostats=True),
        "compute_out": dense_args(S, hid, width, x="c4", xnp=hid // 32, xn=32, out="row"),
    }


# ---- case tables -----------------------------------------------------------------------------------------------------------------------
def dense_case(K, N, S, x="c4", xnp=0, rnp=0, out="c4", ostats=False, stat="uniform", act=0, offset=0.0, tag=""):
    name = f"K{K}-N{N}-S{S}-x{x}" + (f"-xnp{xnp}" if xnp else "") + (f"-rnp{rnp}" if rnp else "") + f"-o{out}" + \
        ("-ostats" if ostats else "") + (f"-{stat}" if xnp or rnp else "") + ("-gelu" if act else "") + ("-offset" if offset else "") + tag
    return dict(name=name, K=K, N=N, S=S, x=x, xnp=xnp, xn=K // xnp if xnp else 0, rnp=rnp, rn=N // rnp if rnp else 0, out=out,
                ostats=ostats, stat=stat, act=act, offset=offset)


def _dense_exact():
    c, it = [], [0]

    def nxt():  # S and the statistics kind cycle over the flag combinations, so that every route meets every S
        it[0] += 1
        return S_EXACT[it[0] % 5], ("uniform", "between")[(it[0] // 5) % 2]

    # every S x both statistics sets on one argument set per route
    for S in S_EXACT:
        for st in ("uniform", "between"):
            c.append(dense_case(512, 256, S, xnp=32, ostats=True, stat=st))            # wide, normalised operand
            c.append(dense_case(2048, 512, S, rnp=32, ostats=True, stat=st))           # deep, LN(R) residual (fp32 tokens: fp32 path)
            c.append(dense_case(2048, 64, S, x="c8", rnp=8, out="row", stat=st))       # deep, bf16 tokens (bf16 path)
        c.append(dense_case(2048, 64, S, x="row", out="row"))                          # deep, row-major tokens (XL = 0)
    # wide: every statistics geometry x every output form
    for xnp in (4, 8, 16, 32):
        for out, ostats in (("row", False), ("row", True), ("c4", False), ("c4", True), ("c8", False)):
            S, st = nxt()
            c.append(dense_case(512, 256, S, xnp=xnp, out=out, ostats=ostats, stat=st))
    for out, ostats in (("row", False), ("c4", True), ("c8", False)):
        S, st = nxt()
        c.append(dense_case(1024, 512, S, xnp=32, out=out, ostats=ostats, stat=st))
    # deep: token layouts x residual geometries x output forms
    for N, rnps in ((64, (8, 16)), (192, (24,)), (512, (32,))):
        for x in ("row", "c4", "c8"):
            for rnp in (0,) + (rnps if x != "row" else ()):
                for out, ostats in (("row", False), ("c4", True)) + ((("row", True), ("c4", False)) if N == 64 else ()):
                    S, st = nxt()
                    c.append(dense_case(2048, N, S, x=x, rnp=rnp, out=out, ostats=ostats, stat=st))
    return list({d["name"]: d for d in c}.values())  # (the combinations walk meets some of the sweep's cases again)


DENSE_EXACT = _dense_exact()

DENSE_GAUSS = [
    dense_case(512, 256, 7, xnp=32, out="c4", ostats=True),
    dense_case(512, 256, 7, xnp=32, out="c4", act=1),
    dense_case(512, 256, 31, xnp=16, out="row", act=1, offset=OFFSET),
    dense_case(512, 256, 8, xnp=32, out="c8", act=1),                                   # bf16 path only
    dense_case(512, 256, 8, xnp=32, out="c8", offset=OFFSET),
    dense_case(2048, 512, 7, x="c4", rnp=32, out="c4", ostats=True),                    # fp32 path only
    dense_case(2048, 512, 7, x="c4", rnp=32, out="c4", ostats=True, act=1, offset=OFFSET),
    dense_case(2048, 512, 7, x="c8", rnp=32, out="c4", ostats=True),                    # bf16 path only
    dense_case(2048, 512, 31, x="c8", rnp=32, out="row", act=1, offset=OFFSET),
    dense_case(2048, 64, 7, x="row", out="row", act=1),
    dense_case(2048, 512, 32, x="c4", out="c4", ostats=True),                           # the projection's argument set
]
# ostats of a deep launch feed xstats of a wide one (16 parts of 32)
CHAIN = (dense_case(2048, 512, 7, x="c4", out="c4", ostats=True, tag="-chain0"), dense_case(512, 256, 7, xnp=16, out="row", act=1, tag="-chain1"))

FOLD_CASES = ((32, 16), (96, 48), (64, 512), (512, 2048))
TABLE_H = (32, 64, 512)


def dense_operands(case, kind, B=3):
    """The logical operands of a dense case, fp64 tensors holding fp32-exact (x = 'c8': bf16-exact) values:
    W [N][K], bias, X [B][S][K], xstats [B][S][xnp][2] and their fold xfold = (mean, rstd), R, rstats, rfold, rgamma, rbeta; eps.
    kind 'exact': integers, hand-made dyadic statistics, eps 0; 'gauss': N(0, 1) rows (+ offset for the normalised operand and
    R), W / sqrt(K), the statistics of the rows themselves rounded to fp32, eps = LN_EPS."""
    t = case["name"] + "." + kind
    K, N, S = case["K"], case["N"], case["S"]
    o = dict(eps=0.0 if kind == "exact" else LN_EPS, xstats=None, xfold=None, R=None, rstats=None, rfold=None, rgamma=None, rbeta=None)
    f32 = lambda v: v.float().double()  # noqa: E731
    if kind == "exact":
        o.update(W=ints(t + "W", (N, K)), bias=ints(t + "b", (N,)), X=ints(t + "X", (B, S, K)))
        if case["xnp"]:
            o["xstats"], m, r = dyadic_stats(t + "xs", B, S, case["xnp"], case["xn"], case["stat"])
            o["xfold"] = (m, r)
        if case["rnp"]:
            o.update(R=ints(t + "R", (B, S, N)), rgamma=ints(t + "rg", (N,)), rbeta=ints(t + "rb", (N,)))
            o["rstats"], m, r = dyadic_stats(t + "rs", B, S, case["rnp"], case["rn"], case["stat"])
            o["rfold"] = (m, r)
        return o
    o.update(W=f32(gaussian(t + "W", (N, K)) / math.sqrt(K)), bias=f32(0.3 * gaussian(t + "b", (N,))))
    x = gaussian(t + "X", (B, S, K))
    if case["xnp"]:
        x = x + case["offset"]
    o["X"] = bf16r(x) if case["x"] == "c8" else f32(x)
    if case["xnp"]:
        o["xstats"] = f32(part_stats(o["X"], case["xnp"]))
        o["xfold"] = fold(o["xstats"], case["xn"], o["eps"])
    if case["rnp"]:
        o.update(R=f32(gaussian(t + "R", (B, S, N)) + case["offset"]), rgamma=f32(1.0 + 0.3 * gaussian(t + "rg", (N,))),
                 rbeta=f32(0.2 * gaussian(t + "rb", (N,))))
        o["rstats"] = f32(part_stats(o["R"], case["rnp"]))
        o["rfold"] = fold(o["rstats"], case["rn"], o["eps"])
    return o


def dense_want(case, o, bf16=False, round_tokens=True):
    return dense(o["W"], o["bias"], o["X"], o["xfold"], case["act"], o["R"], o["rfold"], o["rgamma"], o["rbeta"], bf16, round_tokens)


def errors(got, want, std=None):
    """(max, rms) of got - want in units of the std of `want` (or `std`)."""
    d = got.double().reshape(-1) - want.double().reshape(-1)
    s = (float(want.double().std()) if std is None else float(std)) + 1e-30
    return float(d.abs().max()) / s, float(d.square().mean().sqrt()) / s


def bf16_yardstick(rounded, unrounded):
    """The gate of the bf16 path: the (max, rms) error, in units of the std of the reference, that rounding the token operand to
    bf16 causes in the reference itself (both with bf16-rounded weights).  A kernel that multiplies the same rounded operands differs
    from `rounded` only by its fp32 accumulation and by roundings that flip, which the rounding itself bounds."""
    return errors(unrounded, rounded)


def out_rounding(want):
    """(max, rms) error, in units of the std of `want`, of rounding `want` itself to bf16: what a bf16 OUTPUT adds to any gate."""
    return errors(bf16r(want), want)


def dense_gate(case, o, bf16):
    """(reference, (max, rms) gate) of a Gaussian dense case (the CPU test checks that fp32 arithmetic meets it).
    fp32 path: the project's fp32 gate; for offset rows `offset_gate` of those rows (the larger of the fp32 gate and 8 x the error
    of CPU fp32 F.layer_norm).  bf16 path: the yardstick (fnet_dense_ref.bf16_yardstick); where the tokens are stored in bf16
    nothing is rounded and only the fp32 accumulation differs, so the fp32 gate applies.  A bf16 output adds its own rounding."""
    want = dense_want(case, o, bf16)
    tol = (1e-4, 2e-5)
    assert tol == (G.TOL[G.F32]["mx"], G.TOL[G.F32]["rms"])
    if case["offset"]:
        rows = o["X"] if case["xnp"] else o["R"]
        n = rows.shape[-1]
        tol = offset_gate(rows.reshape(-1, n), torch.ones(n), torch.zeros(n))[0]
    if bf16 and case["x"] != "c8":
        y = bf16_yardstick(want, dense_want(case, o, True, round_tokens=False))
        tol = (max(tol[0], y[0]), max(tol[1], y[1])) if case["offset"] else y
    if case["out"] == "c8":
        r = out_rounding(want)
        tol = (tol[0] + r[0], tol[1] + r[1])
    return want, tol


# ---- exactness budgets -----------------------------------------------------------------------------------------------------------------
XF_MAX, XF_GRID = (OPERAND_MAX + MEAN_MAX) * 2, 1   # |(x - m) 2^-k| <= 10 on the grid 2^-1 (k = 1)


def budget_bits(case):
    """Bits the largest intermediate of an exact dense case needs, in units of its grid: K products of a weight and a (normalised)
    token, the bias, and the residual (R - m) 2^-k rgamma + rbeta."""
    xmax, p = (XF_MAX, XF_GRID) if case["xnp"] else (OPERAND_MAX, 0)
    extra = OPERAND_MAX
    if case["rnp"]:
        extra += XF_MAX * OPERAND_MAX + OPERAND_MAX
        p = XF_GRID
    return X.budget_bits(case["K"], xmax, p, OPERAND_MAX, 0, extra=extra)


def m2_check(got, rows, nparts, grid_log2, what):
    """A kernel's (sum, m2) statistics `got` [..][nparts][2] against the exact ones of `rows` (fp64, multiples of 2^grid_log2).
    Sums: exact.  m2: d = v - sum / n_part lies on the grid 2^grid_log2 / n_part and every partial sum of the d^2 is a multiple of
    that grid squared, so where the total needs fewer than 24 bits of it any order is exact; otherwise an fp32 sum of n_part
    (<= 32) non-negative terms is within 32 * 2^-24 * sum |terms|.  Returns the number of m2 entries held to exactness."""
    want = part_stats(rows.double(), nparts)
    n_part = rows.shape[-1] // nparts
    got = got.double()
    assert torch.equal(got[..., 0], want[..., 0]), f"{what}: part sums differ"
    unit = (2.0 ** grid_log2 / n_part) ** 2
    exact = want[..., 1] / unit < 2.0 ** 24
    assert torch.equal(got[..., 1][exact], want[..., 1][exact]), f"{what}: m2 differs where its budget makes it exact"
    d = (got[..., 1] - want[..., 1]).abs()
    assert bool((d <= 32 * 2.0 ** -24 * want[..., 1]).all()), f"{what}: m2 off by more than 32 * 2^-24 * sum of terms"
    return int(exact.sum())


# ---- fnet_mix2 cases -------------------------------------------------------------------------------------------------------------------
TAB_NNZ, SEQ_NNZ = 4, 2  # non-zeros per row of the integer tables


def sparse_ints(tag, rows, cols, nnz):
    """[rows][cols] with `nnz` entries of +-1 per row at pseudo-random columns, else 0."""
    g = torch.Generator().manual_seed(int.from_bytes(tag.encode(), "little") % (2 ** 31))
    t = torch.zeros(rows, cols, dtype=torch.float64)
    for r in range(rows):
        cols_r = torch.randperm(cols, generator=g)[:nnz]
        t[r, cols_r] = (torch.randint(0, 2, (nnz,), generator=g) * 2 - 1).double()
    return t


def mix2_exact_operands(S, norm, B=3, stat="uniform"):
    """Integer case of fnet_mix2: sparse {0, +-1} tables in the tab [2H][H] and dft_seq [S][2S] positions, integer V, and with
    `norm` dyadic vstats (16 parts of 32), integer gamma / beta / bc."""
    t = f"mix2.S{S}.{int(norm)}.{stat}"
    o = dict(tab=sparse_ints(t + "tab", 2 * HID, HID, TAB_NNZ), dseq=sparse_ints(t + "seq", S, 2 * S, SEQ_NNZ), V=ints(t + "V", (B, S, HID)),
             vstats=None, vfold=None, gamma=None, beta=None, bc=None)
    if norm:
        o["vstats"], m, r = dyadic_stats(t + "vs", B, S, 16, HID // 16, stat)
        o.update(vfold=(m, r), gamma=ints(t + "g", (HID,)), beta=ints(t + "be", (HID,)), bc=ints(t + "bc", (HID,)))
    return o


def mix2_budget_bits(S, norm):
    """Largest |intermediate| of an exact mix2 case on its grid (2^-1 with the normalisation): stage 1, stage 2, + S bc, + X."""
    n, p = (XF_MAX, XF_GRID) if norm else (OPERAND_MAX, 0)
    t = TAB_NNZ * n * SEQ_NNZ + (S * OPERAND_MAX + n * OPERAND_MAX + OPERAND_MAX if norm else n)
    return math.log2(t * 2.0 ** p)


MIX2_MODES = ("plain", "norm", "norm-offset")


def mix2_real_case(S, mode):
    """A Gaussian case of fnet_mix2: (gamma, beta, producer) -- gamma / beta None for 'plain'.  With the normalisation V is the
    output of a dense launch (the projection's shape, 2048 -> 512, chunk-major, with ostats), producer = (its case, its operands);
    'norm-offset': that launch's bias is 32, so V has rows of mean 32 and std 1.  'plain': producer = V itself, N(0, 1)."""
    t = f"mix2real{S}.{mode}"
    if mode == "plain":
        return None, None, gaussian(t + "V", (3, S, HID)).float().double()
    gamma = (1.0 + 0.3 * gaussian(t + "g", (HID,))).float().double()
    beta = (0.2 * gaussian(t + "b", (HID,))).float().double()
    case = dense_case(2048, HID, S, x="c4", out="c4", ostats=True, tag=t)
    o = dense_operands(case, "gauss")
    if mode == "norm-offset":
        o["bias"] = o["bias"] + OFFSET
    return gamma, beta, (case, o)


# ---- the kernels composed as run_fnet composes them --------------------------------------------------------------------------------
def walk_params(tag, width, hid, inter, n_layers):
    """Gaussian weights of a Transformer_Module with non-trivial LayerNorm affines, fp32-exact values in fp64."""
    f32 = lambda v: v.float().double()  # noqa: E731
    ln = lambda t, n: (f32(1.0 + 0.3 * gaussian(t + "g", (n,))), f32(0.2 * gaussian(t + "b", (n,))))  # noqa: E731
    lin = lambda t, n, k: (f32(gaussian(t + "w", (n, k)) / math.sqrt(k)), f32(0.3 * gaussian(t + "b", (n,))))  # noqa: E731
    P = dict(ln0=ln(tag + "ln0", width), proj=lin(tag + "proj", hid, width), out=lin(tag + "out", width, hid), layers=[])
    for i in range(n_layers):
        t = f"{tag}L{i}"
        P["layers"].append(dict(ln1=ln(t + "ln1", hid), ffn1=lin(t + "f1", inter, hid), ffn2=lin(t + "f2", hid, inter), ln2=ln(t + "ln2", hid)))
    return P


def walk(P, h0, eps, bf16=False, round_tokens=True, final="out", round32=True, f32fold=False):
    """projection, L x (mix2, ffn1, ffn2), then compute_out (final 'out') or the next layer's mix2 (final 'mix'), each step one of
    the references above fed as run_fnet feeds the kernels: statistics as per-part pairs folded by `fold`, gamma / beta folded into
    weights, tables and S bc, the LayerNorm(Z) residual recomputed.  h0 [B][S][width]: the embedding LayerNorm's output.
    f32fold: folded weights and tables are rounded to fp32 as the pack-time kernels store them.  Returns every intermediate."""
    r32 = (lambda v: v.float().double()) if f32fold else (lambda v: v)
    S, hid = h0.shape[1], P["proj"][0].shape[0]
    dseq = dft_seq(S, round32)
    o = dict(v=[], z=[], h=[])
    v = dense(P["proj"][0], P["proj"][1], h0, bf16=bf16, round_tokens=round_tokens)
    vfold, prev = None, None

    def mix(v, vfold, prev):
        if prev is None:
            return mix2_table(v, table(None, None, hid, round32)[0], dseq)
        tab, bc = table(prev[0], prev[1], hid, round32)
        return mix2_table(v, r32(tab), dseq, vfold, prev[0], prev[1], r32(bc))

    for L in P["layers"]:
        o["v"].append(v)
        z = mix(v, vfold, prev)
        zfold = fold(part_stats(z, hid // 16), 16, eps)
        w1, b1 = fold_weights(L["ffn1"][0], L["ln1"][0], L["ln1"][1], L["ffn1"][1])
        h = dense(r32(w1), r32(b1), z, zfold, act=1, bf16=bf16, round_tokens=round_tokens)
        if bf16 and round_tokens:
            h = bf16r(h)  # (the walk stores the intermediate activations of the bf16 mode in bf16: the second matrix's tokens)
        v = dense(L["ffn2"][0], L["ffn2"][1], h, None, 0, z, zfold, L["ln1"][0], L["ln1"][1], bf16=bf16, round_tokens=round_tokens)
        vfold, prev = fold(part_stats(v, hid // 32), 32, eps), L["ln2"]
        o["z"].append(z)
        o["h"].append(h)
    o["v"].append(v)
    if final == "mix":
        o["final"] = mix(v, vfold, prev)
    else:
        w, b = fold_weights(P["out"][0], prev[0], prev[1], P["out"][1])
        o["final"] = dense(r32(w), r32(b), v, vfold, bf16=bf16, round_tokens=round_tokens)
    return o
