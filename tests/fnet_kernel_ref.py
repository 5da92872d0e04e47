"""fp64 references and case tables of the FNet bottleneck's kernels, one by one (test infrastructure; no GPU, no library).

tests/test_fnet_kernels_cpu.py checks this file against itself and against torch (autograd, F.layer_norm, the exactness budget of
tests/exact_util.py); tests/test_gpu_fnet_kernels.py parametrizes over the tables below and compares the kernels behind
ddimx_gemm_nt / ddimx_gemm_ln / ddimx_layernorm / ddimx_ln_train / ddimx_ln_bwd / ddimx_gelu / ddimx_transpose / ddimx_colsum /
ddimx_dropout_apply with these functions.

Two kinds of comparison:

* exact -- operands are small integers (``exact_util.dyadic``, |v| <= 3: exactly representable in bf16 as well), so every partial
  sum any kernel can form is an integer below 2^24 and ANY fp32 or bf16-operand summation order gives the fp64 result bit for bit;
* gated -- where a transcendental (tanhf, sqrtf and the division for rstd) or an inexact fp32 sum enters: the project's fp32 gate
  ``gpu_util.TOL[F32]``, max |d| <= 1e-4 and rms(d) <= 2e-5 in units of the std of the expected output (``gate``).
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import exact_util as X
import gpu_util as G

TILE_M, TILE_N = 64, 64      # workgroup tile of gemm_nt_kernel
BK = {0: 32, 1: 64}          # its K chunk, fp32 / bf16
LN_ROWS = 8                  # rows a block of ln_bwd_kernel walks
LN_EPS = 1e-12               # transformers FNetConfig.layer_norm_eps
OPERAND_MAX = 3              # |v| of every exact operand


def gaussian(tag, shape, dtype=torch.float64):
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    return torch.randn(shape, generator=g, dtype=torch.float64).to(dtype)


def ints(tag, shape):
    """Integers uniform in [-3, 3], fp64."""
    return X.dyadic(tag, shape, OPERAND_MAX, 0)


# ---- the gate ------------------------------------------------------------------------------------------------------------------------
def gate(got, want, what, std=None, tol=None):
    """``gpu_util.check_close(.., F32)`` with the unit made explicit: (max, rms) of got - want over `std` (default: the std of
    `want`, which is what check_close uses; a tensor of one element has none, so those cases pass the std of the tensor they are
    a slice of).  tol: (max, rms) instead of the fp32 gate."""
    got = torch.as_tensor(got, dtype=torch.float64).reshape(-1)
    want = torch.as_tensor(want, dtype=torch.float64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    s = (float(want.std()) if std is None else float(std)) + 1e-30
    d = got - want
    mx, rms = float(d.abs().max()) / s, float(d.square().mean().sqrt()) / s
    tmx, trms = (G.TOL[G.F32]["mx"], G.TOL[G.F32]["rms"]) if tol is None else tol
    assert mx <= tmx and rms <= trms, f"{what}: max {mx:.3e} rms {rms:.3e} (rel. to std) exceeds ({tmx:.3e}, {trms:.3e})"
    return mx, rms


# ---- gelu_new (transformers activations.py:59-66) ------------------------------------------------------------------------------------
_K, _A = math.sqrt(2.0 / math.pi), 0.044715


def gelu_new(v):
    return 0.5 * v * (1.0 + torch.tanh(_K * (v + _A * v ** 3)))


def dgelu_new(v):
    t = torch.tanh(_K * (v + _A * v ** 3))
    return 0.5 * (1.0 + t) + 0.5 * v * (1.0 - t * t) * _K * (1.0 + 3.0 * _A * v * v)


# ---- GEMM ----------------------------------------------------------------------------------------------------------------------------
def gemm(A, B, C0=None, bias=None, resid=None, act=0):
    """C[z] = (C0[z] +) A[z or 0] B[z]^T (+ bias) (gelu_new) (+ resid[z]);  A [1 or batch][M][K], B [batch][N][K], fp64 in and out
    (any dtype is widened first, so bf16-rounded operands enter with their rounded values)."""
    v = torch.einsum("zmk,znk->zmn", A.double().expand(B.shape[0], -1, -1), B.double())
    if C0 is not None:
        v = v + C0.double()
    if bias is not None:
        v = v + bias.double()
    if act:
        v = gelu_new(v)
    if resid is not None:
        v = v + resid.double()
    return v


def gemm_case(name, M, N, K, lda=None, ldb=None, ldc=None, batch=1, shared_a=False, pad_c=0, splitk=1, accumulate=0, bias=0, resid=0,
              a_off=0):
    """shared_a: one A for every batch entry (sA = 0); pad_c: floats between the batch entries of C (sC = M * ldc + pad_c);
    a_off: A starts that many floats past a 16-byte boundary."""
    return dict(name=name, M=M, N=N, K=K, lda=lda or K, ldb=ldb or K, ldc=ldc or N, batch=batch, shared_a=shared_a, pad_c=pad_c,
                splitk=splitk, accumulate=accumulate, bias=bias, resid=resid, a_off=a_off)


def _exact_cases():
    c = [
        # full tiles, both K-loop schedules: 4 fp32 / 2 bf16 chunks (all requested at once), 10 / 5 chunks (pipelined loop)
        gemm_case("full-prefetch", 64, 64, 128),
        gemm_case("full-pipelined", 64, 128, 320),
        # ragged M and N, aligned K
        gemm_case("ragged", 70, 50, 96),
        gemm_case("one", 1, 1, 32),
        # unaligned leading dimensions and K tails: scalar loads
        gemm_case("unaligned", 33, 65, 37),
        gemm_case("misaligned-base", 70, 50, 96, a_off=1),
    ]
    # the weight-gradient GEMMs at K = B * S of an odd batch of short clips (blocks.cpp, fnet_bwd_part: gemm(.., width, hid, M))
    c += [gemm_case(f"wgrad-K{k}", 96, 80, k) for k in (1, 3, 6, 15)]
    c += [
        gemm_case("bf16-ktail", 64, 64, 96),  # the second bf16 chunk is half empty
        gemm_case("padded-ld", 40, 72, 64, lda=68, ldb=72, ldc=75),
        # batched, as the two-GEMM Fourier path calls it: the DFT table shared by the samples, then the sequence transform + residual
        gemm_case("batched-shared-a", 128, 12, 64, batch=3, shared_a=True),
        gemm_case("batched-resid", 12, 128, 24, batch=3, shared_a=True, resid=1),
        gemm_case("batched-own-a", 12, 128, 24, batch=3, resid=1, pad_c=5),
    ]
    # epilogue matrix: in the GEMM kernel (splitk 1) and in the split-K reduce kernel (splitk 4)
    for sk in (1, 4):
        for acc in (0, 1):
            for bias in (0, 1):
                for resid in (0, 1):
                    c.append(gemm_case(f"epi-sk{sk}-acc{acc}-bias{bias}-resid{resid}", 40, 72, 512, splitk=sk, accumulate=acc, bias=bias,
                                       resid=resid))
    # split-K slices: K = 288 is 9 fp32 chunks -- 4 slices of 3 leave the last one empty; K = 64 has fewer chunks than slices
    c += [gemm_case(f"splitk{sk}-K288", 40, 72, 288, splitk=sk, bias=1) for sk in (1, 2, 4, 8)]
    c.append(gemm_case("splitk8-K64", 40, 72, 64, splitk=8, bias=1))
    return c


GEMM_EXACT = _exact_cases()
# the library's own split (ddimx_gemm_pick_splitk): the FFN GEMMs of a batch of two clips of S tokens
GEMM_PICK = [(s, n, k) for s in (1, 4, 32, 96) for n, k in ((2048, 512), (512, 2048))]


def gemm_pick_case(s, n, k):
    return gemm_case(f"pick-S{s}-N{n}-K{k}", 2 * s, n, k, bias=1)


def gemm_budget_bits(case):
    """exact_util.budget_bits of an exact case: K products of two operands plus the bias, resid and initial-C terms, on the
    integer grid."""
    extra = OPERAND_MAX * (case["bias"] + case["resid"] + case["accumulate"])
    return X.budget_bits(case["K"], OPERAND_MAX, 0, OPERAND_MAX, 0, extra=extra)


def gemm_operands(case, kind="exact"):
    """fp64 (A [1 or batch][M][K], B [batch][N][K], C0, bias, resid); the absent ones None.  kind 'exact': integers; 'gauss': N(0, 1)
    operands with B scaled to keep the products of order one."""
    t = case["name"] + "." + kind
    M, N, K, z = case["M"], case["N"], case["K"], case["batch"]
    if kind == "exact":
        mk = lambda tag, shape: ints(t + tag, shape)  # noqa: E731
        A, B = mk("A", (1 if case["shared_a"] else z, M, K)), mk("B", (z, N, K))
    else:
        mk = lambda tag, shape: gaussian(t + tag, shape)  # noqa: E731
        A, B = mk("A", (1 if case["shared_a"] else z, M, K)), mk("B", (z, N, K)) / math.sqrt(K)
    C0 = mk("C", (z, M, N)) if case["accumulate"] else None
    bias = mk("bias", (N,)) if case["bias"] else None
    resid = mk("resid", (z, M, N)) if case["resid"] else None
    return A, B, C0, bias, resid


GEMM_ROUNDED = gemm_case("gauss", 70, 50, 200)
GEMM_ACT = [gemm_case(f"gauss-gelu-sk{sk}", 70, 50, 200, splitk=sk, bias=1) for sk in (1, 2)]
# GEMM + LayerNorm: M = 5, K = 128; N = 512 two elements per thread, 100 the clamped-index path, 640 the general loop, 2048 the most
GEMM_LN_N, GEMM_LN_M, GEMM_LN_K = (512, 100, 640, 2048), 5, 128
GEMM_LN_SPLITK = (1, 4)
GEMM_LN_OPTS = ((0, 0), (1, 1), (1, 0), (0, 1))  # (bias, resid)


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------
def layernorm(x, add, gamma, beta, eps=LN_EPS):
    """(y, pre-norm rows, mean, rstd) of LN(x + add[m % add_rows]) * gamma + beta in fp64; add nullable [add_rows][N]."""
    v = x.double()
    if add is not None:
        v = v + add.double()[torch.arange(v.shape[0]) % add.shape[0]]
    mean = v.mean(1, keepdim=True)
    var = (v - mean).square().mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (v - mean) * rstd * gamma.double() + beta.double(), v, mean[:, 0], rstd[:, 0]


def layernorm_f32(x, add, gamma, beta, eps=LN_EPS):
    """The same two-pass arithmetic in fp32 on the CPU (what a sound fp32 kernel computes, up to summation order)."""
    v = x.float()
    if add is not None:
        v = v + add.float()[torch.arange(v.shape[0]) % add.shape[0]]
    mean = v.mean(1, keepdim=True)
    var = (v - mean).square().mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    return (v - mean) * rstd * gamma.float() + beta.float(), v, mean[:, 0], rstd[:, 0]


def ln_bwd(dy, v, mean, rstd, gamma):
    """(dx, dgamma, dbeta) of y = (v - mean) rstd gamma + beta given dy, all fp64; (mean, rstd) as handed to the kernel."""
    dy, v, g = dy.double(), v.double(), gamma.double()
    xh = (v - mean.double()[:, None]) * rstd.double()[:, None]
    gd = dy * g
    m1, m2 = gd.mean(1, keepdim=True), (gd * xh).mean(1, keepdim=True)
    return rstd.double()[:, None] * (gd - m1 - xh * m2), (dy * xh).sum(0), dy.sum(0)


def chunk_index(M, N, chunk_rows):
    """Flat position of y[m][n] in the chunk-major layout [m / chunk_rows][n / 4][32][4] (32 * N floats per sample)."""
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    return (m // chunk_rows) * 32 * N + ((n // 4) * 32 + m % chunk_rows) * 4 + n % 4


LN_N = (100, 256, 512, 1000, 2048)
LN_M = (1, 7, 33)
LN_ADD = dict(M=12, add_rows=4)
LN_CHUNK_ROWS = (8, 32)
LN_CHUNK_N = (100, 512)
LN_OFFSET = dict(M=7, N=512, mean=32.0)
LN_BWD_M = (1, 8, 9, 23)   # one short block; one full block; a full block and one row; three blocks, the last one short
LN_BWD_N = (100, 512, 2048)
LN_BWD_ADD_ROWS = 4


def ln_inputs(tag, M, N, bf16=False, add_rows=0, offset=0.0):
    """(x, add or None, gamma, beta): x fp32 or bf16 values (fp64 tensors holding them exactly are obtained with .double())."""
    x = (gaussian(tag + ".x", (M, N)) + offset).float()
    if bf16:
        x = x.bfloat16()
    add = gaussian(tag + ".add", (add_rows, N)).float() if add_rows else None
    gamma = (1.0 + 0.3 * gaussian(tag + ".g", (N,))).float()
    beta = (0.2 * gaussian(tag + ".b", (N,))).float()
    return x, add, gamma, beta


def offset_gate(x, gamma, beta, eps=LN_EPS):
    """The gate of the offset-rows case and the two numbers it is made of: the larger of the project's fp32 gate and 8 x the error
    of CPU fp32 F.layer_norm against fp64 on the same rows (8: a different but sound summation order).  Returns
    ((max, rms) gate, (max, rms) of F.layer_norm), in units of the std of the expected output."""
    want = layernorm(x, None, gamma, beta, eps)[0].reshape(-1)
    cpu = F.layer_norm(x.float(), (x.shape[1],), gamma.float(), beta.float(), eps).double().reshape(-1)
    s = float(want.std())
    d = cpu - want
    mx, rms = float(d.abs().max()) / s, float(d.square().mean().sqrt()) / s
    return (max(G.TOL[G.F32]["mx"], 8 * mx), max(G.TOL[G.F32]["rms"], 8 * rms)), (mx, rms)


def stat_errors(stat, mean, rstd):
    """Errors of a kernel's (mean, rstd) rows against fp64 in units of the row's std (= 1 / rstd): (mean - mean64) * rstd64 and
    rstd / rstd64 - 1.  (A row count of one has no std over rows; these units do not depend on it.)"""
    stat = stat.double()
    return torch.cat([(stat[:, 0] - mean) * rstd, stat[:, 1] / rstd - 1.0])


# ---- plain kernels -------------------------------------------------------------------------------------------------------------------
TRANSPOSE_SHAPES = ((1, 1), (31, 33), (32, 32), (65, 7), (6, 2048))
GELU_N = (1, 257, 4096 * 256 + 5)       # the last one is past the grid of 4096 blocks: the grid-stride loop wraps
COLSUM_B = (1, 15, 16, 17, 129, 300)
COLSUM_C = (1, 16, 17, 100)
DROPOUT_N = (1, 255, 257, 2048 * 256 + 3)  # the last one is past the grid of 2048 blocks
DROPOUT_P = (0.0, 0.1, 0.5)
DROPOUT_STREAMS = (0, 3)
DROPOUT_SEED = 0x1234_5678_9ABC_DEF1
DROPOUT_PN = [(p, n) for p in DROPOUT_P for n in DROPOUT_N]


def gelu_inputs():
    """(src, aux) of the largest gelu case; the smaller cases take the leading elements.  aux / mode-0 src cover [-8, 8] evenly in
    a fixed shuffled order."""
    n = max(GELU_N)
    g = torch.Generator().manual_seed(7)
    grid = torch.linspace(-8.0, 8.0, n, dtype=torch.float64)[torch.randperm(n, generator=g)].float()
    return grid, gaussian("gelu.src", (n,)).float()


_M64 = (1 << 64) - 1


def dropout_thresh(p):
    """fnet_pointwise.hip: drop_thresh -- (unsigned)((double)p * 2^32) of the fp32 p."""
    p = float(np.float32(p))
    return 0 if p <= 0.0 else int(p * 4294967296.0)


def dropout_scale(p, seed, stream, n, first=0):
    """The factor dropout_keep gives elements first .. first + n - 1, as float32: 1 / (1 - p) (fp32 arithmetic) where the top 32
    bits of the mixed 64-bit word reach the threshold, else 0.  Written from the documented mixing function (fnet_pointwise.hip:
    dropout_keep, a splitmix64 finaliser over seed + golden * (stream + 1) + e * odd constant) in numpy uint64, which wraps."""
    e = np.arange(first, first + n, dtype=np.uint64)
    base = np.full(1, (seed + 0x9E3779B97F4A7C15 * (stream + 1)) & _M64, dtype=np.uint64)
    z = base + e * np.uint64(0xD1342543DE82EF95)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    keep = (z >> np.uint64(32)) >= np.uint64(dropout_thresh(p))
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(keep, inv, np.float32(0.0)).astype(np.float32)


def dropout_apply(src, p, seed, stream, first=0):
    """src (float32 numpy, flat) * dropout_scale: one fp32 multiplication per element, as the kernel does."""
    return (src.astype(np.float32) * dropout_scale(p, seed, stream, src.size, first)).astype(np.float32)


def dropout_hook(p, seed, b, s, hid):
    """The ``drop(site, h)`` callable of ``oracle.ref_cpu.transformer_module`` / ``model_forward`` that drops what the library drops:
    site k multiplies h [b, s, hid] by ``dropout_scale(p, seed, k, b * s * hid)`` read as [b, s, hid] -- mask stream k (0: the
    embedding projection, i + 1: layer i's FFN output), element (b_ * s + s_) * hid + n.  Nothing is permuted: hid is not part of the
    library's token-order permutation and rows are b_ * S + s_ in both worlds.  ``drop.sites`` lists the sites it was called with,
    in call order.  The factor enters as a constant of h's dtype, so autograd through ``drop`` masks the gradient alike."""
    def drop(site, h):
        assert tuple(h.shape) == (b, s, hid), (site, tuple(h.shape), (b, s, hid))
        drop.sites.append(site)
        return h * torch.from_numpy(dropout_scale(p, seed, site, b * s * hid)).reshape(b, s, hid).to(h.dtype)

    drop.sites = []
    return drop


def keep_bound(p, n):
    """Five standard deviations of the kept fraction of n Bernoulli(1 - p) draws."""
    return 5.0 * math.sqrt(p * (1.0 - p) / n)


def colsum(src):
    """float32(fp64 column sums) of src [B][C]: the kernel adds in fp64 and rounds once."""
    return src.double().sum(0).float()
