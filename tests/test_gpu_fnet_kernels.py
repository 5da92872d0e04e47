"""The FNet bottleneck's kernels one by one (gemm.hip, layernorm_kernel, and the LayerNorm / gelu / transpose / colsum / dropout
kernels of fnet_pointwise.hip) through their own C-ABI entry points, against the fp64 references of tests/fnet_kernel_ref.py.

Every output lives inside a larger sentinel-filled allocation (``Out`` of tests/kernel_harness.py, in its `idx` form: every byte
0xFF, a NaN in fp32, compared byte by byte afterwards): the kernel must write every logical element and nothing else
-- not the guard band on either side, not the padding columns of ldc > N, not the unused rows of the chunk-major layout.  The
split-K and LayerNorm-backward workspaces are NaN before each call, so a slice that is read without having been written shows.
Where the arithmetic allows it the comparison is bit for bit; the fp32 gate of tests/gpu_util.py is used only where a
transcendental or an inexact fp32 sum enters, and those tests print the measured worst errors."""
import pytest
import torch

from ddim_audio_amd import _lib
import fnet_kernel_ref as R
import gpu_util as G
from kernel_harness import NAN, Out, dev, dev32, lib as load_lib, placed, refused, report_std as report, same

pytestmark = pytest.mark.gpu

def strided_index(batch, rows, cols, sb, ld):
    z, m, n = torch.arange(batch)[:, None, None], torch.arange(rows)[None, :, None], torch.arange(cols)[None, None, :]
    return z * sb + m * ld + n


# ---- GEMM ------------------------------------------------------------------------------------------------------------------------------
def run_gemm(case, ops, bf16, act=0, ln=None):
    """ddimx_gemm_nt (or, with ln = (gamma, beta), ddimx_gemm_ln) on a case of fnet_kernel_ref with the operands `ops` (fp64, rounded
    to fp32 here).  Returns the output [batch][M][N] on the CPU."""
    lib = load_lib()
    A, B, C0, bias, resid = ops
    M, N, K, z = case["M"], case["N"], case["K"], case["batch"]
    lda, ldb, ldc = case["lda"], case["ldb"], case["ldc"]
    sA = 0 if case["shared_a"] or z == 1 else M * lda
    sB = N * ldb
    sC = M * ldc + case["pad_c"]
    Ad = placed(A, strided_index(A.shape[0], M, K, M * lda, lda), case["a_off"])
    Bd = placed(B, strided_index(z, N, K, sB, ldb))
    cidx = strided_index(z, M, N, sC, ldc)
    Rd = placed(resid, cidx) if resid is not None else None
    pA, pB, pR = _lib.ptr(Ad), _lib.ptr(Bd), _lib.ptr(Rd)
    bias_d = dev32(bias) if bias is not None else None
    sk = case["splitk"]
    part = torch.full((max(sk, 1) * z * M * N,), NAN, device=G.dev())
    if ln is None:
        out = Out(idx=cidx, init=C0)
        rc = lib.ddimx_gemm_nt(pA, pB, out.ptr, _lib.ptr(bias_d), pR, _lib.ptr(part) if sk > 1 else None, M, N, K, lda, ldb, ldc, sA, sB,
                               sC, z, sk, case["accumulate"], act, bf16, _lib.stream())
    else:
        gamma, beta = dev32(ln[0]), dev32(ln[1])
        out = Out(idx=strided_index(1, M, N, 0, N))
        rc = lib.ddimx_gemm_ln(pA, pB, None, _lib.ptr(bias_d), pR, _lib.ptr(part), M, N, K, lda, ldb, ldc, sA, sB, sC, z, sk, 0, 0, bf16,
                               _lib.ptr(gamma), _lib.ptr(beta), R.LN_EPS, out.ptr, _lib.stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    return out.read(case["name"])


def _check_exact(case):
    ops = R.gemm_operands(case)
    want = R.gemm(*ops)
    got = {bf: run_gemm(case, ops, bf) for bf in (0, 1)}
    for bf, g in got.items():
        bad = (g.double() != want) | ~torch.isfinite(g.double())
        if bad.any():
            z, m, n = (int(v[0]) for v in bad.nonzero(as_tuple=True))
            raise AssertionError(f"{case['name']} bf16={bf}: {int(bad.sum())} of {bad.numel()} elements differ; first at batch {z} row {m} "
                                 f"col {n}: got {float(g[z, m, n])!r}, exact {float(want[z, m, n])!r}")
        assert torch.equal(g.double(), want)
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize("case", R.GEMM_EXACT, ids=lambda c: c["name"])
def test_gemm_exact(case):
    """gemm_nt_kernel<fp32 | bf16> and gemm_splitk_reduce_kernel on integer operands (|v| <= 3, exact in bf16): both precisions equal
    the fp64 product bit for bit and each other -- full tiles under both K-loop schedules, ragged M / N, unaligned and padded leading
    dimensions, K tails down to K = 1, batches, every accumulate x bias x resid epilogue in either kernel, empty split-K slices."""
    _check_exact(case)


@pytest.mark.parametrize("s,n,k", R.GEMM_PICK)
def test_gemm_exact_at_the_librarys_own_split(s, n, k):
    """The FFN shapes of a batch of two clips of S tokens at the split ddimx_gemm_pick_splitk chooses (per precision), bit for bit."""
    lib = load_lib()
    case = R.gemm_pick_case(s, n, k)
    ops = R.gemm_operands(case)
    want = R.gemm(*ops)
    got = []
    for bf in (0, 1):
        sk = lib.ddimx_gemm_pick_splitk(s, n, k, bf)
        assert 1 <= sk <= 8, (s, n, k, bf, sk)
        got.append(run_gemm(dict(case, splitk=sk), ops, bf))
        assert torch.equal(got[-1].double(), want), (s, n, k, bf, sk)
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize("bf16", [0, 1], ids=["f32", "bf16"])
def test_gemm_rounded_operands(bf16):
    """Gaussian 70x50x200 operands.  fp32: against fp64 on the operands; bf16: against fp64 on A.bfloat16(), B.bfloat16() -- only
    the fp32 accumulation differs, so the fp32 gate applies and a truncating conversion would miss it (test_fnet_kernels_cpu.py).
    With act = 1 (gelu_new after the bias) at splitk 1 (epilogue in the GEMM kernel) and 2 (in the reduce kernel).
    Measured on MI355X, max / rms of std: fp32 plain 1.7e-6 / 2.6e-7, gelu 2.0e-6 / 2.3e-7; bf16 plain 5.6e-7 / 7.4e-8, gelu
    7.5e-7 / 8.8e-8."""
    for case, act in [(R.GEMM_ROUNDED, 0)] + [(c, 1) for c in R.GEMM_ACT]:
        ops = R.gemm_operands(case, "gauss")
        A, B = ops[0].float(), ops[1].float()
        ref = (A.bfloat16(), B.bfloat16()) if bf16 else (A, B)
        want = R.gemm(ref[0], ref[1], None, None if ops[3] is None else ops[3].float(), None, act)
        got = run_gemm(case, ops, bf16, act)
        report(f"gemm {case['name']} bf16={bf16}", *G.check_close(got, want, G.F32, case["name"]))


@pytest.mark.parametrize("bf16", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("splitk", R.GEMM_LN_SPLITK)
@pytest.mark.parametrize("N", R.GEMM_LN_N)
def test_gemm_ln(N, splitk, bf16):
    """ddimx_gemm_ln (gemm_nt_kernel into the workspace + gemm_reduce_ln_kernel) at M = 5, K = 128 against fp64, fp32 gate: two
    elements per thread (N = 512), clamped indices (100), the general loop (640, 2048); with and without bias and resid (resid rows
    N + 4 apart).  Measured worst case on MI355X: max 2.0e-6 rms 2.3e-7 of std (fp32), 9.7e-7 / 9.8e-8 (bf16)."""
    worst = (0.0, 0.0)
    for has_bias, has_resid in R.GEMM_LN_OPTS:
        case = R.gemm_case(f"ln-N{N}", R.GEMM_LN_M, N, R.GEMM_LN_K, ldc=N + 4 if has_resid else N, splitk=splitk, bias=has_bias,
                           resid=has_resid)
        ops = R.gemm_operands(case, "gauss")
        _, _, gamma, beta = R.ln_inputs(case["name"], 1, N)
        A, B = ops[0].float(), ops[1].float()
        ref = (A.bfloat16(), B.bfloat16()) if bf16 else (A, B)
        f32 = lambda t: None if t is None else t.float()  # noqa: E731
        want = R.layernorm(R.gemm(ref[0], ref[1], None, f32(ops[3]), f32(ops[4]))[0], None, gamma, beta)[0]
        got = run_gemm(case, ops, bf16, ln=(gamma, beta))[0]
        e = G.check_close(got, want, G.F32, f"{case['name']} splitk={splitk} bias={has_bias} resid={has_resid}")
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    report(f"gemm_ln N={N} splitk={splitk} bf16={bf16}", *worst)


@pytest.mark.parametrize("why", ["N=2052", "batch=2", "null partial"])
def test_gemm_ln_rejects(why):
    """What gemm_ln_launch cannot do comes back as an error before any launch: the output stays NaN."""
    lib = load_lib()
    N = 2052 if why == "N=2052" else 512
    M, K = R.GEMM_LN_M, R.GEMM_LN_K
    a, b = torch.zeros(2 * M * K, device=G.dev()), torch.zeros(2 * N * K, device=G.dev())
    gamma, beta = torch.ones(N, device=G.dev()), torch.zeros(N, device=G.dev())
    part = torch.full((2 * M * N,), NAN, device=G.dev())
    out = Out(idx=strided_index(2, M, N, M * N, N))
    rc = lib.ddimx_gemm_ln(_lib.ptr(a), _lib.ptr(b), None, None, None, None if why == "null partial" else _lib.ptr(part), M, N, K, K, K, N,
                           M * K, N * K, M * N, 2 if why == "batch=2" else 1, 1, 0, 0, 0, _lib.ptr(gamma), _lib.ptr(beta), R.LN_EPS, out.ptr,
                           _lib.stream())
    refused(rc, out, who="gemm_ln_launch")
    assert bool(torch.isnan(part).all())


# ---- LayerNorm forward -----------------------------------------------------------------------------------------------------------------
def run_layernorm(x, add, gamma, beta, chunk_rows=0):
    lib = load_lib()
    M, N = x.shape
    xd, ad, gd, bd = dev(x, x.dtype), None if add is None else dev32(add), dev32(gamma), dev32(beta)
    idx = R.chunk_index(M, N, chunk_rows) if chunk_rows else strided_index(1, M, N, 0, N)[0]
    y = Out(idx=idx)
    _lib.check(lib.ddimx_layernorm(G.BF16 if x.dtype == torch.bfloat16 else G.F32, _lib.ptr(xd), _lib.ptr(ad), 0 if add is None else add.shape[0],
                                   _lib.ptr(gd), _lib.ptr(bd), R.LN_EPS, y.ptr, M, N, chunk_rows, _lib.stream()))
    torch.cuda.synchronize()
    return y.read("layernorm y")


def run_ln_train(x, add, gamma, beta, p=0.0, seed=0, mask_stream=0, want_sum=True):
    """(y, sum_out or None, stat) of ddimx_ln_train; x may already live on the device."""
    lib = load_lib()
    M, N = x.shape
    xd, ad, gd, bd = dev(x, x.dtype), None if add is None else dev32(add), dev32(gamma), dev32(beta)
    rows = strided_index(1, M, N, 0, N)[0]
    y, so, stat = Out(idx=rows), Out(idx=rows) if want_sum else None, Out(idx=strided_index(1, M, 2, 0, 2)[0])
    _lib.check(lib.ddimx_ln_train(G.BF16 if x.dtype == torch.bfloat16 else G.F32, _lib.ptr(xd), _lib.ptr(ad), 0 if add is None else add.shape[0],
                                  _lib.ptr(gd), _lib.ptr(bd), R.LN_EPS, y.ptr, so.ptr if so else None, stat.ptr, M, N, p, seed, mask_stream,
                                  None, _lib.stream()))
    torch.cuda.synchronize()
    return y.read("ln_train y"), so.read("ln_train sum_out") if so else None, stat.read("ln_train stat")


def _check_ln_forward(tag, x, add, gamma, beta, chunk_rows=0, tol=None):
    """Both forward kernels on one input; returns the worst (max, rms) over y (both kernels) and the statistics."""
    want, v, mean, rstd = R.layernorm(x, add, gamma, beta)
    y0 = run_layernorm(x, add, gamma, beta, chunk_rows)
    e = [R.gate(y0, want, f"{tag} layernorm", tol=tol)]
    if not chunk_rows:
        y1, so, stat = run_ln_train(x, add, gamma, beta)
        e.append(R.gate(y1, want, f"{tag} ln_train", tol=tol))
        same(so, v.float(), f"{tag}: sum_out is one fp32 add and must be exact")
        e.append(R.gate(R.stat_errors(stat, mean, rstd), torch.zeros(2 * x.shape[0]), f"{tag} stat", std=1.0))
        y2, so2, stat2 = run_ln_train(x, add, gamma, beta, want_sum=False)
        assert so2 is None
        same(y2, y1, f"{tag}: a null sum_out must not change y")
        same(stat2, stat, f"{tag}: a null sum_out must not change stat")
    return max(v[0] for v in e), max(v[1] for v in e)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("M", R.LN_M)
@pytest.mark.parametrize("N", R.LN_N)
def test_layernorm_forward(N, M, bf16):
    """layernorm_kernel and ln_train_kernel (p = 0) on fp32 and bf16 rows of N = 100 .. 2048 (one to eight elements per thread, ragged)
    against fp64: y at the fp32 gate; ln_train's sum_out bit for bit; its (mean, rstd) at the fp32 gate in units of the row's std.
    Measured worst case on MI355X: max 7.6e-7 rms 7.0e-8 of std."""
    x, add, gamma, beta = R.ln_inputs(f"ln{M}.{N}.{int(bf16)}", M, N, bf16)
    report(f"layernorm M={M} N={N} bf16={bf16}", *_check_ln_forward(f"M={M} N={N}", x, add, gamma, beta))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_layernorm_forward_add_rows_wrap(bf16):
    """`add` has 4 rows, x has 12: row m takes add[m % 4] (the positional table of a batch of three clips).  Measured on MI355X:
    max 7.4e-7 rms 6.3e-8 of std."""
    a = R.LN_ADD
    x, add, gamma, beta = R.ln_inputs(f"ln.add.{int(bf16)}", a["M"], 512, bf16, add_rows=a["add_rows"])
    report(f"layernorm add rows bf16={bf16}", *_check_ln_forward("add rows", x, add, gamma, beta))


@pytest.mark.parametrize("N", R.LN_CHUNK_N)
@pytest.mark.parametrize("chunk_rows", R.LN_CHUNK_ROWS)
def test_layernorm_forward_chunk_major(chunk_rows, N):
    """chunk_rows > 0: y goes to [m / chunk_rows][n / 4][32][4], 32 * N floats per sample; with 8 rows per sample the other 24 row
    slots stay NaN.  Measured on MI355X: max 9.3e-7 rms 6.6e-8 of std."""
    M = 3 * chunk_rows
    x, _, gamma, beta = R.ln_inputs(f"ln.chunk{chunk_rows}.{N}", M, N, bf16=True)
    add = R.gaussian(f"ln.chunk{chunk_rows}.{N}.add", (chunk_rows, N)).float()
    report(f"layernorm chunk_rows={chunk_rows} N={N}", *_check_ln_forward("chunk-major", x, add, gamma, beta, chunk_rows))


def test_layernorm_forward_offset_rows():
    """Rows of mean 32 and std 1: a one-pass variance E[x^2] - mean^2 loses them in fp32, the kernels' two-pass form does not.
    Gate: the larger of the fp32 gate and 8 x the error of CPU fp32 F.layer_norm against fp64 on the same rows.
    CPU F.layer_norm: max 3.4e-6 rms 1.0e-6 of std (so the fp32 gate, 1e-4 / 2e-5, is the larger); measured on MI355X: max 5.8e-6 rms 1.6e-6."""
    o = R.LN_OFFSET
    x, _, gamma, beta = R.ln_inputs("ln.offset", o["M"], o["N"], offset=o["mean"])
    tol, cpu = R.offset_gate(x, gamma, beta)
    report("layernorm offset rows, CPU F.layer_norm", *cpu)
    print(f"[layernorm offset rows] gate max {tol[0]:.2e} rms {tol[1]:.2e}")
    report("layernorm offset rows", *_check_ln_forward("offset rows", x, None, gamma, beta, tol=tol))


# ---- LayerNorm backward ----------------------------------------------------------------------------------------------------------------
def run_ln_bwd(dy, x, add, stat, gamma, with_params=True):
    lib = load_lib()
    M, N = dy.shape
    dyd, xd, ad, sd, gd = dev32(dy), dev(x, x.dtype), None if add is None else dev32(add), dev32(stat), dev32(gamma)
    dx = Out(idx=strided_index(1, M, N, 0, N)[0])
    dg, db = Out(N), Out(N)
    nf = int(lib.ddimx_ln_bwd_partial_floats(M, N))
    assert nf == -(-M // R.LN_ROWS) * 2 * N
    part = Out(nf)
    _lib.check(lib.ddimx_ln_bwd(G.BF16 if x.dtype == torch.bfloat16 else G.F32, _lib.ptr(dyd), _lib.ptr(xd), _lib.ptr(ad),
                                0 if add is None else add.shape[0], _lib.ptr(sd), _lib.ptr(gd), dx.ptr, part.ptr, dg.ptr if with_params else None,
                                db.ptr if with_params else None, M, N, _lib.stream()))
    torch.cuda.synchronize()
    part.read("ln_bwd partial")
    if not with_params:
        assert dg.untouched() and db.untouched()
        return dx.read("ln_bwd dx"), None, None
    return dx.read("ln_bwd dx"), dg.read("ln_bwd dgamma"), db.read("ln_bwd dbeta")


@pytest.mark.parametrize("emb", [False, True], ids=["f32", "bf16+add"])
@pytest.mark.parametrize("N", R.LN_BWD_N)
@pytest.mark.parametrize("M", R.LN_BWD_M)
def test_layernorm_backward(M, N, emb):
    """ln_bwd_kernel + the two colsum launches against the fp64 formula (itself equal to autograd of F.layer_norm,
    test_fnet_kernels_cpu.py), statistics computed in fp64 and rounded to fp32 so that the forward kernel is not involved: dx,
    dgamma, dbeta at the fp32 gate for M = 1, 8, 9, 23 rows (blocks of 8) -- fp32 rows, and bf16 rows plus 4 wrapping `add` rows
    as the embedding norm has them.  The data-only form (null dgamma / dbeta) must give the same dx bit for bit.
    Measured worst case on MI355X: max 8.4e-7 rms 9.1e-8 of std."""
    x, add, gamma, beta = R.ln_inputs(f"lnb{M}.{N}.{int(emb)}", M, N, bf16=emb, add_rows=R.LN_BWD_ADD_ROWS if emb else 0)
    dy = R.gaussian(f"lnb{M}.{N}.dy", (M, N)).float()
    _, v, mean, rstd = R.layernorm(x, add, gamma, beta)
    stat = torch.stack([mean, rstd], 1).float()
    want = R.ln_bwd(dy, v, stat[:, 0], stat[:, 1], gamma)
    dx, dg, db = run_ln_bwd(dy, x, add, stat, gamma)
    # (one row: dx has a std over its N elements; dgamma / dbeta over N as well)
    e = [G.check_close(g, w, G.F32, f"{what} M={M} N={N}") for g, w, what in ((dx, want[0], "dx"), (dg, want[1], "dgamma"), (db, want[2], "dbeta"))]
    report(f"ln_bwd M={M} N={N} emb={emb}", max(v[0] for v in e), max(v[1] for v in e))
    dx2, _, _ = run_ln_bwd(dy, x, add, stat, gamma, with_params=False)
    same(dx2, dx)


# ---- transpose, gelu, colsum -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,c", R.TRANSPOSE_SHAPES)
def test_transpose(r, c):
    """transpose_kernel: bit-exact; with act_gelu against fp64 gelu_new at the fp32 gate (in units of the std of gelu_new over the
    input distribution, which a 1x1 matrix does not have by itself).  Measured worst case on MI355X: max 3.2e-7 rms 4.3e-8."""
    lib = load_lib()
    x = (2.0 * R.gaussian(f"tr{r}.{c}", (r, c))).float()
    xd = dev32(x)
    unit = R.gelu_new(2.0 * R.gaussian("tr.unit", (4096,))).std()
    for act in (0, 1):
        out = Out(idx=strided_index(1, c, r, 0, r)[0])
        _lib.check(lib.ddimx_transpose(_lib.ptr(xd), out.ptr, r, c, act, _lib.stream()))
        torch.cuda.synchronize()
        got = out.read(f"transpose {r}x{c}")
        if act:
            report(f"transpose+gelu {r}x{c}", *R.gate(got, R.gelu_new(x.double()).T, f"transpose+gelu {r}x{c}", std=unit))
        else:
            same(got, x.T.contiguous())


_GELU = {}


def _gelu_ref():
    if not _GELU:
        aux, src = R.gelu_inputs()
        _GELU.update(aux=aux, src=src, w0=R.gelu_new(aux.double()), w1=src.double() * R.dgelu_new(aux.double()), auxd=dev32(aux), srcd=dev32(src))
    return _GELU


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", R.GELU_N)
def test_gelu(n, mode):
    """gelu_kernel, mode 0 (gelu_new) and 1 (src * gelu_new'(aux)) with the argument over [-8, 8], against fp64 at the fp32 gate (in
    units of the std of the whole reference, of which the short cases are the leading elements); n = 4096 * 256 + 5 wraps the
    grid-stride loop.  Measured worst case on MI355X: mode 0 max 1.7e-7 rms 2.5e-8, mode 1 max 2.8e-6 rms 1.7e-7."""
    lib = load_lib()
    g = _gelu_ref()
    out = Out(n)
    if mode == 0:
        _lib.check(lib.ddimx_gelu(_lib.ptr(g["auxd"]), None, out.ptr, n, 0, _lib.stream()))
    else:
        _lib.check(lib.ddimx_gelu(_lib.ptr(g["srcd"]), _lib.ptr(g["auxd"]), out.ptr, n, 1, _lib.stream()))
    torch.cuda.synchronize()
    want = g["w1" if mode else "w0"]
    report(f"gelu mode={mode} n={n}", *R.gate(out.read(f"gelu n={n}"), want[:n], f"gelu mode={mode} n={n}", std=want.std()))


@pytest.mark.parametrize("C", R.COLSUM_C)
@pytest.mark.parametrize("B", R.COLSUM_B)
def test_colsum(B, C):
    """colsum_kernel (16 row slices per column, unrolled by 8: B = 129 and 300 enter the unrolled loop): integer-grid inputs bit for
    bit, Gaussian inputs equal to float32(fp64 sum); stride = C and 2 C, the skipped columns holding NaN."""
    import exact_util as X
    lib = load_lib()
    for kind, src in (("dyadic", X.dyadic(f"cs{B}.{C}", (B, C), 64, 3).float()), ("gauss", R.gaussian(f"cs{B}.{C}", (B, C)).float())):
        want = R.colsum(src)
        if kind == "dyadic":
            assert torch.equal(want.double(), src.double().sum(0))
        for stride in (C, 2 * C):
            sd = placed(src[None], strided_index(1, B, C, 0, stride))
            out = Out(C)
            _lib.check(lib.ddimx_colsum(_lib.ptr(sd), B, stride, C, out.ptr, _lib.stream()))
            torch.cuda.synchronize()
            same(out.read(f"colsum {B}x{C}"), want, (kind, B, C, stride))


# ---- dropout ---------------------------------------------------------------------------------------------------------------------------
_DROP = {}


def _drop_src():
    if not _DROP:
        src = R.gaussian("drop.src", (max(R.DROPOUT_N),)).float()
        _DROP.update(src=src, np=src.numpy(), d=dev32(src))
    return _DROP


@pytest.mark.parametrize("mask_stream", R.DROPOUT_STREAMS)
@pytest.mark.parametrize("p,n", R.DROPOUT_PN)
def test_dropout_apply(p, n, mask_stream):
    """dropout_apply_kernel against the numpy uint64 restatement of dropout_keep, bit for bit: out of place, in place (as
    fnet_bwd_part calls it), and with the seed split into a by-value part and a device counter.  The kept fraction lies within five
    binomial standard deviations of 1 - p."""
    lib = load_lib()
    s = _drop_src()
    seed = R.DROPOUT_SEED
    want = torch.from_numpy(R.dropout_apply(s["np"][:n], p, seed, mask_stream))

    def call(dst, src_ptr, sd, ctr):
        _lib.check(lib.ddimx_dropout_apply(src_ptr, dst.ptr, n, p, sd, mask_stream, _lib.ptr(ctr), _lib.stream()))
        torch.cuda.synchronize()
        return dst.read(f"dropout n={n} p={p}")

    got = call(Out(n), _lib.ptr(s["d"]), seed, None)
    same(got, want)
    inplace = Out(n, init=s["src"][:n])
    same(call(inplace, inplace.ptr, seed, None), want)
    c = 0x0123_4567_89AB
    ctr = torch.tensor([c], dtype=torch.int64, device=G.dev())
    same(call(Out(n), _lib.ptr(s["d"]), seed - c, ctr), want)
    if p > 0:
        kept = float((got != 0).double().mean())
        assert abs(kept - (1.0 - p)) <= R.keep_bound(p, n), (p, n, kept)
    else:
        same(got, s["src"][:n])


@pytest.mark.parametrize("mask_stream", [0, 2])
def test_forward_and_backward_agree_on_the_dropout_mask(mask_stream):
    """The forward drops inside ln_train_kernel, the backward regenerates the mask with dropout_apply_kernel: ln_train(x, p) and
    ln_train(dropout_apply(x, p), 0) must give the same sum_out and y bit for bit (same seed and mask stream; M = 5, N = 512)."""
    lib = load_lib()
    M, N, p, seed = 5, 512, 0.1, R.DROPOUT_SEED
    x, _, gamma, beta = R.ln_inputs("ln.mask", M, N)
    add = R.gaussian("ln.mask.add", (M, N)).float()
    y1, so1, st1 = run_ln_train(x, add, gamma, beta, p, seed, mask_stream)
    xd = dev32(x)
    dropped = torch.full_like(xd, NAN)
    _lib.check(lib.ddimx_dropout_apply(_lib.ptr(xd), _lib.ptr(dropped), M * N, p, seed, mask_stream, None, _lib.stream()))
    y2, so2, st2 = run_ln_train(dropped, add, gamma, beta)
    same(so1, so2)
    same(y1, y2)
    same(st1, st2)
    ref = torch.from_numpy(R.dropout_apply(x.numpy().reshape(-1), p, seed, mask_stream)).view(M, N) + add
    same(so1, ref, "the mask is the reference's, over element index m * N + n")
    assert 0 < int((dropped == 0).sum()) < M * N
