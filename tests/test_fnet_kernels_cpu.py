"""The references and case tables of tests/fnet_kernel_ref.py, checked without a GPU: the exactness budget of every exact-operand
GEMM case, the LayerNorm backward against autograd, the dropout reference's statistics, and that every gate the GPU tests apply
is one the reference itself meets when it is evaluated in fp32 (a gate the reference cannot meet is a wrong gate)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_util as X
import fnet_kernel_ref as R
import gpu_util as G


# ---- 1. exact GEMM cases ---------------------------------------------------------------------------------------------------------------
ALL_EXACT = R.GEMM_EXACT + [R.gemm_pick_case(*c) for c in R.GEMM_PICK]


def test_exact_case_names_are_unique_and_cover_the_paths():
    names = [c["name"] for c in ALL_EXACT]
    assert len(set(names)) == len(names)
    by = {c["name"]: c for c in ALL_EXACT}
    for prec, bk in R.BK.items():
        full = lambda c: c["M"] % R.TILE_M == 0 and c["N"] % R.TILE_N == 0 and c["K"] % bk == 0 and c["lda"] % 4 == 0 and c["ldb"] % 4 == 0  # noqa: E731
        chunks = lambda c: -(-c["K"] // bk)  # noqa: E731
        assert full(by["full-prefetch"]) and chunks(by["full-prefetch"]) <= 4, "request-all-chunks schedule"
        assert full(by["full-pipelined"]) and chunks(by["full-pipelined"]) > 4, "pipelined schedule on a full tile"
    assert by["bf16-ktail"]["K"] % R.BK[1] == R.BK[1] // 2
    assert any(c["lda"] % 4 for c in ALL_EXACT) and any(c["lda"] > c["K"] and c["lda"] % 4 == 0 for c in ALL_EXACT)
    assert {c["K"] for c in ALL_EXACT if c["name"].startswith("wgrad")} == {1, 3, 6, 15}
    k288 = by["splitk4-K288"]
    per = -(-(-(-k288["K"] // R.BK[0])) // 4)
    assert 3 * per >= -(-k288["K"] // R.BK[0]), "the fourth fp32 slice of K = 288 is empty"
    epi = [c for c in ALL_EXACT if c["name"].startswith("epi-")]
    assert len({(c["splitk"], c["accumulate"], c["bias"], c["resid"]) for c in epi}) == 16


@pytest.mark.parametrize("case", ALL_EXACT, ids=lambda c: c["name"])
def test_exact_gemm_budget_and_operands(case):
    assert R.gemm_budget_bits(case) < 24
    if case["M"] * case["N"] * case["K"] > 1 << 22:
        return  # (the budget is what matters; the large products are formed once, on the GPU run)
    A, B, C0, bias, resid = R.gemm_operands(case)
    for t in (A, B, C0, bias, resid):
        if t is not None:
            assert float(t.abs().max()) <= R.OPERAND_MAX and torch.equal(t, t.round())
            assert torch.equal(t.bfloat16().double(), t), "operands must be exact in bf16"
    want = R.gemm(A, B, C0, bias, resid)
    assert torch.equal(want.float().double(), want), "the exact result must be an fp32 number"
    # any fp32 summation order gives it: one order, the torch fp32 matmul, must
    got = torch.einsum("zmk,znk->zmn", A.float().expand(B.shape[0], -1, -1), B.float())
    for t in (C0, bias, resid):
        if t is not None:
            got = got + t.float()
    assert torch.equal(got.double(), want)


def test_gemm_reference_against_torch_linear():
    c = R.GEMM_ACT[0]
    A, B, C0, bias, resid = R.gemm_operands(dict(c, resid=1, accumulate=1), "gauss")
    want = C0 + F.linear(A[0], B[0], bias)
    assert torch.allclose(R.gemm(A, B, C0, bias, None)[0], want[0], rtol=0, atol=1e-12)
    hf = F.gelu(want, approximate="tanh") + resid
    assert torch.allclose(R.gemm(A, B, C0, bias, resid, act=1), hf, rtol=0, atol=1e-12)


# ---- 2. LayerNorm ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,add_rows", [(5, 100, 0), (9, 512, 0), (12, 256, 4)])
def test_layernorm_reference_against_torch(M, N, add_rows):
    x, add, gamma, beta = R.ln_inputs(f"cpu.ln{M}.{N}", M, N, add_rows=add_rows)
    y, v, mean, rstd = R.layernorm(x, add, gamma, beta)
    vin = x.double() if add is None else x.double() + add.double().repeat(M // add_rows, 1)
    assert torch.equal(v, vin)
    assert torch.allclose(y, F.layer_norm(vin, (N,), gamma.double(), beta.double(), R.LN_EPS), rtol=0, atol=1e-12)
    assert torch.allclose(mean, vin.mean(1)) and torch.allclose(rstd, 1.0 / vin.var(1, unbiased=False).sqrt())


@pytest.mark.parametrize("M,N", [(1, 100), (9, 512), (23, 2048)])
def test_ln_backward_reference_equals_autograd(M, N):
    x, _, gamma, beta = R.ln_inputs(f"cpu.lnb{M}.{N}", M, N)
    dy = R.gaussian(f"cpu.lnb{M}.{N}.dy", (M, N))
    v = x.double().requires_grad_(True)
    g, b = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.layer_norm(v, (N,), g, b, R.LN_EPS).backward(dy)
    _, _, mean, rstd = R.layernorm(x, None, gamma, beta)
    dx, dg, db = R.ln_bwd(dy, x.double(), mean, rstd, gamma)
    for got, want in ((dx, v.grad), (dg, g.grad), (db, b.grad)):
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-11)


def test_chunk_index_is_the_documented_layout():
    for cr in R.LN_CHUNK_ROWS:
        M, N = 3 * cr, 100
        idx = R.chunk_index(M, N, cr)
        assert idx.unique().numel() == M * N and int(idx.max()) < 3 * 32 * N
        buf = torch.full((3, N // 4, 32, 4), -1, dtype=torch.long)
        buf.view(-1)[idx.reshape(-1)] = torch.arange(M * N)
        for m, n in ((0, 0), (cr - 1, 99), (cr, 4), (M - 1, 50)):
            assert int(buf[m // cr, n // 4, m % cr, n % 4]) == m * N + n
        assert (buf[:, :, cr:, :] == -1).all(), "rows past chunk_rows of a sample are unused"


# ---- 3. dropout -----------------------------------------------------------------------------------------------------------------------
def test_dropout_reference_mixing_function():
    """The mixer is splitmix64's finaliser; spot values computed by hand with Python integers (which do not wrap by themselves)."""
    def keep_word(seed, stream, e):
        m = (1 << 64) - 1
        z = (seed + 0x9E3779B97F4A7C15 * (stream + 1) + e * 0xD1342543DE82EF95) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return (z ^ (z >> 31)) >> 32
    for seed, stream in ((0, 0), (R.DROPOUT_SEED, 3), ((1 << 64) - 5, 7)):
        for p in (0.1, 0.5):
            got = R.dropout_scale(p, seed, stream, 64, first=1000)
            want = [keep_word(seed, stream, 1000 + i) >= R.dropout_thresh(p) for i in range(64)]
            assert (got != 0).tolist() == want
            assert set(np.unique(got).tolist()) <= {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    assert R.dropout_thresh(0.0) == 0 and (R.dropout_scale(0.0, 5, 1, 1000) == 1.0).all()
    assert R.dropout_thresh(0.5) == 1 << 31


@pytest.mark.parametrize("p,n", [pn for pn in R.DROPOUT_PN if pn[0] > 0])
def test_dropout_reference_keep_fraction(p, n):
    for stream in R.DROPOUT_STREAMS:
        kept = float((R.dropout_scale(p, R.DROPOUT_SEED, stream, n) != 0).mean())
        assert abs(kept - (1.0 - p)) <= R.keep_bound(p, n), (p, n, stream, kept)


def test_dropout_reference_streams_and_seeds_differ_and_counter_adds():
    a = R.dropout_scale(0.5, R.DROPOUT_SEED, 0, 4096)
    assert (a != R.dropout_scale(0.5, R.DROPOUT_SEED, 3, 4096)).mean() > 0.4
    assert (a != R.dropout_scale(0.5, R.DROPOUT_SEED + 1, 0, 4096)).mean() > 0.4
    assert np.array_equal(R.dropout_scale(0.5, R.DROPOUT_SEED, 0, 100, first=50), a[50:150])


# ---- 4. every gate is reachable: the reference evaluated in fp32 on the CPU passes the gate its GPU test applies ------------------------
@pytest.mark.parametrize("bf16", [0, 1])
def test_gate_reachable_gemm_rounded(bf16):
    for case, act in [(R.GEMM_ROUNDED, 0)] + [(c, 1) for c in R.GEMM_ACT]:
        A, B, C0, bias, resid = R.gemm_operands(case, "gauss")
        A32, B32 = A.float(), B.float()
        if bf16:
            A32, B32 = A32.bfloat16().float(), B32.bfloat16().float()
        want = R.gemm(A32, B32, C0, bias, resid, act)

        def f32(a, b):
            v = torch.einsum("zmk,znk->zmn", a, b)
            if bias is not None:
                v = v + bias.float()
            return F.gelu(v, approximate="tanh") if act else v

        G.check_close(f32(A32, B32), want, G.F32, case["name"])
        if bf16:  # and the gate tells rounding from truncation: operands cut to bf16 miss it
            cut = lambda t: (t.float().view(torch.int32) & -65536).view(torch.float32)  # noqa: E731
            with pytest.raises(AssertionError):
                G.check_close(f32(cut(A), cut(B)), want, G.F32, "cut")


@pytest.mark.parametrize("N", R.GEMM_LN_N)
def test_gate_reachable_gemm_ln(N):
    case = R.gemm_case(f"ln-N{N}", R.GEMM_LN_M, N, R.GEMM_LN_K, bias=1, resid=1)
    A, B, _, bias, resid = R.gemm_operands(case, "gauss")
    _, _, gamma, beta = R.ln_inputs(case["name"], 1, N)
    want = R.layernorm(R.gemm(A, B, None, bias, resid)[0], None, gamma, beta)[0]
    v = (A[0].float() @ B[0].float().T + bias.float() + resid[0].float())
    G.check_close(R.layernorm_f32(v, None, gamma, beta)[0], want, G.F32, case["name"])


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("N", R.LN_N)
def test_gate_reachable_layernorm(N, bf16):
    M = max(R.LN_M)
    x, add, gamma, beta = R.ln_inputs(f"ln{M}.{N}.{int(bf16)}", M, N, bf16)
    y, v, mean, rstd = R.layernorm(x, add, gamma, beta)
    y32, v32, m32, r32 = R.layernorm_f32(x, add, gamma, beta)
    G.check_close(y32, y, G.F32, "y")
    assert torch.equal(v32.double(), v), "the pre-norm rows are exact in fp32"
    R.gate(R.stat_errors(torch.stack([m32, r32], 1), mean, rstd), torch.zeros(2 * M), "stat", std=1.0)


def test_gate_reachable_layernorm_offset_rows():
    o = R.LN_OFFSET
    x, _, gamma, beta = R.ln_inputs("ln.offset", o["M"], o["N"], offset=o["mean"])
    tol, cpu = R.offset_gate(x, gamma, beta)
    assert tol[0] >= G.TOL[G.F32]["mx"] and tol[1] >= G.TOL[G.F32]["rms"] and tol[0] < 1e-3
    want = R.layernorm(x, None, gamma, beta)[0]
    R.gate(R.layernorm_f32(x, None, gamma, beta)[0], want, "two-pass fp32", tol=tol)
    # the case separates the two formulas: E[x^2] - mean^2 in fp32 on the same rows misses the gate
    v = x.float()
    var1 = (v * v).mean(1, keepdim=True) - v.mean(1, keepdim=True).square()
    y1 = (v - v.mean(1, keepdim=True)) / torch.sqrt(var1 + R.LN_EPS) * gamma + beta
    with pytest.raises(AssertionError):
        R.gate(y1, want, "one-pass fp32", tol=tol)


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("N", R.LN_BWD_N)
def test_gate_reachable_ln_backward(N, add):
    M = max(R.LN_BWD_M)
    x, a, gamma, beta = R.ln_inputs(f"lnb{M}.{N}.{int(add)}", M, N, bf16=add, add_rows=R.LN_BWD_ADD_ROWS if add else 0)
    dy = R.gaussian(f"lnb{M}.{N}.dy", (M, N)).float()
    _, v, mean, rstd = R.layernorm(x, a, gamma, beta)
    m32, r32 = mean.float(), rstd.float()
    want = R.ln_bwd(dy, v, m32, r32, gamma)
    xh = (v.float() - m32[:, None]) * r32[:, None]
    gd = dy * gamma
    dx = r32[:, None] * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True))
    for got, w, what in ((dx, want[0], "dx"), ((dy * xh).sum(0), want[1], "dgamma"), (dy.sum(0), want[2], "dbeta")):
        G.check_close(got, w, G.F32, what)


def test_gate_reachable_gelu_and_transpose():
    aux, src = R.gelu_inputs()
    w0, w1 = R.gelu_new(aux.double()), src.double() * R.dgelu_new(aux.double())
    t = torch.tanh(0.7978845608028654 * (aux + 0.044715 * aux * aux * aux))
    g0 = F.gelu(aux, approximate="tanh")
    g1 = src * (0.5 * (1.0 + t) + 0.5 * aux * (1.0 - t * t) * 0.7978845608028654 * (1.0 + 3.0 * 0.044715 * aux * aux))
    for n in R.GELU_N:
        R.gate(g0[:n], w0[:n], f"gelu n={n}", std=w0.std())
        R.gate(g1[:n], w1[:n], f"gelu' n={n}", std=w1.std())
    for r, c in R.TRANSPOSE_SHAPES:
        x = (2.0 * R.gaussian(f"tr{r}.{c}", (r, c))).float()
        R.gate(F.gelu(x, approximate="tanh").T, R.gelu_new(x.double()).T, "transpose + gelu", std=R.gelu_new(2.0 * R.gaussian("tr.unit", (4096,))).std())


def test_colsum_reference_is_the_rounded_exact_sum():
    import math
    for B in R.COLSUM_B:
        src = R.gaussian(f"cs{B}", (B, 17)).float()
        want = torch.tensor([math.fsum(src[:, c].double().tolist()) for c in range(17)], dtype=torch.float64).float()
        assert torch.equal(R.colsum(src), want)
        d = X.dyadic(f"csd{B}", (B, 17), 64, 3)
        assert torch.equal(R.colsum(d.float()).double(), d.sum(0))
