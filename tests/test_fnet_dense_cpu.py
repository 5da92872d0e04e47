"""tests/fnet_dense_ref.py against itself, torch.fft and oracle/ref_cpu.py (no GPU): the index maps are bijections, Chan's fold of the
per-part statistics is the direct mean / rstd, the table form of the mixing is the FFT, the references composed as run_fnet composes
the kernels are the Transformer_Module (which proves the folding algebra: W diag(gamma), b + W beta, S bc on row 0, the recomputed
LayerNorm residual), the exact cases fit fp32, the gates are met by an honest fp32 evaluation, and the dispatch mirror takes the
argument sets the walk builds."""
import pytest
import torch
import torch.nn.functional as F

import fnet_dense_ref as D
import fnet_kernel_ref as R

from oracle import ref_cpu


# ---- index maps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("N,K", D.FOLD_CASES + ((1024, 512),))
def test_fragment_order_is_a_bijection(N, K, bf16):
    idx = D.frag_index(N, K, bf16).reshape(-1)
    assert torch.equal(idx.sort().values, torch.arange(N * K))
    # one wave load = the 64 lanes' 16 bytes of one (row block, k step): contiguous
    E = 8 if bf16 else 4
    blk = D.frag_index(N, K, bf16)[:32, :2 * E]
    assert torch.equal(blk.reshape(-1).sort().values, torch.arange(64 * E))


@pytest.mark.parametrize("ch", [4, 8])
@pytest.mark.parametrize("S", D.S_EXACT)
def test_chunk_major_is_a_bijection_apart_from_the_padding_rows(S, ch):
    B, K = 3, 64
    idx = D.chunk_index(B, S, K, ch)
    full = D.chunk_index(B, 32, K, ch)
    assert torch.equal(full.reshape(-1).sort().values, torch.arange(B * 32 * K))
    assert torch.equal(idx, full[:, :S])
    assert idx.reshape(-1).unique().numel() == B * S * K


@pytest.mark.parametrize("nparts", [4, 8, 16, 24, 32])
@pytest.mark.parametrize("S", D.S_EXACT)
def test_statistics_layout_is_a_bijection_apart_from_the_padding_rows(S, nparts):
    B = 3
    full = D.stats_index(B, 32, nparts)
    assert torch.equal(full.reshape(-1).sort().values, torch.arange(B * nparts * 64))
    assert torch.equal(D.stats_index(B, S, nparts), full[:, :S])
    # the two parts of a pair sit side by side: one 16-byte load
    assert torch.equal(full[0, 5, 1], full[0, 5, 0] + 2)


def test_chunk_major_4_agrees_with_the_layernorm_kernels_layout():
    S, N = 8, 64
    assert torch.equal(D.chunk_index(3, S, N, 4).reshape(3 * S, N), R.chunk_index(3 * S, N, S))


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
def _geometries():
    g = {(c["xnp"], c["xn"]) for c in D.DENSE_EXACT + D.DENSE_GAUSS + list(D.CHAIN) if c["xnp"]}
    g |= {(c["rnp"], c["rn"]) for c in D.DENSE_EXACT + D.DENSE_GAUSS if c["rnp"]}
    return sorted(g | {(16, D.HID // 16), (32, 16)})


@pytest.mark.parametrize("nparts,n_part", _geometries())
@pytest.mark.parametrize("offset", [0.0, D.OFFSET])
def test_fold_of_part_stats_is_the_direct_mean_and_rstd(nparts, n_part, offset):
    x = R.gaussian(f"fold{nparts}.{n_part}", (5, nparts * n_part)) + offset
    mean, rstd = D.fold(D.part_stats(x, nparts), n_part, R.LN_EPS)
    _, _, m, r = R.layernorm(x, None, torch.ones(x.shape[1]), torch.zeros(x.shape[1]))
    assert float((mean - m).abs().max()) <= 1e-12 * max(1.0, offset)
    assert float((rstd / r - 1.0).abs().max()) <= 1e-12
    hi, lo, rstd2 = D.fold2(D.part_stats(x, nparts), n_part, R.LN_EPS)
    assert float((hi + lo - m).abs().max()) <= 1e-12 * max(1.0, offset) and float((rstd2 / r - 1.0).abs().max()) <= 1e-12


@pytest.mark.parametrize("kind", ["uniform", "between"])
@pytest.mark.parametrize("nparts,n_part", _geometries())
def test_dyadic_statistics_fold_exactly_in_fp32(nparts, n_part, kind):
    st, m, r = D.dyadic_stats(f"dy{nparts}.{n_part}", 3, 7, nparts, n_part, kind)
    assert torch.equal(st.float().double(), st)
    for dt in (torch.float64, torch.float32):
        mean, rstd = D.fold(st.to(dt), n_part)
        assert torch.equal(mean.double(), m) and torch.equal(rstd.double(), r)
        hi, lo, rstd2 = D.fold2(st.to(dt), n_part)
        assert torch.equal((hi + lo).double(), m) and torch.equal(rstd2.double(), r)
    if kind == "between":  # without the between-part term the variance would be 3/4 of it
        s = st.clone()
        assert float((st[..., 0].sum(-1) / (nparts * n_part) - m).abs().max()) == 0
        assert not torch.equal(1.0 / torch.sqrt(s[..., 1].sum(-1) / (nparts * n_part)), r)
        assert not torch.equal(st[:, :, : nparts // 2, 0].sum(-1) * 2 / (nparts * n_part), m)  # one half of the parts is not the row


# ---- mixing ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("S,H", [(8, 32), (24, 64), (32, 512)])
def test_mix2_table_form_is_the_fft(S, H, norm):
    V = R.gaussian(f"mixcpu{S}.{H}", (2, S, H)) + (3.0 if norm else 0.0)
    gamma, beta = 1.0 + 0.3 * R.gaussian("mixcpu.g", (H,)), 0.2 * R.gaussian("mixcpu.b", (H,))
    if norm:
        stats = D.fold(D.part_stats(V, 16), H // 16, R.LN_EPS)
        tab, bc = D.table(gamma, beta, H, round32=False)
        got = D.mix2_table(V, tab, D.dft_seq(S, False), stats, gamma, beta, bc)
        want = D.mix2_fft(V, stats, gamma, beta)
        x = F.layer_norm(V, (H,), gamma, beta, R.LN_EPS)
        assert float((want - (torch.fft.fftn(x, dim=(1, 2)).real + x)).abs().max()) <= 1e-10 * float(want.std())
    else:
        got = D.mix2_table(V, D.table(None, None, H, round32=False)[0], D.dft_seq(S, False))
        want = D.mix2_fft(V)
    assert float((got - want).abs().max()) <= 1e-10 * float(want.std())


def test_table_matches_the_models_tables():
    from ddim_audio_amd.model import _dft_tables
    import numpy as np
    ch, sh = _dft_tables(64)
    tab, bc = D.table(None, None, 64)
    assert bc is None
    assert torch.equal(tab, torch.from_numpy(np.stack([ch, sh], axis=1).reshape(128, 64)).double())
    cs, ss = _dft_tables(24)
    assert torch.equal(D.dft_seq(24), torch.from_numpy(np.concatenate([cs, -ss], axis=1)).double())


# ---- the composition -------------------------------------------------------------------------------------------------------------------
def test_composed_references_are_the_transformer_module():
    """dense and mix2 composed as run_fnet composes the kernels (fnet_dense_ref.walk) against oracle/ref_cpu.transformer_module in
    fp64: two layers, S = 8, LayerNorm affines far from (1, 0)."""
    B, S, width, hid, inter, L = 2, 8, 48, 32, 64, 2
    P = D.walk_params("cpuwalk", width, hid, inter, L)
    sd, p = {}, "transformer."
    for k, (w, b) in (("embedding.LayerNorm", P["ln0"]), ("embedding.projection", P["proj"]), ("compute_out", P["out"])):
        sd[p + k + ".weight"], sd[p + k + ".bias"] = w, b
    for i, Ly in enumerate(P["layers"]):
        q = f"{p}encoder.layer.{i}."
        for k, key in (("fourier.output.LayerNorm", "ln1"), ("intermediate.dense", "ffn1"), ("output.dense", "ffn2"), ("output.LayerNorm", "ln2")):
            sd[q + k + ".weight"], sd[q + k + ".bias"] = Ly[key]
    x = R.gaussian("cpuwalk.x", (B, S, width))
    want = ref_cpu.transformer_module(sd, x, L, R.LN_EPS)
    pe = ref_cpu.add_encoding(torch.zeros(S, width, dtype=torch.float64))
    h0 = F.layer_norm(x + pe, (width,), P["ln0"][0], P["ln0"][1], R.LN_EPS)
    got = D.walk(P, h0, R.LN_EPS, round32=False)["final"]
    assert float((got - want).abs().max()) <= 1e-10 * float(want.std())
    # ... and the form that ends in the next layer's mixing is the mixing of the last output LayerNorm
    v = D.walk(P, h0, R.LN_EPS, round32=False, final="mix")
    y = F.layer_norm(v["v"][-1], (hid,), P["layers"][-1]["ln2"][0], P["layers"][-1]["ln2"][1], R.LN_EPS)
    m = torch.fft.fftn(y, dim=(1, 2)).real + y
    assert float((v["final"] - m).abs().max()) <= 1e-10 * float(m.std())


# ---- budgets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.DENSE_EXACT, ids=lambda c: c["name"])
def test_exact_dense_cases_fit_fp32(case):
    assert D.budget_bits(case) < 24
    o = D.dense_operands(case, "exact")
    want = D.dense_want(case, o)
    assert torch.equal(want.float().double(), want)
    assert torch.equal(D.dense_want(case, o, bf16=True), want), "integer operands and dyadic statistics are bf16-exact"
    assert float(want.abs().max()) < 2.0 ** D.budget_bits(case)
    for f, n_part in ((o["xfold"], "xn"), (o["rfold"], "rn")):
        if f is not None:
            st = o["xstats" if n_part == "xn" else "rstats"]
            mean, rstd = D.fold(st.float(), case[n_part])
            assert torch.equal(mean.double(), f[0]) and torch.equal(rstd.double(), f[1])


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("S", D.S_MIX)
def test_exact_mix2_cases_fit_fp32(S, norm):
    assert D.mix2_budget_bits(S, norm) < 24
    o = D.mix2_exact_operands(S, norm)
    want = D.mix2_table(o["V"], o["tab"], o["dseq"], o["vfold"], o["gamma"], o["beta"], o["bc"])
    assert torch.equal(want.float().double(), want)
    assert float(want.abs().max()) <= 2.0 ** D.mix2_budget_bits(S, norm)
    assert int((o["tab"] != 0).sum(1).max()) == D.TAB_NNZ and int((o["dseq"] != 0).sum(1).max()) == D.SEQ_NNZ


def test_exact_cases_cover_every_instantiation_and_geometry():
    seen = set()
    for c in D.DENSE_EXACT:
        for bf in (0, 1):
            v = D.dense_dispatch(D.dense_args(**c), bf)
            if v:
                seen.add(v)
    # the launcher's ten kernel instantiations: fp32 wide, deep chunk-major with and without the residual, deep row-major; bf16 wide
    # with fp32 and bf16 output, deep bf16 tokens with and without the residual, deep chunk-major fp32 tokens, deep row-major
    assert len(seen) == 10, sorted(seen)
    assert sum(1 for v in seen if v[6] == 0) == 2, "the two row-major-token instantiations"
    assert {c["S"] for c in D.DENSE_EXACT} == set(D.S_EXACT)
    assert {c["xnp"] for c in D.DENSE_EXACT if c["K"] == 512 and c["xnp"]} == {4, 8, 16, 32}
    assert {(c["N"], c["rnp"]) for c in D.DENSE_EXACT if c["rnp"]} == {(64, 8), (64, 16), (192, 24), (512, 32)}


# ---- the gates -------------------------------------------------------------------------------------------------------------------------
def _dense_f32(case, o, bf16):
    """The operation in fp32 with fp32 statistics folded in the kernel's part geometry (what a sound fp32 kernel computes)."""
    f = lambda t: None if t is None else t.float()  # noqa: E731
    v = f(o["X"])
    if case["xnp"]:
        mean, rstd = D.fold(f(o["xstats"]), case["xn"], torch.tensor(o["eps"], dtype=torch.float32))
        v = v * rstd[..., None] + (-mean * rstd)[..., None]
    w = f(o["W"])
    if bf16:
        w, v = w.bfloat16().float(), v.bfloat16().float()
    out = torch.einsum("bsk,nk->bsn", v, w) + f(o["bias"])
    if case["act"]:
        out = R.gelu_new(out)
    if case["rnp"]:
        mean, rstd = D.fold(f(o["rstats"]), case["rn"], torch.tensor(o["eps"], dtype=torch.float32))
        out = out + ((f(o["R"]) - mean[..., None]) * rstd[..., None]) * f(o["rgamma"]) + f(o["rbeta"])
    return out


@pytest.mark.parametrize("bf16", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", D.DENSE_GAUSS + list(D.CHAIN), ids=lambda c: c["name"])
def test_gated_dense_cases_are_met_by_fp32_arithmetic(case, bf16):
    if D.dense_dispatch(D.dense_args(**case), bf16) is None:
        assert D.dense_dispatch(D.dense_args(**case), 1 - bf16) is not None, "a case no precision takes"
        return
    o = D.dense_operands(case, "gauss")
    want, tol = D.dense_gate(case, o, bf16)
    got = _dense_f32(case, o, bf16)
    if case["out"] == "c8":
        got = got.bfloat16().float()
    mx, rms = D.errors(got, want)
    print(f"[{case['name']} bf16={bf16}] fp32 on the CPU: max {mx:.2e} rms {rms:.2e}; gate {tol[0]:.2e} / {tol[1]:.2e}")
    assert mx <= tol[0] and rms <= tol[1]
    if bf16 and case["x"] != "c8":  # a dropped k element is far outside the yardstick
        o2 = dict(o, W=o["W"].clone())
        o2["W"][:, 5] = 0
        bad = D.errors(D.dense_want(case, o2, True), want)
        assert bad[0] > 2 * tol[0] and bad[1] > 2 * tol[1], (bad, tol)


@pytest.mark.parametrize("mode", D.MIX2_MODES[1:])  # ('plain' normalises nothing: products of fp32 numbers, the GEMM cases' arithmetic)
@pytest.mark.parametrize("S", D.S_MIX)
def test_gated_mix2_cases_are_met_by_fp32_arithmetic(S, mode):
    """The Gaussian cases of fnet_mix2 with the normalisation evaluated in fp32 as the kernel file documents it -- fp32 part
    statistics of V (16 parts of 32), the mean folded as hi + lo (fnet_dense_ref.fold2), the operand fma(v - hi, rstd, -lo rstd) -- and
    everything behind it in fp64, against the fp64 reference on the same V at the fp32 gate (max 1e-4, rms 2e-5 of std).
    On the offset rows (mean 32, std 1) this gives max 1.7e-5 .. 2.6e-5 (rms 3.5e-7 .. 4.5e-7).  A single fp32 mean, normalised by
    one fma, gives 6.0e-5, 7.6e-5, 1.07e-4, 8.2e-5 at S = 8, 16, 24, 32 there (printed for comparison): the error of the mean, a
    quarter of an ulp of 32, is common to the 512 elements of a row, and the hidden DFT adds it up at output frequency 0 -- every other
    frequency is within 3.2e-6.  That is what the kernel did before it kept the mean in two parts."""
    gamma, beta, prod = D.mix2_real_case(S, mode)
    case, o = prod
    V = D.dense_want(case, o).float()
    want = D.mix2_fft(V.double(), D.fold(D.part_stats(V.double(), 16), D.HID // 16, R.LN_EPS), gamma, beta)
    eps = torch.tensor(R.LN_EPS, dtype=torch.float32)

    def through(n):
        x = n.double() * gamma + beta
        got = torch.fft.fftn(x, dim=(1, 2)).real + x
        return got, D.errors(got, want), D.errors(got[..., 1:], want[..., 1:], want.std())

    mean, rstd = D.fold(D.part_stats(V, 16), D.HID // 16, eps)
    _, e1, _ = through((V.double() * rstd.double()[..., None] + (-mean * rstd).double()[..., None]).float())  # fmaf(v, rstd, -mean rstd)
    hi, lo, rstd = D.fold2(D.part_stats(V, 16), D.HID // 16, eps)
    assert hi.dtype == torch.float32 and lo.dtype == torch.float32
    n = ((V - hi[..., None]).double() * rstd.double()[..., None] + (-lo * rstd).double()[..., None]).float()  # fmaf(v - hi, rstd, -lo rstd)
    got, e, e0 = through(n)
    print(f"[mix2 S={S} {mode}] fp32 statistics on the CPU: max {e[0]:.2e} rms {e[1]:.2e}; without frequency 0: max {e0[0]:.2e} rms {e0[1]:.2e}; "
          f"with a single fp32 mean: max {e1[0]:.2e} rms {e1[1]:.2e}")
    R.gate(got, want, f"mix2 S={S} {mode}")


# ---- the dispatch mirror ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("S", [8, 16, 24, 32])
def test_dispatch_mirror_accepts_what_run_fnet_builds(S, bf):
    want = {
        "projection": (bf, False, False, 1, 8, 0, 1, 8 if bf else 16, False),
        "ffn1": (bf, False, bool(bf), 1, 4, 1, 1, 8 if bf else 16, False),
        "ffn2": (bf, bool(bf), False, 1, 8, 0, 1, 16, True),
        "compute_out": (bf, False, False, 1, 4, 1, 1, 8 if bf else 16, False),
    }
    for name, a in D.run_fnet_args(S, bf).items():
        assert D.dense_dispatch(a, bf) == want[name], name
    assert D.mix2_accepts(S, D.HID)  # both mixing launches (with and without vstats) share one rule


def test_dispatch_mirror_rejections():
    ok = dict(S=8, K=512, N=256, x="c4", xnp=32, xn=16, out="c4")
    assert D.dense_dispatch(D.dense_args(**ok), 0) and D.dense_dispatch(D.dense_args(**ok), 1)
    for ch in (dict(S=0), dict(S=33), dict(K=256), dict(N=64, xnp=0, xn=0), dict(xnp=36), dict(xnp=6), dict(x="row"), dict(rnp=32),
               dict(out="c8")):
        a = D.dense_args(**dict(ok, **ch))
        assert D.dense_dispatch(a, 0) is None, ch
    assert D.dense_dispatch(D.dense_args(S=8, K=2048, N=512, rnp=40), 0) is None
    assert not D.mix2_accepts(12, 512) and not D.mix2_accepts(40, 512) and not D.mix2_accepts(8, 1024)
