"""The fused dense path of the FNet inference walk (csrc/fnet_dense.hip: fnet_fold_kernel, fnet_table_kernel, fnet_dense_kernel,
fnet_mix2_kernel) one kernel at a time through ddimx_fnet_fold / ddimx_fnet_table / ddimx_fnet_dense / ddimx_fnet_mix2, against the
fp64 references of tests/fnet_dense_ref.py.

In every case: each output lives in a sentinel-filled allocation with guard bands (``Out`` of tests/kernel_harness.py, in its `idx`
form) and must hold the sentinel byte 0xFF -- a NaN in fp32 and bf16 -- everywhere but in its logical elements afterwards, the rows
>= S of the chunk-major and statistics layouts included; every chunk-major and statistics INPUT (``placed``, same module) holds NaN in
its rows >= S, so a kernel that lets a padding row into a sum poisons its output; the batch is three samples and sample 1 run alone
must give its rows of the batch bit for bit.  Integer cases compare bit for bit in both precisions; Gaussian cases at the gates of
fnet_dense_ref.dense_gate, and print the measured worst errors."""
import numpy as np
import pytest
import torch

from ddim_audio_amd import _lib
import exact_util as X
import fnet_dense_ref as D
import fnet_kernel_ref as R
import gpu_util as G
from kernel_harness import Out, dev32, lib as load_lib, placed, refused, report_std as report, same

pytestmark = pytest.mark.gpu
B = 3
HID = D.HID


def packed(W, bf16):
    """W [N][K] in fragment order, fp32 or rounded to bf16 (every element of the buffer is a weight)."""
    dt = torch.bfloat16 if bf16 else torch.float32
    buf = torch.empty(W.numel(), dtype=dt)
    buf[D.frag_index(W.shape[0], W.shape[1], bf16).reshape(-1)] = W.reshape(-1).float().to(dt)
    return buf.to(G.dev())


def tokens(x, layout):
    """x [B][S][K] in a token layout ('row', 'c4', 'c8'), NaN in the rows >= S of the chunk blocks."""
    b, s, k = x.shape
    return placed(x, D.layout_index(layout, b, s, k), size=b * (s if layout == "row" else 32) * k,
                  dtype=torch.bfloat16 if layout == "c8" else torch.float32)


def stats_in(st):
    """st [B][S][nparts][2] in the statistics layout, NaN in rows >= S."""
    b, s, p, _ = st.shape
    return placed(st, D.stats_index(b, s, p), size=b * p * 64)


def call_dense(a, p, act, eps, nb, bf16):
    """ddimx_fnet_dense with the flags of `a` (fnet_dense_ref.dense_args) and the pointers of `p`."""
    g = lambda k: p.get(k)  # noqa: E731
    return load_lib().ddimx_fnet_dense(g("W"), g("bias"), g("X"), g("xstats"), a["xnp"], a["xn"], g("out"), int(a["x_chunk"]), int(a["x_bf16"]),
                                    int(a["out_chunk"]), int(a["out_bf16"]), act, g("R"), g("rstats"), g("rgamma"), g("rbeta"), a["rnp"],
                                    a["rn"], g("ostats"), eps, a["S"], a["K"], a["N"], nb, bf16, _lib.stream())


def run_dense(case, o, bf16, sl=slice(None), ext=None):
    """One launch of a case of fnet_dense_ref on the samples `sl` of the operands `o`; ext: device pointers that replace operands
    (a producer's outputs).  Returns (return code, output Out, ostats Out or None)."""
    N, S = case["N"], case["S"]
    nb = o["X"][sl].shape[0]
    keep = dict(W=packed(o["W"], bf16), bias=dev32(o["bias"]))
    if not (ext and "X" in ext):
        keep["X"] = tokens(o["X"][sl], case["x"])
    if case["xnp"] and not (ext and "xstats" in ext):
        keep["xstats"] = stats_in(o["xstats"][sl])
    if case["rnp"]:
        keep.update(R=tokens(o["R"][sl], "c4"), rstats=stats_in(o["rstats"][sl]), rgamma=dev32(o["rgamma"]), rbeta=dev32(o["rbeta"]))
    p = {k: _lib.ptr(v) for k, v in keep.items()}
    p.update(ext or {})
    out = Out(idx=D.layout_index(case["out"], nb, S, N), dtype=torch.bfloat16 if case["out"] == "c8" else torch.float32)
    ost = Out(idx=D.stats_index(nb, S, N // 32)) if case["ostats"] else None
    p.update(out=out.ptr, ostats=ost.ptr if ost else None)
    rc = call_dense(D.dense_args(**case), p, case["act"], o["eps"], nb, bf16)
    torch.cuda.synchronize()
    return rc, out, ost


def accepted(case, bf16):
    return D.dense_dispatch(D.dense_args(**case), bf16) is not None


# ---- fnet_fold ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "gamma-beta"])
@pytest.mark.parametrize("bf16", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,K", D.FOLD_CASES)
def test_fnet_fold(N, K, bf16, affine):
    """fnet_fold_kernel: Wf equals the Python packing of fl(W gamma) -- for bf16 the fp32 product rounded to nearest even -- bit for
    bit, every element written; bf = bias + W beta exact on integer operands and within K 2^-24 sum |terms| on Gaussian ones; with
    beta null bf stays NaN.  Measured on MI355X: worst |bf - bf64| = 0.053 of that bound at K = 16, 0.016 at K = 48, below 0.001 at K >= 512."""
    lib = load_lib()
    worst = 0.0
    for kind in ("exact", "gauss"):
        t = f"fold{N}.{K}.{kind}"
        mk = (lambda tag, shape: R.ints(t + tag, shape)) if kind == "exact" else (lambda tag, shape: R.gaussian(t + tag, shape).float().double())
        W, bias = mk("W", (N, K)), mk("b", (N,))
        gamma, beta = (mk("g", (K,)), mk("be", (K,))) if affine else (None, None)
        Wd, bd, gd, bed = dev32(W), dev32(bias), None if gamma is None else dev32(gamma), None if beta is None else dev32(beta)
        wf = Out(idx=D.frag_index(N, K, bf16), dtype=torch.bfloat16 if bf16 else torch.float32)
        bf = Out(N)
        _lib.check(lib.ddimx_fnet_fold(_lib.ptr(Wd), _lib.ptr(gd), _lib.ptr(bed), _lib.ptr(bd), wf.ptr, bf16, bf.ptr, N, K, _lib.stream()))
        torch.cuda.synchronize()
        got = wf.read(f"fold {t} Wf")
        assert bool(torch.isfinite(got.float()).all()), "every element of Wf is written"
        want = W.float() * gamma.float() if affine else W.float()
        same(got, want.bfloat16() if bf16 else want, f"{t}: Wf")
        if not affine:
            assert bf.untouched()
            continue
        want_bf = D.fold_weights(W, gamma, beta, bias)[1]
        gbf = bf.read(f"fold {t} bf").double()
        if kind == "exact":
            assert torch.equal(gbf, want_bf), f"{t}: bf on integers"
        else:
            bound = K * 2.0 ** -24 * (bias.abs() + (W * beta).abs().sum(1))
            assert bool(((gbf - want_bf).abs() <= bound).all()), f"{t}: bf"
            worst = max(worst, float(((gbf - want_bf).abs() / bound).max()))
    if affine:
        print(f"[fold N={N} K={K} bf16={bf16}] worst |bf - bf64| = {worst:.3f} of K 2^-24 sum|terms|")


# ---- fnet_table --------------------------------------------------------------------------------------------------------------------------
def run_table(gamma, beta, H):
    lib = load_lib()
    gd, bd = None if gamma is None else dev32(gamma), None if beta is None else dev32(beta)
    tab, bc = Out(idx=D.frag_index(2 * H, H, False)), Out(H)
    _lib.check(lib.ddimx_fnet_table(_lib.ptr(gd), _lib.ptr(bd), tab.ptr, bc.ptr, H, _lib.stream()))
    torch.cuda.synchronize()
    return tab, bc


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "gamma-beta"])
@pytest.mark.parametrize("H", D.TABLE_H)
def test_fnet_table(H, affine):
    """fnet_table_kernel: every slot of the fragment-order table written and nothing else, each entry within one fp32 ulp of
    fl(trig64) gamma (the device's fp64 cos / sin may differ from numpy's in the last place); |bc - bc64| <= 2^-23 sum |cos beta|;
    beta null: bc untouched.  Measured on MI355X: 0 of 2 048 / 8 192 / 524 288 entries differ from the correctly rounded
    product, with and without gamma."""
    gamma = (1.0 + 0.3 * R.gaussian(f"tab{H}.g", (H,))).float().double() if affine else None
    beta = (0.2 * R.gaussian(f"tab{H}.b", (H,))).float().double() if affine else None
    tab, bc = run_table(gamma, beta, H)
    got = tab.read(f"table H={H}").double()
    assert bool(torch.isfinite(got).all()), "every slot of the table is written"
    want, bc64 = D.table(gamma, beta, H)
    assert bool(((got - want).abs() <= X.ulp(want, 24)).all()), "an entry is more than one fp32 ulp from fl(trig) gamma"
    print(f"[table H={H} affine={affine}] {int((got != want.float().double()).sum())} of {want.numel()} entries differ from the rounded product")
    if not affine:
        assert bc.untouched()
        return
    c = D.table(None, None, H)[0][0::2]
    bound = 2.0 ** -23 * (c.abs() * beta.abs()).sum(1)
    assert bool(((bc.read("bc").double() - bc64).abs() <= bound).all())


# ---- fnet_dense, exact -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.DENSE_EXACT, ids=lambda c: c["name"])
def test_fnet_dense_exact(case):
    """fnet_dense_kernel on integer operands (|v| <= 3) with hand-made dyadic statistics and eps = 0: the fold returns exactly the
    integer mean and rstd 2^-k, so the normalised operand, the product, the bias and the LN(R) residual are exact, and the fp32
    and the bf16 launch must both equal the fp64 result bit for bit (a bf16 output: its nearest-even rounding).  The 'between'
    statistics give the parts different sums around the row mean, so the between-part term of Chan's fold carries a quarter of the
    variance.  ostats: part sums exact, m2 exact where its budget allows and within 32 * 2^-24 * sum of terms otherwise.  A
    precision whose launcher has no kernel for the argument set must return an error and leave the outputs untouched."""
    lib = load_lib()
    assert bool(lib.ddimx_fnet_dense_supported(case["S"], case["K"], case["N"])) == D.fnet_dense_supported(case["S"], case["K"], case["N"])
    o = D.dense_operands(case, "exact")
    want = D.dense_want(case, o)
    ran = []
    for bf in (0, 1):
        rc, out, ost = run_dense(case, o, bf)
        if not accepted(case, bf):
            refused(rc, *([out] if ost is None else [out, ost]), who="fnet_dense_launch")
            continue
        _lib.check(rc)
        what = f"{case['name']} bf16={bf}"
        got = out.read(what)
        wo = D.bf16r(want) if case["out"] == "c8" else want
        bad = got.double() != wo
        if bad.any():
            b, s, n = (int(v[0]) for v in bad.nonzero(as_tuple=True))
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at sample {b} row {s} feature {n}: got "
                                 f"{float(got[b, s, n])!r}, exact {float(wo[b, s, n])!r}")
        st = None
        if ost is not None:
            st = ost.read(what + " ostats")
            D.m2_check(st, want, case["N"] // 32, -1 if case["xnp"] or case["rnp"] else 0, what)
        rc1, out1, ost1 = run_dense(case, o, bf, slice(1, 2))
        _lib.check(rc1)
        same(out1.read(what + " alone"), got[1:2], f"{what}: sample 1 alone differs from its rows of the batch")
        if ost1 is not None:
            same(ost1.read(what + " ostats alone"), st[1:2])
        ran.append(got)
    assert ran, "no precision takes this case"


# ---- fnet_dense, Gaussian ----------------------------------------------------------------------------------------------------------------
def _check_gauss(case, o, bf, ext=None):
    want, tol = D.dense_gate(case, o, bf)
    what = f"{case['name']} bf16={bf}"
    rc, out, ost = run_dense(case, o, bf, ext=ext)
    _lib.check(rc)
    got = out.read(what).float()
    mx, rms = R.gate(got, want, what, tol=tol)
    print(f"[{what}] max {mx:.2e} rms {rms:.2e} of std; gate {tol[0]:.2e} / {tol[1]:.2e}")
    st = None
    if ost is not None:  # the statistics of the output the kernel wrote, against fp64 statistics of those very rows
        st = ost.read(what + " ostats")
        ws = D.part_stats(got.double(), case["N"] // 32)
        for c, name in ((0, "sum"), (1, "m2")):
            report(f"{what} ostats {name}", *R.gate(st[..., c], ws[..., c], f"{what} ostats {name}"))
    if ext is None:
        rc1, out1, ost1 = run_dense(case, o, bf, slice(1, 2))
        _lib.check(rc1)
        same(out1.read(what + " alone").float(), got[1:2], f"{what}: sample 1 alone differs from its rows of the batch")
        if ost1 is not None:
            same(ost1.read(what + " ostats alone"), st[1:2])
    return got, out, ost


@pytest.mark.parametrize("case,bf", [(c, bf) for c in D.DENSE_GAUSS for bf in (0, 1) if accepted(c, bf)],
                         ids=lambda v: v["name"] if isinstance(v, dict) else ("bf16" if v else "f32"))
def test_fnet_dense_gaussian(case, bf):
    """Gaussian operands, the statistics of the rows themselves (fp64 part statistics rounded to fp32), gelu on and off, centred
    rows and offset rows (mean 32) as the normalised operand and as R.  fp32 path: the fp32 gate (offset rows: offset_gate).  bf16
    path: bf16-rounded weights times tokens normalised in fp64 and rounded to bf16, within 1 x the yardstick (the error rounding the
    tokens causes in the reference itself; tokens stored in bf16 are not rounded again: fp32 gate); a bf16 output adds its rounding.
    Measured on MI355X (max / rms of std): fp32 path, centred rows 2.0e-6 / 3.3e-7, offset rows 1.9e-5 / 2.0e-6.  bf16 path with fp32
    tokens: centred rows 1.0e-6 / 1.3e-7 (1e-4 x the yardstick 1.0e-2 / 1.8e-3), offset rows 1.6e-3 / 5.7e-5 (0.13 / 0.03 x the
    yardstick: roundings that flip); with bf16 tokens 5.4e-6 / 1.2e-6; bf16 outputs 1.28e-2 / 1.82e-3 against 2.41e-2 / 3.66e-3 and
    7.3e-3 / 1.7e-3 against 1.29e-2 / 3.21e-3 (the output's own rounding).  ostats: 3.4e-7 / 9.1e-8 at most."""
    _check_gauss(case, D.dense_operands(case, "gauss"), bf)


@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
def test_fnet_dense_chain(bf):
    """ostats of one launch (deep, 16 parts of 32) are the xstats of the next (wide, gelu): the second launch is compared with the
    reference on the rows the first one wrote and their fp64 statistics."""
    c0, c1 = D.CHAIN
    got0, out0, ost0 = _check_gauss(c0, D.dense_operands(c0, "gauss"), bf)
    o1 = D.dense_operands(c1, "gauss")
    o1["X"] = got0.double()
    o1["xfold"] = D.fold(D.part_stats(o1["X"], c1["xnp"]), c1["xn"], o1["eps"])
    _check_gauss(c1, o1, bf, ext=dict(X=out0.ptr, xstats=ost0.ptr))


# ---- fnet_mix2 ---------------------------------------------------------------------------------------------------------------------------
def run_mix2(S, tab_ptr, dseq, V_ptr, vstats_ptr, gamma, beta, bc_ptr, nb, eps):
    lib = load_lib()
    ds, gd, bd = dev32(dseq), None if gamma is None else dev32(gamma), None if beta is None else dev32(beta)
    zc, zst = Out(idx=D.chunk_index(nb, S, HID, 4)), Out(idx=D.stats_index(nb, S, HID // 16))
    _lib.check(lib.ddimx_fnet_mix2(tab_ptr, _lib.ptr(ds), V_ptr, vstats_ptr, _lib.ptr(gd), _lib.ptr(bd), bc_ptr, zc.ptr, zst.ptr, eps, S, HID, nb,
                                   _lib.stream()))
    torch.cuda.synchronize()
    return zc, zst


@pytest.mark.parametrize("norm,stat", [(False, "uniform"), (True, "uniform"), (True, "between")], ids=["plain", "norm-uniform", "norm-between"])
@pytest.mark.parametrize("S", D.S_MIX)
def test_fnet_mix2_exact(S, norm, stat):
    """fnet_mix2_kernel with sparse integer tables ({0, +-1}) in the tab and dft_seq positions, integer V, dyadic vstats, integer
    gamma / beta / bc and eps = 0: zc is the table form of the reference bit for bit, S bc appears on row 0 and on no other row,
    the zstats sums are exact and m2 follows its budget."""
    o = D.mix2_exact_operands(S, norm, B, stat)
    want = D.mix2_table(o["V"], o["tab"], o["dseq"], o["vfold"], o["gamma"], o["beta"], o["bc"])
    tab = packed(o["tab"], 0)
    bc = dev32(o["bc"]) if norm else None

    def go(sl):
        V = tokens(o["V"][sl], "c4")
        vs = stats_in(o["vstats"][sl]) if norm else None
        zc, zst = run_mix2(S, _lib.ptr(tab), o["dseq"], _lib.ptr(V), _lib.ptr(vs), o["gamma"], o["beta"], _lib.ptr(bc), V.numel() // (32 * HID), 0.0)
        return zc.read(f"mix2 S={S} zc"), zst.read(f"mix2 S={S} zstats")

    got, st = go(slice(None))
    assert torch.equal(got.double(), want), f"{int((got.double() != want).sum())} elements differ"
    if norm:
        d = got.double() - D.mix2_table(o["V"], o["tab"], o["dseq"], o["vfold"], o["gamma"], o["beta"], torch.zeros(HID))
        assert torch.equal(d[:, 0], (S * o["bc"]).expand(B, HID)) and not bool(d[:, 1:].any()), "S bc belongs to row 0 alone"
    n_exact = D.m2_check(st, want, HID // 16, -1 if norm else 0, f"mix2 S={S} zstats")
    print(f"[mix2 exact S={S} norm={norm}] {n_exact} of {st[..., 1].numel()} m2 entries held to exactness")
    got1, st1 = go(slice(1, 2))
    same(got1, got[1:2], "sample 1 alone differs from its rows of the batch")
    same(st1, st[1:2], "sample 1 alone differs from its rows of the batch (zstats)")


def _dseq(S):
    from ddim_audio_amd.model import _dft_tables
    cs, ss = _dft_tables(S)
    return torch.from_numpy(np.concatenate([cs, -ss], axis=1)).contiguous()


@pytest.mark.parametrize("mode", D.MIX2_MODES)
@pytest.mark.parametrize("S", D.S_MIX)
def test_fnet_mix2_real(S, mode):
    """fnet_mix2_kernel with the tables of ddimx_fnet_table and model.py's dft_seq against Re(fftn(X)) + X in fp64 at the fp32 gate
    (max 1e-4, rms 2e-5 of std), zstats against the fp64 part statistics of the reference.  With the normalisation, V and vstats are
    what a preceding ddimx_fnet_dense(.., ostats) wrote (offset: its bias is 32), and the reference normalises those very rows.
    Measured on MI355X (max / rms of std): centred rows, with and without the normalisation, 1.7e-6 / 2.5e-7; offset rows 1.5e-5, 1.1e-5,
    2.0e-5, 2.7e-5 at S = 8, 16, 24, 32 (rms 4.4e-7 at most; without frequency 0: 1.6e-6 / 2.7e-7); zstats 7.4e-6 / 4.5e-7 at most.
    The offset rows are what made the kernel keep the row mean in two parts (fold_row_stats2): with a single fp32 mean the error of
    the mean, common to the 512 elements of a row, added up at output frequency 0 to max 7.5e-5, 1.10e-4, 1.07e-4, 8.3e-5 at S = 8, 16,
    24, 32, above the gate at two of them, while every other frequency was within 3.6e-6."""
    norm = mode != "plain"
    gamma, beta, prod = D.mix2_real_case(S, mode)
    tab, bc = run_table(gamma, beta, HID)
    tab.read("tab")

    def go(sl):
        if not norm:
            V = prod[sl]
            Vd = tokens(V, "c4")
            zc, zst = run_mix2(S, tab.ptr, _dseq(S), _lib.ptr(Vd), None, None, None, None, V.shape[0], R.LN_EPS)
            return V, None, zc.read("zc"), zst.read("zstats")
        rc, out, ost = run_dense(prod[0], prod[1], 0, sl)
        _lib.check(rc)
        V = out.read("V").double()
        zc, zst = run_mix2(S, tab.ptr, _dseq(S), out.ptr, ost.ptr, gamma, beta, bc.ptr, V.shape[0], R.LN_EPS)
        return V, D.fold(D.part_stats(V, 16), HID // 16, R.LN_EPS), zc.read("zc"), zst.read("zstats")

    V, vfold, got, st = go(slice(None))
    want = D.mix2_fft(V, vfold, gamma, beta)
    if mode == "norm-offset":
        assert abs(float(V.mean()) - D.OFFSET) < 1.0
    e = D.errors(got, want)
    e0 = D.errors(got[..., 1:], want[..., 1:], want.std())
    print(f"[mix2 S={S} {mode}] max {e[0]:.2e} rms {e[1]:.2e} of std; without frequency 0: max {e0[0]:.2e} rms {e0[1]:.2e}")
    ws = D.part_stats(want, HID // 16)
    for c, name in ((0, "sum"), (1, "m2")):
        report(f"mix2 S={S} {mode} zstats {name}", *R.gate(st[..., c], ws[..., c], f"zstats {name}"))
    _, _, got1, st1 = go(slice(1, 2))
    same(got1, got[1:2], "sample 1 alone differs from its rows of the batch")
    same(st1, st[1:2], "sample 1 alone differs from its rows of the batch (zstats)")
    R.gate(got, want, f"mix2 S={S} {mode}")


# ---- one layer end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("S", [8, 24])
def test_one_layer_through_the_exports(S, bf):
    """ddimx_layernorm(chunk_rows = S), projection, mix2, ffn1, ffn2 (LN(Z) residual + ostats), mix2 with the normalisation: the
    launches of one layer of run_fnet and the next layer's mixing, weights and tables packed by ddimx_fnet_fold / ddimx_fnet_table,
    every buffer NaN-poisoned, against the composed reference (fnet_dense_ref.walk, which test_fnet_dense_cpu.py proves equal to
    the Transformer_Module) started from the rows the LayerNorm kernel wrote.  fp32: the fp32 gate; bf16: the yardstick, the error
    rounding the token operands to bf16 causes in the composed reference itself.
    Measured on MI355X (max / rms of std): fp32 2.1e-6 / 4.5e-7; bf16 2.2e-4 / 2.7e-5 = 0.034 / 0.015 x the yardstick
    (6.4e-3 / 1.8e-3 at S = 8, 8.0e-3 / 1.9e-3 at S = 24)."""
    lib = load_lib()
    width, inter = 2048, 2048
    P = D.walk_params(f"layer{S}", width, HID, inter, 1)
    L = P["layers"][0]
    x_all = R.gaussian(f"layer{S}.x", (B * S, width)).float()
    dseq = _dseq(S)

    def fold_(W, g, b, bias):
        N, K = W.shape
        keep = [dev32(W), None if g is None else dev32(g), None if b is None else dev32(b), dev32(bias)]
        wf, bfo = Out(idx=D.frag_index(N, K, bf), dtype=torch.bfloat16 if bf else torch.float32), Out(N)
        _lib.check(lib.ddimx_fnet_fold(*[_lib.ptr(k) for k in keep], wf.ptr, bf, bfo.ptr, N, K, _lib.stream()))
        torch.cuda.synchronize()
        wf.read("Wf")
        return wf, (bfo if b is not None else None), keep

    wp, _, kp = fold_(P["proj"][0], None, None, P["proj"][1])
    w1, b1f, _k1 = fold_(L["ffn1"][0], L["ln1"][0], L["ln1"][1], L["ffn1"][1])
    w2, _, k2 = fold_(L["ffn2"][0], None, None, L["ffn2"][1])
    b1f.read("b1f")
    tab0, _ = run_table(None, None, HID)
    tab1, bc1 = run_table(L["ln2"][0], L["ln2"][1], HID)
    g1, be1 = dev32(L["ln1"][0]), dev32(L["ln1"][1])

    def go(x):
        nb = x.shape[0] // S
        xd, g0, b0 = dev32(x), dev32(P["ln0"][0]), dev32(P["ln0"][1])
        y = Out(idx=R.chunk_index(nb * S, width, S))
        _lib.check(lib.ddimx_layernorm(G.F32, _lib.ptr(xd), None, 0, _lib.ptr(g0), _lib.ptr(b0), R.LN_EPS, y.ptr, nb * S, width, S, _lib.stream()))
        vc = Out(idx=D.chunk_index(nb, S, HID, 4))
        a = D.dense_args(S, width, HID)
        _lib.check(call_dense(a, dict(W=wp.ptr, bias=_lib.ptr(kp[3]), X=y.ptr, out=vc.ptr), 0, R.LN_EPS, nb, bf))
        zc, pz = run_mix2(S, tab0.ptr, dseq, vc.ptr, None, None, None, None, nb, R.LN_EPS)
        hc = Out(idx=D.chunk_index(nb, S, inter, 8 if bf else 4), dtype=torch.bfloat16 if bf else torch.float32)
        a = D.dense_args(S, HID, inter, xnp=HID // 16, xn=16, out="c8" if bf else "c4")
        _lib.check(call_dense(a, dict(W=w1.ptr, bias=b1f.ptr, X=zc.ptr, xstats=pz.ptr, out=hc.ptr), 1, R.LN_EPS, nb, bf))
        v2, pv = Out(idx=D.chunk_index(nb, S, HID, 4)), Out(idx=D.stats_index(nb, S, HID // 32))
        a = D.dense_args(S, inter, HID, x="c8" if bf else "c4", rnp=HID // 16, rn=16, ostats=True)
        _lib.check(call_dense(a, dict(W=w2.ptr, bias=_lib.ptr(k2[3]), X=hc.ptr, out=v2.ptr, R=zc.ptr, rstats=pz.ptr, rgamma=_lib.ptr(g1),
                                      rbeta=_lib.ptr(be1), ostats=pv.ptr), 0, R.LN_EPS, nb, bf))
        z2, pz2 = run_mix2(S, tab1.ptr, dseq, v2.ptr, pv.ptr, L["ln2"][0], L["ln2"][1], bc1.ptr, nb, R.LN_EPS)
        for o_, name in ((vc, "vc"), (zc, "zc"), (pz, "pz"), (hc, "hc"), (v2, "v2"), (pv, "pv"), (pz2, "pz2")):
            o_.read(name)  # (nothing outside the logical elements was written)
        return y.read("ln0").reshape(nb, S, width), z2.read("z2")

    h0, got = go(x_all)
    ref = D.walk(P, h0.double(), R.LN_EPS, bf16=bool(bf), final="mix", f32fold=True)["final"]
    what = f"one layer S={S} bf16={bf}"
    if bf:
        tol = D.bf16_yardstick(ref, D.walk(P, h0.double(), R.LN_EPS, bf16=True, round_tokens=False, final="mix", f32fold=True)["final"])
        mx, rms = R.gate(got, ref, what, tol=tol)
        print(f"[{what}] max {mx:.2e} rms {rms:.2e} of std = {mx / tol[0]:.3f} / {rms / tol[1]:.3f} of the yardstick {tol[0]:.2e} / {tol[1]:.2e}")
    else:
        report(what, *R.gate(got, ref, what))
    _, got1 = go(x_all[S:2 * S])
    same(got1, got[1:2], "sample 1 alone differs from its rows of the batch")


# ---- launcher rejections (argument checks: nothing is launched) ----------------------------------------------------------------------------
_WIDE = dict(S=8, K=512, N=256, x="c4", xnp=32, xn=16, out="c4")
_DEEP = dict(S=8, K=2048, N=512, x="c4", out="c4")
REJECT = {
    "S=0": (dict(_WIDE, S=0), 0, {}),
    "S=33": (dict(_WIDE, S=33), 0, {}),
    "K=256": (dict(_WIDE, K=256, xn=8), 0, {}),
    "deep-too-few-steps": (dict(_DEEP, K=512, N=64), 0, {}),
    "xnp=36": (dict(_WIDE, xnp=36), 0, {}),
    "xnp=6": (dict(_WIDE, xnp=6), 0, {}),
    "x_bf16-without-chunk": (dict(_DEEP), 1, dict(x_chunk=False, x_bf16=True)),
    "res-on-wide": (dict(_WIDE, rnp=32, rn=8), 0, {}),
    "rnp=40": (dict(_DEEP, rnp=40, rn=16), 0, {}),
    "out_bf16-on-fp32": (dict(_WIDE, out="c8"), 0, {}),
}
ACCEPT = {"wide": (_WIDE, 0), "wide-bf16-out": (dict(_WIDE, out="c8"), 1), "deep": (_DEEP, 0), "deep-res": (dict(_DEEP, rnp=32, rn=16), 0)}
_ZEROS = {}


def _zeros():
    """Operands large enough for any accepted argument set of the tables above (2048 x 2048 floats)."""
    if not _ZEROS:
        _ZEROS["z"] = torch.zeros(2048 * 2048, device=G.dev())
    return _ZEROS["z"]


def _call_with_zeros(desc, bf, override):
    a = D.dense_args(**desc)
    a.update(override)
    z = _lib.ptr(_zeros())
    out, ost = Out(3 * 32 * 2048), Out(3 * 64 * 64)
    p = dict(W=z, bias=z, X=z, xstats=z if a["xstats"] else None, out=out.ptr, ostats=ost.ptr)
    if a["res"]:
        p.update(R=z, rstats=z, rgamma=z, rbeta=z)
    rc = call_dense(a, p, 0, 1e-12, B, bf)
    torch.cuda.synchronize()
    return a, rc, out, ost


@pytest.mark.parametrize("why", list(REJECT))
def test_fnet_dense_rejects(why):
    """Every argument set the dispatch mirror rejects comes back non-zero from the export, with the launcher named in the message,
    and the output allocations stay NaN."""
    desc, bf, override = REJECT[why]
    a, rc, out, ost = _call_with_zeros(desc, bf, override)
    assert D.dense_dispatch(a, bf) is None, "the mirror accepts this set: the table is wrong"
    refused(rc, out, ost, who="fnet_dense_launch")


@pytest.mark.parametrize("which", list(ACCEPT))
def test_fnet_dense_accepts(which):
    """... and the sets next to them that it accepts return zero and write the output and its statistics (zero operands)."""
    desc, bf = ACCEPT[which]
    a, rc, out, ost = _call_with_zeros(desc, bf, {})
    assert D.dense_dispatch(a, bf) is not None
    _lib.check(rc)
    assert not out.untouched() and not ost.untouched(), "the output and its statistics are written"


@pytest.mark.parametrize("S,hid", [(12, 512), (40, 512), (8, 1024)])
def test_fnet_mix2_rejects(S, hid):
    lib = load_lib()
    assert not D.mix2_accepts(S, hid)
    z = _lib.ptr(_zeros())
    zc, zst = Out(3 * 32 * 1024), Out(3 * 64 * 64)
    rc = lib.ddimx_fnet_mix2(z, z, z, None, None, None, None, zc.ptr, zst.ptr, 1e-12, S, hid, B, _lib.stream())
    refused(rc, zc, zst, who="fnet_mix2_launch")
