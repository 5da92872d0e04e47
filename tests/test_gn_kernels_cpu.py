"""The references and case tables of tests/gn_kernel_ref.py, checked without a GPU: the forward fold against F.group_norm, the
backward (statistics, coefficients, apply) against fp64 autograd, every case's launch plan against what the case is meant to reach,
the exactness budget of the dyadic cases, and that every gate the GPU tests apply is one the reference itself meets when it is
evaluated in fp32 with the kernels' partition (a gate the reference cannot meet is a wrong gate)."""
import pytest
import torch
import torch.nn.functional as F

import gn_kernel_ref as R
import gpu_util as G


def _nchw(t, H, W):
    return t.reshape(t.shape[0], H, W, t.shape[2]).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1])


CPU_CASES = [c for c in R.SMALL if c["H"] == 7]


# ---- 1. references against torch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CPU_CASES, ids=R.case_id)
def test_forward_reference_equals_group_norm(c):
    C, H, W = c["C"], c["H"], c["W"]
    x = R.rnd(R.gauss("cpu.fwd." + c["id"], (R.B, H * W, C)) + 0.5, c["dt"])
    gamma, beta = R.gamma_beta("cpu.fwd." + c["id"], C)
    geo = R.geometry(c["dt"], C, H, W)
    st = R.chan_stats(x, geo["rpp"])
    assert st.shape == (R.B, geo["nparts"], C, 2)
    tot = R.fold_groups(st.sum(1))
    gs = R.group_slabs(st)
    assert torch.allclose(gs[..., :16].sum(1).view(R.B, 8, 2), tot, rtol=1e-13, atol=0) and not bool(gs[..., 16:].any())
    scale, shift, mean, rstd = R.gn_fold(tot[..., 0], tot[..., 1], float(H * W * geo["GS"]), gamma, beta, R.EPS)
    want = _nhwc(F.group_norm(_nchw(x, H, W), R.GROUPS, gamma, beta, R.EPS))
    assert torch.allclose(x * scale[:, None, :] + shift[:, None, :], want, rtol=0, atol=1e-10)
    s2, h2, _, _ = R.group_norm_fold(x, gamma, None, R.EPS)
    assert torch.allclose(x * s2[:, None, :] + h2[:, None, :], want - beta, rtol=0, atol=1e-10)
    # the three forms of the residual pass
    h = R.gauss("cpu.fwd.h." + c["id"], (R.B, H * W, C))
    assert torch.equal(R.resid(x, h, 1), x + h)
    assert torch.allclose(R.resid(x, x, 0, scale, shift), x + want, rtol=0, atol=1e-10)
    assert torch.allclose(R.resid(x, h, 2, scale, shift), x + F.silu(h) * scale[:, None, :] + shift[:, None, :], rtol=0, atol=1e-12)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", CPU_CASES, ids=R.case_id)
def test_backward_reference_equals_autograd(c, mode):
    """Mode 0 is GN(SiLU(u)); mode 1 is SiLU(GN(x)) plus the identity path (gy).  The reference composed from statistics,
    coefficients and apply gives autograd's input, gamma and beta gradients to 1e-10."""
    C, H, W = c["C"], c["H"], c["W"]
    d = R.bwd_inputs(c, mode)
    geo = R.geometry(c["dt"], C, H, W)
    # (the norm's constants exactly, not rounded to fp32 as the kernels get them)
    v = R.silu(d["u"]) if mode == 0 else d["u"]
    d["scale"], d["shift"], d["mean"], d["rstd"] = R.group_norm_fold(v, d["gamma"], d["beta"], R.EPS)
    PQ, coef, dgb, out = R.bwd_reference(d, mode, geo["rpp"])
    u = d["u"].clone().requires_grad_(True)
    gamma, beta = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
    if mode == 0:
        y = _nhwc(F.group_norm(_nchw(F.silu(u), H, W), R.GROUPS, gamma, beta, R.EPS))
        (y * d["g"]).sum().backward()
    else:
        y = F.silu(_nhwc(F.group_norm(_nchw(u, H, W), R.GROUPS, gamma, beta, R.EPS)))
        ((y * d["g"]).sum() + (u * d["gy"]).sum()).backward()
    assert float((out - u.grad).abs().max()) <= 1e-10
    assert float((dgb[:, 0].sum(0) - gamma.grad).abs().max()) <= 1e-10 * max(1.0, float(gamma.grad.abs().max()))
    assert float((dgb[:, 1].sum(0) - beta.grad).abs().max()) <= 1e-10 * max(1.0, float(beta.grad.abs().max()))
    if mode == 1:
        withx = R.bwd_apply(d["g"], d["u"], 1, coef, d["scale"], d["shift"], d["gy"], d["extra"])
        assert torch.allclose(withx, u.grad + d["extra"], rtol=0, atol=1e-10)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_projection_terms_are_not_small(c, mode):
    """The cb v + cc part of the output is at least a quarter of the output's rms: a wrong S1 / S2 term cannot hide."""
    d = R.bwd_inputs(c, mode)
    geo = R.geometry(c["dt"], c["C"], c["H"], c["W"])
    _, coef, _, out = R.bwd_reference(d, mode, geo["rpp"])
    sc, sh = (d["scale"], d["shift"]) if mode == 1 else (None, None)
    part = R.projection_part(d["g"], d["u"], mode, coef, sc, sh)
    ratio = float(part.square().mean().sqrt() / out.square().mean().sqrt())
    assert ratio >= 0.25, ratio
    # and SiLU's argument stays where SILU_OPS was counted
    arg = d["u"] if mode == 0 else d["u"] * d["scale"][:, None, :] + d["shift"][:, None, :]
    assert float(arg.abs().max()) <= R.SILU_ARG_MAX


# ---- 2. plans ---------------------------------------------------------------------------------------------------------------------------
def test_cases_reach_what_they_are_meant_to():
    geo = {c["id"]: R.geometry(c["dt"], c["C"], c["H"], c["W"]) for c in R.CASES}
    for c in R.CASES:
        g = geo[c["id"]]
        assert g["threads"] == (192 if c["C"] in (96, 192) else 256), c["id"]
        assert g["threads"] % g["cpp"] == 0 and g["nparts"] == -(-g["HW"] // g["rpp"]), c["id"]
    assert geo["tiny-C256-f32"]["rows"] == 4 and geo["tiny-C32-bf16"]["rows"] == 64
    for c in R.SMALL:
        g = geo[c["id"]]
        assert g["iters"] == 1 and g["HW"] % g["rpp"] != 0, c["id"]  # the last part is ragged
    assert geo["tiny-C32-f32"]["nparts"] == geo["tiny-C32-bf16"]["nparts"] == 1   # one ragged part, most threads idle
    assert all(geo[c["id"]]["nparts"] > 1 for c in R.SMALL if c["H"] == 7)
    g = geo[R.ROUNDS65["id"]]
    assert (g["iters"], g["nparts"]) == (5, 65) and g["iters"] % 4 == 1 and g["iters"] % 2 == 1
    g = geo[R.ITERS16["id"]]
    assert g["iters"] == 16 and g["nparts"] > 64
    # 65 slabs: gn_bwd_finalize and partsum read eight partials on each of eight lanes per round -- 64 -- so a second round runs
    assert 65 in R.MULTI_NPARTS
    # gn_finalize_groups / the fused resid: nthreads / 8 slices of eight partials per round
    lib = R._lib.load()
    for nt in R.GROUPS_NTHREADS:
        nps = R.groups_np(nt)
        assert nt in nps and nt + 1 in nps and max(nps) > R.FUSE_MAX_PARTS
    assert {lib.ddimx_resid_threads(dt, C) for dt in R.DTYPES for C in R.CHANNELS} == {192, 256}
    # the fused resid runs its further-rounds loop only with 192 threads: 193 .. 256 partials
    assert lib.ddimx_resid_threads(G.F32, 96) == 192 and 192 + 1 <= R.FUSE_MAX_PARTS


def test_dyadic_cases_stay_inside_the_exactness_budget():
    for c in R.CASES:
        g = R.geometry(c["dt"], c["C"], c["H"], c["W"])
        # the largest sum any slab entry holds: a whole part of one group
        assert R.dyadic_budget_bits(g["rpp"] * g["GS"]) < 24, c["id"]
        x = R.dyadic_x("cpu.dy." + c["id"], (2, 5, c["C"]))
        assert torch.equal(R.rnd(x, G.BF16), x) and torch.equal(R.rnd(x * x, G.F32), x * x)
    # the reductions of dyadic slabs: at most 65 parts / 19 rows of |v| <= 64 * 2^-3
    assert max(R.MULTI_NPARTS + R.MULTI_B) * 64 * 8 < 2 ** 24


# ---- 3. every gate is met by the reference in fp32 ----------------------------------------------------------------------------------------
F32 = torch.float32


@pytest.mark.parametrize("c", CPU_CASES + [R.ROUNDS65], ids=R.case_id)
def test_fp32_reference_meets_the_forward_gates(c):
    dt, C, H, W = c["dt"], c["C"], c["H"], c["W"]
    geo = R.geometry(dt, C, H, W)
    tag = "cpu.g32." + c["id"]
    x, h = R.rnd(R.gauss(tag + ".x", (R.B, H * W, C)), dt), R.rnd(R.gauss(tag + ".h", (R.B, H * W, C)), dt)
    gamma, beta = R.gamma_beta(tag, C)
    scale, shift, _, _ = (t.float().double() for t in R.group_norm_fold(h, gamma, beta))
    for mode in (0, 1, 2):
        want = R.resid(x, h, mode, scale, shift)
        got = R.resid(x, h, mode, scale, shift, dt=F32).to(R.tdt(dt))
        R.gate_elementwise(got, want, dt, f"resid mode {mode}")
        st = R.chan_stats(got.double(), geo["rpp"])
        st32 = R.chan_stats(got.float(), geo["rpp"], dt=F32)
        ab = torch.stack([R.part_sums(got.double().abs(), geo["rpp"]), st[..., 1]], -1)
        R.gate_sum(st32, st, ab, R.chain(geo), "statistics of y")
        R.gate_sum(R.group_slabs(st32.double()).float(), R.group_slabs(st), R.group_slabs(ab), R.chain(geo, True), "group statistics")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", CPU_CASES + [R.ROUNDS65], ids=R.case_id)
def test_fp32_reference_meets_the_backward_gates(c, mode):
    dt = c["dt"]
    geo = R.geometry(dt, c["C"], c["H"], c["W"])
    d = R.bwd_inputs(c, mode)
    sc, sh = (d["scale"], d["shift"]) if mode == 1 else (None, None)
    PQ, coef, dgb, out = R.bwd_reference(d, mode, geo["rpp"])
    PQ32 = R.bwd_stats(d["g"], d["u"], mode, geo["rpp"], sc, sh, dt=F32)
    ab = R.bwd_abs_slabs(d["g"], d["u"], mode, geo["rpp"], sc, sh)
    R.gate_sum(PQ32, PQ, ab, R.chain(geo) + R.SILU_OPS, "P, Q")
    c32, g32 = R.bwd_coef(PQ32.sum(1), d["count"], d["gamma"], d["mean"], d["rstd"])
    for i, n in enumerate(("ca", "cb", "cc")):
        R.gate(c32[:, i], coef[:, i], n)
    R.gate(g32[:, 0], dgb[:, 0], "dgamma terms")
    R.gate(g32[:, 1], dgb[:, 1], "dbeta terms")
    o32 = R.bwd_apply(d["g"], d["u"], mode, coef.float(), sc, sh, d.get("gy"), dt=F32).to(R.tdt(dt))
    R.gate_elementwise(o32, R.bwd_apply(d["g"], d["u"], mode, coef.float().double(), sc, sh, d.get("gy")), dt, "apply")


@pytest.mark.parametrize("dt", R.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("ratio", R.MEAN_OVER_STD)
def test_fp32_reference_meets_the_widened_rstd_gate(ratio, dt):
    """Group mean over std up to 32: fp32 (sum, sumsq) partials with the kernels' partition, totals and variance in fp64 as the
    finalisations form them.  The widening 1 + mean^2 / var is what makes the gate one that such an implementation meets."""
    c = R.ROUNDS65
    C, HW = c["C"], c["H"] * c["W"]
    geo = R.geometry(c["dt"], C, c["H"], c["W"])
    x = R.numerics_x(f"cpu.num.{ratio}", dt, C, HW, ratio)
    gamma, beta = R.gamma_beta("cpu.num", C)
    want = R.group_norm_fold(x, gamma, beta)
    tot = R.fold_groups(R.chan_stats(x.float(), geo["rpp"], dt=F32).double().sum(1))
    got = R.gn_fold(tot[..., 0], tot[..., 1], float(HW * geo["GS"]), gamma, beta)
    worst = R.gate_stats_of_norm(got[0], got[1], got[2], got[3], want, f"ratio {ratio}")
    assert float(want[3][:, R.CONST_GROUP].min()) == float(want[3][:, R.CONST_GROUP].max()) == pytest.approx(R.EPS32 ** -0.5, rel=1e-12)
    print(f"[fp32 reference, mean/std {ratio}] worst {worst:.2e} of std")


def test_finalisation_reference_on_synthetic_slabs():
    """synthetic_slabs gives (sum, sumsq) of real values, so the folded variance is the values' own."""
    st = R.synthetic_slabs("cpu.syn", 5, 64, offset=2.0)
    tot = R.fold_groups(st.sum(1))
    gamma, beta = R.gamma_beta("cpu.syn", 64)
    _, _, mean, rstd = R.gn_fold(tot[..., 0], tot[..., 1], 5 * 4 * 8.0, gamma, beta)
    assert float((mean - 2.0).abs().max()) < 1.0 and float((1.0 / rstd - 1.0).abs().max()) < 0.5


def test_reduction_references():
    src = R.dyadic_x("cpu.ps", (3, 65, 40)) * 8
    assert torch.equal(R.partsum(src, 2).double(), src[..., ::2].sum(1)) and R.partsum(src, 2).shape == (3, 20)
    assert torch.equal(R.colsum(src[:, 0], 20, 20).double(), src[:, 0, 20:].sum(0))
