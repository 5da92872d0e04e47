"""Host checks of the edge-convolution cases (tests/edge_cases.py, run by tests/test_gpu_edge_kernels.py): each case reaches the kernel
variant, tile count, loop trips and reduce path it declares (the library's own ddimx_debug_edge_plan, the function the launchers
call), its operand ranges make every fp32 summation order exact, the fp64 references agree with torch's conv2d and its autograd,
one zeroed tap violates the criterion, and the plan refuses what the exports document.  No GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import exact_util as X
import edge_cases as E
import gn_kernel_ref as R


def _id(c):
    return c["id"]


@pytest.mark.parametrize("case", E.CASES, ids=_id)
def test_case_reaches_what_it_declares(case):
    got = E.plans(case)
    assert set(got) == set(case["want"]) and got
    for key, want in case["want"].items():
        for k, v in want.items():
            assert got[key][k] == v, (case["id"], key, k, got[key][k], v)
    print(E.plan_line(case))


def _count(pred):
    return sum(1 for c in E.CASES if pred(c, E.plans(c)))


def test_the_table_covers_the_branches_the_issue_names():
    """Every branch with no per-op case before this table: counted over both dtypes."""
    w = lambda p: p.get("wgrad", {})  # noqa: E731
    tiled, strip = (lambda c, p: w(p).get("variant") == v for v in (E.GENERIC, E.FIXED))
    assert _count(lambda c, p: tiled(c, p) and w(p)["trips"] > 1) >= 2, "tiled weight gradient, several tiles per block"
    assert _count(lambda c, p: w(p).get("reduce_unrolled", 0) > 0 and w(p)["reduce_tail"] > 0) >= 2, "unrolled reduce with a remainder"
    assert _count(lambda c, p: strip(c, p) and w(p)["tiles_y"] > 1) >= 2, "second strip row"
    assert _count(lambda c, p: strip(c, p) and w(p).get("last_chunk") == 1) >= 2, "a chunk of one row"
    assert _count(lambda c, p: strip(c, p) and w(p)["tiles_x"] == 2 and c["W"] == E.pixb(c["dt"]) + 1) >= 2, "one-column strip"
    assert _count(lambda c, p: p.get("outbd", {}).get("variant") == E.GENERIC and p["outbd"]["trips"] == 2) == 2
    assert _count(lambda c, p: p.get("inbd", {}).get("variant") == E.GENERIC and p["inbd"]["trips"] == 2) == 2
    for key, narrow in (("in", {1, 3, 4}), ("out", {1, 3, 4}), ("outbd", {1, 3, 4}), ("inbd", {1, 3, 4}), ("wgrad", {1, 3, 4})):
        have = {c["cio"] for c in E.CASES if key in c["want"] and E.plans(c)[key]["variant"] == E.GENERIC}
        assert narrow <= have, (key, have)
    assert {c["C0"] for c in E.CASES if c["op"] == "in"} == {8, 16, 32, 64, 256}
    shapes = {(c["H"], c["W"]) for c in E.CASES if c["op"] == "in" and c["C0"] == 32 and c["cio"] == 2}
    assert shapes == {(1, 1), (1, 40), (40, 1), (5, 24), (33, 32), (40, 256)}
    for dt in E.DTS:  # both formats of the statistics at every H x W of the MFMA variant
        assert {(c["H"], c["W"], c["groups"]) for c in E.CASES if c["op"] == "in" and c["C0"] == 32 and c["cio"] == 2 and c["dt"] == dt} == \
            {(h, w, g) for h, w in shapes for g in (0, 1)}
    # a negative control and a batch-independence case per op and variant
    for key, op in (("in", "in"), ("out", "out"), ("outbd", "outb"), ("inbd", "inbd")):
        for flag in ("control", "batch"):
            have = {E.plans(c)[key]["variant"] for c in E.CASES if c["op"] == op and c[flag]}
            assert have == {E.GENERIC, E.FIXED}, (key, flag, have)
    for op in ("inb", "outb"):
        assert {E.plans(c)["wgrad"]["variant"] for c in E.CASES if c["op"] == op and c["control"]} == {E.GENERIC, E.FIXED}


def test_the_tiled_data_gradient_runs_the_fast_out_conv_cases():
    """conv_in's tiled data gradient is the fast out-conv's tile walk: the same shapes, tile counts and flags, in both dtypes."""
    def fixed(op):
        return {(c["dt"], c["B"], c["H"], c["W"], c["control"], c["batch"], p["tiles_x"], p["tiles_y"], p["grid_x"])
                for c in E.CASES if c["op"] == op for p in [E.plans(c)[op]] if p["variant"] == E.FIXED}

    assert fixed("inbd") == fixed("out") and len(fixed("out")) == 10
    assert {(h, w) for _, _, h, w, *_ in fixed("inbd")} == {(1, 1), (1, 33), (9, 1), (8, 32), (9, 33)}


def test_second_trip_shapes_are_the_smallest():
    for dt in E.DTS:
        h = E.SECOND_TRIP_H[dt]
        assert X.edge_plan(X.EDGE_OUT_BWD_DATA, dt, 1, 40, 3, h, 256)["trips"] == 2
        assert X.edge_plan(X.EDGE_OUT_BWD_DATA, dt, 1, 40, 3, h - 1, 256)["trips"] == 1
        assert X.edge_plan(X.EDGE_IN_BWD_DATA, dt, 1, 8, 3, 4096, 256)["trips"] == 1
        assert X.edge_plan(X.EDGE_WGRAD, dt, 2, E.WIDEST_TILED_C, 2, 17, 17)["variant"] == E.GENERIC
        with pytest.raises(RuntimeError, match="LDS"):
            X.edge_plan(X.EDGE_WGRAD, dt, 2, E.WIDEST_TILED_C + 1, 2, 17, 17)


# ---- operand ranges ---------------------------------------------------------------------------------------------------------------
def _f32(op_):
    return {k: v.float() for k, v in op_.items()}


def _small(case):
    """The case with B = 1 and at most 40 rows: the ranges depend on the full shape, the bit comparison needs only a piece."""
    c = dict(case)
    c["B"], c["H"] = 1, min(case["H"], 40)
    return c


@pytest.mark.parametrize("case", E.CASES, ids=_id)
def test_operands_make_the_order_irrelevant(case):
    """The worst-case partial sum fits 24 bits of the product grid, every operand is a number of its storage type, and the float32
    host evaluation of the reference equals the fp64 one bit for bit."""
    op, C0, cio = case["op"], case["C0"], case["cio"]
    n = case["B"] * case["H"] * case["W"]
    full = E.operands(case)
    amax = {k: float(v.abs().max()) for k, v in full.items()}
    if op == "in":
        (kx, px), (kw, pw), (kb, pb) = E.conv_in_ranges(case)
        assert pb <= px + pw and X.budget_bits(9 * cio, kx * 2.0 ** -px, px, kw * 2.0 ** -pw, pw, kb * 2.0 ** -pb) < 24
    elif op == "out":
        assert X.budget_bits(9 * C0, amax["a"] + amax["b"], 3, amax["w"], 6, amax["bias"]) + 1 < 24  # the bias lies one bit finer
        for k in ("a", "b"):
            assert torch.equal(X.rne(full[k]), full[k])
        assert torch.equal(X.rne(full["a"] + full["b"]), full["a"] + full["b"])  # the fast kernel stages a + b in the dtype
    elif op == "inbd":
        assert X.budget_bits(9 * C0, amax["dy"], 4, amax["w"], 5) < 24 and torch.equal(X.rne(full["dy"]), full["dy"])
    elif op == "inb":
        assert X.budget_bits(n, amax["dy"], 3, amax["x"], 3) < 24 and torch.equal(X.rne(full["dy"]), full["dy"])
    else:
        assert X.budget_bits(n, amax["a"] + amax["b"], 3, amax["de"], 3) < 24
        assert X.budget_bits(9 * cio, amax["de"], 3, amax["w"], 6) < 24
        assert torch.equal(X.rne(full["a"]), full["a"]) and torch.equal(X.rne(full["b"]), full["b"])
    for v in full.values():
        assert torch.equal(v.float().double(), v)
    small = _small(case)
    op_ = E.operands(small)
    ref, f32 = E.reference(small, op_), E.reference(small, _f32(op_))
    for k in ref:
        assert f32[k].dtype == torch.float32 and torch.equal(f32[k].double(), ref[k]), (case["id"], k)


@pytest.mark.parametrize("case", [c for c in E.CASES if c["op"] == "in"], ids=_id)
def test_conv_in_statistics_are_exact_in_any_order(case):
    """Sums of |y| and y^2 of the stored values over a sample's group stay below 2^24 units of their grids (so does every partial of
    them), as in test_gpu_gn_kernels.py::test_conv_in_group_statistics."""
    (_, px), (_, pw), _ = E.conv_in_ranges(case)
    py = px + pw
    y = E.reference(case)["y"]
    y = X.rne(y) if case["dt"] == X.BF16 else y
    y = y.reshape(case["B"], -1, case["C0"])
    assert torch.equal(y * 2.0 ** py, torch.round(y * 2.0 ** py))
    tot = R.fold_groups(torch.stack([y.abs().sum(1), (y * y).sum(1)], -1))
    assert float(tot[..., 0].max()) * 2.0 ** py < 2 ** 24 and float(tot[..., 1].max()) * 4.0 ** py < 2 ** 24
    assert float(y.std()) > 0.25, "a degenerate output would check nothing"


def test_weight_gradient_ranges_shrink_with_the_image():
    r = {c["B"] * c["H"] * c["W"]: E.wgrad_ranges(c) for c in E.CASES if c["op"] in ("inb", "outb")}
    sizes = sorted(r)
    assert r[sizes[0]] == (8, 8) and E.wgrad_ranges(dict(id="x", B=8, H=1024, W=256)) == (2, 2)
    assert all(r[a][0] * r[a][1] >= r[b][0] * r[b][1] for a, b in zip(sizes, sizes[1:]))
    assert all(n * kg * ks < 2 ** 24 for n, (kg, ks) in r.items())


# ---- the references against torch ---------------------------------------------------------------------------------------------------
def test_references_agree_with_conv2d_and_its_autograd():
    """conv3 / wgrad3 / conv_transpose2d / conv_out_dgrad and the two packings against fp64 conv2d and autograd, Cin = 3, Cout = 5."""
    x = X.dyadic("ref.x", (2, 3, 7, 9), 8, 3).requires_grad_(True)
    w = X.dyadic("ref.w", (5, 3, 3, 3), 8, 6).requires_grad_(True)
    bias = X.dyadic("ref.b", (5,), 512, 10).requires_grad_(True)
    g = X.dyadic("ref.g", (2, 5, 7, 9), 8, 3)
    y = F.conv2d(x, w, bias, padding=1)
    y.backward(g)
    xn, gn = E.nhwc(x.detach()), E.nhwc(g)
    wd = w.detach()
    assert torch.equal(X.conv3(xn, wd, bias.detach()), E.nhwc(y.detach()))
    assert torch.equal(X.wgrad3(xn, gn), w.grad) and torch.equal(gn.sum((0, 1, 2)), bias.grad)
    assert torch.equal(F.conv_transpose2d(g, wd, padding=1), x.grad)
    assert torch.equal(E.conv_out_dgrad(gn, wd), E.nhwc(x.grad))
    # the packed layouts as the kernels index them: conv_out reads w[(k * cout + o) * C0 + c], conv_in's data gradient is the
    # forward conv of dy with w[(k * NI + i) * C0 + c]
    p9 = E.pack9(wd)
    assert all(torch.equal(p9[k], wd[:, :, k // 3, k % 3]) for k in range(9))
    pd = E.pack9_dgrad(wd)  # [9][3][5]
    gp = F.pad(gn, (0, 0, 1, 1, 1, 1))
    dx = sum(gp[:, k // 3:k // 3 + 7, k % 3:k % 3 + 9, :] @ pd[k].T for k in range(9))
    assert torch.equal(dx, E.nhwc(x.grad))


@pytest.mark.parametrize("op", ["in", "out", "outb", "inbd", "inb"])
def test_one_zeroed_tap_violates_the_criterion(op):
    """What the negative controls of the GPU module do to the kernel's input, done to the reference: it is seen in both dtypes."""
    case = _small(next(c for c in E.CASES if c["op"] == op and c["control"] and c["dt"] == X.BF16))
    good = E.operands(case)
    ref = E.reference(case, good)
    for tap in (0, 4, 8):
        bad = {k: v.clone() for k, v in good.items()}
        if op == "inb":
            bad["x"][:, -1] = 0  # one plane of S
        else:
            bad["w"][:, :, tap // 3, tap % 3] = 0
        got = E.reference(case, bad)
        key = {"in": "y", "out": "eps", "outb": "d_sum", "inbd": "d_x", "inb": "d_w"}[op]
        assert bool(X.mismatches(got[key], ref[key], X.F32).any()), (op, tap)
        if op in ("in", "outb"):
            assert bool(X.mismatches(X.rne(got[key]), ref[key], X.BF16).any()), (op, tap)
    if op == "outb":
        bad = {k: v.clone() for k, v in good.items()}
        bad["de"][:, -1] = 0
        assert bool(X.mismatches(E.reference(case, bad)["d_w"], ref["d_w"], X.F32).any())


# ---- what the plan refuses -----------------------------------------------------------------------------------------------------------
OPS = (X.EDGE_IN, X.EDGE_OUT, X.EDGE_OUT_BWD_DATA, X.EDGE_IN_BWD_DATA, X.EDGE_WGRAD)
BIG = 2 ** 31 - 1


@pytest.mark.parametrize("op", OPS)
def test_the_plan_refuses_bad_arguments(op):
    def refused(match, dt=X.F32, B=2, C0=32, cio=2, H=8, W=8, groups=0):
        with pytest.raises(RuntimeError, match=match):
            X.edge_plan(op, dt, B, C0, cio, H, W, groups)

    X.edge_plan(op, X.F32, 2, 32, 2, 8, 8)
    for dt in (-1, 2, 7):
        refused("dtype", dt=dt)
    for k in ("B", "C0", "cio", "H", "W"):
        refused("at least 1", **{k: 0})
        refused("at least 1", **{k: -3})
    refused("overflow", H=BIG)
    refused("overflow", W=BIG - 100, H=1)
    refused("64-bit", B=65535, H=2 ** 20, W=2 ** 20, C0=64)
    if op in (X.EDGE_IN, X.EDGE_OUT_BWD_DATA):
        refused("grid", B=65536)
    else:
        X.edge_plan(op, X.F32, 65536, 32, 2, 8, 8)  # the sample is folded into grid x
    if op in (X.EDGE_OUT_BWD_DATA, X.EDGE_IN_BWD_DATA):
        refused("grid", B=65536, C0=16)  # their generic kernels have B in grid y
    if op != X.EDGE_IN and op != X.EDGE_OUT_BWD_DATA:
        refused("at most 4", cio=5)


def test_the_plan_refuses_widths_and_index_overflow():
    def refused(op, match, dt=X.F32, B=1, C0=32, cio=2, H=8, W=8, groups=0):
        with pytest.raises(RuntimeError, match=match):
            X.edge_plan(op, dt, B, C0, cio, H, W, groups)

    refused(X.EDGE_IN, "power of two", C0=40)
    refused(X.EDGE_IN, "power of two", C0=12)
    refused(X.EDGE_IN, "power of two", C0=512)
    refused(X.EDGE_IN, "power of two", C0=36, dt=X.BF16)
    refused(X.EDGE_IN, "group", C0=4, groups=1)
    refused(X.EDGE_IN, "LDS", C0=256, cio=7)
    refused(X.EDGE_OUT, "multiple of 8", C0=12)
    refused(X.EDGE_OUT, "LDS", C0=48)
    refused(X.EDGE_OUT_BWD_DATA, "multiple of 4", C0=6)
    refused(X.EDGE_OUT_BWD_DATA, "multiple of 8", C0=12, dt=X.BF16)
    refused(X.EDGE_OUT_BWD_DATA, "LDS", C0=64, cio=32)
    refused(X.EDGE_IN_BWD_DATA, "multiple of 4", C0=6)
    refused(X.EDGE_IN_BWD_DATA, "multiple of 8", C0=12, dt=X.BF16)
    refused(X.EDGE_WGRAD, "items", C0=68)
    refused(X.EDGE_WGRAD, "LDS", C0=64)
    # index types: conv_in's int pixel offsets (MFMA: 2 H W - 1, generic: H W + 1023), the int tile / strip counters
    X.edge_plan(X.EDGE_IN, X.F32, 1, 32, 2, 2 ** 15, 2 ** 15)
    refused(X.EDGE_IN, "pixel", H=2 ** 15, W=2 ** 15 + 1)
    X.edge_plan(X.EDGE_IN, X.F32, 1, 16, 2, 2 ** 15, 2 ** 16 - 1)
    refused(X.EDGE_IN, "pixel", C0=16, H=2 ** 16, W=2 ** 15)
    for op in (X.EDGE_OUT, X.EDGE_IN_BWD_DATA):
        X.edge_plan(op, X.F32, 15, 32, 2, 2 ** 16, 2 ** 19)
        refused(op, "tile", B=16, H=2 ** 16, W=2 ** 19)
    refused(X.EDGE_WGRAD, "strip", B=1024, H=2 ** 17, W=2 ** 16)
    refused(X.EDGE_WGRAD, "tile", C0=16, B=16, H=2 ** 18, W=2 ** 17)
    assert math.log2(X.edge_plan(X.EDGE_WGRAD, X.F32, 15, 16, 2, 2 ** 18, 2 ** 17)["trips"]) > 20
