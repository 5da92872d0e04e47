"""Host checks of the exact-operand tests (tests/test_gpu_exact.py, tests/test_gpu_train_exact.py): each case reaches the kernel family / variant / tiling it
declares (the library's own conv_plan / wgrad_plan, host only), its operand ranges make fp32 summation order irrelevant, one
missing (tap, input channel) term violates its criterion, and the cases cover every kernel key the network walks launch -- the
convs' (test_exact_cases_cover_the_walks_kernel_keys) and the weight gradients' (test_exact_cases_cover_the_walks_wgrad_keys), whose
sparse cases have their own negative controls: one dropped, doubled, wrongly transformed or wrongly cut tile."""
import pytest
import torch

import exact_util as X
from exact_cases import CONV_CASES, DOWNUP_CASES, WGRAD_CASES, DUBWD_CASES, DOWN_PAIRS, UP_PAIRS, conv_operands, wgrad_operands
from exact_cases import TRAIN_FWD_CASES, BATCH_PLAIN_CASES, DGRAD_CASES, BWD_INSTANTIATIONS, dgrad_operands, dgrad_exact
from exact_cases import WGRAD_KEY_CASES, DUBWD_KEY_CASES, WGRAD_KEY_ROWS, WGRAD_WIDTHS, WG_FLAGS, case_wgrad_key, wg_flags
from exact_cases import smallest_wgrad_shapes, wgrad_delta, dubwd_ranges, dubwd_operands, wgrad_hot_tiles, wgrad_tile_mask
from ddim_audio_amd import configs


def _id(c):
    return c["id"]


@pytest.mark.parametrize("case", CONV_CASES + TRAIN_FWD_CASES + BATCH_PLAIN_CASES + DGRAD_CASES, ids=_id)
def test_conv_case_reaches_its_kernel(case):
    p = X.conv_plan(case["dt"], X.CONV3, case["C"], case["C"], case["B"], case["H"], case["W"], case["flags"])
    assert p["family"] == case["family"], (X.FAMILY[p["family"]], case["id"])
    for k, v in case["want"].items():
        assert p[k] == v, (k, p[k], v, case["id"])


@pytest.mark.parametrize("case", DOWNUP_CASES, ids=_id)
def test_downup_case_reaches_its_kernel(case):
    p = X.conv_plan(case["dt"], case["mode"], case["cin"], case["cout"], case["B"], case["H"], case["W"], case["flags"])
    assert p["family"] == case["family"], (X.FAMILY[p["family"]], case["id"])


def test_wgrad_cases_reach_both_sides_of_64_splits_and_the_reduce_kernels():
    for c in WGRAD_CASES:
        p = X.wgrad_plan(c["dt"], X.CONV3, c["C"], c["C"], c["B"], c["H"], c["W"])
        assert (p["nsplit"] >= 64) == c["want"]["many"], (c["id"], p)
    for c in DUBWD_CASES:
        if c["mode"] == X.DOWN4:
            p = X.wgrad_plan(c["dt"], X.DOWN4, c["cin"], c["cout"], c["B"], c["H"] // 2, c["W"] // 2)
        else:
            p = X.wgrad_plan(c["dt"], X.DOWN4, c["cout"], c["cin"], c["B"], c["H"], c["W"])
        assert p["reduce"] == c["reduce"], (c["id"], p)
    # the 16-threads-per-output reduce serves nsplit >= 64 with ntaps * co * ci not a multiple of 4: no instantiated weight
    # gradient has such a shape (every width is a multiple of 32), so no test can reach it -- asserted, so that a new width shows up
    for dt in (X.F32, X.BF16):
        for C in configs.audio_config().model.ch:
            assert X.wgrad_plan(dt, X.CONV3, C, C, 8, 512, 256)["reduce"] != "ks16"


@pytest.mark.parametrize("case", [c for c in CONV_CASES + TRAIN_FWD_CASES + BATCH_PLAIN_CASES if c["xf"] in (X.XF_NONE, X.XF_AFFINE)], ids=_id)
def test_conv_operands_make_the_order_irrelevant(case):
    """The float32 host evaluation equals the fp64 reference bit for bit, and the worst-case partial sum fits 24 bits."""
    B = min(case["B"], 1)
    H = min(case["H"], 24)
    op = conv_operands(case)
    a, w = op["a_ref"][:B, :H], op["w"]
    bias = op["bias"]
    add = op["add"][:B] if op["add"] is not None else None
    assert X.budget_bits(9 * case["C"], float(a.abs().max()), 4, float(w.abs().max()), 6, 1.0) < 24
    ref = X.conv3(a, w, bias, add)
    f32 = X.conv3(a.float(), w.float(), bias.float() if bias is not None else None, add.float() if add is not None else None)
    assert torch.equal(f32.double(), ref)
    # the operands are bf16 numbers, and so is the transformed input
    for t in (op["x"], w, a):
        assert torch.equal(X.rne(t), t)


@pytest.mark.parametrize("C", [32, 64, 96, 128, 192, 256])
def test_one_missing_term_violates_the_criterion(C):
    """Removing one (tap, input channel) term from the reference changes RNE(exact) somewhere, at every width."""
    case = next(c for c in CONV_CASES if c["C"] == C and c["xf"] != X.XF_AFFINE_SILU)
    op = conv_operands(case)
    a, w = op["a_ref"][:1, :16], op["w"]
    ref = X.conv3(a, w, op["bias"], op["add"][:1] if op["add"] is not None else None)
    for tap, ci in ((0, 0), (4, C - 1), (8, C // 2)):
        w2 = w.clone()
        w2[:, ci, tap // 3, tap % 3] = 0
        bad = X.conv3(a, w2, op["bias"], op["add"][:1] if op["add"] is not None else None)
        assert bool(X.mismatches(X.rne(bad), ref, X.BF16).any()), (C, tap, ci)
        assert bool(X.mismatches(bad, ref, X.F32).any()), (C, tap, ci)


@pytest.mark.parametrize("case", [c for c in WGRAD_CASES if c["xf"] in (X.XF_NONE, X.XF_AFFINE)], ids=_id)
def test_wgrad_operands_make_the_order_irrelevant(case):
    op = wgrad_operands(case)
    a, du = op["a_ref"], op["du"]
    assert X.budget_bits(case["B"] * case["H"] * case["W"], float(a.abs().max()), 4, float(du.abs().max()), 6) < 24
    assert torch.equal(X.wgrad3(a.float(), du.float()).double(), X.wgrad3(a, du))


# ---- the weight-gradient keys ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WGRAD_KEY_CASES + DUBWD_KEY_CASES, ids=_id)
def test_wgrad_key_case_reaches_its_key(case):
    kernel, reduce = case_wgrad_key(case)
    if case["flags"] is not None:
        assert wg_flags(kernel) == case["flags"], (case["id"], kernel)
    if case["reduce"] is not None:
        assert reduce == case["reduce"], (case["id"], reduce)
        assert kernel[4] in (X.XF_NONE, X.XF_AFFINE)  # a reduce key counts only under the exact criterion


@pytest.mark.parametrize("dt,mode,ci,co,xf", [(X.BF16, X.CONV3, 256, 256, X.XF_SILU_AFFINE), (X.F32, X.DOWN4, 64, 96, X.XF_NONE)])
def test_wgrad_key_rows_are_the_smallest_shapes(dt, mode, ci, co, xf):
    """The frozen rows of two widths against the search that found them (the full search takes a quarter of a minute)."""
    rows = {f: (B, H, W) for m, i, o, B, H, W, f, xfs in WGRAD_KEY_ROWS if (m, i, o) == (mode, ci, co) and xf in xfs}
    keys = {(mode, ci, co, dt, xf) + tuple(c in f for c in WG_FLAGS): f for f in rows}
    found = smallest_wgrad_shapes(dt, mode, ci, co, xf, keys)
    assert {keys[k]: s for k, s in found.items()} == rows


@pytest.mark.parametrize("case", [c for c in WGRAD_KEY_CASES if not c["sparse"]], ids=_id)
def test_wgrad_reduce_case_operands_make_the_order_irrelevant(case):
    op = wgrad_operands(case)
    a, du = op["a_ref"], op["du"]
    assert wgrad_delta(case, a, du) is None
    assert X.budget_bits(case["B"] * case["H"] * case["W"], float(a.abs().max()), 4, float(du.abs().max()), 6) < 24
    assert torch.equal(X.wgrad3(a.float(), du.float()).double(), X.wgrad3(a, du))


@pytest.mark.parametrize("case", DUBWD_CASES + DUBWD_KEY_CASES, ids=_id)
def test_dubwd_operands_make_the_order_irrelevant(case):
    """XF_NONE: the stride-2 weight gradient sums B Hd Wd products of x (k/8) and dy (k/64), below 2^24 grid units at the case's own
    pixel count, so d_w must equal the fp64 value bit for bit."""
    (kx, px), (kd, pd) = dubwd_ranges(case)
    n = case["B"] * case["H"] * case["W"] // (4 if case["mode"] == X.DOWN4 else 1)  # pixels of the small side: the terms of a sum
    assert X.budget_bits(n, kx * 2.0 ** -px, px, kd * 2.0 ** -pd, pd) < 24
    if n <= 4096:
        op = dubwd_operands(case)
        big, small = (op["x"], op["dy"]) if case["mode"] == X.DOWN4 else (op["dy"], op["x"])
        assert float(op["x"].abs().max()) <= kx * 2.0 ** -px and float(op["dy"].abs().max()) <= kd * 2.0 ** -pd
        assert torch.equal(X.wgrad_down4(big.float(), small.float()).double(), X.wgrad_down4(big, small))


@pytest.mark.parametrize("case", [c for c in WGRAD_KEY_CASES if c["sparse"]], ids=_id)
def test_sparse_wgrad_case_keeps_du_on_the_tiles_that_matter(case):
    p = X.wgrad_plan(case["dt"], X.CONV3, case["C"], case["C"], case["B"], case["H"], case["W"])
    ts, ranges = p["tiles_x"] * p["tiles_y"], X.wgrad_ranges(p, case["B"])
    hot = wgrad_hot_tiles(case)
    assert len(hot) <= 16
    want = {ranges[0][0], ranges[0][1] - 1, ranges[-1][0], ranges[-1][1] - 1}
    for t0, t1 in ranges:
        if t0 // ts != (t1 - 1) // ts:
            want |= {t0, t1 - 1} | {e + d for e in range((t0 // ts + 1) * ts, t1, ts) for d in (-1, 0)}
    if "h" in case["flags"]:
        assert any(t % ts // p["tiles_x"] == p["tiles_y"] - 1 for t in hot)
    if "w" in case["flags"]:
        assert any(t % p["tiles_x"] == p["tiles_x"] - 1 for t in hot)
    assert want <= set(hot)
    if case["dt"] == X.F32 and case["xf"] == X.XF_AFFINE_SILU:  # (the operands of the other three cases of a shape differ by their tag only)
        op = wgrad_operands(case)
        live = (op["du"] != 0).any(-1)
        mask = wgrad_tile_mask(case, hot)
        assert not bool((live & ~mask).any()) and int(live.sum()) > 0.9 * int(mask.sum())
        assert bool((op["a"] != 0).any(-1).float().mean() > 0.99)  # `a` stays dense
        # a dropped or a doubled tile moves d_w by whole terms: either violates the criterion, at every tile that carries du
        a, du = op["a_ref"], op["du"]
        exact, delta = X.wgrad3(a, du), wgrad_delta(case, a, du)
        assert not bool(X.mismatches(exact.float(), exact, X.F32, delta=delta).any())
        for t in hot:
            b, y0, x0 = _sample_tile(p, t)
            term = _tile_terms(a[b], du[b], y0, x0, p["th"], p["tw"], False)
            for sign in (-1, 1):
                assert bool(X.mismatches((exact + sign * term).float(), exact, X.F32, delta=delta).any()), (case["id"], t, sign)


def _tile_terms(a_s, du_s, y0, x0, th, tw, wrap):
    """What wgrad_mfma_kernel adds to dW [Co][Ci][3][3] for the tile at (y0, x0) of one sample: a_s [H][W][Ci] after the transform,
    du_s [H][W][Co].  wrap: without the kernel's x < W test, so that a pixel right of the image is the one that follows in memory
    (the next image row), cut by the sample's buffer bound alone."""
    H, W = du_s.shape[:2]

    def fetch(t, yy, xx):
        ok = (yy >= 0) & (xx >= 0) & (yy < H) & ((yy * W + xx < H * W) if wrap else (xx < W))
        v = t.reshape(H * W, -1)[(yy * W + xx).clamp(0, H * W - 1)]
        return v * ok[..., None]

    ys, xs = torch.meshgrid(torch.arange(th) + y0, torch.arange(tw) + x0, indexing="ij")
    d = fetch(du_s, ys, xs).reshape(th * tw, -1)
    dw = torch.zeros(du_s.shape[-1], a_s.shape[-1], 3, 3, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            dw[:, :, kh, kw] = d.T @ fetch(a_s, ys + kh - 1, xs + kw - 1).reshape(th * tw, -1)
    return dw


def _sample_tile(p, t):
    ts = p["tiles_x"] * p["tiles_y"]
    return t // ts, (t % ts // p["tiles_x"]) * p["th"], (t % p["tiles_x"]) * p["tw"]


@pytest.mark.parametrize("dt", [X.F32, X.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("xf", [X.XF_AFFINE_SILU, X.XF_SILU_AFFINE], ids=["conv0", "conv1"])
@pytest.mark.parametrize("C,flags", [(256, "wmcs"), (32, "mcs")], ids=["ragged", "largest"])
def test_one_wrong_tile_violates_the_wgrad_criterion(C, flags, dt, xf):
    """Negative controls of the sparse cases, on the reference alone: the criterion (delta from the non-zero pixels of du) passes
    the fp64 reference rounded to fp32 and fails, in at least one element, each fault a tile walk can have -- (a) the last tile of
    the short workgroup left out, (b) the first tile of a workgroup counted twice, (c) the tiles behind a sample crossing
    transformed with the previous sample's scale / shift, (d) a ragged tile that reads the next image row where it must read zeros.
    Once at the case that has every feature, once at the one with the most non-zero pixels (the widest bound; no ragged tile)."""
    case = next(c for c in WGRAD_KEY_CASES if (c["dt"], c["xf"], c["C"], c["flags"]) == (dt, xf, C, flags))
    B, H, W = case["B"], case["H"], case["W"]
    p = X.wgrad_plan(dt, X.CONV3, C, C, B, H, W)
    ts, ranges = p["tiles_x"] * p["tiles_y"], X.wgrad_ranges(p, B)
    op = wgrad_operands(case)
    a, du = op["a_ref"], op["du"]
    exact = X.wgrad3(a, du)
    delta = wgrad_delta(case, a, du)

    def violates(v):
        return bool(X.mismatches(v.float(), exact, X.F32, delta=delta).any())

    def tile(t, a_=a):
        b, y0, x0 = _sample_tile(p, t)
        return _tile_terms(a_[b], du[b], y0, x0, p["th"], p["tw"], False)

    assert not violates(exact)
    assert float((sum(tile(t) for t in range(B * ts)) - exact).abs().max()) < 1e-12  # the controls' tile walk is the reference
    t0, t1 = ranges[-1]
    assert t1 - t0 < p["per"]
    assert violates(exact - tile(t1 - 1)), "(a)"
    assert violates(exact + tile(ranges[0][0])), "(b)"
    t0, t1 = next(r for r in ranges if r[0] // ts != (r[1] - 1) // ts)
    stale = X.xf64(op["a"], op["scale"].roll(1, 0), op["shift"].roll(1, 0), xf)  # sample b under the scale / shift of sample b - 1
    stale = X.rne(stale) if dt == X.BF16 else stale
    behind = range((t0 // ts + 1) * ts, t1)
    assert violates(exact + sum(tile(t, stale) - tile(t) for t in behind)), "(c)"
    if "w" not in flags:
        return
    t = next(t for t in wgrad_hot_tiles(case) if t % p["tiles_x"] == p["tiles_x"] - 1)
    b, y0, x0 = _sample_tile(p, t)
    assert violates(exact + _tile_terms(a[b], du[b], y0, x0, p["th"], p["tw"], True) - tile(t)), "(d)"


def test_downup_operands_make_the_order_irrelevant():
    for cin, cout, h, w in DOWN_PAIRS:
        assert X.budget_bits(16 * cin, 1.0, 3, 0.125, 6, 0.5) < 24
    for cin, cout, h, w in UP_PAIRS:
        assert X.budget_bits(4 * cin, 1.0, 3, 0.125, 6, 1.5) < 24
    x = X.dyadic("self.x", (1, 8, 16, 64), 8, 3)
    wd = X.dyadic("self.w", (96, 64, 4, 4), 8, 6)
    assert torch.equal(X.down4(x.float(), wd.float()).double(), X.down4(x, wd))
    wu = X.dyadic("self.wu", (64, 32, 4, 4), 8, 6)
    assert torch.equal(X.up4(x.float(), wu.float()).double(), X.up4(x, wu))


def test_rounding_helpers():
    v = torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, 1 + 2 ** -9, 3.14159, -2.718281828, 1e-3], dtype=torch.float64)
    assert torch.equal(X.rne(v), v.float().bfloat16().double())
    assert torch.equal(X.rne(v, 24), v.float().double())
    assert torch.equal(X.ulp(torch.tensor([1.0, 1.5, 2.0, 0.75], dtype=torch.float64)),
                       torch.tensor([2 ** -7, 2 ** -7, 2 ** -6, 2 ** -8], dtype=torch.float64))
    assert bool(X.near_midpoint(torch.tensor([1 + 2 ** -8], dtype=torch.float64)).all())
    assert not bool(X.near_midpoint(torch.tensor([1 + 2 ** -7], dtype=torch.float64)).any())


def _dgrad_rows():
    """One case per row of DGRAD_CASES (the two bwd_modes of a row share their operands)."""
    return [c for c in DGRAD_CASES if c["bwd_mode"] == 1]


def _fused_nparts(c):
    """The slab count ddimx_conv3x3_dgrad_stats reports, by the rule of dgrad_fused_stats: the conv's workgroups per sample (x its
    classes: one for a 3x3 conv) where resid's partition has room for them, else 0."""
    p = X.conv_plan(c["dt"], X.CONV3, c["C"], c["C"], c["B"], c["H"], c["W"], c["flags"])
    return p["wgs_per_sample"] if p["wgs_per_sample"] <= X.gn_plan(c["dt"], c["C"], c["B"], c["H"], c["W"], 1)["y_np"] else 0


@pytest.mark.parametrize("case", DGRAD_CASES, ids=_id)
def test_dgrad_case_takes_the_statistics_in_its_epilogue(case):
    assert _fused_nparts(case) > 0, case["id"]


def test_dgrad_cases_reach_every_bwd_instantiation_ragged_and_whole():
    """The 15 ConvCfg::BWD kernels (conv_inst_bf16_c3b.hip: 9, conv_inst_f32_c3b.hip: 6), each with a ragged and a whole-tile launch
    and in both bwd_modes; a variant-1 plan of a width without a small-tile kernel would be a new instantiation."""
    have = set()
    for c in DGRAD_CASES:
        p = X.conv_plan(c["dt"], X.CONV3, c["C"], c["C"], c["B"], c["H"], c["W"], c["flags"])
        have.add((c["dt"], c["C"], p["var"], p["ragged"], c["bwd_mode"]))
    assert len(BWD_INSTANTIATIONS) == 15
    assert {k[:3] for k in have} == set(BWD_INSTANTIATIONS)
    assert have == {i + (r, m) for i in BWD_INSTANTIATIONS for r in (False, True) for m in (1, 2)}


@pytest.mark.parametrize("case", _dgrad_rows(), ids=_id)
def test_dgrad_operands_make_the_order_irrelevant(case):
    """The float32 host evaluation of dg equals the fp64 reference bit for bit, and the worst-case partial sum fits 18 bits."""
    op = dgrad_operands(case)
    du, w = op["du"][:1, :24], op["w"]
    assert X.budget_bits(9 * case["C"], float(du.abs().max()), 6, float(w.abs().max()), 6) < 18
    assert X.budget_bits(9 * 256, 0.125, 6, 0.125, 6) < 18
    assert torch.equal(dgrad_exact(du.float(), w.float()).double(), dgrad_exact(du, w))
    for t, bits in ((du, 8), (w, 8), (op["aux"], 8), (op["scale"], 8), (op["shift"], 8)):
        assert torch.equal(X.rne(t, bits), t)


@pytest.mark.parametrize("C", [32, 64, 96, 128, 192, 256])
def test_one_missing_term_violates_the_dgrad_criterion(C):
    """Removing one (tap, input channel) term from the data-gradient reference changes RNE(exact) somewhere, at every width (the
    conv's input channel is the weight's output channel)."""
    case = next(c for c in DGRAD_CASES if c["C"] == C and c["H"] >= 8)
    op = dgrad_operands(case)
    du, w = op["du"][:1, :16], op["w"]
    ref = dgrad_exact(du, w)
    for tap, co in ((0, 0), (4, C - 1), (8, C // 2)):
        w2 = w.clone()
        w2[co, :, tap // 3, tap % 3] = 0
        bad = dgrad_exact(du, w2)
        assert bool(X.mismatches(X.rne(bad), ref, X.BF16).any()), (C, tap, co)
        assert bool(X.mismatches(bad, ref, X.F32).any()), (C, tap, co)


# ---- coverage of the network walks ---------------------------------------------------------------------------------------------
# Keys no per-op entry point can reach, each with the composite test that runs it.
COMPOSITE_ONLY = {
    "gn.stats": "in-kernel GroupNorm prologue: test_gpu_exact.py::test_sample_result_is_batch_and_gn_path_invariant, "
                "test_gpu_model.py::test_model_forward_golden",
}
SWEEP_T = (32, 64, 96, 128, 256, 512, 1024, 2048, 4096, 8192)
SWEEP_B = (1, 2, 3, 4, 8, 16, 32, 64)


def _walk_keys(cfg, T, B, dt):
    """(family, mode, cin, cout, dt, var, ragged, multi, path) of every conv the inference and training walks launch.  path: which
    epilogue of the kernel runs -- "fwd" (the inference forms), "act2" (training forward: pre-activation stored, statistics of its
    SiLU), "bwd1" / "bwd2" (data gradient with the GroupNorm-backward statistics, ConvCfg::BWD)."""
    ch, f = cfg.model.ch, cfg.model.f_size
    keys = set()

    def add(mode, cin, cout, H, W, flags, *paths):
        p = X.conv_plan(dt, mode, cin, cout, B, H, W, flags)  # a shape the walk launches must plan: a failure is a finding
        for path in paths or ("fwd",):
            keys.add((p["family"], mode, cin, cout, dt, p["var"], p["ragged"], p["multi"], path))
        return p

    for l, C in enumerate(ch):
        H, W = T >> l, f >> l
        if H < 1 or W < 1:
            continue
        wf = X.P_WFRAG if dt == X.BF16 else 0
        # inference: GroupNorm input finished in-kernel (composite) or by a finalize launch -- the plan is the same either way
        add(X.CONV3, C, C, H, W, wf | X.P_XF(2) | X.P_ACT(1) | X.P_STATS | X.P_GROUPS)
        add(X.CONV3, C, C, H, W, wf | X.P_XF(1) | X.P_ACT(1) | X.P_STATS | X.P_GROUPS)
        # training forward (run_resblock with a tape, batch plan): conv.0 and conv.1 store their pre-activations
        add(X.CONV3, C, C, H, W, X.P_BATCH | X.P_XF(2) | X.P_ACT(2) | X.P_STATS, "act2")
        add(X.CONV3, C, C, H, W, X.P_BATCH | X.P_XF(3) | X.P_ACT(2) | X.P_STATS, "act2")
        # backward (run_resblock_bwd): the two data-gradient convs take the GroupNorm-backward statistics in their epilogue where
        # resid's partition has room for the conv's slabs (dgrad_fused_stats), and are plain convs otherwise
        p = X.conv_plan(dt, X.CONV3, C, C, B, H, W, X.P_BATCH | X.P_BWD | X.P_STATS)
        if p["wgs_per_sample"] <= X.gn_plan(dt, C, B, H, W, 1)["y_np"]:
            add(X.CONV3, C, C, H, W, X.P_BATCH | X.P_BWD | X.P_STATS, "bwd1", "bwd2")
        else:
            add(X.CONV3, C, C, H, W, X.P_BATCH)
        if l > 0:
            add(X.DOWN4, ch[l - 1], C, 2 * H, 2 * W, wf | X.P_STATS | X.P_GROUPS)
            add(X.UP4, C, ch[l - 1], H, W, wf | X.P_SKIP | X.P_STATS | X.P_GROUPS)
            add(X.DOWN4, ch[l - 1], C, 2 * H, 2 * W, X.P_BATCH)
            add(X.UP4, C, ch[l - 1], H, W, X.P_BATCH)
            add(X.UP4, C, ch[l - 1], H, W, X.P_BATCH | X.P_SKIP)
    return keys


def _case_keys():
    keys = set()
    for c in CONV_CASES + BATCH_PLAIN_CASES:
        p = X.conv_plan(c["dt"], X.CONV3, c["C"], c["C"], c["B"], c["H"], c["W"], c["flags"])
        keys.add((p["family"], X.CONV3, c["C"], c["C"], c["dt"], p["var"], p["ragged"], p["multi"], "fwd"))
    for c in TRAIN_FWD_CASES:
        p = X.conv_plan(c["dt"], X.CONV3, c["C"], c["C"], c["B"], c["H"], c["W"], c["flags"])
        keys.add((p["family"], X.CONV3, c["C"], c["C"], c["dt"], p["var"], p["ragged"], p["multi"], "act2"))
    for c in DGRAD_CASES:
        if _fused_nparts(c):
            p = X.conv_plan(c["dt"], X.CONV3, c["C"], c["C"], c["B"], c["H"], c["W"], c["flags"])
            keys.add((p["family"], X.CONV3, c["C"], c["C"], c["dt"], p["var"], p["ragged"], p["multi"], f"bwd{c['bwd_mode']}"))
    for c in DOWNUP_CASES:
        p = X.conv_plan(c["dt"], c["mode"], c["cin"], c["cout"], c["B"], c["H"], c["W"], c["flags"])
        keys.add((p["family"], c["mode"], c["cin"], c["cout"], c["dt"], p["var"], p["ragged"], p["multi"], "fwd"))
    for c in DUBWD_CASES:  # the data-gradient convs of ddimx_downsample_bwd / ddimx_upsample_add_bwd (batch plan)
        dt, B = c["dt"], c["B"]
        if c["mode"] == X.DOWN4:
            p = X.conv_plan(dt, X.UP4, c["cout"], c["cin"], B, c["H"] // 2, c["W"] // 2, X.P_BATCH | X.P_SKIP)
            keys.add((p["family"], X.UP4, c["cout"], c["cin"], dt, p["var"], p["ragged"], p["multi"], "fwd"))
        else:
            p = X.conv_plan(dt, X.DOWN4, c["cout"], c["cin"], B, 2 * c["H"], 2 * c["W"], X.P_BATCH)
            keys.add((p["family"], X.DOWN4, c["cout"], c["cin"], dt, p["var"], p["ragged"], p["multi"], "fwd"))
    return keys


def test_exact_cases_cover_the_walks_kernel_keys():
    """Every (family, mode, cin, cout, dtype, variant, ragged, multi-tile workgroup, path) key the inference and training walks launch
    at T in {32 .. 8192}, B in {1 .. 64} (audio and tiny configs) is reached by an exact case.  Each (C, variant) is a template
    instantiation of its own (the ConvCfg::BWD ones apart), ragged / multi-tile workgroups run other halo and epilogue code, and
    the path picks the epilogue's store and statistics branch."""
    have = _case_keys()
    missing = set()
    for cfg in (configs.audio_config(), configs.tiny_config()):
        for dt in (X.F32, X.BF16):
            for T in SWEEP_T:
                for B in SWEEP_B:
                    missing |= _walk_keys(cfg, T, B, dt) - have
    assert missing == set(), sorted((X.FAMILY[k[0]],) + k[1:] for k in missing)
    assert set(COMPOSITE_ONLY) == {"gn.stats"}


SWEEP_B_TRAIN = (1, 2, 3, 4, 8, 14, 16, 32)


def _walk_wgrad_keys(cfg, T, B, dt):
    """(kernel keys, reduce keys) of every weight gradient the training walk launches (X.wgrad_key): the two 3x3 convs of each
    level's blocks under their transforms (run_resblock_bwd: conv.0 XF_AFFINE_SILU, conv.1 XF_SILU_AFFINE), and the stride-2 launch
    that the Downsample and the Upsample of a level > 0 share (XF_NONE)."""
    ch, f = cfg.model.ch, cfg.model.f_size
    kernel, reduce = set(), set()
    for l, C in enumerate(ch):
        H, W = T >> l, f >> l
        if H < 1 or W < 1:
            continue
        calls = [(X.CONV3, C, C, X.XF_AFFINE_SILU), (X.CONV3, C, C, X.XF_SILU_AFFINE)]
        if l > 0:
            calls.append((X.DOWN4, ch[l - 1], C, X.XF_NONE))
        for mode, ci, co, xf in calls:
            k, r = X.wgrad_key(dt, mode, ci, co, B, H, W, xf)
            kernel.add(k)
            reduce.add(r)
    return kernel, reduce


def _case_wgrad_keys():
    """A reduce key counts where the case's criterion is E (XF_NONE / XF_AFFINE): there d_w is exact at any number of slabs."""
    kernel, reduce = set(), set()
    for c in WGRAD_CASES + WGRAD_KEY_CASES + DUBWD_CASES + DUBWD_KEY_CASES:
        k, r = case_wgrad_key(c)
        kernel.add(k)
        if k[4] in (X.XF_NONE, X.XF_AFFINE):
            reduce.add(r)
    return kernel, reduce


def test_exact_cases_cover_the_walks_wgrad_keys():
    """Every kernel key (mode, ci, co, dtype, transform, ragged_h, ragged_w, several tiles per workgroup, a range that runs into the
    next sample, short last workgroup) and every reduce key (kind, unrolled iterations, tail, threads that disagree) of the weight
    gradients the training walk launches at T in {32 .. 8192}, B in {1 .. 32} (audio and tiny configs) is reached by an exact case."""
    have_k, have_r = _case_wgrad_keys()
    walk_k, walk_r = set(), set()
    for cfg in (configs.audio_config(), configs.tiny_config()):
        for dt in (X.F32, X.BF16):
            for T in SWEEP_T:
                for B in SWEEP_B_TRAIN:
                    k, r = _walk_wgrad_keys(cfg, T, B, dt)
                    walk_k |= k
                    walk_r |= r
    assert walk_k - have_k == set(), sorted(walk_k - have_k)
    assert walk_r - have_r == set(), sorted(walk_r - have_r)
    assert (len(walk_k), len(walk_r)) == (174, 9)  # (DESIGN.md quotes them)
    # the 16-threads-per-output reduce serves 64 slabs or more of a size that is no multiple of 4, and the ragged last block of
    # either reduce kernel a size that is no multiple of 64: no instantiated width has such a size
    assert not any(r[0] == "ks16" for r in walk_r | have_r)
    for dt in (X.F32, X.BF16):
        for mode, ci, co in WGRAD_WIDTHS:
            p = X.wgrad_plan(dt, mode, ci, co, 8, 512, 256)
            assert p["reduce"] != "ks16" and p["ntaps"] * co * ci % 64 == 0, (mode, ci, co)
        widths = {(X.CONV3, C, C) for C in configs.audio_config().model.ch} | \
                 {(X.DOWN4, a, b) for a, b in zip(configs.audio_config().model.ch, configs.audio_config().model.ch[1:])}
        assert widths == set(WGRAD_WIDTHS)
