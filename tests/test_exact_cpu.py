"""Host checks of the exact-operand tests (tests/test_gpu_exact.py): each case reaches the kernel family / variant / tiling it
declares (the library's own conv_plan / wgrad_plan, host only), its operand ranges make fp32 summation order irrelevant, one
missing (tap, input channel) term violates its criterion, and the cases cover every kernel key the network walks launch."""
import pytest
import torch

import exact_util as X
from exact_cases import CONV_CASES, DOWNUP_CASES, WGRAD_CASES, DUBWD_CASES, DOWN_PAIRS, UP_PAIRS, conv_operands, wgrad_operands
from ddim_audio_amd import configs


def _id(c):
    return c["id"]


@pytest.mark.parametrize("case", CONV_CASES, ids=_id)
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


@pytest.mark.parametrize("case", [c for c in CONV_CASES if c["xf"] != X.XF_AFFINE_SILU], ids=_id)
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


# ---- coverage of the network walks ---------------------------------------------------------------------------------------------
# Keys no per-op entry point can reach, each with the composite test that runs it.
COMPOSITE_ONLY = {
    "gn.stats": "in-kernel GroupNorm prologue: test_gpu_exact.py::test_sample_result_is_batch_and_gn_path_invariant, "
                "test_gpu_model.py::test_model_forward_golden",
    "bwd_mode": "dgrad epilogue with GroupNorm-backward statistics: test_gpu_gn_kernels.py::test_dgrad_conv_statistics_epilogue "
                "(ddimx_conv3x3_dgrad_stats, modes 1 and 2 alone), test_gpu_train.py (ddimx_resblock_bwd, ddimx_unet_bwd)",
    "act2": "training stores of pre-activations: test_gpu_train.py (ddimx_resblock_fwd_train, ddimx_unet_fwd_train)",
}


# Walk keys no per-op entry point can plan: the reason, and the test that runs the launch.
NO_PER_OP = {
    (X.RING, X.CONV3, 128, 128, X.BF16, 1, False, True):
        "training forward of level 3 at T = 4096, B = 1 only: the batch plan picks variant 1 for a sample too large for the "
        "sample-size rule of ddimx_conv3x3_fwd, and only the batch plan gives variant 1 several tiles per workgroup.  No exact test "
        "runs it; the training walk is checked against the oracle at other shapes (test_gpu_train.py, test_gpu_configs.py)",
}


def _walk_keys(cfg, T, B, dt):
    """(family, mode, cin, cout, dt, var, ragged, multi) of every conv the inference and training walks launch."""
    ch, f = cfg.model.ch, cfg.model.f_size
    keys = set()

    def add(mode, cin, cout, H, W, flags):
        p = X.conv_plan(dt, mode, cin, cout, B, H, W, flags)  # a shape the walk launches must plan: a failure is a finding
        keys.add((p["family"], mode, cin, cout, dt, p["var"], p["ragged"], p["multi"]))

    for l, C in enumerate(ch):
        H, W = T >> l, f >> l
        if H < 1 or W < 1:
            continue
        wf = X.P_WFRAG if dt == X.BF16 else 0
        # inference: GroupNorm input finished in-kernel (composite) or by a finalize launch -- the plan is the same either way
        add(X.CONV3, C, C, H, W, wf | X.P_XF(2) | X.P_ACT(1) | X.P_STATS | X.P_GROUPS)
        add(X.CONV3, C, C, H, W, wf | X.P_XF(1) | X.P_ACT(1) | X.P_STATS | X.P_GROUPS)
        # training forward (batch plan, act = 2 stores: composite), backward data-gradient convs (bwd_mode: composite)
        add(X.CONV3, C, C, H, W, X.P_BATCH | X.P_XF(2) | X.P_ACT(1) | X.P_STATS)
        if l > 0:
            add(X.DOWN4, ch[l - 1], C, 2 * H, 2 * W, wf | X.P_STATS | X.P_GROUPS)
            add(X.UP4, C, ch[l - 1], H, W, wf | X.P_SKIP | X.P_STATS | X.P_GROUPS)
            add(X.DOWN4, ch[l - 1], C, 2 * H, 2 * W, X.P_BATCH)
            add(X.UP4, C, ch[l - 1], H, W, X.P_BATCH)
            add(X.UP4, C, ch[l - 1], H, W, X.P_BATCH | X.P_SKIP)
    return keys


def _case_keys():
    keys = set()
    for c in CONV_CASES:
        p = X.conv_plan(c["dt"], X.CONV3, c["C"], c["C"], c["B"], c["H"], c["W"], c["flags"])
        keys.add((p["family"], X.CONV3, c["C"], c["C"], c["dt"], p["var"], p["ragged"], p["multi"]))
    for c in DOWNUP_CASES:
        p = X.conv_plan(c["dt"], c["mode"], c["cin"], c["cout"], c["B"], c["H"], c["W"], c["flags"])
        keys.add((p["family"], c["mode"], c["cin"], c["cout"], c["dt"], p["var"], p["ragged"], p["multi"]))
    for c in DUBWD_CASES:  # the data-gradient convs of ddimx_downsample_bwd / ddimx_upsample_add_bwd (batch plan)
        dt, B = c["dt"], c["B"]
        if c["mode"] == X.DOWN4:
            p = X.conv_plan(dt, X.UP4, c["cout"], c["cin"], B, c["H"] // 2, c["W"] // 2, X.P_BATCH | X.P_SKIP)
            keys.add((p["family"], X.UP4, c["cout"], c["cin"], dt, p["var"], p["ragged"], p["multi"]))
        else:
            p = X.conv_plan(dt, X.DOWN4, c["cout"], c["cin"], B, 2 * c["H"], 2 * c["W"], X.P_BATCH)
            keys.add((p["family"], X.DOWN4, c["cout"], c["cin"], dt, p["var"], p["ragged"], p["multi"]))
    return keys


def test_exact_cases_cover_the_walks_kernel_keys():
    """Every (family, mode, cin, cout, dtype, variant, ragged, multi-tile workgroup) key the inference and training walks launch at
    T in {32, 96, 1024, 4096, 8192}, B in {1, 8, 32} (audio and tiny configs) is reached by an exact case.  Each (C, variant) is a
    template instantiation of its own, and ragged / multi-tile workgroups run other halo and epilogue code."""
    have = _case_keys()
    missing = set()
    for cfg in (configs.audio_config(), configs.tiny_config()):
        for dt in (X.F32, X.BF16):
            for T in (32, 96, 1024, 4096, 8192):
                for B in (1, 8, 32):
                    missing |= _walk_keys(cfg, T, B, dt) - have
    assert missing == set(NO_PER_OP), sorted((X.FAMILY[k[0]],) + k[1:] for k in missing ^ set(NO_PER_OP))
    assert set(COMPOSITE_ONLY) == {"gn.stats", "bwd_mode", "act2"}
