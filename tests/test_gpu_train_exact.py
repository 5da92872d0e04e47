"""Exact-operand tests of the training-only paths of conv_mfma_kernel, and the tape of ddimx_resblock_fwd_train.

The training step runs the conv kernel through three epilogues no inference launch takes: act = 2 (the pre-activation is stored, the
statistics are those of its SiLU), and ConvCfg::BWD with bwd_mode 1 / 2 (a data-gradient conv that takes the GroupNorm-backward sums
(P, Q) of its own output) -- 15 kernels of their own.  On the dyadic operands of tests/exact_cases.py every fp32 summation order is
exact, so the stored tensor must be RNE(exact) in bf16 and the exact value in fp32 (criterion E of tests/exact_util.py; with the
summation bound of tests/test_gpu_exact.py where a SiLU operand feeds the sum): one dropped, doubled or misplaced (tap, channel) term
shows at every width, which the sigma gates of test_gpu_train.py cannot see.  tests/test_exact_cpu.py proves on the host that the
cases reach every (width, dtype, variant, ragged, tiles per workgroup, epilogue) key the training walk launches.

Every output lies in a guarded buffer and every input keeps a snapshot of its bits (tests/kernel_harness.py)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from ddim_audio_amd import _lib, synth
from oracle import ref_cpu
import exact_util as X
from exact_cases import TRAIN_FWD_CASES, BATCH_PLAIN_CASES, DGRAD_CASES, conv_operands, dgrad_operands, dgrad_exact
import gn_kernel_ref as R
import gpu_util as G
import kernel_harness as H
import model_harness as MH
from kernel_harness import Out, Ro

pytestmark = pytest.mark.gpu
TDT = G.TORCH_DT


def _id(c):
    return c["id"]


def _spoil(buf):
    """Zero one nonzero element of a packed weight buffer (the negative control: one (tap, channel) term gone)."""
    nz = (buf != 0).nonzero()
    buf.view(-1)[int(nz[len(nz) // 3])] = 0


def _opt(r):
    return None if r is None else r.ptr


# ---- forward convs of the training walk ---------------------------------------------------------------------------------------------
def _fwd_buffers(case, want_stats=True):
    dt, C, B, Hh, W = case["dt"], case["C"], case["B"], case["H"], case["W"]
    op = conv_operands(case)
    ins = dict(x=Ro(op["x"], TDT[dt]), w=Ro(G.pack_conv(op["w"].float(), dt), TDT[dt]), s=Ro(op["scale"]), h=Ro(op["shift"]),
               bias=None if op["bias"] is None else Ro(op["bias"]), add=None if op["add"] is None else Ro(op["add"]))
    y = Out(B * Hh * W * C, TDT[dt])
    st = Out(int(H.lib().ddimx_conv3x3_stats_floats(dt, C, B, Hh, W))) if want_stats else None
    return op, ins, y, st


def _fwd_call(case, ins, y, st, plan_flags):
    dt, C, B, Hh, W = case["dt"], case["C"], case["B"], case["H"], case["W"]
    return H.lib().ddimx_conv3x3_fwd_ex(dt, C, ins["x"].ptr, ins["w"].ptr, _opt(ins["bias"]), _opt(ins["add"]), C, ins["s"].ptr, ins["h"].ptr,
                                        case["xf"], case["act"], y.ptr, _opt(st), plan_flags, B, Hh, W, _lib.stream())


def _fwd_run(case, want_stats=True):
    """One conv through ddimx_conv3x3_fwd_ex; returns (stored NHWC tensor, statistics buffer, exact pre-activation z, delta)."""
    dt, C, B, Hh, W, xf = case["dt"], case["C"], case["B"], case["H"], case["W"], case["xf"]
    op, ins, y, st = _fwd_buffers(case, want_stats)
    _lib.check(_fwd_call(case, ins, y, st, X.P_BATCH if case.get("batch") else 0))
    H.sync()
    for r in ins.values():
        if r is not None:
            r.check(case["id"])
    a, w = op["a_ref"], op["w"]
    z = X.conv3(a, w, op["bias"], op["add"])
    delta = None
    if xf in (X.XF_AFFINE_SILU, X.XF_SILU_AFFINE):  # the bounds of tests/test_gpu_exact.py::_conv_run for an operand RNE(SiLU(.))
        delta = 9 * C * 2.0 ** -23 * X.conv3(a.abs(), w.abs())
        if dt == X.F32:
            delta = delta + 2.0 ** -20 * X.conv3(a.abs(), w.abs())
    return y.read("y").view(B, Hh, W, C), st, z, delta


def _s_ratio(got, exact, dt, delta):
    """The worst |got - exact| in units of the tolerance X.mismatches allows where a summation bound is given (for the report)."""
    tol = X.ulp(exact, 8) if dt == X.BF16 else 4.0 * X.ulp(exact, 24) + 2.0 ** -18 * exact.abs()
    return float(((got.double() - exact).abs() / (tol + delta)).max())


def _sums12(v):
    """v [B][HW][C] -> (sum, sum of squares) [B][C][2] and the sums of the absolute terms, fp64."""
    return torch.stack([v.sum(1), (v * v).sum(1)], -1), torch.stack([v.abs().sum(1), (v * v).sum(1)], -1)


@pytest.mark.parametrize("case", TRAIN_FWD_CASES, ids=_id)
def test_train_fwd_conv_exact(case):
    """act = 2: the stored tensor is the PRE-activation z = conv(a) + bias / temb -- E where no SiLU feeds the sum (xf 0, 1), E with
    the summation bound of test_gpu_exact.py where one does (xf 2: conv.0 of the block, xf 3: conv.1) -- and the channel-format
    slabs, summed in fp64, are the sums of SiLU(value as stored) within (th tw tiles_per_wg + SILU_OPS) 2^-24 sum |terms|, and
    clearly closer to them than to the sums of the stored values themselves.  Slabs past the plan's count stay untouched.
    Measured on MI355X: where a SiLU feeds the sum the stored tensor is at most 0.50 of the tolerance in bf16 (half an ulp: the
    rounding itself) and 7.9e-3 in fp32; the statistics at most 6.2e-2 of the summation bound."""
    dt, C, B = case["dt"], case["C"], case["B"]
    got, st, z, delta = _fwd_run(case)
    plan = X.conv_plan(dt, X.CONV3, C, C, B, case["H"], case["W"], case["flags"])
    X.check(got, z, dt, case["id"], plan, delta=delta)
    if delta is not None:
        H.report(f"{case['id']} stored", _s_ratio(got, z, dt, delta), "of the S tolerance")
    wgs = plan["wgs_per_sample"]
    slabs = st.read("statistics", used=B * wgs * C * 2).view(B, wgs, C, 2).double()
    assert bool(torch.isfinite(slabs).all()), "statistics partial never written"
    sums = slabs.sum(1)
    v = got.double().reshape(B, -1, C)
    want, ab = _sums12(X.silu64(v))
    worst = R.gate_sum(sums, want, ab, plan["th"] * plan["tw"] * plan["tiles_per_wg"] + R.SILU_OPS, f"{case['id']} statistics")
    other, _ = _sums12(v)
    for k in range(2):
        e_doc, e_oth = (sums[..., k] - want[..., k]).abs().sum(), (sums[..., k] - other[..., k]).abs().sum()
        assert float(e_doc) < 0.5 * float(e_oth), f"{case['id']}: statistic {k} looks like the sum of the stored values, not of their SiLU"
    H.report(f"{case['id']} statistics", worst, "of the summation bound")


@pytest.mark.parametrize("case", [next(c for c in TRAIN_FWD_CASES if c["xf"] == X.XF_AFFINE_SILU and c["dt"] == X.BF16 and c["H"] <= 16)], ids=_id)
def test_train_fwd_negative_control(case):
    """The checker rejects a reference that applies SiLU to the output: comparing with z, not SiLU(z), is what proves the store."""
    got, _, z, delta = _fwd_run(case)
    X.check(got, z, case["dt"], case["id"], delta=delta)
    assert bool(X.mismatches(got, X.silu64(z), case["dt"], False, delta).any()), f"{case['id']}: SiLU(z) passes for z"


@pytest.mark.parametrize("case", BATCH_PLAIN_CASES, ids=_id)
def test_batch_plan_plain_conv_exact(case):
    """The plain epilogue (no statistics, no activation: a data-gradient conv that leaves its statistics to gn_bwd_stats) under a
    plan on the real batch -- variant 1 with several tiles per workgroup, which the sample-size rule never picks: E."""
    got, _, z, _ = _fwd_run(case, want_stats=False)
    plan = X.conv_plan(case["dt"], X.CONV3, case["C"], case["C"], case["B"], case["H"], case["W"], case["flags"])
    assert plan["var"] == 1 and plan["multi"]
    X.check(got, z, case["dt"], case["id"], plan)


def test_fwd_ex_refuses_unknown_plan_flags():
    """Any bit but DDIMX_PLAN_BATCH in plan_flags: a message, nothing launched, the outputs untouched."""
    case = TRAIN_FWD_CASES[0]
    _, ins, y, st = _fwd_buffers(case)
    for flags in (X.P_STATS, X.P_BATCH | X.P_BWD, X.P_XF(2), 1 << 20, -1):
        H.refused(_fwd_call(case, ins, y, st, flags), y, st, who="ddimx_conv3x3_fwd_ex")


# ---- data-gradient convs with the GroupNorm-backward statistics epilogue ---------------------------------------------------------
_ROW = {c["row"]: c for c in DGRAD_CASES}


@functools.lru_cache(maxsize=2)
def _dgrad_ref(row):
    """(operands, exact dg) of one row, shared by its two bwd_modes and left unchanged."""
    op = dgrad_operands(_ROW[row])
    return op, dgrad_exact(op["du"], op["w"])


def _dgrad_run(case, spoil=False):
    dt, C, B, Hh, W, mode = case["dt"], case["C"], case["B"], case["H"], case["W"], case["bwd_mode"]
    op, _ = _dgrad_ref(case["row"])
    wd = G.pack_conv_dgrad(op["w"].float(), dt)
    if spoil:
        _spoil(wd)
    ins = [Ro(op["du"], TDT[dt]), Ro(wd, TDT[dt]), Ro(op["aux"], TDT[dt]), Ro(op["scale"]), Ro(op["shift"])]
    dg = Out(B * Hh * W * C, TDT[dt])
    st = Out(B * X.gn_plan(dt, C, B, Hh, W, 1)["y_np"] * C * 2)  # what the block's workspace holds: resid's partition
    npc = ctypes.c_int(-1)
    _lib.check(H.lib().ddimx_conv3x3_dgrad_stats(dt, C, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr if mode == 2 else None,
                                                 ins[4].ptr if mode == 2 else None, mode, dg.ptr, st.ptr, ctypes.byref(npc), B, Hh, W,
                                                 _lib.stream()))
    H.sync()
    for r in ins:
        r.check(case["id"])
    return dg.read("dg").view(B, Hh, W, C), st, npc.value


def _slab_abs_sums(v, plan):
    """Sums of |v| [B][H][W][C] over the pixels of each workgroup's tiles_per_wg consecutive tiles: [B][wgs_per_sample][C]."""
    B, Hh, W, C = v.shape
    ty, tx = torch.arange(Hh)[:, None] // plan["th"], torch.arange(W)[None, :] // plan["tw"]
    slab = ((ty * plan["tiles_x"] + tx) // plan["tiles_per_wg"]).reshape(-1)
    assert int(slab.max()) == plan["wgs_per_sample"] - 1
    return torch.zeros(B, plan["wgs_per_sample"], C, dtype=torch.float64).index_add_(1, slab, v.abs().reshape(B, -1, C))


@pytest.mark.parametrize("case", DGRAD_CASES, ids=_id)
def test_dgrad_conv_exact(case):
    """dg = conv3(du, w transposed and flipped) is linear: E on every element (RNE(exact) in bf16, the exact value in fp32).
    bwd_mode 1: P = sum dg -- every slab's sum of |dg| fits 24 bits of the 2^-12 grid (asserted on the reference), so the slabs,
    summed in fp64, equal the fp64 sum bit for bit; Q = sum dg SiLU(aux), and both sums of bwd_mode 2 (g' = dg SiLU'(s aux + t),
    P = sum g', Q = sum g' aux), within (HW + SILU_OPS) 2^-24 sum |terms| of the fp64 sums over the stored dg.
    Measured on MI355X: at most 1.4e-1 of the summation bound (at 1 x 4 pixels; 1.7e-2 at the larger shapes)."""
    dt, C, B, Hh, W, bwd_mode = case["dt"], case["C"], case["B"], case["H"], case["W"], case["bwd_mode"]
    op, exact = _dgrad_ref(case["row"])
    got, st, nparts = _dgrad_run(case)
    plan = X.conv_plan(dt, X.CONV3, C, C, B, Hh, W, case["flags"])
    assert nparts == plan["wgs_per_sample"] > 0, "the block takes these statistics from the conv at this shape"
    X.check(got, exact, dt, case["id"], plan)
    slabs = st.read("statistics", used=B * nparts * C * 2).view(B, nparts, C, 2).double()
    assert bool(torch.isfinite(slabs).all()), "statistics partial never written"
    sums = slabs.sum(1)
    HW = Hh * W
    stored = X.rne(exact) if dt == X.BF16 else exact  # (= got, by the check above)
    dgv, aux = stored.reshape(B, HW, C), op["aux"].reshape(B, HW, C)
    s_, t_ = (op["scale"], op["shift"]) if bwd_mode == 2 else (None, None)
    want = R.bwd_stats(dgv, aux, bwd_mode - 1, HW, s_, t_)[:, 0]
    ab = R.bwd_abs_slabs(dgv, aux, bwd_mode - 1, HW, s_, t_)[:, 0]
    n = HW + R.SILU_OPS
    if bwd_mode == 1:
        assert float(_slab_abs_sums(stored, plan).max()) * 2.0 ** 12 < 2.0 ** 24
        assert torch.equal(sums[..., 0], dgv.sum(1)), f"{case['id']}: P is not the sum of the stored dg"
        worst = R.gate_sum(sums[..., 1], want[..., 1], ab[..., 1], n, f"{case['id']} Q")
    else:
        worst = R.gate_sum(sums, want, ab, n, f"{case['id']} (P, Q)")
    H.report(case["id"], worst, "of the summation bound")


@pytest.mark.parametrize("case", [c for c in DGRAD_CASES if c["control"]], ids=_id)
def test_dgrad_negative_control(case):
    """One non-zero element of the packed data-gradient weights zeroed after packing: the checker must reject dg."""
    _, exact = _dgrad_ref(case["row"])
    got, _, nparts = _dgrad_run(case, spoil=True)
    assert nparts > 0
    assert bool(X.mismatches(got, exact, case["dt"]).any()), f"{case['id']}: a missing term went unnoticed"


# ---- the tape of the training forward ---------------------------------------------------------------------------------------------
RB_NAMES = ("norm.0.weight", "norm.0.bias", "norm.1.weight", "norm.1.bias", "norm.2.weight", "conv.1.bias")


def _rb_tape_reference(sd, p, x, temb):
    """(u1, u2, y) of oracle/ref_cpu.residual_block, its lines restated without autograd: u1 = conv.0(SiLU(GN0 x)) + temb,
    u2 = conv.1(GN1 SiLU(u1)) + bias, y = x + GN2 SiLU(u2).  NCHW, in the dtype of its arguments."""
    eps = 1e-6
    h = F.silu(F.group_norm(x, 8, sd[p + "norm.0.weight"], sd[p + "norm.0.bias"], eps))
    u1 = F.conv2d(h, sd[p + "conv.0.weight"], None, stride=1, padding=1) + temb[..., None, None]
    h = F.group_norm(F.silu(u1), 8, sd[p + "norm.1.weight"], sd[p + "norm.1.bias"], eps)
    u2 = F.conv2d(h, sd[p + "conv.1.weight"], sd[p + "conv.1.bias"], stride=1, padding=1)
    return u1, u2, x + F.group_norm(F.silu(u2), 8, sd[p + "norm.2.weight"], None, eps)


@pytest.mark.parametrize("dt", [G.F32, G.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("c,hw", [(32, (40, 72)), (128, (16, 24)), (256, (20, 9))])
def test_resblock_train_tape(dt, c, hw):
    """u1, u2 and y of ddimx_resblock_fwd_train against the fp64 restatement of the oracle's Residual_Block at the forward yardsticks
    of test_gpu_train.py, and tape_small -- [6][B][C] scale / shift of GN0..2, then [3][B][8][2] mean / rstd -- against the fp64
    GroupNorm constants of the tensors as stored (x, SiLU(u1), SiLU(u2)) at the fp32 gate of gn_kernel_ref.gate_stats_of_norm.
    Measured on MI355X: u1 / u2 / y at most max 8.3e-6, rms 1.2e-6 of std in fp32 and max 2.9e-2, rms 4.5e-3 in bf16; tape_small at
    most 5.9e-3 of the gate."""
    lib = H.lib()
    b, (hh, ww) = 2, hw
    p = f"rbt{c}."
    sd = MH.rb_sd(p, c)
    x = synth.gaussian(p + "x", (b, c, hh, ww)) * 1.5 + 0.3
    temb = synth.gaussian(p + "temb", (b, c)) * 0.5
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        u1r, u2r, yr = _rb_tape_reference(sd64, p, x.double(), temb.double())
        assert torch.allclose(yr, ref_cpu.residual_block(sd64, p, x.double(), temb.double()), rtol=0, atol=1e-12)
    xn = Ro(G.to_nhwc(x, dt), TDT[dt])
    k = {n: Ro(sd[p + n]) for n in RB_NAMES}
    w0, w1 = (Ro(G.pack_conv(sd[p + f"conv.{i}.weight"], dt), TDT[dt]) for i in range(2))
    tg = Ro(temb)
    n = b * hh * ww * c
    y, u1, u2 = (Out(n, TDT[dt]) for _ in range(3))
    small = Out(int(lib.ddimx_rb_tape_floats(b, c)))
    ws = torch.empty(int(lib.ddimx_op_workspace_bytes(dt, b, c, hh, ww)), dtype=torch.uint8, device=G.dev())
    _lib.check(lib.ddimx_resblock_fwd_train(dt, c, xn.ptr, y.ptr, tg.ptr, c, k["norm.0.weight"].ptr, k["norm.0.bias"].ptr, w0.ptr,
                                            k["norm.1.weight"].ptr, k["norm.1.bias"].ptr, w1.ptr, k["conv.1.bias"].ptr,
                                            k["norm.2.weight"].ptr, u1.ptr, u2.ptr, small.ptr, _lib.ptr(ws), b, hh, ww, _lib.stream()))
    H.sync()
    for r in [xn, w0, w1, tg] + list(k.values()):
        r.check(f"resblock_fwd_train C={c}")
    nchw = lambda o, what: o.read(what).view(b, hh, ww, c).permute(0, 3, 1, 2).double()  # noqa: E731
    u1g, u2g, yg = nchw(u1, "u1"), nchw(u2, "u2"), nchw(y, "y")
    for got, want, what in ((u1g, u1r, "u1"), (u2g, u2r, "u2"), (yg, yr, "y")):
        mx, rms = G.check_close(got, want, dt, f"tape {what} C={c}")
        H.report_std(f"tape {what} C={c} dt={dt}", mx, rms)
    tape = small.read("tape_small").double()
    aff, mr = tape[:6 * b * c].view(3, 2, b, c), tape[6 * b * c:].view(3, b, 8, 2)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(b, hh * ww, c)  # noqa: E731
    stored = (xn.t.cpu().double().view(b, hh * ww, c), X.silu64(flat(u1g)), X.silu64(flat(u2g)))
    worst = 0.0
    for i, (v, gam, bet) in enumerate(zip(stored, ("norm.0.weight", "norm.1.weight", "norm.2.weight"), ("norm.0.bias", "norm.1.bias", None))):
        want = R.group_norm_fold(v, sd64[p + gam], None if bet is None else sd64[p + bet])
        e = R.gate_stats_of_norm(aff[i, 0], aff[i, 1], mr[i, :, :, 0], mr[i, :, :, 1], want, f"tape_small GN{i} C={c}")
        worst = max(worst, e / G.TOL[G.F32]["mx"])
    H.report(f"tape_small C={c} dt={dt}", worst)
