"""Exact-operand tests of every conv, Down / Upsample and weight-gradient kernel path (tests/exact_util.py).

Dyadic operands make every fp32 summation order exact, so a bf16 output must be RNE(exact) and an fp32 output the exact value
(criterion E); where SiLU enters, criterion S.  Unlike the sigma gates of test_gpu_ops.py these see one dropped, doubled or
misplaced (tap, input channel) term at every width -- the negative controls below prove it on the hardware.  Every case declares
the kernel family / variant it is meant to reach; tests/test_exact_cpu.py confirms that with the library's own launch plan."""
import pytest
import torch

from ddim_audio_amd import _lib
import exact_util as X
from exact_cases import CONV_CASES, DOWNUP_CASES, WGRAD_CASES, DUBWD_CASES, conv_operands, wgrad_operands
from exact_cases import WGRAD_KEY_CASES, DUBWD_KEY_CASES, wgrad_delta, dubwd_operands
import gpu_util as G
from kernel_harness import GUARD, SENTINEL, Out

pytestmark = pytest.mark.gpu
TDT = {X.F32: torch.float32, X.BF16: torch.bfloat16}
REF = torch.device("cpu")  # the fp64 references run on the host (exact on these operands in any order)


_LIVE = []  # device copies handed to the library as raw pointers: alive until the test ends (a temporary's memory is reused at once)


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def _d(t, dt=None):
    d = t.to(G.dev(), TDT[dt] if dt is not None else torch.float32).contiguous()
    _LIVE.append(d)
    return d


def _nan(shape, dt):
    return torch.full(shape, float("nan"), dtype=TDT[dt], device=G.dev())


def _frag(w, kk=9):
    o, i = w.shape[0], w.shape[1]
    wf = torch.empty(kk * o * i, dtype=torch.bfloat16, device=G.dev())
    wd = _d(w)
    _lib.check(_lib.load().ddimx_pack_conv_frag_k(_lib.ptr(wd), _lib.ptr(wf), o, i, kk, _lib.stream()))
    return wf


def _spoil(buf):
    """Zero one nonzero element of a packed weight buffer (the negative control: one (tap, channel) term gone)."""
    nz = (buf != 0).nonzero()
    buf.view(-1)[int(nz[len(nz) // 3])] = 0


def _conv_run(case, spoil=False):
    """Runs one 3x3 conv case through its entry point; returns (got NHWC, exact, approx, delta, plan)."""
    lib = _lib.load()
    dt, fam = case["dt"], case["family"]
    C, B, H, W, xf, act = case["C"], case["B"], case["H"], case["W"], case["xf"], case["act"]
    op = conv_operands(case)
    x, w, bias, add, s, h = op["x"], op["w"], op["bias"], op["add"], op["scale"], op["shift"]
    xn = _d(x, dt)
    y = _nan((B, H, W, C), dt)
    sd, hd = _d(s), _d(h)
    bd = _d(bias) if bias is not None else None
    ad = _d(add) if add is not None else None
    if fam == X.RING:
        wp = G.pack_conv(w.float(), dt)
        if spoil:
            _spoil(wp)
        _lib.check(lib.ddimx_conv3x3_fwd(dt, C, _lib.ptr(xn), _lib.ptr(wp), _lib.ptr(bd), _lib.ptr(ad), C, _lib.ptr(sd), _lib.ptr(hd),
                                         xf, act, _lib.ptr(y), None, B, H, W, _lib.stream()))
        stats = None
    else:
        wp, wf = G.pack_conv(w.float(), dt), _frag(w)
        if spoil:
            _spoil(wf)
        if fam == X.WREG:
            stats = torch.full((int(lib.ddimx_conv3x3_stats_floats(dt, C, B, H, W)),), float("nan"), device=G.dev())
            _lib.check(lib.ddimx_conv3x3_wreg_fwd(C, _lib.ptr(xn), _lib.ptr(wp), _lib.ptr(wf), _lib.ptr(bd), _lib.ptr(ad), C, _lib.ptr(sd),
                                                  _lib.ptr(hd), xf, act, _lib.ptr(y), _lib.ptr(stats), B, H, W, _lib.stream()))
        else:
            stats = torch.full((int(lib.ddimx_conv3x3_pipe_stats_floats(C, B, H, W)),), float("nan"), device=G.dev())
            _lib.check(lib.ddimx_conv3x3_pipe_fwd(C, _lib.ptr(xn), _lib.ptr(wf), _lib.ptr(bd), _lib.ptr(ad), C, _lib.ptr(sd), _lib.ptr(hd),
                                                  xf, _lib.ptr(y), _lib.ptr(stats), B, H, W, _lib.stream()))
    torch.cuda.synchronize()
    dev = REF
    a = op["a_ref"].to(dev)
    z = X.conv3(a, w.to(dev), bias.to(dev) if bias is not None else None, add.to(dev) if add is not None else None)
    delta = None
    if xf == X.XF_AFFINE_SILU:  # operands RNE(silu(.)): products exact, sums not -- bound the order by K 2^-23 conv(|a|, |w|)
        delta = 9 * C * 2.0 ** -23 * X.conv3(a.abs(), w.abs().to(dev))
        if dt == X.F32:  # fp32 mode keeps silu_f's own value (a few ulp of the fp64 one)
            delta = delta + 2.0 ** -20 * X.conv3(a.abs(), w.abs().to(dev))
    approx = act == 1
    exact = X.silu64(z) if approx else z
    if approx and delta is not None:
        delta = 1.1 * delta
    return y, exact, approx, delta, stats, z


def _check_stats(st, doc, other, m, what):
    """st [C][2]: summed per-channel (sum, sum of squares) partials; doc: the values the kernel documents summing (fp64, [..][C]);
    other: the values it must NOT have summed (before / after the output rounding).  Within the fp32 summation bound of the
    documented values (m terms per partial), and -- where the two sets differ -- clearly closer to them than to the other set."""
    for k, f in ((0, lambda v: v), (1, lambda v: v * v)):
        C = doc.shape[-1]
        dv, ov = f(doc).reshape(-1, C).sum(0), f(other).reshape(-1, C).sum(0)
        e_doc, e_oth = (st[:, k] - dv).abs(), (st[:, k] - ov).abs()
        bound = X.sum_bound(f(doc), m) + 1e-6
        assert bool((e_doc <= bound).all()), f"{what}: statistic {k} off by {float(e_doc.max())} (bound {float(bound.max())})"
        if not torch.equal(dv, ov):
            assert float(e_doc.sum()) < 0.5 * float(e_oth.sum()), f"{what}: statistic {k} looks like the sum of the other value set"


def _as_stored(v, dt):
    return X.rne(v) if dt == X.BF16 else v


def _conv_id(c):
    return c["id"]


@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
def test_conv3x3_exact(case):
    y, exact, approx, delta, stats, z = _conv_run(case)
    plan = X.conv_plan(case["dt"], X.CONV3, case["C"], case["C"], case["B"], case["H"], case["W"], case["flags"])
    X.check(y, exact, case["dt"], case["id"], plan, approx=approx, delta=delta)
    if stats is None:
        return
    B, C = case["B"], case["C"]
    got = y.double().cpu()
    if case["family"] == X.PIPE:
        # group slabs [B][wgs][32]: 8 groups x (sum, sumsq) of the fp32 values BEFORE the bf16 rounding, then zeros
        st = stats.cpu().view(B, -1, 32).double()
        assert torch.isfinite(st).all() and float(st[:, :, 16:].abs().max()) == 0.0
        st = st[:, :, :16].sum(1).view(B, 8, 2)
        doc, other = exact.double(), got
        m = plan["th"] * plan["tw"] * plan["tiles_per_wg"] * (C // 8)
        for k, f in ((0, lambda v: v), (1, lambda v: v * v)):
            dv = f(doc).reshape(B, -1, 8, C // 8).sum((1, 3))
            ov = f(other).reshape(B, -1, 8, C // 8).sum((1, 3))
            bound = m * 2.0 ** -23 * f(doc).abs().reshape(B, -1, 8, C // 8).sum((1, 3)) + 1e-3 * 2.0 ** -10
            e_doc, e_oth = (st[:, :, k] - dv).abs(), (st[:, :, k] - ov).abs()
            assert bool((e_doc <= bound).all()), f"{case['id']}: group statistic {k} off the pre-rounding values by {float(e_doc.max())}"
            if not torch.equal(dv, ov):
                assert float(e_doc.sum()) < 0.5 * float(e_oth.sum()), f"{case['id']}: statistics look like the stored values'"
    else:
        # per-channel slabs [B][wgs][C][2] of the stored values
        n = B * plan["wgs_per_sample"] * C * 2
        st = stats.cpu()[:n].view(-1, C, 2).double()
        assert torch.isfinite(st).all(), "statistics partial never written"
        # of the values as stored, not of the fp32 values before the rounding
        _check_stats(st.sum(0), got, exact.double(), plan["th"] * plan["tw"] * plan["tiles_per_wg"], case["id"])


@pytest.mark.parametrize("case", [c for c in CONV_CASES if c.get("control")], ids=_conv_id)
def test_conv3x3_negative_control(case):
    """One element of the packed weights zeroed after packing: the checker must reject the result."""
    y, exact, approx, delta, _, _ = _conv_run(case, spoil=True)
    assert bool(X.mismatches(y, exact, case["dt"], approx, delta).any()), f"{case['id']}: a missing term went unnoticed"


def _downup_run(case, spoil=False):
    lib = _lib.load()
    dt, mode, fam = case["dt"], case["mode"], case["family"]
    cin, cout, B, H, W = case["cin"], case["cout"], case["B"], case["H"], case["W"]
    x = X.dyadic(f"du.x.{case['id']}", (B, H, W, cin), 8, 3)
    bias = X.dyadic(f"du.b.{case['id']}", (cout,), 512, 10)
    xn = _d(x, dt)
    dev = G.dev()
    stats = None
    if mode == X.DOWN4:
        w = X.dyadic(f"du.w.{case['id']}", (cout, cin, 4, 4), 8, 6)
        y = _nan((B, H // 2, W // 2, cout), dt)
        bd = _d(bias)
        if fam == X.WREG:
            wf = _frag(w, 16)
            if spoil:
                _spoil(wf)
            stats = torch.full((int(lib.ddimx_conv_stats_floats(dt, mode, cin, cout, B, H, W)),), float("nan"), device=dev)
            _lib.check(lib.ddimx_downsample_wreg_fwd(cin, cout, _lib.ptr(xn), _lib.ptr(wf), _lib.ptr(bd), _lib.ptr(y), _lib.ptr(stats),
                                                     B, H, W, _lib.stream()))
        else:
            wp = G.pack_conv(w.float(), dt)
            if spoil:
                _spoil(wp)
            _lib.check(lib.ddimx_downsample_fwd(dt, cin, cout, _lib.ptr(xn), _lib.ptr(wp), _lib.ptr(bd), _lib.ptr(y), B, H, W, _lib.stream()))
        exact = X.down4(x, w, bias)
    else:
        w = X.dyadic(f"du.w.{case['id']}", (cin, cout, 4, 4), 8, 6)
        skip = X.dyadic(f"du.s.{case['id']}", (B, 2 * H, 2 * W, cout), 8, 3)
        sn = _d(skip, dt)
        y = _nan((B, 2 * H, 2 * W, cout), dt)
        wp = G.pack_convT(w.float(), dt)
        b2 = _d(torch.cat([bias, bias]))
        if fam == X.WREG:
            wf = torch.empty_like(wp)
            per = 6 * 2 * cout * cin
            for a in range(2):
                _lib.check(lib.ddimx_pack_frag_from_taps(_lib.ptr(wp[a * per:]), _lib.ptr(wf[a * per:]), 6, 2 * cout, cin, _lib.stream()))
            if spoil:
                _spoil(wf)
            stats = torch.full((int(lib.ddimx_conv_stats_floats(dt, mode, cin, cout, B, H, W)),), float("nan"), device=dev)
            _lib.check(lib.ddimx_upsample_add_wreg_fwd(cin, cout, _lib.ptr(xn), _lib.ptr(wf), _lib.ptr(b2), _lib.ptr(sn), _lib.ptr(y),
                                                       _lib.ptr(stats), B, H, W, _lib.stream()))
        else:
            if spoil:
                _spoil(wp)
            _lib.check(lib.ddimx_upsample_add_fwd(dt, cin, cout, _lib.ptr(xn), _lib.ptr(wp), _lib.ptr(b2), _lib.ptr(sn), _lib.ptr(y), B, H, W,
                                                  _lib.stream()))
        # the epilogue stores conv + bias in the activation dtype, then adds the skip tensor and rounds again (bf16 tensors
        # `Upsample(x) + hidden`, models/diffusion.py:284): two roundings, each of an exact value
        exact = _as_stored(X.up4(x, w, bias), dt) + skip
    torch.cuda.synchronize()
    return y, exact, stats


@pytest.mark.parametrize("case", DOWNUP_CASES, ids=_conv_id)
def test_downup_exact(case):
    y, exact, stats = _downup_run(case)
    dt, mode = case["dt"], case["mode"]
    plan = X.conv_plan(dt, mode, case["cin"], case["cout"], case["B"], case["H"], case["W"], case["flags"])
    X.check(y, exact, dt, case["id"], plan if mode == X.DOWN4 else None)
    if stats is None:
        return
    # per-channel slabs of the stored values (Upsample: 2 * cout virtual channels, the two column parities)
    nout = case["cout"] * (2 if mode == X.UP4 else 1)
    ncls = 2 if mode == X.UP4 else 1
    n = case["B"] * plan["wgs_per_sample"] * ncls * nout * 2
    assert n <= stats.numel()
    st = stats.cpu()[:n].double()
    assert torch.isfinite(st).all(), "statistics partial never written"
    st = st.view(-1, nout, 2).sum(0)
    if mode == X.UP4:
        st = st.view(2, case["cout"], 2).sum(0)
    # of the values as stored, not of the values before the last rounding
    _check_stats(st, y.double().cpu(), exact.double(), plan["th"] * plan["tw"] * plan["tiles_per_wg"] * ncls, case["id"])


@pytest.mark.parametrize("case", [c for c in DOWNUP_CASES if c.get("control")], ids=_conv_id)
def test_downup_negative_control(case):
    y, exact, _ = _downup_run(case, spoil=True)
    assert bool(X.mismatches(y, exact, case["dt"]).any()), f"{case['id']}: a missing term went unnoticed"


@pytest.mark.parametrize("dt", [X.F32, X.BF16])
@pytest.mark.parametrize("cin,c0,B,H,W", [(2, 32, 2, 40, 256), (2, 32, 3, 7, 24), (2, 64, 2, 9, 16)])
def test_conv_in_exact(dt, cin, c0, B, H, W):
    """conv_in: fp32 network input with 12 significant bits (products exact in fp32), E on the output in both modes."""
    lib = _lib.load()
    tag = f"cin.{dt}.{c0}.{H}"
    x = X.dyadic(tag + ".x", (B, cin, H, W), 2048, 11)
    w = X.dyadic(tag + ".w", (c0, cin, 3, 3), 8, 6)
    bias = X.dyadic(tag + ".b", (c0,), 512, 10)
    y = _nan((B, H, W, c0), dt)
    stats = torch.full((int(lib.ddimx_conv_in_stats_floats(B, c0, H, W)),), float("nan"), device=G.dev())
    xg, wg, bg = _d(x), _d(w), _d(bias)
    _lib.check(lib.ddimx_conv_in_fwd(dt, _lib.ptr(xg), _lib.ptr(wg), _lib.ptr(bg), _lib.ptr(y), _lib.ptr(stats), B, cin, c0, H, W,
                                     _lib.stream()))
    torch.cuda.synchronize()
    # the fp32 network input enters the exact-fp32 products unrounded in both modes (12 significant bits here: a rounding to
    # bf16 on the way in would show); only the output is rounded
    exact = X.conv3(x.permute(0, 2, 3, 1).contiguous(), w, bias)
    X.check(y, exact, dt, f"conv_in {cin}->{c0} {H}x{W}")


@pytest.mark.parametrize("dt", [X.F32, X.BF16])
@pytest.mark.parametrize("c0,cout,B,H,W", [(32, 2, 2, 40, 256), (32, 2, 3, 9, 24), (40, 2, 2, 10, 16)])
def test_conv_out_exact(dt, c0, cout, B, H, W):
    """conv_out on a + b (a, b on a grid where their sum is exact in bf16): fp32 eps, exact."""
    lib = _lib.load()
    tag = f"cout.{dt}.{c0}.{H}"
    a = X.dyadic(tag + ".a", (B, H, W, c0), 8, 3)
    b = X.dyadic(tag + ".b", (B, H, W, c0), 8, 3)
    w = X.dyadic(tag + ".w", (cout, c0, 3, 3), 8, 6)
    bias = X.dyadic(tag + ".bias", (cout,), 512, 10)
    an, bn = _d(a, dt), _d(b, dt)
    wp, bg = G.pack_conv(w.float(), X.F32), _d(bias)
    eps = torch.full((B, cout, H, W), float("nan"), device=G.dev())
    _lib.check(lib.ddimx_conv_out_fwd(dt, _lib.ptr(an), _lib.ptr(bn), _lib.ptr(wp), _lib.ptr(bg), _lib.ptr(eps), B, c0, cout, H, W,
                                      _lib.stream()))
    torch.cuda.synchronize()
    exact = X.conv3(a + b, w, bias).permute(0, 3, 1, 2)
    X.check(eps, exact, X.F32, f"conv_out {c0}->{cout} {H}x{W}", layout="nchw")


@pytest.mark.parametrize("dt", [X.F32, X.BF16])
@pytest.mark.parametrize("C,B,H,W", [(32, 2, 40, 64), (96, 3, 9, 20), (256, 2, 32, 8)])
def test_resid_gn_exact(dt, C, B, H, W):
    """y = x + (h * scale + shift) with dyadic scale / shift: E, and its per-channel statistics within the fp32 summation bound."""
    lib = _lib.load()
    tag = f"resid.{dt}.{C}"
    x = X.dyadic(tag + ".x", (B, H, W, C), 8, 3)
    h = X.dyadic(tag + ".h", (B, H, W, C), 8, 3)
    s, sh = X.scales(tag + ".s", (B, C)), X.dyadic(tag + ".sh", (B, C), 16, 4)
    y = _nan((B, H, W, C), dt)
    np_ = X.gn_plan(dt, C, B, H, W, 1)["y_np"]
    stats = torch.full((B * np_ * C * 2,), float("nan"), device=G.dev())
    _lib.check(lib.ddimx_resid_gn_fwd(dt, C, _lib.ptr(_d(x, dt)), _lib.ptr(_d(h, dt)), _lib.ptr(_d(s)), _lib.ptr(_d(sh)), _lib.ptr(y),
                                      _lib.ptr(stats), B, H, W, _lib.stream()))
    torch.cuda.synchronize()
    exact = x + X.xf64(h, s, sh, X.XF_AFFINE)
    X.check(y, exact, dt, f"resid C={C} {H}x{W}")
    st = stats.cpu().view(B, np_, C, 2).double()
    assert torch.isfinite(st).all()
    st = st.sum(1)
    for k, f in ((0, lambda v: v), (1, lambda v: v * v)):
        want = f(exact).sum((1, 2))
        bound = (H * W) * 2.0 ** -24 * f(exact).abs().sum((1, 2)) + 1e-6
        assert bool(((st[..., k] - want).abs() <= bound).all()), f"resid statistic {k}"


def _wgrad_run(case):
    """One 3x3 weight-gradient case through ddimx_conv3x3_wgrad, d_w and the partial slabs in guarded buffers; returns (d_w, exact,
    delta, slabs [nsplit][9][C][C])."""
    lib = _lib.load()
    dt, C, B, H, W, xf = case["dt"], case["C"], case["B"], case["H"], case["W"], case["xf"]
    op = wgrad_operands(case)
    dw = Out(C * C * 9)
    part = Out(int(lib.ddimx_conv3x3_wgrad_partial_floats(dt, C, B, H, W)))
    _lib.check(lib.ddimx_conv3x3_wgrad(dt, C, _lib.ptr(_d(op["a"], dt)), _lib.ptr(_d(op["du"], dt)), _lib.ptr(_d(op["scale"])),
                                       _lib.ptr(_d(op["shift"])), xf, part.ptr, dw.ptr, B, H, W, _lib.stream()))
    torch.cuda.synchronize()
    a, du = op["a_ref"], op["du"]
    _guards_intact(part, case["id"] + " partial slabs")
    return dw.read(case["id"] + " d_w").view(C, C, 3, 3), X.wgrad3(a, du), wgrad_delta(case, a, du), part.body.view(-1, 9, C, C)


def _guards_intact(out, what):
    """The guards of an Out alone (Out.read also copies the body to the host: tens of MB for the slabs of the shallow levels)."""
    lo, hi = out.t[:GUARD], out.t[GUARD + out.nbytes:]
    assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), f"{what}: bytes outside the buffer were written"


def _wgrad_check(case):
    dw, exact, delta, slabs = _wgrad_run(case)
    assert slabs.shape[0] == X.wgrad_plan(case["dt"], X.CONV3, case["C"], case["C"], case["B"], case["H"], case["W"])["nsplit"]
    if delta is None:  # exact slabs: their fp64 sum is the exact value, whatever the reduce kernel then does with them
        got = slabs.double().sum(0).permute(1, 2, 0).cpu()
        assert torch.equal(got, exact.reshape(case["C"], case["C"], 9)), case["id"] + ": the sum of the partial slabs is not exact"
    X.check(dw, exact, X.F32, case["id"], layout="nchw", delta=delta)


@pytest.mark.parametrize("case", WGRAD_CASES, ids=_conv_id)
def test_conv3x3_wgrad_exact(case):
    _wgrad_check(case)


@pytest.mark.parametrize("case", WGRAD_KEY_CASES, ids=_conv_id)
def test_conv3x3_wgrad_key_exact(case):
    """One case per (kernel key, reduce key) of the training walk's 3x3 weight gradients (X.wgrad_key): several tiles per workgroup,
    ranges that run into the next sample, a short last workgroup, tiles cut by the image, each under the walk's two transforms."""
    _wgrad_check(case)


def _dubwd_check(case):
    """Downsample / Upsample backward: dx (E in the activation dtype), d_w and d_b (fp32, exact); d_w and the workspace (the
    weight gradient's partial slabs, the bias gradient's partials) in guarded buffers."""
    lib = _lib.load()
    dt, cin, cout, B, H, W = case["dt"], case["cin"], case["cout"], case["B"], case["H"], case["W"]
    tag = case["id"]
    dev = G.dev()
    op = dubwd_operands(case)
    x, dy, w = op["x"], op["dy"], op["w"]
    dx = _nan((B, H, W, cin), dt)
    dwt = Out(cin * cout * 16)
    dbt = torch.full((cout,), float("nan"), device=dev)
    if case["mode"] == X.DOWN4:
        add = op["add"]
        wd = _pack_convT_as(w, dt, I=cout, O=cin)
        ws = Out(int(lib.ddimx_downup_bwd_workspace_bytes(dt, cout, cin, B, H // 2, W // 2)), torch.uint8)
        _lib.check(lib.ddimx_downsample_bwd(dt, cin, cout, _lib.ptr(_d(x, dt)), _lib.ptr(_d(dy, dt)), _lib.ptr(wd), _lib.ptr(_d(add, dt)),
                                            _lib.ptr(dx), dwt.ptr, _lib.ptr(dbt), ws.ptr, B, H, W, _lib.stream()))
        torch.cuda.synchronize()
        X.check(dx, _as_stored(X.up4(dy, w), dt) + add, dt, tag + " dx")  # dx_add joins in the epilogue (as the skip)
        X.check(dwt.read(tag + " d_w").view(cout, cin, 4, 4), X.wgrad_down4(x, dy), X.F32, tag + " d_w", layout="nchw")
    else:
        wd = G.pack_conv(w.float(), dt)  # [O = Cin][I = Cout][4][4]
        ws = Out(int(lib.ddimx_downup_bwd_workspace_bytes(dt, cin, cout, B, H, W)), torch.uint8)
        _lib.check(lib.ddimx_upsample_add_bwd(dt, cin, cout, _lib.ptr(_d(x, dt)), _lib.ptr(_d(dy, dt)), _lib.ptr(wd), _lib.ptr(dx),
                                              dwt.ptr, _lib.ptr(dbt), ws.ptr, B, H, W, _lib.stream()))
        torch.cuda.synchronize()
        X.check(dx, X.down4(dy, w), dt, tag + " dx")
        X.check(dwt.read(tag + " d_w").view(cin, cout, 4, 4), X.wgrad_down4(dy, x), X.F32, tag + " d_w", layout="nchw")
    X.check(dbt, dy.sum((0, 1, 2)), X.F32, tag + " d_b")
    _guards_intact(ws, tag + " workspace")


@pytest.mark.parametrize("case", DUBWD_CASES, ids=_conv_id)
def test_downup_bwd_exact(case):
    _dubwd_check(case)


@pytest.mark.parametrize("case", DUBWD_KEY_CASES, ids=_conv_id)
def test_downup_bwd_key_exact(case):
    """One case per (kernel key, reduce key) of the walk's stride-2 weight gradients, through the Downsample and the Upsample role;
    XF_NONE, so d_w is the fp64 value bit for bit at any number of slabs."""
    _dubwd_check(case)


def _pack_convT_as(w, dt, I, O):
    """The Downsample weight [Cout][Cin][4][4] packed as the ConvTranspose2d weight of its data gradient (I = Cout, O = Cin)."""
    wd = _d(w)
    dst = torch.empty(2 * 6 * 2 * O * I, dtype=TDT[dt], device=G.dev())
    _lib.check(_lib.load().ddimx_pack_convT(dt, _lib.ptr(wd), _lib.ptr(dst), I, O, _lib.stream()))
    return dst


@pytest.mark.parametrize("dt", [X.F32, X.BF16])
@pytest.mark.parametrize("c0,B,H,W", [(32, 2, 40, 256), (32, 3, 9, 24), (40, 2, 10, 16)])
def test_edge_bwd_exact(dt, c0, B, H, W):
    """conv_in / conv_out backward: d_w, d_b exact (fp32) and conv_out's data gradient d_sum (E) -- C0 = 32 takes the register
    kernel conv_out_bwd_data_reg_kernel, C0 = 40 the generic conv_out_bwd_data_kernel; the edge weight gradient its strip form at
    C0 = 32, the tiled form otherwise."""
    lib = _lib.load()
    dev = G.dev()
    cio = 2
    tag = f"edge.{dt}.{c0}.{H}"
    # conv_in: dy [B][H][W][C0], x NCHW fp32 (bf16-exact)
    dy = X.dyadic(tag + ".dy", (B, H, W, c0), 8, 6)
    x = X.dyadic(tag + ".x", (B, cio, H, W), 8, 3)
    part = torch.empty(int(lib.ddimx_edge_bwd_workspace_floats(dt, B, c0, cio, H, W)), device=dev)
    dw = torch.full((c0, cio, 3, 3), float("nan"), device=dev)
    db = torch.full((c0,), float("nan"), device=dev)
    _lib.check(lib.ddimx_conv_in_bwd(dt, _lib.ptr(_d(dy, dt)), _lib.ptr(_d(x)), _lib.ptr(part), _lib.ptr(dw), _lib.ptr(db), B, cio, c0, H,
                                     W, _lib.stream()))
    torch.cuda.synchronize()
    xn = x.permute(0, 2, 3, 1).contiguous()
    X.check(dw, X.wgrad3(xn, dy), X.F32, tag + " conv_in d_w", layout="nchw")
    X.check(db, dy.sum((0, 1, 2)), X.F32, tag + " conv_in d_b")
    # conv_out: d_eps NCHW fp32, a + b NHWC
    de = X.dyadic(tag + ".de", (B, cio, H, W), 8, 6)
    a = X.dyadic(tag + ".a", (B, H, W, c0), 8, 3)
    b = X.dyadic(tag + ".b", (B, H, W, c0), 8, 3)
    w = X.dyadic(tag + ".w", (cio, c0, 3, 3), 8, 6)
    wp = G.pack_conv(w.float(), X.F32)
    ds = _nan((B, H, W, c0), dt)
    part = torch.empty(int(lib.ddimx_edge_bwd_workspace_floats(dt, B, c0, cio, H, W)), device=dev)
    dw = torch.full((cio, c0, 3, 3), float("nan"), device=dev)
    db = torch.full((cio,), float("nan"), device=dev)
    _lib.check(lib.ddimx_conv_out_bwd(dt, _lib.ptr(_d(de)), _lib.ptr(_d(a, dt)), _lib.ptr(_d(b, dt)), _lib.ptr(wp), _lib.ptr(ds),
                                      _lib.ptr(part), _lib.ptr(dw), _lib.ptr(db), B, c0, cio, H, W, _lib.stream()))
    torch.cuda.synchronize()
    den = de.permute(0, 2, 3, 1).contiguous()
    X.check(ds, X.conv3(den, w.transpose(0, 1).flip(2, 3)), dt, tag + " conv_out d_sum")
    X.check(dw, X.wgrad3(a + b, den), X.F32, tag + " conv_out d_w", layout="nchw")
    X.check(db, den.sum((0, 1, 2)), X.F32, tag + " conv_out d_b")


# ---- batch / GroupNorm-path invariance -----------------------------------------------------------------------------------------
def _gn_flips(dt, B, T=1024):
    """{(level, consumer, path)} whose GroupNorm decision (finished in the consumer / by a gn_finalize_groups launch) differs between
    a solo sample and a batch of B: forked, every launch holds one shard of B // 2 samples (model.py forks from 4 samples up,
    walk_infer.cpp: samples [0, B/2) and [B/2, B)); single-stream, all B."""
    from ddim_audio_amd import configs
    cfg = configs.audio_config()
    ch, f = cfg.model.ch, cfg.model.f_size
    flips = set()
    for l, C in enumerate(ch):
        H, W = T >> l, f >> l
        y = X.gn_plan(dt, C, 1, H, W, 1)["y_np"]  # (the first block's input comes from conv_in / Downsample: same order of size)
        solo = X.gn_plan(dt, C, 1, H, W, y)
        for path, n in (("forked", B // 2), ("single", B)):
            got = X.gn_plan(dt, C, n, H, W, y)
            flips |= {(l, cons, path) for cons in ("conv0", "conv1", "resid") if got[cons] != solo[cons]}
    return flips


@pytest.mark.parametrize("dt", [X.F32, X.BF16])
def test_sample_result_is_batch_and_gn_path_invariant(dt):
    """Every sample's eps at T = 1024 in a batch of 64 (cfg3's batch) is bit-identical to its eps alone, forked and single-stream.
    The test asserts, through the library's own GroupNorm rule, that the batch moves levels 0-3 to the other GroupNorm path
    (in-kernel vs gn_finalize_groups) on at least one of the two paths; levels 4-5 stay fused up to 64 samples."""
    from ddim_audio_amd import configs, synth
    import ddim_audio_amd as D
    B = 64
    flips = _gn_flips(dt, B)
    assert {l for l, _, _ in flips} >= {0, 1, 2, 3}, sorted(flips)
    s = {X.F32: "torch.cuda.FloatTensor", X.BF16: "torch.cuda.BFloat16Tensor"}[dt]
    m = synth.fill_module(D.Model(configs.audio_config(s)), seed=5).eval()
    x = synth.gaussian("exact.inv.x", (B, 2, 1024, 256)).cuda()
    t = (torch.arange(B) * 13 + 5).cuda() % 1000
    with torch.no_grad():
        solo = torch.cat([m(x[i:i + 1], t[i:i + 1]) for i in range(B)])
        for fork in (True, False):
            y = m.forward(x, t, _fork=fork)
            same = (y == solo).reshape(B, -1).all(1)
            assert bool(same.all()), f"samples {same.logical_not().nonzero().flatten().tolist()} differ at B = {B} " \
                                     f"({'forked' if fork else 'single stream'})"
