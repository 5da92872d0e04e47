"""The register-streamed Upsample and the three deep Downsample convs (csrc/conv_wreg.h), one launch at a time through the C ABI.

Upsample: a wave multiplies only the two column taps its output-column parity has (of the three the sub-pixel layout stores).
Downsample 96->128, 128->192, 192->256: planned with output-channel splits and / or a split of the taps over two wave groups.

Operands of the exact tests are small integers times powers of two, so every partial sum any summation order can form is exact in
fp32 and a bf16 output has ONE right value: the reference is torch's fp32 convolution on the CPU, compared bit for bit.

* Upsample: x integers in [-4, 4]; w[ci][co][kh][kw] = +-2^(e(kh, kw) + ci % 2), e = 4 * class + place, where class = (kh % 2, kw % 2)
  is the output-pixel parity the tap feeds and place = (kh // 2, kw // 2): 16 different magnitudes, the four taps that meet in one
  output within a factor 2^4 of each other, so |sum| <= (1 + 2 + 4 + 8) * 2 * 256 channels * 4 < 2^15 of the class's grid 2^(4 class).
  The skip tensor is scaled per output parity the same way (so that it shows beside the convolution in every class).
* Downsample: all 16 taps meet in one output, so 16 different powers of two and K = 16 * 192 terms do not fit 24 bits; the taps get
  the distinct integer weights 1 .. 16 instead: w[co][ci][kh][kw] = +-(4 kh + kw + 1) * 2^((ci // 16) % 3 + (co // 32) % 2), x integers in
  [-4, 4]: |sum| <= 136 * 8 * 192 * 4 < 2^20.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

from ddim_audio_amd import _lib, synth
import exact_util as X
import gpu_util as G
import kernel_harness as H

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
B = 3
UP_PAIRS = [(64, 32), (96, 64), (128, 96), (192, 128), (256, 192)]   # (Cin, Cout) of Upsample
DOWN_PAIRS = [(96, 128), (128, 192), (192, 256)]                      # (Cin, Cout) of the three deep Downsample convs
UP_FLAGS = X.P_WFRAG | X.P_SKIP | X.P_STATS
DOWN_FLAGS = X.P_WFRAG | X.P_STATS


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def _ints(tag, shape, k):
    return torch.randint(-k, k + 1, shape, generator=_gen(tag)).float()


def _signs(tag, shape):
    return torch.randint(0, 2, shape, generator=_gen(tag)).float() * 2 - 1


def _tile(mode, cin, cout):
    """(th, tw) of the register-streamed kernel's tile for this conv (a 64 x 64 input is whole tiles of every config)."""
    p = X.conv_plan(X.BF16, mode, cin, cout, B, 64, 64, UP_FLAGS if mode == X.UP4 else DOWN_FLAGS)
    assert p["family"] == X.WREG
    return p["th"], p["tw"]


def _nhwc(t):
    """NCHW fp32 on the CPU -> NHWC bf16 (the values are bf16 numbers already)."""
    assert torch.equal(t.bfloat16().float(), t)
    return t.permute(0, 2, 3, 1).contiguous().bfloat16()


def _up_frag(w):
    """ConvTranspose2d weight [I][O][4][4] -> both row-parity classes in fragment order, as the walk's packing makes them."""
    lib = H.lib()
    cin, cout = w.shape[0], w.shape[1]
    wp = G.pack_convT(w.float(), X.BF16)
    wf = torch.empty_like(wp)
    per = 6 * 2 * cout * cin
    for a in range(2):
        _lib.check(lib.ddimx_pack_frag_from_taps(_lib.ptr(wp[a * per:]), _lib.ptr(wf[a * per:]), 6, 2 * cout, cin, _lib.stream()))
    H.sync()
    return H.Ro(wf, BF)


def _run_up(cin, cout, x, wf, bias, skip):
    """x [b][cin][h][w], skip [b][cout][2h][2w] fp32 on the CPU -> (y [b][2h][2w][cout] bf16, the statistics floats written)."""
    lib = H.lib()
    b, _, h, w = x.shape
    xd, sd, b2 = H.Ro(_nhwc(x), BF), H.Ro(_nhwc(skip), BF), H.Ro(torch.cat([bias, bias]))
    y = H.Out(b * 4 * h * w * cout, BF)
    stats = H.Out(int(lib.ddimx_conv_stats_floats(X.BF16, X.UP4, cin, cout, b, h, w)))
    _lib.check(lib.ddimx_upsample_add_wreg_fwd(cin, cout, xd.ptr, wf.ptr, b2.ptr, sd.ptr, y.ptr, stats.ptr, b, h, w, _lib.stream()))
    H.sync()
    what = f"up {cin}->{cout} B={b}"
    for r in (xd, sd, b2, wf):
        r.check(what)
    plan = X.conv_plan(X.BF16, X.UP4, cin, cout, b, h, w, UP_FLAGS)
    assert plan["family"] == X.WREG
    st = stats.read(what + " statistics", used=b * plan["wgs_per_sample"] * 2 * 2 * cout * 2)
    assert bool(torch.isfinite(st).all()), what + ": a statistics partial was never written"
    return y.read(what).view(b, 2 * h, 2 * w, cout), st


def _run_down(cin, cout, x, wf, bias):
    """x [b][cin][h][w] fp32 on the CPU -> (y [b][h/2][w/2][cout] bf16, statistics [b][parts][cout][2], the plan)."""
    lib = H.lib()
    b, _, h, w = x.shape
    xd, bd = H.Ro(_nhwc(x), BF), H.Ro(bias)
    y = H.Out(b * (h // 2) * (w // 2) * cout, BF)
    stats = H.Out(int(lib.ddimx_conv_stats_floats(X.BF16, X.DOWN4, cin, cout, b, h, w)))
    _lib.check(lib.ddimx_downsample_wreg_fwd(cin, cout, xd.ptr, wf.ptr, bd.ptr, y.ptr, stats.ptr, b, h, w, _lib.stream()))
    H.sync()
    what = f"down {cin}->{cout} B={b}"
    for r in (xd, bd, wf):
        r.check(what)
    plan = X.conv_plan(X.BF16, X.DOWN4, cin, cout, b, h, w, DOWN_FLAGS)
    assert plan["family"] == X.WREG
    st = stats.read(what + " statistics", used=b * plan["wgs_per_sample"] * cout * 2)
    assert bool(torch.isfinite(st).all()), what + ": a statistics partial was never written"
    return y.read(what).view(b, h // 2, w // 2, cout), st.view(b, plan["wgs_per_sample"], cout, 2), plan


# ---- Upsample --------------------------------------------------------------------------------------------------------------------------
def _up_operands(cin, cout, h, w):
    tag = f"dus.up.{cin}"
    x = _ints(tag + ".x", (B, cin, h, w), 4)
    k = torch.arange(4)
    cls = (k[:, None] % 2) * 2 + (k[None, :] % 2)           # [kh][kw]: the output parity the tap feeds
    place = (k[:, None] // 2) * 2 + (k[None, :] // 2)
    e = (4 * cls + place).float()                             # 16 different exponents
    assert len(set(e.reshape(-1).tolist())) == 16
    bump = (torch.arange(cin) % 2).float()[:, None, None, None]
    wt = _signs(tag + ".w", (cin, cout, 4, 4)) * torch.exp2(e[None, None] + bump)
    bias = _ints(tag + ".b", (cout,), 4) * 16.0  # on the 2^4 grid: conv + bias < 2^27 + 2^6 stays exact beside the 2^12 grid of class 3
    oy, ox = torch.arange(2 * h), torch.arange(2 * w)
    ocls = ((1 - oy % 2) * 2)[:, None] + (1 - ox % 2)[None, :]  # output (oy, ox) sums the taps kh = oy + 1 mod 2, kw = ox + 1 mod 2
    skip = _ints(tag + ".s", (B, cout, 2 * h, 2 * w), 8) * torch.exp2(4.0 * ocls.float())
    return x, wt, bias, skip


def _up_want(conv, skip):
    """The two roundings of the epilogue: conv + bias stored as bf16, + skip, bf16 again (models/diffusion.py:284 on bf16 tensors)."""
    return (conv.bfloat16().float() + skip).bfloat16().permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("cin,cout", UP_PAIRS)
def test_upsample_exact_every_tap_in_place(cin, cout):
    th, tw = _tile(X.UP4, cin, cout)
    h, w = 2 * th, 2 * tw  # 2 x 2 tiles: every border and a tile seam in both directions; grid.z covers both row parities
    x, wt, bias, skip = _up_operands(cin, cout, h, w)
    # one transposed conv per tap: exact integers on the class grid, so their sum in any order is the whole conv
    parts = torch.stack([F.conv_transpose2d(x, wt * F.one_hot(torch.tensor(t), 16).view(4, 4).float(), None, stride=2, padding=1)
                         for t in range(16)])
    conv = F.conv_transpose2d(x, wt, bias, stride=2, padding=1)
    assert torch.equal(conv, parts.sum(0) + bias[None, :, None, None]), "the operands are not exact in fp32"
    want = _up_want(conv, skip)
    # condition of the test: taking away any ONE tap changes the expected output in the interior and in each border row / column
    # the tap reaches (output row 0 reads kh = 1 and, through the zero padding, kh = 3: a tap does not reach every border)
    Ho, Wo = 2 * h, 2 * w
    reg = torch.zeros(5, Ho, Wo, dtype=torch.bool)
    reg[0, 1:-1, 1:-1] = True
    reg[1, 0], reg[2, -1], reg[3, :, 0], reg[4, :, -1] = True, True, True, True
    for t in range(16):
        reach = (parts[t] != 0).any(1).any(0)                 # [Ho][Wo]: pixels this tap feeds
        without = _up_want(conv - parts[t], skip)
        changed = (without != want).any(-1).any(0)
        for r, name in enumerate(("interior", "top row", "bottom row", "left column", "right column")):
            if bool((reach & reg[r]).any()):
                assert bool((changed & reg[r]).any()), f"tap {divmod(t, 4)} could vanish unnoticed in the {name}"
        assert bool(reach[1:-1, 1:-1].any())
    y, _ = _run_up(cin, cout, x, _up_frag(wt), bias, skip)
    H.same(y, want, f"Upsample {cin}->{cout} against torch's fp32 conv_transpose2d + skip")


def test_upsample_random_data_and_batch_independence():
    """64->32 on random bf16 data with packer-made weights: against fp32 torch on the same operands (the gate of
    test_wreg_upsample_add_vs_fp32_reference), and sample 1 of B = 3 bit for bit what it is alone."""
    cin, cout = 64, 32
    th, tw = _tile(X.UP4, cin, cout)
    h, w = 2 * th, 2 * tw
    x = (synth.gaussian("dus.r.x", (B, cin, h, w)) * 1.1).bfloat16().float()
    skip = synth.gaussian("dus.r.s", (B, cout, 2 * h, 2 * w)).bfloat16().float()
    wt = synth.gaussian("dus.r.w", (cin, cout, 4, 4)) / (4 * cin) ** 0.5
    bias = synth.gaussian("dus.r.b", (cout,)) * 0.3
    wf = _up_frag(wt)
    y, st = _run_up(cin, cout, x, wf, bias, skip)
    want = F.conv_transpose2d(x, wt.bfloat16().float(), bias, stride=2, padding=1) + skip
    mx, rms = G.check_close(y.float().permute(0, 3, 1, 2), want, G.BF16, "wreg up 64->32, random data")
    H.report_std("wreg up 64->32", mx, rms)
    y1, st1 = _run_up(cin, cout, x[1:2], wf, bias, skip[1:2])
    H.same(y1[0], y[1], "Upsample: a sample alone and inside a batch of 3")
    H.same(st1, st.view(B, -1)[1], "Upsample statistics: a sample alone and inside a batch of 3")


# ---- Downsample -----------------------------------------------------------------------------------------------------------------------
def _down_operands(cin, cout, h, w):
    tag = f"dus.down.{cin}"
    x = _ints(tag + ".x", (B, cin, h, w), 4)
    tapw = (torch.arange(16).float() + 1).view(4, 4)                                   # a distinct weight per tap
    grp = torch.exp2(((torch.arange(cin) // 16) % 3).float())[None, :, None, None]     # a pattern over the 16-channel groups
    blk = torch.exp2(((torch.arange(cout) // 32) % 2).float())[:, None, None, None]  # and over the 32-cout blocks
    wt = _signs(tag + ".w", (cout, cin, 4, 4)) * blk * tapw[None, None] * grp
    bias = _ints(tag + ".b", (cout,), 8)
    return x, wt, bias


def _down_frag(wt):
    cout, cin = wt.shape[0], wt.shape[1]
    wd = H.dev32(wt)
    wf = torch.empty(16 * cout * cin, dtype=BF, device=G.dev())
    _lib.check(H.lib().ddimx_pack_conv_frag_k(_lib.ptr(wd), _lib.ptr(wf), cout, cin, 16, _lib.stream()))
    H.sync()
    return H.Ro(wf, BF)


@pytest.mark.parametrize("cin,cout", DOWN_PAIRS)
def test_deep_downsample_exact_statistics_and_batch_independence(cin, cout):
    th, tw = _tile(X.DOWN4, cin, cout)
    h, w = 4 * th, 4 * tw  # the output is 2 x 2 tiles
    x, wt, bias = _down_operands(cin, cout, h, w)
    assert 136 * 4 * 2 * cin * 4 + 8 < 2 ** 24  # sum of the tap weights x group x block pattern x channels x |x|, + bias
    wf = _down_frag(wt)
    y, st, plan = _run_down(cin, cout, x, wf, bias)
    want = F.conv2d(x, wt, bias, stride=2, padding=1).bfloat16().permute(0, 2, 3, 1).contiguous()
    H.same(y, want, f"Downsample {cin}->{cout} against torch's fp32 conv2d")
    # the statistics: per-channel (sum, sum of squares) partials, one per workgroup; the consumer adds a sample's partials in
    # order in fp64 and folds the channels into the 8 groups -- they must be those of the bf16 values as stored
    tot = torch.zeros(B, cout, 2, dtype=torch.float64)
    for p in range(st.shape[1]):
        tot += st[:, p].double()
    got = tot.view(B, 8, cout // 8, 2).sum(2)
    v = y.double().view(B, -1, 8, cout // 8)
    m = plan["th"] * plan["tw"] * plan["tiles_per_wg"]  # terms of one fp32 partial
    for k, f in ((0, lambda a: a), (1, lambda a: a * a)):
        ref, bound = f(v).sum((1, 3)), m * 2.0 ** -24 * f(v).abs().sum((1, 3))
        err = (got[:, :, k] - ref).abs()
        print(f"[down {cin}->{cout} statistic {k}] worst {float((err / (bound + 1e-30)).max()):.2e} of the fp32 summation bound")
        assert bool((err <= bound).all()), f"Downsample {cin}->{cout}: statistic {k} is not that of the stored values ({float(err.max())})"
    y1, st1, _ = _run_down(cin, cout, x[1:2], wf, bias)
    H.same(y1[0], y[1], "Downsample: a sample alone and inside a batch of 3")
    H.same(st1[0], st[1], "Downsample statistics: a sample alone and inside a batch of 3")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_ineligible_shapes_are_refused():
    """The register-streamed entry points refuse what the kernel cannot take (the walk then plans the LDS-ring kernel): an Upsample
    whose Cout is no multiple of 32 (a 32-cout block would straddle the two column parities), and images that are not whole tiles."""
    lib = H.lib()
    one = H.Ro(torch.zeros(1 << 16), BF)
    fl = H.Ro(torch.zeros(1 << 12))
    y, st = H.Out(1 << 16, BF), H.Out(1 << 16)
    H.refused(lib.ddimx_upsample_add_wreg_fwd(64, 48, one.ptr, one.ptr, fl.ptr, one.ptr, y.ptr, st.ptr, 1, 8, 32, _lib.stream()),
              y, st)  # (no kernel of any family has this width: the planner says so)
    H.refused(lib.ddimx_upsample_add_wreg_fwd(64, 32, one.ptr, one.ptr, fl.ptr, one.ptr, y.ptr, st.ptr, 1, 12, 32, _lib.stream()),
              y, st, who="ddimx_upsample_add_wreg_fwd")
    H.refused(lib.ddimx_downsample_wreg_fwd(192, 256, one.ptr, one.ptr, fl.ptr, y.ptr, st.ptr, 1, 12, 16, _lib.stream()),
              y, st, who="ddimx_downsample_wreg_fwd")
