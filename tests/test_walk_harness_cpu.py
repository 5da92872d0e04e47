"""tests/walk_harness.py on the CPU: fake walks in torch make each check fire on the fault it is there for -- a store one byte past
a region's requested size, into a gap, into a guard, a result that depends on a byte the walk never wrote, a `0 * stale` product --
and a clean fake walk passes; then the properties of every layout the library hands out (the library plans on a CPU), over a sweep
of configs, modes, batches and lengths, with and without the carve gap."""
import ctypes

import pytest
import torch

from ddim_audio_amd import _lib, configs
from ddim_audio_amd.model import Model
import kernel_harness as KH
import walk_harness as WH

CPU = torch.device("cpu")
SIZES = [100, 300, 256, 1, 4096 + 7]  # requested bytes: ragged, a whole number of 256, one byte, more than the gap
F, B16 = "torch.FloatTensor", "torch.BFloat16Tensor"


def fake_layout(sizes=SIZES, gap=WH.GAP):
    regions, off = [], 0
    for s in sizes:
        regions.append((off, s))
        off += WH.al256(s) + gap
    return regions, off


def scratch(gap=WH.GAP):
    regions, total = fake_layout(gap=gap)
    WH.check_layout(regions, total, gap, "fake")
    return WH.Scratch(regions, total, device=CPU)


def fake_walk(s, x, stray=None, read=None, times_zero=False):
    """A walk over scratch `s`: writes all of region 0 (x's bytes, repeated), the first half of region 1 and all of region 4, and
    returns a float that depends on what it wrote alone -- unless `read` = (region, byte) names a byte it folds in too, or
    `times_zero` multiplies region 2's first float (never written) by zero.  `stray`: a position (the library's coordinates) that
    gets one byte more."""
    t = s.t
    (o0, n0), (o1, n1), (o2, _), _, (o4, n4) = s.regions
    src = x.view(torch.uint8)
    t[o0:o0 + n0] = src.repeat(n0 // src.numel() + 1)[:n0]
    t[o1:o1 + n1 // 2] = 3
    t[o4:o4 + n4] = 5
    out = t[o0:o0 + n0].float().sum() + t[o1:o1 + n1 // 2].float().sum() + t[o4:o4 + n4].float().sum()
    if read is not None:
        out = out + float(t[s.regions[read[0]][0] + read[1]])
    if times_zero:
        out = out + 0.0 * t[o2:o2 + 4].view(torch.float32)[0]
    if stray is not None:
        s.out.t[KH.GUARD + stray] = 0x42
    return {"out": out.reshape(1)}


def run_of(s, x, **kw):
    def run(pattern):
        s.fill(pattern)
        got = fake_walk(s, x, **kw)
        s.check("fake walk")
        return got
    return run


X = torch.arange(8, dtype=torch.float32)


def test_a_fresh_scratch_and_its_fill():
    s = scratch()
    assert s.t.numel() == s.total and s.t.dtype == torch.uint8 and s.ptr.value == s.out.t.data_ptr() + KH.GUARD
    assert s.out.untouched()
    s.check("fresh")
    for pattern in WH.FILLS:
        s.fill(pattern)
        s.check("filled")  # a fill stays inside the regions
        inside = sum(n for _, n in s.regions)
        if pattern != KH.SENTINEL:
            assert int((s.out.t == pattern).sum()) == inside and int((s.out.t == KH.SENTINEL).sum()) == s.out.t.numel() - inside
    assert bool(torch.isnan(torch.tensor([0xFF] * 4, dtype=torch.uint8).view(torch.float32)))
    big = torch.tensor([0x7F] * 4, dtype=torch.uint8)
    assert float(big.view(torch.float32)) > 3e38 and float(big[:2].view(torch.bfloat16)) > 3e38  # finite and large in both types


def test_a_clean_walk_passes():
    s = scratch()
    first = WH.under_fills(run_of(s, X), "clean")
    assert first["out"].shape == (1,) and bool(torch.isfinite(first["out"]).all())


@pytest.mark.parametrize("region", [0, 1, 3, 4])
def test_one_byte_past_a_regions_requested_size(region):
    """The rounding tail [bytes, al256(bytes)): what the library's own 256-byte alignment would hide."""
    s = scratch()
    off, size = s.regions[region]
    assert size % 256, "this region has a rounding tail"
    with pytest.raises(AssertionError, match=rf"fake walk: 1 bytes outside the regions were written, the first at {off + size}: byte 0 behind region {region} "):
        run_of(s, X, stray=off + size)(0x00)
    s = scratch()
    s.fill(0x00)
    fake_walk(s, X, stray=off + size - 1)  # the region's last byte is the region's
    s.check("last byte")


@pytest.mark.parametrize("region", [0, 2, 4])
def test_one_byte_into_a_gap(region):
    s = scratch()
    off, size = s.regions[region]
    at = off + WH.al256(size) + 10
    with pytest.raises(AssertionError, match=rf"the first at {at}: byte {at - off - size} behind region {region} "):
        run_of(s, X, stray=at)(0x00)
    s = scratch()  # the last byte of the gap: one in front of the next region, or of the high guard
    at = off + WH.al256(size) + WH.GAP - 1
    with pytest.raises(AssertionError, match=rf"behind region {region} "):
        run_of(s, X, stray=at)(0xFF)


def test_one_byte_into_a_guard():
    s = scratch()
    with pytest.raises(AssertionError, match="the first at -1: in the low guard, in front of region 0"):
        run_of(s, X, stray=-1)(0x00)
    s = scratch()
    with pytest.raises(AssertionError, match="in the low guard"):
        run_of(s, X, stray=-KH.GUARD)(0x00)
    for at in (0, KH.GUARD - 1):
        s = scratch()
        with pytest.raises(AssertionError, match=rf"the first at {s.total + at}: byte .* behind region 4 "):
            run_of(s, X, stray=s.total + at)(0x00)


def test_a_stored_sentinel_is_the_one_byte_a_byte_check_cannot_see_and_every_other_is_seen():
    s = scratch()
    s.fill(0x00)
    s.out.t[KH.GUARD + s.regions[0][1]] = 0xFE
    with pytest.raises(AssertionError, match="1 bytes outside"):
        s.check("0xFE")
    s.out.t[KH.GUARD + s.regions[0][1] + 1] = 0x00
    with pytest.raises(AssertionError, match="2 bytes outside"):
        s.check("two")


def test_a_result_that_depends_on_an_unwritten_byte():
    """The second half of region 1, all of region 2 and region 3 are never written by the fake walk."""
    for read in ((1, SIZES[1] - 1), (2, 0), (3, 0)):
        s = scratch()
        with pytest.raises(AssertionError, match="stale: out under fill 0x00 against fill 0xFF: 1 of 1 elements differ"):
            WH.under_fills(run_of(s, X, read=read), "stale")
    s = scratch()
    WH.under_fills(run_of(s, X, read=(1, 0)), "a byte the walk wrote")  # reading what was written is no dependence
    s = scratch()  # the previous call's correct values left in place: what the suite's repeated calls at one shape amount to
    run = run_of(s, X, read=(2, 0))
    s.fill(0x00)
    a = fake_walk(s, X, read=(2, 0))
    b = fake_walk(s, X, read=(2, 0))
    KH.same(a["out"], b["out"])
    with pytest.raises(AssertionError):
        WH.under_fills(run, "stale")


def test_zero_times_stale():
    """0 * x is 0 under the fills 0x00 and 0x7F and NaN under 0xFF: a product is no select."""
    s = scratch()
    with pytest.raises(AssertionError, match="fill 0x00 against fill 0xFF"):
        WH.under_fills(run_of(s, X, times_zero=True), "0 * stale")
    s = scratch()
    WH.under_fills(run_of(s, X, times_zero=True), "0 * stale", fills=(0x00, 0x7F))  # which is why 0xFF is one of the fills


def test_body_and_frozen_and_the_tape_as_an_input():
    o = KH.Out(4, device=CPU)
    o.body.copy_(torch.arange(4.0))
    KH.same(WH.body(o, "out"), torch.arange(4.0))
    o.t[KH.GUARD + 16] = 0
    with pytest.raises(AssertionError, match="out: 1 bytes outside the output"):
        WH.body(o, "out")
    w = torch.arange(6.0)
    f = WH.Frozen(w)
    assert f.t is w
    f.check("weights")
    w[2] = -w[2]
    with pytest.raises(AssertionError, match="weights: a read-only input was written"):
        f.check("weights")
    s = scratch()
    s.fill(0x7F)
    keep = s.snapshot()
    s.unchanged(keep, "tape")
    s.t[s.regions[2][0] + 3] = 0
    with pytest.raises(AssertionError, match="tape: a read-only scratch buffer"):
        s.unchanged(keep, "tape")


def test_inject():
    """A Model takes a Scratch as workspace slot 0 / as its training workspace: a uint8 view of exactly `total` bytes at the body."""
    m = Model(configs.tiny_config(F))
    a, b = scratch(), scratch()
    assert m._workspace is None
    WH.inject(m, workspace=a)
    assert WH.injected(m, workspace=a) and m._workspace[0].numel() == a.total and m._workspace[0].dtype == torch.uint8
    WH.inject(m, train_ws=b, workspace=b, slot=1)
    assert WH.injected(m, workspace=a) and WH.injected(m, workspace=b, train_ws=b, slot=1) and set(m._workspace) == {0, 1}
    m._train_ws = torch.empty(b.total + 1, dtype=torch.uint8)  # what a re-allocation leaves behind
    assert not WH.injected(m, train_ws=b)
    m._workspace[0] = a.out.t[KH.GUARD:KH.GUARD + a.total + 1]
    assert not WH.injected(m, workspace=a)


def test_check_layout_fires():
    regions, total = fake_layout()
    WH.check_layout(regions, total, WH.GAP, "ok")
    WH.check_layout(*fake_layout(gap=0), 0, "ok")
    with pytest.raises(AssertionError, match="does not end at the total"):
        WH.check_layout(regions, total + 256, WH.GAP, "slack at the end")
    with pytest.raises(AssertionError, match="region 4"):
        WH.check_layout(regions, total - 256, WH.GAP, "short")
    with pytest.raises(AssertionError, match="region 0 .* fewer than 4352"):
        WH.check_layout(regions, total, WH.GAP + 256, "a wider gap than carved")
    bad = list(regions)
    bad[2] = (bad[2][0] - 256, bad[2][1])
    with pytest.raises(AssertionError, match="region 1"):
        WH.check_layout(bad, total, WH.GAP, "region 2 starts inside region 1's gap")
    bad = list(regions)
    bad[1] = (bad[1][0] + 16, bad[1][1])
    with pytest.raises(AssertionError):
        WH.check_layout(bad, total, WH.GAP, "unaligned")


# ---- the library's own layouts ------------------------------------------------------------------------------------------------------
MODELS = [(name, tag) for name in ("tiny", "audio") for tag in ("f32", "bf16", "mixed")]
BATCHES = (1, 2, 3, 5, 9, 64)
LONG = (1024, 1056, 4096, 8192)


def _model(name, tag):
    act, fnet = {"f32": (F, None), "bf16": (B16, None), "mixed": (B16, F)}[tag]
    m = Model((configs.tiny_config if name == "tiny" else configs.audio_config)(act, fnet))
    return m, m._ensure_handle()


def _exports(lib):
    return {WH.WORKSPACE: lib.ddimx_workspace_bytes, WH.TRAIN_WORKSPACE: lib.ddimx_train_workspace_bytes, WH.TAPE: lib.ddimx_train_tape_bytes}


@pytest.mark.parametrize("name, tag", MODELS, ids=[f"{n}-{t}" for n, t in MODELS])
def test_layout_sweep(name, tag):
    """Every legal T up to 256 and four long ones, six batches, the three layouts: in order, disjoint, 256-aligned, ending at the
    total, the total what the *_bytes export says; with gap 0 each region starts where the one before ends rounded up to 256 (the
    carver of before the gap knob); with gap g the same regions, each g further apart."""
    m, lib = _model(name, tag)
    step = 1 << (len(m.config.ch) - 1)
    lengths = list(range(step, 257, step)) + list(LONG)
    assert all(t % step == 0 for t in lengths)
    g = WH.GAP
    for which, export in _exports(lib).items():
        for B in BATCHES:
            plain = {}
            for T in lengths:
                what = f"{name} {tag} layout {which} B={B} T={T}"
                regions, total = WH.layout(m._handle, which, B, T)
                WH.check_layout(regions, total, 0, what)
                assert total == export(m._handle, B, T), what
                at = 0
                for off, size in regions:
                    assert off == at and size > 0, what
                    at += WH.al256(size)
                plain[T] = regions
            with WH.carve_gap(g):
                for T in lengths:
                    what = f"{name} {tag} layout {which} B={B} T={T} gap {g}"
                    regions, total = WH.layout(m._handle, which, B, T, g)
                    WH.check_layout(regions, total, g, what)
                    assert total == export(m._handle, B, T), what
                    assert regions == [(off + i * g, size) for i, (off, size) in enumerate(plain[T])], what
            assert WH.layout(m._handle, which, B, lengths[0])[0] == plain[lengths[0]]


def test_op_layout_sweep():
    lib = KH.lib()
    g = WH.GAP
    for dt in (_lib.DDIMX_F32, _lib.DDIMX_BF16):
        for B in (1, 3):
            for C, Cb in ((32, 32), (64, 32), (96, 64), (128, 96), (192, 128), (256, 192)):
                for H, W in ((8, 8), (20, 12), (64, 32), (132, 256)):
                    totals = {WH.OP_RESBLOCK: lib.ddimx_op_workspace_bytes(dt, B, C, H, W),
                              WH.OP_RESBLOCK_BWD: lib.ddimx_resblock_bwd_workspace_bytes(dt, B, C, H, W),
                              WH.OP_DOWNUP_BWD: lib.ddimx_downup_bwd_workspace_bytes(dt, C, Cb, B, H, W)}
                    for which, want in totals.items():
                        what = f"op layout {which} dt={dt} B={B} C={C} {H}x{W}"
                        regions, total = WH.op_layout(which, dt, B, C, Cb, H, W)
                        WH.check_layout(regions, total, 0, what)
                        assert total == want and len(regions) == {WH.OP_RESBLOCK: 6, WH.OP_RESBLOCK_BWD: 7, WH.OP_DOWNUP_BWD: 3}[which], what
                        with WH.carve_gap(g):
                            spaced, total_g = WH.op_layout(which, dt, B, C, Cb, H, W, g)
                            WH.check_layout(spaced, total_g, g, what)
                            assert spaced == [(off + i * g, size) for i, (off, size) in enumerate(regions)] and total_g == want + len(regions) * g


def test_the_gap_knob_and_the_export_refuse_and_reset():
    lib = KH.lib()
    m, _ = _model("tiny", "f32")
    before = lib.ddimx_workspace_bytes(m._handle, 2, 16)
    for bad in (-256, -1, 1, 255, 4097):
        assert lib.ddimx_debug_set_carve_gap(bad) != 0 and b"ddimx_debug_set_carve_gap" in lib.ddimx_last_error()
        assert lib.ddimx_workspace_bytes(m._handle, 2, 16) == before  # a refused value changes nothing
    with pytest.raises(RuntimeError):
        with WH.carve_gap(512):
            assert lib.ddimx_workspace_bytes(m._handle, 2, 16) == before + 512 * len(WH.layout(m._handle, WH.WORKSPACE, 2, 16)[0])
            raise RuntimeError("the block fails")
    assert lib.ddimx_workspace_bytes(m._handle, 2, 16) == before  # ... and the gap is 0 again
    n = ctypes.c_int(-1)
    for which in (-1, 3):
        assert lib.ddimx_debug_layout(m._handle, which, 2, 16, None, None, 0, ctypes.byref(n)) != 0 and b"ddimx_debug_layout" in lib.ddimx_last_error()
    assert lib.ddimx_debug_layout(m._handle, WH.TAPE, 2, 18, None, None, 0, ctypes.byref(n)) != 0  # T no multiple of 4
    assert lib.ddimx_debug_layout(m._handle, WH.TAPE, 0, 16, None, None, 0, ctypes.byref(n)) != 0
    assert lib.ddimx_debug_layout(None, WH.TAPE, 2, 16, None, None, 0, ctypes.byref(n)) != 0
    assert lib.ddimx_debug_layout(m._handle, WH.TAPE, 2, 16, None, None, 0, None) != 0
    assert lib.ddimx_debug_layout(m._handle, WH.TAPE, 2, 16, None, None, 4, ctypes.byref(n)) != 0  # room for four, no arrays
    assert lib.ddimx_debug_op_layout(3, 0, 1, 32, 32, 8, 8, None, None, 0, ctypes.byref(n)) != 0 and b"ddimx_debug_op_layout" in lib.ddimx_last_error()
    off, size = (ctypes.c_longlong * 4)(*[-7] * 4), (ctypes.c_longlong * 4)(*[-7] * 4)
    assert lib.ddimx_debug_layout(m._handle, WH.TAPE, 2, 16, off, size, 3, ctypes.byref(n)) == 0  # a short array: the first three, the full count
    assert n.value == len(WH.layout(m._handle, WH.TAPE, 2, 16)[0]) > 3 and off[3] == size[3] == -7 and off[0] == 0 and off[2] > off[1] > 0


def test_setting_the_gap_back_restores_the_plan_dump():
    """tests/plan_dump.py's rows before, under and after a gap: the byte rows grow under it and nothing else moves; afterwards every
    row is what it was."""
    import plan_dump
    before = plan_dump.dump()
    with WH.carve_gap():
        under = plan_dump.dump()
    after = plan_dump.dump()
    assert after == before
    assert under.keys() == before.keys()
    moved = {k for k in before if under[k] != before[k]}
    rows = {k for k in before if k.startswith("bytes:")}
    assert moved == rows and len(rows) == 8
    assert all(u > b for k in rows for u, b in zip(under[k], before[k]))
