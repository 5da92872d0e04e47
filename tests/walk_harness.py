"""What tests/test_gpu_walk_scratch.py needs to run a whole walk of the library (a network forward, a training pair, an FNet, a per-op
block) inside scratch whose every byte is accounted for: the region table the walk's own carver reports (ddimx_debug_layout), a
buffer of exactly the layout's size between guards, with a gap of unused bytes behind every region (ddimx_debug_set_carve_gap), the
three fill patterns, and the two checks -- containment (nothing outside the regions' requested bytes is written) and independence
(the outputs are the same bits whatever the scratch held before).  Built on kernel_harness; tests/test_walk_harness_cpu.py runs
every check against the fault it is there for, and the layout's properties over a sweep of shapes.

The sentinel of gaps, rounding tails and guards is kernel_harness's 0xFF.  The fills of the regions themselves: 0xFF (a NaN in fp32
and bf16), 0x00 (zeros: what a `0 * stale` product survives) and 0x7F (3.39e38 in fp32, 3.39e38 in bf16: finite, so a maximum, a
comparison or a select on it behaves unlike one on a NaN, and large enough that any sum it enters overflows or drowns the rest)."""
import contextlib
import ctypes

import torch

from ddim_audio_amd import _lib
import kernel_harness as KH

GAP = 4096  # the carve gap of the GPU runs: a page, more than any rounding tail and a multiple of 256
FILLS = (0xFF, 0x00, 0x7F)
WORKSPACE, TRAIN_WORKSPACE, TAPE = _lib.DDIMX_LAYOUT_WORKSPACE, _lib.DDIMX_LAYOUT_TRAIN_WORKSPACE, _lib.DDIMX_LAYOUT_TAPE
OP_RESBLOCK, OP_RESBLOCK_BWD, OP_DOWNUP_BWD = _lib.DDIMX_OP_LAYOUT_RESBLOCK, _lib.DDIMX_OP_LAYOUT_RESBLOCK_BWD, _lib.DDIMX_OP_LAYOUT_DOWNUP_BWD


def al256(n):
    return (n + 255) & ~255


@contextlib.contextmanager
def carve_gap(gap=GAP):
    """Inside the block every layout of the library has `gap` unused bytes behind each region; afterwards it is 0 again, whatever
    happened inside."""
    lib = KH.lib()
    _lib.check(lib.ddimx_debug_set_carve_gap(gap))
    try:
        yield
    finally:
        _lib.check(lib.ddimx_debug_set_carve_gap(0))


def _regions(call):
    n = ctypes.c_int()
    _lib.check(call(None, None, 0, ctypes.byref(n)))
    off, size = (ctypes.c_longlong * n.value)(), (ctypes.c_longlong * n.value)()
    cap = n.value
    _lib.check(call(off, size, cap, ctypes.byref(n)))
    assert n.value == cap
    return list(zip(off, size))


def _total(regions, gap):
    off, size = regions[-1]
    return off + al256(size) + gap


def layout(handle, which, B, T, gap=0):
    """([(offset, requested bytes)] in carve order, total bytes) of the inference workspace, the training workspace or the tape
    of a model's handle at (B, T), under the carve gap that is set now (`gap` says which: the total follows from it)."""
    lib = KH.lib()
    regions = _regions(lambda *a: lib.ddimx_debug_layout(handle, which, B, T, *a))
    return regions, _total(regions, gap)


def op_layout(which, dtype, B, C, Cbig, H, W, gap=0):
    """The same for the per-op workspaces (ddimx_op_workspace_bytes, ddimx_resblock_bwd_workspace_bytes,
    ddimx_downup_bwd_workspace_bytes: C, H, W the small side, Cbig the big side's channels)."""
    lib = KH.lib()
    regions = _regions(lambda *a: lib.ddimx_debug_op_layout(which, dtype, B, C, Cbig, H, W, *a))
    return regions, _total(regions, gap)


def check_layout(regions, total, gap, what):
    """The properties every layout has: regions in order, disjoint, 256-aligned, each followed by at least `gap` bytes that belong
    to no region, the last one (with its rounding and its gap) ending exactly at `total`."""
    assert regions and regions[0][0] == 0, what
    for i, (off, size) in enumerate(regions):
        assert off % 256 == 0 and size >= 0, (what, i, off, size)
        end = regions[i + 1][0] if i + 1 < len(regions) else total
        assert off + al256(size) + gap <= end, f"{what}: region {i} [{off}, +{size}) is followed by fewer than {gap} free bytes (next at {end})"
    assert regions[-1][0] + al256(regions[-1][1]) + gap == total, f"{what}: the last region does not end at the total {total}"


class Scratch:
    """A workspace or tape of exactly `total` bytes (a kernel_harness.Out of uint8: guards on either side) with its region table.
    Fresh, every byte is the sentinel."""

    def __init__(self, regions, total, device=None):
        self.regions, self.total = list(regions), total
        self.out = KH.Out(total, torch.uint8, device=device)

    @property
    def t(self):
        """The buffer as the library sees it: a uint8 view of exactly `total` bytes."""
        return self.out.body

    @property
    def ptr(self):
        return self.out.ptr

    def fill(self, pattern):
        """Every byte a region asked for = `pattern`; gaps, rounding tails and guards are left as they are (the sentinel)."""
        body = self.out.body
        for off, size in self.regions:
            body[off:off + size] = pattern
        return self

    def _outside(self):
        """[(start, end, index of the region in front or -1)] of the allocation's bytes that belong to no region, allocation offsets."""
        g, segs, at, front = KH.GUARD, [], 0, -1
        for i, (off, size) in enumerate(self.regions):
            if g + off > at:
                segs.append((at, g + off, front))
            at, front = g + off + size, i
        segs.append((at, self.out.t.numel(), front))
        return segs

    def check(self, what):
        """Both guards, every gap between regions and every rounding tail [bytes, al256(bytes)) still hold the sentinel."""
        segs = self._outside()
        flat = torch.cat([self.out.t[a:b] for a, b, _ in segs])
        bad = (flat != KH.SENTINEL).nonzero()
        if bad.numel() == 0:
            return
        first, count = int(bad[0]), int(bad.numel())
        for a, b, front in segs:
            if first < b - a:
                pos = a + first - KH.GUARD  # in the library's coordinates
                break
            first -= b - a
        if front < 0:
            where = "in the low guard, in front of region 0"
        else:
            off, size = self.regions[front]
            where = f"byte {pos - (off + size)} behind region {front} [{off}, +{size})"
        raise AssertionError(f"{what}: {count} bytes outside the regions were written, the first at {pos}: {where}")

    def snapshot(self):
        return self.out.t.clone()

    def unchanged(self, keep, what):
        assert torch.equal(self.out.t, keep), f"{what}: a read-only scratch buffer (the tape during the backward) was written"


class Frozen:
    """A device tensor the walks read through its OWN pointer (the packed weights, a table), with a snapshot of its bits."""

    def __init__(self, t):
        self.t, self.keep = t, t.clone()

    def check(self, what):
        assert torch.equal(self.t.view(torch.uint8), self.keep.view(torch.uint8)), f"{what}: a read-only input was written"


def inject(model, workspace=None, train_ws=None, slot=0):
    """Hands a Model its scratch: `workspace` (a Scratch) becomes inference workspace `slot`, `train_ws` the training workspace.
    Model.reserve and the training node keep a buffer whose numel() is not below the need, so one of exactly the needed size stays
    (the caller asserts that afterwards: `injected`).  The tape cannot be injected: the training node allocates it per forward."""
    if workspace is not None:
        model._workspace = dict(model._workspace or {})
        model._workspace[slot] = workspace.t
    if train_ws is not None:
        model._train_ws = train_ws.t


def injected(model, workspace=None, train_ws=None, slot=0):
    """The Model still runs on the scratch it was handed (it did not re-allocate)."""
    ok = workspace is None or (model._workspace[slot].data_ptr() == workspace.out.addr and model._workspace[slot].numel() == workspace.total)
    return ok and (train_ws is None or (model._train_ws.data_ptr() == train_ws.out.addr and model._train_ws.numel() == train_ws.total))


def body(o, what):
    """The body of a kernel_harness.Out as a device tensor of its own (no trip to the host), after asserting that both guards
    still hold the sentinel."""
    g = KH.GUARD
    stray = int((o.t[:g] != KH.SENTINEL).sum()) + int((o.t[g + o.nbytes:] != KH.SENTINEL).sum())
    assert stray == 0, f"{what}: {stray} bytes outside the output were written"
    return o.body.clone()


def under_fills(run, what, fills=FILLS):
    """`run(pattern)` fills its scratch with `pattern`, runs the walk, makes its containment checks and returns {name: tensor}.
    Asserts that every output has the same bits under every fill; returns the outputs of the first."""
    first = None
    for pattern in fills:
        got = run(pattern)
        if first is None:
            first = got
            continue
        assert got.keys() == first.keys()
        for name in first:
            KH.same(got[name], first[name], f"{what}: {name} under fill 0x{pattern:02X} against fill 0x{fills[0]:02X}")
    return first
