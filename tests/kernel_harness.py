"""What the per-kernel GPU tests (test_gpu_gn_kernels, _tail_kernels, _fnet_kernels, _fnet_dense, _temb_step_pack, _edge_kernels) share: guarded
output buffers, read-only inputs with a bit snapshot, inputs placed in padded layouts, one bit comparison, one refusal check and the
lines the gated tests print.  tests/test_kernel_harness_cpu.py runs every check of this module against the ways it could be fooled.

The sentinel is the byte 0xFF: four of them are a NaN in fp32, two in bf16, so scratch "is NaN before each call" and padding that
is read poisons the result, and -- unlike an isnan test -- a byte comparison also sees a stray store of a NaN."""
import ctypes

import numpy as np
import torch

from ddim_audio_amd import _lib
import gpu_util as G

GUARD = 4096  # bytes on either side of every output; a multiple of 16, so the body keeps the allocation's alignment
SENTINEL = 0xFF
NAN = float("nan")


def lib():
    return _lib.load()


def sync():
    torch.cuda.synchronize()


def dev(a, dtype=None):
    """`a` (numpy, list or tensor) on the GPU, contiguous, in its own dtype unless one is given."""
    t = torch.as_tensor(a)
    return t.to(G.dev(), dtype or t.dtype).contiguous()


def dev32(a):
    """`a` on the GPU as fp32 (the fp64 references hand out fp32 numbers held in fp64)."""
    return dev(a, torch.float32)


class Out:
    """An output of `n` elements of `dtype` inside an allocation whose every byte is SENTINEL, GUARD bytes on either side of the
    body.  With `idx` (flat element positions, any shape) the logical elements lie at those positions of a body of max(idx) + 1
    elements and every other byte of it is padding.  `init`: what the logical elements hold when a kernel updates them in place."""

    def __init__(self, n=None, dtype=torch.float32, *, init=None, idx=None, device=None):
        device = G.dev() if device is None else device
        self.dtype, self.es = dtype, dtype.itemsize
        self.shape = (n,) if idx is None else tuple(idx.shape)
        self.n = n if idx is None else idx.numel()
        self.idx = None if idx is None else idx.reshape(-1).to(device)
        self.nbytes = (n if idx is None else int(idx.max()) + 1) * self.es
        self.t = torch.full((self.nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=device)
        if init is not None:
            v = torch.as_tensor(init).to(dtype).reshape(-1).to(device)
            if idx is None:
                self.body.copy_(v)
            else:
                self.body[self.idx] = v

    @property
    def body(self):
        """The body as a device tensor of `dtype` (a view)."""
        return self.t[GUARD:GUARD + self.nbytes].view(self.dtype)

    @property
    def addr(self):
        return self.t.data_ptr() + GUARD

    @property
    def ptr(self):
        return ctypes.c_void_p(self.addr)

    def _logical(self, used):
        return slice(0, used) if self.idx is None else self.idx[:used]

    def read(self, what, used=None):
        """The logical elements (in the shape of `idx`), or the first `used` of them, on the CPU; asserts that every other byte of
        the allocation -- both guards, the unused tail, the padding between the logical elements -- still is SENTINEL."""
        used = self.n if used is None else used
        stray = (self.t != SENTINEL).view(-1, self.es)  # [element][byte], the low guard's elements first
        stray[GUARD // self.es:][self._logical(used)] = False
        stray = int(stray.sum())
        assert stray == 0, f"{what}: {stray} bytes outside the output were written"
        got = self.body[self._logical(used)].cpu()
        return got.view(self.shape) if used == self.n else got

    def untouched(self):
        return bool((self.t == SENTINEL).all())


class Ro:
    """A read-only input on the device with a snapshot of its bits."""

    def __init__(self, a, dtype=torch.float32, device=None):
        self.t = torch.as_tensor(a).to(G.dev() if device is None else device, dtype, copy=True).contiguous()
        self.keep = self.t.clone()

    @property
    def addr(self):
        return self.t.data_ptr()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.addr)

    def check(self, what):
        assert torch.equal(self.t.view(torch.uint8), self.keep.view(torch.uint8)), f"{what}: a read-only input was written"


def placed(values, idx, offset=0, size=None, dtype=torch.float32, device=None):
    """An INPUT in a strided or padded layout: `values` at the flat positions `idx` of `size` elements (default: max(idx) + 1), NaN
    everywhere else, so that a kernel that reads padding poisons its output.  The tensor returned starts `offset` elements past a
    16-byte boundary; its pointer is _lib.ptr(tensor)."""
    size = int(idx.max()) + 1 if size is None else size
    assert int(idx.max()) < size
    buf = torch.full((offset + size,), NAN, dtype=dtype)
    buf[idx.reshape(-1) + offset] = values.reshape(-1).float().to(dtype)
    return buf.to(G.dev() if device is None else device)[offset:]


_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def same(got, want, what="bit for bit"):
    """Asserts that two arrays (numpy or torch) have one dtype, one shape and the same bits in every element."""
    got, want = (torch.as_tensor(a).contiguous() for a in (got, want))
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    got, want = (a.view(_INT[a.element_size()]) for a in (got, want))
    if not torch.equal(got, want):
        bad = (got != want).reshape(-1)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, the first at {int(bad.nonzero()[0])}")


def refused(rc, *outs, who=None):
    """A refused call: non-zero, a message (one that contains `who`, if given: the export or the launcher), nothing written."""
    sync()
    msg = lib().ddimx_last_error().decode(errors="replace")
    assert rc != 0 and msg and (who is None or who in msg), (rc, msg, who)
    assert all(o.untouched() for o in outs), f"{who or 'a refused call'} wrote to its outputs"


# ---- what the gated tests print ----------------------------------------------------------------------------------------------------------
def report(what, worst, unit="of the gate"):
    print(f"[{what}] worst {worst:.2e} {unit}")


def report_std(what, mx, rms):
    print(f"[{what}] max {mx:.2e} rms {rms:.2e} of std")


def report_gate(what, mx, rms):
    print(f"[{what}] worst max {mx / G.TOL[G.F32]['mx']:.2e}, rms {rms / G.TOL[G.F32]['rms']:.2e} of the gate")


class Worst:
    """The worst (max, rms) of a test's G.check_close calls, in units of the F32 gate."""

    def __init__(self):
        self.mx = self.rms = 0.0

    def close(self, got, want, what):
        want = torch.as_tensor(np.asarray(want), dtype=torch.float64).reshape(-1)
        got = torch.as_tensor(np.asarray(got), dtype=torch.float64).reshape(-1)
        if want.numel() == 1:  # one number has no spread: its own magnitude takes the place of the standard deviation in the gate
            assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
            mx = rms = float((got - want).abs()) / (float(want.abs()) + 1e-30)
            tol = G.TOL[G.F32]
            assert mx <= tol["mx"] and rms <= tol["rms"], f"{what}: {mx:.3e} (rel. to the value) exceeds {tol}"
        else:
            mx, rms = G.check_close(got, want, G.F32, what)
        self.mx, self.rms = max(self.mx, mx), max(self.rms, rms)
