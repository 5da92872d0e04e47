"""tests/kernel_harness.py on the CPU: every check the per-kernel GPU tests lean on, against the ways it could be fooled -- a stray
store of a NaN, a store into padding, a lost sign of zero, another NaN payload, a refusal without a message."""
import numpy as np
import pytest
import torch

import kernel_harness as H

CPU = torch.device("cpu")
F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64
QNAN = {F32: [0x00, 0x00, 0xC0, 0x7F], BF16: [0xC0, 0x7F]}  # the bytes of torch's own NaN, little-endian


def out(n=None, dtype=F32, **kw):
    return H.Out(n, dtype, device=CPU, **kw)


def poke(o, at, byte=0x00):
    """One byte of the allocation, `at` bytes from the start of the body (negative: in the low guard)."""
    o.t[H.GUARD + at] = byte


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_a_fresh_buffer_is_untouched_and_reads_as_nan(dtype):
    o = out(5, dtype)
    assert o.untouched()
    got = o.read("fresh")
    assert got.shape == (5,) and got.dtype == dtype and bool(torch.isnan(got).all())
    assert o.addr == o.t.data_ptr() + H.GUARD and o.ptr.value == o.addr and H.GUARD % 16 == 0


@pytest.mark.parametrize("dtype", [F32, BF16, I64])
def test_the_whole_body_and_nothing_else(dtype):
    o = out(7, dtype)
    want = torch.arange(-3, 4).to(dtype)
    o.body.copy_(want)
    H.same(o.read("body"), want)
    assert not o.untouched()


@pytest.mark.parametrize("at", [-1, -4095, 12, 12 + 4094], ids=["low-1", "low-4095", "high-1", "high-4095"])
def test_one_byte_in_a_guard(at):
    """1 and 4095 bytes from either end of a body of 3 floats (12 bytes)."""
    o = out(3)
    o.body.zero_()
    poke(o, at)
    with pytest.raises(AssertionError, match="guarded: 1 bytes outside"):
        o.read("guarded")
    assert not o.untouched()


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("low", [True, False])
def test_a_quiet_nan_stored_into_a_guard(dtype, low):
    """What an isnan test of the guard cannot see."""
    o = out(4, dtype)
    o.body.zero_()
    q = QNAN[dtype]
    at = -len(q) if low else o.nbytes
    for k, b in enumerate(q):
        poke(o, at + k, b)
    assert bool(torch.isnan(o.t[H.GUARD + at:H.GUARD + at + len(q)].view(dtype)).all()), "what was stored is a NaN"
    with pytest.raises(AssertionError, match=f"{len(q)} bytes outside"):
        o.read("nan store")


def test_read_used():
    o = out(6)
    o.body[:3] = 1.0
    H.same(o.read("used", used=3), torch.ones(3))
    with pytest.raises(AssertionError, match="4 bytes outside"):
        o.read("used", used=2)
    o.body[3] = 2.0  # element k = 3 written
    with pytest.raises(AssertionError, match="4 bytes outside"):
        o.read("used", used=3)


def test_idx_form_padding_and_init():
    """Two rows of three elements, five apart: the elements 3, 4 are a hole, and the body ends with the last logical element."""
    idx = torch.arange(2)[:, None] * 5 + torch.arange(3)[None, :]
    init = torch.arange(6.0).view(2, 3)
    o = out(idx=idx, init=init)
    assert o.n == 6 and o.nbytes == 8 * 4 and not o.untouched()
    flat = o.body.clone()
    assert torch.equal(flat[idx], init) and bool((o.t[H.GUARD + 12:H.GUARD + 20] == H.SENTINEL).all())
    got = o.read("rows")
    assert got.shape == (2, 3)
    H.same(got, init)
    o.body[idx] = -init  # the logical positions
    H.same(o.read("rows"), -init)
    o.body[4] = 0.0  # the hole
    with pytest.raises(AssertionError, match="hole: 4 bytes outside"):
        o.read("hole")
    o = out(idx=idx, dtype=BF16)
    o.t[H.GUARD + 2 * 3] = 0x7F  # one byte of the bf16 hole
    with pytest.raises(AssertionError, match="1 bytes outside"):
        o.read("hole")


@pytest.mark.parametrize("at", [-H.GUARD, -1, 0, 7, 8, 8 + H.GUARD - 1])
def test_untouched_sees_any_single_byte(at):
    o = out(2)
    poke(o, at, 0xFE)
    assert not o.untouched()


def test_ro():
    r = H.Ro(np.array([0.0, 1.5, -2.0], np.float32), device=CPU)
    r.check("unchanged")
    assert r.ptr.value == r.addr == r.t.data_ptr()
    r.t.view(torch.int32)[1] ^= 1  # the lowest bit of 1.5
    with pytest.raises(AssertionError, match="flipped: a read-only input was written"):
        r.check("flipped")
    r = H.Ro([0.0, 1.0], device=CPU)
    r.t[0] = -0.0
    assert bool((r.t == r.keep).all())
    with pytest.raises(AssertionError):
        r.check("the sign of zero")
    r = H.Ro([0, 999], I64, device=CPU)
    assert r.t.dtype == I64
    r.check("int64")
    a = np.ones(3, np.float32)
    r = H.Ro(a, device=CPU)
    a[0] = 5.0  # the snapshot and the tensor are copies
    assert float(r.t[0]) == 1.0
    r.check("a copy")


def test_placed():
    idx = torch.arange(2)[:, None] * 4 + torch.arange(3)[None, :]
    v = torch.arange(1.0, 7.0, dtype=torch.float64).view(2, 3)
    t = H.placed(v, idx, device=CPU)
    assert t.dtype == F32 and t.numel() == 7 and torch.equal(t[idx], v.float()) and bool(torch.isnan(t[3]))
    t = H.placed(v, idx, offset=3, size=10, dtype=BF16, device=CPU)
    assert t.dtype == BF16 and t.numel() == 10 and t.storage_offset() == 3 and torch.equal(t[idx], v.bfloat16())
    assert int(torch.isnan(t).sum()) == 4
    with pytest.raises(AssertionError):
        H.placed(v, idx, size=6, device=CPU)


def _nan(payload):
    return torch.tensor([0x7FC00000 | payload], dtype=torch.int32).view(F32)


def test_same():
    a = torch.tensor([[1.0, 2.0], [3.0, 4.0]])
    H.same(a, a.clone())
    H.same(a.numpy(), a)  # numpy against torch
    H.same(np.float32(1.5), np.float32(1.5))
    H.same(a.T, a.T.contiguous())
    for dtype in (BF16, I64, torch.float64, torch.uint8):
        H.same(a.to(dtype), a.to(dtype))
    H.same(_nan(5), _nan(5))
    with pytest.raises(AssertionError):
        H.same(a, a.double())  # dtype
    with pytest.raises(AssertionError):
        H.same(a, a.reshape(-1))  # shape
    with pytest.raises(AssertionError, match="zero: 1 of 2 elements differ, the first at 1"):
        H.same(torch.tensor([0.0, 0.0]), torch.tensor([0.0, -0.0]), "zero")
    with pytest.raises(AssertionError, match="1 of 1 elements differ, the first at 0"):
        H.same(_nan(5), _nan(6))
    b = a.clone()
    b[0, 1], b[1, 1] = 2.5, 0.0
    with pytest.raises(AssertionError, match="2 of 4 elements differ, the first at 1"):
        H.same(a, b)
    with pytest.raises(AssertionError, match="1 of 2 elements differ, the first at 1"):
        H.same(torch.tensor([1.0, 1.0]).bfloat16(), torch.tensor([1.0, 1.0078125]).bfloat16())


class _Stub:
    def __init__(self, msg):
        self.msg = msg

    def ddimx_last_error(self):
        return self.msg


@pytest.fixture
def last_error(monkeypatch):
    """Puts a stub with a chosen ddimx_last_error() in place of the library (and nothing in place of the device synchronisation)."""
    monkeypatch.setattr(H, "sync", lambda: None)

    def set_(msg):
        monkeypatch.setattr(H, "lib", lambda: _Stub(msg))
    return set_


def test_refused(last_error):
    o = out(4)
    last_error(b"ddimx_qsample: B must be positive")
    H.refused(1, o)
    H.refused(-3, o, who="ddimx_qsample")
    H.refused(1)
    with pytest.raises(AssertionError):
        H.refused(0, o)  # accepted
    with pytest.raises(AssertionError):
        H.refused(1, o, who="ddimx_sqerr_loss")  # another export's message
    last_error(b"")
    with pytest.raises(AssertionError):
        H.refused(1, o)  # no message
    last_error(b"ddimx_qsample: B must be positive")
    p = out(4)
    poke(p, 5)
    with pytest.raises(AssertionError, match="wrote to its outputs"):
        H.refused(1, o, p)


def test_the_printed_lines(capsys):
    H.report("a", 0.5)
    H.report("a", 0.25, "of the summation bound")
    H.report_std("b", 1e-6, 2e-7)
    H.report_gate("c", 1e-5, 2e-6)
    assert capsys.readouterr().out.splitlines() == [
        "[a] worst 5.00e-01 of the gate", "[a] worst 2.50e-01 of the summation bound", "[b] max 1.00e-06 rms 2.00e-07 of std",
        "[c] worst max 1.00e-01, rms 1.00e-01 of the gate"]
