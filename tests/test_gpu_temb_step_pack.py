"""The kernels of csrc/pack_kernels.hip, temb_kernels.hip and step_kernels.hip one by one through their own C-ABI entry points, against
the references of tests/temb_step_pack_ref.py.

Every output lives inside an allocation whose bytes are all 0xFF (a NaN in fp32 and in bf16) with guard bands that must still be 0xFF
afterwards (``Out`` of tests/kernel_harness.py).  Packing, layout conversion, the table lookup, the step counter kernels and
ddpm_update are compared bit for bit; ddim_update at the gate of test_gpu_ops.py::test_ddim_update_matches_oracle_bitwise; the four
dense kernels of the embedding MLP, which sum in fp32 in an order of their own, at G.check_close(.., G.F32) against float64, and they
print their worst error in units of it."""
import ctypes
import time

import numpy as np
import pytest
import torch

from ddim_audio_amd import _lib, configs, schedule
import gpu_util as G
from kernel_harness import GUARD, SENTINEL, Out, Worst, dev, lib as L, refused, report_gate as report, same, sync
import step_math_ref as SM
import temb_step_pack_ref as P
from tail_kernel_ref import alphas, gauss, rng

pytestmark = pytest.mark.gpu
DTS = [G.F32, G.BF16]
DT_IDS = ["f32", "bf16"]


def cast(ref, dt):
    """A reference in the destination dtype: fp32 as it is, bf16 rounded to nearest even."""
    return P.bf16(ref) if dt == G.BF16 else ref.to(torch.float32)


def weights(tag, shape):
    """Gaussian fp32 weights; every third one is put exactly between two bf16 neighbours (the low half 0x8000), so that a rounding
    other than to nearest even shows in about a sixth of the elements."""
    w = gauss(tag, shape).reshape(-1).view(np.int32).copy()
    w[::3] = (w[::3] & ~0xFFFF) | 0x8000
    return torch.from_numpy(w.view(np.float32).reshape(shape))


# =========================================================================================================================================
# single-launch packing and layout
# =========================================================================================================================================
CONV_SHAPES = [(3, 2, 3, 3), (32, 16, 3, 3), (5, 7, 4, 4), (2, 64, 3, 3), (256, 256, 3, 3)]  # the last: 2304 blocks > the 2048 cap


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pack_conv(shape, dt):
    O, I, KH, KW = shape
    w = weights(f"pc.{shape}", shape)
    dst = Out(w.numel(), G.TORCH_DT[dt])
    wd = dev(w)
    _lib.check(L().ddimx_pack_conv(dt, _lib.ptr(wd), dst.ptr, O, I, KH, KW, _lib.stream()))
    sync()
    same(dst.read("pack_conv"), cast(P.pack_conv(w), dt).reshape(-1), "pack_conv")


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("I, O", [(2, 3), (16, 32), (7, 5), (160, 144)])  # the last: 24 * 160 * 144 elements = 2160 blocks > 2048
def test_pack_convT(I, O, dt):
    w = weights(f"pct.{I}.{O}", (I, O, 4, 4))
    dst = Out(24 * O * I, G.TORCH_DT[dt])
    wd = dev(w)
    _lib.check(L().ddimx_pack_convT(dt, _lib.ptr(wd), dst.ptr, I, O, _lib.stream()))
    sync()
    got = dst.read("pack_convT")
    zero = P.convT_zero_mask(I, O).reshape(-1)
    assert int(zero.sum()) == 8 * O * I
    assert bool((P.bits(got)[zero] == 0).all()), "kernel columns outside 0..3 must be packed as +0"
    assert bool((P.bits(got)[~zero] != 0).all()), "a real kernel element was packed as zero"
    same(got, cast(P.pack_convT(w), dt).reshape(-1), "pack_convT")


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("O, I", [(3, 2), (32, 16), (5, 7), (2, 64)])
def test_pack_conv_dgrad(O, I, dt):
    w = weights(f"pcd.{O}.{I}", (O, I, 3, 3))
    dst = Out(9 * O * I, G.TORCH_DT[dt])
    wd = dev(w)
    _lib.check(L().ddimx_pack_conv_dgrad(dt, _lib.ptr(wd), dst.ptr, O, I, _lib.stream()))
    sync()
    same(dst.read("pack_conv_dgrad"), cast(P.pack_conv_dgrad(w), dt).reshape(-1), "pack_conv_dgrad")


FRAG_SHAPES = [(32, 16, 9), (64, 96, 9), (96, 64, 16)]


def _frag_weights(O, I, KK):
    return weights(f"frag.{O}.{I}.{KK}", (O, I, 3, 3) if KK == 9 else (O, I, 4, 4))


@pytest.mark.parametrize("O, I, KK", FRAG_SHAPES)
def test_pack_conv_frag(O, I, KK):
    w = _frag_weights(O, I, KK)
    want = P.bf16(P.pack_conv_frag(w)).reshape(-1)
    wd = dev(w)
    calls = [lambda d: L().ddimx_pack_conv_frag_k(_lib.ptr(wd), d.ptr, O, I, KK, _lib.stream())]
    if KK == 9:
        calls.append(lambda d: L().ddimx_pack_conv_frag(_lib.ptr(wd), d.ptr, O, I, _lib.stream()))
    for call in calls:
        dst = Out(w.numel(), torch.bfloat16)
        _lib.check(call(dst))
        sync()
        same(dst.read("pack_conv_frag"), want, "pack_conv_frag")


@pytest.mark.parametrize("O, I", [(48, 16), (32, 24)])
def test_pack_conv_frag_refuses_partial_fragments(O, I):
    wd = dev(weights("frag.bad", (O, I, 3, 3)))
    dst = Out(9 * O * I, torch.bfloat16)
    refused(L().ddimx_pack_conv_frag(_lib.ptr(wd), dst.ptr, O, I, _lib.stream()), dst)
    refused(L().ddimx_pack_conv_frag_k(_lib.ptr(wd), dst.ptr, O, I, 9, _lib.stream()), dst)


@pytest.mark.parametrize("O, I, KK", FRAG_SHAPES)
def test_pack_frag_from_taps(O, I, KK):
    """From the bf16 tap layout (the reference's, uploaded): the reference permutation of those taps, and the same bits as
    pack_conv_frag of the fp32 weights."""
    w = _frag_weights(O, I, KK)
    taps = P.bf16(P.pack_conv(w))
    td, wd = dev(taps), dev(w)
    dst, direct = Out(w.numel(), torch.bfloat16), Out(w.numel(), torch.bfloat16)
    _lib.check(L().ddimx_pack_frag_from_taps(_lib.ptr(td), dst.ptr, KK, O, I, _lib.stream()))
    _lib.check(L().ddimx_pack_conv_frag_k(_lib.ptr(wd), direct.ptr, O, I, KK, _lib.stream()))
    sync()
    got = dst.read("pack_frag_from_taps")
    same(got, P.frag_from_taps(taps).reshape(-1), "pack_frag_from_taps")
    same(got, direct.read("pack_conv_frag_k"), "pack_frag_from_taps against pack_conv_frag_k")
    same(td.cpu(), taps, "the taps are read-only")


@pytest.mark.parametrize("NOUT, CIN", [(48, 16), (32, 24)])
def test_pack_frag_from_taps_refuses_partial_fragments(NOUT, CIN):
    td = dev(P.bf16(gauss("taps.bad", (6, NOUT, CIN))))
    dst = Out(6 * NOUT * CIN, torch.bfloat16)
    refused(L().ddimx_pack_frag_from_taps(_lib.ptr(td), dst.ptr, 6, NOUT, CIN, _lib.stream()), dst)


def _specials(x):
    """Rounding ties (down to even, up to even, with a carry into the exponent), the largest fp32, a NaN, both infinities, a denormal
    that rounds to zero, one on a tie and the largest one, and both zeros, at the front of x."""
    b = [0x3F808000, 0x3F818000, 0x3FFF8000, 0xBF808000, 0x7F7FFFFF, 0x7FC00000, 0x7F800000, 0xFF800000, 0x00000001, 0x00018000,
         0x007FFFFF, 0x00000000, 0x80000000]
    flat = x.reshape(-1)
    k = min(len(b), flat.numel())
    flat[:k] = torch.from_numpy(np.array(b[:k], dtype=np.uint32).view(np.float32))
    return x


NHWC_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 64, 4, 8), (2, 33, 129, 124)]  # the last: 1 055 736 elements > 4096 * 256


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("shape", NHWC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nhwc_converters(shape, dt):
    B, C, H, W = shape
    x = weights(f"nhwc.{shape}", shape)
    if x.numel() > 1:
        x = _specials(x)
    xd = dev(x)
    y = Out(x.numel(), G.TORCH_DT[dt])
    _lib.check(L().ddimx_to_nhwc(dt, _lib.ptr(xd), y.ptr, B, C, H, W, _lib.stream()))
    sync()
    got, want = y.read("to_nhwc"), cast(P.to_nhwc(x), dt)
    nan = torch.isnan(want.float()).reshape(-1)
    assert torch.equal(torch.isnan(got.float()), nan), "NaN in, NaN out"
    same(got[~nan], want.reshape(-1)[~nan], "to_nhwc")  # a NaN's payload is no part of the rounding rule
    back = Out(x.numel())
    _lib.check(L().ddimx_from_nhwc(dt, y.ptr, back.ptr, B, C, H, W, _lib.stream()))
    sync()
    rt = back.read("from_nhwc")
    want_rt = cast(x, dt).float().reshape(-1)  # f32: the identity; bf16: the rounding to nearest even, widened exactly
    nan = torch.isnan(want_rt)
    assert torch.equal(torch.isnan(rt), nan)
    same(rt[~nan], want_rt[~nan], "from_nhwc(to_nhwc(x))")
    same(xd.cpu(), x, "the input is read-only")


# =========================================================================================================================================
# permutations and the batched kernels
# =========================================================================================================================================
@pytest.mark.parametrize("rows, C, Fr", [(1, 5, 3), (4, 256, 8), (1, 3, 5), (4, 8, 256)])  # the last two: the gradient direction
def test_pack_perm_cols(rows, C, Fr):
    src = torch.from_numpy(gauss(f"permc.{rows}.{C}.{Fr}", (rows, C * Fr)))
    dst = Out(src.numel())
    sd = dev(src)
    _lib.check(L().ddimx_pack_perm_cols(_lib.ptr(sd), dst.ptr, rows, C, Fr, _lib.stream()))
    sync()
    got = dst.read("pack_perm_cols")
    same(got, P.perm_cols(src, C, Fr).reshape(-1), "pack_perm_cols")
    back = Out(src.numel())  # ... and blocks.cpp's way back: C and Fr swapped
    _lib.check(L().ddimx_pack_perm_cols(dst.ptr, back.ptr, rows, Fr, C, _lib.stream()))
    sync()
    same(back.read("pack_perm_cols back"), src.reshape(-1), "pack_perm_cols there and back")


@pytest.mark.parametrize("K", [1, 7, 512])
@pytest.mark.parametrize("C, Fr", [(5, 3), (256, 8), (3, 5), (8, 256)])
def test_pack_perm_rows(C, Fr, K):
    src = torch.from_numpy(gauss(f"permr.{C}.{Fr}.{K}", (C * Fr, K)))
    dst = Out(src.numel())
    sd = dev(src)
    _lib.check(L().ddimx_pack_perm_rows(_lib.ptr(sd), dst.ptr, C, Fr, K, _lib.stream()))
    sync()
    same(dst.read("pack_perm_rows"), P.perm_rows(src, C, Fr).reshape(-1), "pack_perm_rows")
    back = Out(src.numel())
    _lib.check(L().ddimx_pack_perm_rows(dst.ptr, back.ptr, Fr, C, K, _lib.stream()))
    sync()
    same(back.read("pack_perm_rows back"), src.reshape(-1), "pack_perm_rows there and back")


def test_pack_perm_validates():
    a, d = dev(gauss("perm.bad", 64)), Out(64)
    refused(L().ddimx_pack_perm_cols(_lib.ptr(a), d.ptr, 0, 8, 8, _lib.stream()), d)
    refused(L().ddimx_pack_perm_cols(None, d.ptr, 1, 8, 8, _lib.stream()), d)
    refused(L().ddimx_pack_perm_rows(_lib.ptr(a), d.ptr, 8, 0, 8, _lib.stream()), d)
    refused(L().ddimx_pack_perm_rows(_lib.ptr(a), None, 8, 8, 1, _lib.stream()), d)


GAP = 64  # sentinel bytes between two destinations of a batched call


def _carve(sizes_bytes):
    """Offsets of regions of the given byte sizes in one buffer, 16-byte aligned, GAP sentinel bytes or more between neighbours."""
    offs, at = [], 0
    for nb in sizes_bytes:
        offs.append(at)
        at = (at + nb + GAP + 15) // 16 * 16
    return offs, at


def _expect(total, offs, refs):
    want = torch.full((total,), SENTINEL, dtype=torch.uint8)
    for o, r in zip(offs, refs):
        raw = r.contiguous().reshape(-1).view(torch.uint8)
        want[o:o + raw.numel()] = raw
    return want


@pytest.mark.parametrize("count", [1, 96, 97, 200])
def test_pack_copy_multi(count):
    """One, exactly one launch's worth, one more, and two launches and a rest; a 70 000-element entry needs 274 blocks of the 256 the
    grid has; the destinations lie in one buffer whose every other byte must stay as it was."""
    r = rng(f"pcm.{count}")
    lens = [int(v) for v in r.choice([1, 3, 255, 256, 257, 70000], size=count)]
    lens[0] = 3 if count > 1 else 70000
    lens[-1] = 70000
    if count > 96:
        lens[95], lens[96] = 257, 70000  # the last entry of the first launch and the first of the second
    src = torch.from_numpy(gauss(f"pcm.src.{count}", sum(lens)))
    sd = dev(src)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    offs, total = _carve([4 * n for n in lens])
    out = Out(total, torch.uint8)
    srcs = (ctypes.c_void_p * count)(*[sd.data_ptr() + 4 * int(s) for s in starts])
    dsts = (ctypes.c_void_p * count)(*[out.addr + o for o in offs])
    ns = (ctypes.c_longlong * count)(*lens)
    _lib.check(L().ddimx_pack_copy_multi(srcs, dsts, ns, count, _lib.stream()))
    sync()
    want = _expect(total, offs, [src[int(s):int(s) + n] for s, n in zip(starts, lens)])
    assert torch.equal(out.read("pack_copy_multi"), want), "pack_copy_multi: a destination or a gap differs"
    same(sd.cpu(), src, "the sources are read-only")


def test_pack_copy_multi_validates():
    a, d = dev(gauss("pcm.bad", 8)), Out(8)
    one = lambda v, ty=ctypes.c_void_p: (ty * 1)(v)  # noqa: E731
    refused(L().ddimx_pack_copy_multi(one(a.data_ptr()), one(d.addr), one(8, ctypes.c_longlong), 0, _lib.stream()), d)
    refused(L().ddimx_pack_copy_multi(one(a.data_ptr()), one(d.addr), one(0, ctypes.c_longlong), 1, _lib.stream()), d)
    refused(L().ddimx_pack_copy_multi(one(None), one(d.addr), one(8, ctypes.c_longlong), 1, _lib.stream()), d)
    refused(L().ddimx_pack_copy_multi(None, one(d.addr), one(8, ctypes.c_longlong), 1, _lib.stream()), d)


def _conv_entries(count):
    """(O, I, KK, mode, dtype) of a batch: many tiny entries of every combination and one of 17 280 elements (68 blocks of the 64 the
    grid has), which is neither first nor last unless it is alone."""
    r = rng(f"pcv.{count}")
    ent = []
    for i in range(count):
        mode = int(r.integers(0, 2))
        ent.append((int(r.choice([1, 2, 3, 5, 32])), int(r.choice([1, 2, 4, 7, 16])), 9 if mode else int(r.choice([9, 16])), mode,
                    int(r.integers(0, 2))))
    ent[count // 2] = (48, 40, 9, count % 2, G.BF16 if count % 3 else G.F32)
    if count >= 65:
        ent[63], ent[64] = (5, 7, 16, 0, G.BF16), (3, 5, 9, 1, G.F32)  # the last of the first launch, the first of the second
    return ent


@pytest.mark.parametrize("count", [1, 64, 65, 130])
def test_pack_conv_multi(count):
    ent = _conv_entries(count)
    assert {(m, d) for _, _, _, m, d in ent} == {(0, 0), (0, 1), (1, 0), (1, 1)} or count == 1
    ws = [weights(f"pcv.w.{count}.{i}", (O, I, 3, 3) if KK == 9 else (O, I, 4, 4)) for i, (O, I, KK, _, _) in enumerate(ent)]
    wd = [dev(w) for w in ws]
    refs = [cast(P.pack_conv_dgrad(w) if m else P.pack_conv(w), d) for w, (_, _, _, m, d) in zip(ws, ent)]
    offs, total = _carve([r.numel() * r.element_size() for r in refs])
    out = Out(total, torch.uint8)
    arr = lambda ty, v: (ty * count)(*v)  # noqa: E731
    col = lambda k: arr(ctypes.c_int, [e[k] for e in ent])  # noqa: E731
    rc = L().ddimx_pack_conv_multi(arr(ctypes.c_void_p, [w.data_ptr() for w in wd]), arr(ctypes.c_void_p, [out.addr + o for o in offs]),
                                   col(0), col(1), col(2), col(3), col(4), count, _lib.stream())
    _lib.check(rc)
    sync()
    got, want = out.read("pack_conv_multi"), _expect(total, offs, refs)
    for i, (o, r) in enumerate(zip(offs, refs)):
        nb = r.numel() * r.element_size()
        assert torch.equal(got[o:o + nb], want[o:o + nb]), f"pack_conv_multi: entry {i} {ent[i]} differs"
    assert torch.equal(got, want), "pack_conv_multi: a gap between two destinations was written"


def test_pack_conv_multi_validates():
    a, d = dev(gauss("pcv.bad", 9 * 16)), Out(9 * 16)
    one = lambda v, ty=ctypes.c_int: (ty * 1)(v)  # noqa: E731

    def call(O=4, I=4, KK=9, mode=0, dtype=0, count=1, src=a.data_ptr()):
        return L().ddimx_pack_conv_multi(one(src, ctypes.c_void_p), one(d.addr, ctypes.c_void_p), one(O), one(I), one(KK), one(mode),
                                         one(dtype), count, _lib.stream())
    for bad in (dict(count=0), dict(O=0), dict(mode=2), dict(mode=1, KK=16), dict(dtype=2), dict(src=None), dict(O=1 << 20, I=1 << 12)):
        refused(call(**bad), d)


@pytest.mark.parametrize("E", [4, 4416])
@pytest.mark.parametrize("B", [1, 19])
def test_temb_gather(B, E):
    table = torch.from_numpy(gauss(f"tg.{E}", (1000, E)))
    t = ([0, 999, 5, 999, 0, 417] * 4)[:B] if B > 1 else [999]
    td, tt = dev(table), dev(t, torch.int64)
    for tl in (t, [0] * B):
        tt.copy_(torch.tensor(tl))
        out = Out(B * E)
        _lib.check(L().ddimx_temb_gather(_lib.ptr(td), _lib.ptr(tt), out.ptr, B, E, _lib.stream()))
        sync()
        same(out.read("temb_gather"), table[torch.tensor(tl)].reshape(-1), "temb_gather")
    same(td.cpu(), table, "the table is read-only")


def test_temb_gather_refuses_rows_that_are_no_whole_float4s():
    td, tt, out = dev(gauss("tg.bad", (8, 6))), dev([1, 2], torch.int64), Out(12)
    refused(L().ddimx_temb_gather(_lib.ptr(td), _lib.ptr(tt), out.ptr, 2, 6, _lib.stream()), out)
    refused(L().ddimx_temb_gather(_lib.ptr(td), _lib.ptr(tt), out.ptr, 0, 8, _lib.stream()), out)
    refused(L().ddimx_temb_gather(_lib.ptr(td), None, out.ptr, 2, 8, _lib.stream()), out)


# =========================================================================================================================================
# step kernels
# =========================================================================================================================================
@pytest.mark.parametrize("stride", [6, 7, 9])  # generalized_steps, ddpm_steps, inpaint_steps
@pytest.mark.parametrize("B", [1, 64, 65])
def test_step_begin_and_end(B, stride):
    """t = the first entry of the counter's row as int64, for tables whose rows start with 0, 1 and 999, at the first and the last
    row; step_end adds one to the counter and touches nothing else."""
    for first in ([999.0, 500.0, 1.0, 0.0], [0.0, 1.0, 999.0], [1.0, 999.0, 0.0]):
        coef = gauss(f"sb.{stride}", (len(first), stride)) * np.float32(1000)
        coef[:, 0] = first
        cd = dev(coef)
        for step in (0, len(first) - 1):
            ctr = Out(1, torch.int32, init=torch.tensor([step], dtype=torch.int32))
            t = Out(B, torch.int64)
            if stride == 6:
                _lib.check(L().ddimx_step_begin(_lib.ptr(cd), ctr.ptr, t.ptr, B, _lib.stream()))
                sync()
                assert t.read("step_begin").tolist() == P.step_begin(coef, 6, step, B).tolist()
                t = Out(B, torch.int64)
            _lib.check(L().ddimx_step_begin_ex(_lib.ptr(cd), stride, ctr.ptr, t.ptr, B, _lib.stream()))
            sync()
            assert t.read("step_begin_ex").tolist() == P.step_begin(coef, stride, step, B).tolist() == [int(first[step])] * B
            assert ctr.read("step counter").tolist() == [step]
            _lib.check(L().ddimx_step_end(ctr.ptr, _lib.stream()))
            sync()
            assert ctr.read("step_end").tolist() == [step + 1]
        same(cd.cpu(), torch.from_numpy(coef), "the table is read-only")


SEQ = list(range(0, 1000, 100))


@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 3])  # the last: a second trip for the first three threads of the grid
def test_ddpm_update(n):
    betas = np.linspace(1e-4, 0.02, 1000, dtype=np.float64).astype(np.float32)
    coef = schedule.ddpm_coefficients(SEQ, betas)
    cd = dev(coef)
    seen = set()
    for step in (0, len(SEQ) - 1):
        # the first row (t = 900) multiplies x by about 80, the last (t = 0) by 1: inside the clamp everywhere at the smallest scale
        # of each, beyond it on both sides for many elements at the largest
        for scale in (0.001, 0.2, 3.0):
            x, e, z = (gauss(f"ddpm.{k}.{n}", n) * np.float32(scale) for k in "xez")
            xd, ed, zd, ctr = dev(x), dev(e), dev(z), dev([step], torch.int32)
            x0, xn = Out(n), Out(n)
            _lib.check(L().ddimx_ddpm_update(_lib.ptr(xd), _lib.ptr(ed), _lib.ptr(zd), x0.ptr, xn.ptr, _lib.ptr(cd), _lib.ptr(ctr), n,
                                             _lib.stream()))
            sync()
            want0, want = P.ddpm_update(x, e, z, coef[step])
            if (np.abs(want0) < 1).all():
                seen.add((step, "clear"))
            if (want0 == 1).any() and (want0 == -1).any() and (np.abs(want0) < 1).any():
                seen.add((step, "both"))
            same(x0.read("ddpm x0"), torch.from_numpy(want0), f"ddpm_update x0, step {step} scale {scale}")
            same(xn.read("ddpm xn"), torch.from_numpy(want), f"ddpm_update sample, step {step} scale {scale}")
            for d, h in ((xd, x), (ed, e), (zd, z)):
                same(d.cpu(), torch.from_numpy(h), "the inputs are read-only")
    want_seen = {(s, k) for s in (0, len(SEQ) - 1) for k in (("clear", "both") if n > 1000 else ("clear",))}
    assert want_seen <= seen, f"every row must run with the clamp never reached and (long inputs) reached on both sides: {sorted(seen)}"


@pytest.mark.parametrize("with_noise", [False, True], ids=["ode", "noise"])
@pytest.mark.parametrize("n", [4, 1024, 2048 * 256 * 4 + 4])  # the last: one float4 more than 2048 blocks of 256 threads take in a trip
def test_ddim_update(n, with_noise):
    """x0 and the new xt against step_math.h's operations in fp32, at test_ddim_update_matches_oracle_bitwise's gate."""
    x, e, z = (gauss(f"ddim.{k}.{n}", n) for k in "xez")
    mattered = False
    for eta in (0.0, 0.5):
        coef = schedule.ddim_coefficients(SEQ, alphas(), eta).astype(np.float32)
        cd = dev(coef)
        for step in (0, len(SEQ) - 1):
            xt, x0 = Out(n, init=torch.from_numpy(x)), Out(n)
            ed, zd, ctr = dev(e), dev(z), dev([step], torch.int32)
            _lib.check(L().ddimx_ddim_update(xt.ptr, _lib.ptr(ed), _lib.ptr(zd) if with_noise else None, x0.ptr, _lib.ptr(cd),
                                             _lib.ptr(ctr), n, _lib.stream()))
            sync()
            want, want0 = SM.update_core3(x, e, None, None, None, SM.load_row(coef[step]), False, False, False, with_noise, z)
            for what, got, ref in (("x0", x0.read("ddim x0"), want0), ("xt", xt.read("ddim xt"), want)):
                ref = torch.from_numpy(ref)
                worst = float(((got - ref).abs() / (1e-7 + 3e-7 * ref.abs())).max())
                print(f"[ddim_update n={n} eta={eta} step={step} {what}] worst {worst:.2e} of the gate")
                assert torch.allclose(got, ref, rtol=3e-7, atol=1e-7), (what, eta, step)
            if with_noise and coef[step, 5] != 0:  # c1 is 0 at eta = 0 and in the row that lands on t = -1
                assert not np.array_equal(want, SM.ddim_next(want0, e, *coef[step, 3:5])), "the noise term must matter in this case"
                mattered = True
            same(ed.cpu(), torch.from_numpy(e), "eps is read-only")
    assert mattered == with_noise


def test_ddim_update_refuses_a_length_that_is_no_multiple_of_four():
    coef, ctr = dev(schedule.ddim_coefficients(SEQ, alphas(), 0.0).astype(np.float32)), dev([0], torch.int32)
    xt, x0, ed = Out(8), Out(8), dev(gauss("ddim.bad", 8))
    refused(L().ddimx_ddim_update(xt.ptr, _lib.ptr(ed), None, x0.ptr, _lib.ptr(coef), _lib.ptr(ctr), 6, _lib.stream()), xt, x0)


# =========================================================================================================================================
# the embedding MLP's dense kernels against float64
# =========================================================================================================================================
ROWS = 23  # rows of the table a gather reads from


def _idx(B):
    return [int(v) for v in ([22, 3, 3, 0, 17, 22, 1, 9, 3, 8, 21, 4, 4, 16, 2, 0, 13, 22, 5])[:B]]  # unsorted, with repeats


@pytest.mark.parametrize("N, K", [(1, 4), (5, 260), (4, 256), (7, 516), (512, 128)])
def test_linear_rows(N, K):
    worst = Worst()
    W, bias = gauss(f"lr.w.{N}.{K}", (N, K)) * np.float32(K ** -0.5), gauss(f"lr.b.{N}.{K}", N)
    table = gauss(f"lr.x.{N}.{K}", (ROWS, K))
    Wd, bd, xd = dev(W), dev(bias), dev(table)
    for B in (1, 8, 9, 19):
        for idx in (None, _idx(B)):
            idd = None if idx is None else dev(idx, torch.int64)
            for act in (0, 1):
                for ins in (0, 1):
                    y = Out(B * N)
                    _lib.check(L().ddimx_linear_rows(_lib.ptr(xd), _lib.ptr(idd), _lib.ptr(Wd), _lib.ptr(bd), y.ptr, B, N, K, act, ins,
                                                     _lib.stream()))
                    sync()
                    want = P.linear(table[:B] if idx is None else table, W, bias, idx, bool(act), bool(ins))
                    worst.close(y.read("linear_rows"), want, f"linear_rows N={N} K={K} B={B} idx={idx is not None} act={act} in={ins}")
    report(f"linear_rows N={N} K={K}", worst.mx, worst.rms)
    same(xd.cpu(), torch.from_numpy(table), "x is read-only")


def test_linear_rows_validates():
    a, y = dev(gauss("lr.bad", 64)), Out(8)
    refused(L().ddimx_linear_rows(_lib.ptr(a), None, _lib.ptr(a), _lib.ptr(a), y.ptr, 2, 4, 6, 0, 0, _lib.stream()), y)
    refused(L().ddimx_linear_rows(_lib.ptr(a), None, _lib.ptr(a), None, y.ptr, 2, 4, 8, 0, 0, _lib.stream()), y)
    refused(L().ddimx_linear_rows(_lib.ptr(a), None, _lib.ptr(a), _lib.ptr(a), y.ptr, 0, 4, 8, 0, 0, _lib.stream()), y)


@pytest.mark.parametrize("N, K", [(1, 1), (3, 255), (3, 257), (5, 600)])
def test_linear_bwd_w(N, K):
    wdw, wdb = Worst(), Worst()
    table = gauss(f"lbw.x.{N}.{K}", (ROWS, K))
    xd = dev(table)
    for B in (1, 19):
        dy = gauss(f"lbw.dy.{N}.{K}.{B}", (B, N))
        dyd = dev(dy)
        for idx in (None, _idx(B)):
            idd = None if idx is None else dev(idx, torch.int64)
            for xs in (0, 1):
                dW, db = Out(N * K), Out(N)
                _lib.check(L().ddimx_linear_bwd_w(_lib.ptr(dyd), _lib.ptr(xd), _lib.ptr(idd), dW.ptr, db.ptr, B, N, K, xs, _lib.stream()))
                sync()
                want_w, want_b = P.linear_bwd_w(dy, table[:B] if idx is None else table, idx, bool(xs))
                tag = f"N={N} K={K} B={B} idx={idx is not None} silu={xs}"
                wdw.close(dW.read("linear_bwd_w dW"), want_w, "linear_bwd_w dW " + tag)
                wdb.close(db.read("linear_bwd_w db"), want_b, "linear_bwd_w db " + tag)
    report(f"linear_bwd_w dW N={N} K={K}", wdw.mx, wdw.rms)
    report(f"linear_bwd_w db N={N} K={K}", wdb.mx, wdb.rms)


@pytest.mark.parametrize("N, K", [(1, 1), (15, 17), (16, 16), (33, 40)])
def test_linear_bwd_x(N, K):
    worst = Worst()
    W = gauss(f"lbx.w.{N}.{K}", (N, K))
    Wd = dev(W)
    for B in (1, 5):
        dy, xpre = gauss(f"lbx.dy.{N}.{K}.{B}", (B, N)), gauss(f"lbx.x.{N}.{K}.{B}", (B, K)) * np.float32(2)
        dx = Out(B * K)
        dyd, xd = dev(dy), dev(xpre)
        _lib.check(L().ddimx_linear_bwd_x(_lib.ptr(dyd), _lib.ptr(Wd), _lib.ptr(xd), dx.ptr, B, N, K, _lib.stream()))
        sync()
        worst.close(dx.read("linear_bwd_x"), P.linear_bwd_x(dy, W, xpre), f"linear_bwd_x N={N} K={K} B={B}")
    report(f"linear_bwd_x N={N} K={K}", worst.mx, worst.rms)


def test_linear_bwd_validates():
    a, o1, o2 = dev(gauss("lb.bad", 64)), Out(16), Out(4)
    refused(L().ddimx_linear_bwd_w(_lib.ptr(a), _lib.ptr(a), None, o1.ptr, o2.ptr, 0, 4, 4, 0, _lib.stream()), o1, o2)
    refused(L().ddimx_linear_bwd_w(_lib.ptr(a), _lib.ptr(a), None, o1.ptr, None, 2, 4, 4, 0, _lib.stream()), o1, o2)
    refused(L().ddimx_linear_bwd_x(_lib.ptr(a), _lib.ptr(a), _lib.ptr(a), o1.ptr, 2, 0, 4, _lib.stream()), o1)
    refused(L().ddimx_linear_bwd_x(_lib.ptr(a), _lib.ptr(a), None, o1.ptr, 2, 4, 4, _lib.stream()), o1)


def test_temb_train_forward_and_backward_at_a_ragged_shape():
    """(pos_ch, emb_ch, E) = (12, 20, 37), B = 3: no dimension is a whole tile of any of the four kernels.  Every output, the two
    pre-activations and the two scratch gradients d_h2 / d_h1 included, against autograd in float64."""
    pos, emb, E, B = 12, 20, 37, 3
    g = lambda k, shape, s=1.0: gauss("tt." + k, shape) * np.float32(s)  # noqa: E731
    te, t = g("te", (50, pos)), [49, 0, 49]
    p = dict(w0=g("w0", (emb, pos), pos ** -0.5), b0=g("b0", emb, 0.1), w1=g("w1", (emb, emb), emb ** -0.5), b1=g("b1", emb, 0.1),
             w2=g("w2", (E, emb), emb ** -0.5), b2=g("b2", E, 0.1))
    d_out = g("dout", (B, E))
    want = P.temb_autograd(te, t, d_out=d_out, **p)
    d = {k: dev(v) for k, v in p.items()}
    ted, td, dod = dev(te), dev(t, torch.int64), dev(d_out)
    o = {k: Out(int(np.prod(v.shape))) for k, v in want.items()}
    _lib.check(L().ddimx_temb_fwd_train(_lib.ptr(ted), _lib.ptr(td), *[_lib.ptr(d[k]) for k in ("w0", "b0", "w1", "b1", "w2", "b2")],
                                        o["h1_pre"].ptr, o["h2_pre"].ptr, o["out"].ptr, B, pos, emb, E, _lib.stream()))
    _lib.check(L().ddimx_temb_bwd(_lib.ptr(dod), _lib.ptr(ted), _lib.ptr(td), _lib.ptr(d["w1"]), _lib.ptr(d["w2"]), o["h1_pre"].ptr,
                                  o["h2_pre"].ptr, o["d_h2"].ptr, o["d_h1"].ptr, o["d_w0"].ptr, o["d_b0"].ptr, o["d_w1"].ptr,
                                  o["d_b1"].ptr, o["d_w2"].ptr, o["d_b2"].ptr, B, pos, emb, E, _lib.stream()))
    sync()
    for k in sorted(want):
        w = Worst()
        w.close(o[k].read(k), want[k], f"temb {k}")
        report(f"temb (12, 20, 37) B=3 {k}", w.mx, w.rms)


# =========================================================================================================================================
# the whole packed buffer
# =========================================================================================================================================
def _param_pack(lib, h, i):
    kind, off, nbytes, dims = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong(), (ctypes.c_int * 4)()
    _lib.check(lib.ddimx_debug_param_pack(h, i, ctypes.byref(kind), ctypes.byref(off), ctypes.byref(nbytes), dims))
    return kind.value, off.value, nbytes.value, tuple(dims)


def _region_ref(kind, dims, w, adt, C5):
    """What ddimx_pack_weights writes for one parameter, on the parameter's device, as the bytes of its layout."""
    d0, d1, d2, d3 = dims
    if kind == _lib.DDIMX_PACK_COPY:
        r = w
    elif kind in (_lib.DDIMX_PACK_CONV, _lib.DDIMX_PACK_CONV_F32):
        r = P.pack_conv(w.reshape(d0, d1, d2, d3))
        r = r.to(adt) if kind == _lib.DDIMX_PACK_CONV else r
    elif kind == _lib.DDIMX_PACK_CONVT:
        r = P.pack_convT(w.reshape(d0, d1, 4, 4).cpu()).to(w.device).to(adt)
    elif kind == _lib.DDIMX_PACK_BIAS2:
        r = torch.cat([w.reshape(-1), w.reshape(-1)])
    elif kind == _lib.DDIMX_PACK_PERM_COLS:
        r = P.perm_cols(w.reshape(d0, d1), C5, d1 // C5)
    elif kind == _lib.DDIMX_PACK_PERM_ROWS:
        r = P.perm_rows(w.reshape(d0, d1), C5, d0 // C5)
    else:
        raise AssertionError(f"pack kind {kind}")
    return r.contiguous().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("tensor", ["torch.cuda.FloatTensor", "torch.cuda.BFloat16Tensor"], ids=DT_IDS)
def test_pack_weights_writes_every_region_and_nothing_else(tensor):
    """The full-size audio model: every parameter's region of the packed buffer bit for bit against the reference of its kind (applied
    on the device: torch indexing and torch's bf16 cast, which rounds to nearest even), the regions pairwise disjoint, every other
    byte -- padding, and the ranges only ddimx_pack_fnet_inference writes -- left as it was; after one conv weight and one bias change,
    a second pack changes those two regions and no other byte."""
    t0 = time.time()
    import ddim_audio_amd as D
    model = D.Model(configs.audio_config(tensor)).to(G.dev())
    lib = model._ensure_handle()
    h = model._handle
    adt = torch.bfloat16 if "BFloat16" in tensor else torch.float32
    C5 = model.config.ch[-1]
    names = list(model._inventory)
    tensors = [t.detach() for t in model._state_tensors()]
    gen = torch.Generator(device=G.dev())
    gen.manual_seed(11)
    for t in tensors:
        t.normal_(generator=gen)
    n = lib.ddimx_num_params(h)
    assert n == len(tensors)
    total = int(lib.ddimx_packed_bytes(h))
    packed = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=G.dev())
    body = packed[GUARD:GUARD + total]
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    info = [_param_pack(lib, h, i) for i in range(n)]
    kinds = {k for k, _, _, _ in info}
    assert kinds == set(range(7)), f"the config must have every pack kind, has {sorted(kinds)}"
    assert sum(k in (_lib.DDIMX_PACK_CONV, _lib.DDIMX_PACK_CONV_F32) for k, _, _, _ in info) > 64
    assert sum((k == _lib.DDIMX_PACK_COPY) + 2 * (k == _lib.DDIMX_PACK_BIAS2) for k, _, _, _ in info) > 96
    spans = sorted((off, off + nb, i) for i, (_, off, nb, _) in enumerate(info))
    assert spans[0][0] >= 0 and spans[-1][1] <= total
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "two parameters' regions overlap"

    def pack_and_check(changed=None, before=None):
        _lib.check(lib.ddimx_pack_weights(h, arr, n, ctypes.c_void_p(body.data_ptr()), _lib.stream()))
        sync()
        outside = torch.ones(total, dtype=torch.bool, device=G.dev())
        for i, (kind, off, nb, dims) in enumerate(info):
            want = _region_ref(kind, dims, tensors[i], adt, C5)
            assert want.numel() == nb, (names[i], want.numel(), nb)
            assert torch.equal(body[off:off + nb], want), f"{names[i]} (kind {kind}, dims {dims}): the packed region differs"
            outside[off:off + nb] = False
            if before is not None:
                assert torch.equal(body[off:off + nb], before[off:off + nb]) == (i not in changed), f"{names[i]}: changed / unchanged"
        assert bool((body[outside] == 0xA5).all()), "a byte outside every parameter's region was written"
        assert bool((packed[:GUARD] == 0xA5).all()) and bool((packed[GUARD + total:] == 0xA5).all()), "written outside the buffer"
        return int(outside.sum())

    free = pack_and_check()
    assert free > 0, "the buffer holds inference-only copies and padding that ddimx_pack_weights must not touch"
    before = body.clone()
    conv = next(i for i, (k, _, _, _) in enumerate(info) if k == _lib.DDIMX_PACK_CONV and i > n // 3)
    bias = next(i for i, (k, _, _, _) in enumerate(info) if k == _lib.DDIMX_PACK_BIAS2)
    with torch.no_grad():
        tensors[conv].mul_(-1.5)
        tensors[bias].add_(1.0)
    pack_and_check(changed={conv, bias}, before=before)
    print(f"[pack_weights {tensor}] {n} parameters, {total} bytes, {free} outside every region; {time.time() - t0:.1f} s")
