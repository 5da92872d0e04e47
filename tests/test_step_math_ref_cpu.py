"""tests/step_math_ref.py on the CPU: the fused multiply-add against exact rational arithmetic -- random operands, sums that the
fp64 evaluation puts exactly on an fp32 tie while the exact sum lies beside it, results below the normal range -- and why the
double-rounding form that the kernel references used before is gone; ``updater32`` against the scalar operations, and that a term
whose flag is off never reads its input."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import step_math_ref as SM

F32 = np.float32


def _rn32(v):
    """The fp32 nearest to the rational v, ties to even: the nearest of the fp32 neighbours of its fp64 rounding, chosen exactly."""
    f = F32(float(v))
    cands = [f, np.nextafter(f, F32(np.inf)), np.nextafter(f, F32(-np.inf))]
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - v), int(c.view(np.uint32)) & 1))


def _exact(a, b, c):
    return np.array([_rn32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], dtype=F32)


def _double_rounding(a, b, c):
    """What tests/tail_kernel_ref.py called fma32 before: the exact product, the sum rounded to fp64 and then to fp32."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def test_fma32_rounds_once():
    f = np.float32
    # a b = 1 + 2^-11 + 2^-24: halfway between two fp32 neighbours; the addend decides, however small
    x = f(1 + 2.0 ** -12)
    lo, hi = f(1 + 2.0 ** -11), np.nextafter(f(1 + 2.0 ** -11), f(2))
    assert float(x) * float(x) == float(lo) + 2.0 ** -24
    assert SM.fma32(x, x, f(2.0 ** -70)) == hi and SM.fma32(x, x, f(-2.0 ** -70)) == lo
    assert SM.fma32(x, x, f(0)) == lo  # the tie itself goes to even
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(4096).astype(f) for _ in range(3))
    got = SM.fma32(a, b, c)
    want = torch.addcmul(torch.from_numpy(c).double(), torch.from_numpy(a).double(), torch.from_numpy(b).double()).float().numpy()
    assert np.array_equal(got, want), "where double rounding does not bite the plain fp64 evaluation agrees"


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -20, 2.0 ** 30], ids=["unit", "small_addend", "cancelling"])
def test_fma32_equals_the_exact_sum_on_random_operands(scale):
    rng = np.random.default_rng(7)
    a, b = rng.standard_normal(2000).astype(F32), rng.standard_normal(2000).astype(F32)
    c = (rng.standard_normal(2000) * scale).astype(F32)
    if scale > 1:  # c close to -a b: the sum keeps only the product's low bits
        c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(F32)
    assert np.array_equal(_bits(SM.fma32(a, b, c)), _bits(_exact(a, b, c)))


def _ties():
    """(a, a, c) with a = 1 + k 2^-12, k odd: a a = 1 + k 2^-11 + k^2 2^-24 ends in the half-ulp bit and nothing below it, and
    c = +-2^-70 vanishes in the fp64 sum but not in the exact one -- once per side of the tie."""
    k = np.arange(1, 1600, 2)
    a = (1.0 + k * 2.0 ** -12).astype(F32)
    assert (a.astype(np.float64) ** 2 < 2).all() and ((a.astype(np.float64) ** 2 * 2.0 ** 24) % 2 == 1).all()
    a = np.concatenate([a, a])
    c = np.concatenate([np.full(k.size, 2.0 ** -70), np.full(k.size, -2.0 ** -70)]).astype(F32)
    return a, c


def test_fma32_on_constructed_ties_follows_the_exact_sum_on_both_sides():
    a, c = _ties()
    s64 = a.astype(np.float64) * a.astype(np.float64) + c.astype(np.float64)
    assert ((s64.view(np.int64) & 0x1FFFFFFF) == 0x10000000).all(), "the fp64 sum sits exactly on the fp32 tie"
    want = _exact(a, a, c)
    got = SM.fma32(a, a, c)
    assert np.array_equal(_bits(got), _bits(want))
    n = a.size // 2
    assert (got[:n] > got[n:]).all(), "the sign of the addend decides"


def test_the_double_rounding_form_misses_the_constructed_ties():
    """Why it was removed: it sends every such sum to the even neighbour, whichever side of the tie the exact sum lies on -- wrong
    for exactly one of the two signs of c at every a."""
    a, c = _ties()
    old, want = _double_rounding(a, a, c), _exact(a, a, c)
    n = a.size // 2
    wrong = _bits(old) != _bits(want)
    assert np.array_equal(_bits(old[:n]), _bits(old[n:])), "it cannot see the addend"
    assert (wrong[:n] ^ wrong[n:]).all() and wrong.sum() == n
    assert not (_bits(SM.fma32(a, a, c)) != _bits(want)).any()


def test_fma32_below_the_normal_range():
    rng = np.random.default_rng(11)
    n = 1500
    a = (rng.standard_normal(n) * 2.0 ** -70).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** -62).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** -135).astype(F32)  # subnormal addends, some flushed to +-0 by the cast
    want = _exact(a, b, c)
    assert (np.abs(want) < 2.0 ** -126).all() and (want != 0).sum() > n // 2
    assert np.array_equal(_bits(SM.fma32(a, b, c)), _bits(want))
    # products of m 2^-150: halfway between two subnormals for odd m, exactly (ties to even), and beside it with an addend
    m = np.arange(1, 400, dtype=np.float64)
    a, b = (m * 2.0 ** -75).astype(F32), np.full(m.size, 2.0 ** -75, dtype=F32)
    for c in (0.0, 2.0 ** -149, -2.0 ** -149):
        cc = np.full(m.size, c, dtype=F32)
        assert np.array_equal(_bits(SM.fma32(a, b, cc)), _bits(_exact(a, b, cc))), c


# ---- the update ---------------------------------------------------------------------------------------------------------------------------
def _arrays(n=4099):
    rng = np.random.default_rng(3)
    return [rng.standard_normal(n).astype(F32) for _ in range(6)]


ROW9 = np.array([412.0, 0.83, 0.55, 0.61, 0.79, 0.27, 0.4, -0.3, 0.2], dtype=F32)


@pytest.mark.parametrize("cols", [6, 8, 9])
def test_updater32_without_history_terms_or_noise_is_ddim_x0_and_ddim_next(cols):
    x, e, m1, m2, m3, z = _arrays()
    row = ROW9[:cols].copy()
    row[5:] = 0
    u, m0 = SM.updater32(x, e, m1, m2, m3, z=z)(row)
    want0 = SM.ddim_x0(x, e, row[1], row[2])
    assert m0.dtype == F32 and u.dtype == F32
    assert np.array_equal(_bits(m0), _bits(want0)) and np.array_equal(_bits(u), _bits(SM.ddim_next(want0, e, row[3], row[4])))
    # and the operations are the header's: fma and division, product and fma, each rounded once
    assert np.array_equal(_bits(want0), _bits((SM.fma32(e, -row[1], x) / row[2]).astype(F32)))
    assert np.array_equal(_bits(u), _bits(SM.fma32(e, row[4], (want0 * row[3]).astype(F32))))


@pytest.mark.parametrize("hist,hist2", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("k", range(16))
def test_a_term_whose_flag_is_off_never_reads_its_input(k, hist, hist2):
    """Bit 0 / 1 / 2 / 3 of k: c1 / w1 / w2 / w3 non-zero.  Every input whose term is off -- by the row or by a null buffer -- is all
    NaN: the result is finite and is the unpoisoned one; every term that is on changes it."""
    x, e, m1, m2, m3, z = _arrays()
    row = ROW9.copy()
    for bit, col in enumerate((5, 6, 7, 8)):
        if not k >> bit & 1:
            row[col] = 0
    on = dict(z=bool(k & 1), w1=bool(k & 2), w2=bool(k & 4 and hist), w3=bool(k & 8 and hist2))
    reads = dict(z=on["z"], m1=on["w1"] or on["w2"], m2=on["w2"] or on["w3"], m3=on["w3"])
    nan = np.full_like(x, np.nan)
    want_u, want_0 = SM.updater32(x, e, m1, m2, m3, z=z)(row, hist, hist2)
    poisoned = {name: (v if reads[name] else nan) for name, v in dict(m1=m1, m2=m2, m3=m3, z=z).items()}
    got_u, got_0 = SM.updater32(x, e, poisoned["m1"], poisoned["m2"], poisoned["m3"], z=poisoned["z"])(row, hist, hist2)
    assert np.isfinite(got_u).all() and np.array_equal(_bits(got_u), _bits(want_u)) and np.array_equal(_bits(got_0), _bits(want_0))
    for name, col in (("z", 5), ("w1", 6), ("w2", 7), ("w3", 8)):
        if on[name]:
            less = row.copy()
            less[col] = 0
            assert not np.array_equal(SM.updater32(x, e, m1, m2, m3, z=z)(less, hist, hist2)[0], want_u), name
    # an input that IS read reaches the result
    for name in ("m1", "m2", "m3", "z"):
        if reads[name]:
            args = dict(dict(m1=m1, m2=m2, m3=m3, z=z), **{name: nan})
            assert np.isnan(SM.updater32(x, e, args["m1"], args["m2"], args["m3"], z=args["z"])(row, hist, hist2)[0]).all(), name


def test_updater32_keeps_its_stages_and_rows_share_them():
    x, e, m1, m2, m3, z = _arrays(64)
    up = SM.updater32(x, e, m1, m2, m3, z=z)
    full, _ = up(ROW9)
    less = ROW9.copy()
    less[8] = 0
    a, b = up(less, True, True), up(ROW9, True, False)
    assert a[0] is b[0] and a[1] is b[1], "a null hist2 and w3 = 0 are the same chain"
    assert up(ROW9)[0] is full and not np.array_equal(full, a[0])
    assert np.array_equal(up(ROW9[:8])[0], a[0]) and SM.load_row(ROW9[:6])[5:] == (0, 0, 0)
    with pytest.raises(AssertionError):
        SM.load_row(ROW9[:7])
