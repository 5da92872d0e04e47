"""Restoring pool, host side (no GPU): the rows of a restoration request against ``schedule.inpaint_solver_coefficients`` and
those of a generation request against ``request_rows``; ``RestoreTable``'s images and flags word through a mixed queue with
more requests than slots, slot reuse included, driven by ``RestorePool`` itself over a stepper that does nothing; every refusal
before any device work; the fourth header table of ``_lib`` (membership, never its full contents), the binding of
``rpx_pool_update``, the library's ``rpx_`` symbols, the source list, the launcher's refusals; and the float32 restatement of
the kernel (tests/restore_pool_ref.py) against a float64 one of the known region's path."""
import contextlib
import os
import shutil
import subprocess
from ctypes import c_int, c_longlong, c_void_p

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, build, restore_pool as RP
from ddim_audio_amd.pool import LEN, POS, SAMPLE, SEED_HI, SEED_LO, Ticket, request_rows
from ddim_audio_amd.schedule import inpaint_solver_coefficients

import model_harness as MH
import restore_pool_ref as R
import step_math_ref as S

HEADER = "restore_pool/rpx_restore_pool.h"
RPX = ("rpx_pool_update",)
SHAPE = (2, 8, 4)  # C, T, F of the host-side pools (any callable is a model)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("tau", [0.0, 1.0])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_restoration_rows_are_the_named_columns_of_inpaint_solver_coefficients(order, tau, prediction):
    a = MH.alphas()
    seq = MH.spread(9)
    rows, known = RP.restore_rows(seq, a, order, tau, prediction)
    c = inpaint_solver_coefficients(seq, a, order, tau, 0.0, prediction)
    c32 = np.ascontiguousarray(c, dtype=np.float32)  # InpaintSolverStepper's cast of its table (sampler.DDIMStepper)
    assert rows.dtype == np.float32 and rows.shape == (9, 8) and rows.flags.c_contiguous
    assert known.dtype == np.float32 and known.shape == (9, RP.KNOWN_STRIDE) and known.flags.c_contiguous
    for col, name in enumerate(["t", "s1", "s2", "s3", "c2", "c1"]):
        assert np.array_equal(_bits(rows[:, col]), _bits(c32[:, col])), name
    assert np.array_equal(_bits(rows[:, 6]), _bits(c32[:, 11])) and np.array_equal(_bits(rows[:, 7]), _bits(c32[:, 12])), "w1, w2"
    assert np.array_equal(_bits(known[:, 0]), _bits(c32[:, 9])) and np.array_equal(_bits(known[:, 1]), _bits(c32[:, 10])), "cx, w0"
    assert (c[:, 8] == 0).all(), "no guidance: rho = 0 in every row"
    assert known[-1].tolist() == [0.0, 1.0], "the final row puts y back exactly"
    assert (known[:-1, 0] != 0).all() and ((rows[:, 5] != 0).any() == (tau > 0))
    assert (rows[:, 6] != 0).any() == (order >= 2) and (rows[:, 7] != 0).any() == (order == 3)


# ---- a pool on the host: the stepper does nothing, every device call of RestorePool lands on the CPU ------------------------------------
class _NoStepper:
    captures = 0

    def __init__(self, model, table, sample_shape, device, **kw):
        self.xt = torch.zeros((table.slots,) + tuple(sample_shape))
        self.table, self.kw, self.log = table, kw, []

    def admit(self, b, entry):
        p = entry.payload
        self.log.append((b, isinstance(p, RP.Known)))
        if isinstance(p, RP.Known):
            assert p.y.shape == p.mask.shape == p.x.shape == self.xt[b].shape and p.y.dtype == p.mask.dtype == torch.float32
            assert bool((p.y[p.mask == 0] == 0).all()), "_known: y is 0 where the mask is 0"
            assert np.array_equal(p.rows, self.table.known[b, :entry.rows.shape[0]]), "the table's image was written first"

    def step(self):
        pass

    def close(self):
        pass


@pytest.fixture
def host(monkeypatch):
    monkeypatch.setattr(RP, "RestoreStepper", _NoStepper)
    monkeypatch.setattr(RP, "_device", lambda model, x: torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())

    def make(slots=2, max_steps=8, prediction=None):
        return D.RestorePool(lambda x, t: x, MH.alphas(), slots=slots, t_size=SHAPE[1], max_steps=max_steps, prediction=prediction)
    return make


def _x(n, tag):
    return D.synth.gaussian("rpool.cpu." + tag, (n,) + SHAPE)


def _mask():
    m = torch.zeros(SHAPE)
    m[:, :3] = 1
    m[:, 3] = 0.25
    return m


def test_generation_rows_equal_request_rows(host):
    pool = host(slots=4)
    a = MH.alphas()
    ns = D.NoiseStream(0x1234567890, first_sample=5)
    cases = [dict(eta=0.0, order=1), dict(eta=0.5, order=1, noise=ns), dict(order=2), dict(order=3), dict(order=2, tau=1.0, noise=ns),
             dict(order=2, corrector=True)]
    for kw in cases:
        seq = MH.spread(6)
        tk = pool.submit(_x(2, "gen"), seq, **kw)
        e0, e1 = list(pool.table.queue)[-2:]
        want = request_rows(seq, a, kw.get("eta", 0.0), kw.get("order", 1), kw.get("tau", 0.0), kw.get("corrector", False))
        assert e0.rows.dtype == np.float32 and np.array_equal(_bits(e0.rows), _bits(want)) and e1.rows is e0.rows, kw
        assert not isinstance(e0.payload, RP.Known) and e0.ticket is tk and (e0.index, e1.index) == (0, 1)
        seed, first = (ns.seed, 5) if "noise" in kw else (0, 0)
        assert (e0.seed, e0.sample, e1.sample) == (seed, first, first + 1), "SamplerPool's noise identity"
    # a restoration request beside them: the same identity rule, its rows from restore_rows
    tk = pool.submit(_x(2, "res"), MH.spread(6), order=3, tau=1.0, noise=ns, y=_x(2, "y"), mask=_mask())
    e0, e1 = list(pool.table.queue)[-2:]
    rows, known = RP.restore_rows(MH.spread(6), a, 3, 1.0, "eps")
    assert np.array_equal(_bits(e0.rows), _bits(rows)) and np.array_equal(_bits(e0.payload.rows), _bits(known))
    assert isinstance(e1.payload, RP.Known) and (e0.seed, e0.sample, e1.sample) == (ns.seed, 5, 6)


def test_v_pool_takes_its_rows_for_v(host):
    pool = host(prediction="v")
    pool.submit(_x(1, "v"), MH.spread(5), order=2, y=_x(1, "vy"), mask=_mask())
    rows, known = RP.restore_rows(MH.spread(5), MH.alphas(), 2, 0.0, "v")
    e = pool.table.queue[-1]
    assert np.array_equal(_bits(e.rows), _bits(rows)) and np.array_equal(_bits(e.payload.rows), _bits(known))
    assert pool._stepper.kw["v_table"] is not None


# ---- 2. slot images --------------------------------------------------------------------------------------------------------------------
def test_slot_images_and_flags_through_a_mixed_queue_with_slot_reuse(host):
    """Two slots, five samples.  R1 (restoration, 3 steps) and G1 (generation, 2 steps) enter first; R2 (two restoring samples, 2
    steps, tau = 1) follows into whichever slot frees; G2 (generation, 4 steps) is admitted into slot 1 right after R2's first
    sample has left it: its flag is 0."""
    pool = host(slots=2, max_steps=4)
    a, tb = MH.alphas(), None
    ns_g, ns_r = D.NoiseStream(77, first_sample=3), D.NoiseStream((9 << 32) | 5, first_sample=40)
    seq3, seq2, seq4 = MH.spread(3), MH.spread(2), MH.spread(4)
    t_r1 = pool.submit(_x(1, "r1"), seq3, order=2, y=_x(1, "y1"), mask=_mask())
    t_g1 = pool.submit(_x(1, "g1"), seq2, eta=0.5, noise=ns_g)
    t_r2 = pool.submit(_x(2, "r2"), seq2, order=1, tau=1.0, noise=ns_r, y=_x(1, "y2")[0], mask=_mask() > 0)  # broadcast; bool mask
    t_g2 = pool.submit(_x(1, "g2"), seq4, order=2)
    tb = pool.table
    assert isinstance(tb, RP.RestoreTable) and tb.known.shape == (2, 4, 2) and tb.header.shape == (2, 8) and not tb.known.any()
    r1, k1 = RP.restore_rows(seq3, a, 2, 0.0, "eps")
    r2, k2 = RP.restore_rows(seq2, a, 1, 1.0, "eps")
    # per pool step: (pos, len, flags) of slot 0 and of slot 1 afterwards, and the tickets the step completes
    want = [((1, 3, 1), (1, 2, 0), []), ((2, 3, 1), (2, 2, 0), [t_g1]), ((3, 3, 1), (1, 2, 1), [t_r1]), ((1, 2, 1), (2, 2, 1), []),
            ((2, 2, 1), (1, 4, 0), [t_r2]), ((2, 2, 1), (2, 4, 0), []), ((2, 2, 1), (3, 4, 0), []), ((2, 2, 1), (4, 4, 0), [t_g2])]
    for i, (s0, s1, done) in enumerate(want):
        got = pool.step()
        hd = tb.header
        assert [tuple(int(hd[b, w]) for w in (POS, LEN, RP.FLAGS)) for b in (0, 1)] == [s0, s1], i
        assert got == done and (hd[:, 7] == 0).all(), i
        if i == 0:
            assert np.array_equal(tb.arena[0, :3], r1) and np.array_equal(tb.known[0, :3], k1) and not tb.known[1].any()
            assert np.array_equal(tb.arena[1, :2], request_rows(seq2, a, 0.5, 1)) and int(hd[1, SAMPLE]) == 3 and int(hd[1, SEED_LO]) == 77
        if i == 2:  # R2's first sample in the slot G1 left
            assert np.array_equal(tb.arena[1, :2], r2) and np.array_equal(tb.known[1, :2], k2)
            assert [int(hd[1, w]) for w in (SEED_LO, SEED_HI, SAMPLE)] == [5, 9, 40]
        if i == 3:  # ... and its second in the slot R1 left: the third row of R1's image stays, beyond len, and is never read
            assert np.array_equal(tb.known[0, :2], k2) and np.array_equal(tb.known[0, 2], k1[2]) and int(hd[0, SAMPLE]) == 41
        if i == 4:  # a generation request into the slot a restoration request has just left
            assert int(hd[1, RP.FLAGS]) == 0 and np.array_equal(tb.arena[1, :4], request_rows(seq4, a, 0.0, 2))
    assert pool.step() == [] and not tb.queue and not tb.active()
    assert pool._stepper.log == [(0, True), (1, False), (1, True), (0, True), (1, False)]
    assert pool.stats == {"steps": 8, "busy": 3 + 2 + 2 + 2 + 4, "idle": 16 - 13, "captures": 0}
    pool.close()
    with pytest.raises(ValueError, match="closed"):
        pool.submit(_x(1, "late"), seq2)


def test_restore_table_alone_needs_no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the host side loaded the library")))
    tb = RP.RestoreTable(3, 5)
    rows, known = RP.restore_rows(MH.spread(4), MH.alphas(), 2)
    tk = Ticket(2)
    tb.push(tk, 0, rows, 1, 2, 0, RP.Known(None, None, None, known))
    tb.push(tk, 1, request_rows(MH.spread(4), MH.alphas(), 0.0, 2), payload=None)
    with pytest.raises(ValueError, match="cx, w0"):
        tb.push(tk, 0, rows, payload=RP.Known(None, None, None, known[:-1]))
    with pytest.raises(ValueError, match="cx, w0"):
        tb.push(tk, 0, rows, payload=RP.Known(None, None, None, known.astype(np.float64)))
    assert [b for b, _ in tb.admit()] == [0, 1]
    assert tb.header[:, RP.FLAGS].tolist() == [RP.KNOWN, 0, 0] and np.array_equal(tb.known[0, :4], known) and not tb.known[1:].any()
    for _ in range(4):
        tb.advance()
    assert tk.done and tb.active() == []


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_device_work(monkeypatch):
    def never(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(_lib, "load", never)
    monkeypatch.setattr(RP, "RestoreStepper", never)
    monkeypatch.setattr(RP, "_device", never)
    a = MH.alphas()
    model = lambda x, t: x  # noqa: E731  (never called)
    with pytest.raises(ValueError, match="threshold"):
        D.RestorePool(model, a, threshold=D.X0Clip(1.0))
    pool = D.RestorePool(model, a, slots=2, t_size=SHAPE[1], max_steps=8)
    x, y, m, seq = _x(1, "bad"), _x(1, "bady"), _mask(), MH.spread(5)
    ns = D.NoiseStream(1)
    bs = D.BrownianStream(1)
    bad = [(dict(y=y), "mask"), (dict(mask=m), r"\by\b"), (dict(y=y, mask=m, eta=0.5, noise=ns), "eta"),
           (dict(y=y, mask=m, corrector=True), "corrector"), (dict(y=y, mask=m, tau=1.0, noise=bs), "BrownianStream"),
           (dict(tau=1.0, noise=bs), "BrownianStream"), (dict(y=y, mask=m, tau=1.0), "noise"), (dict(tau=1.0), "noise"),
           (dict(y=y, mask=m * 2), "mask"), (dict(y=y[:, :1, :3], mask=m), "y"), (dict(y=y, mask=m, order=4), "order"),
           (dict(y=y.long(), mask=m), "y")]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            pool.submit(x, seq, **kw)
        assert pool._stepper is None and not pool.table.queue, kw
    with pytest.raises(ValueError, match="max_steps"):
        pool.submit(x, MH.spread(9), y=y, mask=m)
    assert pool._stepper is None


# ---- 4. binding and build ----------------------------------------------------------------------------------------------------------------
def test_the_header_is_a_member_of_the_fourth_table_and_of_no_other():
    assert HEADER in _lib.FEATURE_DIRS and list(_lib.FEATURE_DIRS) == sorted(_lib.FEATURE_DIRS)
    assert os.path.isfile(os.path.join(_lib._INCLUDE, "features", *HEADER.split("/")))
    for table in (_lib.HEADERS, _lib.FEATURE_HEADERS, _lib.FEATURES):
        assert HEADER not in table and os.path.basename(HEADER) not in table
    h = _lib.FEATURE_DIRS[HEADER]
    assert tuple(h.funcs) == RPX and h.structs == {}
    assert h.consts["RPX_KNOWN_STRIDE"] == 2 and h.consts["RPX_KNOWN"] == 1 and h.consts["RPX_FLAGS_WORD"] == 6
    assert all(getattr(_lib, k) == v for k, v in h.consts.items())
    assert h.consts["RPX_FLAGS_WORD"] < _lib.DDIMX_POOL_SLOT_WORDS and RP.FLAGS == 6 and RP.KNOWN == 1
    P = c_void_p
    assert h.funcs["rpx_pool_update"] == (c_int, [P, P, P, P, P, P, P, P, P, c_int, c_int, c_longlong, P])
    assert not set(RPX) & (set(_lib._OWNER) | set(_lib._FEATURE_OWNER) | set(_lib._FEATURES_OWNER))
    assert _lib._FEATURE_DIRS_OWNER["rpx_pool_update"] == HEADER
    assert not any(name.endswith("_EXPORTS") and set(RPX) & set(getattr(_lib, name)) for name in dir(_lib))
    assert _lib.DDIMX_ABI_VERSION == 2
    assert "FEATURE_DIRS" in _lib.__doc__ and "MEMBER" in _lib.__doc__
    assert D.RestorePool is RP.RestorePool and issubclass(RP.RestorePool, D.SamplerPool)


def test_rpx_pool_update_is_bound_on_first_use_and_refuses_without_a_gpu():
    lib = _lib._Library(_lib.LIB_PATH)  # a fresh object: nothing bound yet
    assert "rpx_pool_update" not in vars(lib)
    fn = lib.rpx_pool_update
    want = _lib.FEATURE_DIRS[HEADER].funcs["rpx_pool_update"]
    assert "rpx_pool_update" in vars(lib) and (fn.restype, list(fn.argtypes)) == (want[0], want[1])
    with pytest.raises(AttributeError, match="rpx_nonesuch"):
        getattr(lib, "rpx_nonesuch")
    p = c_void_p(4096)  # never dereferenced: every call below is refused before the launch
    ok = [p] * 9

    def call(ptrs=ok, n_slots=2, max_steps=3, per_sample=8):
        rc = fn(*ptrs, n_slots, max_steps, per_sample, None)
        return rc, lib.ddimx_last_error().decode()

    for i in range(9):
        rc, msg = call(ok[:i] + [None] + ok[i + 1:])
        assert rc != 0 and "rpx_pool_update: null argument" in msg, i
    for kw, text in ((dict(n_slots=0), "n_slots"), (dict(n_slots=65536), "n_slots"), (dict(max_steps=0), "max_steps"),
                     (dict(per_sample=0), "multiple of 4"), (dict(per_sample=6), "multiple of 4"), (dict(per_sample=-4), "multiple of 4"),
                     (dict(per_sample=4 * ((1 << 32) + 1)), "2^32 groups")):
        rc, msg = call(**kw)
        assert rc != 0 and "rpx_pool_update" in msg and text in msg, (kw, msg)


def test_a_function_another_table_declares_is_refused():
    with pytest.raises(RuntimeError, match="b/rpx_b.h: rpx_g is declared in a/rpx_a.h too"):
        _lib._parse_all({"a/rpx_a.h": "int rpx_g(int n);", "b/rpx_b.h": "int rpx_g(int n);"})


@pytest.mark.skipif(shutil.which("nm") is None, reason="nm (binutils) is needed to list the library's dynamic symbols")
def test_library_defines_exactly_the_declared_rpx_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.split()}
    assert {n for n in defined if n.startswith("rpx_")} == set(RPX)


def test_the_new_sources_are_feature_sources():
    new = {"restore_pool.cpp", "restore_pool_kernels.hip"}
    assert new <= set(build.FEATURE_SOURCES) and not new & set(build.SOURCES)
    assert all(os.path.isfile(os.path.join(build.CSRC, f)) for f in new)


# ---- 5. the arithmetic ---------------------------------------------------------------------------------------------------------------------
def _data(n=4 * 37):
    rng = np.random.default_rng(5)
    x, e, m1, m2, y, z = (rng.standard_normal(n).astype(np.float32) for _ in range(6))
    m = rng.choice(np.array([0, 1, 0.25], np.float32), n)
    return x, e, m1, m2, y, m, z


@pytest.mark.parametrize("order,tau", [(1, 0.0), (2, 0.0), (3, 0.0), (3, 1.0)])
def test_fp32_restatement_against_the_float64_path(order, tau):
    a = MH.alphas()
    seq = MH.spread(8)
    rows, known = RP.restore_rows(seq, a, order, tau)
    x, e, m1, m2, y, m, z = _data()
    for k in (0, 1, 3, len(seq) - 1):
        row, (cx, w0) = rows[k], known[k]
        use1, use2, add_z = R.flags_of(row)
        nan = np.full_like(x, np.nan)
        u, m0, h = R.update32(x, e, m1 if use1 or use2 else nan, m2 if use2 else nan, y, m, row, known[k], R.KNOWN, z if add_z else None)
        plain, p0, _ = R.update32(x, e, m1 if use1 or use2 else nan, m2 if use2 else nan, None, None, row, None, 0, z if add_z else None)
        assert not np.isnan(u).any() and np.array_equal(_bits(m0), _bits(p0)), "a switched-off term's operand never enters"
        assert np.array_equal(_bits(m0), _bits(S.ddim_x0(x, e, row[1], row[2])))
        assert np.array_equal(_bits(u[m == 0]), _bits(plain[m == 0])), "outside the mask: the plain update's bits"
        kv64 = R.known64(x, y, cx, w0, row[5], z)
        # two roundings (w0 y, then the fma) and one more with noise, each at most half an ulp of a term no larger than the sum of magnitudes
        bound = 3 * 2.0 ** -24 * (abs(float(cx)) * np.abs(x) + abs(float(w0)) * np.abs(y) + abs(float(row[5])) * np.abs(z))
        assert (np.abs(u[m == 1].astype(np.float64) - kv64[m == 1]) <= bound[m == 1]).all(), k
        mix = m == 0.25
        want = 0.25 * kv64 + 0.75 * plain.astype(np.float64)
        assert (np.abs(u[mix].astype(np.float64) - want[mix]) <= 2 * bound[mix] + 3 * 2.0 ** -24 * np.abs(want[mix])).all(), k
        if k == len(seq) - 1:
            assert (float(cx), float(w0), float(row[5])) == (0.0, 1.0, 0.0)
            assert np.array_equal(R.known64(x, y, cx, w0), y.astype(np.float64)), "the float64 path returns y exactly"
            assert np.array_equal(_bits(u[m == 1]), _bits(y[m == 1])), "the final row gives y's bits where the mask is 1"


# ---- 6. the timing tool, as far as it runs without a device ------------------------------------------------------------------------------
def test_tool_parses_its_usage_line_and_refuses_without_a_gpu(monkeypatch):
    import importlib
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    timing = importlib.import_module("timing")
    mod = importlib.import_module("restore_pool_time")
    assert "usage: python tools/restore_pool_time.py [T=1024] [rounds=6] [what=abc] [n=32]" in mod.__doc__
    assert not torch.cuda.is_available(), "this module is the CPU half; tests/test_gpu_restore_pool_tool.py is the other"
    with pytest.raises(RuntimeError, match="GPU"):
        mod.main([])
    seen = []
    parse = timing.parse_args
    monkeypatch.setattr(timing, "parse_args", lambda argv, spec, flags=(): seen.append(vars(parse(argv, spec, flags))) or sys.exit("parsed"))
    for line, want in (("", dict(T=1024, rounds=6, what="abc", n=32)), ("64 1 what=b 4", dict(T=64, rounds=1, what="b", n=4))):
        with pytest.raises(SystemExit, match="parsed"):
            mod.main(line.split())
        assert seen.pop() == want
    assert not torch.cuda.is_initialized()
