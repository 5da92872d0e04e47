"""The walks that string the kernels together -- ddimx_unet_fwd, its forked form, the training forward and the three backward forms,
the FNet alone and the per-op blocks -- inside scratch whose every byte is accounted for (tests/walk_harness.py): the workspace and
the tape are exactly the size the library asks for, lie between guards, and have a gap of 4096 unused bytes behind every region
(ddimx_debug_set_carve_gap), so that a store past ANY region lands on a sentinel and not in its neighbour or in the allocator's slack.

Per case: (a) containment -- guards, gaps and rounding tails of workspace and tape keep the sentinel, the outputs' guards hold, every
input keeps its bits (the tape is an input of the backward); (b) independence -- the outputs have the same bits whether the
scratch held 0xFF, 0x00 or 0x7F bytes before the call (workspace and tape are filled with the same pattern in a run: each sees all
three; the workspace is filled again between the forward and each backward); (c) carry-over -- shape 2 after shape 1 in one
buffer gives what shape 2 gives in fresh scratch; (d) refusal -- one byte too few is refused by name before anything is written;
(e) anchor -- on the tiny config the first fill's outputs pass model_harness's gates against the CPU oracle, so the invariants
hold on walks that also compute the right thing.

Not asserted: that unwritten bytes are never LOADED.  A load whose value is discarded (unconditional load, select afterwards;
padding rows of a chunk no output depends on) is allowed; only dependence is an error, and (b) measures it.  Tape bytes are not
compared between fills (regions may hold padding that is never written); what is computed from the tape is.

Every walk is called through the C ABI, as tests/test_gpu_train.py's _fnet_setup / _fnet_run do (the training ones through
model.py's own two call helpers): the product allocates its tape inside the autograd node, where nothing can be injected.

Shapes: the smallest that reach each sizing term.  The audio config's (1, 1056) keeps its f32 leg: every case of this file, that one
included, runs in about a second or less on an MI355X."""
import ctypes

import pytest
import torch

from ddim_audio_amd import _lib, synth
from ddim_audio_amd.model import _unet_bwd, _unet_fwd_train
from oracle import ref_cpu
import gpu_util as G
import kernel_harness as KH
import model_harness as MH
import walk_harness as WH

pytestmark = pytest.mark.gpu

BF, FL = "torch.cuda.BFloat16Tensor", "torch.cuda.FloatTensor"
MODES = [(s, dt, None) for s, dt in MH.MODES] + [(BF, G.BF16, FL)]  # + mixed: bf16 convs, fp32 FNet (test_gpu_model.py builds the same)
MODE_IDS = MH.MODE_IDS + ["mixed"]
TINY_SHAPES = [(B, T) for B in (1, 2, 3, 5) for T in (4, 12, 20, 64, 132)] + [(1, 1040)]
AUDIO_SHAPES = [(1, 32), (3, 32), (2, 96), (5, 64), (1, 1056)]
CASES = [("tiny", s) for s in TINY_SHAPES] + [("audio", s) for s in AUDIO_SHAPES]
CASE_IDS = [f"{n}-B{b}-T{t}" for n, (b, t) in CASES]
FORK_MASKS = {"tiny": (0x10007,), "audio": (0x10003, 0x24, 0x1003F)}
# (shape 1, shape 2) of the carry-over runs; the first of each config grows B while T shrinks
CARRY = [("tiny", (2, 64), (5, 12)), ("tiny", (1, 132), (3, 20)), ("tiny", (5, 4), (1, 20)),
         ("audio", (2, 96), (5, 64)), ("audio", (3, 32), (1, 64))]
CARRY_IDS = [f"{n}-{a[0]}x{a[1]}-then-{b[0]}x{b[1]}" for n, a, b in CARRY]


@pytest.fixture(autouse=True)
def gap():
    with WH.carve_gap(WH.GAP):
        yield


# ---- models, inputs, the oracle ---------------------------------------------------------------------------------------------------------
_CTX = {}


class Ctx:
    """One eval-mode model of a config and mode behind the C ABI: handle, packed weights (inference copies included) and the
    backward's packing, each with a snapshot of its bits."""

    def __init__(self, name, mode):
        dtype_str, self.dt, fnet = mode
        self.name, self.dev, self.lib = name, G.dev(), _lib.load()
        self.cfg, self.m = MH.build(name, dtype_str, 5, mode="eval", fnet=fnet)
        m = self.m
        lib = m._ensure_handle()
        with torch.cuda.device(self.dev):
            m._ensure_packed(lib, self.dev)
            m._ensure_packed_bwd(lib, self.dev)
        torch.cuda.synchronize()
        self.h = m._handle
        self.frozen = [WH.Frozen(m._packed), WH.Frozen(m._packed_bwd), WH.Frozen(m._temb_table)]
        self.levels = len(m.config.ch)
        self.width = m.config.ch[-1] * (m.config.f_size >> (self.levels - 1))
        self.grad_total, self.grad_layout = m._grad_layout(self.lib)
        self._tab = {}

    def tables(self, T):
        """(the three tables as the model builds them, their snapshots) for T; kept here, the model keeps only the latest."""
        if T not in self._tab:
            with torch.cuda.device(self.dev):
                tabs = self.m._ensure_tables(T, self.dev)
            self._tab[T] = (tabs, [WH.Frozen(v) for v in tabs])
        return self._tab[T]

    def struct(self, T, temb=False):
        tabs = self.tables(T)[0]
        return _lib.DdimxTables(*(v.data_ptr() for v in tabs), self.m._temb_table.data_ptr() if temb else None)

    def inputs_unchanged(self, T, what, *ros):
        for f in self.frozen + self.tables(T)[1]:
            f.check(what)
        for r in ros:
            r.check(what)

    def layout(self, which, B, T):
        regions, total = WH.layout(self.h, which, B, T, WH.GAP)
        export = {WH.WORKSPACE: self.lib.ddimx_workspace_bytes, WH.TRAIN_WORKSPACE: self.lib.ddimx_train_workspace_bytes,
                  WH.TAPE: self.lib.ddimx_train_tape_bytes}[which]
        assert total == export(self.h, B, T)
        WH.check_layout(regions, total, WH.GAP, f"layout {which}")
        return regions, total

    def scratch(self, which, B, T):
        return WH.Scratch(*self.layout(which, B, T))


def ctx(name, mode):
    key = (name, MODE_IDS[MODES.index(mode)])
    if key not in _CTX:
        _CTX[key] = Ctx(name, mode)
    return _CTX[key]


def net_inputs(c, B, T):
    shape = (B, c.m.config.channels, T, c.m.config.f_size)
    x = KH.Ro(synth.gaussian(f"walk.x.{B}.{T}", shape))
    t = KH.Ro(torch.tensor([(37 + 211 * b) % 1000 for b in range(B)]), torch.int64)
    d_eps = KH.Ro(synth.gaussian(f"walk.d.{B}.{T}", shape))
    return x, t, d_eps


_ORACLE = {}


def oracle(c, B, T):
    """eps, d x and every parameter gradient of sum(eps * d_eps) of the tiny network at (B, T) through the CPU oracle: once per
    shape (the three modes share the fp32 parameters), never changed."""
    if (B, T) not in _ORACLE:
        x, t, d_eps = (r.keep.cpu() for r in net_inputs(c, B, T))
        live, ocfg = MH.oracle(c.m, "tiny")
        xr = x.clone().requires_grad_(True)
        eps = ref_cpu.model_forward(live, ocfg, xr, t)
        eps.backward(d_eps)
        _ORACLE[(B, T)] = {"eps": eps.detach(), "d_x": xr.grad, "grads": {k: v.grad for k, v in live.items() if k != "temb.te"}}
    return _ORACLE[(B, T)]


def gate_grads(c, flat, ref, what):
    """model_harness.backward_case's gate on a flat gradient buffer: each tensor's worst element within 2e-3 (fp32) / 0.6 (bf16) of
    the tensor's own RMS gradient (floor: a 1e-4 share of the global norm)."""
    flat = flat.cpu()
    total = sum(float(g.double().square().sum()) for g in ref.values()) ** 0.5
    for (pname, _), (off, numel, shape) in zip(c.m.named_parameters(), c.grad_layout):
        want = ref[pname]
        got = flat[off:off + numel].view(shape)
        scale = max(float(want.double().square().mean().sqrt()), 1e-4 * total / want.numel() ** 0.5)
        err = float((got - want).abs().max()) / scale
        assert err <= (2e-3 if c.dt == G.F32 else 0.6), f"{what} {pname}: {err:.3e} x rms"


# ---- the walks ----------------------------------------------------------------------------------------------------------------------------
def unet_fwd(c, ws, ws_bytes, x, t, eps, B, T, mask=None):
    """ddimx_unet_fwd over the embedding table (the product's eval path), or ddimx_unet_fwd_forked with `mask` and the timestep MLP."""
    if mask is None:
        tb = c.struct(T, temb=True)
        return c.lib.ddimx_unet_fwd(c.h, _lib.ptr(c.m._packed), ctypes.byref(tb), ws.ptr, ws_bytes, x.ptr, t.ptr, eps.ptr, B, T, _lib.stream())
    tb = c.struct(T)
    with torch.cuda.device(c.dev):
        fc = c.m._eager_context(c.dev)
    return c.lib.ddimx_unet_fwd_forked(c.h, _lib.ptr(c.m._packed), ctypes.byref(tb), ws.ptr, ws_bytes, x.ptr, t.ptr, eps.ptr, B, T,
                                       _lib.stream(), ctypes.c_void_p(fc.aux_handle), fc.event_array(), len(fc.events), mask)


def infer_walk(c, B, T, mask=None):
    """Containment and independence of one inference walk; returns the first fill's eps (device)."""
    ws = c.scratch(WH.WORKSPACE, B, T)
    x, t, _ = net_inputs(c, B, T)
    what = f"{c.name} unet_fwd B={B} T={T} mask={mask}"

    def run(pattern):
        ws.fill(pattern)
        eps = KH.Out(x.t.numel())
        _lib.check(unet_fwd(c, ws, ws.total, x, t, eps, B, T, mask))
        KH.sync()
        ws.check(f"{what} fill 0x{pattern:02X}: workspace")
        c.inputs_unchanged(T, what, x, t)
        return {"eps": WH.body(eps, what + ": eps")}
    return WH.under_fills(run, what)["eps"]


BWD_FORMS = ("staged", "forked", "ex", "ex-data-only")


def unet_bwd(c, form, ws, tape, x, t, d_eps, T, p, seed):
    """One backward form over the tape: (flat gradient Out or None, d_x Out or None)."""
    grads = None if form == "ex-data-only" else KH.Out(c.grad_total)
    d_x = KH.Out(x.t.numel()) if form.startswith("ex") else None
    kw = {}
    with torch.cuda.device(c.dev):
        if form == "staged":  # with its three bucket events: the deferred batch sums are flushed in the middle of the walk
            kw["events"] = [torch.cuda.Event() for _ in range(3)]
            for e in kw["events"]:
                e.record()
        if form == "forked":
            kw["side"] = c.m._eager_bwd_context(c.dev)
        _unet_bwd(c.m, c.tables(T)[0], ws.t, tape.t, x.t, t.t, d_eps.t, None if grads is None else grads.body, p, seed,
                  d_x=None if d_x is None else d_x.body, data_only=form == "ex-data-only", **kw)
    KH.sync()
    return grads, d_x


def train_walk(c, B, T, p=0.0, seed=0, forms=BWD_FORMS):
    """Containment and independence of ddimx_unet_fwd_train followed by each backward form; returns the first fill's outputs."""
    ws, tape = c.scratch(WH.TRAIN_WORKSPACE, B, T), c.scratch(WH.TAPE, B, T)
    x, t, d_eps = net_inputs(c, B, T)
    what = f"{c.name} train B={B} T={T} p={p}"

    def run(pattern):
        w = f"{what} fill 0x{pattern:02X}"
        ws.fill(pattern)
        tape.fill(pattern)
        eps = KH.Out(x.t.numel())
        with torch.cuda.device(c.dev):
            _unet_fwd_train(c.m, c.tables(T)[0], ws.t, tape.t, x.t, t.t, eps.body, p, seed)
        KH.sync()
        ws.check(w + ": workspace after the forward")
        tape.check(w + ": tape after the forward")
        c.inputs_unchanged(T, w, x, t)
        out = {"eps": WH.body(eps, w + ": eps")}
        keep = tape.snapshot()
        for form in forms:
            ws.fill(pattern)
            grads, d_x = unet_bwd(c, form, ws, tape, x, t, d_eps, T, p, seed)
            ws.check(f"{w}: workspace after bwd {form}")
            tape.unchanged(keep, f"{w}: bwd {form}")
            c.inputs_unchanged(T, w, x, t, d_eps)
            if grads is not None:
                out[form + ".grads"] = WH.body(grads, f"{w}: bwd {form} gradients")
            if d_x is not None:
                out[form + ".d_x"] = WH.body(d_x, f"{w}: bwd {form} d_x")
        return out
    first = WH.under_fills(run, what)
    # what include/ddimx.h promises of the forms: the same gradients bit for bit, the data-only d_x that of the full backward
    for form in forms[1:]:
        if form + ".grads" in first:
            KH.same(first[form + ".grads"], first[forms[0] + ".grads"], f"{what}: gradients of bwd {form} against {forms[0]}")
    if "ex-data-only.d_x" in first and "ex.d_x" in first:
        KH.same(first["ex-data-only.d_x"], first["ex.d_x"], f"{what}: data-only d_x")
    return first


# ---- the whole network ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, shape", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_unet_fwd(mode, name, shape):
    c = ctx(name, mode)
    B, T = shape
    eps = infer_walk(c, B, T)
    if B >= 3 and B % 2:  # shard 1 is the larger one; the result is the unforked one for every mask
        for mask in FORK_MASKS[name]:
            KH.same(infer_walk(c, B, T, mask), eps, f"forked 0x{mask:X} against unforked")
    if name == "tiny":
        mx, er = MH.gate(eps.view(B, -1), oracle(c, B, T)["eps"].view(B, -1), c.dt, f"eps B={B} T={T}")
        print(f"[walk scratch unet_fwd tiny {shape}] max {mx:.2e} rms {er:.2e} x rms")


@pytest.mark.parametrize("name, shape", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_unet_train_pair(mode, name, shape):
    c = ctx(name, mode)
    B, T = shape
    first = train_walk(c, B, T)
    if name == "tiny":
        ref = oracle(c, B, T)
        MH.gate(first["eps"].view(B, -1), ref["eps"].view(B, -1), c.dt, f"training eps B={B} T={T}")
        MH.gate(first["ex.d_x"].view(B, -1), ref["d_x"].view(B, -1), c.dt, f"d_x B={B} T={T}")
        gate_grads(c, first["staged.grads"], ref["grads"], f"B={B} T={T}")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_unet_train_pair_with_dropout(mode):
    """p > 0 with a fixed seed: the masks are a function of (seed, layer, element), so nothing of (a), (b) changes."""
    c = ctx("tiny", mode)
    first = train_walk(c, 3, 20, p=0.25, seed=0x5EED)
    plain = train_walk(c, 3, 20, forms=("ex",))
    assert not torch.equal(first["eps"], plain["eps"]), "dropout was on"
    assert bool(torch.isfinite(first["eps"]).all()) and bool(torch.isfinite(first["ex.d_x"]).all())


@pytest.mark.parametrize("name, s1, s2", CARRY, ids=CARRY_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_carry_over(mode, name, s1, s2):
    """Shape 1, then shape 2, in one buffer of the larger size (what Model.reserve and _train_ws keep between calls): shape 2's
    outputs are those of fresh, 0xFF-filled scratch of its own size."""
    c = ctx(name, mode)
    # inference
    big = KH.Out(max(c.layout(WH.WORKSPACE, *s)[1] for s in (s1, s2)), torch.uint8)
    got = None
    for B, T in (s1, s2):
        x, t, _ = net_inputs(c, B, T)
        eps = KH.Out(x.t.numel())
        _lib.check(unet_fwd(c, big, big.nbytes, x, t, eps, B, T))
        KH.sync()
        got = WH.body(eps, "eps")
    WH.body(big, "the shared workspace")  # (its guards)
    B, T = s2
    ws = c.scratch(WH.WORKSPACE, B, T).fill(0xFF)
    x, t, d_eps = net_inputs(c, B, T)
    eps = KH.Out(x.t.numel())
    _lib.check(unet_fwd(c, ws, ws.total, x, t, eps, B, T))
    KH.sync()
    KH.same(got, WH.body(eps, "eps"), f"eps of {s2} after {s1}")
    # the training pair
    bigw = KH.Out(max(c.layout(WH.TRAIN_WORKSPACE, *s)[1] for s in (s1, s2)), torch.uint8)
    bigt = KH.Out(max(c.layout(WH.TAPE, *s)[1] for s in (s1, s2)), torch.uint8)

    def pair(wsb, tpb, B, T):
        x, t, d_eps = net_inputs(c, B, T)
        eps, grads, d_x = KH.Out(x.t.numel()), KH.Out(c.grad_total), KH.Out(x.t.numel())
        with torch.cuda.device(c.dev):
            _unet_fwd_train(c.m, c.tables(T)[0], wsb, tpb, x.t, t.t, eps.body)
            _unet_bwd(c.m, c.tables(T)[0], wsb, tpb, x.t, t.t, d_eps.t, grads.body, d_x=d_x.body)
        KH.sync()
        return [WH.body(o, n) for o, n in ((eps, "eps"), (grads, "gradients"), (d_x, "d_x"))]
    for B, T in (s1, s2):
        got = pair(bigw.body, bigt.body, B, T)
    WH.body(bigw, "the shared training workspace")
    WH.body(bigt, "the shared tape")
    B, T = s2
    want = pair(c.scratch(WH.TRAIN_WORKSPACE, B, T).fill(0xFF).t, c.scratch(WH.TAPE, B, T).fill(0xFF).t, B, T)
    for g, w, n in zip(got, want, ("eps", "gradients", "d_x")):
        KH.same(g, w, f"training {n} of {s2} after {s1}")


@pytest.mark.parametrize("name, shape", [("tiny", (5, 20)), ("audio", (5, 64))], ids=["tiny", "audio"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_the_product_path_on_injected_scratch(mode, name, shape):
    """Model.forward itself -- the forked eval forward of B >= 4, and the tape-keeping node with its forked backward -- on a
    workspace slot and a training workspace of exactly the needed size (the tape is the node's own allocation): contained,
    independent of the fill, and the same bits as the C-ABI walks above."""
    c = ctx(name, mode)
    m, (B, T) = c.m, shape
    ws, tws = c.scratch(WH.WORKSPACE, B, T), c.scratch(WH.TRAIN_WORKSPACE, B, T)
    x, t, d_eps = net_inputs(c, B, T)
    what = f"{name} Model.forward B={B} T={T}"
    saved = (m._workspace, getattr(m, "_train_ws", None))

    def run(pattern):
        w = f"{what} fill 0x{pattern:02X}"
        ws.fill(pattern)
        tws.fill(pattern)
        WH.inject(m, workspace=ws, train_ws=tws)
        with torch.no_grad():
            eps = m(x.t, t.t)
        KH.sync()
        ws.check(w + ": workspace after the eval forward")
        xg = x.t.clone().requires_grad_(True)
        y = m(xg, t.t)
        y.backward(d_eps.t)
        KH.sync()
        assert WH.injected(m, workspace=ws, train_ws=tws), "the model re-allocated its scratch"
        ws.check(w + ": workspace after the training node")
        tws.check(w + ": training workspace")
        c.inputs_unchanged(T, w, x, t, d_eps)
        grads = torch.cat([p.grad.reshape(-1) for p in m.parameters()])
        for p in m.parameters():
            p.grad = None
        return {"eps": eps.reshape(-1).clone(), "train.eps": y.detach().reshape(-1).clone(), "d_x": xg.grad.reshape(-1).clone(), "grads": grads}
    try:
        first = WH.under_fills(run, what)
    finally:
        m._workspace, m._train_ws = saved
        for p in m.parameters():
            p.grad = None
    KH.same(first["eps"], infer_walk(c, B, T), f"{what}: eps against ddimx_unet_fwd")
    abi = train_walk(c, B, T, forms=("ex",))
    KH.same(first["train.eps"], abi["eps"], f"{what}: training eps against ddimx_unet_fwd_train")
    KH.same(first["d_x"], abi["ex.d_x"], f"{what}: d_x against ddimx_unet_bwd_ex")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_control_a_region_claimed_one_byte_short(mode):
    """The containment check sees the kernels' own stores: region 3 of the inference workspace and of the tape is the input conv's
    output, written to its last element by every walk.  With a region table that claims one byte less for it, the walk's last byte
    is a stray one, and `check` names that region; with the true table the same walk passes (test_unet_fwd, test_unet_train_pair)."""
    c = ctx("tiny", mode)
    B, T = 3, 20
    x, t, _ = net_inputs(c, B, T)
    act_bytes = B * T * c.m.config.f_size * c.m.config.ch[0] * c.m._act_dtype.itemsize
    for which in (WH.WORKSPACE, WH.TAPE):
        regions, total = c.layout(which, B, T)
        off, size = regions[3]
        assert size == act_bytes, "region 3 is hidden[0]"
        s = WH.Scratch(regions[:3] + [(off, size - 1)] + regions[4:], total).fill(0x00)
        eps = KH.Out(x.t.numel())
        if which == WH.WORKSPACE:
            _lib.check(unet_fwd(c, s, total, x, t, eps, B, T))
        else:
            ws = c.scratch(WH.TRAIN_WORKSPACE, B, T).fill(0x00)
            with torch.cuda.device(c.dev):
                _unet_fwd_train(c.m, c.tables(T)[0], ws.t, s.t, x.t, t.t, eps.body)
        KH.sync()
        with pytest.raises(AssertionError, match=rf"control: 1 bytes outside the regions were written, the first at {off + size - 1}: byte 0 behind region 3 "):
            s.check("control")


@pytest.mark.parametrize("name, shape", [("tiny", (3, 20)), ("audio", (3, 32))], ids=["tiny", "audio"])
def test_one_byte_too_few_is_refused(name, shape):
    c = ctx(name, MODES[0])
    lib, B, T = c.lib, *shape
    x, t, d_eps = net_inputs(c, B, T)
    ws, tws, tape = (c.scratch(w, B, T) for w in (WH.WORKSPACE, WH.TRAIN_WORKSPACE, WH.TAPE))
    eps, grads, d_x = KH.Out(x.t.numel()), KH.Out(c.grad_total), KH.Out(x.t.numel())
    bufs = (ws.out, tws.out, tape.out, eps, grads, d_x)
    KH.refused(unet_fwd(c, ws, ws.total - 1, x, t, eps, B, T), *bufs, who="ddimx_unet_fwd")
    KH.refused(unet_fwd(c, ws, ws.total - 1, x, t, eps, B, T, FORK_MASKS[name][0]), *bufs, who="ddimx_unet_fwd")
    tb = c.struct(T)
    pk, pkb, st = _lib.ptr(c.m._packed), _lib.ptr(c.m._packed_bwd), _lib.stream()
    for wb, tpb, short in ((tws.total - 1, tape.total, "workspace"), (tws.total, tape.total - 1, "tape")):
        rc = lib.ddimx_unet_fwd_train(c.h, pk, ctypes.byref(tb), tws.ptr, wb, tape.ptr, tpb, x.ptr, t.ptr, eps.ptr, B, T, 0.0, 0, st)
        KH.refused(rc, *bufs, who="ddimx_unet_fwd_train: " + short)
        for flags, g in ((0, grads.ptr), (_lib.DDIMX_BWD_DATA_ONLY, None)):
            rc = lib.ddimx_unet_bwd_ex(c.h, pk, pkb, ctypes.byref(tb), tws.ptr, wb, tape.ptr, tpb, x.ptr, t.ptr, d_eps.ptr, g, B, T, 0.0, 0,
                                       None, 0, st, None, None, 0, d_x.ptr, flags)
            KH.refused(rc, *bufs, who="ddimx_unet_bwd: " + short)
        rc = lib.ddimx_unet_bwd_staged(c.h, pk, pkb, ctypes.byref(tb), tws.ptr, wb, tape.ptr, tpb, x.ptr, t.ptr, d_eps.ptr, grads.ptr, B, T,
                                       0.0, 0, None, 0, st)
        KH.refused(rc, *bufs, who="ddimx_unet_bwd: " + short)
        with torch.cuda.device(c.dev):
            fc = c.m._eager_bwd_context(c.dev)
        rc = lib.ddimx_unet_bwd_forked(c.h, pk, pkb, ctypes.byref(tb), tws.ptr, wb, tape.ptr, tpb, x.ptr, t.ptr, d_eps.ptr, grads.ptr, B, T,
                                       0.0, 0, None, 0, st, ctypes.c_void_p(fc.aux_handle), fc.event_array(), len(fc.events))
        KH.refused(rc, *bufs, who="ddimx_unet_bwd: " + short)
        tok, out, d_out, _ = fnet_inputs(c, B, T)
        rc = lib.ddimx_fnet_fwd_train(c.h, pk, ctypes.byref(tb), tws.ptr, wb, tape.ptr, tpb, tok.ptr, out.ptr, B, T, 0.0, 0, st)
        KH.refused(rc, out, *bufs, who="ddimx_fnet_fwd_train: " + short)
        rc = lib.ddimx_fnet_bwd(c.h, pk, pkb, ctypes.byref(tb), tws.ptr, wb, tape.ptr, tpb, tok.ptr, d_out.ptr, out.ptr, grads.ptr, B, T, 0.0, 0, st)
        KH.refused(rc, out, *bufs, who="ddimx_fnet_bwd: " + short)
    tok, out, _, _ = fnet_inputs(c, B, T)
    rc = lib.ddimx_fnet_fwd(c.h, pk, ctypes.byref(tb), ws.ptr, ws.total - 1, tok.ptr, out.ptr, B, T, st)
    KH.refused(rc, out, *bufs, who="ddimx_fnet_fwd: workspace")
    c.inputs_unchanged(T, "refusals", x, t, d_eps, tok)


# ---- the FNet alone -----------------------------------------------------------------------------------------------------------------------
def fnet_inputs(c, B, T):
    """(tokens in the activation dtype [B][S][Fr][C], a guarded output [B * S][width] fp32, its gradient, S)"""
    S = T >> (c.levels - 1)
    tok = KH.Ro(synth.gaussian(f"walk.tok.{B}.{S}", (B * S, c.width)), c.m._act_dtype)
    d_out = KH.Ro(synth.gaussian(f"walk.dtok.{B}.{S}", (B * S, c.width)))
    return tok, KH.Out(B * S * c.width), d_out, S


@pytest.mark.parametrize("name, shape", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_fnet_walks(mode, name, shape):
    """ddimx_fnet_fwd on the inference workspace; ddimx_fnet_fwd_train + ddimx_fnet_bwd on the training workspace and the tape."""
    c = ctx(name, mode)
    lib, (B, T) = c.lib, shape
    pk, pkb = _lib.ptr(c.m._packed), _lib.ptr(c.m._packed_bwd)
    tb = c.struct(T)
    ws, tws, tape = (c.scratch(w, B, T) for w in (WH.WORKSPACE, WH.TRAIN_WORKSPACE, WH.TAPE))
    tok, _, d_out, S = fnet_inputs(c, B, T)
    n = B * S * c.width
    what = f"{c.name} fnet B={B} T={T}"

    def run(pattern):
        w = f"{what} fill 0x{pattern:02X}"
        ws.fill(pattern)
        out = KH.Out(n)
        _lib.check(lib.ddimx_fnet_fwd(c.h, pk, ctypes.byref(tb), ws.ptr, ws.total, tok.ptr, out.ptr, B, T, _lib.stream()))
        KH.sync()
        ws.check(w + ": workspace")
        res = {"out": WH.body(out, w + ": out")}
        tws.fill(pattern)
        tape.fill(pattern)
        out = KH.Out(n)
        _lib.check(lib.ddimx_fnet_fwd_train(c.h, pk, ctypes.byref(tb), tws.ptr, tws.total, tape.ptr, tape.total, tok.ptr, out.ptr, B, T,
                                            0.0, 0, _lib.stream()))
        KH.sync()
        tws.check(w + ": training workspace after the forward")
        tape.check(w + ": tape after the forward")
        res["train.out"] = WH.body(out, w + ": training out")
        keep = tape.snapshot()
        tws.fill(pattern)
        d_x, grads = KH.Out(n), KH.Out(c.grad_total)
        _lib.check(lib.ddimx_fnet_bwd(c.h, pk, pkb, ctypes.byref(tb), tws.ptr, tws.total, tape.ptr, tape.total, tok.ptr, d_out.ptr, d_x.ptr,
                                      grads.ptr, B, T, 0.0, 0, _lib.stream()))
        KH.sync()
        tws.check(w + ": training workspace after the backward")
        tape.unchanged(keep, w + ": fnet_bwd")
        c.inputs_unchanged(T, w, tok, d_out)
        res["d_x"], res["grads"] = WH.body(d_x, w + ": d_x"), WH.body(grads, w + ": gradients")
        return res
    first = WH.under_fills(run, what)
    assert all(bool(torch.isfinite(first[k]).all()) for k in ("out", "train.out", "d_x"))


# ---- the per-op blocks on their own workspaces ----------------------------------------------------------------------------------------------
# one ragged and one whole-tile shape per width, from the tables of exact_cases.py: (C, (B, H, W) ragged, (B, H, W) whole tiles)
RB_SHAPES = [(32, (3, 13, 20), (2, 8, 32)), (64, (1, 4, 8), (2, 16, 64)), (96, (3, 13, 20), (2, 16, 32)), (128, (3, 13, 20), (2, 8, 64)),
             (192, (1, 4, 8), (2, 8, 32)), (256, (3, 13, 20), (2, 8, 16))]
RB_CASES = [(C, s) for C, ragged, whole in RB_SHAPES for s in (ragged, whole)]
# Downsample cbig -> csmall at its input size (its backward; the Upsample backward runs the mirrored shapes on the same workspace)
DU_CASES = [(32, 64, (1, 26, 40)), (32, 64, (2, 32, 64)), (64, 96, (1, 4, 8)), (64, 96, (2, 16, 64)), (96, 128, (1, 4, 8)), (96, 128, (2, 16, 32)),
            (128, 192, (1, 4, 8)), (128, 192, (2, 16, 32)), (192, 256, (1, 4, 8)), (192, 256, (2, 8, 32))]
DTS = [G.F32, G.BF16]
DT_IDS = ["f32", "bf16"]


def op_scratch(which, dt, B, C, Cbig, H, W, export):
    regions, total = WH.op_layout(which, dt, B, C, Cbig, H, W, WH.GAP)
    assert total == export
    WH.check_layout(regions, total, WH.GAP, f"op layout {which}")
    return WH.Scratch(regions, total)


def act(tag, shape, dt):
    return KH.Ro(synth.gaussian(tag, shape), G.TORCH_DT[dt])


@pytest.mark.parametrize("C, shape", RB_CASES, ids=[f"C{C}-{b}x{h}x{w}" for C, (b, h, w) in RB_CASES])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_resblock_walks(dt, C, shape):
    """ddimx_resblock_fwd, and ddimx_resblock_fwd_train + ddimx_resblock_bwd, on ddimx_op_workspace_bytes /
    ddimx_resblock_bwd_workspace_bytes."""
    lib = _lib.load()
    B, H, W = shape
    sd = MH.rb_sd("b.", C)
    k = {n: KH.Ro(sd["b." + n]) for n in ("norm.0.weight", "norm.0.bias", "norm.1.weight", "norm.1.bias", "norm.2.weight", "conv.1.bias")}
    w0, w1 = (WH.Frozen(G.pack_conv(sd[f"b.conv.{i}.weight"], dt)) for i in (0, 1))
    wd0, wd1 = (WH.Frozen(G.pack_conv_dgrad(sd[f"b.conv.{i}.weight"], dt)) for i in (0, 1))
    x, dy = act(f"walk.rb.x.{C}", (B, H, W, C), dt), act(f"walk.rb.dy.{C}", (B, H, W, C), dt)
    temb = KH.Ro(synth.gaussian(f"walk.rb.temb.{C}", (B, C)))
    n, es = B * H * W * C, G.TORCH_DT[dt]
    ws = op_scratch(WH.OP_RESBLOCK, dt, B, C, C, H, W, lib.ddimx_op_workspace_bytes(dt, B, C, H, W))
    bws = op_scratch(WH.OP_RESBLOCK_BWD, dt, B, C, C, H, W, lib.ddimx_resblock_bwd_workspace_bytes(dt, B, C, H, W))
    small_n = int(lib.ddimx_rb_tape_floats(B, C))
    what = f"resblock C={C} {shape}"
    ptr = lambda t: _lib.ptr(t.t)  # noqa: E731
    gshapes = {"norm.0.weight": C, "norm.0.bias": C, "conv.0.weight": 9 * C * C, "norm.1.weight": C, "norm.1.bias": C, "conv.1.weight": 9 * C * C,
               "conv.1.bias": C, "norm.2.weight": C}

    def run(pattern):
        w = f"{what} fill 0x{pattern:02X}"
        st = _lib.stream()
        common = lambda: (ptr(k["norm.0.weight"]), ptr(k["norm.0.bias"]), ptr(w0), ptr(k["norm.1.weight"]), ptr(k["norm.1.bias"]),  # noqa: E731
                          ptr(w1), ptr(k["conv.1.bias"]), ptr(k["norm.2.weight"]))
        ws.fill(pattern)
        y = KH.Out(n, es)
        _lib.check(lib.ddimx_resblock_fwd(dt, C, x.ptr, y.ptr, temb.ptr, C, *common(), ws.ptr, B, H, W, st))
        KH.sync()
        ws.check(w + ": workspace after ddimx_resblock_fwd")
        res = {"y": WH.body(y, w + ": y")}
        ws.fill(pattern)
        y, u1, u2, small = KH.Out(n, es), KH.Out(n, es), KH.Out(n, es), KH.Out(small_n)
        _lib.check(lib.ddimx_resblock_fwd_train(dt, C, x.ptr, y.ptr, temb.ptr, C, *common(), u1.ptr, u2.ptr, small.ptr, ws.ptr, B, H, W, st))
        KH.sync()
        ws.check(w + ": workspace after ddimx_resblock_fwd_train")
        res["train.y"] = WH.body(y, w + ": training y")
        tape = [WH.Frozen(o.t) for o in (u1, u2, small)]  # (whole allocations: their guards are part of the snapshot)
        assert all(o.untouched() is False for o in (u1, u2, small))
        bws.fill(pattern)
        dx, dtemb = KH.Out(n, es), KH.Out(B * C)
        g = {name: KH.Out(numel) for name, numel in gshapes.items()}
        _lib.check(lib.ddimx_resblock_bwd(dt, C, x.ptr, u1.ptr, u2.ptr, small.ptr, dy.ptr, dx.ptr, ptr(k["norm.0.weight"]), ptr(k["norm.1.weight"]),
                                          ptr(k["norm.2.weight"]), ptr(wd0), ptr(wd1), *[g[name].ptr for name in gshapes], dtemb.ptr, C,
                                          bws.ptr, B, H, W, st))
        KH.sync()
        bws.check(w + ": workspace after ddimx_resblock_bwd")
        for f in tape + [w0, w1, wd0, wd1]:
            f.check(w)
        for r in list(k.values()) + [x, dy, temb]:
            r.check(w)
        res["dx"], res["dtemb"] = WH.body(dx, w + ": dx"), WH.body(dtemb, w + ": dtemb")
        for name, o in g.items():
            res["d." + name] = WH.body(o, f"{w}: d {name}")
        return res
    first = WH.under_fills(run, what)
    assert all(bool(torch.isfinite(v.float()).all()) for v in first.values())


@pytest.mark.parametrize("cbig, csmall, shape", DU_CASES, ids=[f"{a}to{b}-{s[0]}x{s[1]}x{s[2]}" for a, b, s in DU_CASES])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_downup_backward_walks(dt, cbig, csmall, shape):
    """ddimx_downsample_bwd (cbig -> csmall, input B x H x W) and ddimx_upsample_add_bwd (csmall -> cbig, input B x H/2 x W/2) on
    ddimx_downup_bwd_workspace_bytes."""
    lib = _lib.load()
    B, H, W = shape
    Hs, Ws = H // 2, W // 2
    sd = synth.fill_state_dict({"d.conv.weight": torch.empty(csmall, cbig, 4, 4), "u.conv.weight": torch.empty(csmall, cbig, 4, 4)})
    tdt = G.TORCH_DT[dt]
    wd = torch.empty(2 * 6 * 2 * cbig * csmall, dtype=tdt, device=G.dev())  # the Downsample's data gradient is an Upsample
    _lib.check(lib.ddimx_pack_convT(dt, _lib.ptr(G.g(sd["d.conv.weight"])), _lib.ptr(wd), csmall, cbig, _lib.stream()))
    wd, wu = WH.Frozen(wd), WH.Frozen(G.pack_conv(sd["u.conv.weight"], dt))  # ... and the Upsample's a Downsample
    big = lambda tag: act(f"walk.du.{tag}.{cbig}", (B, H, W, cbig), dt)  # noqa: E731
    small = lambda tag: act(f"walk.du.{tag}.{csmall}", (B, Hs, Ws, csmall), dt)  # noqa: E731
    x_d, dy_d, add = big("xd"), small("dyd"), big("add")
    x_u, dy_u = small("xu"), big("dyu")
    ws = op_scratch(WH.OP_DOWNUP_BWD, dt, B, csmall, cbig, Hs, Ws, lib.ddimx_downup_bwd_workspace_bytes(dt, csmall, cbig, B, Hs, Ws))
    what = f"down/up bwd {cbig}<->{csmall} {shape}"
    nb, ns, nw = B * H * W * cbig, B * Hs * Ws * csmall, 16 * cbig * csmall

    def run(pattern):
        w = f"{what} fill 0x{pattern:02X}"
        ws.fill(pattern)
        dx, d_w, d_b = KH.Out(nb, tdt), KH.Out(nw), KH.Out(csmall)
        _lib.check(lib.ddimx_downsample_bwd(dt, cbig, csmall, x_d.ptr, dy_d.ptr, _lib.ptr(wd.t), add.ptr, dx.ptr, d_w.ptr, d_b.ptr, ws.ptr,
                                            B, H, W, _lib.stream()))
        KH.sync()
        ws.check(w + ": workspace after ddimx_downsample_bwd")
        res = {"down.dx": WH.body(dx, w + ": down dx"), "down.d_w": WH.body(d_w, w + ": down d_w"), "down.d_b": WH.body(d_b, w + ": down d_b")}
        ws.fill(pattern)
        dx, d_w, d_b = KH.Out(ns, tdt), KH.Out(nw), KH.Out(cbig)
        _lib.check(lib.ddimx_upsample_add_bwd(dt, csmall, cbig, x_u.ptr, dy_u.ptr, _lib.ptr(wu.t), dx.ptr, d_w.ptr, d_b.ptr, ws.ptr, B, Hs, Ws,
                                              _lib.stream()))
        KH.sync()
        ws.check(w + ": workspace after ddimx_upsample_add_bwd")
        res.update({"up.dx": WH.body(dx, w + ": up dx"), "up.d_w": WH.body(d_w, w + ": up d_w"), "up.d_b": WH.body(d_b, w + ": up d_b")})
        for f in (wd, wu):
            f.check(w)
        for r in (x_d, dy_d, add, x_u, dy_u):
            r.check(w)
        return res
    first = WH.under_fills(run, what)
    assert all(bool(torch.isfinite(v.float()).all()) for v in first.values())
