"""The wiring of the inference path: every parameter is read where the reference reads it, from a copy built from that parameter.

1. ddimx_pack_fnet_inference writes every derived region (fragment-order conv copies, folded FNet copies and their tables) from the
   right source, bit for bit, and nothing else -- the regions are found differentially, from what changes when one source changes;
2. every parameter, one at a time, through the walk, against the CPU oracle's response to the same replacement (tests/wiring_ref.py):
   the output's bits change, its change projects onto the oracle's with c in [0.5, 1.5], and the whole-network gate still passes;
3. after ddimx_pack_weights alone the derived copies are stale and must not be read."""
import ctypes
import time

import pytest
import torch

import exact_util as X
import gpu_util as G
import model_harness as H
import wiring_ref as W
from ddim_audio_amd import _lib, synth

pytestmark = pytest.mark.gpu

F32T, BF16T = "torch.cuda.FloatTensor", "torch.cuda.BFloat16Tensor"
MODES = {"f32": (F32T, None, G.F32), "bf16": (BF16T, None, G.BF16), "mixed": (BF16T, F32T, G.BF16)}  # convs, FNet, the gate's dtype
GUARD = 4096
FILL = 0xA5

_MODELS = {}
_REFS = {}


def _model(net, mode):
    """(cfg, eval-mode model) of the network in the mode, seed 5 (the same weights in every mode), once per process."""
    if (net, mode) not in _MODELS:
        act, fnet, _ = MODES[mode]
        _MODELS[net, mode] = H.build(net, act, 5, mode="eval", fnet=fnet)
    return _MODELS[net, mode]


def _refs(case, m, names):
    """The oracle's side of a case, shared by the modes: (cache of wiring_ref.oracle_responses, holding at least ``names``)."""
    net = W.CASES[case]["net"]
    if case not in _REFS:
        live, ocfg = H.oracle(m, net)
        _REFS[case] = ({k: v.detach() for k, v in live.items()}, W.case_forward(case, ocfg), {})
    sd, fwd, cache = _REFS[case]
    return W.oracle_responses(fwd, sd, names, W.AMP[case], cache)


# =========================================================================================================================================
# 1. the derived regions of the packed buffer
# =========================================================================================================================================
def _al256(n):
    return (n + 255) & ~255


def _param_pack(lib, h, i):
    kind, off, nbytes, dims = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong(), (ctypes.c_int * 4)()
    _lib.check(lib.ddimx_debug_param_pack(h, i, ctypes.byref(kind), ctypes.byref(off), ctypes.byref(nbytes), dims))
    return kind.value, off.value, nbytes.value, tuple(dims)


class _Guarded:
    """A device byte buffer of FILL between two guards of FILL."""

    def __init__(self, nbytes):
        self.n = nbytes
        self.all = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=G.dev())
        self.body = self.all[GUARD:GUARD + nbytes]

    def ptr(self, off=0):
        return ctypes.c_void_p(self.body.data_ptr() + off)

    def intact(self):
        return bool((self.all[:GUARD] == FILL).all()) and bool((self.all[GUARD + self.n:] == FILL).all())


@pytest.mark.parametrize("mode", list(MODES))
def test_pack_fnet_inference_writes_every_derived_region_from_its_source_and_nothing_else(mode):
    """The full-size audio network.  Which bytes derive from which parameters is found from the outside: every source tensor in turn
    is multiplied by -1.5 and packed again; what changes outside all parameters' own regions, grouped by the set of sources that
    change it (wiring_ref.regions), are the derived regions.  Their set, sizes and contents must be what csrc/plan.cpp says."""
    t0 = time.time()
    cfg, m = _model("audio", mode)
    lib = m._ensure_handle()
    h = m._handle
    bf_conv, bf_fnet = MODES[mode][0] == BF16T, (MODES[mode][0] == BF16T and MODES[mode][1] is None)
    names = list(m._inventory)
    idx = {n: i for i, n in enumerate(names)}
    tensors = [t.detach() for t in m._state_tensors()]
    n = len(tensors)
    info = [_param_pack(lib, h, i) for i in range(n)]
    total = int(lib.ddimx_packed_bytes(h))
    assert total % 256 == 0
    nblk = total // 256
    pk = _Guarded(total)
    body = pk.body
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    kw = cfg.model.transformers.kwargs
    hid, inter, layers = kw.hidden_size, kw.intermediate_size, kw.num_hidden_layers
    width = cfg.model.ch[-1] * (cfg.model.f_size >> (len(cfg.model.ch) - 1))

    def pack(derived=True):
        _lib.check(lib.ddimx_pack_weights(h, arr, n, pk.ptr(), _lib.stream()))
        if derived:
            _lib.check(lib.ddimx_pack_fnet_inference(h, pk.ptr(), _lib.stream()))
        torch.cuda.synchronize()

    def blocks(mask):
        return mask.view(nblk, 256).any(dim=1)

    try:
        pack()
        base = body.clone()
        main_blk = torch.zeros(nblk, dtype=torch.bool, device=G.dev())
        own = torch.full((nblk,), -1, dtype=torch.int64, device=G.dev())  # block -> the parameter whose own region it lies in
        known = torch.zeros(total, dtype=torch.bool, device=G.dev())
        for i, (_, off, nb, _) in enumerate(info):
            assert off % 256 == 0
            main_blk[off // 256:_al256(off + nb) // 256] = True
            own[off // 256:_al256(off + nb) // 256] = i
            known[off:off + nb] = True

        # ---- the sources
        lyr = lambda i, leaf: f"transformer.encoder.layer.{i}.{leaf}"  # noqa: E731
        FN = dict(w1="intermediate.dense.weight", b1="intermediate.dense.bias", w2="output.dense.weight",
                  ln1_w="fourier.output.LayerNorm.weight", ln1_b="fourier.output.LayerNorm.bias", ln2_w="output.LayerNorm.weight",
                  ln2_b="output.LayerNorm.bias")
        PROJ, COUT_W, COUT_B = "transformer.embedding.projection.weight", "transformer.compute_out.weight", "transformer.compute_out.bias"
        conv3 = [k for k in names if k.endswith(("conv.0.weight", "conv.1.weight"))]
        downup = [k for k in names if k.endswith(".conv.weight")]
        fnet_src = [lyr(i, v) for i in range(layers) for v in FN.values()] + [PROJ, COUT_W, COUT_B]
        assert len(conv3) == 64 and len(downup) == 10 and len(fnet_src) == 7 * layers + 3
        sources = conv3 + downup + fnet_src

        # ---- differentially: what each source changes
        changed = {}
        for s in sources:
            t = tensors[idx[s]]
            keep = t.clone()
            t.mul_(-1.5)
            pack()
            cb = blocks(body != base)
            in_main = cb & main_blk
            assert bool(in_main.any()) and bool((own[in_main] == idx[s]).all()), f"{s}: changes another parameter's own region, or not its own"
            changed[s] = (cb & ~main_blk).nonzero().reshape(-1).cpu().numpy()
            t.copy_(keep)
        pack()
        assert torch.equal(body, base), "with every source restored the buffer must be the baseline again"
        found = W.regions(changed, total)  # raises if the regions of two sets of sources overlap

        # ---- which sources have derived regions, and of what size
        wes = 2 if bf_fnet else 4
        want = {}  # frozenset of sources -> bytes
        if bf_conv:
            for k in conv3:
                C = tensors[idx[k]].shape[0]
                want[frozenset([k])] = 9 * C * C * 2
            for k in downup:  # every Downsample / Upsample width pair of this network has a register-streamed kernel
                want[frozenset([k])] = tensors[idx[k]].numel() * 2 if k.startswith("down") else 2 * 6 * 2 * tensors[idx[k]].shape[1] * tensors[idx[k]].shape[0] * 2
        for i in range(layers):
            want[frozenset([lyr(i, FN["w1"]), lyr(i, FN["ln1_w"])])] = inter * hid * wes                       # w1f
            want[frozenset([lyr(i, FN["w1"]), lyr(i, FN["ln1_b"]), lyr(i, FN["b1"])])] = inter * 4           # b1f
            want[frozenset([lyr(i, FN["w2"])])] = hid * inter * wes                                             # w2c
            if i > 0:
                want[frozenset([lyr(i - 1, FN["ln2_w"])])] = 2 * hid * hid * 4                                  # tab of layer i
                want[frozenset([lyr(i - 1, FN["ln2_b"])])] = hid * 4                                            # bc of layer i
        last = layers - 1
        want[frozenset([PROJ])] = hid * width * wes
        want[frozenset([COUT_W, lyr(last, FN["ln2_w"])])] = width * hid * wes                                   # coutf
        want[frozenset([COUT_W, lyr(last, FN["ln2_b"]), COUT_B])] = width * 4                                   # coutb
        assert set(found) == set(want), (sorted(map(sorted, set(found) - set(want))), sorted(map(sorted, set(want) - set(found))))
        for k, (lo, hi) in found.items():
            assert hi - lo == _al256(want[k]), (sorted(k), lo, hi, want[k])
            assert not bool(main_blk[lo // 256:hi // 256].any()), f"the region of {sorted(k)} overlaps a parameter's own region"
        spans = sorted(found.values())
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "two derived regions overlap"

        # ---- content: the composition of the C calls, on the same sources
        def main_ptr(name):
            return None if name is None else pk.ptr(info[idx[name]][1])

        def same(k, got, what):
            lo = found[frozenset(k)][0]
            assert got.intact(), what
            assert torch.equal(body[lo:lo + got.n], got.body), f"{what}: the derived region differs from the C call on its sources"

        for k in conv3 + downup if bf_conv else []:
            kind, off, nb, (d0, d1, d2, d3) = info[idx[k]]
            out = _Guarded(want[frozenset([k])])
            if kind == _lib.DDIMX_PACK_CONV:
                _lib.check(lib.ddimx_pack_frag_from_taps(pk.ptr(off), out.ptr(), d2 * d3, d0, d1, _lib.stream()))
            else:  # Upsample: both row-parity classes of the sub-pixel form
                assert kind == _lib.DDIMX_PACK_CONVT
                cls = 6 * 2 * d1 * d0 * 2
                for a in range(2):
                    _lib.check(lib.ddimx_pack_frag_from_taps(pk.ptr(off + a * cls), out.ptr(a * cls), 6, 2 * d1, d0, _lib.stream()))
            torch.cuda.synchronize()
            same([k], out, k)

        def fold(W_, gamma, beta, bias, N, K, kw_, kb_):
            wf, bfo = _Guarded(N * K * wes), (_Guarded(N * 4) if kb_ else None)
            _lib.check(lib.ddimx_fnet_fold(main_ptr(W_), main_ptr(gamma), main_ptr(beta), main_ptr(bias), wf.ptr(), int(bf_fnet),
                                           bfo.ptr() if bfo else None, N, K, _lib.stream()))
            torch.cuda.synchronize()
            same(kw_, wf, f"fold {W_}")
            if bfo:
                same(kb_, bfo, f"fold {W_} bias")

        def table(gamma, beta, ktab, kbc, lo=None):
            tab, bc = _Guarded(2 * hid * hid * 4), (_Guarded(hid * 4) if beta else None)
            _lib.check(lib.ddimx_fnet_table(main_ptr(gamma), main_ptr(beta), tab.ptr(), bc.ptr() if bc else None, hid, _lib.stream()))
            torch.cuda.synchronize()
            if ktab is None:
                assert tab.intact() and torch.equal(body[lo:lo + tab.n], tab.body), "layer 0's table differs from ddimx_fnet_table(null, null)"
            else:
                same(ktab, tab, f"table {gamma}")
                same(kbc, bc, f"table {beta}")

        for i in range(layers):
            fold(lyr(i, FN["w1"]), lyr(i, FN["ln1_w"]), lyr(i, FN["ln1_b"]), lyr(i, FN["b1"]), inter, hid,
                 [lyr(i, FN["w1"]), lyr(i, FN["ln1_w"])], [lyr(i, FN["w1"]), lyr(i, FN["ln1_b"]), lyr(i, FN["b1"])])
            fold(lyr(i, FN["w2"]), None, None, None, hid, inter, [lyr(i, FN["w2"])], None)
            if i > 0:
                table(lyr(i - 1, FN["ln2_w"]), lyr(i - 1, FN["ln2_b"]), [lyr(i - 1, FN["ln2_w"])], [lyr(i - 1, FN["ln2_b"])])
        fold(PROJ, None, None, None, hid, width, [PROJ], None)
        fold(COUT_W, lyr(last, FN["ln2_w"]), lyr(last, FN["ln2_b"]), COUT_B, width, hid, [COUT_W, lyr(last, FN["ln2_w"])],
             [COUT_W, lyr(last, FN["ln2_b"]), COUT_B])

        # ---- nothing else written: layer 0's table depends on no parameter, so no diff finds it; it is whatever else was written
        for k, (lo, hi) in found.items():
            known[lo:lo + want[k]] = True
        rest = blocks((body != FILL) & ~known).nonzero().reshape(-1)
        assert rest.numel() > 0, "layer 0's hidden-DFT table was not written"
        lo0, hi0 = int(rest.min()) * 256, (int(rest.max()) + 1) * 256
        assert hi0 - lo0 == 2 * hid * hid * 4, f"written outside every known region: blocks {lo0 // 256}..{hi0 // 256}"
        assert not bool(known[lo0:hi0].any())
        table(None, None, None, None, lo=lo0)
        known[lo0:hi0] = True
        assert bool((body[~known] == FILL).all()), "a byte outside every parameter's region and every derived region was written"
        assert pk.intact(), "written outside the buffer"

        # ---- a second ddimx_pack_fnet_inference rewrites the same bytes
        derived = known.clone()
        for _, off, nb, _ in info:
            derived[off:off + nb] = False
        body[derived] = 0x5A
        _lib.check(lib.ddimx_pack_fnet_inference(h, pk.ptr(), _lib.stream()))
        torch.cuda.synchronize()
        assert torch.equal(body, base) and pk.intact(), "ddimx_pack_fnet_inference alone must rewrite every derived region, the same"

        # ---- negative control: ddimx_pack_weights alone leaves the derived copies as they were, and the diff sees that
        stale = ([conv3[5]] if bf_conv else []) + [lyr(0, FN["w2"])]
        for s in stale:
            t = tensors[idx[s]]
            keep = t.clone()
            t.mul_(-1.5)
            pack(derived=False)
            lo, hi = found[frozenset([s])]
            _, off, nb, _ = info[idx[s]]
            assert not torch.equal(body[off:off + nb], base[off:off + nb]), f"{s}: its own region must follow"
            assert torch.equal(body[lo:hi], base[lo:hi]), f"{s}: ddimx_pack_weights alone rewrote the derived copy"
            t.copy_(keep)
        pack()
        assert torch.equal(body, base)
        print(f"[wiring pack {mode}] {total} bytes, {len(sources)} sources, {len(found) + 1} derived regions of "
              f"{int(derived.sum())} bytes, {int((~known).sum())} bytes of padding untouched; {time.time() - t0:.1f} s")
    finally:
        m.invalidate()  # the handle's notion of which buffer holds fresh derived copies now names this test's buffer


# =========================================================================================================================================
# 2. every parameter, through the walk, against the oracle
# =========================================================================================================================================
def _respond(case, mode, m, names, run, g, gate):
    """The procedure of one case: ``run()`` -> the walk's output on the CPU with the model's current parameters (the model repacks
    itself when one has changed); ``gate(got, ref, what)`` the existing gate of that output; ``g`` its bound, for the input condition."""
    t0 = time.time()
    net = W.CASES[case]["net"]
    cache = _refs(case, m, names)
    base = cache["base"]
    params = dict(m.named_parameters())
    # the input condition, from the oracle's numbers alone
    judged = W.judge_inputs(cache, names, g)
    loud = max(names, key=lambda k: judged[k][1])
    assert judged[loud][1] <= W.N_MAX, f"{loud}: m {judged[loud][0]:.3e}, n {judged[loud][1]:.3e} misses the input condition"
    pairs = W.control_pairs(names, net)
    for i, j in pairs:
        c = W.projection(cache[j][1] - base, cache[i][1] - base)
        assert abs(c) < W.CONTROL_MAX, f"control pair {i} / {j}: the oracle alone gives {c:.3f}"

    with torch.no_grad():
        y0 = run()
        gate(y0, base, f"{case} {mode} baseline")
        d_got, failures, worst_c, worst_gate, done = {}, [], (0.0, None), (0.0, None), 0
        for k in names:
            p = params[k]
            keep = p.detach().clone()
            p.copy_(cache[k][0].to(p.device))
            try:
                y = run()
            finally:
                p.copy_(keep)
            d_got[k] = y - y0
            if torch.equal(H.bits(y), H.bits(y0)):
                failures.append(f"{k}: (a) the output's bits did not change")
            c = W.projection(d_got[k], cache[k][1] - base)
            worst_c = max(worst_c, (abs(c - 1.0), k))
            if not W.C_LO <= c <= W.C_HI:
                failures.append(f"{k}: (b) c = {c:.4f}")
            try:
                worst_gate = max(worst_gate, (gate(y, cache[k][1], f"{k} replaced")[1], k))
            except AssertionError as e:
                failures.append(f"{k}: (c) {e}")
            done += 1
        again = run()
    worst_ij = (0.0, None)
    for i, j in pairs:
        c = W.projection(d_got[j], cache[i][1] - base)
        worst_ij = max(worst_ij, (abs(c), (i, j)))
        if not abs(c) < W.C_LO:
            failures.append(f"control {i} / {j}: c_ij = {c:.4f}")
    print(f"[wiring {case} {mode}] {done} parameters: worst |c - 1| {worst_c[0]:.4f} ({worst_c[1]}), largest n {judged[loud][1]:.4f} "
          f"({loud}), worst rms error at a replaced point {worst_gate[0]:.3e} ({worst_gate[1]}); {len(pairs)} control pairs, worst "
          f"|c_ij| {worst_ij[0]:.3f} {worst_ij[1]}; {time.time() - t0:.1f} s")
    assert done == len(names)
    assert not failures, "\n".join(failures)
    assert torch.equal(H.bits(again), H.bits(y0)), "with every parameter put back the output must have the baseline's bits"


def _network_run(case, m):
    c = W.CASES[case]
    x = synth.gaussian(f"wiring.{case}.x", c["shape"]).to(G.dev())
    t = torch.tensor(c["steps"], device=G.dev())
    return lambda: m(x, t).cpu()


_AUDIO_GROUPS = ["temb", "edge"] + [f"down{l}" for l in range(6)] + [f"up{l}" for l in range(6)] + ["transformer_a", "transformer_b"]
_AUDIO_COUNTS = dict(temb=6, edge=4, down0=16, down1=18, down2=26, down3=26, down4=26, down5=26, up0=16, up1=18, up2=26, up3=26,
                     up4=26, up5=26, transformer_a=51, transformer_b=51)


@pytest.mark.parametrize("group", _AUDIO_GROUPS)
@pytest.mark.parametrize("mode", list(MODES))
def test_every_audio_parameter_reaches_the_output_as_in_the_oracle(mode, group):
    """The full-size network at B = 1, T = 32 (S = 1: the FNet takes the GEMM path), all 388 parameters over the 16 groups."""
    cfg, m = _model("audio", mode)
    names = W.groups(list(m._inventory), len(cfg.model.ch))[group]
    assert len(names) == _AUDIO_COUNTS[group] and sum(_AUDIO_COUNTS.values()) == 388
    dt = MODES[mode][2]
    _respond("audio", f"{mode} {group}", m, names, _network_run("audio", m), W.G_BOUND[mode], lambda got, ref, what: H.gate(got, ref, dt, what))


FNET_GATES = {"f32": (1e-4, 2e-5), "mixed": (2e-2, 4e-3), "bf16": (6e-2, 1.2e-2)}  # test_fnet_dense_path_vs_oracle_and_batch_independence


@pytest.mark.parametrize("mode", list(MODES))
def test_every_transformer_parameter_reaches_the_dense_path_output(mode):
    """transformer.* again through ddimx_fnet_fwd at S = 8, B = 2: the dense path with the LayerNorm-folded copies, which only the
    full-size widths reach, against ref_cpu.transformer_module."""
    cfg, m = _model("audio", mode)
    lib = _lib.load()
    dev = G.dev()
    b, s, width = W.CASES["fnet"]["shape"]
    t_len = s << (len(cfg.model.ch) - 1)
    c_last, fr = cfg.model.ch[-1], width // cfg.model.ch[-1]
    tok = synth.gaussian("wiring.fnet.x", (b, s, width))
    x = tok.view(b, s, c_last, fr).permute(0, 1, 3, 2).contiguous().to(dev, m._act_dtype)  # reference token order c*Fr + f -> NHWC rows
    lib2 = m._ensure_handle()
    ws = torch.empty(int(lib.ddimx_workspace_bytes(m._handle, b, t_len)), dtype=torch.uint8, device=dev)

    def run():
        with torch.cuda.device(dev):
            m._ensure_packed(lib2, dev)
            pe, dh, ds = m._ensure_tables(t_len, dev)
        tb = _lib.DdimxTables(pe.data_ptr(), dh.data_ptr(), ds.data_ptr())
        out = torch.full((b * s, width), float("nan"), device=dev)
        _lib.check(lib.ddimx_fnet_fwd(m._handle, _lib.ptr(m._packed), ctypes.byref(tb), _lib.ptr(ws), ws.numel(), _lib.ptr(x), _lib.ptr(out),
                                      b, t_len, _lib.stream()))
        return out.cpu().view(b, s, fr, c_last).permute(0, 1, 3, 2).reshape(b, s, width)

    mx, rms = FNET_GATES[mode]

    def gate(got, ref, what):
        got, ref = got.double().reshape(-1), ref.double().reshape(-1)
        assert torch.isfinite(got).all(), what
        sd = float(ref.std())
        e_mx, e_rms = float((got - ref).abs().max()) / sd, float((got - ref).square().mean().sqrt()) / sd
        assert e_mx <= mx and e_rms <= rms, f"{what}: max {e_mx:.3e}, rms {e_rms:.3e} of std"
        return e_mx, e_rms

    names = W.case_names("fnet", list(m._inventory))
    assert len(names) == 102
    _respond("fnet", mode, m, names, run, rms, gate)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_level0_parameters_reach_the_output_on_the_gn_finalize_path(mode):
    """The tiny network at the shortest clip for which the input conv hands level 0 more statistics partials per sample than a conv
    finishes in-kernel (kGnFuseMaxParts = 256): the first block's first GroupNorm is then finished by a gn_finalize_groups launch.
    The level-0 blocks' norm.* and conv parameters."""
    cfg, m = _model("tiny", mode)
    lib = _lib.load()
    b, _, T, F = W.CASES["long"]["shape"]
    dt, C0 = MODES[mode][2], cfg.model.ch[0]

    def plan(t_len):
        xn = int(lib.ddimx_conv_in_stats_floats(b, C0, t_len, F)) // (b * C0 * 2)
        return xn, X.gn_plan(dt, C0, b, t_len, F, xn)

    xn, p = plan(T)
    assert xn > 256 and p["conv0_np"] == xn and not p["conv0"], (xn, p)
    step = 1 << (len(cfg.model.ch) - 1)
    xs, ps = plan(T - step)
    assert max(xs, ps["conv1_np"], ps["resid_np"]) <= 256 and ps["conv0"], f"T = {T} is not the shortest such clip: {xs}, {ps}"
    names = W.case_names("long", list(m._inventory))
    assert len(names) == 16
    _respond("long", mode, m, names, _network_run("long", m), W.G_BOUND[mode], lambda got, ref, what: H.gate(got, ref, dt, what))


# =========================================================================================================================================
# 3. stale derived copies are not read
# =========================================================================================================================================
@pytest.mark.parametrize("mode", ["bf16", "mixed"])
@pytest.mark.parametrize("net", ["tiny", "audio"])
def test_stale_derived_copies_are_not_read(net, mode):
    """The C ABI on a buffer of the test's own: after ddimx_pack_weights alone the fragment-order conv copies (and the folded FNet
    copies) hold the previous weights, and ddimx_unet_fwd must compute with the new ones -- through the tap-layout copies -- as it
    does after ddimx_pack_fnet_inference through the fresh derived ones."""
    cfg, m = _model(net, mode)
    lib = m._ensure_handle()
    h, dev, dt = m._handle, G.dev(), MODES[mode][2]
    case = net
    L = len(cfg.model.ch)
    pair = ["down_modules.1.0.conv.1.weight", f"down_modules.{L}.1.conv.1.weight"]
    cache = _refs(case, m, pair)
    sd, fwd, _ = _REFS[case]
    both = dict(sd)
    for k in pair:
        both[k] = cache[k][0]
    with torch.no_grad():
        y_ref = fwd(both)
    base = cache["base"]
    c_ref = [W.projection(y_ref - base, cache[k][1] - base) for k in pair]
    assert all(0.75 <= c <= 1.25 for c in c_ref), f"the oracle's joint response must project onto each single one: {c_ref}"
    g = W.G_BOUND[mode]
    assert all(W.noise(g, W.strength(cache[k][1] - base, cache[k][1]), base.numel()) <= W.N_MAX for k in pair)

    shape = W.CASES[case]["shape"]
    b, t_len = shape[0], shape[2]
    x = synth.gaussian(f"wiring.{case}.x", shape).to(dev)
    t = torch.tensor(W.CASES[case]["steps"], device=dev)
    tensors = [v.detach() for v in m._state_tensors()]
    params = dict(zip(m._inventory, tensors))
    arr = (ctypes.c_void_p * len(tensors))(*[v.data_ptr() for v in tensors])
    pk = _Guarded(int(lib.ddimx_packed_bytes(h)))
    ws = torch.empty(int(lib.ddimx_workspace_bytes(h, b, t_len)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        pe, dh, ds = m._ensure_tables(t_len, dev)
    tb = _lib.DdimxTables(pe.data_ptr(), dh.data_ptr(), ds.data_ptr())

    def pack(derived):
        _lib.check(lib.ddimx_pack_weights(h, arr, len(tensors), pk.ptr(), _lib.stream()))
        if derived:
            _lib.check(lib.ddimx_pack_fnet_inference(h, pk.ptr(), _lib.stream()))

    def forward():
        out = torch.full(shape, float("nan"), device=dev)
        _lib.check(lib.ddimx_unet_fwd(h, pk.ptr(), ctypes.byref(tb), _lib.ptr(ws), ws.numel(), _lib.ptr(x), _lib.ptr(t), _lib.ptr(out), b,
                                      t_len, _lib.stream()))
        return out.cpu()

    def judge(y, what):
        _, er = H.gate(y, y_ref, dt, f"{net} {mode} {what}")
        cs = [W.projection(y - y_a, cache[k][1] - base) for k in pair]
        assert all(W.C_LO <= c <= W.C_HI for c in cs), f"{what}: c = {cs}"
        return er, cs

    keep = {k: params[k].clone() for k in pair}
    try:
        pack(True)
        y_a = forward()
        H.gate(y_a, base, dt, f"{net} {mode} baseline")
        for k in pair:
            params[k].copy_(cache[k][0].to(dev))
        pack(False)
        y_b = forward()
        er_b, c_b = judge(y_b, "stale derived copies")
        pack(True)
        y_c = forward()
        er_c, c_c = judge(y_c, "fresh derived copies")
        assert not torch.equal(H.bits(y_c), H.bits(y_a))
        for k in pair:
            params[k].copy_(keep[k])
        pack(True)
        assert torch.equal(H.bits(forward()), H.bits(y_a)), "the weights put back and packed again must give the first output's bits"
        assert pk.intact()
        print(f"[wiring stale {net} {mode}] oracle-alone c {c_ref[0]:.3f} {c_ref[1]:.3f}; pack_weights alone: rms error {er_b:.3e}, c "
              f"{c_b[0]:.3f} {c_b[1]:.3f}; with the derived copies: rms error {er_c:.3e}, c {c_c[0]:.3f} {c_c[1]:.3f}; "
              f"same bits both ways: {torch.equal(H.bits(y_b), H.bits(y_c))}")
    finally:
        for k in pair:
            params[k].copy_(keep[k])
        m.invalidate()  # the handle's notion of which buffer holds fresh derived copies now names this test's buffer
