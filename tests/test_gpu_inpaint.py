"""Masked DDIM inpainting with reconstruction guidance (ddim_audio_amd.inpaint_steps, ddimx_inpaint_residual / _update).

Against generalized_steps bit for bit where the definition reduces to it, against the CPU restatement (tests/inpaint_ref.py,
autograd through the oracle) within model_harness's gates, against the autograd recipe of INTEGRATION.md section E on the
same GPU model, replayed against eager steps, per-sample independence, no side effects, and the kernels on exact operands."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, synth
from ddim_audio_amd.schedule import inpaint_coefficients
import gpu_util as G
import inpaint_ref
import model_harness as MH
from model_harness import MODES, MODE_IDS

pytestmark = pytest.mark.gpu
DROPOUT = 0.1  # every model here is built with it, in eval mode: must never be applied
SHAPES = {"tiny": ("tiny", (2, 2, 16, 32)), "audio": ("audio", (2, 2, 32, 256)), "ragged": ("tiny", (3, 2, 24, 32))}


def _mask(kind, shape):
    b, c, t, f = shape
    if kind == "gap":    # a time gap (packet loss): [B, 1, T, 1]
        m = torch.ones(b, 1, t, 1)
        m[:, :, t // 4: t // 2] = 0
    elif kind == "band":  # missing high bands (bandwidth extension): [1, 1, 1, F]
        m = torch.ones(1, 1, 1, f)
        m[..., f // 2:] = 0
    else:                 # a time gap with a soft (0.5) edge band, per sample
        m = torch.ones(b, 1, t, f)
        m[:, :, t // 4: t // 2] = 0
        m[:, :, :, -f // 4:] *= 0.5
        m[-1, :, : t // 8] = 0
    return m


# ---- 1. empty mask, no guidance: generalized_steps bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("replace", [True, False], ids=["replace", "plain"])
@pytest.mark.parametrize("n", [3, 10], ids=["eager", "replayed"])
@pytest.mark.parametrize("name", ["tiny", "audio"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_empty_mask_equals_generalized_steps(mode, name, n, replace):
    cfg, m = MH.build(name, mode[0], 5, mode="eval", dropout=DROPOUT)
    shape = (4, 2, 32, cfg.model.f_size)  # B = 4: the replacement-only graph forks into two shards like DDIMStepper's
    x, y = MH.pair_data("inp.empty", shape)
    seq = list(range(0, 1000, 1000 // n))[:n]
    a = MH.alphas(cfg)
    want_xs, want_x0 = D.generalized_steps(x.cuda(), seq, m, a, None)
    xs, x0 = D.inpaint_steps(x.cuda(), seq, m, a, None, y=y, mask=torch.zeros(1, 1, 1, 1), guidance=0.0, replace=replace)
    assert len(xs) == len(want_xs) == n + 1 and len(x0) == n
    for i in range(1, n + 1):
        assert torch.equal(xs[i], want_xs[i]), f"xs[{i}]"
        assert torch.equal(x0[i - 1], want_x0[i - 1]), f"x0_preds[{i - 1}]"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_empty_mask_with_eta_equals_generalized_steps(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval", dropout=DROPOUT)
    shape = (2, 2, 16, 32)
    x, y = MH.pair_data("inp.eta", shape)
    seq, a = [0, 250, 500, 750, 900], MH.alphas(cfg)
    torch.manual_seed(11)
    want_xs, want_x0 = D.generalized_steps(x.cuda(), seq, m, a, None, eta=0.5)
    torch.manual_seed(11)
    xs, x0 = D.inpaint_steps(x.cuda(), seq, m, a, None, y=y, mask=torch.zeros(shape, dtype=torch.bool), eta=0.5)
    for i in range(1, len(seq) + 1):
        assert torch.equal(xs[i], want_xs[i]) and torch.equal(x0[i - 1], want_x0[i - 1]), i


# ---- 2. replacement only -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gap", "band"])
@pytest.mark.parametrize("name", ["tiny", "audio"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_replacement_only_vs_reference(mode, name, kind):
    dtype_str, dt = mode
    cfg, m = MH.build(name, dtype_str, 5, mode="eval", dropout=DROPOUT)
    shape = SHAPES[name][1]
    x, y = MH.pair_data("inp.repl", shape)
    mask = _mask(kind, shape)
    seq, a = [0, 250, 500, 750], MH.alphas(cfg)  # 4 steps: the replayed path
    xs, x0 = D.inpaint_steps(x.cuda(), seq, m, a, None, y=y.cuda(), mask=mask.bool(), replace=True)
    MH.known_exact(xs[-1], y, mask)
    rxs, rx0 = inpaint_ref.inpaint_steps(x, seq, MH.oracle_eps(m, name), a, y, mask, 0.0, True)
    for i in range(len(seq)):
        MH.gate(xs[i + 1], rxs[i + 1], dt, f"xs[{i + 1}] {kind}")
        MH.gate(x0[i], rx0[i], dt, f"x0[{i}] {kind}")


# ---- 3. guided ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 4])
@pytest.mark.parametrize("case", ["tiny", "audio", "ragged"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_guided_vs_reference(mode, case, steps):
    dtype_str, dt = mode
    name, shape = SHAPES[case]
    cfg, m = MH.build(name, dtype_str, 5, mode="eval", dropout=DROPOUT)
    x, y = MH.pair_data("inp.guid." + case, shape)
    mask = _mask("soft", shape)
    seq = [400] if steps == 1 else [0, 250, 500, 750]
    zeta = 0.3 if steps == 1 else [0.2, 0.3, 0.0, 0.25]
    a = MH.alphas(cfg)
    xs, x0 = D.inpaint_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=zeta, replace=True)
    rxs, rx0 = inpaint_ref.inpaint_steps(x, seq, MH.oracle_eps(m, name), a, y, mask, zeta, True)
    for i in range(len(seq)):
        mx, er = MH.gate(xs[i + 1], rxs[i + 1], dt, f"xs[{i + 1}] {case}")
        MH.gate(x0[i], rx0[i], dt, f"x0[{i}] {case}")
    print(f"[inpaint guided {case} {steps} {MODE_IDS[dt]}] final max {mx:.3e} rms err {er:.3e} x rms")
    if seq[0] == 0:
        MH.known_exact(xs[-1], y, mask)


# ---- 4. one guided step against the section-E autograd recipe on the same GPU model --------------------------------------------
def _residual(xt, eps, y, mask, coef):
    lib = _lib.load()
    b, per = xt.size(0), xt[0].numel()
    x0, seed = torch.empty_like(xt), torch.empty_like(xt)
    part = torch.empty(int(lib.ddimx_inpaint_partials_floats(b, per)), device=xt.device)
    ctr = torch.zeros(1, dtype=torch.int32, device=xt.device)
    _lib.check(lib.ddimx_inpaint_residual(_lib.ptr(xt), _lib.ptr(eps), _lib.ptr(y), _lib.ptr(mask), _lib.ptr(x0), _lib.ptr(seed),
                                          _lib.ptr(part), _lib.ptr(coef), _lib.ptr(ctr), b, per, _lib.stream()))
    return x0, seed, part


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_guided_step_vs_autograd_recipe(mode):
    cfg, m = MH.build("audio", mode[0], 5, mode="eval", dropout=DROPOUT)
    shape = (3, 2, 32, 256)
    x, y = MH.pair_data("inp.recipe", shape)
    mask = _mask("soft", shape)
    seq, zeta, a = [300], 0.4, MH.alphas(cfg)
    coef64 = inpaint_coefficients(seq, a, 0.0, zeta)
    xs, x0s = D.inpaint_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=zeta, replace=True)
    # section E: autograd through the eval-mode model; x0 and the seed from the residual kernel (a torch-formed seed can flip a
    # bf16 rounding inside the backward), the rest in torch ops
    ti, s1, s2, s3, c2, c1, k1, k2, _ = [float(v) for v in coef64[0]]
    coef = torch.from_numpy(coef64.astype(np.float32)).cuda()
    mk = torch.broadcast_to(mask, shape).contiguous().cuda()
    yk = torch.where(mk == 0, torch.zeros((), device="cuda"), y.cuda()).contiguous()
    xg = x.cuda().requires_grad_(True)
    eps = m(xg, torch.full((3,), int(ti), device="cuda"))
    x0, seed, _ = _residual(xg.detach(), eps.detach().contiguous(), yk, mk, coef)
    (d_x,) = torch.autograd.grad(eps, xg, seed)
    eps = eps.detach()
    r = mk * (x0 - yk)
    L = r.double().square().flatten(1).sum(1).float()
    g = np.float32(k2) * (mk * r) + d_x
    u = s3 * x0 + c2 * eps - (zeta / L.sqrt()).view(-1, 1, 1, 1) * g
    want = mk * (s3 * yk + c2 * eps) + (1 - mk) * u
    assert torch.equal(x0s[0], x0.cpu())
    rms = float(want.double().square().mean().sqrt())
    err = float((xs[1].double() - want.cpu().double()).abs().max())
    assert err <= 1e-5 * rms, f"max {err / rms:.3e} x rms"


# ---- 5. replayed steps = eager steps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "replace_only"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_replayed_equals_eager(mode, guided):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval", dropout=DROPOUT)
    shape = (4, 2, 32, 32)
    x, y = MH.pair_data("inp.replay", shape)
    mask = _mask("soft", shape)
    seq, a = [0, 200, 400, 600, 800], MH.alphas(cfg)
    kw = dict(y=y, mask=mask, guidance=0.3 if guided else 0.0, replace=True)
    g_xs, g_x0 = D.inpaint_steps(x.cuda(), seq, m, a, None, **kw)
    with MH.eager_steps():
        e_xs, e_x0 = D.inpaint_steps(x.cuda(), seq, m, a, None, **kw)
        for i in range(len(seq)):
            assert torch.equal(g_xs[i + 1], e_xs[i + 1]) and torch.equal(g_x0[i], e_x0[i]), i


def test_stepper_replays_one_graph():
    cfg, m = MH.build("tiny", "torch.cuda.FloatTensor", 5, mode="eval", dropout=DROPOUT)
    from ddim_audio_amd.inpaint import InpaintStepper
    shape = (2, 2, 16, 32)
    x = synth.gaussian("inp.one", shape).cuda()
    mk = torch.ones(shape, device="cuda")
    coef = inpaint_coefficients([0, 200, 400, 600, 800], MH.alphas(cfg), 0.0, 0.3)
    with torch.no_grad():
        st = InpaintStepper(m, x, torch.zeros_like(x), mk, coef, True, True)
        try:
            for _ in range(5):
                st.step()
            assert st.captures == 1 and st.graph is not None
            st.rewind()
            m.invalidate()  # new packed values in place: the graph stays
            st.step()
            assert st.captures == 1
            m._packed_bwd = None  # a re-allocated backward packing does not bump Model._gen: still stale
            st.step()
            assert st.captures == 2
        finally:
            st.close()


# ---- 6. per-sample independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_samples_are_independent(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval", dropout=DROPOUT)
    shape = (2, 2, 16, 32)
    x, y = MH.pair_data("inp.indep", shape)
    mask = _mask("soft", shape)
    seq, a = [0, 300, 600, 900], MH.alphas(cfg)
    xs_a, x0_a = D.inpaint_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=0.3)
    y2, mask2 = y.clone(), mask.clone()
    y2[0] *= 3.0
    mask2[0] = 1.0
    xs_b, x0_b = D.inpaint_steps(x.cuda(), seq, m, a, None, y=y2, mask=mask2, guidance=0.3)
    assert not torch.equal(xs_a[-1][0], xs_b[-1][0])
    for i in range(len(seq)):
        assert torch.equal(xs_a[i + 1][1], xs_b[i + 1][1]) and torch.equal(x0_a[i][1], x0_b[i][1]), i


# ---- 7. no side effects --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_no_side_effects(mode, train):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval", dropout=DROPOUT)
    assert all(p.requires_grad for p in m.parameters())
    shape = (2, 2, 16, 32)
    x, y = MH.pair_data("inp.side", shape)
    mask = _mask("gap", shape)
    seq, a = [0, 300, 600, 900], MH.alphas(cfg)
    before = D.generalized_steps(x.cuda(), seq, m, a, None)
    ref_xs, _ = D.inpaint_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=0.3)
    m._dropout_calls = 17
    m.train(train)
    xs, _ = D.inpaint_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=0.3)
    assert m._dropout_calls == 17
    assert all(p.grad is None for p in m.parameters())
    assert getattr(m, "_flat_grad", None) is None
    for i in range(1, len(seq) + 1):
        assert torch.equal(xs[i], ref_xs[i]), f"train={train}: xs[{i}] differs from the eval-mode run"
    m.eval()
    after = D.generalized_steps(x.cuda(), seq, m, a, None)
    for u, v in zip(before[0][1:] + before[1], after[0][1:] + after[1]):
        assert torch.equal(u, v)


# ---- 8. the kernels on exact operands ----------------------------------------------------------------------------------------------
def _ints(tag, shape, lim, scale):
    v = synth.uniform_pm1(tag, int(np.prod(shape)))
    return torch.from_numpy(np.rint(v * lim).astype(np.float64) * scale).reshape(shape)


@pytest.mark.parametrize("B,per", [(3, 5132), (2, 20), (2, 4 * 256 * 300)])
def test_kernels_exact(B, per):
    """Operands are small integers times powers of two and s1, s2 powers of two: x0, the seed, every partial sum and the update
    without guidance are exact in fp32 and must equal fp64; the guidance coefficient zeta / sqrt(L_b) and the few roundings after
    it (two fmas) are replayed on the host with the kernel's operation order.  The last sample's mask is empty: L_b = 0, no guidance term."""
    lib = _lib.load()
    dev = G.dev()
    tag = f"inp.exact.{B}.{per}"
    shape = (B, per)
    xt, eps, z = _ints(tag + ".x", shape, 3, 0.25), _ints(tag + ".e", shape, 3, 0.25), _ints(tag + ".z", shape, 3, 0.25)
    m = (_ints(tag + ".m", shape, 1, 1.0) + 1.0) * 0.5  # {0, 0.5, 1}
    if per > 65536:
        m[:, torch.arange(per) % 16 != 0] = 0.0  # keeps every partial and L_b below 2^24 units of r^2
    m[-1] = 0.0
    y = _ints(tag + ".y", shape, 1, 0.5) * (m != 0)
    dx = _ints(tag + ".dx", shape, 7, 0.125)
    s1, s2, s3, c2, c1, zeta = 0.5, 0.25, 0.5, 0.75, 0.25, 2.0
    k1, k2 = -2 * s1 / s2, 2 / s2
    coef = torch.tensor([[7.0, s1, s2, s3, c2, c1, k1, k2, zeta]], dtype=torch.float32, device=dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    g32 = lambda v: v.float().to(dev).contiguous()  # noqa: E731
    dxt, de, dz, dm, dy, ddx = g32(xt), g32(eps), g32(z), g32(m), g32(y), g32(dx)
    nparts = int(lib.ddimx_inpaint_partials_floats(B, per))
    assert nparts >= B and nparts % B == 0
    x0, seed = torch.full_like(dxt, float("nan")), torch.full_like(dxt, float("nan"))
    part = torch.full((nparts,), float("nan"), device=dev)
    s = _lib.stream()
    _lib.check(lib.ddimx_inpaint_residual(_lib.ptr(dxt), _lib.ptr(de), _lib.ptr(dy), _lib.ptr(dm), _lib.ptr(x0), _lib.ptr(seed),
                                          _lib.ptr(part), _lib.ptr(coef), _lib.ptr(ctr), B, per, s))
    x0_64 = (xt - s1 * eps) / s2
    r = m * (x0_64 - y)
    L = r.square().sum(1)
    torch.cuda.synchronize()
    assert torch.equal(x0.cpu().double(), x0_64)
    assert torch.equal(seed.cpu().double(), k1 * m * r)
    assert torch.equal(part.cpu().double().view(B, -1).sum(1), L) and float(L[-1]) == 0.0
    u64 = s3 * x0_64 + c2 * eps + c1 * z
    k64 = s3 * y + c2 * eps + c1 * z
    L32 = L.numpy().astype(np.float32)
    L64 = L32.astype(np.float64)
    w_rn = np.where(L64 > 0, zeta / np.sqrt(np.maximum(L64, 1e-300)), 0.0).astype(np.float32)  # in double, rounded once
    g = (k2 * m * r + dx).numpy().astype(np.float32)  # exact
    mm, kk = m.numpy().astype(np.float32), k64.numpy().astype(np.float32)

    def expect(flags, w):
        u = u64.numpy().astype(np.float32)
        if flags & 2:
            # fmaf(-w, g, u): the product and the sum are exact in fp64 for these operands, so one rounding to fp32 is the fma's
            upd = (u.astype(np.float64) - w.astype(np.float64)[:, None] * g.astype(np.float64)).astype(np.float32)
            u = np.where(w[:, None] != 0, upd, u)
        if flags & 1:
            blend = (mm.astype(np.float64) * kk + ((np.float32(1) - mm) * u).astype(np.float64)).astype(np.float32)  # fmaf
            u = np.where(mm == 1, kk, np.where(mm == 0, u, blend))
        return u.astype(np.float32).view(np.int32)

    for flags in (0, 1, 2, 3):
        out, x0b = dxt.clone(), (x0.clone() if flags & 2 else torch.full_like(dxt, float("nan")))
        _lib.check(lib.ddimx_inpaint_update(_lib.ptr(out), _lib.ptr(de), _lib.ptr(dz), _lib.ptr(x0b), _lib.ptr(dy), _lib.ptr(dm),
                                            _lib.ptr(ddx), _lib.ptr(part), _lib.ptr(coef), _lib.ptr(ctr), B, per, flags, s))
        torch.cuda.synchronize()
        assert torch.equal(x0b.cpu().double(), x0_64), flags
        got = out.cpu().numpy()
        assert np.isfinite(got).all(), flags
        got = got.view(np.int32)
        if not flags & 2:
            assert np.array_equal(got, expect(flags, w_rn)), f"flags {flags}"
            continue
        # the guidance coefficient zeta / sqrt(L_b) is formed in double and rounded once (one ulp of slack for the device's
        # double sqrt), the same for every element of a sample; everything after it is rounded as replayed here
        for b in range(B):
            cands = [np.nextafter(w_rn, np.float32(-np.inf)), w_rn, np.nextafter(w_rn, np.float32(np.inf))]
            ok = [np.array_equal(got[b], expect(flags, np.where(w_rn != 0, c, w_rn).astype(np.float32))[b]) for c in cands]
            bad = got[b] != expect(flags, w_rn)[b]
            assert any(ok), f"flags {flags} sample {b}: {int(bad.sum())} elements differ, e.g. {got[b][bad][:4]}"
        # the empty-mask sample: no guidance term at all
        assert np.array_equal(got[-1], expect(flags & 1, w_rn)[-1])
    # validation before the launch
    bad = [(lambda: lib.ddimx_inpaint_residual(None, _lib.ptr(de), _lib.ptr(dy), _lib.ptr(dm), _lib.ptr(x0), _lib.ptr(seed),
                                               _lib.ptr(part), _lib.ptr(coef), _lib.ptr(ctr), B, per, s), "null"),
           (lambda: lib.ddimx_inpaint_residual(_lib.ptr(dxt), _lib.ptr(de), _lib.ptr(dy), _lib.ptr(dm), _lib.ptr(x0), _lib.ptr(seed),
                                               _lib.ptr(part), _lib.ptr(coef), _lib.ptr(ctr), B, per - 2, s), "multiple of 4"),
           (lambda: lib.ddimx_inpaint_update(_lib.ptr(dxt), _lib.ptr(de), None, _lib.ptr(x0), _lib.ptr(dy), _lib.ptr(dm), None,
                                             _lib.ptr(part), _lib.ptr(coef), _lib.ptr(ctr), B, per, 2, s), "d_x"),
           (lambda: lib.ddimx_inpaint_update(_lib.ptr(dxt), _lib.ptr(de), None, _lib.ptr(x0), None, _lib.ptr(dm), None,
                                             None, _lib.ptr(coef), _lib.ptr(ctr), B, per, 1, s), "y and mask"),
           (lambda: lib.ddimx_inpaint_update(_lib.ptr(dxt), _lib.ptr(de), None, _lib.ptr(x0), _lib.ptr(dy), _lib.ptr(dm), None,
                                             None, _lib.ptr(coef), _lib.ptr(ctr), B, per, 4, s), "flags"),
           (lambda: lib.ddimx_inpaint_update(_lib.ptr(dxt), _lib.ptr(de), None, _lib.ptr(x0), None, None, None,
                                             None, _lib.ptr(coef), _lib.ptr(ctr), 0, per, 0, s), "B = 0")]
    for call, msg in bad:
        assert call() != 0
        assert msg in lib.ddimx_last_error().decode()
    assert lib.ddimx_inpaint_partials_floats(B, per + 2) == -1


# ---- 9. long sequence -----------------------------------------------------------------------------------------------------------
def test_t8192_guided_bf16():
    cfg, m = MH.build("audio", "torch.cuda.BFloat16Tensor", 5, mode="eval", dropout=DROPOUT)
    shape = (1, 2, 8192, 256)
    x, y = MH.pair_data("inp.long", shape)
    mask = _mask("gap", shape)
    xs, x0 = D.inpaint_steps(x.cuda(), [0, 500], m, MH.alphas(cfg), [-1], y=y, mask=mask, guidance=0.3, replace=True)
    assert torch.isfinite(xs[-1]).all() and torch.isfinite(x0[-1]).all()
    MH.known_exact(xs[-1], y, mask)
