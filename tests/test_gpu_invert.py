"""DDIM inversion with fixed-point refinement and latent slerp on the GPU (ddim_audio_amd.invert_steps / slerp,
ddimx_invert_update, ddimx_slerp).

The update kernel alone: its x0 against ddimx_ddim_update's bit for bit, its x_new against fp64 arithmetic on its own fp32
operands within a bound counted from its roundings, the base-point rule, the residual log.  The whole sampler replayed / forked
against the eager, unforked launches bit for bit and row by row against that bound; against the fp64 restatement written from the
equations (tests/invert_ref.py) driving the CPU oracle within model_harness's gates; the contraction of the round-trip error
with ``iters`` and the order of convergence against a closed-form solution; batch independence, in-place semantics, graph
ownership; the slerp kernel against fp64 and end to end between two inverted clips."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, synth
from ddim_audio_amd.invert import InvertStepper
from ddim_audio_amd.schedule import invert_coefficients, logsnr_seq, make_seq
from oracle import ref_cpu
import gpu_util as G
import model_harness as MH
from model_harness import MODES, MODE_IDS, TINY, U
import invert_ref as IR
import solver_ref as R

pytestmark = pytest.mark.gpu
VAR = 0.25           # data variance of the Gaussian model
# the network's fixed-point iteration contracts on these grids (synth.fill_module's random weights are expansive on coarse ones)
FINE, MEDIUM = [0, 20, 40, 60, 80], [0, 100, 200, 300, 400]


def _f64(v):
    return v.detach().cpu().double().numpy()


def _sample_norm(v):
    return np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(axis=1))


# ---- the rounding bound -------------------------------------------------------------------------------------------------------------
def _fp64_row(x, e, base, row):
    """One row in fp64 on fp32 operands (float64 arrays holding fp32 values; row: the fp32 table row as float64).  Returns
    (x_new, x0, bound on |kernel x_new - x_new|, bound on |kernel x0 - x0|).

    x_new = fma(e, q, p * base) rounds twice: the product, then the fma.  Each rounding errs by at most 2^-24 of its result, and
    both results are at most |p base| + |q e|; so |error| <= 2 * 2^-24 * (|p base| + |q e|) to first order, and one more unit
    covers the second-order term.  x0: the fma and the division, 2 roundings (+ 1) of at most (|x| + |s1 e|) / s2."""
    _, s1, s2, p, q, _ = row
    top = (np.abs(x) + np.abs(s1 * e)) / s2
    return p * base + q * e, (x - s1 * e) / s2, 3 * (U * (np.abs(p * base) + np.abs(q * e)) + TINY), 3 * (U * top + TINY)


def _update(xt, eps, base, x0, log, coef, ctr, partials=None):
    lib = _lib.load()
    b, per = xt.size(0), xt[0].numel()
    if partials is None:
        partials = torch.empty(int(lib.ddimx_invert_partials_doubles(b, per)), dtype=torch.float64, device=xt.device)
    _lib.check(lib.ddimx_invert_update(_lib.ptr(xt), _lib.ptr(eps), _lib.ptr(base), _lib.ptr(x0), _lib.ptr(partials), _lib.ptr(log),
                                       log.size(0), _lib.ptr(coef), _lib.ptr(ctr), b, per, _lib.stream()))
    torch.cuda.synchronize()


# ---- 1. the kernel through the C ABI ------------------------------------------------------------------------------------------------
N_STRIDE = 4 * (2048 * 256 + 1000)  # per sample: more float4s than a sample's blocks have threads, the grid-stride loop runs again


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [20, 3 * 5132, N_STRIDE])
def test_kernel_rows_vs_fp64(n, B):
    lib, dev = _lib.load(), G.dev()
    a = MH.alphas()
    seq, iters = logsnr_seq(a, 20), 2
    c32 = invert_coefficients(seq, a, iters).astype(np.float32)
    rows = c32.shape[0]
    coef = torch.from_numpy(c32).to(dev)
    # ddim_update's table with the same (s1, s2): its x0 does not depend on the other columns
    c6 = c32.copy()
    c6[:, 3], c6[:, 4], c6[:, 5] = 1.0, 0.0, 0.0
    coef6 = torch.from_numpy(c6).to(dev)
    tag = f"inv.k.{n}.{B}"
    x, e, b0 = (synth.gaussian(f"{tag}.{s}", (B, n)) for s in "xeb")
    worst = rworst = 0.0
    for k in (0, 1, 6, 7, rows - 2, rows - 1):
        row = c32[k].astype(np.float64)
        first = bool(row[5] != 0)
        assert first == (k % 2 == 0)
        ctr = torch.full((1,), k, dtype=torch.int32, device=dev)
        xt, x0 = x.to(dev), torch.full((B, n), float("nan"), device=dev)
        # a first row never reads base: NaN there must not reach any output
        base = torch.full((B, n), float("nan"), device=dev) if first else b0.to(dev)
        log = torch.full((rows, B), -7.0, device=dev)
        _update(xt, e.to(dev), base, x0, log, coef, ctr)
        want, _, bound, _ = _fp64_row(_f64(x), _f64(e), _f64(x if first else b0), row)
        got = _f64(xt)
        assert np.isfinite(got).all() and bool(torch.isfinite(x0).all())
        assert (np.abs(got - want) <= bound).all(), f"row {k}: worst {np.max(np.abs(got - want) / bound):.3f} x bound"
        worst = max(worst, float(np.max(np.abs(got - want) / bound)))
        assert torch.equal(base.cpu(), x if first else b0), "base: x_old exactly after a first row, untouched otherwise"
        # x0 is ddim_update's prediction from the same (x, e, s1, s2), bit for bit
        ref_x, ref_x0 = x.to(dev).view(-1), torch.empty(B * n, device=dev)
        _lib.check(lib.ddimx_ddim_update(_lib.ptr(ref_x), _lib.ptr(e.to(dev)), None, _lib.ptr(ref_x0), _lib.ptr(coef6), _lib.ptr(ctr),
                                         B * n, _lib.stream()))
        torch.cuda.synchronize()
        assert torch.equal(x0.view(-1), ref_x0)
        # the residual: fp64 on the same fp32 operands (the kernel's own x_new and x_old)
        r = _sample_norm(got - _f64(x)) / _sample_norm(got)
        lg = _f64(log)
        assert (np.abs(lg[k] - r) <= 1e-6 * r).all(), (k, lg[k], r)
        rworst = max(rworst, float(np.max(np.abs(lg[k] - r) / r)))
        assert (np.delete(lg, k, axis=0) == -7.0).all(), "the other rows of the log are untouched"
    print(f"[invert kernel n {n} B {B}] worst error {worst:.3f} x the rounding bound; residual log worst {rworst:.2e} relative")


def test_kernel_zero_norm_and_counter_outside_the_table():
    dev = G.dev()
    coef = torch.tensor([[5.0, 0.6, 0.8, 0.8, 0.6, 1.0], [5.0, 0.6, 0.8, 0.9, 0.2, 0.0]], device=dev)
    z = torch.zeros(2, 16, device=dev)
    log = torch.full((2, 2), -7.0, device=dev)
    xt, base, x0 = z.clone(), torch.full_like(z, float("nan")), torch.full_like(z, float("nan"))
    _update(xt, z, base, x0, log, coef, torch.zeros(1, dtype=torch.int32, device=dev))
    assert log.cpu().tolist() == [[0.0, 0.0], [-7.0, -7.0]], "r = 0 when |x_new| = 0"
    assert torch.equal(xt, z) and torch.equal(x0, z) and torch.equal(base, z)
    # a counter past the table (a replay too many) reads and writes nothing
    for k in (2, -1):
        xt, x0 = torch.ones_like(z), torch.full_like(z, 3.0)
        _update(xt, torch.ones_like(z), base, x0, log, coef, torch.full((1,), k, dtype=torch.int32, device=dev))
        assert bool((xt == 1).all()) and bool((x0 == 3).all()) and log.cpu().tolist() == [[0.0, 0.0], [-7.0, -7.0]]


def test_kernels_validate_before_the_launch():
    lib, dev = _lib.load(), G.dev()
    x = torch.zeros(2, 16, device=dev)
    pd = torch.zeros(64, dtype=torch.float64, device=dev)
    log = torch.zeros(1, 2, device=dev)
    coef = torch.zeros(1, 6, device=dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    P, s = _lib.ptr, _lib.stream()
    inv = lib.ddimx_invert_update
    bad = [(lambda: inv(None, P(x), P(x), P(x), P(pd), P(log), 1, P(coef), P(ctr), 2, 16, s), "null"),
           (lambda: inv(P(x), P(x), None, P(x), P(pd), P(log), 1, P(coef), P(ctr), 2, 16, s), "null"),
           (lambda: inv(P(x), P(x), P(x), P(x), None, P(log), 1, P(coef), P(ctr), 2, 16, s), "null"),
           (lambda: inv(P(x), P(x), P(x), P(x), P(pd), None, 1, P(coef), P(ctr), 2, 16, s), "null"),
           (lambda: inv(P(x), P(x), P(x), P(x), P(pd), P(log), 1, P(coef), None, 2, 16, s), "null"),
           (lambda: inv(P(x), P(x), P(x), P(x), P(pd), P(log), 0, P(coef), P(ctr), 2, 16, s), "rows"),
           (lambda: inv(P(x), P(x), P(x), P(x), P(pd), P(log), 1, P(coef), P(ctr), 0, 16, s), "B ="),
           (lambda: inv(P(x), P(x), P(x), P(x), P(pd), P(log), 1, P(coef), P(ctr), 65536, 16, s), "B ="),
           (lambda: inv(P(x), P(x), P(x), P(x), P(pd), P(log), 1, P(coef), P(ctr), 2, 14, s), "per_sample"),
           (lambda: inv(P(x), P(x), P(x), P(x), P(pd), P(log), 1, P(coef), P(ctr), 2, 0, s), "per_sample"),
           (lambda: lib.ddimx_slerp(None, P(x), P(x), 1, P(x), P(pd), 2, 16, s), "null"),
           (lambda: lib.ddimx_slerp(P(x), P(x), None, 1, P(x), P(pd), 2, 16, s), "null"),
           (lambda: lib.ddimx_slerp(P(x), P(x), P(x), 1, P(x), None, 2, 16, s), "null"),
           (lambda: lib.ddimx_slerp(P(x), P(x), P(x), 0, P(x), P(pd), 2, 16, s), "M ="),
           (lambda: lib.ddimx_slerp(P(x), P(x), P(x), 1, P(x), P(pd), 0, 16, s), "P ="),
           (lambda: lib.ddimx_slerp(P(x), P(x), P(x), 1, P(x), P(pd), 2, 18, s), "per_sample")]
    for call, msg in bad:
        assert call() != 0
        assert msg in lib.ddimx_last_error().decode()
    assert lib.ddimx_invert_partials_doubles(2, 14) == -1 and lib.ddimx_invert_partials_doubles(0, 16) == -1
    assert lib.ddimx_invert_partials_doubles(2, 16) == 2 * 1 * 3
    with pytest.raises(ValueError, match="first"):
        InvertStepper(None, torch.zeros(1, 2, 16, 32, device=dev), invert_coefficients([0, 5], MH.alphas(), 2)[1:])


# ---- 2. the whole sampler: replay and fork change nothing; every row meets the rounding bound ---------------------------------
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("rows", [3, 12], ids=["eager", "replayed"])
@pytest.mark.parametrize("name", ["tiny", "audio"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_sampler_replayed_equals_recorded_eager_and_meets_the_bound(mode, name, rows, iters):
    cfg, m = MH.build(name, mode[0], 5, mode="eval")
    x = synth.gaussian("inv.run", (4, 2, 32, cfg.model.f_size))  # B = 4: the captured graph forks into two shards
    n = rows // iters
    seq, a = list(range(0, 20 * n, 20)), MH.alphas(cfg)  # a fine grid: the random-weight network is no denoiser
    st, e_st = {}, {}
    xs, x0 = D.invert_steps(x.cuda(), seq, m, a, None, iters=iters, stats=st)
    # the same run through the non-native branch: model(x, t) as any callable, every launch eager and unforked
    rec_x, rec_e = [], []

    def recording(xt, t):
        e = m(xt, t, _fork=False)
        rec_x.append(xt.clone())
        rec_e.append(e.clone())
        return e

    with MH.eager_steps():
        e_xs, e_x0 = D.invert_steps(x.cuda(), seq, recording, a, None, iters=iters, stats=e_st)
    assert len(rec_e) == rows and len(xs) == n + 1 and len(x0) == n
    for i in range(n):
        assert torch.equal(xs[i + 1], e_xs[i + 1]), f"xs[{i + 1}]"
        assert torch.equal(x0[i], e_x0[i]), f"x0_preds[{i}]"
    r, e_r = st["residual"], e_st["residual"]
    assert r.shape == (n, iters, 4) and r.dtype == torch.float32 and not r.is_cuda
    assert bool(torch.isfinite(r).all()) and bool((r > 0).all())
    assert bool(((r - e_r).abs() <= 1e-6 * e_r).all())
    # every row recombined in fp64 from the recorded (x_old, eps); x_new is the next row's recorded input, or the level's copy
    c32 = invert_coefficients(seq, a, iters).astype(np.float32).astype(np.float64)
    worst = 0.0
    for k in range(rows):
        lvl, it = divmod(k, iters)
        base = _f64(rec_x[lvl * iters])
        assert it != 0 or torch.equal(rec_x[k].cpu(), x if lvl == 0 else xs[lvl]), "a level starts from the one below"
        new = _f64(xs[lvl + 1]) if it == iters - 1 else _f64(rec_x[k + 1])
        u, p0, bu, bp = _fp64_row(_f64(rec_x[k]), _f64(rec_e[k]), base, c32[k])
        assert (np.abs(new - u) <= bu).all(), f"row {k}: {np.max(np.abs(new - u) / bu):.3f} x bound"
        worst = max(worst, float(np.max(np.abs(new - u) / bu)))
        if it == iters - 1:
            assert (np.abs(_f64(x0[lvl]) - p0) <= bp).all(), f"row {k}: x0 {np.max(np.abs(_f64(x0[lvl]) - p0) / bp):.3f} x bound"
        rr = _sample_norm(new - _f64(rec_x[k])) / _sample_norm(new)
        assert (np.abs(_f64(r[lvl, it]) - rr) <= 1e-6 * rr).all()
    print(f"[invert sampler {name} {MODE_IDS[mode[1]]} rows {rows} iters {iters}] worst row error {worst:.3f} x the rounding bound; "
          f"residuals {float(r.min()):.3e} .. {float(r.max()):.3e}")


# ---- 3. against the restatement driving the CPU oracle -------------------------------------------------------------------------
# f32 mode: the worst relative difference between stats["residual"] and the restatement's over every case below, measured on
# an MI355X, is 4.8e-5 (iters = 3 at level 0, where the third residual is 2.6e-5: the network's fp32 error of ~1e-5 sigma is
# divided by it; 3.4e-6 with iters = 2, 1.2e-7 with iters = 1, where the log only sees the kernel's own rounding).  The gate is
# 4 x the measured value.  bf16 is printed, not gated: its eps error (1e-2 sigma) exceeds the smallest residuals.
RESIDUAL_MEASURED = 4.8e-5
RESIDUAL_GATE = 4 * RESIDUAL_MEASURED


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("seq", [FINE, MEDIUM], ids=["fine", "medium"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_sampler_vs_reference(mode, seq, iters):
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 5, mode="eval")
    a = MH.alphas(cfg)
    live, ocfg = MH.oracle(m, "tiny")
    sd = {k: v.detach() for k, v in live.items()}

    def ref_fn(xn, t):
        with torch.no_grad():
            xt = torch.from_numpy(xn).float()
            return ref_cpu.model_forward(sd, ocfg, xt, torch.full((xt.size(0),), int(t), dtype=torch.long)).double().numpy()

    x = synth.gaussian("inv.ref", (2, 2, 16, 32))
    st = {}
    xs, x0 = D.invert_steps(x.cuda(), seq, m, a, None, iters=iters, stats=st)
    rxs, rx0, rres = IR.invert_steps(x.double().numpy(), seq, ref_fn, a, iters)
    assert len(xs) == len(seq) + 1 and len(x0) == len(seq)
    for i in range(len(seq)):
        mx, er = MH.gate(xs[i + 1], torch.from_numpy(rxs[i + 1]), dt, f"xs[{i + 1}] iters {iters}")
        MH.gate(x0[i], torch.from_numpy(rx0[i]), dt, f"x0[{i}] iters {iters}")
    got = _f64(st["residual"])
    rel = float(np.max(np.abs(got - rres) / rres))
    print(f"[invert vs reference {MODE_IDS[dt]} seq {seq} iters {iters}] final max {mx:.3e} rms err {er:.3e} x rms; latent rms "
          f"{float(xs[-1].square().mean().sqrt()):.3f}; residuals {rres.min():.3e} .. {rres.max():.3e}, worst relative difference "
          f"{rel:.3e}")
    if dt == G.F32:
        assert rel <= RESIDUAL_GATE, f"residual log: {rel:.3e}"


# ---- 4. contraction and order on the HIP path ------------------------------------------------------------------------------------
def _gaussian_callable(a):
    a64 = a.double()
    gain = ((1.0 - a64).sqrt() / (a64 * VAR + 1.0 - a64)).float().cuda()  # eps(x, t) = gain[t] x
    return lambda x, t: x * gain[t].view(-1, 1, 1, 1)


def _round_trip(x, seq, model, a, iters):
    lat = D.invert_steps(x.cuda(), seq, model, a, [-1], iters=iters)[0][-1]
    back = D.generalized_steps(lat.cuda(), seq, model, a, [-1], eta=0.0)[0][-1]
    return float((back.double() - x.double()).abs().max() / x.double().abs().max())


def test_round_trip_and_order_on_the_gpu():
    """tests/test_invert_cpu.py's conditions 3 and 4 with the update running in the kernel and the decode by generalized_steps:
    the Gaussian model as a GPU callable.  fp32 puts a floor under the round trip (an emulation gave 9e-7), so error(8) <= 1e-6
    becomes error(8) <= error(1) / 1000."""
    a = MH.alphas()
    model = _gaussian_callable(a)
    x = 0.5 * synth.gaussian("inv.conv", (2, 2, 32, 256))
    seq = make_seq(1000, 50)
    e = {k: _round_trip(x, seq, model, a, k) for k in (1, 2, 3, 4, 5, 8)}
    for k, v in sorted(e.items()):
        print(f"[round trip gpu] uniform 50 steps, iters {k}: {v:.3e}")
    print(f"[round trip gpu] fp32 floor (iters 8): {e[8]:.3e}")
    for k in (1, 2, 3):
        assert e[k + 1] <= e[k] / 5, (k, e[k], e[k + 1])
    assert e[8] <= e[1] / 1000
    coarse = make_seq(1000, 10)
    c1, c8 = _round_trip(x, coarse, model, a, 1), _round_trip(x, coarse, model, a, 8)
    print(f"[round trip gpu] uniform 10 steps, iters 1: {c1:.3e}, iters 8: {c8:.3e}")
    assert c8 <= c1 / 100

    def latent_error(s):
        lat = D.invert_steps(x.cuda(), s, model, a, [-1], iters=8)[0][-1]
        want = x.double().numpy() / R.gaussian_exact(a, VAR, np.ones(1), s[-1])
        return float(np.abs(lat.double().numpy() - want).max() / np.abs(want).max())

    for name, grid in (("uniform", lambda n: make_seq(1000, n)), ("logsnr", lambda n: logsnr_seq(a, n))):
        le = {n: latent_error(grid(n)) for n in (25, 50, 100)}
        print(f"[latent vs closed form gpu] {name} grid, iters 8: " + ", ".join(f"{n}: {v:.3e}" for n, v in le.items())
              + f"; ratios {le[25] / le[50]:.3f}, {le[50] / le[100]:.3f}")
        assert 1.6 <= le[25] / le[50] <= 2.5
        assert 1.6 <= le[50] / le[100] <= 2.5


# ---- 5. batch independence, in-place semantics, ownership ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_sample_result_does_not_depend_on_the_batch(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    x = synth.gaussian("inv.indep", (3, 2, 16, 32))
    st, solo_st = {}, {}
    xs, x0 = D.invert_steps(x.cuda(), FINE, m, a, None, iters=2, stats=st)
    solo_xs, solo_x0 = D.invert_steps(x[:1].cuda(), FINE, m, a, None, iters=2, stats=solo_st)
    for i in range(len(FINE)):
        assert torch.equal(xs[i + 1][0], solo_xs[i + 1][0]) and torch.equal(x0[i][0], solo_x0[i][0]), i
    # the log's reduction order depends on the launch shape (blocks per sample), which depends on B: equal to rounding
    assert bool(((st["residual"][:, :, :1] - solo_st["residual"]).abs() <= 1e-6 * solo_st["residual"]).all())


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_in_place_semantics_and_select_index(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    x = synth.gaussian("inv.inplace", (4, 2, 16, 32))
    n = len(FINE)
    xin = x.cuda()
    xs, x0 = D.invert_steps(xin, FINE, m, a, None, iters=2)
    assert xs[0] is xin and len(xs) == n + 1 and len(x0) == n
    assert all(not v.is_cuda for v in xs[1:] + x0)
    assert torch.equal(xin.cpu(), xs[-1]), "a contiguous fp32 GPU x is updated in place"
    # select_index counts levels, as generalized_steps counts iterations
    sxs, sx0 = D.invert_steps(x.cuda(), FINE, m, a, [0, -1], iters=2)
    assert len(sxs) == 3 and len(sx0) == 2
    assert torch.equal(sxs[1], xs[1]) and torch.equal(sxs[2], xs[-1]) and torch.equal(sx0[0], x0[0]) and torch.equal(sx0[1], x0[-1])
    lxs, lx0 = D.invert_steps(x.cuda(), FINE, m, a, [-1], iters=2)
    assert len(lxs) == 2 and len(lx0) == 1 and torch.equal(lxs[-1], xs[-1])
    # a CPU x is copied, not written
    keep = x.clone()
    cxs, _ = D.invert_steps(x, FINE, m, a, [-1], iters=2)
    assert cxs[0] is x and torch.equal(x, keep) and torch.equal(cxs[-1], xs[-1])
    # stats is optional and only written when given
    st = {}
    D.invert_steps(x.cuda(), FINE, m, a, [-1], iters=2, stats=st)
    assert set(st) == {"residual"} and st["residual"].shape == (n, 2, 4)


def test_stepper_recaptures_when_the_model_moves_on_and_close_destroys_the_graph_first():
    """As test_gpu_solver's test of MultistepStepper: ownership, staleness and re-capture are GraphOwner's /
    DDIMStepper's, unchanged."""
    cfg, m = MH.build("audio", "torch.cuda.BFloat16Tensor", 0, mode="eval")
    a = MH.alphas(cfg)
    coef = invert_coefficients(list(range(0, 100, 20)), a, 2)  # 10 rows
    x = synth.gaussian("inv.own", (5, 2, 64, 256)).cuda()

    def run(disturb):
        xt = x.clone()
        with torch.no_grad():
            st = InvertStepper(m, xt, coef)
            for i in range(coef.shape[0]):
                disturb(i, st)
                st.step()
            torch.cuda.synchronize()
            out = (xt.clone(), st.x0.clone(), st.base.clone(), st.log.clone(), st.captures)
            st.close()
        assert st.graph is None and st._ctx is None and st._refs is None
        return out

    ref = run(lambda i, st: None)
    assert ref[4] == 1

    def move(i, st):
        if i == 4:
            assert st.graph is not None and st._ctx is not None and len(st._refs) >= 5
            m.float()  # nn.Module._apply: the model drops its packed weights, tables, workspaces, embedding table
            assert m._packed is None and m._workspace is None

    def grow(i, st):
        if i == 4:
            m.reserve(x.device, 9, 64, 0)  # what a forward of a larger batch does first: a new, larger workspace

    for disturb in (move, grow):
        got = run(disturb)
        assert got[4] == 2, "the stepper must re-capture after the model re-allocated its buffers"
        assert all(torch.equal(u, v) for u, v in zip(got[:4], ref[:4]))


# ---- 6. slerp -------------------------------------------------------------------------------------------------------------------------
WEIGHTS = np.arange(0.0, 1.01, 0.1)  # the reference's sample_interpolation: 11 weights, 0 .. 1


@pytest.mark.parametrize("P,shape", [(1, (2, 16, 32)), (3, (2, 16, 32)), (3, (1, 1, 20)), (1, (2, 1030, 512))],
                         ids=["p1", "p3", "p3-small", "p1-grid-stride"])
def test_slerp_kernel_vs_fp64(P, shape):
    """Per element the kernel rounds 4 times: a and b once each, the product a z1, the fma.  Each errs by at most 2^-24 of a
    quantity bounded by |a z1| + |b z2|.  theta's own error is negligible beside that: the three sums are in double (at most
    2^21 terms here, each product exact, relative error below 2^21 * 2^-53 = 2^-32 each), and around theta = pi / 2 -- random
    inputs -- the coefficients are as well conditioned as theta."""
    z1, z2 = synth.gaussian(f"slerp.a.{P}.{shape}", (P,) + shape), 1.7 * synth.gaussian(f"slerp.b.{P}.{shape}", (P,) + shape)
    w32 = WEIGHTS.astype(np.float32)
    assert w32[0] == 0.0 and w32[-1] == 1.0 and len(w32) == 11
    out = D.slerp(z1.cuda(), z2.cuda(), WEIGHTS)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (P * 11,) + shape
    got = _f64(out).reshape((P, 11) + shape)
    assert np.isfinite(got).all()
    worst = 0.0
    for p in range(P):
        ca, cb = IR.slerp_coefficients(_f64(z1[p]), _f64(z2[p]), w32.astype(np.float64))
        for mi in range(11):
            ta, tb = ca[mi] * _f64(z1[p]), cb[mi] * _f64(z2[p])
            bound = 4 * (U * (np.abs(ta) + np.abs(tb)) + TINY)
            d = np.abs(got[p, mi] - (ta + tb))
            assert (d <= bound).all(), f"pair {p} weight {mi}: {np.max(d / bound):.3f} x bound"
            worst = max(worst, float(np.max(d / bound)))
    o = out.cpu().view((P, 11) + shape)
    assert torch.equal(o[:, 0], z1) and torch.equal(o[:, -1], z2), "w = 0 / 1 return the inputs bit for bit"
    print(f"[slerp kernel P {P} {shape}] worst error {worst:.3f} x the rounding bound")
    # CPU inputs and a weights tensor are accepted; the result is the same
    assert torch.equal(D.slerp(z1, z2, torch.from_numpy(w32)), out)


def test_slerp_parallel_and_zero_inputs_give_the_straight_line():
    z = synth.gaussian("slerp.same", (3, 2, 16, 32))
    w32 = WEIGHTS.astype(np.float32)
    a32, b32 = (1.0 - w32.astype(np.float64)).astype(np.float32).astype(np.float64), w32.astype(np.float64)
    for u, v in ((z, z), (z, 2.0 * z), (torch.zeros_like(z), z), (z, torch.zeros_like(z))):
        out = D.slerp(u.cuda(), v.cuda(), WEIGHTS).cpu().view(3, 11, 2, 16, 32)
        assert bool(torch.isfinite(out).all())
        for mi in range(11):
            ta, tb = a32[mi] * _f64(u), b32[mi] * _f64(v)  # the coefficients are exact in fp32 up to their one rounding
            assert (np.abs(_f64(out[:, mi]) - (ta + tb)) <= 3 * (U * (np.abs(ta) + np.abs(tb)) + TINY)).all(), mi
        assert torch.equal(out[:, 0], u) and torch.equal(out[:, -1], v)


def test_interpolation_between_two_inverted_clips():
    """Invert two clips, slerp the latents at [0, 0.5, 1], decode: the ends reproduce the clips, the middle is a sample of the
    same scale.  Gaussian model as a GPU callable; the yardstick is the naive (iters = 1) round trip of the same clips."""
    a = MH.alphas()
    model = _gaussian_callable(a)
    clips = 0.5 * synth.gaussian("slerp.clips", (2, 2, 32, 256))
    seq = make_seq(1000, 50)
    naive = _round_trip(clips, seq, model, a, 1)
    lat = D.invert_steps(clips.cuda(), seq, model, a, [-1], iters=5)[0][-1]
    z = D.slerp(lat[:1], lat[1:], [0.0, 0.5, 1.0])
    assert tuple(z.shape) == (3, 2, 32, 256) and torch.equal(z[0].cpu(), lat[0]) and torch.equal(z[2].cpu(), lat[1])
    out = D.generalized_steps(z, seq, model, a, [-1], eta=0.0)[0][-1]
    err = [float((out[i].double() - clips[j].double()).abs().max() / clips[j].double().abs().max()) for i, j in ((0, 0), (2, 1))]
    rms = [float(v.double().square().mean().sqrt()) for v in (clips[0], clips[1], out[1])]
    print(f"[interpolation] naive round trip {naive:.3e}; ends after iters = 5: {err[0]:.3e}, {err[1]:.3e}; rms of the clips "
          f"{rms[0]:.3f}, {rms[1]:.3f}, of the midpoint {rms[2]:.3f}")
    assert max(err) <= naive / 1000
    assert bool(torch.isfinite(out[1]).all())
    assert 0.5 * min(rms[:2]) <= rms[2] <= 2.0 * max(rms[:2])
