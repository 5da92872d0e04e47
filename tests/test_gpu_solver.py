"""DPM-Solver++ multistep sampler on the GPU (ddim_audio_amd.dpm_solver_steps, ddimx_multistep_update).

Order 1 against generalized_steps bit for bit; the kernel alone against fp64 arithmetic on its own fp32 operands within a bound
counted from its roundings; the whole sampler replayed / forked against the eager, unforked launches bit for bit and step by step
against that bound; against the fp64 restatement in the paper's form (tests/solver_ref.py) driving the CPU oracle within
model_harness's gates; the order of convergence against a closed-form solution; graph ownership and batch independence."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, synth
from ddim_audio_amd.schedule import ddim_coefficients, dpm_coefficients, logsnr_seq, make_seq
from ddim_audio_amd.solver import MultistepStepper
from oracle import ref_cpu
import gpu_util as G
import model_harness as MH
from model_harness import MODES, MODE_IDS, TINY, U
import solver_ref as R

pytestmark = pytest.mark.gpu


# ---- the rounding bound -------------------------------------------------------------------------------------------------------------
def _fp64_step(x, e, m1, m2, row):
    """One update in fp64 on fp32 operands (x, e, m1, m2: float64 arrays holding fp32 values; row: the fp32 table row as float64).
    Returns (u, m0, bound on |kernel u - u|, bound on |kernel m0 - m0|).

    The kernel rounds 8 times: fma and division (m0), product, fma (the DDIM bracket), subtraction and fma (first history term),
    subtraction and fma (second).  Each rounding errs by at most 2^-24 of its result, and every result -- carried to the output
    through the factors s3 + w1, 1, w1, w2 it is multiplied by afterwards -- is at most
        S = (|s3| + |w1|) (|x| + |s1 e|) / s2 + |c2 e| + |w1| (|m0| + |m1|) + |w2| (|m1| + |m2|),
    the sum of the magnitudes of the terms.  So |error| <= 8 * 2^-24 * S to first order; one more unit covers the second-order
    terms.  m0 alone: 2 roundings (+ 1) of at most (|x| + |s1 e|) / s2."""
    _, s1, s2, s3, c2, _, w1, w2 = row
    m0 = (x - s1 * e) / s2
    u = s3 * m0 + c2 * e
    top = (np.abs(x) + np.abs(s1 * e)) / s2
    S = (abs(s3) + abs(w1)) * top + np.abs(c2 * e)
    if w1 != 0.0:
        u = u + w1 * (m0 - m1)
        S = S + abs(w1) * (np.abs(m0) + np.abs(m1))
    if w2 != 0.0:
        u = u + w2 * (m1 - m2)
        S = S + abs(w2) * (np.abs(m1) + np.abs(m2))
    return u, m0, 9 * (U * S + TINY), 3 * (U * top + TINY)


def _update(xt, eps, x0, hist, coef, ctr):
    lib = _lib.load()
    _lib.check(lib.ddimx_multistep_update(_lib.ptr(xt), _lib.ptr(eps), _lib.ptr(x0), _lib.ptr(hist), _lib.ptr(coef), _lib.ptr(ctr),
                                          xt.numel(), _lib.stream()))
    torch.cuda.synchronize()


# ---- 1. order 1 = generalized_steps(eta=0), bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 10], ids=["eager", "replayed"])
@pytest.mark.parametrize("name", ["tiny", "audio"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_order1_equals_generalized_steps(mode, name, n):
    cfg, m = MH.build(name, mode[0], 5, mode="eval")
    x = synth.gaussian("dpm.o1", (4, 2, 32, cfg.model.f_size))  # B = 4: the captured graph forks into two shards
    seq = list(range(0, 1000, 1000 // n))[:n]
    a = MH.alphas(cfg)
    want_xs, want_x0 = D.generalized_steps(x.cuda(), seq, m, a, None, eta=0.0)
    xin = x.cuda()
    xs, x0 = D.dpm_solver_steps(xin, seq, m, a, None, order=1)
    assert xs[0] is xin and len(xs) == len(want_xs) == n + 1 and len(x0) == n
    for i in range(1, n + 1):
        assert torch.equal(xs[i], want_xs[i]), f"xs[{i}]"
        assert torch.equal(x0[i - 1], want_x0[i - 1]), f"x0_preds[{i - 1}]"
    assert torch.equal(xin.cpu(), xs[-1]), "a contiguous fp32 GPU x is updated in place"
    # select_index as generalized_steps reads it
    sxs, sx0 = D.dpm_solver_steps(x.cuda(), seq, m, a, [0, -1], order=1)
    assert len(sxs) == 3 and len(sx0) == 2 and torch.equal(sxs[1], xs[1]) and torch.equal(sxs[2], xs[-1])


# ---- 2. the kernel through the C ABI ------------------------------------------------------------------------------------------------
N_STRIDE = 4 * (2048 * 256 + 1000)  # more float4s than the grid has threads: the grid-stride loop runs twice


@pytest.mark.parametrize("n", [20, 3 * 5132, N_STRIDE])
def test_kernel_first_order_row_ignores_the_history(n):
    """A row with w1 = w2 = 0: ddim_update's bits, with NaN in both history buffers; x0 <- m0, hist <- the old x0 (NaN)."""
    lib, dev = _lib.load(), G.dev()
    a = MH.alphas()
    seq = logsnr_seq(a, 20)
    c8 = torch.from_numpy(dpm_coefficients(seq, a, 1).astype(np.float32)).to(dev)
    c6 = torch.from_numpy(ddim_coefficients(seq, a, 0.0).astype(np.float32)).to(dev)
    x, e = synth.gaussian(f"dpm.k1.x.{n}", (n,)).to(dev), synth.gaussian(f"dpm.k1.e.{n}", (n,)).to(dev)
    for k in (0, 7, len(seq) - 1):
        ctr = torch.full((1,), k, dtype=torch.int32, device=dev)
        want_x, want_x0 = x.clone(), torch.empty_like(x)
        _lib.check(lib.ddimx_ddim_update(_lib.ptr(want_x), _lib.ptr(e), None, _lib.ptr(want_x0), _lib.ptr(c6), _lib.ptr(ctr), n,
                                         _lib.stream()))
        for with_hist in (True, False):
            xt, x0 = x.clone(), torch.full_like(x, float("nan"))
            hist = torch.full_like(x, float("nan")) if with_hist else None
            _update(xt, e, x0, hist, c8, ctr)
            assert torch.equal(xt, want_x) and torch.equal(x0, want_x0), (k, with_hist)
            assert hist is None or bool(torch.isnan(hist).all())


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("n", [20, 3 * 5132, N_STRIDE])
def test_kernel_history_rows_vs_fp64(n, order):
    """Rows of order 2 and 3 of a real table on random operands, one step at a time, against fp64 on the same fp32 inputs."""
    dev = G.dev()
    a = MH.alphas()
    seq = logsnr_seq(a, 20)
    c32 = dpm_coefficients(seq, a, order).astype(np.float32)
    coef = torch.from_numpy(c32).to(dev)
    coef6 = coef[:, :6].contiguous()
    lib = _lib.load()
    tag = f"dpm.k{order}.{n}"
    x, e, m1, m2 = (synth.gaussian(f"{tag}.{s}", (n,)) for s in "xepq")
    worst = 0.0
    for k in (order - 1, 5, 12, len(seq) - 2):
        row = c32[k].astype(np.float64)
        assert row[6] != 0 and (row[7] != 0) == (order == 3)
        ctr = torch.full((1,), k, dtype=torch.int32, device=dev)
        xt, x0, hist = x.to(dev), m1.to(dev), m2.to(dev)
        _update(xt, e.to(dev), x0, hist, coef, ctr)
        u, m0, bu, bm = _fp64_step(*(v.double().numpy() for v in (x, e, m1, m2)), row)
        got_u, got_m = xt.cpu().double().numpy(), x0.cpu().double().numpy()
        assert np.isfinite(got_u).all()
        assert (np.abs(got_u - u) <= bu).all(), f"row {k}: worst {np.max(np.abs(got_u - u) / bu):.3f} x bound"
        assert (np.abs(got_m - m0) <= bm).all(), f"row {k}: x0 worst {np.max(np.abs(got_m - m0) / bm):.3f} x bound"
        worst = max(worst, float(np.max(np.abs(got_u - u) / bu)))
        assert torch.equal(hist.cpu(), m1), "hist must hold the old x0 exactly"
        # x0 is ddim_update's prediction, bit for bit
        ref_x, ref_x0 = x.to(dev), torch.empty(n, device=dev)
        _lib.check(lib.ddimx_ddim_update(_lib.ptr(ref_x), _lib.ptr(e.to(dev)), None, _lib.ptr(ref_x0), _lib.ptr(coef6), _lib.ptr(ctr), n,
                                         _lib.stream()))
        torch.cuda.synchronize()
        assert torch.equal(x0, ref_x0)
        if order == 2:  # no hist buffer at order 2: same bits
            xt2, x02 = x.to(dev), m1.to(dev)
            _update(xt2, e.to(dev), x02, None, coef, ctr)
            assert torch.equal(xt2, xt) and torch.equal(x02, x0)
    print(f"[multistep kernel order {order} n {n}] worst error {worst:.3f} x the rounding bound")


def test_kernel_validates_before_the_launch():
    lib, dev = _lib.load(), G.dev()
    x = torch.zeros(16, device=dev)
    coef = torch.zeros(1, 8, device=dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    P, s = _lib.ptr, _lib.stream()
    bad = [(lambda: lib.ddimx_multistep_update(None, P(x), P(x), None, P(coef), P(ctr), 16, s), "null"),
           (lambda: lib.ddimx_multistep_update(P(x), P(x), None, None, P(coef), P(ctr), 16, s), "null"),
           (lambda: lib.ddimx_multistep_update(P(x), P(x), P(x), None, P(coef), None, 16, s), "null"),
           (lambda: lib.ddimx_multistep_update(P(x), P(x), P(x), None, P(coef), P(ctr), 14, s), "multiple of 4"),
           (lambda: lib.ddimx_multistep_update(P(x), P(x), P(x), None, P(coef), P(ctr), 0, s), "multiple of 4")]
    for call, msg in bad:
        assert call() != 0
        assert msg in lib.ddimx_last_error().decode()
    # the host refuses a table with a second history weight when no hist buffer will exist
    a = MH.alphas()
    with pytest.raises(ValueError, match="order = 3"):
        MultistepStepper(None, torch.zeros(1, 2, 16, 32, device=dev), dpm_coefficients(logsnr_seq(a, 10), a, 3), 2)


# ---- 3. the whole sampler: replay and fork change nothing; every step meets the rounding bound -------------------------------
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("n", [3, 10], ids=["eager", "replayed"])
@pytest.mark.parametrize("name", ["tiny", "audio"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_sampler_replayed_equals_recorded_eager_and_meets_the_bound(mode, name, n, order):
    cfg, m = MH.build(name, mode[0], 5, mode="eval")
    x = synth.gaussian("dpm.run", (4, 2, 32, cfg.model.f_size))
    seq, a = MH.spread(n), MH.alphas(cfg)
    assert len(seq) == n
    xs, x0 = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order)
    # the same run through the non-native branch: model(x, t) as any callable, every launch eager and unforked
    rec = []

    def recording(xt, t):
        e = m(xt, t, _fork=False)
        rec.append(e.clone())
        return e

    with MH.eager_steps():
        e_xs, e_x0 = D.dpm_solver_steps(x.cuda(), seq, recording, a, None, order=order)
    assert len(rec) == n and len(xs) == n + 1 and len(x0) == n
    for i in range(n):
        assert torch.equal(xs[i + 1], e_xs[i + 1]), f"xs[{i + 1}]"
        assert torch.equal(x0[i], e_x0[i]), f"x0_preds[{i}]"
    # (b) every step recombined in fp64 from the recorded eps and the run's own previous outputs
    c32 = dpm_coefficients(seq, a, order).astype(np.float32).astype(np.float64)
    f64 = lambda v: v.cpu().double().numpy()  # noqa: E731
    worst = 0.0
    for k in range(n):
        m1 = f64(x0[k - 1]) if k >= 1 else None
        m2 = f64(x0[k - 2]) if k >= 2 else None
        u, m0, bu, bm = _fp64_step(f64(x if k == 0 else xs[k]), f64(rec[k]), m1, m2, c32[k])
        du, dm = np.abs(f64(xs[k + 1]) - u), np.abs(f64(x0[k]) - m0)
        assert (du <= bu).all() and (dm <= bm).all(), f"step {k}: {np.max(du / bu):.3f} / {np.max(dm / bm):.3f} x bound"
        worst = max(worst, float(np.max(du / bu)))
    assert (c32[1:-1, 6] != 0).all() and ((c32[2:-1, 7] != 0).all() if order == 3 else (c32[:, 7] == 0).all())
    print(f"[multistep sampler {name} {MODE_IDS[mode[1]]} n {n} order {order}] worst step error {worst:.3f} x the rounding bound")


# ---- 4. against the paper's form driving the CPU oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_sampler_vs_reference(mode, order):
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 5, mode="eval")
    a = MH.alphas(cfg)
    seq = logsnr_seq(a, 5)  # five steps: the replayed path
    assert len(seq) == 5
    w = np.abs(dpm_coefficients(seq, a, order)[:, 6:])
    # the step ratios are close to 1 on this grid, so the history terms do not amplify the network's bf16 noise much
    if order == 2:
        assert w[:, 0].max() <= 0.46
    else:
        assert w.sum(1).max() <= 1.5
    live, ocfg = MH.oracle(m, "tiny")
    sd = {k: v.detach() for k, v in live.items()}

    def ref_fn(xn, t):
        with torch.no_grad():
            xt = torch.from_numpy(xn).float()
            return ref_cpu.model_forward(sd, ocfg, xt, torch.full((xt.size(0),), int(t), dtype=torch.long)).double().numpy()

    x = synth.gaussian("dpm.ref", (2, 2, 16, 32))
    xs, x0 = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order)
    rxs, rx0 = R.dpm_solver_steps(x.double().numpy(), seq, ref_fn, a, order)
    for i in range(len(seq)):
        mx, er = MH.gate(xs[i + 1], torch.from_numpy(rxs[i + 1]), dt, f"xs[{i + 1}] order {order}")
        MH.gate(x0[i], torch.from_numpy(rx0[i]), dt, f"x0[{i}] order {order}")
    print(f"[multistep vs reference order {order} {MODE_IDS[dt]}] final max {mx:.3e} rms err {er:.3e} x rms")


# ---- 5. convergence on the HIP path ------------------------------------------------------------------------------------------------
def test_convergence_conditions_on_the_gpu():
    """tests/test_solver_cpu.py::test_convergence_conditions with the update running in the kernel: the Gaussian model as a GPU
    callable (errors of 1e-3..1e-1 are far above fp32 rounding, so the same conditions hold)."""
    a, var = MH.alphas(), 0.25
    a64 = a.double()
    gain = ((1.0 - a64).sqrt() / (a64 * var + 1.0 - a64)).float().cuda()  # eps(x, t) = gain[t] x
    model = lambda x, t: x * gain[t].view(-1, 1, 1, 1)  # noqa: E731
    x = synth.gaussian("dpm.conv", (2, 2, 32, 256))

    def err(seq, order):
        xs, _ = D.dpm_solver_steps(x.cuda(), seq, model, a, [-1], order=order)
        want = R.gaussian_exact(a, var, x.double().numpy(), seq[-1])
        return float(np.abs(xs[-1].double().numpy() - want).max() / np.abs(want).max())

    e = {(n, p): err(logsnr_seq(a, n), p) for n in (20, 25, 50) for p in (1, 2, 3)}
    ddim_100 = err(make_seq(1000, 100), 1)
    for k, v in sorted(e.items()):
        print(f"[convergence gpu] log-SNR grid, {k[0]} requested steps, order {k[1]}: {v:.3e}")
    print(f"[convergence gpu] uniform grid, 100 steps, order 1: {ddim_100:.3e}")
    assert e[20, 2] <= e[20, 1] / 5
    assert e[20, 3] <= e[20, 2]
    assert 1.6 <= e[25, 1] / e[50, 1] <= 2.5
    assert e[25, 2] / e[50, 2] >= 3
    assert e[25, 3] / e[50, 3] >= 5
    assert e[20, 2] <= ddim_100


# ---- 6. ownership, batch independence ----------------------------------------------------------------------------------------------
def test_stepper_recaptures_when_the_model_moves_on_and_close_destroys_the_graph_first():
    """As test_gpu_configs' test of DDIMStepper: ownership, staleness and re-capture are GraphOwner's / DDIMStepper's,
    unchanged -- after ``model.float()`` (every derived buffer dropped) or a larger batch (the workspace re-allocated) the next
    step runs eagerly and captures again, on the same trajectory bit for bit."""
    cfg, m = MH.build("audio", "torch.cuda.BFloat16Tensor", 0, mode="eval")
    a = MH.alphas(cfg)
    seq = logsnr_seq(a, 10)
    coef = dpm_coefficients(seq, a, 3)
    x = synth.gaussian("dpm.own", (5, 2, 64, 256)).cuda()

    def run(disturb):
        xt = x.clone()
        with torch.no_grad():
            st = MultistepStepper(m, xt, coef, 3)
            for i in range(len(seq)):
                disturb(i, st)
                st.step()
            torch.cuda.synchronize()
            out = (xt.clone(), st.x0.clone(), st.hist.clone(), st.captures)
            st.close()
        assert st.graph is None and st._ctx is None and st._refs is None
        return out

    ref = run(lambda i, st: None)
    assert ref[3] == 1

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
        assert got[3] == 2, "the stepper must re-capture after the model re-allocated its buffers"
        assert all(torch.equal(u, v) for u, v in zip(got[:3], ref[:3]))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_sample_result_does_not_depend_on_the_batch(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = logsnr_seq(a, 6)
    x = synth.gaussian("dpm.indep", (3, 2, 16, 32))
    xs, x0 = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=3)
    solo_xs, solo_x0 = D.dpm_solver_steps(x[:1].cuda(), seq, m, a, None, order=3)
    for i in range(len(seq)):
        assert torch.equal(xs[i + 1][0], solo_xs[i + 1][0]) and torch.equal(x0[i][0], solo_x0[i][0]), i
