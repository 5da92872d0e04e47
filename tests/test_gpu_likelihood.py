"""Log-likelihood along the probability-flow ODE on the GPU (include/features/lkx_likelihood.h, ddim_audio_amd/likelihood.py).

1. ``lkx_probe_fill``; 2. ``lkx_stage`` + ``lkx_finish``; 3. ``lkx_sumsq``; 4. the launchers' refusals; 5. the native stepper (r . g,
replay = eager, sharding, probes); 6. the trajectory against the CPU oracle; 7. the convergence gate on the device; 8. the model's
state after a run.

Tolerances: bit equality against tests/likelihood_ref.py's fp32 mirror; for the double sums the bound of ANY summation order of D
terms, (D - 1) 2^-53 sum|g|, plus one rounding of the product with wd: D 2^-53 sum|g| in all (Higham 2002, eq. 4.4)."""
import math

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, schedule, synth
from ddim_audio_amd.noise import NoiseStream
import gpu_util as G
import kernel_harness as KH
import likelihood_ref as R
import model_harness as MH
from model_harness import MODES, MODE_IDS

pytestmark = pytest.mark.gpu
P, chk = _lib.ptr, _lib.check
F = np.float32
SEED = 0x11CE11
U53 = 2.0 ** -53
# per_sample: one group | a ragged single block | three blocks, the last ragged | the block cap (256 blocks, grid-stride past it)
PERS = [4, 4 * 257, 4 * (2 * 1024 + 300), 4 * (256 * 1024 + 500)]
PER_IDS = ["one_group", "ragged", "three_blocks", "block_cap"]


def _operand(tag, b, per):
    return synth.gaussian(f"likelihood.{tag}.{b}.{per}", (b, per)).numpy()


def _blocks(per):
    return int(KH.lib().lkx_partials_doubles(1, per))


def _step(i):
    return torch.tensor([i], dtype=torch.int32, device=G.dev())


# ---- 1. the probe -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("per", PERS[:3], ids=PER_IDS[:3])
def test_probe_fill(b, per):
    """fp32 +-1 bit for bit against the CPU Philox (bit 31 of the word clear: +1), with a non-zero first sample and probe index."""
    assert [_blocks(p) for p in PERS] == [1, 1, 3, 256]
    for first, k in ((0, 0), (41, 2)):
        out = KH.Out(b * per)
        chk(KH.lib().lkx_probe_fill(out.ptr, b, per, SEED, first, k, _lib.stream()))
        want = R.probe(SEED, first, (b, per), k).astype(F)
        KH.same(out.read("r").view(b, per), want, f"lkx_probe_fill first={first} probe={k}")
        assert set(np.unique(want)) <= {-1.0, 1.0} and (b * per < 64 or abs(want.mean()) < 0.2)


# ---- 2. the update and the sums -----------------------------------------------------------------------------------------------------------
def _row(wk, we, an, wd, flags):
    return np.array([[7.0, wk, we, an, wd, float(flags), 0.0, 0.0]], dtype=np.float64)


def _stage(uh, kh, eh, gh, row, wd, first=0, k=0, acc0=None, replays=1):
    """One row through lkx_stage + lkx_finish on guarded buffers; k1 is all-sentinel (NaN) unless ``kh`` is given.  Returns the
    buffers and the host results."""
    b, per = uh.shape
    lib, nb = KH.lib(), _blocks(uh.shape[1])
    u, k1 = KH.Out(b * per, init=uh), (KH.Out(b * per) if kh is None else KH.Out(b * per, init=kh))
    e, g = KH.Ro(eh), KH.Ro(gh)
    xin, partial = KH.Out(b * per), KH.Out(b * nb, torch.float64)
    acc = KH.Out(b, torch.float64, init=np.zeros(b) if acc0 is None else acc0)
    coef, wdt = KH.Ro(row.astype(F)), KH.Ro(np.asarray([wd], dtype=np.float64), torch.float64)
    step = _step(0)
    assert int(lib.lkx_partials_doubles(b, per)) == b * nb
    for _ in range(replays):
        chk(lib.lkx_stage(u.ptr, k1.ptr, e.ptr, g.ptr, xin.ptr, partial.ptr, coef.ptr, P(step), b, per, SEED, first, k, _lib.stream()))
        chk(lib.lkx_finish(partial.ptr, acc.ptr, wdt.ptr, P(step), b, nb, _lib.stream()))
    KH.sync()
    for ro, name in ((e, "e"), (g, "g"), (coef, "coef"), (wdt, "wd")):
        ro.check(name)
    return u, k1, xin, partial, acc


@pytest.mark.parametrize("flags", [0, 1, 2, 3], ids=["none", "save", "commit", "save_commit"])
@pytest.mark.parametrize("wk", [0.0, 0.375], ids=["wk0", "wk"])
@pytest.mark.parametrize("per", PERS, ids=PER_IDS)
def test_stage(per, wk, flags):
    """u, k1, xin bit for bit against the fp32 mirror for every flag combination; a k1 that is not read is NaN throughout (it would
    poison xin) and one that is not written still holds its sentinel; a u that is not committed keeps its bits; acc within
    D 2^-53 sum|g| |wd| of the float64 sum."""
    b = 1 if per == PERS[-1] else 3
    uh, eh, gh = _operand("s.u", b, per), _operand("s.e", b, per), _operand("s.g", b, per)
    kh = _operand("s.k", b, per) if wk != 0 else None
    row, wd = _row(wk, 1.625, 0.8125, 0.3, flags), 0.3 + 2.0 ** -40  # a wd that fp32 cannot hold: the double table is what is read
    u, k1, xin, partial, acc = _stage(uh, kh, eh, gh, row, wd, first=9, k=1)
    r = R.probe(SEED, 9, (b, per), 1).astype(F)
    un, kn, xn, d = R.stage32(uh, kh if kh is not None else np.zeros_like(uh), eh, gh, r, row[0].astype(F))
    KH.same(xin.read("xin").view(b, per), xn, "xin")
    KH.same(u.read("u").view(b, per), un if flags & 2 else uh, "u")
    assert np.isfinite(xn).all()
    if flags & 1:
        KH.same(k1.read("k1").view(b, per), eh, "k1 <- e")
    elif kh is None:
        assert k1.untouched(), "k1 was written by a row that neither saves nor reads it"
    else:
        KH.same(k1.read("k1").view(b, per), kh, "k1 kept")
    got = acc.read("acc").numpy()
    bound = per * U53 * np.abs(gh.astype(np.float64)).sum(axis=1) * abs(wd)
    assert np.all(np.abs(got - wd * d) <= bound), (got, wd * d, bound)
    assert bool(torch.isfinite(partial.read("partial")).all())


@pytest.mark.parametrize("per", PERS[:3], ids=PER_IDS[:3])
def test_stage_is_batch_invariant_and_replays_to_the_same_bits(per):
    """Sample 1 of a batch of 3 (global sample 6) and the same sample alone: u, xin and acc bit for bit; two replays of the same
    launches from the same state twice: the same acc bits (the accumulator takes the row twice)."""
    uh, eh, gh, kh = (_operand(f"i.{n}", 3, per) for n in "uegk")
    row, wd, acc0 = _row(0.25, 1.5, 0.75, 0.0, 3), -1.7, np.array([0.5, -2.0, 3.0])
    full = _stage(uh, kh, eh, gh, row, wd, first=5, acc0=acc0)
    one = _stage(uh[1:2], kh[1:2], eh[1:2], gh[1:2], row, wd, first=6, acc0=acc0[1:2])
    for f, o, name in zip(full, one, ("u", "k1", "xin", "partial", "acc")):
        fv = f.read(name)
        KH.same(fv.view(3, -1)[1], o.read(name).view(-1), f"{name}: sample 1 of 3 against the sample alone")
    twice_a = _stage(uh, kh, eh, gh, _row(0.25, 1.5, 0.75, 0.0, 0), wd, first=5, acc0=acc0, replays=2)[4].read("acc")
    twice_b = _stage(uh, kh, eh, gh, _row(0.25, 1.5, 0.75, 0.0, 0), wd, first=5, acc0=acc0, replays=2)[4].read("acc")
    KH.same(twice_a, twice_b, "acc after two replays")
    assert not torch.equal(twice_a, full[4].read("acc"))


# ---- 3. the sum of squares ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", PERS, ids=PER_IDS)
def test_sumsq(per):
    """sum x^2 per sample within D 2^-53 sum x^2 of the float64 sum; a sample alone gives its bits inside a batch; twice the same."""
    b = 1 if per == PERS[-1] else 3
    xh = _operand("q.x", b, per)

    def run(x):
        n = x.shape[0]
        xin, partial, out = KH.Ro(x), KH.Out(n * _blocks(per), torch.float64), KH.Out(n, torch.float64)
        chk(KH.lib().lkx_sumsq(xin.ptr, partial.ptr, out.ptr, n, per, _lib.stream()))
        KH.sync()
        xin.check("x")
        partial.read("partial")
        return out.read("out")

    got = run(xh)
    want = R.exact_sum(xh.astype(np.float64) ** 2)
    assert np.all(np.abs(got.numpy() - want) <= per * U53 * want)
    KH.same(run(xh), got, "lkx_sumsq twice")
    if b > 1:
        KH.same(run(xh[2:3]), got[2:3], "lkx_sumsq: a sample alone")


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------
def test_launcher_refusals():
    """Every launcher validates before launching: nothing is written, the message names the export and the argument."""
    lib, st = KH.lib(), _lib.stream()
    f, d, step = KH.Out(64), KH.Out(64, torch.float64), _step(0)
    big, last = 4 * ((1 << 32) + 1), (1 << 32) - 1

    def stage(b=1, per=4, first=0, **null):
        a = dict(u=f.ptr, k1=f.ptr, e=f.ptr, g=f.ptr, xin=f.ptr, partial=d.ptr, coef=f.ptr, step=P(step))
        a.update(null)
        return lib.lkx_stage(a["u"], a["k1"], a["e"], a["g"], a["xin"], a["partial"], a["coef"], a["step"], b, per, SEED, first, 0, st)

    def msg(rc, text):
        KH.refused(rc, f, d, who=text.split(":")[0])
        assert text in lib.ddimx_last_error().decode(), lib.ddimx_last_error().decode()

    for name in ("u", "k1", "e", "g", "xin", "partial", "coef", "step"):
        msg(stage(**{name: None}), "lkx_stage: null argument")
    msg(stage(b=0), "lkx_stage: B = 0 (1..65535)")
    msg(stage(b=65536), "lkx_stage: B = 65536 (1..65535)")
    msg(stage(per=0), "lkx_stage: per_sample = 0 must be a positive multiple of 4")
    msg(stage(per=6), "lkx_stage: per_sample = 6 must be a positive multiple of 4")
    msg(stage(per=big), f"lkx_stage: per_sample = {big} has more than 2^32 groups of four")
    msg(stage(b=2, first=last), f"lkx_stage: first_sample + B = {last + 2} exceeds 2^32")

    fill = lambda r=f.ptr, b=1, per=4, first=0: lib.lkx_probe_fill(r, b, per, SEED, first, 0, st)
    msg(fill(r=None), "lkx_probe_fill: null argument")
    msg(fill(b=0), "lkx_probe_fill: B = 0 (1..65535)")
    msg(fill(b=65536), "lkx_probe_fill: B = 65536 (1..65535)")
    msg(fill(per=-4), "lkx_probe_fill: per_sample = -4 must be a positive multiple of 4")
    msg(fill(per=10), "lkx_probe_fill: per_sample = 10 must be a positive multiple of 4")
    msg(fill(per=big), f"lkx_probe_fill: per_sample = {big} has more than 2^32 groups of four")
    msg(fill(b=3, first=last), f"lkx_probe_fill: first_sample + B = {last + 3} exceeds 2^32")

    fin = lambda partial=d.ptr, acc=d.ptr, wd=d.ptr, s=P(step), b=1, nb=1: lib.lkx_finish(partial, acc, wd, s, b, nb, st)
    for name in ("partial", "acc", "wd", "s"):
        msg(fin(**{name: None}), "lkx_finish: null argument")
    msg(fin(b=0), "lkx_finish: B = 0 (1..65535)")
    msg(fin(b=65536), "lkx_finish: B = 65536 (1..65535)")
    msg(fin(nb=0), "lkx_finish: blocks_per_sample = 0 must be positive")

    sq = lambda x=f.ptr, partial=d.ptr, out=d.ptr, b=1, per=4: lib.lkx_sumsq(x, partial, out, b, per, st)
    for name in ("x", "partial", "out"):
        msg(sq(**{name: None}), "lkx_sumsq: null argument")
    msg(sq(b=0), "lkx_sumsq: B = 0 (1..65535)")
    msg(sq(b=65536), "lkx_sumsq: B = 65536 (1..65535)")
    msg(sq(per=0), "lkx_sumsq: per_sample = 0 must be a positive multiple of 4")
    msg(sq(per=5), "lkx_sumsq: per_sample = 5 must be a positive multiple of 4")
    assert lib.lkx_partials_doubles(0, 4) == 0 and lib.lkx_partials_doubles(1, 5) == 0 and lib.lkx_partials_doubles(65536, 4) == 0


# ---- 5. the native stepper ----------------------------------------------------------------------------------------------------------------
SEQ = [0, 250, 600, 999]  # Heun: 6 rows, so the step is captured (4 or more) and replayed


def _native(mode, kind):
    cfg, mv, ms, a = MH.pair("tiny", mode[0])
    m = mv if kind == "v" else ms
    return m, a, (m.config.channels, 16, m.config.f_size)


def _data(b, shape, tag="x"):
    return (0.5 * synth.gaussian(f"likelihood.data.{tag}", (b,) + shape)).to(G.dev())


@pytest.mark.parametrize("kind", ["eps", "v"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_native_run(mode, kind):
    """On the smallest native model: the stepper's r . g of the first evaluation is the float64 dot of r with autograd's
    J^T r (the same kernels: only the summation bound separates them); replayed = eager bit for bit, from one capture; 8 samples
    = 4 + 4 = 3 + 3 + 2 bit for bit in logp and latent; with three probes the three latents of a sample are equal and the
    standard error is finite; nothing of the model moved (test 8 looks at the rest)."""
    m, a, shape = _native(mode, kind)
    x = _data(8, shape)
    per = x[0].numel()
    st = {}
    full = D.log_likelihood(x, SEQ, m, a, noise=NoiseStream(SEED), stats=st)
    assert st["evaluations"] == 6 and st["captures"] == 1 and st["divergence"].shape == (6, 8)
    assert full.logp.dtype == torch.float64 and full.logp.shape == (8,) and bool(torch.isfinite(full.logp).all())
    assert torch.equal(full.bpd, -full.logp / (per * math.log(2.0))) and bool(torch.isnan(full.stderr).all())
    assert full.latent.shape == x.shape and full.latent.dtype == torch.float32 and full.latent.is_cuda
    # r . g against autograd through the same model
    r = torch.from_numpy(R.probe(SEED, 0, (8, per), 0).astype(F)).view_as(x).to(G.dev())
    xg = x.clone().requires_grad_(True)
    with torch.enable_grad():
        out = m(xg, torch.zeros(8, dtype=torch.int64, device=G.dev()))
        g, = torch.autograd.grad(out, xg, r)
    g64 = g.double().view(8, per).cpu().numpy()
    want = R.exact_sum(r.double().view(8, per).cpu().numpy() * g64)
    bound = per * U53 * np.abs(g64).sum(axis=1)
    assert np.all(np.abs(st["divergence"][0] - want) <= bound), (st["divergence"][0], want, bound)
    assert all(p.grad is None for p in m.parameters())
    # eager
    se = {}
    with MH.eager_steps():
        eager = D.log_likelihood(x, SEQ, m, a, noise=NoiseStream(SEED), stats=se)
    assert se["captures"] == 0
    assert torch.equal(eager.logp, full.logp) and torch.equal(eager.latent, full.latent)
    assert np.array_equal(se["divergence"], st["divergence"])
    # shards
    for cuts in ((0, 4, 8), (0, 3, 6, 8)):
        parts = [D.log_likelihood(x[lo:hi], SEQ, m, a, noise=NoiseStream(SEED).shard(lo)) for lo, hi in zip(cuts, cuts[1:])]
        assert torch.equal(torch.cat([p.logp for p in parts]), full.logp), cuts
        assert torch.equal(torch.cat([p.latent for p in parts]), full.latent), cuts
    # probes
    sp = {}
    three = D.log_likelihood(x[:2], SEQ, m, a, probes=3, noise=NoiseStream(SEED), stats=sp)
    assert sp["latents"].shape == (3, 2) + shape and sp["divergence"].shape == (6, 6)
    for k in range(3):
        assert torch.equal(sp["latents"][k], full.latent[:2]), k
    assert np.array_equal(sp["divergence"][:, :2], st["divergence"][:, :2])  # probe 0 is the single-probe run
    assert not np.array_equal(sp["divergence"][:, 2:4], sp["divergence"][:, :2])
    assert bool(torch.isfinite(three.stderr).all()) and bool((three.stderr > 0).all())
    assert torch.equal(three.latent, full.latent[:2])


# ---- 6. the trajectory --------------------------------------------------------------------------------------------------------------------
def test_trajectory_against_the_cpu_oracle():
    """The fp32 eps model's run against the float64 integrator driving the CPU oracle (eps and J^T r by autograd through it).
    First gate: the forward's parity allowance of 1.2e-5 sigma per evaluation, times the evaluations, on the latent; the same
    relative allowance on every divergence (against sum|g|, plus the summation bound) and, through the weights, on logp.  If the
    latent misses that, the gap between ``generalized_steps`` on the device and on the oracle (same model, same ``seq``) is measured
    here and every allowance becomes twice that gap -- the printed line says which gate held."""
    m, a, shape = _native(MODES[0], "eps")
    b, per = 2, int(np.prod(shape))
    x = _data(b, shape, "traj")
    fn = MH.oracle_eps(m)
    r = R.probe(SEED, 0, (b, per), 0)
    tab = schedule.likelihood_coefficients(SEQ, a, 2, "eps")

    def eps_g(xin, t):
        xt = torch.from_numpy(xin.reshape((b,) + shape)).float().requires_grad_(True)
        out = fn(xt, torch.full((b,), int(t), dtype=torch.long))
        g, = torch.autograd.grad(out, xt, torch.from_numpy(r.reshape((b,) + shape)).float())
        return out.detach().double().numpy().reshape(b, per), g.double().numpy().reshape(b, per)

    al0 = R.levels(SEQ, a)[0][0]
    xh = x.cpu().double().numpy().reshape(b, per)
    u, k1, xin, acc, divs, gabs = xh / al0, None, xh.copy(), np.zeros(b), [], []
    for row, wd in zip(tab.rows, tab.wd):
        e, g = eps_g(xin, row[0])
        d = (r * g).sum(axis=1)
        un = u + row[2] * e + (row[1] * k1 if row[1] != 0 else 0.0)
        xin = row[3] * un
        k1 = e if int(row[5]) & R.SAVE else k1
        u = un if int(row[5]) & R.COMMIT else u
        acc += wd * d
        divs.append(d)
        gabs.append(np.abs(g).sum(axis=1))
    want = R.log_normal(xin) + per * tab.logdet_per_dim + acc
    st = {}
    got = D.log_likelihood(x, SEQ, m, a, noise=NoiseStream(SEED), stats=st)
    n_eval = len(tab.rows)
    lat = got.latent.double().view(b, per).cpu().numpy()
    err_lat = np.abs(lat - xin).max() / xin.std()
    rel, gate = 1.2e-5 * n_eval, "the forward's parity gate times the evaluations"
    if err_lat > rel:
        noise = synth.gaussian("likelihood.traj.xT", (b,) + shape)
        dev_xs, _ = D.generalized_steps(noise.to(G.dev()), SEQ, m, a, None)
        ref_xs, _ = _oracle_ddim(noise, SEQ, fn, a)
        gap = float((dev_xs[-1].double() - ref_xs[-1].double()).abs().max() / ref_xs[-1].double().std())
        rel, gate = 2.0 * gap, f"twice the generalized_steps gap of {gap:.3e}"
    err_div = max(float((np.abs(st["divergence"][i] - divs[i]) / gabs[i]).max()) for i in range(n_eval))
    tol_div = [rel * gabs[i] + per * U53 * gabs[i] for i in range(n_eval)]
    tol_logp = sum(abs(wd) * t for wd, t in zip(tab.wd, tol_div)) + np.abs(xin).sum(axis=1) * rel * xin.std()
    err_logp = np.abs(got.logp.numpy() - want)
    print(f"[likelihood trajectory] latent {err_lat:.3e} sigma, divergence {err_div:.3e} of sum|g|, logp {err_logp.max():.3e} nats "
          f"(allowed {tol_logp.min():.3e}); gate: {gate} = {rel:.3e}")
    assert err_lat <= rel
    for i in range(n_eval):
        assert np.all(np.abs(st["divergence"][i] - divs[i]) <= tol_div[i]), i
    assert np.all(err_logp <= tol_logp)


def _oracle_ddim(x, seq, fn, a):
    """eta = 0 DDIM on the CPU oracle in float64 state: (xs, None), xs[-1] the final sample."""
    ab = np.asarray(a, dtype=np.float32).astype(np.float64)
    xt = x.double()
    for i in reversed(range(len(seq))):
        at, an = ab[seq[i]], (ab[seq[i - 1]] if i else 1.0)
        with torch.no_grad():
            e = fn(xt.float(), torch.full((x.size(0),), seq[i], dtype=torch.long)).double()
        x0 = (xt - math.sqrt(1 - at) * e) / math.sqrt(at)
        xt = math.sqrt(an) * x0 + math.sqrt(1 - an) * e
    return [xt], None


# ---- 7. convergence on the device ---------------------------------------------------------------------------------------------------------
def test_convergence_on_the_device():
    """CPU test 1 through the callable path in fp32: the closed-form Gaussian predictor as torch operations on the device, g by
    autograd, the steps through lkx_stage / lkx_finish.  The same ratios, and Heun at n = 100 within 1e-3 bits/dim of float64."""
    a = R.linear_alphas()
    ab = torch.from_numpy(a.astype(np.float64)).to(G.dev())
    c = ((1.0 - ab).sqrt() / (ab * 0.25 + 1.0 - ab)).float()
    model = lambda x, t: c[t].view(-1, 1, 1, 1) * x
    dim = 64
    xh = np.random.default_rng(0).standard_normal((1, dim)) * math.sqrt(float(a[0]) * 0.25 + 1.0 - float(a[0]))
    x = torch.from_numpy(xh.astype(F)).view(1, 1, 4, 16).to(G.dev())
    exact = R.iso_logp(x.double().cpu().numpy().reshape(1, dim), a, 0)
    err, ref = {}, {}
    for order in (1, 2):
        for n in (100, 200):
            st = {}
            got = D.log_likelihood(x, R.grid(n), model, a, order=order, stats=st)
            assert st["evaluations"] == order * n and st["captures"] == 0
            err[order, n] = float(got.logp[0] - exact[0]) / (dim * math.log(2.0))
            ref[order, n] = float((R.integrate(x.double().cpu().numpy().reshape(1, dim), R.grid(n), a, order, R.iso_eps_div(a))[0] - exact)[0]) / (dim * math.log(2.0))
            print(f"[likelihood device order {order}] n = {n}: {err[order, n]:.5g} bits/dim (float64 {ref[order, n]:.5g})")
    assert 3.5 <= err[2, 100] / err[2, 200] <= 4.5
    assert 1.8 <= err[1, 100] / err[1, 200] <= 2.2
    assert abs(err[2, 100]) < 0.01 and abs(err[2, 100] - ref[2, 100]) <= 1e-3


# ---- 8. the model afterwards --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["eps", "v"])
def test_model_state_after_a_run(kind):
    m, a, shape = _native(MODES[0], kind)
    noise = synth.gaussian("likelihood.state.xT", (2,) + shape)
    before, _ = D.generalized_steps(noise.to(G.dev()), SEQ, m, a, None)
    m._dropout_calls = 17
    # (the model is shared with the tests above, whose autograd call may have left a flat gradient buffer: it must not move or change)
    flat = getattr(m, "_flat_grad", None)
    flat_bits = None if flat is None else flat.clone()
    D.log_likelihood(_data(2, shape, "state"), SEQ, m, a, probes=2)
    assert m._dropout_calls == 17
    assert all(p.grad is None for p in m.parameters()) and getattr(m, "_flat_grad", None) is flat
    assert flat is None or torch.equal(flat.view(torch.int32), flat_bits.view(torch.int32))
    assert not m.training
    after, _ = D.generalized_steps(noise.to(G.dev()), SEQ, m, a, None)
    MH.same_list(after[1:], before[1:], "generalized_steps after log_likelihood")
    with pytest.raises(ValueError, match="eval mode"):
        D.log_likelihood(_data(2, shape, "state"), SEQ, m.train(), a)
    m.eval()
