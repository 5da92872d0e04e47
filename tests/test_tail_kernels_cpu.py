"""The references, case tables and gates of tests/tail_kernel_ref.py, checked without a GPU: each reference against torch or the
oracle, the table builder and the per-step scalars against the package's own, and that every gate the GPU tests apply is one an fp32
mirror of the kernel meets with a factor of two to spare (a gate the mirror cannot meet is a wrong gate)."""
import math

import numpy as np
import pytest
import torch

import tail_kernel_ref as R
from oracle import ref_cpu

F = np.float32


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F))


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


# ---- 1. references against torch and the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ti", [0, 412, 999])
def test_qsample_mirror_equals_torch(ti):
    """The reference expression x0 * a.sqrt() + e * (1.0 - a).sqrt() (functions/losses.py:12-13), evaluated by torch in fp32."""
    al = R.alphas()
    assert 0.0 < float(al[999]) < float(al[0]) < 1.0
    x0, e = R.gauss("cpu.qs.x0", (3, 257)), R.gauss("cpu.qs.e", (3, 257))
    t = torch.tensor([ti, 999 - ti, ti])
    a = t32(al).index_select(0, t).view(-1, 1)
    want = t32(x0) * a.sqrt() + t32(e) * (1.0 - a).sqrt()
    assert torch.equal(t32(R.qsample(x0, e, al, t.tolist())), want)


@pytest.mark.parametrize("B", R.SQ_B)
def test_sqerr_equals_oracle_loss(B):
    """noise_estimation_loss with an identity model: out = x_t, so the loss is sum (e - x_t)^2 per sample and its batch mean."""
    al = R.alphas().astype(np.float64)
    x0, e = R.gauss(f"cpu.sq.x0.{B}", (B, 2, 5, 13)).astype(np.float64), R.gauss(f"cpu.sq.e.{B}", (B, 2, 5, 13)).astype(np.float64)
    t = torch.arange(B) * 142 + 3
    a = al[t.numpy()]
    xt = x0 * np.sqrt(a)[:, None, None, None] + e * np.sqrt(1.0 - a)[:, None, None, None]
    got = R.sqerr(e.reshape(B, -1), xt.reshape(B, -1))
    per = ref_cpu.noise_estimation_loss(lambda x, t_: x, t64(x0), t, t64(e), t64(al), keepdim=True)
    mean = ref_cpu.noise_estimation_loss(lambda x, t_: x, t64(x0), t, t64(e), t64(al))
    assert np.allclose(got[:B], per.numpy(), rtol=1e-12, atol=0) and abs(got[B] - float(mean)) <= 1e-12 * float(mean)


def test_sqerr_bwd_equals_autograd():
    B, per = 3, 65
    e, out = R.loss_inputs(B, per)
    g = R.loss_grads(B)
    o = t64(out).requires_grad_(True)
    ps = (t64(e) - o).square().sum(1)
    torch.cat([ps, ps.mean().view(1)]).backward(t64(g))
    assert np.allclose(R.sqerr_bwd(e, out, g, 1), o.grad.numpy(), rtol=1e-13, atol=1e-15)
    o.grad = None
    (t64(e) - o).square().sum(1).backward(t64(g[:B]))
    assert np.allclose(R.sqerr_bwd(e, out, g, 0), o.grad.numpy(), rtol=1e-13, atol=1e-15)


def _ema_pair(n=100000):
    p = R.gauss("cpu.ema.p", n)
    return (F(0.99) * p - F(0.003)).astype(F), p


@pytest.mark.parametrize("mu", R.MUS)
def test_ema_equals_oracle(mu):
    sh, p = _ema_pair()
    want = ref_cpu.ema_update({"w": t32(sh)}, {"w": t32(p)}, mu)["w"]
    assert torch.equal(t32(R.ema(sh, p, mu)), want)


def test_ema_coefficient_of_the_rounded_mu_differs():
    """The finding behind ddimx_ema_update_multi_coef: a C float mu can only give fp32(1 - fp32(mu)) = 1.00016594e-4 for mu = 0.9999,
    not the reference's fp32(1.0 - mu) = 1e-4, and then 20 528 of these 100 000 shadows miss the reference's bits (16 005 at 0.999)."""
    sh, p = _ema_pair()
    for mu, n_diff in ((0.9999, 20528), (0.999, 16005)):
        want = ref_cpu.ema_update({"w": t32(sh)}, {"w": t32(p)}, mu)["w"].numpy()
        old = R.ema(sh, p, mu, c_param=R.ema_old_coef(mu))
        diff = int((old.view(np.int32) != want.view(np.int32)).sum())
        print(f"[ema mu={mu}] coefficient {float(R.ema_old_coef(mu)):.9e} instead of {float(F(1.0 - mu)):.9e}: {diff} of {p.size} differ")
        assert diff > 0
    assert float(R.ema_old_coef(0.9999)) == float(F(1.00016594e-4)) and R.ema_old_coef(0.5) == F(0.5)


@pytest.mark.parametrize("hp", range(len(R.HYPER)))
@pytest.mark.parametrize("decoupled", [0, 1, 2])
@pytest.mark.parametrize("wd", R.WDS)
def test_adam_equals_torch(decoupled, wd, hp):
    """Six steps from the zero state in float64 with the float-valued hyperparameters: torch.optim.Adam / AdamW, and the oracle's
    restatement of AdaBelief."""
    h = R.HYPER[hp]
    lr, b1, b2, eps, wdf = (R.f32v(x) for x in (h["lr"], h["betas"][0], h["betas"][1], h["eps"], wd))
    n = 257
    p0 = R.gauss("cpu.adam.p", n).astype(np.float64)
    tp = t64(p0).clone().requires_grad_(True)
    tm, tv = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    opt = None if decoupled == 2 else (torch.optim.AdamW if decoupled else torch.optim.Adam)([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wdf)
    p, m, v = p0, np.zeros(n), np.zeros(n)
    for step in range(1, 7):
        g = R.gauss(f"cpu.adam.g.{step}", n).astype(np.float64)
        w = R.adam(p, g, m, v, step, h, wd, decoupled)
        p, m, v = w["p"], w["m"], w["v"]
        if decoupled == 2:
            with torch.no_grad():
                ref_cpu.adabelief_step(tp, t64(g), tm, tv, step, lr, (b1, b2), eps, wdf)
        else:
            tp.grad = t64(g).clone()
            opt.step()
            tm, tv = opt.state[tp]["exp_avg"], opt.state[tp]["exp_avg_sq"]
        assert np.allclose(p, tp.detach().numpy(), rtol=1e-12, atol=1e-15), step
        assert np.allclose(m, tm.numpy(), rtol=1e-12, atol=1e-18) and np.allclose(v, tv.numpy(), rtol=1e-12, atol=1e-24), step


def test_adam_clip_is_a_factor_on_the_gradient():
    p, g, m, v = R.adam_state("cpu.clip", 100, 2, 1.0)
    a = R.adam(p, g, m, v, 2, R.HYPER[0], 1e-2, 0, clip=0.37)
    b = R.adam(p, g.astype(np.float64) * R.f32v(0.37), m, v, 2, R.HYPER[0], 1e-2, 0)
    assert all(np.array_equal(a[k], b[k]) for k in "pmv")


def test_tables_and_scalars_equal_the_package():
    from ddim_audio_amd import ema as E, optim as O
    assert R.BLOCK == O._lib.load().ddimx_ema_block_elems()
    ts = [torch.zeros(n) for n in R.SIZES]
    bt, bo = R.tables(R.SIZES)
    tb = O._Tables([ts, ts], torch.device("cpu"))
    assert tb.bt.tolist() == bt and tb.bo.tolist() == bo and tb.sizes.tolist() == list(R.SIZES) and tb.nblk == len(bt)
    et = E.EMAHelper()._build_tables([(t, t) for t in ts], torch.device("cpu"))
    assert et["bt"].tolist() == bt and et["bo"].tolist() == bo and et["n"].tolist() == list(R.SIZES) and et["nblk"] == len(bt)
    assert len(bt) == sum(-(-n // R.BLOCK) for n in R.SIZES) and all(o % R.BLOCK == 0 for o in bo)
    for hp in R.HYPER:
        for step in R.STEPS + (3, 7, 100000):
            got = tuple(float(x) for x in R.dyn_scalars(hp, step))
            assert got == O.adam_step_scalars(dict(hp), step), (hp, step)


# ---- 2. the cases reach what they are meant to reach, on admissible operands -------------------------------------------------------------------
def test_cases_are_admissible():
    assert all(0 <= t < R.N_STEPS for ts in R.QS_T.values() for tl in ts for t in tl)
    assert set(len(tl) for tl in R.QS_T[3]) == {3} and any(len(set(tl)) < 3 for tl in R.QS_T[3])
    assert -(-R.QS_PER[-1] // 256) > 1024  # the block cap bites: a second grid-stride trip
    assert [R.sqerr_trips(n) for n in R.SQ_PER] == [1, 1, 1, 1, 1, 1, 2, 4]
    # parts entirely past the end (per < 64, and ceil-chunks that run out early), and a clamped last part
    assert any(n < R.SQ_PARTS for n in R.SQ_PER) and any(-(-n // 64) * 63 < n < -(-n // 64) * 64 for n in R.SQ_PER)
    e, out = R.loss_inputs(7, R.SQ_PER[-1], integer=True)
    d = e - out
    assert np.all(d == np.round(d)) and np.all(np.abs(d) >= 1) and np.all(np.abs(d) <= 4) and float((d * d).sum()) < 2.0 ** 24
    assert {1, R.BLOCK - 1, R.BLOCK, R.BLOCK + 1} <= set(R.SIZES) and list(R.SIZES) != sorted(R.SIZES)
    for cfg in R.adam_configs():
        hp = R.HYPER[cfg[2]]
        omb2 = 1.0 - R.f32v(hp["betas"][1])
        assert all(R.f32v(b) >= 0.5 for b in hp["betas"])  # 1.0f - beta is exact
        for step, gs, tensors in R.adam_cases(cfg):
            for p, g, m, v in tensors:
                w = R.adam(p, g, m, v, step, hp, cfg[1], cfg[0])
                # the operand of the second moment's fma.  (AdaBelief squares r = g' - m_new instead, which cancellation can make
                # arbitrarily small; its v carries eps >= 1e-8, so an r^2 lost to the subnormals is 2^-126 against a gate of 8 u eps.)
                q = w["gabs"] ** 2 * omb2
                assert np.all((q == 0) | (q > 2.0 ** -100)), (cfg, step, gs)
                assert np.all(v >= 0) and ((step == 1) == (not m.any() and not v.any()))
                assert (step == 1) == bool((g == 0).any())
                for a in (p, g, m, v, w["p"].astype(F), w["m"].astype(F), w["v"].astype(F)):
                    assert np.all((a == 0) | (np.abs(a) >= 2.0 ** -126))


# ---- 3. every gate against an fp32 mirror: at most half ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", R.SQ_B)
def test_sqerr_mirror_within_half_gate(B):
    worst = 0.0
    for per in R.SQ_PER:
        e, out = R.loss_inputs(B, per, integer=True)
        want = R.sqerr(e, out)
        got = R.sqerr_mirror(e, out)
        assert np.array_equal(got[:B].astype(np.float64), want[:B])
        if B & (B - 1) == 0:
            assert float(got[B]) == want[B]
        e, out = R.loss_inputs(B, per)
        want = R.sqerr(e, out)
        worst = max(worst, R.worst(R.sqerr_mirror(e, out) - want, R.sqerr_gate(want, per)))
    print(f"[sqerr mirror B={B}] worst {worst:.2e} of the gate")
    assert worst <= 0.5


def test_sqerr_bwd_mirror_within_half_gate():
    worst = 0.0
    for B in R.BWD_B:
        for per in R.SQ_PER[:5]:
            e, out = R.loss_inputs(B, per)
            for wm in (0, 1):
                want = R.sqerr_bwd(e, out, R.loss_grads(B), wm)
                worst = max(worst, R.worst(R.sqerr_bwd_mirror(e, out, R.loss_grads(B), wm) - want, R.sqerr_bwd_gate(want)))
    print(f"[sqerr_bwd mirror] worst {worst:.2e} of the gate")
    assert worst <= 0.5


def test_grad_norm_mirror_within_half_gate():
    assert R.NORM_K == 13
    worst = 0.0
    seen = {}
    for name, gs in R.norm_cases():
        want, coef = R.grad_norm(gs, R.MAX_NORM)
        got = R.grad_norm_mirror(gs)
        worst = max(worst, abs(float(got) - want) / R.grad_norm_gate(want))
        assert abs(float(R.clip_coef32(got, R.MAX_NORM)) - coef) <= 16 * R.U * coef
        seen[name] = (want, coef, got)
    assert seen["below"][1] == 1.0 and seen["below"][0] < 0.1 and 1.01 < seen["about"][0] < 1.03 and seen["above"][1] < 1e-3
    # the 1e-6 shows in the bits of the middle case's coefficient
    assert R.clip_coef32(seen["about"][2], R.MAX_NORM) != F(R.MAX_NORM) / seen["about"][2]
    print(f"[grad_norm mirror] worst {worst:.2e} of the gate")
    assert worst <= 0.5


def test_adam_mirror_within_half_gate():
    """Also the measurement behind ADAM_P_C: the mirror's worst p error in the gate's unit (c = 1)."""
    wp = wm = wv = 0.0
    for cfg in R.adam_configs():
        hp = R.HYPER[cfg[2]]
        for step, gs, tensors in R.adam_cases(cfg):
            for p, g, m, v in tensors:
                w = R.adam(p, g, m, v, step, hp, cfg[1], cfg[0])
                gp, gm, gv = R.adam_gates(w)
                mp, mm, mv = R.adam_mirror(p, g, m, v, step, hp, cfg[1], cfg[0])
                wp, wm, wv = max(wp, R.worst(mp - w["p"], gp)), max(wm, R.worst(mm - w["m"], gm)), max(wv, R.worst(mv - w["v"], gv))
                if step == 1 and cfg[0] != 2 and cfg[1] == 0:
                    z = g == 0
                    assert z.any() and np.array_equal(mp[z], p[z]) and np.array_equal(w["p"][z], p[z].astype(np.float64))
    print(f"[adam mirror] worst p {wp:.3f} m {wm:.3f} v {wv:.3f} of the gates; p in the unit of c: {wp * R.ADAM_P_C:.3f}")
    assert wp <= 0.5 and wm <= 0.5 and wv <= 0.5
    assert R.ADAM_P_C == math.ceil(2.0 * wp * R.ADAM_P_C), "ADAM_P_C is twice the mirror's worst value, rounded up"
