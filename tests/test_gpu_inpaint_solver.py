"""Multistep inpainting on the GPU (ddim_audio_amd.inpaint_solver_steps, ddimxi_residual / ddimxi_multistep_update).

The kernel alone through guarded buffers: its bits against the fp32 restatement of the documented operation order
(tests/inpaint_solver_ref.py: update32) for the four flag combinations, every zero / non-zero (w1, w2, c1), h2 null and given,
the noise handed over and drawn in the kernel, masks of 0, 1 and fractions and a sample with L = 0 -- every buffer that the row
and the flags leave unread poisoned, so that a read of it shows --; the final row; the rows it shares with
ddimxs_multistep_update; refusals.  The sampler on the tiny model: where it reduces to dpm_solver_steps bit for bit, order 1
against inpaint_steps, the trajectory against the fp64 restatement over the CPU oracle under model_harness's gate, replayed ==
eager, one capture, independent samples, shards, a v model, the known region of the final sample; and the convergence study's
replacement-only gate with the update running in the kernel in fp32."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, synth
from ddim_audio_amd.inpaint_solver import InpaintSolverStepper
from ddim_audio_amd.schedule import guidance_per_step, inpaint_solver_coefficients, logsnr_seq, v_table
import gpu_util as G
import kernel_harness as KH
import model_harness as MH
from model_harness import KERNEL_CASES, KERNEL_IDS, MODES, MODE_IDS
import inpaint_solver_ref as R

pytestmark = pytest.mark.gpu
SEED, FIRST, DRAW_BASE = 0x0123456789ABCDEF, 100, 5


# ---- the kernel through the C ABI --------------------------------------------------------------------------------------------------------
def _rows():
    """Ten fp32 rows.  Row k < 8: a third-order row of a real table at tau = 1, guided, with w1 / w2 / c1 zeroed unless bit 0 / 1 / 2
    of k is set; row 8: the table's final row; row 9: row 7 with rho = 0."""
    a = MH.alphas()
    tab = inpaint_solver_coefficients(logsnr_seq(a, 20), a, 3, 1.0, 0.4).astype(np.float32)
    row = tab[5]
    assert (row[[5, 8, 9, 10, 11, 12]] != 0).all()
    rows = np.tile(row, (10, 1))
    for k in range(8):
        for bit, col in enumerate((11, 12, 5)):
            if not k >> bit & 1:
                rows[k, col] = 0.0
    rows[8] = tab[-1]
    assert rows[8, 4] == 0 and rows[8, 5] == 0 and rows[8, 3] == 1 and rows[8, 9] == 0 and rows[8, 10] == 1 and rows[8, 8] != 0
    rows[9, 8] = 0.0
    return rows


def _nparts(b, per):
    n = int(KH.lib().ddimx_inpaint_partials_floats(b, per))
    assert n > 0 and n % b == 0
    return n // b


def _inputs(b, per):
    """x, e, z, m0, m1, m2, y, d [b, per]; the mask with 0, 1, 0.5 and other fractions; L [b] -- the last sample of a batch has
    L = 0 -- and partials [b, nparts] that add up to it exactly in any order (units of 0.25 spread over the blocks)."""
    v = {s: synth.gaussian(f"isolve.k.{s}.{b}.{per}", (b, per)).numpy() for s in ("x", "e", "z", "m0", "m1", "m2", "y", "d")}
    u = synth.uniform_pm1(f"isolve.k.m.{b}.{per}", b * per).reshape(b, per)
    v["m"] = np.where(u < -0.5, 0.0, np.where(u < 0.0, 1.0, np.where(u < 0.5, 0.5, np.abs(u)))).astype(np.float32)
    v["y"] = (v["y"] * (v["m"] != 0)).astype(np.float32)
    L = np.array({1: [7.0], 2: [7.0, 0.0], 3: [7.0, 2.25, 0.0]}[b], dtype=np.float32)
    nb = _nparts(b, per)
    parts = np.zeros((b, nb), dtype=np.float32)
    for s in range(b):
        for j in range(int(L[s] * 4)):
            parts[s, (j * 5) % nb] += 0.25
    assert np.array_equal(parts.astype(np.float64).sum(1), L.astype(np.float64))
    return v, L, parts


def _nan(*shape):
    return torch.full(shape, KH.NAN)


def _call(v, L, parts, rows, k, flags, h2_given, noise_given, xt_init=None):
    """One call on row k: (outs, want) -- the guarded buffers after it and update32's results.  Whatever the row and the flags
    leave unread is poisoned (NaN in every word)."""
    b, per = v["x"].shape
    n = b * per
    row = rows[k]
    guided, replace = bool(flags & 2), bool(flags & 1)
    use1, use2, add_z = row[11] != 0, bool(row[12] != 0 and h2_given), row[5] != 0
    load1 = use1 or use2
    xt = KH.Out(n, init=(v["x"] if xt_init is None else xt_init) if (replace or not guided) else None)
    x0 = KH.Out(n, init=v["m0"] if guided else None)
    h1 = KH.Out(n, init=v["m1"] if load1 else None)
    h2 = KH.Out(n, init=v["m2"] if use2 else None) if h2_given else None
    e, coef, ctr = KH.Ro(v["e"]), KH.Ro(rows), KH.Ro([k], torch.int32)
    noise = KH.Ro(v["z"] if add_z else _nan(b, per)) if noise_given else None
    y, m = (KH.Ro(v[s] if flags else _nan(b, per)) for s in ("y", "m"))
    d = torch.as_tensor(v["d"]).clone()
    d[torch.as_tensor(L == 0) | (not guided) | bool(row[8] == 0)] = KH.NAN  # read only where the weight is not 0
    d, part = KH.Ro(d), KH.Ro(parts if guided else _nan(*parts.shape))
    rc = KH.lib().ddimxi_multistep_update(xt.ptr, e.ptr, None if noise is None else noise.ptr, x0.ptr, h1.ptr, None if h2 is None else h2.ptr,
                                          y.ptr, m.ptr, d.ptr, part.ptr, coef.ptr, ctr.ptr, b, per, flags, SEED, FIRST, DRAW_BASE,
                                          _lib.stream())
    _lib.check(rc)
    KH.sync()
    for r in (e, coef, ctr, y, m, d, part) + (() if noise is None else (noise,)):
        r.check(f"row {k} flags {flags}")
    z = v["z"]
    if add_z and not noise_given:  # what ddimx_noise_fill writes for this draw
        z = D.NoiseStream(SEED, FIRST).step_noise((b, per), DRAW_BASE + k, G.dev()).cpu().numpy()
    want = R.update32(row, flags, v["x"] if xt_init is None else xt_init, v["e"], z, v["m0"], v["m1"], v["m2"], v["y"], v["m"], v["d"], L,
                      h2_given)
    return (xt, x0, h1, h2), want


def _compare(outs, want, v, what):
    xt, x0, h1, h2 = outs
    b, per = v["x"].shape
    got = xt.read("xt").view(b, per)
    assert bool(torch.isfinite(got).all()), f"{what}: a poisoned buffer reached xt"
    KH.same(got, want[0], f"xt, {what}")
    KH.same(x0.read("x0").view(b, per), v["m0"] if want[1] is None else want[1], f"x0, {what}")
    KH.same(h1.read("h1").view(b, per), want[2], f"h1 <- the guided prediction, {what}")
    if h2 is not None:
        if want[3] is None:
            assert h2.untouched(), f"h2 was written though h1 was not read, {what}"
        else:
            KH.same(h2.read("h2").view(b, per), want[3], f"h2 <- the old h1, {what}")


@pytest.mark.parametrize("b, per", KERNEL_CASES[:2], ids=KERNEL_IDS[:2])
def test_kernel_gives_the_fp32_restatements_bits_and_never_reads_what_a_row_leaves_out(b, per):
    rows = _rows()
    v, L, parts = _inputs(b, per)
    seen = {}
    for flags in range(4):
        for k in range(8):
            for h2_given in (False, True):
                for noise_given in (True, False):
                    outs, want = _call(v, L, parts, rows, k, flags, h2_given, noise_given)
                    _compare(outs, want, v, f"flags {flags}, row {k}, h2 {h2_given}, noise {'given' if noise_given else 'drawn'}")
                    seen[(flags, k, h2_given, noise_given)] = want[0]
    # the terms are really there: the flags, every weight, the drawn noise and the guidance each change the bits
    assert not np.array_equal(seen[(3, 7, True, True)], seen[(1, 7, True, True)]), "guided"
    assert not np.array_equal(seen[(3, 7, True, True)], seen[(2, 7, True, True)]), "replace"
    assert not np.array_equal(seen[(3, 7, True, True)], seen[(3, 7, True, False)]), "the drawn noise is not the buffer's"
    for bit in range(3):
        assert not np.array_equal(seen[(3, 7, True, True)], seen[(3, 7 & ~(1 << bit), True, True)]), f"term {bit}"
    assert not np.array_equal(seen[(3, 3, True, True)], seen[(3, 3, False, True)]), "h2 null: no w2 term"
    # the sample with L = 0 has no guidance term: the bits of the row with rho = 0; the others have one
    unguided = R.update32(rows[9], 3, *(v[s] for s in ("x", "e", "z", "m0", "m1", "m2", "y", "m", "d")), L, True)[0]
    assert np.array_equal(seen[(3, 7, True, True)][-1], unguided[-1]) and not np.array_equal(seen[(3, 7, True, True)][0], unguided[0])


def test_kernel_on_a_sample_longer_than_the_grid():
    b, per = KERNEL_CASES[2]
    rows = _rows()
    v, L, parts = _inputs(b, per)
    outs, want = _call(v, L, parts, rows, 7, 3, True, False)
    _compare(outs, want, v, "grid stride")


@pytest.mark.parametrize("b, per", KERNEL_CASES[:2], ids=KERNEL_IDS[:2])
def test_final_row_returns_y_where_the_mask_is_one(b, per):
    rows = _rows()
    v, L, parts = _inputs(b, per)
    x_bad = v["x"].copy()
    x_bad[:, ::3] = np.inf  # cx = 0: x_t does not reach the known region (guided: nor the prediction, which is read)
    for flags in (1, 3):
        outs, want = _call(v, L, parts, rows, 8, flags, True, True, xt_init=x_bad if flags == 3 else None)
        _compare(outs, want, v, f"final row, flags {flags}")
        got = outs[0].read("xt").view(b, per)
        KH.same(got[torch.as_tensor(v["m"] == 1)], torch.as_tensor(v["y"][v["m"] == 1]), "the known region is y")


@pytest.mark.parametrize("b, per", KERNEL_CASES[:2], ids=KERNEL_IDS[:2])
def test_rows_with_an_empty_mask_and_no_guidance_equal_the_stochastic_solvers_update(b, per):
    """m = 0 everywhere and rho = 0: ddimxs_multistep_update's bits on (t, s1, s2, s3, c2, c1, w1, w2), noise handed and drawn."""
    lib = KH.lib()
    rows = _rows()
    rows[:8, 8] = 0.0
    v, L, parts = _inputs(b, per)
    v = dict(v, m=np.zeros_like(v["m"]), y=np.zeros_like(v["y"]))
    n = b * per
    rows8 = KH.Ro(np.concatenate([rows[:, :6], rows[:, 11:]], axis=1).copy())
    e = KH.Ro(v["e"])
    for k in range(8):
        for h2_given in (False, True):
            for noise_given in (True, False):
                ctr = KH.Ro([k], torch.int32)
                xt, x0 = KH.Out(n, init=v["x"]), KH.Out(n, init=v["m1"])
                hist = KH.Out(n, init=v["m2"]) if h2_given else None
                z = KH.Ro(v["z"]) if noise_given else None
                _lib.check(lib.ddimxs_multistep_update(xt.ptr, e.ptr, None if z is None else z.ptr, x0.ptr, None if hist is None else hist.ptr,
                                                       rows8.ptr, ctr.ptr, b, per, SEED, FIRST, DRAW_BASE, _lib.stream()))
                KH.sync()
                want_x, want_0 = xt.read("xt"), x0.read("x0")
                for flags in (0, 1, 3):
                    vv = dict(v, m0=want_0.view(b, per).numpy()) if flags & 2 else v
                    outs, _ = _call(vv, L, parts, rows, k, flags, h2_given, noise_given)
                    what = f"row {k}, flags {flags}, h2 {h2_given}, noise {'given' if noise_given else 'drawn'}"
                    KH.same(outs[0].read("xt"), want_x, "xt, " + what)
                    KH.same(outs[1].read("x0"), want_0, "x0, " + what)
                    KH.same(outs[2].read("h1"), want_0, "h1, " + what)
                    if h2_given and (rows[k, 11] != 0 or rows[k, 12] != 0):
                        KH.same(outs[3].read("h2"), hist.read("hist"), "h2, " + what)


def test_kernel_refuses_bad_arguments_and_writes_nothing():
    lib, st = KH.lib(), _lib.stream()
    b, per = 2, 16
    n = b * per
    rows = _rows()
    v, L, parts = _inputs(b, per)
    ro = {s: KH.Ro(v[s]) for s in ("e", "z", "y", "m", "d")}
    part, coef, ctr = KH.Ro(parts), KH.Ro(rows), KH.Ro([7], torch.int32)
    outs = {s: KH.Out(n) for s in ("xt", "x0", "h1", "h2")}
    seed_out, part_out = KH.Out(n), KH.Out(parts.size)
    good = dict(xt=outs["xt"].ptr, eps=ro["e"].ptr, noise=ro["z"].ptr, x0=outs["x0"].ptr, h1=outs["h1"].ptr, h2=outs["h2"].ptr, y=ro["y"].ptr,
                mask=ro["m"].ptr, d_x=ro["d"].ptr, partials=part.ptr, coef=coef.ptr, step=ctr.ptr, B=b, per=per, flags=3, first=0)
    bad = [dict(xt=None), dict(eps=None), dict(x0=None), dict(h1=None), dict(coef=None), dict(step=None), dict(y=None), dict(mask=None),
           dict(d_x=None), dict(partials=None), dict(flags=4), dict(flags=-1), dict(flags=1, y=None), dict(B=0), dict(B=65536), dict(per=0),
           dict(per=-16), dict(per=14), dict(first=2 ** 32 - 1)]
    for edit in bad:
        a = dict(good, **edit)
        rc = lib.ddimxi_multistep_update(a["xt"], a["eps"], a["noise"], a["x0"], a["h1"], a["h2"], a["y"], a["mask"], a["d_x"], a["partials"],
                                         a["coef"], a["step"], a["B"], a["per"], a["flags"], SEED, a["first"], 0, st)
        KH.refused(rc, *outs.values(), who="ddimxi_multistep_update")
    rgood = dict(xt=ro["z"].ptr, eps=ro["e"].ptr, y=ro["y"].ptr, mask=ro["m"].ptr, x0=outs["x0"].ptr, seed=seed_out.ptr, partials=part_out.ptr,
                 coef=coef.ptr, step=ctr.ptr, B=b, per=per)
    for edit in [dict(xt=None), dict(eps=None), dict(y=None), dict(mask=None), dict(x0=None), dict(seed=None), dict(partials=None),
                 dict(coef=None), dict(step=None), dict(B=0), dict(per=18)]:
        a = dict(rgood, **edit)
        rc = lib.ddimxi_residual(a["xt"], a["eps"], a["y"], a["mask"], a["x0"], a["seed"], a["partials"], a["coef"], a["step"], a["B"],
                                 a["per"], st)
        KH.refused(rc, outs["x0"], seed_out, part_out, who="ddimxi_residual")
    for r in list(ro.values()) + [part, coef, ctr]:
        r.check("refusals")


@pytest.mark.parametrize("b, per", KERNEL_CASES[:2], ids=KERNEL_IDS[:2])
def test_residual_on_the_wide_row_is_ddimx_inpaint_residual(b, per):
    """The sibling launch: the same kernel on a 13-float row gives the 9-float row's bits in x0, seed and every partial."""
    lib, st = KH.lib(), _lib.stream()
    rows = _rows()
    v, _, parts = _inputs(b, per)
    n = b * per
    ins = [KH.Ro(v[s]) for s in ("x", "e", "y", "m")]
    ctr = KH.Ro([3], torch.int32)
    res = []
    for fn, tab in ((lib.ddimxi_residual, rows), (lib.ddimx_inpaint_residual, rows[:, :9].copy())):
        coef = KH.Ro(tab)
        outs = [KH.Out(n), KH.Out(n), KH.Out(parts.size)]
        _lib.check(fn(*(i.ptr for i in ins), *(o.ptr for o in outs), coef.ptr, ctr.ptr, b, per, st))
        KH.sync()
        res.append([o.read("residual") for o in outs])
    for g, w, what in zip(res[0], res[1], ("x0", "seed", "partials")):
        KH.same(g, w, what)


# ---- the sampler on the tiny model ------------------------------------------------------------------------------------------------------
SHAPES = {"tiny": (2, 2, 16, 32), "ragged": (3, 2, 24, 32)}
FORK = (4, 2, 32, 32)  # B = 4: the replacement-only graph forks into two shards


def _soft_mask(shape):
    b, c, t, f = shape
    m = torch.ones(b, 1, t, f)
    m[:, :, t // 4: t // 2] = 0
    m[:, :, :, -f // 4:] *= 0.5
    m[-1, :, : t // 8] = 0
    return m


@pytest.mark.parametrize("tau", [0.0, 1.0])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_empty_mask_without_guidance_equals_dpm_solver_steps(mode, tau):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    x, y = MH.pair_data("isolve.empty", FORK)
    seq = logsnr_seq(a, 7)
    ns = D.NoiseStream(41, 3) if tau else None
    for order in (1, 2, 3):
        want = D.dpm_solver_steps(x.cuda(), seq, m, a, None, order=order, tau=tau, noise=ns)
        for replace in (True, False):
            got = D.inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y, mask=torch.zeros(1, 1, 1, 1), replace=replace, order=order, tau=tau,
                                         noise=ns)
            MH.same_run(got, want, f"order {order}, replace {replace}")


@pytest.mark.parametrize("case", list(SHAPES))
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_order_1_guided_is_inpaint_steps_with_guidance_per_step(mode, case):
    """Both functions against the fp64 restatement of the folded form over the CPU oracle, each inside model_harness's gate (the
    margin of test_gpu_inpaint.py's guided tests); in fp64 the two agree to 1e-12 (test_inpaint_solver_cpu.py)."""
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 5, mode="eval")
    a, shape = MH.alphas(cfg), SHAPES[case]
    x, y = MH.pair_data("isolve.o1." + case, shape)
    mask, seq, rho = _soft_mask(shape), [0, 250, 500, 750], 0.3
    new = D.inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=rho, replace=False, order=1)
    old = D.inpaint_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=list(guidance_per_step(seq, a, rho)), replace=False)
    ref = R.solver_steps(x.double(), seq, MH.oracle_eps(m), a, y, mask, guidance=rho, replace=False, order=1)
    worst = 0.0
    for i in range(len(seq)):
        for got, name in ((new, "inpaint_solver_steps"), (old, "inpaint_steps")):
            worst = max(worst, MH.gate(got[0][i + 1], ref[0][i + 1], dt, f"{name} xs[{i + 1}]")[0])
            MH.gate(got[1][i], ref[1][i], dt, f"{name} x0[{i}]")
        assert torch.equal(new[1][0], old[1][0]), "the first prediction sees no guidance yet"
    unguided = D.inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=0.0, replace=False, order=1)
    assert MH.differs_anywhere(new, unguided)
    print(f"[inpaint solver order 1 vs inpaint_steps {case} {MODE_IDS[dt]}] worst max {worst:.3e} x rms")


@pytest.mark.parametrize("guided", [False, True], ids=["replace_only", "guided"])
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("case", list(SHAPES))
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_trajectory_vs_the_restatement_on_the_cpu_oracle(mode, case, order, guided):
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 5, mode="eval")
    a, shape = MH.alphas(cfg), SHAPES[case]
    x, y = MH.pair_data("isolve.traj." + case, shape)
    mask, seq = _soft_mask(shape), logsnr_seq(a, 7)
    assert len(seq) == 7
    rho = [0.3, 0.2, 0.0, 0.25, 0.3, 0.3, 0.2] if guided else 0.0
    xs, x0 = D.inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, guidance=rho, replace=True, order=order)
    rxs, rx0 = R.solver_steps(x.double(), seq, MH.oracle_eps(m), a, y, mask, guidance=rho, replace=True, order=order)
    worst = (0.0, 0.0)
    for i in range(len(seq)):
        worst = max(worst, MH.gate(xs[i + 1], rxs[i + 1], dt, f"xs[{i + 1}]"))
        worst = max(worst, MH.gate(x0[i], rx0[i], dt, f"x0[{i}]"))
    print(f"[inpaint solver vs restatement {case} order {order} {'guided' if guided else 'replace'} {MODE_IDS[dt]}] worst max "
          f"{worst[0]:.3e} rms err {worst[1]:.3e} x rms")
    MH.known_exact(xs[-1], y, mask)
    if guided:
        plain = R.solver_steps(x.double(), seq, MH.oracle_eps(m), a, y, mask, guidance=0.0, replace=True, order=order)[0]
        assert float((plain[-2] - rxs[-2]).abs().max()) > 1e-3, "the reference's guidance is no small term"


@pytest.mark.parametrize("guided", [True, False], ids=["guided", "replace_only"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_replayed_equals_eager(mode, guided):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    x, y = MH.pair_data("isolve.replay", FORK)
    kw = dict(y=y, mask=_soft_mask(FORK), guidance=0.3 if guided else 0.0, order=3, tau=1.0, noise=D.NoiseStream(42, 1))
    seq = logsnr_seq(a, 6)
    got = D.inpaint_solver_steps(x.cuda(), seq, m, a, None, **kw)
    with MH.eager_steps():
        MH.same_run(D.inpaint_solver_steps(x.cuda(), seq, m, a, None, **kw), got, "eager")
    assert MH.differs_anywhere(got, D.inpaint_solver_steps(x.cuda(), seq, m, a, None, **dict(kw, tau=0.0))), "the noise is no small term"


@pytest.mark.parametrize("guided", [True, False], ids=["guided", "replace_only"])
def test_stepper_captures_one_graph_and_owns_its_history(guided):
    cfg, m = MH.build("tiny", "torch.cuda.FloatTensor", 5, mode="eval")
    a = MH.alphas(cfg)
    shape = SHAPES["tiny"]
    x = synth.gaussian("isolve.one", shape).cuda()
    seq = logsnr_seq(a, 6)
    coef = inpaint_solver_coefficients(seq, a, 3, 1.0, 0.3 if guided else 0.0)
    with torch.no_grad():
        st = InpaintSolverStepper(m, x, torch.zeros_like(x), torch.ones_like(x), coef, 3, guided, True, noise=D.NoiseStream(1, 0))
        try:
            for _ in range(len(seq)):
                st.step()
            assert st.captures == 1 and st.graph is not None
            assert st.h1.shape == x.shape and st.h2.shape == x.shape and st.noise_buf is None
            st.rewind()
            m.invalidate()  # new packed values in place: the graph stays
            st.step()
            assert st.captures == 1
        finally:
            st.close()
        st = InpaintSolverStepper(m, x, torch.zeros_like(x), torch.ones_like(x), inpaint_solver_coefficients(seq, a, 2, 0.0, 0.0), 2, False, True)
        assert st.h2 is None and st.seed is None
        st.close()
        with pytest.raises(ValueError, match="beyond its order"):
            InpaintSolverStepper(m, x, torch.zeros_like(x), torch.ones_like(x), coef, 2, guided, True, noise=D.NoiseStream(1, 0))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_samples_are_independent(mode):
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a, shape = MH.alphas(cfg), SHAPES["tiny"]
    x, y = MH.pair_data("isolve.indep", shape)
    mask, seq = _soft_mask(shape), logsnr_seq(a, 5)
    kw = dict(guidance=0.3, order=3)
    one = D.inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, **kw)
    y2, mask2 = y.clone(), mask.clone()
    y2[0] *= 3.0
    mask2[0] = 1.0
    two = D.inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y2, mask=mask2, **kw)
    assert not torch.equal(one[0][-1][0], two[0][-1][0])
    for i in range(len(seq)):
        assert torch.equal(one[0][i + 1][1], two[0][i + 1][1]) and torch.equal(one[1][i][1], two[1][i][1]), i


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_eight_samples_equal_two_shards_of_four(mode):
    """Replacement only, whose forward is the inference one (a sample's bits do not depend on its batch); the noise is the
    stream's, by global sample index."""
    cfg, m = MH.build("tiny", mode[0], 5, mode="eval")
    a = MH.alphas(cfg)
    shape = (8,) + FORK[1:]
    x, y = MH.pair_data("isolve.shard", shape)
    mask, seq, ns = _soft_mask(shape), logsnr_seq(a, 5), D.NoiseStream(43, 7)
    mask[3, :, :2] = 0  # the whole batch's last-sample edit, on a sample of the first shard too
    kw = dict(order=3, tau=1.0)
    whole = D.inpaint_solver_steps(x.cuda(), seq, m, a, None, y=y, mask=mask, noise=ns, **kw)
    for lo in (0, 4):
        part = D.inpaint_solver_steps(x[lo:lo + 4].cuda(), seq, m, a, None, y=y[lo:lo + 4], mask=mask[lo:lo + 4], noise=ns.shard(lo), **kw)
        MH.same_run(part, ([u[lo:lo + 4] for u in whole[0]], [u[lo:lo + 4] for u in whole[1]]), f"shard {lo}")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_v_model_equals_the_wrapped_eps_callable(mode):
    cfg, mv, ms, a = MH.pair("tiny", mode[0])
    x, y = MH.pair_data("isolve.v", FORK)
    kw = dict(y=y, mask=_soft_mask(FORK), order=2, tau=1.0, noise=D.NoiseStream(44, 2))
    seq = logsnr_seq(a, 6)
    got = D.inpaint_solver_steps(x.cuda(), seq, mv, a, None, **kw)
    with MH.eager_steps():  # the callable allocates
        want = D.inpaint_solver_steps(x.cuda(), seq, MH.v_wrapped(ms, v_table(a)), a, None, prediction="eps", **kw)
    MH.same_run(got, want, "v model")
    assert MH.differs_anywhere(got, D.inpaint_solver_steps(x.cuda(), seq, ms, a, None, **kw)), "the twin reads the output as eps"
    MH.known_exact(got[0][-1], y, kw["mask"])
    # guided: the seed is the gradient w.r.t. v (k1, k2 of prediction="v"); the run is finite, moves, and keeps the known region
    guided = D.inpaint_solver_steps(x.cuda(), seq, mv, a, None, guidance=0.3, **kw)
    assert all(bool(torch.isfinite(u).all()) for u in guided[0][1:]) and MH.differs_anywhere(guided, got)
    MH.known_exact(guided[0][-1], y, kw["mask"])


def test_device_repeats_the_replacement_only_gate_in_fp32():
    """tests/test_inpaint_solver_cpu.py's study with the update running in the kernel: the 12-dimensional correlated Gaussian, its
    exact predictor as the callable, against the float64 order-2 run on logsnr_seq(a, 734).  Errors of 1e-3 and more sit three
    orders above the fp32 floor."""
    a = MH.alphas()
    _, x, y, mask, M = R.gaussian_case(a)
    Md = M.float().to(G.dev())
    model = lambda xx, t: (Md[t] * xx.view(xx.size(0), 1, -1)).sum(-1).view_as(xx)  # noqa: E731  (eps = M[t] x)
    shape = (1, 1, 1, R.DIM)

    def final(seq, order, **kw):
        xs, _ = D.inpaint_solver_steps(x.float().view(shape).cuda(), seq, model, a, [-1], y=y.float().view(shape), mask=mask.view(shape),
                                       order=order, **kw)
        return xs[-1].view(1, R.DIM)

    e = R.study(a, modes={"replace": R.MODES["replace"]}, steps=(20, 50), orders=(1, 2), final=final)["replace"]
    r_order, r_steps = e[(20, 1)] / e[(20, 2)], e[(20, 2)] / e[(50, 2)]
    print(f"[inpaint solver study on the device]\n{R.table(e, (20, 50), (1, 2))}\n"
          f"order 1 / order 2 at 20 steps = {r_order:.2f}; order 2 at 20 / at 50 steps = {r_steps:.2f}")
    assert r_order >= 3.0 and r_steps >= 3.0
