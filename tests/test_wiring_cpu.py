"""tests/wiring_ref.py on the CPU: the response statistic and its noise formula on synthetic fields, the oracle against itself on the
tiny network (every parameter meets the input condition at the shape and amplitudes the GPU test uses; the control pairs are apart
with the reference alone), and the bookkeeping that turns byte diffs of a packed buffer into regions."""
import math

import numpy as np
import pytest
import torch

import model_harness as H
import wiring_ref as W
from ddim_audio_amd import synth


# ---- the statistic on synthetic fields -------------------------------------------------------------------------------------------------
def _field(tag, n):
    return synth.gaussian("wiring.cpu." + tag, (n,)).double()


@pytest.mark.parametrize("g", [W.G_BOUND["bf16"], W.G_BOUND["f32"]], ids=["bf16", "f32"])
@pytest.mark.parametrize("m", [0.016, 0.3])
def test_projection_on_synthetic_fields(g, m):
    """y = a field of rms 1, D_ref of rms m; both outputs carry white noise of rms g (the gate's level): a true response projects to 1
    within 5 n, no response to 0 within 5 n, n = sqrt(2) g / (m sqrt(N))."""
    N = 8192
    d_ref = _field("dref", N) * m
    y_i = _field("y", N)
    m_i = W.strength(d_ref, y_i)
    n = W.noise(g, m_i, N)
    e0, e1 = _field("e0", N) * g * W.rms(y_i), _field("e1", N) * g * W.rms(y_i)
    c_read = W.projection((y_i + e1) - (y_i - d_ref + e0), d_ref)
    c_ignored = W.projection(e1 - e0, d_ref)
    print(f"[wiring statistic g={g:g} m={m:g}] n {n:.2e}, c read {c_read:.4f}, c ignored {c_ignored:.4f}")
    assert abs(c_read - 1.0) <= 5 * n and abs(c_ignored) <= 5 * n
    assert (W.C_LO <= c_read <= W.C_HI) and not (W.C_LO <= c_ignored <= W.C_HI)


def test_noise_formula_matches_the_empirical_spread():
    """200 draws of the two outputs' noise: the standard deviation of c within a factor of 2 of the formula."""
    N, g, m = 4096, 5e-2, 0.05
    d_ref = _field("spread.dref", N) * m
    y_i = _field("spread.y", N)
    n = W.noise(g, W.strength(d_ref, y_i), N)
    cs = []
    for k in range(200):
        e0, e1 = _field(f"spread.e0.{k}", N), _field(f"spread.e1.{k}", N)
        cs.append(W.projection(d_ref + (e1 - e0) * g * W.rms(y_i), d_ref))
    sd = float(np.std(cs))
    print(f"[wiring noise] formula {n:.3e}, empirical {sd:.3e}, mean c {np.mean(cs):.4f}")
    assert n / 2 <= sd <= 2 * n
    assert abs(np.mean(cs) - 1.0) <= 5 * n / math.sqrt(200) + 1e-12


# ---- the oracle against itself, tiny network ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    cfg, m = H.build("tiny", "torch.FloatTensor", 5, mode="eval")  # a CPU model: only its state dict is used
    live, ocfg = H.oracle(m, "tiny")
    sd = {k: v.detach() for k, v in live.items()}
    return cfg, sd, W.case_forward("tiny", ocfg)


def test_every_tiny_parameter_meets_the_input_condition_and_the_table_is_minimal(tiny):
    """At CASES["tiny"] with AMP["tiny"]: n_i <= N_MAX under the loosest gate (bf16) for all 104 parameters; and the table is what the
    rule gives: amplitude 1 where that meets the condition with 1 % to spare (N_TABLE), else 4, else 16."""
    cfg, sd, fwd = tiny
    names = W.case_names("tiny", list(sd))
    assert len(names) == 104
    g = W.G_BOUND["bf16"]
    plain = W.judge_inputs(W.oracle_responses(fwd, sd, names, {}, {}), names, g)
    derived = {}
    for n in names:
        if plain[n][1] <= W.N_TABLE:
            continue
        for a in (4.0, 16.0):
            if W.judge_inputs(W.oracle_responses(fwd, sd, [n], {n: a}, {}), [n], g)[n][1] <= W.N_TABLE:
                derived[n] = a
                break
        else:
            raise AssertionError(f"{n}: no amplitude up to 16 meets the input condition")
    assert derived == W.AMP["tiny"], (sorted(set(derived.items()) ^ set(W.AMP["tiny"].items())))
    final = W.judge_inputs(W.oracle_responses(fwd, sd, names, W.AMP["tiny"], {}), names, g)
    worst = max(final, key=lambda k: final[k][1])
    print(f"[wiring tiny oracle] {len(names)} parameters, {len(derived)} at amplitude 4; faintest {worst}: m {final[worst][0]:.3e}, "
          f"n {final[worst][1]:.3e}")
    assert final[worst][1] <= W.N_TABLE


def test_tiny_control_pairs_are_apart_with_the_reference_alone(tiny):
    cfg, sd, fwd = tiny
    names = W.case_names("tiny", list(sd))
    cache = W.oracle_responses(fwd, sd, names, W.AMP["tiny"], {})
    base = cache["base"]
    pairs = [p for ns in W.groups(list(sd), len(cfg.model.ch)).values() for p in W.control_pairs(ns, "tiny")]
    assert len(pairs) >= 40
    worst = (0.0, None)
    for i, j in pairs:
        assert sd[i].shape == sd[j].shape
        c = W.projection(cache[j][1] - base, cache[i][1] - base)
        worst = max(worst, (abs(c), (i, j)))
        assert abs(c) < W.CONTROL_MAX, (i, j, c)
        assert abs(W.projection(cache[i][1] - base, cache[i][1] - base) - 1.0) < 1e-12
    print(f"[wiring tiny control] {len(pairs)} ordered pairs, worst |c_ij| {worst[0]:.3f} {worst[1]}")


def test_groups_cover_the_audio_inventory():
    from ddim_audio_amd import configs
    from ddim_audio_amd.model import state_inventory
    names = list(state_inventory(configs.audio_config("torch.FloatTensor")))
    gs = W.groups(names, 6)
    assert sum(len(v) for v in gs.values()) == 388 and len(gs) == 16
    assert max(len(v) for v in gs.values()) == 51 and len(gs["temb"]) == 6 and len(gs["edge"]) == 4
    assert set(W.AMP["audio"]) <= set(names) and len(W.case_names("fnet", names)) == 102
    for net, dropped in W.CONTROL_DROPPED.items():
        for u, v in dropped:
            assert u != v and (net != "audio" or (u in names and v in names))


# ---- region bookkeeping --------------------------------------------------------------------------------------------------------------------
def test_regions_from_byte_diffs():
    """A hand-made buffer of 256-byte blocks: [0, 512) from a; [512, 768) from a and b, directly behind it; [768, 1024) untouched;
    [1024, 2048) from c with its two middle blocks and most bytes of the others unchanged; the last region ends with the buffer,
    which is no whole block."""
    total = 2048 + 100
    mk = lambda: np.zeros(total, dtype=bool)  # noqa: E731
    a, b, c, d = mk(), mk(), mk(), mk()
    a[0:512] = True
    a[512:768:2] = True
    b[513:768:2] = True
    c[1024 + 7] = True
    c[2047] = True
    d[2048:total] = True
    blk = lambda **masks: {k: W.changed_blocks(v) for k, v in masks.items()}  # noqa: E731
    assert W.changed_blocks(c).tolist() == [4, 7] and W.changed_blocks(d).tolist() == [8]
    got = W.regions(blk(a=a, b=b, c=c, d=d), total)
    assert got == {frozenset("a"): (0, 512), frozenset("ab"): (512, 768), frozenset("c"): (1024, 2048), frozenset("d"): (2048, total)}
    assert W.regions(blk(a=mk()), total) == {} and W.regions({}, total) == {}
    # a set of sources whose blocks lie on both sides of another set's: not a layout of regions
    e, f = mk(), mk()
    e[0] = e[600] = True
    f[300] = True
    with pytest.raises(ValueError):
        W.regions(blk(e=e, f=f), total)
