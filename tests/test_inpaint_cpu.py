"""Masked DDIM inpainting, host side (no GPU): the coefficient table the kernels read, argument validation before any device
work, and the k1 / k2 split of the guidance gradient against plain autograd in fp64 through the CPU oracle."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import configs, synth
from ddim_audio_amd.schedule import ddim_coefficients, inpaint_coefficients
from oracle import ref_cpu

import inpaint_ref
import model_harness as MH


@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("seq", [list(range(0, 1000, 100)), [0, 13, 400, 999], [250]])
def test_coefficient_table(seq, eta):
    a = MH.alphas()
    n = len(seq)
    zeta = [0.1 * (i + 1) for i in range(n)]
    for g, want in ((0.0, np.zeros(n)), (0.35, np.full(n, 0.35)), (zeta, np.asarray(zeta))):
        c = inpaint_coefficients(seq, a, eta, g)
        assert c.dtype == np.float64 and c.shape == (n, 9)
        base = ddim_coefficients(seq, a, eta)
        assert np.array_equal(c[:, :6], base), "columns 0-5 must be ddim_coefficients bit for bit"
        s1, s2 = base[:, 1], base[:, 2]
        assert np.array_equal(c[:, 6], -2.0 * s1 / s2)
        assert np.array_equal(c[:, 7], 2.0 / s2)
        assert np.array_equal(c[:, 8], want)
    # the last row of a schedule that starts at 0 ends the path: s3 = 1, c2 = c1 = 0 (the known region becomes y exactly)
    if seq[0] == 0:
        assert tuple(c[-1, 3:6]) == (1.0, 0.0, 0.0)


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf"), [0.1, 0.2], [[0.1] * 3], [0.1, -0.2, 0.0]])
def test_coefficient_table_rejects_bad_guidance(bad):
    with pytest.raises(ValueError):
        inpaint_coefficients([0, 100, 200], MH.alphas(), 0.0, bad)


def _call(**kw):
    x = kw.pop("x", torch.zeros(2, 2, 16, 32))
    args = dict(y=torch.zeros(2, 2, 16, 32), mask=torch.ones(2, 1, 16, 1), guidance=0.0)
    args.update(kw)
    # the model is never reached: validation comes before any device work (None would fail at the first forward)
    return D.inpaint_steps(x, [0, 300, 600], None, MH.alphas(), None, **args)


@pytest.mark.parametrize("kw,msg", [
    (dict(mask=torch.ones(2, 2, 16, 3)), "broadcast"),
    (dict(mask=torch.ones(3, 1, 1, 1)), "broadcast"),
    (dict(y=torch.zeros(2, 2, 17, 32)), "broadcast"),
    (dict(y=torch.zeros(2, 2, 16, 32, 1)), "broadcast"),
    (dict(mask=torch.full((1, 1, 1, 32), 1.5)), "[0, 1]"),
    (dict(mask=torch.full((1, 1, 1, 32), -1)), "[0, 1]"),
    (dict(mask=torch.full((1, 1, 1, 32), float("nan"))), "[0, 1]"),
    (dict(mask=torch.full((1, 1, 1, 32), 2, dtype=torch.int64)), "[0, 1]"),
    (dict(guidance=-1.0), "guidance"),
    (dict(guidance=float("inf")), "guidance"),
    (dict(guidance=[1.0, 2.0]), "guidance"),
    (dict(guidance=[1.0, 2.0, 3.0, 4.0]), "guidance"),
    (dict(mask=None), "mask"),
    (dict(y=None), "y="),
    (dict(x=torch.zeros(2, 16, 32)), "[B, C, T, F]"),
    (dict(x=torch.zeros(1, 1, 3, 3), y=torch.zeros(1, 1, 3, 3), mask=torch.ones(1, 1, 3, 3)), "multiple of 4"),
    (dict(x=torch.zeros(2, 1, 3, 6), y=torch.zeros(2, 1, 3, 6), mask=torch.ones(2, 1, 3, 6)), "multiple of 4"),
    (dict(eta=-0.5), "eta"),
])
def test_invalid_arguments_raise_before_device_work(kw, msg):
    with pytest.raises(ValueError) as e:
        _call(**kw)
    assert msg in str(e.value)


@pytest.mark.parametrize("guidance", [0.3, 0.0], ids=["guided", "replace_only"])
@pytest.mark.parametrize("shape,msg", [((2, 2, 16, 16), "does not match the model"), ((2, 2, 16, 64), "does not match the model"),
                                       ((2, 1, 16, 32), "does not match the model"), ((2, 2, 10, 32), "multiple of 4 for this model")])
def test_shape_must_match_the_model(shape, msg, guidance):
    """The guided step gives x, eps and d_x to the library, which sizes them from the model's config: a sample of another C or F,
    or a T the U-Net cannot halve, must raise before any device work (the model here never leaves the CPU)."""
    m = D.Model(configs.tiny_config("torch.FloatTensor"))  # F = 32, C = 2, three levels
    with pytest.raises(ValueError) as e:
        D.inpaint_steps(torch.zeros(shape), [0, 300, 600], m, MH.alphas(), None, y=torch.zeros(shape),
                        mask=torch.ones(1, 1, shape[2], 1), guidance=guidance)
    assert msg in str(e.value)


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_k1_k2_decomposition_equals_autograd_fp64(name):
    """g = k2 m r + J_eps^T (k1 m r) with k1, k2 from the table the kernels read equals autograd of L_b w.r.t. x_t (fp64)."""
    cfg = configs.micro_config("torch.FloatTensor") if name == "micro" else configs.tiny_config("torch.FloatTensor")
    sd = {k: v.double() for k, v in synth.fill_state_dict(_state(cfg), seed=4).items()}
    f = cfg.model.f_size
    shape = (2, cfg.model.channels, 16, f)
    x = synth.gaussian("inp.dec.x", shape).double()
    y = synth.gaussian("inp.dec.y", shape).double()
    m = torch.ones(2, 1, 16, f, dtype=torch.float64)
    m[:, :, 5:11] = 0
    m[1, :, :, : f // 2] *= 0.5
    seq = [0, 300, 700]
    coef = inpaint_coefficients(seq, MH.alphas(), 0.0, 0.5)
    row = coef[1]
    t = torch.full((2,), int(row[0]), dtype=torch.long)
    s1, s2, k1, k2 = row[1], row[2], row[6], row[7]

    def fwd(v, tt=t):
        return ref_cpu.model_forward(sd, cfg, v, tt)

    # plain DPS: autograd of the per-sample norm
    xg = x.clone().requires_grad_(True)
    e = fwd(xg)
    x0 = (xg - s1 * e) / s2
    L = (m * (x0 - y)).square().flatten(1).sum(1)
    (g_auto,) = torch.autograd.grad(L.sum(), xg)
    # the split the kernels compute: seed = k1 m r through J_eps^T, plus k2 m r
    xg2 = x.clone().requires_grad_(True)
    e2 = fwd(xg2)
    x0d = ((x - s1 * e2.detach()) / s2)
    q = m * (m * (x0d - y))
    (d_x,) = torch.autograd.grad(e2, xg2, k1 * q)
    g = k2 * q + d_x
    rel = float((g - g_auto).abs().max() / g_auto.abs().max())
    assert rel <= 1e-10, rel
    # and the restatement the GPU tests use takes the same gradient
    _, _, L_ref = inpaint_ref.step(fwd, x, row[:6], 0.5, y * (m != 0), m, True, False)
    assert torch.allclose(L_ref, L.detach(), rtol=1e-12, atol=0)


def _state(cfg):
    from ddim_audio_amd.model import state_inventory, timestep_table
    sd = {k: torch.zeros(v) for k, v in state_inventory(cfg).items()}
    sd["temb.te"] = timestep_table(*state_inventory(cfg)["temb.te"])
    return sd
