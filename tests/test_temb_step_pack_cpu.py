"""The references of tests/temb_step_pack_ref.py held to torch and to the oracle, without a GPU: a convolution through each packed
layout equals the torch op in float64, the two token-order permutations undo each other, the bf16 rounding is round to nearest even,
the linear-layer references chained as the library chains them equal autograd of oracle/ref_cpu.beta_embedding, and the two
sampler-step mirrors equal torch's fp32 chains."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import step_math_ref as SM
import temb_step_pack_ref as P
from tail_kernel_ref import gauss, rng
from oracle import ref_cpu


def t64(tag, shape):
    return torch.from_numpy(rng(tag).standard_normal(shape))


def close64(got, want, what):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((got - want).abs().max()) / float(want.abs().max())
    assert err <= 1e-12, (what, err)


# ---- conv layouts -----------------------------------------------------------------------------------------------------------------------
def test_pack_conv_3x3_is_the_conv():
    w, x = t64("cpu.c3.w", (5, 7, 3, 3)), t64("cpu.c3.x", (2, 7, 6, 9))
    close64(P.conv_from_packed(x, P.pack_conv(w), 3, 3, 1), F.conv2d(x, w, padding=1), "3x3")


def test_pack_conv_4x4_stride_2_is_the_downsample_conv():
    w, x = t64("cpu.c4.w", (8, 3, 4, 4)), t64("cpu.c4.x", (2, 3, 6, 10))
    close64(P.conv_from_packed(x, P.pack_conv(w), 4, 4, 2), F.conv2d(x, w, stride=2, padding=1), "4x4 s2")


def test_pack_convT_is_the_transposed_conv():
    w, x = t64("cpu.ct.w", (6, 5, 4, 4)), t64("cpu.ct.x", (2, 6, 3, 7))
    packed = P.pack_convT(w)
    close64(P.convT_from_packed(x, packed), F.conv_transpose2d(x, w, stride=2, padding=1), "convT")
    mask = P.convT_zero_mask(6, 5)
    assert int(mask.sum()) == 2 * 2 * 2 * 5 * 6  # per row parity a: two dyi x (b = 0 at dx = 2, b = 1 at dx = 0)
    assert (packed[mask] == 0).all() and (packed[~mask] != 0).all()


def test_pack_conv_dgrad_is_the_data_gradient():
    w, dy = t64("cpu.dg.w", (5, 7, 3, 3)), t64("cpu.dg.dy", (2, 5, 4, 6))
    x = torch.zeros(2, 7, 4, 6, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, padding=1).backward(dy)
    close64(P.conv_from_packed(dy, P.pack_conv_dgrad(w), 3, 3, 1), x.grad, "dgrad")


def test_fragment_order_from_its_formula():
    """Every element of the fragment layout, by the index formula of conv_wreg.h in plain loops."""
    O, I, KK = 64, 32, 4
    w = t64("cpu.frag.w", (O, I, 2, 2))
    got = P.pack_conv_frag(w)
    assert got.shape == (KK * I // 16, O // 32, 64, 8)
    flat = w.reshape(O, I, KK)
    for step in range(KK * I // 16):
        tap, kg = divmod(step, I // 16)
        for nb in range(O // 32):
            for lane in range(64):
                h, l31 = divmod(lane, 32)
                want = flat[nb * 32 + l31, kg * 16 + h * 8:kg * 16 + h * 8 + 8, tap]
                assert torch.equal(got[step, nb, lane], want), (step, nb, lane)
    assert torch.equal(P.frag_from_taps(P.pack_conv(w)), got)


def test_layout_converters_are_transposes():
    x = t64("cpu.nhwc", (2, 3, 5, 7))
    y = P.to_nhwc(x)
    assert y.shape == (2, 5, 7, 3) and y[1, 4, 6, 2] == x[1, 2, 4, 6] and torch.equal(P.from_nhwc(y), x)


# ---- permutations -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C, Fr", [(5, 3), (256, 8), (1, 4), (4, 1)])
def test_token_order_permutations_are_inverses(C, Fr):
    cols, rows = t64(f"cpu.pc.{C}.{Fr}", (3, C * Fr)), t64(f"cpu.pr.{C}.{Fr}", (C * Fr, 7))
    pc, pr = P.perm_cols(cols, C, Fr), P.perm_rows(rows, C, Fr)
    assert pc[2, (Fr - 1) * C + (C - 1) // 2] == cols[2, ((C - 1) // 2) * Fr + Fr - 1]
    assert torch.equal(pr[(Fr - 1) * C + (C - 1) // 2], rows[((C - 1) // 2) * Fr + Fr - 1])
    assert torch.equal(P.perm_cols(pc, Fr, C), cols) and torch.equal(P.perm_rows(pr, Fr, C), rows)
    assert torch.equal(P.perm_rows(cols.t().contiguous(), C, Fr).t(), pc)  # the two are one permutation, of columns or of rows


# ---- bf16 ---------------------------------------------------------------------------------------------------------------------------------
def test_bf16_reference_rounds_to_nearest_even():
    f = lambda b: torch.tensor([b], dtype=torch.int32).view(torch.float32)  # noqa: E731
    h = lambda x: int(P.bits(P.bf16(x))[0]) & 0xFFFF  # noqa: E731
    assert h(f(0x3F808000)) == 0x3F80 and h(f(0x3F818000)) == 0x3F82  # ties: to the even neighbour, down and up
    assert h(f(0x3F808001)) == 0x3F81 and h(f(0x3F817FFF)) == 0x3F81  # just above / below a tie
    assert h(f(0x7F7FFFFF)) == 0x7F80                                  # the largest fp32 rounds to +inf
    assert h(f(0x00000001)) == 0x0000 and h(f(0x00018000)) == 0x0002   # denormals: flushed by rounding, and a denormal tie


# ---- the embedding MLP ------------------------------------------------------------------------------------------------------------------
def test_linear_references_chain_to_autograd_of_the_oracle():
    pos_ch, emb_ch, E, B = 128, 512, 4416, 4
    g = lambda tag, shape, s=1.0: rng("cpu.temb." + tag).standard_normal(shape) * s  # noqa: E731
    te, t = g("te", (1000, pos_ch)), np.array([999, 0, 417, 0])
    w0, b0 = g("w0", (emb_ch, pos_ch), pos_ch ** -0.5), g("b0", (emb_ch,), 0.1)
    w1, b1 = g("w1", (emb_ch, emb_ch), emb_ch ** -0.5), g("b1", (emb_ch,), 0.1)
    w2, b2 = g("w2", (E, emb_ch), emb_ch ** -0.5), g("b2", (E,), 0.1)
    d_out = g("dout", (B, E))
    got = P.temb_train(te, t, w0, b0, w1, b1, w2, b2, d_out)
    want = P.temb_autograd(te, t, w0, b0, w1, b1, w2, b2, d_out)
    assert set(got) == set(want)
    for k in sorted(got):
        close64(got[k], want[k], k)
    names = ("weight.0.weight", "weight.0.bias", "weight.1.weight", "weight.1.bias", "weight.2.weight", "weight.2.bias")
    sd = {"temb." + n: torch.from_numpy(v).requires_grad_(True) for n, v in zip(names, (w0, b0, w1, b1, w2, b2))}
    sd["temb.te"] = torch.from_numpy(te)
    out = ref_cpu.beta_embedding(sd, torch.from_numpy(t))
    out.backward(torch.from_numpy(d_out))
    close64(got["out"], out.detach(), "out against the oracle")
    for n, k in zip(names, ("d_w0", "d_b0", "d_w1", "d_b1", "d_w2", "d_b2")):
        close64(got[k], sd["temb." + n].grad, k + " against the oracle")
    # the activations on their own, and the row gather
    x = g("x", (5, 8))
    close64(P.linear(x, g("w", (3, 8)), g("b", (3,)), idx=[4, 0, 4], act_silu=True, in_silu=True),
            F.silu(F.linear(F.silu(torch.from_numpy(x)[[4, 0, 4]]), torch.from_numpy(g("w", (3, 8))), torch.from_numpy(g("b", (3,))))), "linear")


# ---- sampler steps ------------------------------------------------------------------------------------------------------------------------
def test_ddim_update_mirror_equals_the_torch_chain():
    """The mirror against the reference's in-place fp32 chain (functions/denoising.py:27,41-43): torch's add_(alpha=) is a product and
    a sum rounded separately where step_math.h fuses them, so the two differ by an ulp here and there and no more."""
    from ddim_audio_amd import schedule
    from tail_kernel_ref import alphas
    for eta in (0.0, 0.5):
        coef = schedule.ddim_coefficients(list(range(0, 1000, 100)), alphas(), eta).astype(np.float32)
        for row in (coef[0], coef[-1]):
            x, e, z = gauss("cpu.ddim.x", 4096), gauss("cpu.ddim.e", 4096), gauss("cpu.ddim.z", 4096)
            u, x0 = SM.update_core3(x, e, None, None, None, SM.load_row(row), False, False, False, bool(eta), z)
            _, s1, s2, s3, c2, c1 = (float(v) for v in row)
            ref = torch.from_numpy(x.copy()).add_(torch.from_numpy(e), alpha=-s1).div_(s2)
            assert torch.allclose(torch.from_numpy(x0), ref, rtol=3e-7, atol=1e-7)
            ref = ref.mul_(s3).add_(torch.from_numpy(e), alpha=c2)
            if eta:
                ref.add_(torch.from_numpy(z), alpha=c1)
            assert torch.allclose(torch.from_numpy(u), ref, rtol=1e-6, atol=1e-6)
    assert P.step_begin(coef, 6, len(coef) - 1, 3).tolist() == [0, 0, 0] and P.step_begin(coef, 6, 0, 2).tolist() == [900, 900]


def test_ddpm_update_mirror_equals_the_torch_chain_bit_for_bit():
    from ddim_audio_amd import schedule
    betas = np.linspace(1e-4, 0.02, 1000, dtype=np.float64).astype(np.float32)
    coef = schedule.ddpm_coefficients(list(range(0, 1000, 100)), betas)
    for row in (coef[0], coef[-1]):
        for scale in (0.2, 3.0):
            x, e, z = (torch.from_numpy(gauss(f"cpu.ddpm.{k}", 4099) * np.float32(scale)) for k in "xez")
            _, a0, a1, m1, m2, den, sig = (torch.tensor(v) for v in row)
            p0 = torch.clamp(a0 * x - a1 * e, -1, 1)
            want = (m1 * p0 + m2 * x) / den + sig * z
            got0, got = P.ddpm_update(x.numpy(), e.numpy(), z.numpy(), row)
            assert np.array_equal(got0, p0.numpy()) and np.array_equal(got, want.numpy())
            assert scale < 1 or ((got0 == 1).any() and (got0 == -1).any() and (np.abs(got0) < 1).any())
