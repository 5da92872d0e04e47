"""References for the kernels of csrc/pack_kernels.hip, temb_kernels.hip and step_kernels.hip (test infrastructure; CPU only).

Packing and layout: explicit permute / flip / reshape on the parameter's own shape, written from the layout comments of
pack_kernels.h, pack_kernels.hip, conv_wreg.h and include/ddimx.h -- never from a kernel's flattened index arithmetic.  They return
fp32 torch tensors in the packed layout's shape; ``bf16`` rounds one the way the activation dtype is defined (torch's CPU cast:
round to nearest even).  Linear layers: float64.  ddimx_ddim_update has no reference here: it is ``step_math_ref.update_core3``.
ddpm_update: the separately rounded fp32 chain of test_host_cpu.py::test_ddpm_coefficients_reproduce_golden."""
import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32


# ---- number formats ------------------------------------------------------------------------------------------------------------------
def bf16(x):
    """fp32 -> bf16, round to nearest even (torch's CPU cast)."""
    return torch.as_tensor(x, dtype=torch.float32).to(torch.bfloat16)


def bits(x):
    """The bits of a tensor as integers of its element size, for exact comparisons (NaN payloads included)."""
    x = x.detach().cpu().contiguous()
    return x.view({2: torch.int16, 4: torch.int32}[x.element_size()])


# ---- conv weights ---------------------------------------------------------------------------------------------------------------------
def pack_conv(w):
    """Conv2d.weight [O][I][KH][KW] -> [KH*KW][O][I] (tap = kh * KW + kw)."""
    O, I, KH, KW = w.shape
    return w.permute(2, 3, 0, 1).reshape(KH * KW, O, I).contiguous()


def pack_conv_dgrad(w):
    """[O][I][3][3] -> [9][I][O]: input and output channels transposed, the kernel flipped in both directions (tap' = 8 - tap)."""
    O, I, KH, KW = w.shape
    assert (KH, KW) == (3, 3)
    return torch.flip(w, dims=(2, 3)).permute(2, 3, 1, 0).reshape(9, I, O).contiguous()


def convT_taps():
    """The sub-pixel form's definition as a list of (a, tap, b, kh, kw): output (2 py + a, 2 px + b) reads input
    (py + dy - 1, px + dx - 1), dy = a + dyi, tap = dyi * 3 + dx, through kernel element (3 + a - 2 dy, 3 + b - 2 dx); kw is None where
    that element lies outside 0..3 (the packed weight is zero there)."""
    out = []
    for a in range(2):
        for dyi in range(2):
            for dx in range(3):
                for b in range(2):
                    kh, kw = 3 + a - 2 * (a + dyi), 3 + b - 2 * dx
                    assert 0 <= kh < 4
                    out.append((a, dyi * 3 + dx, b, kh, kw if 0 <= kw < 4 else None))
    return out


def pack_convT(w):
    """ConvTranspose2d(k4, s2, p1).weight [I][O][4][4] -> [2 (a)][6 (tap)][2 * O (b * O + co)][I]."""
    I, O = w.shape[:2]
    out = torch.zeros(2, 6, 2, O, I, dtype=w.dtype)
    for a, tap, b, kh, kw in convT_taps():
        if kw is not None:
            out[a, tap, b] = w[:, :, kh, kw].t()
    return out.reshape(2, 6, 2 * O, I)


def convT_zero_mask(I, O):
    """True where pack_convT's zero-fill rule applies, in the packed shape."""
    m = torch.zeros(2, 6, 2, O, I, dtype=torch.bool)
    for a, tap, b, kh, kw in convT_taps():
        if kw is None:
            m[a, tap, b] = True
    return m.reshape(2, 6, 2 * O, I)


def frag_from_taps(taps):
    """Tap layout [ntaps][NOUT][CIN] -> MFMA fragment order (conv_wreg.h):
    wf[step = tap * KG + kg][nb][lane = h * 32 + l31][j] = W[cout = nb * 32 + l31][tap][cin = kg * 16 + h * 8 + j]."""
    nt, NOUT, CIN = taps.shape
    assert NOUT % 32 == 0 and CIN % 16 == 0
    v = taps.reshape(nt, NOUT // 32, 32, CIN // 16, 2, 8)  # tap, nb, l31, kg, h, j
    return v.permute(0, 3, 1, 4, 2, 5).reshape(nt * (CIN // 16), NOUT // 32, 64, 8).contiguous()


def pack_conv_frag(w):
    """[O][I][KH][KW] fp32 -> fragment order of the tap layout (the caller rounds to bf16)."""
    return frag_from_taps(pack_conv(w))


# ---- activations ------------------------------------------------------------------------------------------------------------------------
def to_nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def from_nhwc(y):
    return y.permute(0, 3, 1, 2).contiguous()


# ---- the FNet boundary's token order ---------------------------------------------------------------------------------------------------
def perm_cols(src, C, Fr):
    """dst[r][f * C + c] = src[r][c * Fr + f]."""
    rows = src.shape[0]
    return src.reshape(rows, C, Fr).transpose(1, 2).reshape(rows, Fr * C).contiguous()


def perm_rows(src, C, Fr):
    """dst[f * C + c][k] = src[c * Fr + f][k]."""
    K = src.shape[1]
    return src.reshape(C, Fr, K).transpose(0, 1).reshape(Fr * C, K).contiguous()


# ---- naive convolutions over the packed layouts (test_temb_step_pack_cpu.py holds the references above to torch with them) -----------------
def conv_from_packed(x, packed, KH, KW, stride):
    """Conv2d(k, stride, padding 1) of x [B][I][H][W] through the tap layout [KH*KW][O][I], one tap at a time."""
    B, I, H, W = x.shape
    Ho, Wo = (H + 2 - KH) // stride + 1, (W + 2 - KW) // stride + 1
    xp = F.pad(x, (1, 1, 1, 1))
    y = torch.zeros(B, packed.shape[1], Ho, Wo, dtype=x.dtype)
    for kh in range(KH):
        for kw in range(KW):
            win = xp[:, :, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride]
            y += torch.einsum("oi,bihw->bohw", packed[kh * KW + kw], win)
    return y


def convT_from_packed(x, packed):
    """ConvTranspose2d(k4, s2, p1) of x [B][I][H][W] through the sub-pixel form [2][6][2 * O][I]."""
    B, I, H, W = x.shape
    O = packed.shape[2] // 2
    xp = F.pad(x, (1, 1, 1, 1))  # xp[.., py + dy, px + dx] = x[.., py + dy - 1, px + dx - 1]
    y = torch.zeros(B, O, 2 * H, 2 * W, dtype=x.dtype)
    for a in range(2):
        for dyi in range(2):
            for dx in range(3):
                win = xp[:, :, a + dyi:a + dyi + H, dx:dx + W]
                both = torch.einsum("vi,bihw->bvhw", packed[a, dyi * 3 + dx], win)
                for b in range(2):
                    y[:, :, a::2, b::2] += both[:, b * O:(b + 1) * O]
    return y


# ---- timestep-embedding MLP (float64) -----------------------------------------------------------------------------------------------------
def silu(v):
    return v / (1.0 + np.exp(-v))


def dsilu(v):
    s = 1.0 / (1.0 + np.exp(-v))
    return s * (1.0 + v * (1.0 - s))


def _rows(x, idx):
    x = np.asarray(x, dtype=np.float64)
    return x if idx is None else x[np.asarray(idx, dtype=np.int64)]


def linear(x, W, bias, idx=None, act_silu=False, in_silu=False):
    """y = g(f(x[idx]) W^T + bias), f / g = SiLU where asked."""
    xr = _rows(x, idx)
    y = (silu(xr) if in_silu else xr) @ np.asarray(W, dtype=np.float64).T + np.asarray(bias, dtype=np.float64)
    return silu(y) if act_silu else y


def linear_bwd_w(dy, x, idx=None, x_silu=False):
    """(dW, db) = (dy^T f(x[idx]), column sums of dy)."""
    xr, dy = _rows(x, idx), np.asarray(dy, dtype=np.float64)
    return dy.T @ (silu(xr) if x_silu else xr), dy.sum(axis=0)


def linear_bwd_x(dy, W, xpre):
    """dx = (dy W) SiLU'(xpre)."""
    return (np.asarray(dy, dtype=np.float64) @ np.asarray(W, dtype=np.float64)) * dsilu(np.asarray(xpre, dtype=np.float64))


def temb_train(te, t, w0, b0, w1, b1, w2, b2, d_out):
    """The training forward and backward of BetaEmbedding as the library splits it, from the three functions above: a dict of
    h1_pre, h2_pre, out, d_h2, d_h1 and the six parameter gradients."""
    r = {}
    r["h1_pre"] = linear(te, w0, b0, idx=t)
    r["h2_pre"] = linear(r["h1_pre"], w1, b1, in_silu=True)
    r["out"] = linear(r["h2_pre"], w2, b2, in_silu=True)
    r["d_w2"], r["d_b2"] = linear_bwd_w(d_out, r["h2_pre"], x_silu=True)
    r["d_h2"] = linear_bwd_x(d_out, w2, r["h2_pre"])
    r["d_w1"], r["d_b1"] = linear_bwd_w(r["d_h2"], r["h1_pre"], x_silu=True)
    r["d_h1"] = linear_bwd_x(r["d_h2"], w1, r["h1_pre"])
    r["d_w0"], r["d_b0"] = linear_bwd_w(r["d_h1"], te, idx=t)
    return r


def temb_autograd(te, t, w0, b0, w1, b1, w2, b2, d_out):
    """The same through torch autograd in float64 (pre-activations kept as leaves' consumers): the same dict."""
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    p = {k: T(v).requires_grad_(True) for k, v in dict(w0=w0, b0=b0, w1=w1, b1=b1, w2=w2, b2=b2).items()}
    h1 = F.linear(T(te).index_select(0, torch.as_tensor(np.asarray(t, dtype=np.int64))), p["w0"], p["b0"])
    h2 = F.linear(F.silu(h1), p["w1"], p["b1"])
    out = F.linear(F.silu(h2), p["w2"], p["b2"])
    h1.retain_grad(), h2.retain_grad()
    out.backward(T(d_out))
    r = {"h1_pre": h1, "h2_pre": h2, "out": out, "d_h1": h1.grad, "d_h2": h2.grad}
    r.update({"d_" + k: v.grad for k, v in p.items()})
    return {k: v.detach().numpy() for k, v in r.items()}


# ---- sampler steps ------------------------------------------------------------------------------------------------------------------------
def step_begin(coef, stride, step, B):
    """t[B] = the first entry of row `step` of a table with `stride` floats per row, as int64."""
    return np.full(B, int(np.asarray(coef, dtype=F32).reshape(-1)[step * stride]), dtype=np.int64)


def ddpm_update(x, e, noise, row):
    """functions/denoising.py:72-90 with every product, sum and the division rounded to fp32 on its own.  row: the 7 fp32 scalars
    of schedule.ddpm_coefficients.  Returns (clamped x0 prediction, sample)."""
    _, a0, a1, m1, m2, den, sig = (F32(v) for v in row)
    x, e, noise = (np.asarray(v, dtype=F32) for v in (x, e, noise))
    p0 = np.clip((a0 * x).astype(F32) - (a1 * e).astype(F32), -1, 1).astype(F32)
    mean = (((m1 * p0).astype(F32) + (m2 * x).astype(F32)).astype(F32) / den).astype(F32)
    return p0, (mean + (sig * noise).astype(F32)).astype(F32)
