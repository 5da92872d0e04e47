"""GPU parity tests, per operator: HIP kernels (through the C ABI) vs the CPU oracle and the golden
vectors produced by the real reference.  fp32 mode gate: max|d| <= 1e-4*std; bf16 mode gate:
rms <= 2e-2*std, max <= 1.5e-1*std."""
import numpy as np
import pytest
import torch

from ddim_audio_amd import _lib, synth
from oracle import ref_cpu
import gpu_util as G
from model_harness import rb_sd

pytestmark = pytest.mark.gpu
DTS = [G.F32, G.BF16]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c,hw", [(32, (16, 8)), (64, (5, 7)), (96, (8, 8)), (128, (4, 8)), (192, (3, 5)), (256, (2, 8))])
def test_resblock_golden(golden, dt, c, hw):
    p = f"rb{c}."
    sd = rb_sd(p, c)
    x = synth.gaussian(p + "x", (2, c, *hw))
    temb = synth.gaussian(p + "temb", (2, c)) * 0.5
    y = G.resblock(sd, p, x, temb, dt)
    G.check_close(y, golden("blocks")[f"rb{c}_y"], dt, f"resblock C={c}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c,hw,b", [(32, (40, 72), 3), (32, (40, 96), 3), (64, (24, 40), 2), (96, (17, 33), 2), (128, (16, 24), 2),
                                    (192, (9, 20), 1), (256, (20, 9), 2)])
def test_resblock_multi_tile(dt, c, hw, b):
    """Shapes that span several workgroup tiles with ragged edges, checked against the CPU oracle."""
    p = f"rbm{c}."
    sd = rb_sd(p, c)
    x = synth.gaussian(p + "x", (b, c, *hw)) * 1.5 + 0.3
    temb = synth.gaussian(p + "temb", (b, c)) * 0.5
    y = G.resblock(sd, p, x, temb, dt)
    G.check_close(y, ref_cpu.residual_block(sd, p, x, temb), dt, f"resblock C={c} {hw}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin,cout,hw", [(32, 64, (8, 16)), (96, 128, (6, 10)), (192, 256, (4, 8))])
def test_down_up_golden(golden, dt, cin, cout, hw):
    gb = golden("blocks")
    sd = synth.fill_state_dict({f"down{cin}.conv.weight": torch.empty(cout, cin, 4, 4), f"down{cin}.conv.bias": torch.empty(cout),
                                f"up{cout}.conv.weight": torch.empty(cout, cin, 4, 4), f"up{cout}.conv.bias": torch.empty(cin)})
    yd = G.downsample(sd[f"down{cin}.conv.weight"], sd[f"down{cin}.conv.bias"], synth.gaussian(f"down{cin}.x", (2, cin, *hw)), dt)
    G.check_close(yd, gb[f"down{cin}_y"], dt, f"down {cin}->{cout}")
    xu = synth.gaussian(f"up{cout}.x", (2, cout, hw[0] // 2, hw[1] // 2))
    zero = torch.zeros(2, cin, hw[0], hw[1])
    yu = G.upsample_add(sd[f"up{cout}.conv.weight"], sd[f"up{cout}.conv.bias"], xu, zero, dt)
    G.check_close(yu, gb[f"up{cout}_y"], dt, f"up {cout}->{cin}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin,cout,hw", [(32, 64, (36, 44)), (64, 96, (20, 36)), (96, 128, (18, 22)), (128, 192, (10, 18)),
                                         (192, 256, (12, 20))])
def test_down_up_multi_tile(dt, cin, cout, hw):
    sd = synth.fill_state_dict({"d.conv.weight": torch.empty(cout, cin, 4, 4), "d.conv.bias": torch.empty(cout),
                                "u.conv.weight": torch.empty(cout, cin, 4, 4), "u.conv.bias": torch.empty(cin)})
    x = synth.gaussian(f"dm{cin}.x", (2, cin, *hw))
    yd = G.downsample(sd["d.conv.weight"], sd["d.conv.bias"], x, dt)
    G.check_close(yd, ref_cpu.downsample(sd, "d.", x), dt, f"down {cin}->{cout}")
    xu = synth.gaussian(f"um{cout}.x", (2, cout, hw[0] // 2, hw[1] // 2))
    skip = synth.gaussian(f"um{cout}.s", (2, cin, 2 * (hw[0] // 2), 2 * (hw[1] // 2)))
    yu = G.upsample_add(sd["u.conv.weight"], sd["u.conv.bias"], xu, skip, dt)
    G.check_close(yu, ref_cpu.upsample(sd, "u.", xu) + skip, dt, f"up {cout}->{cin}")


def test_temb_golden(golden):
    gm = golden("model")
    lib = _lib.load()
    shapes = {"temb.weight.0.weight": (512, 128), "temb.weight.0.bias": (512,), "temb.weight.1.weight": (512, 512),
              "temb.weight.1.bias": (512,), "temb.weight.2.weight": (4416, 512), "temb.weight.2.bias": (4416,)}
    sd = synth.fill_state_dict({k: torch.empty(s) for k, s in shapes.items()})
    te = G.g(ref_cpu.timestep_table(1000))
    t = torch.from_numpy(gm["temb_t"]).to(G.dev())
    ws = [G.g(sd[f"temb.weight.{i}.{k}"]) for i in range(3) for k in ("weight", "bias")]
    h1, h2 = torch.empty(4, 512, device=G.dev()), torch.empty(4, 512, device=G.dev())
    out = torch.empty(4, 4416, device=G.dev())
    _lib.check(lib.ddimx_temb_fwd(_lib.ptr(te), _lib.ptr(t), *[_lib.ptr(w) for w in ws], _lib.ptr(h1), _lib.ptr(h2), _lib.ptr(out),
                                  4, 128, 512, 4416, _lib.stream()))
    G.check_close(out.cpu(), gm["temb_y"], G.F32, "temb")


def test_temb_vs_oracle_batch_19():
    """ddimx_temb_fwd at B = 19 against ref_cpu.beta_embedding (models/diffusion.py:110-120): linear_rows_kernel walks the batch in
    groups of 8 -- two full groups and one of three rows, with a repeated timestep."""
    lib = _lib.load()
    shapes = {"temb.weight.0.weight": (512, 128), "temb.weight.0.bias": (512,), "temb.weight.1.weight": (512, 512),
              "temb.weight.1.bias": (512,), "temb.weight.2.weight": (4416, 512), "temb.weight.2.bias": (4416,)}
    sd = synth.fill_state_dict({k: torch.empty(s) for k, s in shapes.items()})
    sd["temb.te"] = ref_cpu.timestep_table(1000)
    t = torch.tensor([0, 999, 123, 500, 7, 7, 1, 998, 250, 251, 640, 33, 812, 77, 404, 999, 512, 5, 321])
    B = t.numel()
    te, tg = G.g(sd["temb.te"]), t.to(G.dev())
    ws = [G.g(sd[f"temb.weight.{i}.{k}"]) for i in range(3) for k in ("weight", "bias")]
    h1, h2 = torch.empty(B, 512, device=G.dev()), torch.empty(B, 512, device=G.dev())
    out = torch.full((B, 4416), float("nan"), device=G.dev())
    _lib.check(lib.ddimx_temb_fwd(_lib.ptr(te), _lib.ptr(tg), *[_lib.ptr(w) for w in ws], _lib.ptr(h1), _lib.ptr(h2), _lib.ptr(out),
                                  B, 128, 512, 4416, _lib.stream()))
    G.check_close(out.cpu(), ref_cpu.beta_embedding(sd, t), G.F32, "temb B=19")


def test_ddim_update_matches_oracle_bitwise(golden):
    """The fused update kernel against the oracle's in-place chain with an analytic eps (exact same fp32 ops)."""
    from ddim_audio_amd import schedule
    lib = _lib.load()
    gs = golden("schedule")
    alphas = torch.from_numpy(gs["alphas"])
    seq = list(range(0, 1000, 100))
    coef = schedule.ddim_coefficients(seq, alphas, 0.0)
    x = synth.gaussian("upd.x", (2, 2, 8, 16))
    e = synth.gaussian("upd.e", (2, 2, 8, 16))
    cd = torch.from_numpy(coef.astype(np.float32)).to(G.dev())
    step = torch.zeros(1, dtype=torch.int32, device=G.dev())
    xt, eg = x.to(G.dev()).clone(), e.to(G.dev())
    x0 = torch.empty_like(xt)
    ref = x.clone()
    a = [1.0] + alphas.numpy().tolist()
    for k, (i, j) in enumerate(zip(reversed(seq), reversed([-1] + seq[:-1]))):
        _lib.check(lib.ddimx_ddim_update(_lib.ptr(xt), _lib.ptr(eg), None, _lib.ptr(x0), _lib.ptr(cd), _lib.ptr(step), xt.numel(), _lib.stream()))
        _lib.check(lib.ddimx_step_end(_lib.ptr(step), _lib.stream()))
        at, an = a[i + 1], a[j + 1]
        ref.add_(e, alpha=-((1 - at) ** 0.5)).div_(at ** 0.5)
        r0 = ref.clone()
        ref.mul_(an ** 0.5).add_(e, alpha=(1 - an) ** 0.5)
        assert torch.allclose(x0.cpu(), r0, rtol=3e-7, atol=1e-7), k
        assert torch.allclose(xt.cpu(), ref, rtol=3e-7, atol=1e-7), k
    assert int(step.item()) == len(seq)


@pytest.mark.parametrize("b,s_len,hid", [(3, 32, 512), (2, 16, 512), (1, 8, 256), (2, 24, 128)])
def test_fnet_fourier_mixing(b, s_len, hid):
    """Re(FFT2(x)) + x: the single-launch kernel and the two-GEMM path against torch.fft on the CPU (fp32, exact MFMA)."""
    import numpy as np
    from ddim_audio_amd.model import _dft_tables
    lib = _lib.load()
    x = synth.gaussian(f"mix.x{s_len}.{hid}", (b, s_len, hid))
    want = torch.fft.fftn(x.double(), dim=(1, 2)).real.float() + x
    ch, sh = _dft_tables(hid)
    cs, ss = _dft_tables(s_len)
    dh = torch.from_numpy(np.stack([ch, sh], axis=1).reshape(2 * hid, hid)).cuda()
    ds = torch.from_numpy(np.concatenate([cs, -ss], axis=1)).contiguous().cuda()
    xg = x.cuda()
    ut = torch.empty(b * 2 * hid * s_len, device="cuda")
    part = torch.empty(8 * b * 2 * hid * s_len, device="cuda")
    outs = {}
    for fused in (0, 1):
        if fused and not lib.ddimx_fnet_mix_supported(s_len, hid):
            continue
        z = torch.full_like(xg, float("nan"))
        _lib.check(lib.ddimx_fnet_mix(_lib.ptr(dh), _lib.ptr(ds), _lib.ptr(xg), _lib.ptr(z), _lib.ptr(ut), _lib.ptr(part), b, s_len, hid,
                                      fused, _lib.stream()))
        outs[fused] = z.cpu()
        G.check_close(outs[fused], want, G.F32, f"fourier mixing fused={fused}")
    assert 1 in outs or not lib.ddimx_fnet_mix_supported(s_len, hid)


# ---- Transformer_Module as one op (ddimx_fnet_fwd) against the reference-generated G5 fixtures -------------------------
_FNET_MODELS = {}


def _fnet_model(act, fnet):
    """The full-size network's parameters (hash fill by name, as oracle/make_golden.py gave the reference), packed once."""
    import ddim_audio_amd as D
    from ddim_audio_amd import configs
    key = (act, fnet)
    if key not in _FNET_MODELS:
        _FNET_MODELS.clear()
        m = synth.fill_module(D.Model(configs.audio_config(f"torch.cuda.{act}", f"torch.cuda.{fnet}"))).eval()
        _FNET_MODELS[key] = m
    return _FNET_MODELS[key]


@pytest.mark.parametrize("act,fnet,mx,rms", [("FloatTensor", "FloatTensor", 1e-4, 2e-5),          # parity mode
                                            ("BFloat16Tensor", "FloatTensor", 2e-2, 4e-3),        # the reference's mixed mode
                                            ("BFloat16Tensor", "BFloat16Tensor", 6e-2, 1.2e-2)])  # bf16 GEMM operands
@pytest.mark.parametrize("s", [4, 32, 96])
def test_fnet_fwd_golden(golden, act, fnet, mx, rms, s):
    """models/diffusion.py:148-167 (pos-enc + LayerNorm + projection + 12 FNet layers + compute_out) through ddimx_fnet_fwd
    against `fnet_s{4,32,96}_y` written by the real reference (S = 96 exercises the rounded-up pos-enc table and the
    two-GEMM Fourier path, S <= 32 the fused mixing kernel).  Gates relative to the std of the expected output; measured
    worst cases on MI355X: fp32 3e-6 / 6e-7, bf16 activations + fp32 FNet 6e-3 / 1.3e-3 (only the token rounding),
    bf16 operands 2.3e-2 / 4.5e-3."""
    import ctypes
    lib = _lib.load()
    m = _fnet_model(act, fnet)
    dev = G.dev()
    t_len = s * 32
    lib2 = m._ensure_handle()
    with torch.cuda.device(dev):
        m._ensure_packed(lib2, dev)
        pe, dh, ds = m._ensure_tables(t_len, dev)
    tok = synth.gaussian(f"fnet.x{s}", (1, s, 2048))
    # reference token order c*8 + f (models/diffusion.py:273-278)  ->  NHWC rows [S][Fr=8][C=256]
    x = tok.view(1, s, 256, 8).permute(0, 1, 3, 2).contiguous().to(dev, m._act_dtype)
    ws = torch.empty(int(lib.ddimx_workspace_bytes(m._handle, 1, t_len)), dtype=torch.uint8, device=dev)
    out = torch.full((s, 2048), float("nan"), device=dev)
    tb = _lib.DdimxTables(pe.data_ptr(), dh.data_ptr(), ds.data_ptr())
    _lib.check(lib.ddimx_fnet_fwd(m._handle, _lib.ptr(m._packed), ctypes.byref(tb), _lib.ptr(ws), ws.numel(), _lib.ptr(x), _lib.ptr(out),
                                  1, t_len, _lib.stream()))
    y = out.cpu().view(1, s, 8, 256).permute(0, 1, 3, 2).reshape(1, s, 2048)
    want = torch.from_numpy(golden("model")[f"fnet_s{s}_y"]).double().reshape(-1)
    got = y.double().reshape(-1)
    assert torch.isfinite(got).all()
    sd = float(want.std())
    e_mx, e_rms = float((got - want).abs().max()) / sd, float((got - want).square().mean().sqrt()) / sd
    print(f"[fnet_fwd {act}/{fnet} S={s}] max {e_mx:.2e} rms {e_rms:.2e} of std")
    assert e_mx <= mx and e_rms <= rms, (act, fnet, s, e_mx, e_rms)


@pytest.mark.parametrize("act,fnet,mx,rms", [("FloatTensor", "FloatTensor", 1e-4, 2e-5), ("BFloat16Tensor", "FloatTensor", 2e-2, 4e-3),
                                            ("BFloat16Tensor", "BFloat16Tensor", 6e-2, 1.2e-2)])
@pytest.mark.parametrize("s", [8, 16, 24, 32])
def test_fnet_dense_path_vs_oracle_and_batch_independence(act, fnet, mx, rms, s):
    """S <= 32 runs the FNet without split-K workspaces and LayerNorm launches (csrc/fnet_dense.hip: row statistics handed
    from producer to consumer, gamma / beta folded into packed weights, waves of a workgroup splitting K): every supported
    sequence length, three samples at once, against ``ref_cpu.transformer_module`` (models/diffusion.py:148-167); the middle
    sample alone must reproduce its rows of the batch bit for bit (per-sample workgroups, fixed summation orders)."""
    import ctypes
    from oracle import ref_cpu
    lib = _lib.load()
    m = _fnet_model(act, fnet)
    dev = G.dev()
    t_len = s * 32
    lib2 = m._ensure_handle()
    with torch.cuda.device(dev):
        m._ensure_packed(lib2, dev)
        pe, dh, ds = m._ensure_tables(t_len, dev)
    tok = synth.gaussian(f"fnet.dense.x{s}", (3, s, 2048))
    tb = _lib.DdimxTables(pe.data_ptr(), dh.data_ptr(), ds.data_ptr())

    def run(tk):
        n = tk.shape[0]
        x = tk.view(n, s, 256, 8).permute(0, 1, 3, 2).contiguous().to(dev, m._act_dtype)
        ws = torch.empty(int(lib.ddimx_workspace_bytes(m._handle, n, t_len)), dtype=torch.uint8, device=dev)
        out = torch.full((n * s, 2048), float("nan"), device=dev)
        _lib.check(lib.ddimx_fnet_fwd(m._handle, _lib.ptr(m._packed), ctypes.byref(tb), _lib.ptr(ws), ws.numel(), _lib.ptr(x), _lib.ptr(out),
                                      n, t_len, _lib.stream()))
        return out.cpu().view(n, s, 8, 256).permute(0, 1, 3, 2).reshape(n, s, 2048)

    y = run(tok)
    kw = m.config.transformers.kwargs
    sd = {k: v.detach().cpu().float() for k, v in m.state_dict().items() if k.startswith("transformer.")}
    with torch.no_grad():
        want = ref_cpu.transformer_module(sd, tok, kw.num_hidden_layers, kw.layer_norm_eps).double().reshape(-1)
    got = y.double().reshape(-1)
    assert torch.isfinite(got).all()
    sdv = float(want.std())
    e_mx, e_rms = float((got - want).abs().max()) / sdv, float((got - want).square().mean().sqrt()) / sdv
    print(f"[fnet_dense {act}/{fnet} S={s}] max {e_mx:.2e} rms {e_rms:.2e} of std")
    assert e_mx <= mx and e_rms <= rms, (act, fnet, s, e_mx, e_rms)
    assert torch.equal(run(tok[1:2])[0], y[1]), "a sample's FNet output depends on its batch neighbours"


def test_fnet_dense_and_gemm_paths_agree_and_follow_the_packing():
    """ddimx_pack_weights alone (what a training step's repack does) leaves the FNet's inference-only copies stale, and the forward
    must then take the GEMM path; ddimx_pack_fnet_inference brings the launch-lean path back.  Both paths compute the same function
    (models/diffusion.py:148-167): fp32 mode, S = 32 -- equal to rounding; the dense path before and after is bit-identical."""
    import ctypes
    lib = _lib.load()
    m = _fnet_model("FloatTensor", "FloatTensor")
    dev = G.dev()
    s, t_len = 32, 1024
    lib2 = m._ensure_handle()
    with torch.cuda.device(dev):
        m._ensure_packed(lib2, dev)
        pe, dh, ds = m._ensure_tables(t_len, dev)
    tok = synth.gaussian("fnet.paths.x", (2, s, 2048))
    x = tok.view(2, s, 256, 8).permute(0, 1, 3, 2).contiguous().to(dev, m._act_dtype)
    ws = torch.empty(int(lib.ddimx_workspace_bytes(m._handle, 2, t_len)), dtype=torch.uint8, device=dev)
    tb = _lib.DdimxTables(pe.data_ptr(), dh.data_ptr(), ds.data_ptr())

    def run():
        out = torch.full((2 * s, 2048), float("nan"), device=dev)
        _lib.check(lib.ddimx_fnet_fwd(m._handle, _lib.ptr(m._packed), ctypes.byref(tb), _lib.ptr(ws), ws.numel(), _lib.ptr(x), _lib.ptr(out),
                                      2, t_len, _lib.stream()))
        return out.cpu()

    dense = run()
    tensors = m._state_tensors()
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    _lib.check(lib.ddimx_pack_weights(m._handle, arr, len(tensors), _lib.ptr(m._packed), _lib.stream()))
    gemm = run()
    assert torch.isfinite(gemm).all()
    assert not torch.equal(gemm, dense), "the repack should have sent the forward down the GEMM path"
    sd = float(dense.double().std())
    assert float((gemm - dense).abs().max()) / sd <= 2e-5
    _lib.check(lib.ddimx_pack_fnet_inference(m._handle, _lib.ptr(m._packed), _lib.stream()))
    assert torch.equal(run(), dense)


# ---- edge convolutions as single ops -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin,c0,hw,b", [(2, 32, (40, 256), 2), (2, 32, (7, 24), 3), (2, 64, (9, 16), 2)])
def test_conv_in_fwd_vs_oracle(dt, cin, c0, hw, b):
    """`down_modules[0]` (models/diffusion.py:189-198): NCHW fp32 -> NHWC, plus the GroupNorm partials of its output."""
    lib = _lib.load()
    h, w = hw
    sd = synth.fill_state_dict({"cin.weight": torch.empty(c0, cin, 3, 3), "cin.bias": torch.empty(c0)})
    x = synth.gaussian(f"cin.x{c0}.{h}", (b, cin, h, w))
    want = torch.nn.functional.conv2d(x, sd["cin.weight"], sd["cin.bias"], padding=1)
    y = torch.empty((b, h, w, c0), dtype=G.TORCH_DT[dt], device=G.dev())
    n_st = int(lib.ddimx_conv_in_stats_floats(b, c0, h, w))
    stats = torch.full((n_st,), float("nan"), device=G.dev())
    xg, wg, bg = G.g(x), G.g(sd["cin.weight"]), G.g(sd["cin.bias"])
    _lib.check(lib.ddimx_conv_in_fwd(dt, _lib.ptr(xg), _lib.ptr(wg), _lib.ptr(bg), _lib.ptr(y), _lib.ptr(stats), b, cin, c0, h, w,
                                     _lib.stream()))
    got = G.from_nhwc(y, dt)
    G.check_close(got, want, dt, f"conv_in {cin}->{c0} {hw}")
    # statistics slabs [B][nparts][C0][2] = per-channel (sum, sum of squares) of the values as stored
    st = stats.cpu().view(b, -1, c0, 2).double().sum(1)
    ref = got.double()
    assert torch.allclose(st[..., 0], ref.sum((2, 3)), rtol=1e-4, atol=1e-2 * h * w ** 0.5)
    assert torch.allclose(st[..., 1], ref.square().sum((2, 3)), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c0,cout,hw,b", [(32, 2, (40, 256), 2), (32, 2, (9, 24), 3), (40, 2, (10, 16), 2)])
def test_conv_out_fwd_vs_oracle(dt, c0, cout, hw, b):
    """`up_modules[-1]` applied to `x + hidden[0]` (models/diffusion.py:199-208,283-292): two NHWC tensors -> NCHW fp32."""
    lib = _lib.load()
    h, w = hw
    sd = synth.fill_state_dict({"cout.weight": torch.empty(cout, c0, 3, 3), "cout.bias": torch.empty(cout)})
    a = synth.gaussian(f"cout.a{c0}.{h}", (b, c0, h, w))
    s = synth.gaussian(f"cout.b{c0}.{h}", (b, c0, h, w)) * 0.7
    an, sn = G.to_nhwc(a, dt), G.to_nhwc(s, dt)
    a_r, s_r = G.from_nhwc(an, dt), G.from_nhwc(sn, dt)  # the operands as the kernel sees them (rounded in bf16 mode)
    # bf16 mode: the 32-channel kernel stages the sum in the activation dtype (one more bf16 rounding, like `x + hidden[0]`
    # on bf16 tensors), the generic kernel keeps the fp32 sum; fp32 accumulation either way
    ssum = (a_r + s_r).bfloat16().float() if (dt == G.BF16 and c0 == 32) else a_r + s_r
    want = torch.nn.functional.conv2d(ssum, sd["cout.weight"], sd["cout.bias"], padding=1)
    wp = G.pack_conv(sd["cout.weight"], G.F32)
    bg = G.g(sd["cout.bias"])
    eps = torch.full((b, cout, h, w), float("nan"), device=G.dev())
    _lib.check(lib.ddimx_conv_out_fwd(dt, _lib.ptr(an), _lib.ptr(sn), _lib.ptr(wp), _lib.ptr(bg), _lib.ptr(eps), b, c0, cout, h, w,
                                      _lib.stream()))
    G.check_close(eps.cpu(), want, G.F32, f"conv_out {c0}->{cout} {hw}")


# ---- 3x3 conv with the weights streamed straight into registers (csrc/conv_wreg.h) -------------------------------------------------
@pytest.mark.parametrize("xf", [2, 1, 0], ids=["affine_silu", "affine", "none"])
@pytest.mark.parametrize("c,hw", [(64, (16, 64)), (96, (16, 32)), (128, (8, 64)), (192, (8, 32)), (256, (8, 16)),
                                  (96, (1040, 32)), (64, (1048, 32))])  # (tall: two tiles per workgroup -- the weight ring wraps)
def test_wreg_conv_vs_fp32_reference(c, hw, xf):
    """Both convs of Residual_Block (models/diffusion.py:46-53) as the inference walk launches them from C = 64 up: GroupNorm
    affine (+ SiLU) on the input while the halo is staged, weights in MFMA fragment order read straight into registers, + bias /
    + timestep embedding, SiLU, group statistics.  Against fp32 torch on the same bf16-rounded operands: multi-tile images with all
    four borders, statistics of the values as stored."""
    import torch.nn.functional as F
    lib = _lib.load()
    dt, b = G.BF16, 2
    h, w = hw
    dev = G.dev()
    x = (synth.gaussian(f"wreg.x{c}", (b, c, h, w)) * 1.2 + 0.2).bfloat16().float()
    wt = synth.gaussian(f"wreg.w{c}", (c, c, 3, 3)) / (9 * c) ** 0.5
    bias = synth.gaussian(f"wreg.b{c}", (c,)) * 0.3
    temb = synth.gaussian(f"wreg.t{c}", (b, c)) * 0.3
    scale = synth.gaussian(f"wreg.s{c}", (b, c)) * 0.3 + 1.0
    shift = synth.gaussian(f"wreg.h{c}", (b, c)) * 0.5
    xn, wp = G.to_nhwc(x, dt), G.pack_conv(wt, dt)
    wf = torch.empty(9 * c * c, dtype=torch.bfloat16, device=dev)
    wt_d = wt.to(dev).contiguous()
    _lib.check(lib.ddimx_pack_conv_frag(_lib.ptr(wt_d), _lib.ptr(wf), c, c, _lib.stream()))
    y = torch.empty_like(xn)
    stats = torch.zeros(int(lib.ddimx_conv3x3_stats_floats(dt, c, b, h, w)), device=dev)
    bias_d, temb_d, scale_d, shift_d = bias.to(dev), temb.to(dev), scale.to(dev), shift.to(dev)
    use_temb = xf == 2
    _lib.check(lib.ddimx_conv3x3_wreg_fwd(c, _lib.ptr(xn), _lib.ptr(wp), _lib.ptr(wf), None if use_temb else _lib.ptr(bias_d),
                                          _lib.ptr(temb_d) if use_temb else None, c, _lib.ptr(scale_d), _lib.ptr(shift_d), xf, 1,
                                          _lib.ptr(y), _lib.ptr(stats), b, h, w, _lib.stream()))
    torch.cuda.synchronize()
    got = G.from_nhwc(y, dt)
    yn = x
    if xf:
        yn = x * scale[:, :, None, None] + shift[:, :, None, None]
        if xf == 2:
            yn = F.silu(yn)
    yn = yn.bfloat16().float()  # the kernel rounds the transformed input to bf16 before the MFMAs
    add = temb[:, :, None, None] if use_temb else bias[None, :, None, None]
    want = F.silu(F.conv2d(yn, wt.bfloat16().float(), None, padding=1) + add)
    G.check_close(got, want, dt, f"wreg conv C={c} {hw} xf={xf}")
    st = stats.cpu().view(-1, c, 2).double().sum(0)
    gs = got.double()
    assert torch.allclose(st[:, 0], gs.sum(dim=(0, 2, 3)), rtol=1e-4, atol=1e-2)
    assert torch.allclose(st[:, 1], gs.square().sum(dim=(0, 2, 3)), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("xf", [1, 2], ids=["affine", "affine_silu"])
@pytest.mark.parametrize("c,hw,b", [(32, (16, 32), 2), (32, (48, 64), 2), (32, (16 * 17, 32), 3), (32, (16 * 4, 256), 1),
                                    (64, (8, 32), 2), (64, (24, 64), 2), (64, (8 * 9, 32), 3), (64, (8 * 5, 128), 1)])
def test_pipe_conv_vs_fp32_reference(c, hw, b, xf):
    """Both convs of Residual_Block (models/diffusion.py:46-53) through the software-pipelined kernel (csrc/conv_pipe.h): the
    MFMAs of tile t run from one halo buffer while the same wave transforms tile t + 1 into the other and drains the previous
    block.  Against fp32 torch on the same bf16-rounded operands: one tile (pipeline fill + drain only), several tiles per
    workgroup (all four borders, both halo buffers, the rolling prefetch two tiles ahead), more tiles than one workgroup takes
    (17 / 9 tile rows: a second, shorter workgroup per sample), full-width images (8 / 4 tiles per row), three samples; every
    pixel written; group statistics (taken before the bf16 rounding: 2^-9 / sqrt(N) relative to the stored values')."""
    import torch.nn.functional as F
    lib = _lib.load()
    dt = G.BF16
    h, w = hw
    dev = G.dev()
    x = (synth.gaussian(f"pipe.x{c}", (b, c, h, w)) * 1.2 + 0.2).bfloat16().float()
    wt = synth.gaussian(f"pipe.w{c}", (c, c, 3, 3)) / (9 * c) ** 0.5
    bias = synth.gaussian(f"pipe.b{c}", (c,)) * 0.3
    temb = synth.gaussian(f"pipe.t{c}", (b, c)) * 0.3
    scale = synth.gaussian(f"pipe.s{c}", (b, c)) * 0.3 + 1.0
    shift = synth.gaussian(f"pipe.h{c}", (b, c)) * 0.5
    xn = G.to_nhwc(x, dt)
    wf = torch.empty(9 * c * c, dtype=torch.bfloat16, device=dev)
    wt_d = wt.to(dev).contiguous()
    _lib.check(lib.ddimx_pack_conv_frag(_lib.ptr(wt_d), _lib.ptr(wf), c, c, _lib.stream()))
    y = torch.full_like(xn, float("nan"))
    nst = int(lib.ddimx_conv3x3_pipe_stats_floats(c, b, h, w))
    assert nst > 0 and nst % (32 * b) == 0
    stats = torch.full((nst,), float("nan"), device=dev)
    bias_d, temb_d, scale_d, shift_d = bias.to(dev), temb.to(dev), scale.to(dev), shift.to(dev)
    use_temb = xf == 2
    _lib.check(lib.ddimx_conv3x3_pipe_fwd(c, _lib.ptr(xn), _lib.ptr(wf), None if use_temb else _lib.ptr(bias_d),
                                          _lib.ptr(temb_d) if use_temb else None, c, _lib.ptr(scale_d), _lib.ptr(shift_d), xf,
                                          _lib.ptr(y), _lib.ptr(stats), b, h, w, _lib.stream()))
    torch.cuda.synchronize()
    got = G.from_nhwc(y, dt)
    assert torch.isfinite(got).all(), "a pixel was never written"
    yn = x * scale[:, :, None, None] + shift[:, :, None, None]
    if xf == 2:
        yn = F.silu(yn)
    yn = yn.bfloat16().float()  # the kernel rounds the transformed input to bf16 before the MFMAs
    add = temb[:, :, None, None] if use_temb else bias[None, :, None, None]
    want = F.silu(F.conv2d(yn, wt.bfloat16().float(), None, padding=1) + add)
    G.check_close(got, want, dt, f"pipe conv C={c} {hw} xf={xf}")
    # one 32-float slab per workgroup: 8 groups x (sum, sumsq), then zeros
    st = stats.cpu().view(b, -1, 32).double()
    assert torch.isfinite(st).all() and float(st[:, :, 16:].abs().max()) == 0.0
    st = st[:, :, :16].sum(1).view(b, 8, 2)
    gs = got.double().view(b, 8, c // 8, h, w)
    assert torch.allclose(st[:, :, 0], gs.sum(dim=(2, 3, 4)), rtol=1e-3, atol=0.5)
    assert torch.allclose(st[:, :, 1], gs.square().sum(dim=(2, 3, 4)), rtol=1e-3, atol=0.5)


@pytest.mark.parametrize("cin,cout,hw", [(32, 64, (32, 64)), (64, 96, (16, 64)), (96, 128, (16, 32)), (128, 192, (16, 32)), (192, 256, (8, 32))])
def test_wreg_downsample_vs_fp32_reference(cin, cout, hw):
    """Downsample = Conv2d(k4, s2, p1) + bias (models/diffusion.py:70-78) through the register-streamed-weights kernel, as the
    inference walk launches it: against fp32 torch on the same bf16-rounded operands, plus the statistics of the stored values.
    (ddimx_downsample_fwd with fragment-order weights handed over next to the LDS layout.)"""
    import torch.nn.functional as F
    lib = _lib.load()
    dt, b = G.BF16, 2
    h, w = hw
    dev = G.dev()
    x = (synth.gaussian(f"wdn.x{cin}", (b, cin, h, w)) * 1.2 + 0.1).bfloat16().float()
    wt = synth.gaussian(f"wdn.w{cin}", (cout, cin, 4, 4)) / (16 * cin) ** 0.5
    bias = synth.gaussian(f"wdn.b{cin}", (cout,)) * 0.3
    xn = G.to_nhwc(x, dt)
    wt_d, bias_d = wt.to(dev).contiguous(), bias.to(dev)
    wf = torch.empty(16 * cin * cout, dtype=torch.bfloat16, device=dev)
    _lib.check(lib.ddimx_pack_conv_frag_k(_lib.ptr(wt_d), _lib.ptr(wf), cout, cin, 16, _lib.stream()))
    y = torch.empty(b, h // 2, w // 2, cout, dtype=torch.bfloat16, device=dev)
    stats = torch.zeros(b * (h // 2) * (w // 2) * cout * 2 // 8 + 4096, device=dev)
    _lib.check(lib.ddimx_downsample_wreg_fwd(cin, cout, _lib.ptr(xn), _lib.ptr(wf), _lib.ptr(bias_d), _lib.ptr(y), _lib.ptr(stats), b, h, w,
                                             _lib.stream()))
    torch.cuda.synchronize()
    got = G.from_nhwc(y, dt)
    want = F.conv2d(x, wt.bfloat16().float(), bias, stride=2, padding=1)
    G.check_close(got, want, dt, f"wreg down {cin}->{cout} {hw}")
    st = stats.cpu()[: (stats.numel() // (cout * 2)) * cout * 2].view(-1, cout, 2).double().sum(0)
    gs = got.double()
    assert torch.allclose(st[:, 0], gs.sum(dim=(0, 2, 3)), rtol=1e-4, atol=1e-2)
    assert torch.allclose(st[:, 1], gs.square().sum(dim=(0, 2, 3)), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("cin,cout,hw", [(256, 192, (8, 16)), (192, 128, (8, 32)), (128, 96, (8, 64)), (96, 64, (8, 64)), (64, 32, (16, 64))])
def test_wreg_upsample_add_vs_fp32_reference(cin, cout, hw):
    """Upsample = ConvTranspose2d(k4, s2, p1) + bias, then the skip addition (models/diffusion.py:59-67,284) through the
    register-streamed-weights kernel (both row-parity classes, the two column parities as 2 * Cout virtual channels): against fp32
    torch on the same bf16-rounded operands, plus the statistics of the stored values."""
    import torch.nn.functional as F
    lib = _lib.load()
    dt, b = G.BF16, 2
    h, w = hw
    dev = G.dev()
    x = (synth.gaussian(f"wup.x{cin}", (b, cin, h, w)) * 1.1).bfloat16().float()
    skip = synth.gaussian(f"wup.s{cin}", (b, cout, 2 * h, 2 * w)).bfloat16().float()
    wt = synth.gaussian(f"wup.w{cin}", (cin, cout, 4, 4)) / (4 * cin) ** 0.5
    bias = synth.gaussian(f"wup.b{cin}", (cout,)) * 0.3
    xn, sn = G.to_nhwc(x, dt), G.to_nhwc(skip, dt)
    wp = G.pack_convT(wt, dt)                       # [2][6][2*cout][cin]
    wf = torch.empty_like(wp)
    per = 6 * 2 * cout * cin
    for a in range(2):
        _lib.check(lib.ddimx_pack_frag_from_taps(_lib.ptr(wp[a * per:]), _lib.ptr(wf[a * per:]), 6, 2 * cout, cin, _lib.stream()))
    b2 = torch.cat([bias, bias]).to(dev)
    y = torch.empty_like(sn)
    stats = torch.zeros(b * 4 * h * w * cout * 2 // 8 + 8192, device=dev)
    _lib.check(lib.ddimx_upsample_add_wreg_fwd(cin, cout, _lib.ptr(xn), _lib.ptr(wf), _lib.ptr(b2), _lib.ptr(sn), _lib.ptr(y), _lib.ptr(stats),
                                               b, h, w, _lib.stream()))
    torch.cuda.synchronize()
    got = G.from_nhwc(y, dt)
    want = F.conv_transpose2d(x, wt.bfloat16().float(), bias, stride=2, padding=1) + skip
    G.check_close(got, want, dt, f"wreg up {cin}->{cout} {hw}")
    # per-channel statistics come in 2 * cout virtual channels (the two column parities): fold them
    st = stats.cpu()[: (stats.numel() // (4 * cout)) * 4 * cout].view(-1, 2, cout, 2).double().sum(dim=(0, 1))
    gs = got.double()
    assert torch.allclose(st[:, 0], gs.sum(dim=(0, 2, 3)), rtol=1e-4, atol=1e-2)
    assert torch.allclose(st[:, 1], gs.square().sum(dim=(0, 2, 3)), rtol=1e-4, atol=1e-2)
