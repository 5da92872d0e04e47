"""Gradients w.r.t. the U-Net input (ddimx_unet_bwd_ex, ddimx_conv_in_bwd_data) and the data-only backward.

The reference gets d eps / d x from plain autograd (models/diffusion.py:237-294; x feeds only the input conv, :255-256).  Here:
the whole-network input gradient in train and eval mode against autograd through the CPU oracle (gates relative to the reference
tensor's RMS, the parameter-gradient yardsticks of test_gpu_train.py), the data-only backward against the full one bit for bit,
the input conv's data-gradient kernel on exact operands, and that nothing the training step computed before has moved."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from ddim_audio_amd import _lib, losses, synth
from ddim_audio_amd.schedule import make_schedule
from oracle import ref_cpu
import exact_util as X
import gpu_util as G
import model_harness as MH
from model_harness import MODES, MODE_IDS

pytestmark = pytest.mark.gpu


# ---- 1. whole network, train mode: x0.grad through noise_estimation_loss vs autograd through the oracle -------------------------
CASES = [("tiny", (2, 2, 16, 32), [3, 870]), ("audio", (2, 2, 32, 256), [0, 999]), ("tiny", (3, 2, 24, 32), [0, 999, 412]),
         ("tiny", (2, 2, 256, 32), [77, 940])]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name,shape,tt", CASES, ids=["tiny", "audio", "ragged", "tall"])
def test_train_mode_input_grad_vs_oracle(mode, name, shape, tt):
    dtype_str, dt = mode
    cfg, m = MH.build(name, dtype_str, 5, mode=None, dropout=0.0)
    m.train()
    _, alphas = make_schedule(cfg.diffusion)
    x0, e, t = synth.gaussian("igrad.x0", shape), synth.gaussian("igrad.e", shape), torch.tensor(tt)
    xg = x0.cuda().requires_grad_(True)
    loss = losses.noise_estimation_loss(m, xg, t.cuda(), e.cuda(), alphas.cuda())
    loss.backward()
    assert xg.grad is not None
    live, ocfg = MH.oracle(m, name)
    xr = x0.clone().requires_grad_(True)
    want = ref_cpu.noise_estimation_loss(lambda a, b: ref_cpu.model_forward(live, ocfg, a, b), xr, t, e, alphas)
    want.backward()
    mx, er = MH.gate(xg.grad, xr.grad, dt, f"x0.grad {name} {shape}")
    print(f"[input grad {name} {shape} {'f32' if dt == G.F32 else 'bf16'}] max {mx:.3e} rms err {er:.3e} x rms")


# ---- 2. eval mode: vector-Jacobian product w.r.t. the input ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_eval_mode_vjp_vs_oracle(mode):
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 7, mode=None, dropout=0.1)
    m.eval()
    shape = (3, 2, 24, 32)
    x, v, t = synth.gaussian("evjp.x", shape), synth.gaussian("evjp.v", shape), torch.tensor([5, 999, 400])
    calls = getattr(m, "_dropout_calls", 0)
    xg = x.cuda().requires_grad_(True)
    eps = m(xg, t.cuda())
    assert eps.grad_fn is not None
    (g1,) = torch.autograd.grad(eps, xg, v.cuda())
    (g2,) = torch.autograd.grad(m(xg, t.cuda()), xg, v.cuda())
    assert torch.equal(g1, g2), "two eval-mode VJPs differ"
    assert getattr(m, "_dropout_calls", 0) == calls, "the eval-mode input gradient advanced the dropout stream"
    live, ocfg = MH.oracle(m, "tiny")
    xr = x.clone().requires_grad_(True)
    want_eps = ref_cpu.model_forward(live, ocfg, xr, t)
    (want,) = torch.autograd.grad(want_eps, xr, v)
    MH.gate(g1, want, dt, "eval VJP")
    MH.gate(eps, want_eps, dt, "eval eps (tape-keeping forward)")
    # every other eval call keeps the inference path
    with torch.no_grad():
        plain = m(x.cuda(), t.cuda())
    assert m(x.cuda(), t.cuda()).grad_fn is None
    assert torch.equal(m(x.cuda(), t.cuda()), plain)
    if dt == G.F32:
        G.check_close(eps.detach().cpu(), plain.cpu(), dt, "eval eps, tape vs inference")
    # first order only
    with pytest.raises(RuntimeError):
        (gg,) = torch.autograd.grad(m(xg, t.cuda()), xg, v.cuda(), create_graph=True)
        gg.sum().backward()
    assert getattr(m, "_dropout_calls", 0) == calls


# ---- 3. frozen parameters: the data-only backward --------------------------------------------------------------------------------
@pytest.mark.parametrize("fork", [True, False], ids=["fork", "one_stream"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_frozen_parameters_take_the_data_only_backward(mode, fork):
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 9, mode=None, dropout=0.1)
    m.train()
    m.bwd_fork = fork
    shape = (3, 2, 24, 32)
    x, v, t = synth.gaussian("frz.x", shape).cuda(), synth.gaussian("frz.v", shape).cuda(), torch.tensor([1, 500, 998]).cuda()

    def run():
        m._dropout_calls = 41  # the same dropout masks for both runs
        xg = x.clone().requires_grad_(True)
        eps = m(xg, t)
        m._train_ws.fill_(0xFF)  # the backward takes nothing from the forward's scratch
        eps.backward(v)
        torch.cuda.synchronize()
        return xg.grad

    full = run()
    assert all(p.grad is not None for p in m.parameters())
    flat = m._flat_grad
    snap = flat.clone()
    m.zero_grad(set_to_none=True)
    m.requires_grad_(False)
    synced = []
    m.grad_sync = lambda buf: synced.append(buf)
    got = run()
    assert torch.equal(got, full), "data-only x.grad differs from the full backward's"
    assert all(p.grad is None for p in m.parameters())
    assert m._flat_grad is flat and torch.equal(flat.view(torch.int32), snap.view(torch.int32)), "the flat gradient buffer was touched"
    assert not synced, "data-only backward invoked grad_sync"


# ---- 4. the kernel: exact operands -------------------------------------------------------------------------------------------------
def _conv_in_bwd_data(dt, dy, wp, B, cin, c0, H, W):
    lib = _lib.load()
    d_x = torch.full((B, cin, H, W), float("nan"), device=G.dev())
    _lib.check(lib.ddimx_conv_in_bwd_data(dt, _lib.ptr(dy), _lib.ptr(wp), _lib.ptr(d_x), B, cin, c0, H, W, _lib.stream()))
    torch.cuda.synchronize()
    return d_x.cpu()


@pytest.mark.parametrize("dt", [G.F32, G.BF16], ids=MODE_IDS)
@pytest.mark.parametrize("B,H,W,cin,c0", [(2, 16, 32, 2, 32), (3, 24, 32, 2, 32), (1, 37, 256, 2, 32), (2, 1024, 256, 2, 32),
                                          (2, 19, 40, 1, 64), (1, 9, 12, 3, 32)])
def test_conv_in_bwd_data_exact(dt, B, H, W, cin, c0):
    """d_x = the fp64 value exactly (criterion E, fp32 output): 9 * c0 products of k/16 and k/32 (|k| <= 15) sum exactly in fp32
    in any order.  The last two shapes take the generic kernel; the others the tiled one, ragged in H (37) and W."""
    tag = f"cinbd.{dt}.{B}.{H}.{W}.{cin}.{c0}"
    assert X.budget_bits(9 * c0, 15 / 16, 4, 15 / 32, 5) < 24
    dy64 = X.dyadic(tag + ".dy", (B, H, W, c0), 15, 4)
    w64 = X.dyadic(tag + ".w", (c0, cin, 3, 3), 15, 5)
    dy = dy64.to(G.TORCH_DT[dt]).to(G.dev()).contiguous()
    assert torch.equal(dy.double().cpu(), dy64)
    wp = G.pack_conv_dgrad(w64.float(), G.F32)  # [9][cin][c0], transposed and flipped
    exact = F.conv_transpose2d(dy64.permute(0, 3, 1, 2), w64, padding=1)  # d(input) of Conv2d(cin -> c0, k3 p1)
    got = _conv_in_bwd_data(dt, dy, wp, B, cin, c0, H, W)
    X.check(got, exact, G.F32, f"conv_in_bwd_data {tag}", layout="nchw")
    # negative control: one flipped tap zeroed is caught
    bad = wp.clone().view(9, cin, c0)
    bad[2].zero_()
    assert X.mismatches(_conv_in_bwd_data(dt, dy, bad, B, cin, c0, H, W), exact, G.F32).any()


# ---- 5. nothing the training step computed before has moved ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_input_grad_leaves_the_training_step_unchanged(mode):
    dtype_str, dt = mode
    cfg, m = MH.build("audio", dtype_str, 11, mode=None, dropout=0.1)  # the full parameter set
    m.train()
    _, alphas = make_schedule(cfg.diffusion)
    shape = (2, 2, 32, 256)
    x0, e, t = synth.gaussian("keep.x0", shape).cuda(), synth.gaussian("keep.e", shape).cuda(), torch.tensor([2, 999]).cuda()

    def step(with_x):
        m._dropout_calls = 7
        eps = []
        xin = x0.clone().requires_grad_(with_x)
        loss = losses.noise_estimation_loss(lambda a, b: eps.append(m(a, b)) or eps[-1], xin, t, e, alphas.cuda())
        loss.backward()
        out = (loss.detach().clone(), eps[0].detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}, xin.grad)
        m.zero_grad(set_to_none=True)
        return out

    loss_a, eps_a, grads_a, xg_a = step(False)
    loss_b, eps_b, grads_b, xg_b = step(True)
    assert xg_a is None and xg_b is not None and torch.isfinite(xg_b).all()
    assert torch.equal(loss_a, loss_b) and torch.equal(eps_a, eps_b)
    assert len(grads_a) == 388
    for n in grads_a:
        assert torch.equal(grads_a[n], grads_b[n]), n


def _abi_args(m, node, d_eps):
    tb = _lib.DdimxTables(node.tables[0].data_ptr(), node.tables[1].data_ptr(), node.tables[2].data_ptr())
    ws = m._train_ws
    b, t_len = node.x.size(0), node.x.size(2)
    return tb, [m._handle, _lib.ptr(node.packed), _lib.ptr(node.packed_bwd), ctypes.byref(tb), _lib.ptr(ws), ws.numel(), _lib.ptr(node.tape),
                node.tape.numel(), _lib.ptr(node.x), _lib.ptr(node.t), _lib.ptr(d_eps)], (b, t_len, node.p, node.seed)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_bwd_ex_matches_forked_and_validates_first(mode):
    """ddimx_unet_bwd_ex(d_x, flags = 0) writes the flat gradient buffer of ddimx_unet_bwd_forked bit for bit; its d_x is the data-only
    call's; bad flag / null combinations are refused."""
    dtype_str, dt = mode
    cfg, m = MH.build("tiny", dtype_str, 13, mode=None, dropout=0.0)
    m.train()
    lib = m._ensure_handle()
    shape = (2, cfg.model.channels, 64, cfg.model.f_size)
    x, t = synth.gaussian("abi.x", shape).cuda(), torch.tensor([4, 777]).cuda()
    d_eps = synth.gaussian("abi.v", shape).cuda()
    eps = m(x, t)
    node = eps.grad_fn  # the autograd node keeps the tape and the buffers of this forward
    total = int(lib.ddimx_grad_floats(m._handle))
    tb, head, tail = _abi_args(m, node, d_eps)
    s = _lib.stream()
    flat_a = torch.full((total,), float("nan"), device="cuda")
    flat_b = torch.full((total,), float("nan"), device="cuda")
    d_x = torch.full(shape, float("nan"), device="cuda")
    d_x2 = torch.full(shape, float("nan"), device="cuda")
    _lib.check(lib.ddimx_unet_bwd_forked(*head, _lib.ptr(flat_a), *tail, None, 0, s, None, None, 0))
    _lib.check(lib.ddimx_unet_bwd_ex(*head, _lib.ptr(flat_b), *tail, None, 0, s, None, None, 0, _lib.ptr(d_x), 0))
    _lib.check(lib.ddimx_unet_bwd_ex(*head, None, *tail, None, 0, s, None, None, 0, _lib.ptr(d_x2), _lib.DDIMX_BWD_DATA_ONLY))
    torch.cuda.synchronize()
    assert torch.equal(flat_a.view(torch.int32), flat_b.view(torch.int32))
    assert torch.isfinite(d_x).all() and torch.equal(d_x, d_x2)
    ev = (ctypes.c_void_p * 3)()
    for args, msg in (((None, 0, s, None, None, 0, _lib.ptr(d_x), 2), "unknown flags"),
                      ((ev, 3, s, None, None, 0, _lib.ptr(d_x), _lib.DDIMX_BWD_DATA_ONLY), "gradient buckets"),
                      ((None, 0, s, None, None, 0, None, _lib.DDIMX_BWD_DATA_ONLY), "needs d_x")):
        assert lib.ddimx_unet_bwd_ex(*head, None, *tail, *args) != 0
        assert msg in lib.ddimx_last_error().decode()
    assert lib.ddimx_unet_bwd_ex(*head, None, *tail, None, 0, s, None, None, 0, _lib.ptr(d_x), 0) != 0  # grads null, full mode
    eps.backward(d_eps)  # the node still owns its tape: the ordinary backward runs on
    torch.cuda.synchronize()
