"""GPU parity tests of the training path: HIP forward-with-tape and backward kernels (through the C ABI) against
autograd over the CPU oracle (itself pinned to the reference's gradients by tests/golden/train.npz).
Gates: fp32 mode max|d| <= 1e-4 * std (x4 for parameter gradients, which are long fp32 sums); bf16 mode
rms <= 2e-2 * std, max <= 1.5e-1 * std -- the same yardsticks as the forward."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ddim_audio_amd as D
from ddim_audio_amd import _lib, configs, losses, synth
from ddim_audio_amd.schedule import make_schedule
from oracle import ref_cpu
from conftest import rel_err
import fnet_kernel_ref as R
import gpu_util as G
import model_harness as MH
from model_harness import MODES

pytestmark = pytest.mark.gpu
DTS = [G.F32, G.BF16]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c,hw,b", [(32, (40, 72), 3), (64, (24, 40), 2), (96, (17, 33), 2), (128, (16, 24), 2),
                                    (192, (9, 20), 1), (256, (20, 9), 2),
                                    (32, (200, 48), 7)])  # 75 tiles per sample, 525 in all: workgroups walk 2 tiles and straddle samples
def test_resblock_backward(dt, c, hw, b):
    p = f"rbt{c}."
    sd = MH.rb_sd(p, c)
    x = synth.gaussian(p + "x", (b, c, *hw)) * 1.5 + 0.3
    temb = synth.gaussian(p + "temb", (b, c)) * 0.5
    dy = synth.gaussian(p + "dy", (b, c, *hw))
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr, tr = x.clone().requires_grad_(True), temb.clone().requires_grad_(True)
    yr = ref_cpu.residual_block(leaf, p, xr, tr)
    yr.backward(dy)
    y, dx, grads, dtemb = G.resblock_train(sd, p, x, temb, dy, dt)
    G.check_close(y, yr.detach(), dt, f"train fwd C={c}")
    G.check_close(dx, xr.grad, dt, f"dx C={c}")
    G.check_close(dtemb, tr.grad, dt, f"dtemb C={c}", scale=4.0)
    for n, gv in grads.items():
        G.check_close(gv, leaf[p + n].grad, dt, f"d {n} C={c}", scale=4.0)


# ---- whole network: loss.backward() through the reference-shaped Python API vs the reference's own gradients ----
def _train_model(name, dtype_str, seed, dropout=0.0):
    return MH.build(name, dtype_str, seed, mode="train", dropout=dropout, optimizer="Adam")


@pytest.mark.parametrize("mode", MODES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name,shape,seed", [("tiny", (2, 2, 16, 32), 3), ("audio", (2, 2, 32, 256), 0)])
def test_model_backward_golden(golden, mode, name, shape, seed):
    """loss + all 388 parameter gradients against the digest the real reference produced (tests/golden/train.npz)."""
    dtype_str, dt = mode
    g = golden("train")
    cfg, m = _train_model(name, dtype_str, seed)
    _, alphas = make_schedule(cfg.diffusion)
    x0, e = synth.gaussian(f"train.{name}.x0", shape).cuda(), synth.gaussian(f"train.{name}.e", shape).cuda()
    t = torch.from_numpy(g[f"{name}_t"]).cuda()
    loss = losses.noise_estimation_loss(m, x0, t, e, alphas.cuda())
    loss.backward()
    ref_loss = float(g[f"{name}_loss"])
    assert abs(float(loss) - ref_loss) <= (1e-5 if dt == G.F32 else 2e-3) * ref_loss
    names, norms = [str(n) for n in g[f"{name}_names"]], g[f"{name}_gnorms"]
    total = float(np.sqrt((norms ** 2).sum()))
    params = dict(m.named_parameters())
    assert list(params.keys()) == names
    worst = 0.0
    got_total = 0.0
    for pname, ref_norm in zip(names, norms):
        grad = params[pname].grad
        assert grad is not None and torch.isfinite(grad).all(), pname
        flat = grad.detach().cpu().reshape(-1)
        got_total += float(flat.double().square().sum())
        ref = g[f"{name}_g::{pname}"]
        stride = max(1, flat.numel() // 256)
        got = flat[::stride][:256].numpy()
        # per-tensor gate: relative to the tensor's own RMS gradient (floor: a 1e-4 share of the global norm)
        rms_ref = ref_norm / np.sqrt(flat.numel())
        scale = max(rms_ref, 1e-4 * total / np.sqrt(flat.numel()))
        err = float(np.abs(got - ref).max()) / scale
        worst = max(worst, err)
        tol = 2e-3 if dt == G.F32 else 0.5
        assert err <= tol, f"{pname}: max err {err:.3e} x rms (tol {tol})"
        nerr = abs(float(flat.double().square().sum()) ** 0.5 - ref_norm) / max(ref_norm, 1e-4 * total)
        assert nerr <= (5e-4 if dt == G.F32 else 6e-2), f"{pname}: norm err {nerr:.3e}"
    print(f"[backward golden {name} {'f32' if dt == G.F32 else 'bf16'}] worst element {worst:.3e} x rms, global norm rel err "
          f"{abs(got_total ** 0.5 - total) / total:.2e}")
    assert abs(got_total ** 0.5 - total) <= (1e-4 if dt == G.F32 else 2e-2) * total


def test_reference_runner_sequence_golden(golden):
    """The literal statement sequence of the reference's Diffusion.train_step (runners/diffusion.py:130-173) over the drop-in
    symbols -- loss_registry, zero_grad, backward, torch.nn.utils.clip_grad_norm_, optimizer / scheduler steps, EMAHelper --
    reproduces the reference's first optimisation step."""
    from ddim_audio_amd import train
    from ddim_audio_amd.dropin.functions import get_optimizer, get_scheduler
    from ddim_audio_amd.dropin.functions.losses import loss_registry
    from ddim_audio_amd.dropin.models.ema import EMAHelper
    g = golden("train")
    cfg, model = _train_model("tiny", "torch.cuda.FloatTensor", 3)
    optimizers, schedulers = {}, {}
    for name, p_opt in train.classify_group(cfg.optimization.optimizer, model).items():
        optimizers[name] = get_optimizer(p_opt.config, p_opt.params)
        schedulers[name] = get_scheduler(p_opt.config, optimizers[name])
    grad_group = train.classify_group(cfg.optimization.grad_norm, model)
    ema_helper = EMAHelper(mu=cfg.model.ema_rate)
    ema_helper.register(model)
    _, alphas = make_schedule(cfg.diffusion)
    x = synth.gaussian("train.tiny.x0", (2, 2, 16, 32)).cuda()
    e = synth.gaussian("train.tiny.e", (2, 2, 16, 32)).cuda()
    t = torch.from_numpy(g["tiny_t"]).cuda()
    model.train()
    loss = loss_registry[cfg.model.type](model, x, t, e, alphas.cuda())
    assert abs(loss.item() - float(g["step0_loss"])) < 1e-4 * float(g["step0_loss"])
    for optimizer in optimizers.values():
        optimizer.zero_grad()
    loss.backward()
    for name, p_opt in grad_group.items():
        norm = torch.nn.utils.clip_grad_norm_(p_opt.params, p_opt.config.grad_clip)
        assert abs(float(norm) - float(g[f"step0_norm_{name}"])) < 1e-3 * float(norm)
    for optimizer in optimizers.values():
        optimizer.step()
    for scheduler in schedulers.values():
        scheduler.step()
    ema_helper.update(model)
    states = [model.state_dict(), optimizer.state_dict(), 0, 1, ema_helper.state_dict()]
    assert len(states[0]) == 1 + len(list(model.parameters())) and "state" in states[1]
    for n, p in model.named_parameters():
        stride = max(1, p.numel() // 64)
        ref = g[f"step0_p::{n}"]
        lr = 5e-4 if n.startswith("transformer.") else 3e-4
        assert np.abs(p.detach().cpu().reshape(-1)[::stride][:64].numpy() - ref).max() <= 0.02 * lr + 1e-6 * np.abs(ref).max(), n
        sh = ema_helper.shadow[n].cpu().reshape(-1)[::stride][:64].numpy()
        assert np.abs(sh - g[f"step0_ema::{n}"]).max() <= 1e-5 * np.abs(ref).max() + 1e-7, n
    # the next forward must see the updated weights without any explicit invalidation
    with torch.no_grad():
        y1 = model.eval()(x, t)
        fresh = D.Model(cfg)
        fresh.load_state_dict(model.state_dict())
        y2 = fresh.eval()(x, t)
    assert torch.equal(y1, y2)


def test_training_steps_golden(golden):
    """Two full optimisation steps (loss, backward, clip, fused Adam/AdamW, LambdaLR, EMA) against the reference's own
    train_step tail (fp32 mode).  Adam divides by sqrt(v) + eps, which amplifies gradient noise where |g| ~ eps; the gate
    is therefore on the parameter UPDATE relative to lr."""
    from ddim_audio_amd import train
    g = golden("train")
    cfg, m = _train_model("tiny", "torch.cuda.FloatTensor", 3)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    state = train.TrainingState(cfg, m)
    assert list(state.optimizers.keys()) == [str(s) for s in g["step_groups"]]
    _, alphas = make_schedule(cfg.diffusion)
    alphas = alphas.cuda()
    shape = (2, 2, 16, 32)
    for it in range(2):
        sfx = f".{it}" if it else ""
        x0, e = synth.gaussian(f"train.tiny.x0{sfx}", shape).cuda(), synth.gaussian(f"train.tiny.e{sfx}", shape).cuda()
        t = torch.tensor([5, 994]) if it else torch.from_numpy(g["tiny_t"])
        loss, norms = train.train_step(m, x0, state, alphas, e=e, t=t)
        assert abs(float(loss) - float(g[f"step{it}_loss"])) < 1e-4 * float(g[f"step{it}_loss"])
        for k, v in norms.items():
            assert abs(float(v) - float(g[f"step{it}_norm_{k}"])) < 1e-3 * float(v)
        bad = []
        for n, p in m.named_parameters():
            stride = max(1, p.numel() // 64)
            got = p.detach().cpu().reshape(-1)[::stride][:64].numpy()
            ref = g[f"step{it}_p::{n}"]
            lr = 5e-4 if n.startswith("transformer.") else 3e-4
            # updates are at most ~lr per step (times the warm-up factor); allow 2 % of lr per step taken
            if np.abs(got - ref).max() > 0.02 * lr * (it + 1) + 1e-6 * np.abs(ref).max():
                bad.append((n, float(np.abs(got - ref).max())))
            sh = state.ema_helper.shadow[n].cpu().reshape(-1)[::stride][:64].numpy()
            assert np.abs(sh - g[f"step{it}_ema::{n}"]).max() <= 1e-5 * np.abs(ref).max() + 1e-7, n
        assert not bad, bad[:5]
    assert np.allclose([o.param_groups[0]["lr"] for o in state.optimizers.values()], g["step_lrs"], rtol=1e-6)
    moved = sum(int((p.detach() != before[n]).any()) for n, p in m.named_parameters())
    assert moved == len(before)


def test_dropout_training_mode():
    """hidden_dropout_prob > 0 (the reference's train mode): masks are a function of (seed, call counter), the backward
    regenerates them -- checked with a directional finite difference of the loss at a fixed mask (fp32 mode)."""
    cfg, m = _train_model("tiny", "torch.cuda.FloatTensor", 3, dropout=0.1)
    _, alphas = make_schedule(cfg.diffusion)
    alphas = alphas.cuda()
    shape = (2, 2, 16, 32)
    x0, e = synth.gaussian("train.tiny.x0", shape).cuda(), synth.gaussian("train.tiny.e", shape).cuda()
    t = torch.tensor([123, 876]).cuda()

    def loss_at(call):
        m._dropout_calls = call
        return losses.noise_estimation_loss(m, x0, t, e, alphas)

    l1 = loss_at(7)
    l1.backward()
    g1 = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    l1b = loss_at(7)
    l2 = loss_at(8)
    assert float(l1) == float(l1b) and float(l1) != float(l2)       # same seed -> same mask; next call -> another mask
    m.eval()
    with torch.no_grad():
        l_eval = losses.noise_estimation_loss(m, x0, t, e, alphas)
    m.train()
    assert abs(float(l1) - float(l_eval)) > 1e-6 * float(l_eval)     # dropout is really active in train mode
    # directional derivative along a random direction restricted to the transformer (where dropout acts) + one conv
    names = [n for n in g1 if n.startswith("transformer.")] + ["down_modules.1.0.conv.0.weight"]
    params = dict(m.named_parameters())
    dirs = {n: synth.gaussian("dd." + n, tuple(params[n].shape)).cuda() for n in names}
    want = sum(float((g1[n].double() * dirs[n].double()).sum()) for n in names)
    h = 1e-3
    vals = []
    for sgn in (+1, -1):
        with torch.no_grad():
            for n in names:
                params[n].add_(dirs[n], alpha=sgn * h)
        m.invalidate()
        vals.append(float(loss_at(7).detach()))
        with torch.no_grad():
            for n in names:
                params[n].add_(dirs[n], alpha=-sgn * h)
    m.invalidate()
    fd = (vals[0] - vals[1]) / (2 * h)
    assert abs(fd - want) <= 2e-2 * abs(want) + 1e-3, (fd, want)


@pytest.mark.parametrize("mode", MODES, ids=["f32", "bf16"])
def test_model_backward_ragged_shape_vs_oracle(mode):
    """Odd batch and a T whose bottleneck length is not a power of two (ragged conv tiles, ragged weight-gradient tiles,
    non-power-of-two DFT): loss and gradients against autograd through the CPU oracle."""
    _ragged_case(mode, (3, 2, 24, 32), [0, 999, 412])


@pytest.mark.parametrize("mode", MODES, ids=["f32", "bf16"])
def test_model_backward_tall_shape_vs_oracle(mode):
    """T = 256: several row chunks / strips in the edge-conv gradient kernels, multi-tile persistent conv workgroups."""
    _ragged_case(mode, (2, 2, 256, 32), [77, 940])


def _ragged_case(mode, shape, tt):
    MH.backward_case(mode, shape, tt, build_model=_train_model, loss=losses.noise_estimation_loss, ref_loss=ref_cpu.noise_estimation_loss)


def test_training_reduces_the_loss_and_state_dicts_roundtrip():
    """A few optimisation steps on one fixed batch lower the loss (bf16 mode, dropout on); optimizer / EMA state survives a
    state_dict round trip in the reference's checkpoint layout."""
    from ddim_audio_amd import train
    cfg, m = _train_model("tiny", "torch.cuda.BFloat16Tensor", 11, dropout=0.1)
    cfg.optimization.optimizer.default.warmup = 2     # reach the full learning rate within the test
    cfg.optimization.optimizer.transformer.warmup = 2
    state = train.TrainingState(cfg, m)
    _, alphas = make_schedule(cfg.diffusion)
    alphas = alphas.cuda()
    x = synth.gaussian("fit.x", (4, 2, 32, 32)).cuda()
    e = synth.gaussian("fit.e", (4, 2, 32, 32)).cuda()
    t = torch.tensor([10, 500, 989, 250])
    losses_seen = [float(train.train_step(m, x, state, alphas, e=e, t=t)[0]) for _ in range(12)]
    assert all(np.isfinite(losses_seen)) and losses_seen[-1] < 0.9 * losses_seen[0], losses_seen
    sd = {k: o.state_dict() for k, o in state.optimizers.items()}
    for k, o in state.optimizers.items():
        o.load_state_dict(sd[k])
    loss_after, _ = train.train_step(m, x, state, alphas, e=e, t=t)
    assert np.isfinite(float(loss_after))


# ---- backward twins of the remaining per-op forwards ("_bwd twin of each forward op") ---------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin,cout,hw,b", [(32, 64, (36, 44), 2), (96, 128, (18, 22), 2), (192, 256, (12, 20), 1)])
def test_downsample_upsample_backward_vs_oracle(dt, cin, cout, hw, b):
    """ddimx_downsample_bwd / ddimx_upsample_add_bwd against autograd through the oracle's Downsample / Upsample
    (models/diffusion.py:59-78): input gradients (incl. the accumulated skip gradient), weight and bias gradients."""
    lib = _lib.load()
    tdt = G.TORCH_DT[dt]
    sd = synth.fill_state_dict({"d.conv.weight": torch.empty(cout, cin, 4, 4), "d.conv.bias": torch.empty(cout),
                                "u.conv.weight": torch.empty(cout, cin, 4, 4), "u.conv.bias": torch.empty(cin)})
    h, w = hw
    # ---- Downsample
    x = synth.gaussian(f"dbw{cin}.x", (b, cin, h, w))
    dy = synth.gaussian(f"dbw{cin}.dy", (b, cout, h // 2, w // 2))
    extra = synth.gaussian(f"dbw{cin}.extra", (b, cin, h, w)) * 0.5
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    ref_cpu.downsample(leaf, "d.", xr).backward(dy)
    xn, dyn, exn = G.to_nhwc(x, dt), G.to_nhwc(dy, dt), G.to_nhwc(extra, dt)
    dxn = torch.empty_like(xn)
    wdg = G.g(sd["d.conv.weight"])
    wd_dgrad = torch.empty(2 * 6 * 2 * cin * cout, dtype=tdt, device=G.dev())
    _lib.check(lib.ddimx_pack_convT(dt, _lib.ptr(wdg), _lib.ptr(wd_dgrad), cout, cin, _lib.stream()))
    d_w, d_b = torch.full((cout, cin, 4, 4), float("nan"), device=G.dev()), torch.full((cout,), float("nan"), device=G.dev())
    ws = torch.empty(int(lib.ddimx_downup_bwd_workspace_bytes(dt, cout, cin, b, h // 2, w // 2)), dtype=torch.uint8, device=G.dev())
    _lib.check(lib.ddimx_downsample_bwd(dt, cin, cout, _lib.ptr(xn), _lib.ptr(dyn), _lib.ptr(wd_dgrad), _lib.ptr(exn), _lib.ptr(dxn),
                                        _lib.ptr(d_w), _lib.ptr(d_b), _lib.ptr(ws), b, h, w, _lib.stream()))
    ex_r = G.from_nhwc(exn, dt)
    G.check_close(G.from_nhwc(dxn, dt), xr.grad + ex_r, dt, f"downsample dx {cin}->{cout}")
    G.check_close(d_w.cpu(), leaf["d.conv.weight"].grad, dt, "downsample dW", scale=4.0)
    G.check_close(d_b.cpu(), leaf["d.conv.bias"].grad, dt, "downsample db", scale=4.0)
    # ---- Upsample (+ skip add: the skip's gradient is dy itself)
    xu = synth.gaussian(f"ubw{cout}.x", (b, cout, h // 2, w // 2))
    dyu = synth.gaussian(f"ubw{cout}.dy", (b, cin, h, w))
    xur = xu.clone().requires_grad_(True)
    ref_cpu.upsample(leaf, "u.", xur).backward(dyu)
    xun, dyun = G.to_nhwc(xu, dt), G.to_nhwc(dyu, dt)
    dxun = torch.empty_like(xun)
    wu_dgrad = G.pack_conv(sd["u.conv.weight"], dt)  # [O = cout(Cin of the upsample)][I = cin][4][4] read as a Conv2d weight
    du_w, du_b = torch.full((cout, cin, 4, 4), float("nan"), device=G.dev()), torch.full((cin,), float("nan"), device=G.dev())
    ws = torch.empty(int(lib.ddimx_downup_bwd_workspace_bytes(dt, cout, cin, b, h // 2, w // 2)), dtype=torch.uint8, device=G.dev())
    _lib.check(lib.ddimx_upsample_add_bwd(dt, cout, cin, _lib.ptr(xun), _lib.ptr(dyun), _lib.ptr(wu_dgrad), _lib.ptr(dxun), _lib.ptr(du_w),
                                          _lib.ptr(du_b), _lib.ptr(ws), b, h // 2, w // 2, _lib.stream()))
    G.check_close(G.from_nhwc(dxun, dt), xur.grad, dt, f"upsample dx {cout}->{cin}")
    G.check_close(du_w.cpu(), leaf["u.conv.weight"].grad, dt, "upsample dW", scale=4.0)
    G.check_close(du_b.cpu(), leaf["u.conv.bias"].grad, dt, "upsample db", scale=4.0)


@pytest.mark.parametrize("dt", DTS)
def test_edge_conv_backward_vs_oracle(dt):
    """ddimx_conv_in_bwd / ddimx_conv_out_bwd against autograd of Conv2d(2->32) and Conv2d(32->2) on `x + hidden[0]`
    (models/diffusion.py:189-208,283-292)."""
    lib = _lib.load()
    b, h, w, c0, cio = 2, 40, 256, 32, 2
    sd = synth.fill_state_dict({"ci.weight": torch.empty(c0, cio, 3, 3), "ci.bias": torch.empty(c0),
                                "co.weight": torch.empty(cio, c0, 3, 3), "co.bias": torch.empty(cio)})
    x = synth.gaussian("ebw.x", (b, cio, h, w))
    dy = synth.gaussian("ebw.dy", (b, c0, h, w))
    wr, br = sd["ci.weight"].clone().requires_grad_(True), sd["ci.bias"].clone().requires_grad_(True)
    dyn = G.to_nhwc(dy, dt)
    torch.nn.functional.conv2d(x, wr, br, padding=1).backward(G.from_nhwc(dyn, dt))
    part = torch.empty(int(lib.ddimx_edge_bwd_workspace_floats(dt, b, c0, cio, h, w)), device=G.dev())
    d_w, d_b = torch.full((c0, cio, 3, 3), float("nan"), device=G.dev()), torch.full((c0,), float("nan"), device=G.dev())
    xg = G.g(x)
    _lib.check(lib.ddimx_conv_in_bwd(dt, _lib.ptr(dyn), _lib.ptr(xg), _lib.ptr(part), _lib.ptr(d_w), _lib.ptr(d_b), b, cio, c0, h, w, _lib.stream()))
    G.check_close(d_w.cpu(), wr.grad, G.F32, "conv_in dW", scale=4.0)
    G.check_close(d_b.cpu(), br.grad, G.F32, "conv_in db", scale=4.0)
    # output conv
    a, s2 = synth.gaussian("ebw.a", (b, c0, h, w)), synth.gaussian("ebw.s", (b, c0, h, w)) * 0.7
    d_eps = synth.gaussian("ebw.de", (b, cio, h, w))
    an, sn = G.to_nhwc(a, dt), G.to_nhwc(s2, dt)
    ssum = (G.from_nhwc(an, dt) + G.from_nhwc(sn, dt)).requires_grad_(True)
    wo, bo = sd["co.weight"].clone().requires_grad_(True), sd["co.bias"].clone().requires_grad_(True)
    torch.nn.functional.conv2d(ssum, wo, bo, padding=1).backward(d_eps)
    wp = G.pack_conv(sd["co.weight"], G.F32)
    dsn = torch.empty_like(an)
    d_wo, d_bo = torch.full((cio, c0, 3, 3), float("nan"), device=G.dev()), torch.full((cio,), float("nan"), device=G.dev())
    deg = G.g(d_eps)
    _lib.check(lib.ddimx_conv_out_bwd(dt, _lib.ptr(deg), _lib.ptr(an), _lib.ptr(sn), _lib.ptr(wp), _lib.ptr(dsn), _lib.ptr(part), _lib.ptr(d_wo),
                                      _lib.ptr(d_bo), b, c0, cio, h, w, _lib.stream()))
    G.check_close(G.from_nhwc(dsn, dt), ssum.grad, dt, "conv_out d(a+b)")
    G.check_close(d_wo.cpu(), wo.grad, G.F32 if dt == G.F32 else G.BF16, "conv_out dW", scale=4.0)
    G.check_close(d_bo.cpu(), bo.grad, G.F32, "conv_out db", scale=4.0)


def test_temb_backward_vs_oracle():
    """ddimx_temb_fwd_train / ddimx_temb_bwd against autograd of BetaEmbedding (models/diffusion.py:110-120)."""
    _temb_backward(torch.tensor([0, 999, 123, 500, 7]), "tbw.dout")


def test_temb_backward_vs_oracle_batch_19():
    """The same at B = 19: linear_rows_kernel walks the batch in groups of 8, so two full groups and one of three rows (with a
    repeated timestep), and 19-term batch sums in the weight-gradient kernels."""
    _temb_backward(torch.tensor([0, 999, 123, 500, 7, 7, 1, 998, 250, 251, 640, 33, 812, 77, 404, 999, 512, 5, 321]), "tbw.dout19")


def _temb_backward(t, tag):
    lib = _lib.load()
    B = t.numel()
    shapes = {"temb.weight.0.weight": (512, 128), "temb.weight.0.bias": (512,), "temb.weight.1.weight": (512, 512),
              "temb.weight.1.bias": (512,), "temb.weight.2.weight": (4416, 512), "temb.weight.2.bias": (4416,)}
    sd = synth.fill_state_dict({k: torch.empty(s) for k, s in shapes.items()})
    sd["temb.te"] = ref_cpu.timestep_table(1000)
    d_out = synth.gaussian(tag, (B, 4416))
    leaf = {k: (v.clone().requires_grad_(True) if k != "temb.te" else v) for k, v in sd.items()}
    out_ref = ref_cpu.beta_embedding(leaf, t)
    out_ref.backward(d_out)
    te, tg = G.g(sd["temb.te"]), t.to(G.dev())
    ws = [G.g(sd[f"temb.weight.{i}.{k}"]) for i in range(3) for k in ("weight", "bias")]
    h1, h2 = torch.empty(B, 512, device=G.dev()), torch.empty(B, 512, device=G.dev())
    out = torch.full((B, 4416), float("nan"), device=G.dev())
    _lib.check(lib.ddimx_temb_fwd_train(_lib.ptr(te), _lib.ptr(tg), *[_lib.ptr(v) for v in ws], _lib.ptr(h1), _lib.ptr(h2), _lib.ptr(out),
                                        B, 128, 512, 4416, _lib.stream()))
    G.check_close(out.cpu(), out_ref.detach(), G.F32, "temb forward (training)")
    grads = [torch.full_like(v, float("nan")) for v in ws]
    dh2, dh1 = torch.empty(B, 512, device=G.dev()), torch.empty(B, 512, device=G.dev())
    dg = G.g(d_out)
    _lib.check(lib.ddimx_temb_bwd(_lib.ptr(dg), _lib.ptr(te), _lib.ptr(tg), _lib.ptr(ws[2]), _lib.ptr(ws[4]), _lib.ptr(h1), _lib.ptr(h2),
                                  _lib.ptr(dh2), _lib.ptr(dh1), *[_lib.ptr(v) for v in grads], B, 128, 512, 4416, _lib.stream()))
    for i in range(3):
        for j, k in enumerate(("weight", "bias")):
            G.check_close(grads[2 * i + j].cpu(), leaf[f"temb.weight.{i}.{k}"].grad, G.F32, f"temb d{k}{i}", scale=4.0)


# ---- Transformer_Module alone: the `_bwd` twin of ddimx_fnet_fwd ----------------------------------------
def _fnet_setup(s_len, b):
    """The audio-width Transformer_Module behind the C ABI for a batch of b clips of s_len tokens: the filled model, its packed
    weights and tables, gaussian tokens and output gradient (reference token order, CPU) and the device buffers of a
    ddimx_fnet_fwd_train + ddimx_fnet_bwd pair."""
    import types
    lib = _lib.load()
    cfg = configs.audio_config("torch.cuda.FloatTensor")
    m = synth.fill_module(D.Model(cfg)).train()
    dev = G.dev()
    t_len = s_len * 32
    lib2 = m._ensure_handle()
    with torch.cuda.device(dev):
        m._ensure_packed(lib2, dev)
        m._ensure_packed_bwd(lib2, dev)
        pe, dh, ds = m._ensure_tables(t_len, dev)
    tok = synth.gaussian(f"fnetbwd.x{s_len}", (b, s_len, 2048))  # (the tags do not name b: the b = 2 cases keep their data)
    dout = synth.gaussian(f"fnetbwd.dy{s_len}", (b, s_len, 2048))
    to_lib = lambda v: v.view(b, s_len, 256, 8).permute(0, 1, 3, 2).contiguous()      # reference token order c*8+f -> f*256+c
    total, layout = m._grad_layout(lib)
    return types.SimpleNamespace(
        lib=lib, cfg=cfg, m=m, dev=dev, b=b, s_len=s_len, t_len=t_len, tables=(pe, dh, ds), tok=tok, dout=dout,
        from_lib=lambda v: v.view(b, s_len, 8, 256).permute(0, 1, 3, 2).reshape(b, s_len, 2048),
        x=to_lib(tok).to(dev), d_out=to_lib(dout).reshape(b * s_len, 2048).to(dev), total=total, layout=layout,
        ws=torch.empty(int(lib.ddimx_train_workspace_bytes(m._handle, b, t_len)), dtype=torch.uint8, device=dev),
        tape=torch.empty(int(lib.ddimx_train_tape_bytes(m._handle, b, t_len)), dtype=torch.uint8, device=dev))


def _fnet_run(c, p, seed):
    """ddimx_fnet_fwd_train + ddimx_fnet_bwd with dropout (p, seed) into NaN-filled buffers: (output, d_tokens, flat gradient buffer)
    on the device, the first two [B * S, 2048] in the library's token order."""
    import ctypes
    lib, m, b, s_len, dev = c.lib, c.m, c.b, c.s_len, c.dev
    out = torch.full((b * s_len, 2048), float("nan"), device=dev)
    d_x = torch.full((b * s_len, 2048), float("nan"), device=dev)
    grads = torch.full((c.total,), float("nan"), device=dev)
    tb = _lib.DdimxTables(*(v.data_ptr() for v in c.tables))
    st = _lib.stream()
    _lib.check(lib.ddimx_fnet_fwd_train(m._handle, _lib.ptr(m._packed), ctypes.byref(tb), _lib.ptr(c.ws), c.ws.numel(), _lib.ptr(c.tape),
                                        c.tape.numel(), _lib.ptr(c.x), _lib.ptr(out), b, c.t_len, p, seed, st))
    _lib.check(lib.ddimx_fnet_bwd(m._handle, _lib.ptr(m._packed), _lib.ptr(m._packed_bwd), ctypes.byref(tb), _lib.ptr(c.ws), c.ws.numel(),
                                  _lib.ptr(c.tape), c.tape.numel(), _lib.ptr(c.x), _lib.ptr(c.d_out), _lib.ptr(d_x), _lib.ptr(grads), b,
                                  c.t_len, p, seed, st))
    torch.cuda.synchronize()
    return out, d_x, grads


def _ratio(res, dt, scale=1.0):
    """The worse of a check_close result's (max, rms) as a share of its gate."""
    return max(res[0] / (G.TOL[dt]["mx"] * scale), res[1] / (G.TOL[dt]["rms"] * scale))


def _fnet_train_case(s_len, b, p, seed):
    """The module output, d_tokens and every transformer.* gradient of one ddimx_fnet_fwd_train + ddimx_fnet_bwd pair with dropout
    (p, seed) against autograd through ``ref_cpu.transformer_module``; with p > 0 the oracle drops the elements the library drops
    (``fnet_kernel_ref.dropout_hook``).  Returns (setup, module output in the reference token order, the hook or None)."""
    c = _fnet_setup(s_len, b)
    m, cfg = c.m, c.cfg
    out, d_x, grads = _fnet_run(c, p, seed)
    # oracle: autograd through the CPU restatement
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if k.startswith("transformer.")}
    for v in sd.values():
        v.requires_grad_(True)
    xin = c.tok.clone().requires_grad_(True)
    kw = cfg.model.transformers.kwargs
    hook = R.dropout_hook(p, seed, b, s_len, kw.hidden_size) if p > 0.0 else None
    y = ref_cpu.transformer_module(sd, xin, kw.num_hidden_layers, kw.layer_norm_eps, drop=hook)
    y.backward(c.dout)
    got = c.from_lib(out.cpu())
    r_out = G.check_close(got, y.detach(), G.F32, f"fnet train fwd S={s_len}")
    r_dx = G.check_close(c.from_lib(d_x.cpu()), xin.grad, G.F32, f"fnet d_tokens S={s_len}", scale=5.0)
    checked, worst = 0, 0.0
    for (name, _), (off, numel, shape) in zip(m.named_parameters(), c.layout):
        g = grads[off:off + numel].cpu().view(shape)
        if not name.startswith("transformer."):
            assert torch.isnan(g).all(), f"{name}: ddimx_fnet_bwd must leave other gradients untouched"
            continue
        want = sd[name].grad
        rms = float(want.double().square().mean().sqrt()) + 1e-30
        err = float((g.double() - want.double()).abs().max()) / rms
        assert torch.isfinite(g).all() and err <= 2e-3, (name, err)
        worst = max(worst, err)
        checked += 1
    assert checked == 4 + 8 * kw.num_hidden_layers + 2
    print(f"[fnet train S={s_len} B={b} p={p}] worst output {_ratio(r_out, G.F32):.3f}, d_tokens {_ratio(r_dx, G.F32, 5.0):.3f}, "
          f"parameter gradient {worst / 2e-3:.3f} of the gate")
    return c, got, hook


@pytest.mark.parametrize("s_len,b", [(4, 2), (32, 2), (96, 2), (1, 3), (3, 5)], ids=["4", "32", "96", "1-b3", "3-b5"])
def test_fnet_bwd_per_op_vs_autograd_through_the_oracle(s_len, b):
    """ddimx_fnet_fwd_train + ddimx_fnet_bwd (models/diffusion.py:148-167 and autograd through it) against
    ``ref_cpu.transformer_module`` differentiated by torch autograd on the CPU, fp32 mode, dropout 0: the module output,
    the gradient w.r.t. the input tokens and EVERY transformer.* parameter gradient (102 tensors; S = 96 takes the two-GEMM
    Fourier path and the rounded-up positional table, S <= 32 the fused mixing kernel).  (S, B) = (1, 3) and (3, 5): M = B * S = 3
    and 15 rows, odd and no multiple of 4 -- the K of every weight-gradient GEMM (scalar loads, less than one K chunk) and the
    short side of every transpose."""
    _fnet_train_case(s_len, b, 0.0, 1234)


DROPOUT_SEED = 0x9E3779B97F4A7C15


def _masked_after_the_residual(sd, x, n_layers, eps, drop):
    """``ref_cpu.transformer_module`` with one mistake: layer i's mask falls on ``output.dense(..) + y``, after the residual add."""
    p = "transformer."
    s, width = x.shape[1], x.shape[2]
    h = x + ref_cpu.add_encoding(torch.zeros(2 ** int(np.ceil(np.log2(s))), width))[:s]
    h = F.layer_norm(h, (width,), sd[p + "embedding.LayerNorm.weight"], sd[p + "embedding.LayerNorm.bias"], eps)
    h = drop(0, F.linear(h, sd[p + "embedding.projection.weight"], sd[p + "embedding.projection.bias"]))
    for i in range(n_layers):
        q = f"{p}encoder.layer.{i}."
        hid = h.shape[-1]
        y = F.layer_norm(h + torch.fft.fftn(h, dim=(1, 2)).real, (hid,), sd[q + "fourier.output.LayerNorm.weight"],
                         sd[q + "fourier.output.LayerNorm.bias"], eps)
        z = ref_cpu.gelu_new(F.linear(y, sd[q + "intermediate.dense.weight"], sd[q + "intermediate.dense.bias"]))
        z = F.linear(z, sd[q + "output.dense.weight"], sd[q + "output.dense.bias"])
        h = F.layer_norm(drop(i + 1, z + y), (hid,), sd[q + "output.LayerNorm.weight"], sd[q + "output.LayerNorm.bias"], eps)
    return F.linear(h, sd[p + "compute_out.weight"], sd[p + "compute_out.bias"])


@pytest.mark.parametrize("s_len,b,p", [(4, 2, 0.1), (96, 2, 0.1), (3, 5, 0.5)], ids=["4", "96", "3-b5-p0.5"])
def test_fnet_train_with_dropout_vs_oracle_with_the_same_masks(s_len, b, p):
    """The same comparison with dropout on, at the same gates: the oracle takes the masks of ``dropout_keep(seed, stream, element)``
    (restated in tests/fnet_kernel_ref.py) at its own dropout sites -- stream 0 on the embedding projection's output, stream i + 1 on
    layer i's ``output.dense`` result before the residual add, element (b * S + s) * hid + n -- so the GPU and the oracle agree only
    if ``fnet_fwd_train_part`` / ``fnet_bwd_part`` drop that tensor, on that side of the residual, with that stream and index, and
    mask d(FFN out) but not the residual's gradient.  S = 4: the fused mixing kernel; S = 96: the two-GEMM Fourier path and the
    rounded-up positional table; (S, B, p) = (3, 5, 0.5): 15 rows, half of everything dropped.  The case S = 4 also meets three wrong
    oracles (two sites exchanged, every mask shifted by one element, the mask after the residual add) and must miss each one's
    output gate by a factor of 10 at least."""
    c, got, hook = _fnet_train_case(s_len, b, p, DROPOUT_SEED)
    kw = c.cfg.model.transformers.kwargs
    n, hid = kw.num_hidden_layers, kw.hidden_size
    assert hook.sites == list(range(n + 1))
    plain = c.from_lib(_fnet_run(c, 0.0, DROPOUT_SEED)[0].cpu())
    assert float((got != plain).double().mean()) > 0.5, "dropout changed less than half of the module's output"
    if s_len != 4:
        return
    sd = {k: v.detach().cpu() for k, v in c.m.state_dict().items() if k.startswith("transformer.")}
    good = R.dropout_hook(p, DROPOUT_SEED, b, s_len, hid)

    def shifted(site, h):
        return h * torch.from_numpy(R.dropout_scale(p, DROPOUT_SEED, site, h.numel(), first=1)).reshape(h.shape)

    with torch.no_grad():
        wrong = {
            "sites 1 and 2 exchanged": ref_cpu.transformer_module(sd, c.tok, n, kw.layer_norm_eps,
                                                                  drop=lambda site, h: good({1: 2, 2: 1}.get(site, site), h)),
            "masks shifted by one element": ref_cpu.transformer_module(sd, c.tok, n, kw.layer_norm_eps, drop=shifted),
            "mask after the residual add": _masked_after_the_residual(sd, c.tok, n, kw.layer_norm_eps, good),
        }
    for what, y in wrong.items():
        r = _ratio(rel_err(got, y), G.F32)
        print(f"[fnet dropout control: {what}] {r:.3e} of the gate")
        assert r >= 10.0, f"{what}: the GPU output is within {r:.3e} of the gate of a wrong oracle"
        with pytest.raises(AssertionError):
            G.check_close(got, y, G.F32, what)


@pytest.mark.parametrize("seed,k", [(1234, 1), (2 ** 64 - 3, 7)], ids=["plain", "wrap"])
def test_dropout_device_counter_adds_to_the_seed(seed, k):
    """ddimx_set_dropout_counter: with a device counter holding k, every dropout launch of the forward and the backward takes the
    mask stream of seed + k mod 2^64 -- output, d_tokens and the whole gradient buffer equal those of that seed by value, bit for
    bit ((2^64 - 3) + 7 wraps to 4)."""
    c = _fnet_setup(4, 2)
    ctr = torch.tensor([k], dtype=torch.int64, device=c.dev)
    try:
        _lib.check(c.lib.ddimx_set_dropout_counter(c.m._handle, _lib.ptr(ctr)))
        with_ctr = _fnet_run(c, 0.1, seed)
    finally:
        _lib.check(c.lib.ddimx_set_dropout_counter(c.m._handle, None))
    by_value = _fnet_run(c, 0.1, (seed + k) % 2 ** 64)
    other = _fnet_run(c, 0.1, seed)
    for what, a, v, o in zip(("output", "d_tokens", "gradients"), with_ctr, by_value, other):
        assert torch.equal(a.view(torch.int32), v.view(torch.int32)), what
        assert not torch.equal(a.view(torch.int32), o.view(torch.int32)), f"{what}: the counter changed nothing"
    assert torch.isfinite(with_ctr[0]).all() and torch.isfinite(with_ctr[1]).all()


# ---- the whole network with dropout on: the oracle drops what the library drops ------------------------------------------------------
DROPOUT_CASES = [("tiny", (3, 2, 24, 32), [0, 999, 412]), ("audio", (2, 2, 32, 256), [0, 999])]
DROPOUT_P, TORCH_SEED, CALLS_BEFORE = 0.1, 2022, 6


def _dropout_model(name, dtype_str, seed):
    cfg, m = _train_model(name, dtype_str, seed, dropout=DROPOUT_P)
    torch.manual_seed(TORCH_SEED)
    m._dropout_calls = CALLS_BEFORE
    return cfg, m


def _mask_seed():
    """model.py's rule for the mask stream of a forward: (torch.initial_seed() * 0x9E3779B1 + rank * 0xC2B2AE3D27D4EB4F + calls)
    mod 2^64, ``calls`` counted after the increment -- here seed 2022, rank 0, the seventh call."""
    return (TORCH_SEED * 0x9E3779B1 + 0 * 0xC2B2AE3D27D4EB4F + (CALLS_BEFORE + 1)) % 2 ** 64


def _oracle_forward_with_the_masks(name, shape, hooks):
    """``forward`` of MH.backward_case: ref_cpu.model_forward under a fresh ``dropout_hook`` per call, kept in ``hooks``."""
    ocfg = (configs.tiny_config if name == "tiny" else configs.audio_config)("torch.FloatTensor")
    s = shape[2] >> (len(ocfg.model.ch) - 1)
    hid = ocfg.model.transformers.kwargs.hidden_size

    def forward(live, cfg, x, t):
        hooks.append(R.dropout_hook(DROPOUT_P, _mask_seed(), shape[0], s, hid))
        return ref_cpu.model_forward(live, cfg, x, t, drop=hooks[-1])

    return forward


@pytest.mark.parametrize("mode", MODES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name,shape,tt", DROPOUT_CASES, ids=["tiny", "audio"])
def test_model_backward_with_dropout_vs_oracle(mode, name, shape, tt):
    """hidden_dropout_prob = 0.1 (the shipped audio configuration): loss and every parameter gradient against autograd through the
    oracle with the library's masks, at ``MH.backward_case``'s gates -- the mask seed restated from model.py's rule."""
    seen, hooks = {}, []

    def loss(m, x0, t, e, a):
        seen.update(m=m, args=(x0, t, e, a), loss=losses.noise_estimation_loss(m, x0, t, e, a))
        return seen["loss"]

    MH.backward_case(mode, shape, tt, build_model=_dropout_model, loss=loss, ref_loss=ref_cpu.noise_estimation_loss,
                     forward=_oracle_forward_with_the_masks(name, shape, hooks), name=name)
    m = seen["m"]
    assert m._dropout_calls == CALLS_BEFORE + 1
    n_layers = m.config.transformers.kwargs.num_hidden_layers
    assert len(hooks) == 1 and hooks[0].sites == list(range(n_layers + 1))
    m.eval()
    with torch.no_grad():
        l_eval = losses.noise_estimation_loss(m, *seen["args"])
    diff = abs(float(seen["loss"]) - float(l_eval)) / float(l_eval)
    print(f"[backward dropout {name} {'f32' if mode[1] == G.F32 else 'bf16'}] training loss differs from the eval-mode loss by {diff:.3e}")
    # dropout is really on: in fp32 mode the difference is beyond the loss gate above, so the oracle without masks would fail it
    assert diff > (1e-5 if mode[1] == G.F32 else 0.0), "the training loss is the eval-mode loss: no dropout?"


@pytest.mark.parametrize("mode", MODES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name,shape,tt", DROPOUT_CASES, ids=["tiny", "audio"])
def test_train_mode_input_grad_with_dropout_vs_oracle(mode, name, shape, tt):
    """The gradient w.r.t. the network input with dropout on, against autograd through the oracle with the library's masks, at
    ``MH.gate``: once beside the parameter gradients and once with every parameter frozen (the data-only backward meets the same
    gate against the oracle; it is not merely compared with the full one)."""
    dtype_str, dt = mode
    cfg, m = _dropout_model(name, dtype_str, 5)
    a = MH.alphas(cfg)
    x0, e, t = synth.gaussian("igrad.x0", shape), synth.gaussian("igrad.e", shape), torch.tensor(tt)
    live, ocfg = MH.oracle(m, name)
    hooks = []
    xr = x0.clone().requires_grad_(True)
    fwd = _oracle_forward_with_the_masks(name, shape, hooks)
    want = ref_cpu.noise_estimation_loss(lambda xx, ts: fwd(live, ocfg, xx, ts), xr, t, e, a)
    want.backward()
    assert len(hooks) == 1 and hooks[0].sites == list(range(cfg.model.transformers.kwargs.num_hidden_layers + 1))
    for frozen in (False, True):
        m.requires_grad_(not frozen)
        m.zero_grad(set_to_none=True)
        m._dropout_calls = CALLS_BEFORE
        xg = x0.cuda().requires_grad_(True)
        loss = losses.noise_estimation_loss(m, xg, t.cuda(), e.cuda(), a.cuda())
        loss.backward()
        assert m._dropout_calls == CALLS_BEFORE + 1
        assert all((q.grad is None) == frozen for q in m.parameters())
        what = f"x0.grad {name} {shape} dropout {'data-only' if frozen else 'full'}"
        mx, er = MH.gate(xg.grad, xr.grad, dt, what)
        lim = (2e-3, float("inf")) if dt == G.F32 else (0.6, 5e-2)
        print(f"[input grad dropout {name} {'f32' if dt == G.F32 else 'bf16'} {'data-only' if frozen else 'full'}] max {mx:.3e} "
              f"rms err {er:.3e} x rms, worst {max(mx / lim[0], er / lim[1]):.3f} of the gate")
