"""GPU parity tests at the BASELINE.json configuration shapes that the per-op / small-shape suites do not reach:

* configs[2]: batch 64, 50-step DDIM (stride 20), hipGraph-captured step  -> test_cfg3_*
* configs[3]: the training step at T = 1024 with the audio.yml widths (32 samples per GPU) -> test_cfg4_*
* the eta > 0 branch of generalized_steps with the noise the sampler really drew -> test_sampler_eta_*
* backward weight packings after out-of-band parameter writes -> test_backward_packings_*
* 1-rank vs 2-rank equality on the GPU path (needs two devices; skipped on a one-GPU box) -> test_two_ranks_*

Size-independent properties do the work at full size (bit-exact batch independence, graph == eager, replicated-batch
gradient identity); the CPU oracle is used where it finishes in seconds (one B = 2 training step at T = 1024: ~15 s).
"""
import os

import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import configs, losses, synth
from ddim_audio_amd.schedule import make_schedule
from oracle import ref_cpu
import gpu_util as G
import model_harness as MH
from model_harness import MODES

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------- configs[2]
@pytest.mark.parametrize("mode", MODES, ids=["f32", "bf16"])
def test_cfg3_batch64_50step_graph_sampler(mode):
    """BASELINE configs[2]: B = 64 spectrograms [2,1024,256], seq = range(0, 1000, 20) (50 iterations), eta = 0, the step
    replayed from a hipGraph.  Checked: finite; graph replay == eager launches bit for bit (bf16; fp32 on a 10-step prefix to
    bound the run time); sample k of the batch == the same sample run alone through its own graph, bit for bit."""
    dtype_str, dt = mode
    cfg, m = MH.build("audio", dtype_str, 0, mode="eval")
    alphas = make_schedule(cfg.diffusion)[1]
    seq = list(range(0, 1000, 20))
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    x = torch.randn(64, 2, 1024, 256, device="cuda", generator=g)
    k = 37
    xin = x.clone()
    xs, x0 = D.generalized_steps(xin, seq, m, alphas, [-1], eta=0.0)
    assert len(xs) == 2 and len(x0) == 1 and xs[0] is xin
    final = xs[-1]
    assert final.shape == (64, 2, 1024, 256) and torch.isfinite(final).all()
    assert float(final.std()) > 1e-3
    solo_xs, _ = D.generalized_steps(x[k:k + 1].clone(), seq, m, alphas, [-1], eta=0.0)
    assert torch.equal(solo_xs[-1][0], final[k]), "sample 37 differs between the batch of 64 and a batch of 1"
    # graph == eager
    short = seq if dt == G.BF16 else seq[-10:]
    a, _ = D.generalized_steps(x.clone(), short, m, alphas, [-1], eta=0.0)
    with MH.eager_steps():
        b, _ = D.generalized_steps(x.clone(), short, m, alphas, [-1], eta=0.0)
    assert torch.equal(a[-1], b[-1]), "hipGraph replay and eager stepping disagree"
    if dt == G.BF16:
        assert torch.equal(a[-1], final)


# ------------------------------------------------------------------------------------------------- configs[3]
@pytest.fixture(scope="module")
def cfg4_oracle():
    """loss + every parameter gradient of ONE training forward/backward at the configs[3] sample shape (B = 2, T = 1024,
    audio.yml widths) by autograd through the CPU oracle (oracle/ref_cpu.py, itself pinned to the reference's gradients by
    tests/golden/train.npz)."""
    cfg = configs.audio_config("torch.FloatTensor")
    from ddim_audio_amd.model import state_inventory  # (not `D.model`: the submodule attribute exists only once something imported it)
    sd = {k: torch.empty(s) for k, s in state_inventory(cfg).items()}
    synth.fill_state_dict(sd)
    sd["temb.te"] = ref_cpu.timestep_table(cfg.diffusion.num_diffusion_timesteps)
    alphas = make_schedule(cfg.diffusion)[1]
    shape = (2, 2, 1024, 256)
    x0, e = synth.gaussian("cfg4.x0", shape), synth.gaussian("cfg4.e", shape)
    t = torch.tensor([812, 187])
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k != "temb.te"}
    live = dict(params, **{"temb.te": sd["temb.te"]})
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    loss = ref_cpu.noise_estimation_loss(lambda a, b: ref_cpu.model_forward(live, cfg, a, b), x0, t, e, alphas)
    loss.backward()
    grads = {k: p.grad.detach() for k, p in params.items()}
    return dict(x0=x0, e=e, t=t, alphas=alphas, loss=float(loss), grads=grads)


# (loss, worst gradient element / RMS gradient of its tensor, global gradient norm) gates.  Measured on MI355X:
#   fp32: loss exact to the last printed digit, element 8.6e-5, norm 5e-8
#   bf16 activations + fp32 FNet: loss 3.5e-5, element 0.27 (transformer.encoder.layer.5.output.dense.weight), norm 6e-5
#   bf16 activations + bf16 FNet operands: loss 2.7e-5, element 0.30 (transformer.encoder.layer.4.intermediate.dense.weight), norm 3e-5
#   (round 4, profiles/r04/cfg4_gradient_parity.txt; the element gate went from 0.55 to 0.40 x RMS)
# (the worst elements sit in the FNet weight gradients in both bf16 modes: their error comes from the bf16 bottleneck
#  activations feeding the FNet, not from the GEMM operand type) -> gates at 1.3-2x the measured values
_CFG4_GATES = {("torch.cuda.FloatTensor", None): (1e-6, 2e-4, 1e-6), ("torch.cuda.BFloat16Tensor", "torch.cuda.FloatTensor"): (1e-4, 0.40, 3e-4),
               ("torch.cuda.BFloat16Tensor", None): (1e-4, 0.40, 3e-4)}


@pytest.mark.parametrize("key", list(_CFG4_GATES), ids=["f32", "bf16_fnet32", "bf16"])
def test_cfg4_training_step_full_size_vs_oracle(cfg4_oracle, key):
    """configs[3] shape: one training forward + backward at T = 1024 with the audio.yml widths.  (a) B = 2: loss and all 388
    gradients against the oracle; (b) B = 32 (the per-GPU batch of configs[3]) made of the same pair 16 times: the batch-mean
    loss and every gradient must equal the B = 2 ones up to fp32 summation order, because every op is per sample and the
    reductions over the batch are fixed-order sums."""
    dtype_str, fnet = key
    loss_tol, elem_tol, norm_tol = _CFG4_GATES[key]
    o = cfg4_oracle
    # dropout 0: a deterministic function (the oracle has no dropout)
    cfg, m = MH.build("audio", dtype_str, 0, mode="train", dropout=0.0, optimizer="AdamW", fnet=fnet)
    al = o["alphas"].cuda()
    loss = losses.noise_estimation_loss(m, o["x0"].cuda(), o["t"].cuda(), o["e"].cuda(), al)
    loss.backward()
    assert abs(float(loss) - o["loss"]) <= loss_tol * o["loss"], (float(loss), o["loss"])
    total = sum(float(g.double().square().sum()) for g in o["grads"].values()) ** 0.5
    got_total, worst, worst_name = 0.0, 0.0, ""
    g2 = {}
    for name, p in m.named_parameters():
        ref = o["grads"][name]
        got = p.grad.detach().cpu()
        g2[name] = p.grad.detach().clone()
        assert torch.isfinite(got).all(), name
        got_total += float(got.double().square().sum())
        scale = max(float(ref.double().square().mean().sqrt()), 1e-4 * total / ref.numel() ** 0.5)
        err = float((got - ref).abs().max()) / scale
        if err > worst:
            worst, worst_name = err, name
    print(f"[cfg4 {key}] loss rel err {abs(float(loss) - o['loss']) / o['loss']:.2e}, worst gradient element {worst:.3e} x rms ({worst_name}), "
          f"global norm rel err {abs(got_total ** 0.5 - total) / total:.2e}")
    assert worst <= elem_tol, f"{worst_name}: {worst:.3e} x rms (gate {elem_tol})"
    assert abs(got_total ** 0.5 - total) <= norm_tol * total
    # (b) the per-GPU batch of configs[3]
    m.zero_grad(set_to_none=True)
    rep = lambda v: v.cuda().repeat(16, *([1] * (v.dim() - 1)))  # noqa: E731
    loss32 = losses.noise_estimation_loss(m, rep(o["x0"]), rep(o["t"]), rep(o["e"]), al)
    loss32.backward()
    assert abs(float(loss32) - float(loss)) <= (2e-6 if dtype_str.endswith("FloatTensor") else 2e-4) * abs(float(loss))
    # fp32: only the order of the fp32 / fp64 partial sums differs (the training step picks its tile variant from the real
    # batch, so the statistics partition changes with B).  bf16: those last-bit differences in the GroupNorm statistics flip
    # some bf16 roundings of the activations, which the gradients then carry: gate relative to the tensor's RMS gradient.
    rep_tol = 2e-3 if dtype_str.endswith("FloatTensor") else 0.25  # measured: fp32 2.8e-5, bf16 0.11
    worst_rep = 0.0
    for name, p in m.named_parameters():
        a, b = p.grad.detach().double(), g2[name].double()
        rms = max(float(b.square().mean().sqrt()), 1e-4 * total / b.numel() ** 0.5)
        worst_rep = max(worst_rep, float((a - b).abs().max()) / rms)
        assert float((a - b).abs().max()) <= rep_tol * rms, (name, float((a - b).abs().max()) / rms)
    print(f"[cfg4 {key}] B=32 (pair x16) vs B=2: worst gradient element {worst_rep:.3e} x rms")


def test_backward_packings_follow_out_of_band_writes():
    """ADVICE r1 (model.py:369): writes through ``p.data`` bump no version counter; after ``invalidate()`` the forward packing
    is rebuilt and the backward packings (data-gradient conv layouts, transposed FNet matrices) must be rebuilt with it."""
    cfg = configs.tiny_config("torch.cuda.FloatTensor")
    cfg.model.transformers.kwargs.hidden_dropout_prob = 0.0
    m = synth.fill_module(D.Model(cfg), 3).train()
    alphas = make_schedule(cfg.diffusion)[1].cuda()
    shape = (2, 2, 16, 32)
    x0, e = synth.gaussian("stale.x0", shape).cuda(), synth.gaussian("stale.e", shape).cuda()
    t = torch.tensor([123, 876]).cuda()
    losses.noise_estimation_loss(m, x0, t, e, alphas).backward()   # builds both packings
    m.zero_grad(set_to_none=True)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("conv.0.weight") or n.endswith("dense.weight") or n.endswith("conv.weight"):
                p.data.mul_(1.25)                                    # no version bump
    m.invalidate()
    losses.noise_estimation_loss(m, x0, t, e, alphas).backward()
    fresh = D.Model(cfg)
    fresh.load_state_dict(m.state_dict())
    fresh.train()
    losses.noise_estimation_loss(fresh, x0, t, e, alphas).backward()
    for (n, a), (_, b) in zip(m.named_parameters(), fresh.named_parameters()):
        assert torch.equal(a.grad, b.grad), f"{n}: gradient computed with stale backward packings"


# ------------------------------------------------------------------------------------------------- eta > 0
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_sampler_eta_nonzero_matches_oracle_with_the_drawn_noise(eta):
    """functions/denoising.py:36-43 with eta > 0: the sampler draws ``randn_like`` from torch's CUDA generator every step.
    Re-seeding reproduces exactly that noise sequence, which is then injected into the oracle's loop (same c1 / c2 algebra in
    double, same update order) -- an exact check of the stochastic branch instead of "runs and is finite"."""
    alphas = make_schedule(configs.audio_config().diffusion)[1]
    fake = lambda x, t: 0.1 * x + 0.01 * t.float().view(-1, 1, 1, 1)  # noqa: E731  (a stand-in model, torch ops)
    seq = list(range(0, 1000, 125))
    x = synth.gaussian("eta.x", (2, 2, 8, 16))
    torch.manual_seed(4321)
    xs, x0 = D.generalized_steps(x.cuda().clone(), seq, fake, alphas, None, eta=eta)
    torch.manual_seed(4321)
    ref_like = torch.empty(2, 2, 8, 16, device="cuda")
    noises = [torch.randn_like(ref_like).cpu() for _ in seq]
    exs, ex0 = ref_cpu.generalized_steps(x.clone(), seq, fake, alphas, None, eta=eta, noise_fn=lambda k, ref: noises[k])
    assert len(xs) == len(exs) and len(x0) == len(ex0)
    for k, (a, b) in enumerate(zip(xs[1:], exs[1:])):
        assert torch.allclose(a, b, rtol=2e-5, atol=2e-5), k
    for k, (a, b) in enumerate(zip(x0, ex0)):
        assert torch.allclose(a, b, rtol=2e-5, atol=2e-5), k
    # and the noise really entered: eta = 0 gives another trajectory
    xs0, _ = D.generalized_steps(x.cuda().clone(), seq, fake, alphas, None, eta=0.0)
    assert not torch.allclose(xs0[-2], xs[-2], rtol=1e-3, atol=1e-3)


# ------------------------------------------------------------------------------------------------- the full schedule
def test_generalized_steps_over_the_full_1000_entry_schedule_vs_oracle():
    """functions/denoising.py:10-52 with ``seq = range(1000)`` -- the step count of BASELINE configs[1] and configs[4] -- on the
    tiny network in fp32: 1000 U-Net evaluations through the hipGraph-replayed step against the CPU oracle's loop around its own
    forward (about 10 s of CPU).  Judged on the final x0 prediction and the final x (the trajectory feeds every step's error
    into the next 999, hence the per-forward gate x 30), plus ``select_index`` semantics at this length and graph == eager."""
    cfg, m = MH.build("tiny", "torch.cuda.FloatTensor", 3, mode="eval")
    alphas = make_schedule(cfg.diffusion)[1]
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ocfg = configs.tiny_config("torch.FloatTensor")
    seq = list(range(1000))
    x = synth.gaussian("full_schedule.x", (2, 2, 16, 32))
    sel = [0, 499, -1]
    xs, x0 = D.generalized_steps(x.cuda().clone(), seq, m, alphas, sel, eta=0.0)
    with torch.no_grad():
        exs, ex0 = ref_cpu.generalized_steps(x.clone(), seq, lambda a, t: ref_cpu.model_forward(sd, ocfg, a, t), alphas, sel, eta=0.0)
    assert len(xs) == len(exs) == 4 and len(x0) == len(ex0) == 3
    for k in range(3):
        G.check_close(x0[k].cpu(), ex0[k], G.F32, f"x0 prediction at selected step {sel[k]}", scale=30.0)
        G.check_close(xs[k + 1].cpu(), exs[k + 1], G.F32, f"x at selected step {sel[k]}", scale=30.0)
    assert torch.isfinite(xs[-1]).all()
    with MH.eager_steps():
        xs2, _ = D.generalized_steps(x.cuda().clone(), seq, m, alphas, [-1], eta=0.0)
    assert torch.equal(xs2[-1].cpu(), xs[-1].cpu()), "graph replay and eager stepping differ after 1000 steps"


# ------------------------------------------------------------------------------------------------- two ranks
def _rank_main(rank, world, port, ret):
    import torch.distributed as dist
    from ddim_audio_amd import dist as ddist, train
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    try:
        cfg = configs.tiny_config("torch.cuda.FloatTensor")
        cfg.model.transformers.kwargs.hidden_dropout_prob = 0.0
        m = synth.fill_module(D.Model(cfg), 3).eval()
        alphas = make_schedule(cfg.diffusion)[1]
        x = synth.gaussian("ranks.x", (4, 2, 32, 32)).cuda()
        seq = list(range(0, 1000, 100))
        out = ddist.sample_sharded(x, lambda xs: D.generalized_steps(xs, seq, m, alphas, [-1], eta=0.0)[0][-1].cuda())
        # training: 2 ranks x B=2 with grad sync == 1 rank x B=4
        m.train()
        ddist.attach_grad_sync(m)
        x0, e = synth.gaussian("ranks.x0", (4, 2, 32, 32)).cuda(), synth.gaussian("ranks.e", (4, 2, 32, 32)).cuda()
        t = torch.tensor([5, 994, 300, 650]).cuda()
        lo, hi = ddist.shard_bounds(4, rank, world)
        losses.noise_estimation_loss(m, x0[lo:hi], t[lo:hi], e[lo:hi], alphas.cuda()).backward()
        flat = torch.cat([p.grad.reshape(-1) for p in m.parameters()])
        if rank == 0:
            ret["sample"] = out.cpu()
            ret["grad"] = flat.cpu()
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_one_rank_on_the_gpu_path():
    """two spawned ranks (one per GPU, RCCL) sample a batch of 4 sharded 2 + 2 and must reproduce the
    single-rank result bit for bit; 2 ranks x 2 samples of training with attach_grad_sync must give the single-rank B = 4 flat
    gradient to fp32 tolerance.  Needs two devices: skipped on the one-GPU test box (the gloo world-2 tests in
    tests/test_host_cpu.py cover the host logic there)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    cfg = configs.tiny_config("torch.cuda.FloatTensor")
    cfg.model.transformers.kwargs.hidden_dropout_prob = 0.0
    m = synth.fill_module(D.Model(cfg), 3).eval()
    alphas = make_schedule(cfg.diffusion)[1]
    x = synth.gaussian("ranks.x", (4, 2, 32, 32)).cuda()
    one = D.generalized_steps(x.clone(), list(range(0, 1000, 100)), m, alphas, [-1], eta=0.0)[0][-1]
    assert torch.equal(ret["sample"], one)
    m.train()
    x0, e = synth.gaussian("ranks.x0", (4, 2, 32, 32)).cuda(), synth.gaussian("ranks.e", (4, 2, 32, 32)).cuda()
    t = torch.tensor([5, 994, 300, 650]).cuda()
    losses.noise_estimation_loss(m, x0, t, e, alphas.cuda()).backward()
    flat = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).cpu()
    assert torch.allclose(ret["grad"], flat, rtol=1e-4, atol=1e-6 * float(flat.abs().max()))


# ------------------------------------------------------------------------------------------------- eval-mode embedding table, live graphs
@pytest.mark.parametrize("mode", MODES, ids=["f32", "bf16"])
def test_eval_timestep_embedding_table_equals_the_mlp(mode):
    """Eval mode: BetaEmbedding (models/diffusion.py:110-120) is looked up in a [1000][E] table built once per weight set with
    the same kernels; the result must equal the per-call MLP bit for bit (the table is dropped in train mode)."""
    dtype_str, dt = mode
    cfg, m = MH.build("audio", dtype_str, 0, mode="eval")
    x = synth.gaussian("branches.x", (5, 2, 64, 256)).cuda()
    t = torch.tensor([0, 999, 123, 500, 7]).cuda()
    with torch.no_grad():
        y_tab = m(x, t)
        assert m._temb_table is not None
        keep, m._temb_table = m._temb_table, None
        y_mlp = m(x, t)
        m._temb_table = keep
    assert torch.equal(y_tab, y_mlp)


def test_live_graph_sees_load_state_dict_and_in_place_parameter_writes():
    """a stepper whose graph is live across ``nn.Module.load_state_dict`` or an in-place ``p.copy_()`` (neither sets
    ``Model._dirty``) must replay with the NEW weights, embedding table and folded FNet copies: before every replay the stepper
    runs the model's own (data_ptr, version) staleness test and repacks in place.  Compared with an eager run that makes the
    same updates at the same steps; one capture throughout."""
    from ddim_audio_amd.sampler import DDIMStepper
    from ddim_audio_amd import schedule
    cfg, m = MH.build("tiny", "torch.cuda.BFloat16Tensor", 3, mode="eval")
    other = synth.fill_module(D.Model(cfg), 11).eval().state_dict()
    first = {k: v.clone() for k, v in m.state_dict().items()}
    alphas = make_schedule(cfg.diffusion)[1]
    seq = list(range(0, 1000, 100))
    coef = schedule.ddim_coefficients(seq, alphas, 0.0)
    x = synth.gaussian("livegraph.x", (4, 2, 32, 32)).cuda()
    outs = []
    for graph in (False, True):
        m.load_state_dict(first)
        xt = x.clone()
        st = DDIMStepper(m, xt, coef, use_graph=graph)
        for k in range(len(seq)):
            if k == 4:
                m.load_state_dict(other)            # plain nn.Module.load_state_dict: copy_ into the parameters
            if k == 7:
                with torch.no_grad():
                    pb = dict(m.named_parameters())["temb.weight.2.bias"]
                    pb.copy_(pb * 0.5 + 0.1)   # in-place write: bumps _version only
            st.step()
        torch.cuda.synchronize()
        outs.append((xt.clone(), st.x0.clone()))
        if graph:
            assert st.captures == 1 and st.graph is not None
        st.close()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # and the updates really changed the trajectory
    m.load_state_dict(first)
    xt = x.clone()
    st = DDIMStepper(m, xt, coef, use_graph=False)
    for _ in seq:
        st.step()
    torch.cuda.synchronize()
    assert not torch.equal(xt, outs[0][0])


def test_conv_results_do_not_depend_on_concurrent_kernels():
    """Regression test of a round-1 hazard in the streamed-weight convolutions (C >= 64): reads of a ring stage were still
    in flight at the stage barrier, so with a second kernel loading the CU's LDS pipeline a later LDS-DMA could land first
    (a few samples off by ~1e-2 in 5-50 % of runs).  Victim: fused convolutions and a down/up pair of the streamed-weight
    levels on a side stream; aggressor: whole B = 32 forwards on the main stream.  Every victim run must be bit-identical
    to its quiet run."""
    from ddim_audio_amd import _lib
    lib = _lib.load()
    dt, tdt = G.BF16, torch.bfloat16
    cfg, m = MH.build("audio", "torch.cuda.BFloat16Tensor", 0, mode="eval")
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    xa = torch.randn(32, 2, 1024, 256, device="cuda", generator=g)
    ta = torch.randint(0, 1000, (32,), device="cuda")
    ch = [32, 64, 96, 128, 192, 256]
    b = 8

    def conv(l):
        c, h, w = ch[l], 1024 >> l, 256 >> l
        x = torch.randn(b, h, w, c, device="cuda", generator=g).to(tdt)
        y = torch.empty_like(x)
        wt = (torch.randn(9 * c * c, device="cuda", generator=g) / (9 * c) ** 0.5).to(tdt)
        temb = torch.randn(b, c, device="cuda", generator=g) * 0.1
        sc, sh = torch.rand(b, c, device="cuda", generator=g) + 0.5, torch.randn(b, c, device="cuda", generator=g) * 0.1
        stats = torch.zeros(int(lib.ddimx_conv3x3_stats_floats(dt, c, b, h, w)), device="cuda")

        def run():
            _lib.check(lib.ddimx_conv3x3_fwd(dt, c, _lib.ptr(x), _lib.ptr(wt), None, _lib.ptr(temb), c, _lib.ptr(sc), _lib.ptr(sh), 2, 1,
                                             _lib.ptr(y), _lib.ptr(stats), b, h, w, _lib.stream()))
            return torch.cat([y.float().flatten(), stats])
        return run

    def downup(l):
        cp, c, h, w = ch[l - 1], ch[l], 1024 >> (l - 1), 256 >> (l - 1)
        x = torch.randn(b, h, w, cp, device="cuda", generator=g).to(tdt)
        wd = (torch.randn(16 * c * cp, device="cuda", generator=g) / (16 * cp) ** 0.5).to(tdt)
        bd = torch.randn(c, device="cuda", generator=g) * 0.1
        y = torch.empty(b, h // 2, w // 2, c, device="cuda", dtype=tdt)
        wu = (torch.randn(2 * 6 * 2 * cp * c, device="cuda", generator=g) / (16 * c) ** 0.5).to(tdt)
        bu = torch.randn(2 * cp, device="cuda", generator=g) * 0.1
        z = torch.empty_like(x)

        def run():
            _lib.check(lib.ddimx_downsample_fwd(dt, cp, c, _lib.ptr(x), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y), b, h, w, _lib.stream()))
            _lib.check(lib.ddimx_upsample_add_fwd(dt, c, cp, _lib.ptr(y), _lib.ptr(wu), _lib.ptr(bu), _lib.ptr(x), _lib.ptr(z), b, h // 2,
                                                  w // 2, _lib.stream()))
            return torch.cat([y.float().flatten(), z.float().flatten()])
        return run

    side = torch.cuda.Stream()
    with torch.no_grad():
        m(xa, ta)
        torch.cuda.synchronize()
        for name, fn in [("conv L1", conv(1)), ("conv L2", conv(2)), ("conv L5", conv(5)), ("down/up L2", downup(2)), ("down/up L4", downup(4))]:
            ref = fn().clone()
            torch.cuda.synchronize()
            bad = 0
            for _ in range(8):
                main = torch.cuda.current_stream()
                side.wait_stream(main)
                m(xa, ta)
                with torch.cuda.stream(side):
                    outs = [fn().clone() for _ in range(3)]
                main.wait_stream(side)
                torch.cuda.synchronize()
                bad += sum(0 if torch.equal(o, ref) else 1 for o in outs)
            assert bad == 0, f"{name}: {bad}/24 runs differ from the quiet run while another stream is busy"


# ------------------------------------------------------------------------------------------------- checkpoints
def test_reference_written_checkpoint_samples_like_the_reference(golden, tmp_path):
    """tests/golden/ckpt_micro.pth was written by the reference's own ``Diffusion.train_step``
    (oracle/make_golden.py::g9_checkpoint).  Loaded here with ``strict=True`` plus the EMA swap-in
    (runners/diffusion.py:293-313,331), the HIP path must reproduce the forward and the 10-step DDIM trajectory that the
    reference itself produced from that file."""
    import shutil
    from ddim_audio_amd import checkpoint
    g = golden("ckpt")
    shutil.copyfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_micro.pth"), tmp_path / "ckpt.pth")
    cfg = configs.micro_config("torch.cuda.FloatTensor")
    m, ema = checkpoint.load_for_sampling(str(tmp_path), D.Model(cfg), use_ema=True, ema_rate=cfg.model.ema_rate, map_location="cuda")
    assert not m.training
    with torch.no_grad():
        y = m(synth.gaussian("ckpt.fwd.x", (2, 2, 8, 8)).cuda(), torch.tensor([3, 777]).cuda())
    G.check_close(y.cpu(), g["ema_model_y"], G.F32, "forward from the reference-written checkpoint")
    alphas = make_schedule(cfg.diffusion)[1]
    xs, x0 = D.generalized_steps(synth.gaussian("ckpt.sample.x", (2, 2, 8, 8)).cuda(), list(range(0, 1000, 100)), m, alphas, None, eta=0.0)
    G.check_close(xs[-1], g["sample_final"], G.F32, "sample from the reference-written checkpoint", scale=10.0)
    G.check_close(x0[-1], g["sample_x0_last"], G.F32, "x0 prediction from the reference-written checkpoint", scale=10.0)


def test_training_resume_is_bit_exact(tmp_path):
    """Fixed-forward resume (runners/diffusion.py:239-254): train 2 steps, save, train a 3rd (A); a fresh model + state resumed
    from the file trains the same 3rd step (B).  A and B must agree bit for bit -- both optimizers' moments and step counts,
    both LambdaLR schedulers, the EMA shadow and the dropout call counter (bf16 mode, dropout 0.1) all travel."""
    from ddim_audio_amd import checkpoint, train
    d = configs.tiny_dict("torch.cuda.BFloat16Tensor")
    d["optimization"]["optimizer"]["default"]["optimizer"] = "AdamW"
    d["optimization"]["optimizer"]["default"]["warmup"] = 3
    cfg = configs.dict2namespace(d)
    alphas = make_schedule(cfg.diffusion)[1].cuda()
    xs = [synth.gaussian(f"resume.x{i}", (4, 2, 32, 32)).cuda() for i in range(3)]
    es = [synth.gaussian(f"resume.e{i}", (4, 2, 32, 32)).cuda() for i in range(3)]
    ts = [torch.tensor([10 + i, 500, 989 - i, 250]) for i in range(3)]
    torch.manual_seed(77)
    m = synth.fill_module(D.Model(cfg), 11)
    st = train.TrainingState(cfg, m)
    for i in range(2):
        train.train_step(m, xs[i], st, alphas, e=es[i], t=ts[i])
    checkpoint.save_checkpoint(str(tmp_path), m, st.optimizers, 0, 2, st.ema_helper, st.schedulers)
    loss_a, _ = train.train_step(m, xs[2], st, alphas, e=es[2], t=ts[2])
    m2 = D.Model(cfg)
    st2 = train.TrainingState(cfg, m2)
    assert checkpoint.resume_training(str(tmp_path), m2, st2.optimizers, st2.schedulers, st2.ema_helper, map_location="cuda") == (0, 2)
    loss_b, _ = train.train_step(m2, xs[2], st2, alphas, e=es[2], t=ts[2])
    assert float(loss_a) == float(loss_b)
    for (n, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), n
        assert torch.equal(st.ema_helper.shadow[n], st2.ema_helper.shadow[n]), n
    for k in st.optimizers:
        assert st.optimizers[k].param_groups[0]["lr"] == st2.optimizers[k].param_groups[0]["lr"]


def test_staged_backward_buckets_are_final_when_their_event_fires():
    """ddimx_unet_bwd_staged (data-parallel overlap): the three gradient buckets -- up_modules.*, transformer.*,
    temb.* + down_modules.* -- must be complete when their HIP event fires, because the all-reduce of a bucket starts then,
    while the rest of the backward is still running.  A stand-in ``grad_sync`` snapshots each bucket on a side stream behind
    its event; the snapshots must equal the final buffer, the result must equal the plain backward bit for bit, and the
    ranges must tile the flat buffer by parameter name."""
    cfg, m = MH.build("audio", "torch.cuda.BFloat16Tensor", 0, mode="train", dropout=0.0, optimizer="AdamW")
    alphas = make_schedule(cfg.diffusion)[1].cuda()
    shape = (4, 2, 256, 256)
    x0, e = synth.gaussian("staged.x0", shape).cuda(), synth.gaussian("staged.e", shape).cuda()
    t = torch.tensor([5, 994, 300, 650]).cuda()
    losses.noise_estimation_loss(m, x0, t, e, alphas).backward()
    plain = m._flat_grad.clone()
    m.zero_grad(set_to_none=True)
    seen = {}

    def staged(flat, ranges, events):
        side = torch.cuda.Stream()
        seen["ranges"] = ranges
        seen["snaps"] = []
        for (lo, hi), ev in zip(ranges, events):
            side.wait_event(ev)
            with torch.cuda.stream(side):
                seen["snaps"].append(flat[lo:hi].clone())
        torch.cuda.current_stream().wait_stream(side)
        return flat

    sync = lambda flat: flat  # noqa: E731
    sync.staged, sync.active = staged, (lambda: True)
    m.grad_sync = sync
    losses.noise_estimation_loss(m, x0, t, e, alphas).backward()
    torch.cuda.synchronize()
    flat = m._flat_grad
    # (bitwise: unowned words of the buffer -- alignment padding -- may hold NaN patterns left by other tests' poison)
    assert torch.equal(flat.view(torch.int32), plain.view(torch.int32)), "the staged backward must compute the same gradients"
    (a0, b0), (a1, b1), (a2, b2) = seen["ranges"]
    assert a2 == 0 and b2 == a0 and b0 == a1 and b1 == flat.numel()
    for snap, (lo, hi) in zip(seen["snaps"], seen["ranges"]):
        assert torch.equal(snap.view(torch.int32), flat[lo:hi].view(torch.int32)), "a bucket changed after its event fired"
    total, layout = m._grad_layout(__import__("ddim_audio_amd")._lib.load())
    for (name, _), (off, numel, _) in zip(m.named_parameters(), layout):
        b = 0 if name.startswith("up_modules.") else (1 if name.startswith("transformer.") else 2)
        lo, hi = seen["ranges"][b]
        assert lo <= off and off + numel <= hi, name


@pytest.mark.parametrize("mode", MODES, ids=["f32", "bf16"])
def test_forked_backward_is_bit_identical_to_the_one_stream_backward(mode):
    """ddimx_unet_bwd_forked: the weight gradients leave the data-gradient chain for a second stream (each behind an event, reading
    the branch's own two ``du`` buffers, which the chain may only overwrite behind the event of their last reader).  Same kernels,
    same partitions, same order of additions: every gradient must carry the bits of the one-stream backward -- at two shapes (so
    that both the full-chip and the launch-bound levels race if anything can), five times over with the gradient buffer and the
    workspace poisoned in between, and with kernels of another stream in flight."""
    dtype_str, dt = mode
    cfg, m = MH.build("audio", dtype_str, 0, mode="train", dropout=0.0, optimizer="AdamW")
    alphas = make_schedule(cfg.diffusion)[1].cuda()
    for shape, tt in (((4, 2, 256, 256), [5, 994, 300, 650]), ((2, 2, 32, 256), [0, 999])):
        x0, e = synth.gaussian("bwdfork.x0", shape).cuda(), synth.gaussian("bwdfork.e", shape).cuda()
        t = torch.tensor(tt).cuda()
        m.bwd_fork = False
        loss = losses.noise_estimation_loss(m, x0, t, e, alphas)
        m._train_ws.fill_(0xFF)  # the backward takes nothing from the forward's scratch: the tape holds what it needs
        loss.backward()
        plain = {n: p.grad.clone() for n, p in m.named_parameters()}
        assert all(bool(torch.isfinite(g).all()) for g in plain.values())
        lib = __import__("ddim_audio_amd")._lib.load()
        assert int(lib.ddimx_bwd_side_events(m._handle)) == 4 * 2 * sum(cfg.model.res) + 2 * (len(cfg.model.ch) - 1) + 3
        m.zero_grad(set_to_none=True)
        m.bwd_fork = True
        other = torch.cuda.Stream()
        junk = torch.randn(1 << 22, device="cuda")
        for rep in range(5):
            m._flat_grad.fill_(float("nan"))
            loss = losses.noise_estimation_loss(m, x0, t, e, alphas)
            m._train_ws.fill_(0xFF)  # NaN patterns in every buffer of the backward, `du` and the slabs included
            if rep % 2:
                with torch.cuda.stream(other):
                    for _ in range(20):
                        junk = junk * 1.0001
            loss.backward()
            torch.cuda.synchronize()
            for n, p in m.named_parameters():
                assert torch.equal(p.grad, plain[n]), (shape, rep, n)
            m.zero_grad(set_to_none=True)


@pytest.mark.parametrize("mode", MODES, ids=["f32", "bf16"])
def test_forked_forward_is_bit_identical_for_every_mask(mode):
    """ddimx_unet_fwd_forked: any subset of levels / the FNet run as two batch shards on two streams must give the bits of the
    plain forward (every op is per sample, the launch plan depends on the sample's size only) -- eagerly, for an odd batch,
    and replayed from a hipGraph with the second stream captured through the fork / join events."""
    dtype_str, dt = mode
    cfg, m = MH.build("audio", dtype_str, 0, mode="eval")
    x = synth.gaussian("fork.x", (5, 2, 64, 256)).cuda()
    t = torch.tensor([0, 999, 123, 500, 7]).cuda()
    with torch.no_grad():
        m.fork_mask = 0
        ref = m(x, t).clone()
        for mask in (0x1, 0x3, 0x10000, 0x10003, 0x24, 0x1003F):
            m.fork_mask = mask
            assert torch.equal(m(x, t), ref), hex(mask)
            assert torch.equal(m(x[:4], t[:4]), ref[:4]), hex(mask)
        m.fork_mask = 0x10003
        g = torch.cuda.CUDAGraph()
        xs, ts = x.clone(), t.clone()
        m(xs, ts)
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            ys = m(xs, ts)
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(ys, ref)
        xs.copy_(x.flip(0)); ts.copy_(t.flip(0))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(ys, ref.flip(0))


@pytest.mark.parametrize("default_opt", ["AdamW", "AdaBelief"])
def test_graphed_train_step_is_bit_identical_to_eager(default_opt):
    """train.GraphedTrainStep: two eager warm-up steps, one capture, four replays must leave exactly what six eager steps leave
    -- parameters, EMA shadow, Adam moments and step counts, LambdaLR state, the dropout call counter -- and return the same
    losses.  bf16 mode with dropout 0.1 and a 3-step LR warm-up, so the per-step scalars that live in device memory under replay
    (learning rate, bias corrections, dropout counter) all change between replays."""
    from ddim_audio_amd import train
    d = configs.tiny_dict("torch.cuda.BFloat16Tensor")
    d["optimization"]["optimizer"]["default"]["optimizer"] = default_opt  # AdaBelief: the reference's default group (kernel mode 2)
    d["optimization"]["optimizer"]["default"]["warmup"] = 3
    cfg = configs.dict2namespace(d)
    alphas = make_schedule(cfg.diffusion)[1].cuda()
    n = 6
    xs = [synth.gaussian(f"graphed.x{i}", (4, 2, 32, 32)).cuda() for i in range(n)]
    es = [synth.gaussian(f"graphed.e{i}", (4, 2, 32, 32)).cuda() for i in range(n)]
    ts = [torch.tensor([10 + i, 500, 989 - i, 250]) for i in range(n)]

    def run(graphed):
        torch.manual_seed(77)
        m = synth.fill_module(D.Model(cfg), 11)
        st = train.TrainingState(cfg, m)
        step = train.GraphedTrainStep(m, st, alphas, warmup=2) if graphed else None
        losses = []
        for i in range(n):
            if graphed:
                loss, _ = step(xs[i], e=es[i], t=ts[i])
            else:
                loss, _ = train.train_step(m, xs[i], st, alphas, e=es[i], t=ts[i])
            losses.append(float(loss))
        if graphed:
            assert step.graph is not None
            step.close()
            # back to eager: one more step must continue the same trajectory
        loss, _ = train.train_step(m, xs[0], st, alphas, e=es[1], t=ts[2])
        losses.append(float(loss))
        return m, st, losses

    ma, sa, la = run(False)
    mb, sb, lb = run(True)
    assert la == lb, (la, lb)
    assert ma._dropout_calls == mb._dropout_calls == n + 1
    for (name, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a, b), name
        assert torch.equal(sa.ema_helper.shadow[name], sb.ema_helper.shadow[name]), name
    for k in sa.optimizers:
        oa, ob = sa.optimizers[k], sb.optimizers[k]
        assert oa.param_groups[0]["lr"] == ob.param_groups[0]["lr"]
        for pa, pb in zip(oa.param_groups[0]["params"], ob.param_groups[0]["params"]):
            assert oa.state[pa]["step"] == ob.state[pb]["step"] == n + 1
            assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"])
            assert torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])
    for k in sa.schedulers:
        assert sa.schedulers[k].state_dict()["last_epoch"] == sb.schedulers[k].state_dict()["last_epoch"]


# ------------------------------------------------------------------------------- round 3: ownership / coverage gaps
def test_stepper_owns_what_its_graph_references_and_recaptures_when_the_model_moves_on():
    """DESIGN 9a (round 3).  (1) The graph's buffers and event set belong to the stepper: dropping every other reference to
    the model's derived buffers (``_apply`` does exactly that) must not free what a live graph points at, and the next step
    must notice the new generation, run eagerly and re-capture -- same trajectory, bit for bit, as an undisturbed run.
    (2) A repack in between (``invalidate``) is picked up by the replayed graph: the embedding table is rebuilt IN PLACE.
    (3) ``close`` destroys the graph before the events; a closed stepper keeps stepping eagerly."""
    from ddim_audio_amd.sampler import DDIMStepper
    from ddim_audio_amd import schedule
    cfg, m = MH.build("audio", "torch.cuda.BFloat16Tensor", 0, mode="eval")
    alphas = make_schedule(cfg.diffusion)[1]
    seq = list(range(0, 1000, 100))
    coef = schedule.ddim_coefficients(seq, alphas, 0.0)
    x = synth.gaussian("own.x", (5, 2, 64, 256)).cuda()

    def run(disturb):
        xt = x.clone()
        st = DDIMStepper(m, xt, coef, use_graph=True)
        for i in range(len(seq)):
            disturb(i, st)
            st.step()
        torch.cuda.synchronize()
        out = (xt.clone(), st.x0.clone(), st.captures)
        st.close()
        assert st.graph is None and st._ctx is None and st._refs is None
        return out

    ref = run(lambda i, st: None)
    assert ref[2] == 1

    def move(i, st):
        if i == 4:
            assert st.graph is not None and st._ctx is not None and len(st._refs) >= 5
            m.float()  # nn.Module._apply: the model drops its packed weights, tables, workspaces, embedding table
            assert m._packed is None and m._workspace is None
            junk = [torch.full((1 << 20,), float("nan"), device="cuda") for _ in range(8)]  # would land in freed blocks
            del junk
    got = run(move)
    assert got[2] == 2, "the stepper must re-capture after the model re-allocated its buffers"
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])

    def repack(i, st):
        if i == 4:
            tb = m._temb_buf.data_ptr()
            m.invalidate()
            st._tb = tb
        if i == 5:
            assert m._temb_buf.data_ptr() == st._tb and not m._dirty
    got = run(repack)
    assert got[2] == 1, "a repack must not need a new capture: every buffer is rebuilt in place"
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])

    # (3) a closed stepper keeps working (eagerly, then captures again)
    xt = x.clone()
    st = DDIMStepper(m, xt, coef, use_graph=True)
    for i in range(len(seq)):
        if i == 3:
            st.close()
        st.step()
    torch.cuda.synchronize()
    assert torch.equal(xt, ref[0])
    st.close()


def test_graphed_train_step_with_device_resident_inputs_and_no_host_reads():
    """the per-step scalars of GraphedTrainStep went through ONE pinned buffer uploaded asynchronously; with
    device-resident ``t`` and nobody reading the loss between replays the host runs several replays ahead, and step k's
    upload could carry step k+1's learning rate / bias corrections / dropout counter.  Now a ring of event-guarded pinned
    slots: six replays without any host synchronisation must leave exactly the state of six eager steps."""
    from ddim_audio_amd import train
    cfg = configs.tiny_config("torch.cuda.FloatTensor")
    cfg.optimization.optimizer.default.optimizer = "AdamW"
    cfg.optimization.optimizer.default.warmup = 3     # the learning rate changes every step
    alphas = make_schedule(cfg.diffusion)[1].cuda()
    n = 8
    xs = [synth.gaussian(f"ring.x{i}", (4, cfg.model.channels, 32, cfg.model.f_size)).cuda() for i in range(n)]
    es = [synth.gaussian(f"ring.e{i}", (4, cfg.model.channels, 32, cfg.model.f_size)).cuda() for i in range(n)]
    ts = [torch.tensor([7 + i, 992 - i, 300 + i, 699 - i], device="cuda") for i in range(n)]

    def make():
        torch.manual_seed(11)
        m = synth.fill_module(D.Model(cfg), 5)
        return m, train.TrainingState(cfg, m)

    m1, s1 = make()
    for i in range(n):
        train.train_step(m1, xs[i], s1, alphas, e=es[i], t=ts[i])
    m2, s2 = make()
    step = train.GraphedTrainStep(m2, s2, alphas, warmup=2)
    for i in range(n):
        step(xs[i], e=es[i], t=ts[i])      # device-resident t, the returned loss is never read
    torch.cuda.synchronize()
    step.close()
    for (k, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), k
    for k in s1.ema_helper.shadow:
        assert torch.equal(s1.ema_helper.shadow[k], s2.ema_helper.shadow[k]), k
    # the hooks of the capture are gone: an eager step on the same model / state continues the same trajectory
    train.train_step(m1, xs[0], s1, alphas, e=es[0], t=ts[0])
    train.train_step(m2, xs[0], s2, alphas, e=es[0], t=ts[0])
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), k


def test_graphed_train_step_keeps_its_tables_and_recaptures_when_the_model_reallocates():
    """the train graph points at the posenc / DFT tables too, and ``Model._tables`` keeps only the latest T -- an eval
    forward at another length between replays used to free tables the graph still read.  Now the graph's owner keeps
    ``Model.captured_refs()`` next to the graph, records ``Model._gen`` at capture and captures again when it moved: six graphed
    steps with an eval forward at another T in the middle must leave exactly the state of six eager steps (and two captures)."""
    from ddim_audio_amd import train
    cfg = configs.tiny_config("torch.cuda.FloatTensor")
    cfg.optimization.optimizer.default.optimizer = "AdamW"
    alphas = make_schedule(cfg.diffusion)[1].cuda()
    n = 6
    xs = [synth.gaussian(f"regen.x{i}", (4, cfg.model.channels, 32, cfg.model.f_size)).cuda() for i in range(n)]
    es = [synth.gaussian(f"regen.e{i}", (4, cfg.model.channels, 32, cfg.model.f_size)).cuda() for i in range(n)]
    ts = [torch.tensor([7 + i, 992 - i, 300 + i, 699 - i], device="cuda") for i in range(n)]
    other = synth.gaussian("regen.other", (2, cfg.model.channels, 64, cfg.model.f_size)).cuda()

    def make():
        torch.manual_seed(11)
        m = synth.fill_module(D.Model(cfg), 5)
        return m, train.TrainingState(cfg, m)

    def disturb(m):
        m.eval()
        with torch.no_grad():
            m(other, torch.tensor([3, 500], device="cuda"))   # another T: new tables, new workspace -> the generation moves
        junk = [torch.full((1 << 18,), float("nan"), device="cuda") for _ in range(8)]  # would land in freed blocks
        del junk
        m.train()

    m1, s1 = make()
    for i in range(n):
        if i == 4:
            disturb(m1)
        train.train_step(m1, xs[i], s1, alphas, e=es[i], t=ts[i])
    m2, s2 = make()
    step = train.GraphedTrainStep(m2, s2, alphas, warmup=1)
    captures = 0
    for i in range(n):
        if i == 4:
            assert step.graph is not None
            disturb(m2)
        had = step.graph is not None
        step(xs[i], e=es[i], t=ts[i])
        captures += int(step.graph is not None and (not had or i == 4))
    torch.cuda.synchronize()
    assert captures == 2, captures
    step.close()
    for (k, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), k


def test_graphed_train_step_keeps_the_clip_norm_tables_it_captured():
    """the train graph reads the clip-norm pointer tables of ``optim._clip_cache``, a one-entry cache that the next
    gradient set to be clipped empties.  The graph's owner keeps the entry its capture used next to the graph: with the cache
    cleared and the freed blocks sprayed with NaNs between replays, six graphed steps still leave exactly the state of six eager
    steps, from one capture."""
    from ddim_audio_amd import optim, train
    cfg = configs.tiny_config("torch.cuda.FloatTensor")
    cfg.optimization.optimizer.default.optimizer = "AdamW"
    alphas = make_schedule(cfg.diffusion)[1].cuda()
    n = 6
    xs = [synth.gaussian(f"clip.x{i}", (4, cfg.model.channels, 32, cfg.model.f_size)).cuda() for i in range(n)]
    es = [synth.gaussian(f"clip.e{i}", (4, cfg.model.channels, 32, cfg.model.f_size)).cuda() for i in range(n)]
    ts = [torch.tensor([7 + i, 992 - i, 300 + i, 699 - i], device="cuda") for i in range(n)]

    def make():
        torch.manual_seed(11)
        m = synth.fill_module(D.Model(cfg), 5)
        return m, train.TrainingState(cfg, m)

    m1, s1 = make()
    for i in range(n):
        train.train_step(m1, xs[i], s1, alphas, e=es[i], t=ts[i])
    m2, s2 = make()
    step = train.GraphedTrainStep(m2, s2, alphas, warmup=1)
    for i in range(n):
        if i == 3:
            assert step.graph is not None and len(optim._clip_cache) == 1
            (tb,) = optim._clip_cache.values()
            for v in tb.ptrs + [tb.sizes, tb.bt, tb.bo, tb.partial, tb.out]:
                assert any(r is v for r in step._refs), "the graph's owner must keep the clip-norm tables of its capture"
            torch.cuda.synchronize()
            optim._clip_cache.clear()
            del tb, v
            junk = [torch.full((1 << 18,), float("nan"), device="cuda") for _ in range(8)]  # would land in freed blocks
            del junk
        step(xs[i], e=es[i], t=ts[i])
    torch.cuda.synchronize()
    assert step.captures == 1
    step.close()
    for (k, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), k
    for k in s1.ema_helper.shadow:
        assert torch.equal(s1.ema_helper.shadow[k], s2.ema_helper.shadow[k]), k
