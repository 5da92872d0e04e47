"""What the feature GPU tests (tests/test_gpu_{train,vpred,distill,solver,inpaint,invert,input_grad,window,pool,noise,model,configs,ops,
zz_rccl}.py) share, once: the mode table and the fp32 constants, the seeded model builder, the schedule, the v / simple twin, the
whole-network gates against the CPU oracle, the eager-steps switch, the sentinel buffer, and the loss-and-gradients case.  A test
module takes these from here and never from another test module; what one file alone uses stays in that file."""
import contextlib
import os

import torch

import ddim_audio_amd as D
from ddim_audio_amd import configs, synth
from ddim_audio_amd.schedule import make_schedule
from oracle import ref_cpu
import gpu_util as G

MODES = [("torch.cuda.FloatTensor", G.F32), ("torch.cuda.BFloat16Tensor", G.BF16)]
MODE_IDS = ["f32", "bf16"]
U = 2.0 ** -24       # unit roundoff of fp32
TINY = 2.0 ** -126   # smallest normal fp32: covers an underflowing intermediate, per rounding
PATTERN = 0x7FC0BEEF  # a NaN with a payload: any arithmetic on it, or any store over it, shows
# (B, per_sample) of the per-sample elementwise kernels (v-prediction, distillation), and the table rows their samples take
N_STRIDE = 4 * (2048 * 256 + 1000)  # more float4s in one sample than the grid has threads: the grid-stride loop runs twice
KERNEL_CASES = [(3, 20), (2, 4 * 5132), (1, N_STRIDE)]
KERNEL_IDS = ["sub_block", "ragged", "grid_stride"]
ROWS = [0, 412, 999]


# ---- models ---------------------------------------------------------------------------------------------------------------------------
def config_dict(name, dtype_str, *, kind=None, dropout=None, optimizer=None, loss_weight=None, fnet=None):
    """``configs.tiny_dict`` / ``audio_dict`` with the keys edited whose argument is given; None leaves a key as ``configs`` made it."""
    d = (configs.tiny_dict if name == "tiny" else configs.audio_dict)(dtype_str, fnet)
    if kind is not None:
        d["model"]["type"] = kind
    if dropout is not None:
        d["model"]["transformers"]["kwargs"]["hidden_dropout_prob"] = dropout
    if optimizer is not None:
        d["optimization"]["optimizer"]["default"]["optimizer"] = optimizer
    if loss_weight is not None:
        d["model"]["loss_weight"] = loss_weight
    return d


def build(name, dtype_str, seed, *, mode, **edits):
    """(cfg, model): ``D.Model`` of ``config_dict(name, dtype_str, **edits)`` filled by ``synth.fill_module(m, seed)``; ``mode`` is
    "eval", "train" or None (as constructed)."""
    cfg = configs.dict2namespace(config_dict(name, dtype_str, **edits))
    m = synth.fill_module(D.Model(cfg), seed)
    if mode is not None:
        m = {"train": m.train, "eval": m.eval}[mode]()
    return cfg, m


def alphas(cfg=None):
    return make_schedule((cfg or configs.audio_config()).diffusion)[1]


_PAIRS = {}


def pair(name, dtype_str):
    """(cfg, Mv, Ms, alphas): a model of type v and its ``type: simple`` twin over the same weights, eval mode, once per case and
    process."""
    key = (name, dtype_str)
    if key not in _PAIRS:
        cfg, mv = build(name, dtype_str, 5, mode="eval", kind="v")
        _, ms = build(name, dtype_str, 5, mode="eval", kind="simple")
        assert mv.prediction == "v" and ms.prediction == "eps"
        _PAIRS[key] = (cfg, mv, ms, alphas(cfg))
    return _PAIRS[key]


def rb_sd(p, c):
    shapes = {p + "norm.0.weight": (c,), p + "norm.0.bias": (c,), p + "norm.1.weight": (c,), p + "norm.1.bias": (c,),
              p + "norm.2.weight": (c,), p + "conv.0.weight": (c, c, 3, 3), p + "conv.1.weight": (c, c, 3, 3),
              p + "conv.1.bias": (c,)}
    return synth.fill_state_dict({k: torch.empty(s) for k, s in shapes.items()})


# ---- the oracle and its gate ----------------------------------------------------------------------------------------------------------
def oracle(m, name):
    """(live state dict with leaf parameters, the oracle's fp32 config) for autograd through ref_cpu.model_forward."""
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k != "temb.te"}
    live = dict(params, **{"temb.te": sd["temb.te"]})
    ocfg = configs.dict2namespace(configs.tiny_dict("torch.FloatTensor") if name == "tiny" else configs.audio_dict("torch.FloatTensor"))
    return live, ocfg


def gate(got, ref, dt, what):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert torch.isfinite(got).all(), what
    rms = float(ref.square().mean().sqrt())
    d = got - ref
    mx, er = float(d.abs().max()) / rms, float(d.square().mean().sqrt()) / rms
    if dt == G.F32:
        assert mx <= 2e-3, f"{what}: max {mx:.3e} x rms"
    else:
        assert mx <= 0.6 and er <= 5e-2, f"{what}: max {mx:.3e}, rms err {er:.3e} x rms"
    return mx, er


def backward_case(mode, shape, tt, *, build_model, loss, ref_loss, forward=None, name="tiny"):
    """Loss and every parameter gradient of the network ``name`` (the tiny one by default) against autograd through the CPU oracle.
    ``build_model(name, dtype_str, seed) -> (cfg, train-mode model)``; ``loss(m, x0, t, e, alphas)`` is the loss under test, on the GPU;
    ``ref_loss(model_fn, x0, t, e, alphas)`` the reference, on the CPU; ``forward(live, ocfg, x, t) -> eps`` the oracle's forward under
    it, ``ref_cpu.model_forward`` by default (a test with dropout on passes one that hands the oracle the library's masks).  Gates: the
    loss within 1e-5 (fp32) / 2e-3 (bf16) relative; each gradient's worst element within 2e-3 / 0.6 of the tensor's own RMS gradient
    (floor: a 1e-4 share of the global norm)."""
    dtype_str, dt = mode
    forward = forward or ref_cpu.model_forward
    cfg, m = build_model(name, dtype_str, 5)
    a = alphas(cfg)
    x0, e = synth.gaussian("ragged.x0", shape), synth.gaussian("ragged.e", shape)
    t = torch.tensor(tt)
    got = loss(m, x0.cuda(), t.cuda(), e.cuda(), a.cuda())
    got.backward()
    live, ocfg = oracle(m, name)
    params = {k: v for k, v in live.items() if k != "temb.te"}
    want = ref_loss(lambda xx, ts: forward(live, ocfg, xx, ts), x0, t, e, a)
    want.backward()
    lerr = abs(float(got) - float(want)) / float(want)
    assert lerr <= (1e-5 if dt == G.F32 else 2e-3), f"loss {float(got)!r} vs {float(want)!r}: rel. err {lerr:.3e}"
    total = sum(float(p.grad.double().square().sum()) for p in params.values()) ** 0.5
    worst = 0.0
    for pname, p in m.named_parameters():
        ref = params[pname].grad
        grad = p.grad.detach().cpu()
        scale = max(float(ref.double().square().mean().sqrt()), 1e-4 * total / ref.numel() ** 0.5)
        err = float((grad - ref).abs().max()) / scale
        worst = max(worst, err)
        assert err <= (2e-3 if dt == G.F32 else 0.6), f"{pname}: {err:.3e} x rms"
    print(f"[backward ragged {name} {shape} {'f32' if dt == G.F32 else 'bf16'}] loss rel. err {lerr:.3e}, worst element {worst:.3e} x rms")


# ---- running and buffers ----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def eager_steps():
    """Inside the block every sampler step is launched eagerly (DDIMX_GRAPH=0); afterwards the variable is as it was before."""
    before = os.environ.get("DDIMX_GRAPH")
    os.environ["DDIMX_GRAPH"] = "0"
    try:
        yield
    finally:
        if before is None:
            del os.environ["DDIMX_GRAPH"]
        else:
            os.environ["DDIMX_GRAPH"] = before


def sentinel(b, per, device=None):
    """A [b, per] fp32 buffer with PATTERN in every word."""
    return torch.full((b, per), PATTERN, dtype=torch.int32, device=G.dev() if device is None else device).view(torch.float32)


def bits(t):
    return t.view(torch.int32)
