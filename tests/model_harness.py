"""What the feature GPU tests (tests/test_gpu_{train,train_exact,vpred,distill,solver,sde,unic,brownian,threshold,inpaint,
inpaint_solver,invert,input_grad,window,window_solver,window_inpaint,pool,noise,model,configs,ops,walk_scratch,wiring,zz_rccl}.py) share,
once.  The CPU tests take the schedule from here too (``alphas``), and tests/pool_ref.py the uneven sequences (``spread``).

* constants: the mode table, the fp32 unit roundoff and smallest normal, the sentinel pattern, the (B, per_sample) kernel cases;
* models: ``config_dict`` / ``build`` (the seeded model builder), ``alphas``, ``pair`` (the v / simple twin), ``rb_sd``;
* the CPU oracle and its gates: ``oracle``, ``gate``, ``backward_case`` (loss and every parameter gradient);
* running and buffers: ``eager_steps``, ``sentinel`` / ``bits``, ``stepper_run`` (a stepper's loop, closed twice, nothing left);
* inputs: ``spread`` (uneven timesteps), ``pair_data`` (the inpainting tests' x and y);
* eps callables: ``oracle_eps`` (torch, differentiable), ``oracle_eps_np`` (float64 numpy), ``v_wrapped`` (the twin read as v);
* exact comparisons of runs: ``same_run``, ``same_list``, ``differs``, ``differs_anywhere``, ``known_exact``.

A test module takes these from here and never from another test module; what one file alone uses stays in that file."""
import contextlib
import os

import numpy as np
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, configs, synth
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


def stepper_run(make_stepper, n_steps, disturb=None, keep=None):
    """``n_steps`` steps of the stepper ``make_stepper()`` builds, ``disturb(i)`` before step i: (outs, captures, has_graph) with
    outs[i] = clones of (xt, x0) after step i, read before the close -- and ``keep(st)`` as a fourth, when given.  Closing twice is
    harmless and leaves no graph, capture context or reference behind."""
    outs = []
    with torch.no_grad():
        st = make_stepper()
        try:
            for i in range(n_steps):
                if disturb is not None:
                    disturb(i)
                st.step()
                outs.append((st.xt.clone(), st.x0.clone()))
            torch.cuda.synchronize()
            captures, has_graph = st.captures, st.graph is not None
            kept = None if keep is None else keep(st)
        finally:
            st.close()
            st.close()  # twice is harmless
    assert st.graph is None and st._ctx is None and st._refs is None
    return (outs, captures, has_graph) if keep is None else (outs, captures, has_graph, kept)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def spread(n):
    """n increasing timesteps in 0..999, uneven on purpose (the step ratios r0, r1 differ from row to row), starting at 0; one
    step: a single mid-schedule level."""
    return [400] if n == 1 else sorted({int(round(999 * (i / (n - 1)) ** 1.7)) for i in range(n)})


def pair_data(tag, shape):
    """(x, y) of the inpainting tests: the seeded Gaussians ``tag``.x and ``tag``.y."""
    return synth.gaussian(tag + ".x", shape), synth.gaussian(tag + ".y", shape)


# ---- eps callables --------------------------------------------------------------------------------------------------------------------------
def oracle_eps(m, name="tiny"):
    """eps(x, t) of the CPU oracle with ``m``'s weights, in torch: fp32 forward, the result in x's dtype, differentiable w.r.t. x.
    Further positional arguments (a window index) are ignored."""
    live, ocfg = oracle(m, name)
    sd = {k: v.detach() for k, v in live.items()}
    return lambda x, t, *_: ref_cpu.model_forward(sd, ocfg, x.float(), t).to(x.dtype)


def oracle_eps_np(m, name="tiny"):
    """``oracle_eps`` for the float64 numpy references: eps(x [B, ...] array, t int) -> float64 array, no gradient.  Further
    positional arguments (a window index) are ignored."""
    fn = oracle_eps(m, name)

    def eps(x, t, *_):
        with torch.no_grad():
            xt = torch.from_numpy(np.ascontiguousarray(x)).float()
            return fn(xt, torch.full((xt.size(0),), int(t), dtype=torch.long)).double().numpy()

    return eps


def v_wrapped(ms, table64, record=False):
    """A plain callable (no ``forward_slot``: the samplers call it as ``model(x, t)``, eagerly) that returns the eps of the
    ``type: simple`` twin's output read as v: ``ms``' unforked forward, then ddimx_v_to_eps with the fp32 of ``table64``
    (``schedule.v_table``).  ``record``: ``model.outputs`` holds every (eps it returned, a clone made at once), for a caller that
    checks afterwards that the callable's tensors were never rewritten."""
    vt = torch.from_numpy(np.ascontiguousarray(table64, dtype=np.float32)).to(G.dev())
    lib = _lib.load()

    def model(x, t):
        v = ms(x, t, _fork=False)
        eps = torch.empty_like(v)
        _lib.check(lib.ddimx_v_to_eps(_lib.ptr(x), _lib.ptr(v), _lib.ptr(eps), _lib.ptr(vt), vt.size(0), _lib.ptr(t), x.size(0),
                                      x[0].numel(), _lib.stream()))
        if record:
            model.outputs.append((eps, eps.clone()))
        return eps

    model.outputs = []
    assert not hasattr(model, "forward_slot") and not hasattr(model, "prediction")
    return model


# ---- exact comparisons of runs ------------------------------------------------------------------------------------------------------------
def same_list(got, want, what):
    """Two lists of tensors, equal in length and element for element bit for bit (on whichever device each lives)."""
    assert len(got) == len(want), f"{what}: {len(got)} entries against {len(want)}"
    for i, (u, v) in enumerate(zip(got, want)):
        assert torch.equal(u.cpu(), v.cpu()), f"{what}[{i}]"


def same_run(got, want, what):
    """Two (xs, x0_preds) pairs of a sampler: equal lengths, at least one prediction, every xs[1:] and every prediction bit for
    bit (xs[0] is the caller's input)."""
    (xs, x0), (wxs, wx0) = got, want
    assert len(xs) == len(wxs) and len(x0) == len(wx0) and len(x0) >= 1, f"{what}: {len(xs)}, {len(x0)} entries against {len(wxs)}, {len(wx0)}"
    same_list(x0, wx0, f"{what}: x0_preds")
    for i in range(1, len(xs)):
        assert torch.equal(xs[i].cpu(), wxs[i].cpu()), f"{what}: xs[{i}]"


def differs(got, want):
    """The runs part before the end: xs[-2] (the last sample that is not the final prediction) differs."""
    return not torch.equal(got[0][-2], want[0][-2])


def differs_anywhere(got, want):
    """Some xs[1:] differs."""
    return any(not torch.equal(u, v) for u, v in zip(got[0][1:], want[0][1:]))


def known_exact(last, y, mask):
    """The mask has a known element, and where it is 1 the final sample holds y's bits."""
    k = torch.broadcast_to(mask, last.shape) == 1
    assert bool(k.any()), "the mask has no known element"
    assert torch.equal(last[k], torch.broadcast_to(y, last.shape)[k]), "the known region of the final sample is not y exactly"
