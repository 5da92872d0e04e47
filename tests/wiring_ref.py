"""What the wiring tests (tests/test_wiring_cpu.py, tests/test_gpu_wiring.py) share: is every parameter read where the reference reads
it, from a copy built from that parameter?

* the response statistic: parameter i of the weights theta is replaced by ``draw(name, p)``; with D_ref = y_ref(theta_i) - y_ref(theta)
  from the CPU oracle and D_got likewise from the walk under test, ``projection(D_got, D_ref)`` = <D_got, D_ref> / <D_ref, D_ref> is
  about 1 where the walk reads the parameter as the oracle does and about 0 where it ignores it or reads it at another layer.  The
  bounds [0.5, 1.5] are the midpoint between those two hypotheses, not a measured tolerance;
* ``noise``: what the project's own gate g (rms error of an output / rms of the output) allows that statistic to scatter by if the
  error is white: both outputs carry an error of rms g * rms(y), so D_got - D_ref has one of sqrt(2) g rms(y), and its projection on
  the unit vector along D_ref (N elements, rms m * rms(y)) has standard deviation sqrt(2) g / (m sqrt(N)).  The tests require that
  to be at most ``N_MAX`` = 0.05, a factor of ten below the halfway point, which leaves room for spatially correlated rounding
  errors; it is asserted from the oracle's numbers alone, before the walk's result is judged;
* ``AMP``: the draws that need a larger amplitude (x 4, then x 16) to meet that condition at the shapes the tests use;
* ``groups`` / ``control_pairs``: the cases and the same-shape pairs of the negative control (a swap would show as c_ij about 1);
* ``oracle_responses``: baseline and per-parameter outputs of the oracle, computed by the caller once per process;
* ``regions``: a byte diff of a packed buffer per source tensor -> the regions derived from each set of sources."""
import math

import numpy as np
import torch

from ddim_audio_amd import synth

G_BOUND = {"f32": 2e-3, "bf16": 5e-2, "mixed": 5e-2}  # model_harness.gate: fp32 worst element, bf16 rms error, of the output's rms
N_MAX = 0.05
N_TABLE = 0.99 * N_MAX  # what AMP is built to: 1 % to spare, so that the condition does not hang on the last bits of a CPU's math library
C_LO, C_HI = 0.5, 1.5

# The cases: the network, the input's shape and the timesteps of its samples.  "long" is the shortest clip at which the input conv of
# the tiny network hands level 0 more statistics partials per sample than a conv finishes in-kernel (test_gpu_wiring.py asserts that
# from the plan); "fnet" is the bottleneck alone, through ddimx_fnet_fwd, on (B, S, width) tokens at S = 8: the dense, folded path.
CASES = {"tiny": dict(net="tiny", shape=(2, 2, 64, 32), steps=[100, 800]),
         "audio": dict(net="audio", shape=(1, 2, 32, 256), steps=[400]),
         "long": dict(net="tiny", shape=(1, 2, 8196, 32), steps=[400]),
         "fnet": dict(net="audio", shape=(2, 8, 2048))}

# Draws whose response at amplitude 1 is too faint for N_TABLE in their case under the bf16 gate: name -> 4 or 16 (test_wiring_cpu.py
# derives the tiny network's entries again from the oracle; every GPU case asserts the condition before it judges the walk)
_AMP4_TINY = """
    up_modules.0.0.norm.1.bias up_modules.0.0.norm.0.bias up_modules.0.0.conv.1.bias up_modules.1.0.norm.0.bias up_modules.1.0.conv.1.bias
    up_modules.1.1.norm.0.bias up_modules.1.1.norm.1.bias up_modules.1.1.conv.1.bias up_modules.2.0.norm.0.bias
    up_modules.2.0.norm.1.bias up_modules.2.0.conv.1.bias transformer.embedding.LayerNorm.bias
    transformer.embedding.projection.bias transformer.encoder.layer.0.intermediate.dense.bias
    transformer.encoder.layer.0.output.dense.bias
"""
_AMP4_AUDIO = """
    transformer.encoder.layer.8.output.dense.bias down_modules.5.3.norm.0.bias down_modules.5.3.norm.1.bias down_modules.6.1.norm.0.bias down_modules.6.2.norm.0.bias
    down_modules.6.2.norm.1.bias down_modules.6.3.norm.0.bias down_modules.6.3.norm.1.bias up_modules.0.0.norm.0.bias
    up_modules.0.0.norm.1.bias up_modules.0.0.conv.1.bias up_modules.0.1.norm.0.bias up_modules.0.1.norm.1.bias
    up_modules.0.1.conv.1.bias up_modules.0.2.norm.0.bias up_modules.0.2.norm.1.bias up_modules.1.0.norm.0.bias
    up_modules.1.0.norm.1.bias up_modules.1.1.norm.0.bias up_modules.1.1.norm.1.bias up_modules.1.2.norm.0.bias
    up_modules.1.2.norm.1.bias up_modules.1.2.conv.1.bias up_modules.2.0.norm.0.bias up_modules.2.0.norm.1.bias
    up_modules.2.0.conv.1.bias up_modules.2.1.norm.0.bias up_modules.2.1.norm.1.bias up_modules.2.1.conv.1.bias
    up_modules.2.2.norm.0.bias up_modules.2.2.norm.1.bias up_modules.2.2.conv.1.bias up_modules.3.0.norm.0.bias
    up_modules.3.0.norm.1.bias up_modules.3.0.conv.1.bias up_modules.3.1.norm.0.bias up_modules.3.1.norm.1.bias
    up_modules.3.1.conv.1.bias up_modules.3.2.norm.0.bias up_modules.3.2.norm.1.bias up_modules.3.2.conv.1.bias
    up_modules.4.0.norm.0.bias up_modules.4.0.norm.1.bias up_modules.4.0.conv.1.bias up_modules.4.1.norm.0.bias
    up_modules.4.1.norm.1.bias up_modules.4.1.conv.1.bias up_modules.5.0.norm.0.bias up_modules.5.0.norm.1.bias
    up_modules.5.0.conv.1.bias up_modules.5.1.norm.0.bias up_modules.5.1.conv.1.bias
    transformer.encoder.layer.0.intermediate.dense.bias transformer.encoder.layer.1.intermediate.dense.bias
    transformer.encoder.layer.1.output.dense.bias transformer.encoder.layer.2.intermediate.dense.bias
    transformer.encoder.layer.2.output.dense.bias transformer.encoder.layer.3.intermediate.dense.bias
    transformer.encoder.layer.3.output.dense.bias transformer.encoder.layer.4.intermediate.dense.bias
    transformer.encoder.layer.4.output.dense.bias transformer.encoder.layer.5.fourier.output.LayerNorm.bias
    transformer.encoder.layer.5.intermediate.dense.bias transformer.encoder.layer.5.output.dense.bias
    transformer.encoder.layer.6.intermediate.dense.bias transformer.encoder.layer.6.output.dense.bias
    transformer.encoder.layer.7.intermediate.dense.bias transformer.encoder.layer.7.output.dense.bias
    transformer.encoder.layer.8.intermediate.dense.bias transformer.encoder.layer.9.intermediate.dense.bias
    transformer.encoder.layer.9.output.dense.bias transformer.encoder.layer.10.intermediate.dense.bias
    transformer.encoder.layer.10.output.dense.bias transformer.encoder.layer.11.intermediate.dense.bias
"""
AMP = {"tiny": dict.fromkeys(_AMP4_TINY.split(), 4.0), "audio": dict.fromkeys(_AMP4_AUDIO.split(), 4.0), "long": {}, "fnet": {}}


def case_forward(case, ocfg):
    """sd -> the oracle's output for the case's input (ref_cpu.model_forward, or transformer_module for "fnet")."""
    from oracle import ref_cpu
    c = CASES[case]
    x = synth.gaussian(f"wiring.{case}.x", c["shape"])
    if case == "fnet":
        kw = ocfg.model.transformers.kwargs
        return lambda sd: ref_cpu.transformer_module(sd, x, kw.num_hidden_layers, kw.layer_norm_eps)
    t = torch.tensor(c["steps"])
    return lambda sd: ref_cpu.model_forward(sd, ocfg, x, t)


def case_names(case, names):
    """The parameters a case perturbs, in plan order."""
    names = [n for n in names if n != "temb.te"]
    if case == "fnet":
        return [n for n in names if n.startswith("transformer.")]
    if case == "long":  # the level-0 blocks (down_modules.1.0, up_modules.2.0 of the tiny network), all eight leaves of each
        return [n for n in names if n.startswith(("down_modules.1.0.", "up_modules.2.0."))]
    return names


def rms(t):
    return float(t.detach().double().square().mean().sqrt())


def draw(name, p, amp=1.0):
    """The replacement of parameter ``name``: an independent Gaussian of the parameter's own size (0.05 at least)."""
    return synth.gaussian("wiring." + name, tuple(p.shape)) * (max(rms(p), 0.05) * amp)


def projection(d_got, d_ref):
    a, b = d_got.detach().double().reshape(-1), d_ref.detach().double().reshape(-1)
    return float(a @ b) / float(b @ b)


def strength(d_ref, y_ref_i):
    """m_i = rms(D_ref) / rms(y_ref(theta_i))."""
    return rms(d_ref) / rms(y_ref_i)


def noise(g, m, n_elements):
    return math.sqrt(2.0) * g / (m * math.sqrt(n_elements))


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def groups(names, n_levels):
    """The parameters (``temb.te`` is a buffer: left out) by module group, in plan order: temb, edge (input and output conv), each
    down level, each up level, the transformer in two halves.  Every parameter is in exactly one group."""
    names = [n for n in names if n != "temb.te"]
    out = {"temb": [n for n in names if n.startswith("temb.")],
           "edge": [n for n in names if n.startswith(("down_modules.0.", f"up_modules.{n_levels}."))]}
    for l in range(n_levels):
        out[f"down{l}"] = [n for n in names if n.startswith(f"down_modules.{l + 1}.")]
    for k in range(n_levels):
        out[f"up{n_levels - 1 - k}"] = [n for n in names if n.startswith(f"up_modules.{k}.")]
    tr = [n for n in names if n.startswith("transformer.")]
    out["transformer_a"], out["transformer_b"] = tr[:len(tr) // 2], tr[len(tr) // 2:]
    flat = [n for g in out.values() for n in g]
    assert sorted(flat) == sorted(names), "the groups must cover every parameter once"
    return out


_BLOCK_LEAVES = ("norm.0.weight", "norm.0.bias", "norm.1.weight", "norm.1.bias", "norm.2.weight", "conv.0.weight", "conv.1.weight",
                 "conv.1.bias")

# The control asks |c_ij| < C_LO of the walk, so a pair belongs to it only where the oracle alone stays two N_MAX below that:
CONTROL_MAX = C_LO - 2 * N_MAX

# Same-shape pairs that are left out of the control because the oracle alone does not keep them below CONTROL_MAX (the bound stays):
# * conv.0.weight / conv.1.weight and norm.0.weight / norm.1.weight of one block, all of them.  A block's branch ends in a GroupNorm
#   (norm.2), so its output h has a fixed size, and an independent draw for any weight inside the branch exchanges h for an h' that is
#   independent of it: D_i = h_i' - h and D_j = h_j' - h share -h, and <D_j, D_i> / <D_i, D_i> = |h|^2 / (2 |h|^2) = 0.5 whichever of
#   the two was replaced (measured with the oracle alone: 0.30 to 0.66 over both networks).  The projection cannot place a weight
#   inside its block; the bit-for-bit content test of the derived copies (test_gpu_wiring.py, part 1) does that for the convs;
# * the pairs below, one by one (oracle alone, 0.36 to 1.3): biases whose own response is faint, so that a neighbour's projects large.
CONTROL_DROPPED = {
    "tiny": {("up_modules.1.0.norm.1.bias", "up_modules.1.0.norm.0.bias"), ("up_modules.1.0.norm.1.bias", "up_modules.1.1.norm.1.bias"),
             ("up_modules.0.0.norm.1.bias", "up_modules.0.0.norm.0.bias"), ("down_modules.2.2.conv.1.bias", "down_modules.2.1.conv.1.bias")},
    "audio": {("up_modules.5.1.norm.1.bias", "up_modules.5.1.norm.0.bias"), ("up_modules.5.1.norm.1.bias", "up_modules.5.0.norm.1.bias"),
              ("down_modules.6.1.norm.1.bias", "down_modules.6.1.norm.0.bias")},
}


def control_pairs(names, net):
    """Ordered pairs (i, j) of same-shape parameters inside ``names`` (one group) for c_ij = <D_got(j), D_ref(i)> / <D_ref(i), D_ref(i)>:
    norm.0.bias / norm.1.bias of a block, and every leaf of a block with the same leaf of the level's next block, both ways round,
    less CONTROL_DROPPED (either way round)."""
    have = set(names)
    blocks = sorted({n[:-len(leaf)] for n in names for leaf in _BLOCK_LEAVES if n.endswith("." + leaf)})
    pairs = [(b + "norm.0.bias", b + "norm.1.bias") for b in blocks]
    for b in blocks:
        head, idx = b[:-1].rsplit(".", 1)
        nxt = f"{head}.{int(idx) + 1}."
        if nxt in blocks:
            pairs += [(b + leaf, nxt + leaf) for leaf in _BLOCK_LEAVES]
    dropped = {frozenset(p) for p in CONTROL_DROPPED.get(net, ())}
    pairs = [(u, v) for u, v in pairs if u in have and v in have and frozenset((u, v)) not in dropped]
    return pairs + [(v, u) for u, v in pairs]


# ---- the oracle's side ------------------------------------------------------------------------------------------------------------------
def oracle_responses(forward, sd, names, amps, cache):
    """``cache`` (a dict the caller keeps for the process) gets "base" = forward(sd) and, per name, (draw, y_ref(theta_i)): whatever
    it lacks is computed, with ``sd[name]`` replaced for the call and put back."""
    with torch.no_grad():
        if "base" not in cache:
            cache["base"] = forward(sd)
        for n in names:
            if n not in cache:
                keep = sd[n]
                d = draw(n, keep, amps.get(n, 1.0))
                sd[n] = d
                try:
                    cache[n] = (d, forward(sd))
                finally:
                    sd[n] = keep
    return cache


def judge_inputs(cache, names, g):
    """{name: (m_i, n_i)} from the oracle's responses alone."""
    base = cache["base"]
    out = {}
    for n in names:
        y = cache[n][1]
        m = strength(y - base, y)
        out[n] = (m, noise(g, m, y.numel()))
    return out


# ---- packed-buffer bookkeeping ----------------------------------------------------------------------------------------------------------
def changed_blocks(mask, align=256):
    """Indices of the ``align``-byte blocks of a buffer in which a byte changed (``mask``: bool per byte); the GPU test makes the same
    reduction on the device."""
    m = np.asarray(mask, dtype=bool)
    pad = np.zeros(-(-m.size // align) * align, dtype=bool)
    pad[:m.size] = m
    return np.nonzero(pad.reshape(-1, align).any(axis=1))[0]


def regions(blocks, total, align=256):
    """``blocks``: {source: indices of the ``align``-byte blocks of a ``total``-byte buffer that changing that source changed}.  The
    buffer is a sequence of regions that start on multiples of ``align``; a region is derived from a fixed set of sources, and two
    regions next to each other from different sets.  Returns {frozenset of sources: (lo, hi)} in bytes: per set, the span from the
    first to the last block that exactly that set changes.  Blocks inside a span that nothing changed (values that come out equal,
    such as zeros) belong to it.  Raises ValueError if the spans of two sets overlap: then the buffer is not laid out as regions."""
    sig = {}
    for s in sorted(blocks):
        for b in np.asarray(blocks[s]).reshape(-1).tolist():
            sig.setdefault(int(b), set()).add(s)
    spans = {}
    for b, who in sig.items():
        k = frozenset(who)
        lo, hi = spans.get(k, (b, b))
        spans[k] = (min(lo, b), max(hi, b))
    order = sorted((lo, hi, sorted(k)) for k, (lo, hi) in spans.items())
    for (_, hi, k), (lo2, _, k2) in zip(order, order[1:]):
        if lo2 <= hi:
            raise ValueError(f"the regions of {k} and {k2} overlap")
    return {k: (lo * align, min((hi + 1) * align, total)) for k, (lo, hi) in spans.items()}
