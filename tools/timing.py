"""The measuring method of the feature timing tools (tools/*_time.py), in its one copy: the interleaved rounds of sampler legs, the
two kernel-alone timers, the bandwidth arithmetic, the audio model and the command line.  A tool keeps what is its own -- its legs,
its kernel rows and pass counts, its derived ratios, its usage text -- and takes the rest from here.

Everything here needs a GPU and says so (``require_gpu``); nothing falls back.  Importing this module, or a tool, does no device work.
"""
import collections
import os
import re
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import configs, synth  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec
WARMUP_ROUNDS = 2  # the first captures every graph; a stepper whose first step re-allocated a buffer of the model (the backward
#                    packing, a workspace) makes the graphs captured before it stale, and the second round captures those again


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("the timing tools measure a GPU and there is none: no device is visible to torch")


def audio_model():
    """A fresh bf16 audio model with synthetic weights, in eval mode."""
    require_gpu()
    m = D.Model(configs.dict2namespace(configs.audio_dict("torch.cuda.BFloat16Tensor")))
    synth.fill_module(m, 0)
    return m.eval()


# ---- the command line ----
def parse_args(argv, spec, flags=()):
    """The tools' command lines: ``[T=1024] [rounds=R] [B ...]``, ``[rounds=R] [long] [NxW ...]`` and their kin.  ``spec`` is the
    usage line as an ordered {name: default}: an int default takes one integer, a str default one word, a list of ints every
    argument that is left, a list of pairs every ``NxW``.  The words in ``flags`` and the ``NxW`` are known by their shape and may
    stand anywhere; the rest is positional, and ``name=value`` may be written for ``value``.  Returns a namespace of the spec's
    names and the flags (bool)."""
    args = list(sys.argv[1:] if argv is None else argv)
    out = types.SimpleNamespace(**{f: f in args for f in flags})
    args = [a.split("=", 1)[-1] for a in args if a not in flags]

    def integer(name, tok):
        if not re.fullmatch(r"-?\d+", tok):
            raise SystemExit(f"{name}: `{tok}` is not an integer")
        return int(tok)

    for name, default in spec.items():
        if isinstance(default, list) and isinstance(default[0], tuple):
            cases = [a for a in args if re.fullmatch(r"\d+x\d+", a)]
            args = [a for a in args if a not in cases]
            setattr(out, name, [tuple(int(v) for v in a.split("x")) for a in cases] or default)
    for name, default in spec.items():
        if isinstance(default, list) and isinstance(default[0], tuple):
            continue
        if isinstance(default, list):
            value, args = [integer(name, a) for a in args] or default, []
        elif not args:
            value = default
        else:
            value = integer(name, args.pop(0)) if isinstance(default, int) else args.pop(0)
        setattr(out, name, value)
    if args:
        raise SystemExit(f"arguments left over: {' '.join(args)}")
    return out


# ---- interleaved rounds of legs ----
# reset(): puts the leg back to its start (the sample copied back and the stepper rewound, or a request submitted to a pool);
# step(): one sampler step; timed / untimed: steps inside the window and in front of it (row 0 stays outside: after a rewind the
# history buffers are stale and row 0 never reads them; in the first round it is the eager step in front of the capture);
# after(): what must follow the window (a pool's drain); stepper: the graph owner the leg uses, if it has one -- closed at the end
Leg = collections.namedtuple("Leg", "reset step timed untimed after stepper", defaults=(1, None, None))


def stepper_leg(stepper, xt, x_init, timed, untimed=1):
    """The usual leg: ``stepper`` steps the sample ``xt`` in place, which starts every round as ``x_init``."""
    def reset():
        xt.copy_(x_init)
        stepper.rewind()
    return Leg(reset, stepper.step, timed, untimed, None, stepper)


def leg_order(names, r, fixed=False):
    """Round ``r``'s order: forwards, then backwards, so that no leg always runs first or always behind the same neighbour."""
    return tuple(names) if fixed or r % 2 == 0 else tuple(names)[::-1]


def summary(samples):
    return {"ms_per_step": statistics.median(samples), "spread_ms": max(samples) - min(samples)}


def capture_counts(warm, end):
    """``warm`` / ``end``: {leg: stepper.captures} after the warm-up rounds and after the last round.  ``captures_while_timed`` is 0
    when every timed step was a replay of a graph captured during the warm-up."""
    return {k: {"captures": end[k], "captures_while_timed": end[k] - warm.get(k, end[k])} for k in end}


def time_legs(legs, rounds, fixed_order=False, expect_captures=1):
    """``legs``: ordered {name: Leg}.  ``WARMUP_ROUNDS`` untimed rounds, then ``rounds`` timed ones; every round runs each leg once,
    in ``leg_order``.  Returns ({name: summary of its ms per timed step}, {name: capture_counts} of the legs with a stepper).
    ``expect_captures``: the captures every stepper must end with -- an int, or {name: int} for the legs that differ from 1 --
    or None for no check.  The steppers are closed whatever happens."""
    require_gpu()
    names = tuple(legs)
    res = {k: [] for k in names}
    owners = {k: leg.stepper for k, leg in legs.items() if leg.stepper is not None}
    warm = {}
    try:
        for r in range(rounds + WARMUP_ROUNDS):
            if r == WARMUP_ROUNDS:
                warm = {k: st.captures for k, st in owners.items()}
            for name in leg_order(names, r, fixed_order):
                leg = legs[name]
                leg.reset()
                with torch.no_grad():
                    for _ in range(leg.untimed):
                        leg.step()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(leg.timed):
                        leg.step()
                    e1.record()
                torch.cuda.synchronize()
                if leg.after is not None:
                    leg.after()
                if r >= WARMUP_ROUNDS:
                    res[name].append(e0.elapsed_time(e1) / leg.timed)
        counts = capture_counts(warm, {k: st.captures for k, st in owners.items()})
        if expect_captures is not None:
            want = expect_captures if isinstance(expect_captures, dict) else dict.fromkeys(owners, expect_captures)
            assert all(c["captures"] == want.get(k, 1) for k, c in counts.items()), counts
    finally:
        for st in owners.values():
            st.close()
    return {k: summary(v) for k, v in res.items()}, counts


# ---- one kernel (or a short sequence) alone ----
# Two methods, because the numbers quoted for each tool were taken with one of them.  time_launches suits calls of tens of
# microseconds and more: the host stays ahead of the device.  A kernel of a few microseconds launched from Python would be timed
# by the interpreter, not by the GPU, so the noise and window tools time the replay of one graph of ``reps`` calls instead.  The
# counts differ from tool to tool too (warm 1 or 3, reps 20 or 50; tools/distill_time.py alone synchronises in front of the
# window): each tool passes the ones its quoted figures were taken with.
def time_launches(fn, reps, warm, sync=False):
    """ms per call of ``fn``: ``warm`` calls, then ``reps`` eager back-to-back calls between two events."""
    require_gpu()
    for _ in range(warm):
        fn()
    if sync:
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def time_graph_replay(fn, reps, warm):
    """ms per call of ``fn``: ``reps`` calls captured into one graph, ``warm`` replays, then one replay between two events."""
    require_gpu()
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    for _ in range(warm):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    del g
    torch.cuda.synchronize()
    return ms


def bandwidth_record(what, ms, passes, nbytes, unit="ms", **fields):
    """A kernel's record: the ``passes * nbytes`` bytes it must move, over its time, as TB/s and as a share of the HBM peak.
    ``unit``: the time is printed as ``ms`` or as ``us``."""
    moved = passes * nbytes
    return {"what": what, **fields, unit: ms if unit == "ms" else ms * 1e3, "bytes": moved, "TB_per_s": moved / ms / 1e9,
            "frac_of_8TBps": moved / HBM_PEAK / (ms * 1e-3)}
