"""Input-gradient timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Per batch size it times one forward + backward (train mode, ``eps.backward(v)``) three ways, alternating them round by round:
  full      -- every parameter gradient, no input gradient (the training step's backward);
  full_dx   -- the same plus the gradient w.r.t. the input (ddimx_unet_bwd_ex with d_x: one more launch behind the chain);
  data_only -- parameters frozen (``requires_grad_(False)``): the data-gradient chain and d_x alone (DDIMX_BWD_DATA_ONLY).
and then the input conv's data-gradient kernel alone (ddimx_conv_in_bwd_data, back-to-back launches between two events), with
the bytes it must move (dy read once, d_x written once) over its time as a share of the HBM peak.
usage: python tools/input_grad_time.py [T=1024] [rounds=5] [B ...=8 32]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402

HBM_PRACTICAL = 6.3e12  # bytes/s, streaming copy


def _step(m, x, t, v, want_x):
    """one forward + backward; returns (fwd_ms, bwd_ms)"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    xin = x.detach().requires_grad_(want_x)
    ev[0].record()
    eps = m(xin, t)
    ev[1].record()
    eps.backward(v)
    ev[2].record()
    torch.cuda.synchronize()
    for p in m.parameters():
        p.grad = None
    return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


def time_modes(m, b, t_len, rounds):
    """Not timing.time_legs: a leg here is one forward + backward under autograd with an event between the two, no stepper."""
    x = torch.randn(b, 2, t_len, 256, device="cuda")
    v = torch.randn_like(x)
    t = torch.randint(0, 1000, (b,), device="cuda")
    modes = {"full": (True, False), "full_dx": (True, True), "data_only": (False, True)}
    res = {k: [] for k in modes}
    for r in range(rounds + timing.WARMUP_ROUNDS):
        for name, (params, want_x) in modes.items():
            m.requires_grad_(params)
            f, bw = _step(m, x, t, v, want_x)
            if r >= timing.WARMUP_ROUNDS:
                res[name].append((f, bw))
    m.requires_grad_(True)
    out = {}
    for name, v_ in res.items():
        tot = [f + bw for f, bw in v_]
        out[name] = {"fwd_bwd_ms": statistics.median(tot), "bwd_ms": statistics.median([bw for _, bw in v_]),
                     "fwd_ms": statistics.median([f for f, _ in v_]), "spread_ms": max(tot) - min(tot)}
    return out


def time_kernel(b, t_len, dt):
    lib = _lib.load()
    c0, cin, f = 32, 2, 256
    tdt = torch.bfloat16 if dt == _lib.DDIMX_BF16 else torch.float32
    dy = torch.randn(b, t_len, f, c0, device="cuda").to(tdt)
    w = torch.randn(c0, cin, 3, 3, device="cuda")
    wp = torch.empty(9 * cin * c0, device="cuda")
    _lib.check(lib.ddimx_pack_conv_dgrad(_lib.DDIMX_F32, _lib.ptr(w), _lib.ptr(wp), c0, cin, _lib.stream()))
    d_x = torch.empty(b, cin, t_len, f, device="cuda")
    args = (dt, _lib.ptr(dy), _lib.ptr(wp), _lib.ptr(d_x), b, cin, c0, t_len, f, _lib.stream())
    ms = timing.time_launches(lambda: _lib.check(lib.ddimx_conv_in_bwd_data(*args)), reps=20, warm=3)
    nbytes = dy.numel() * dy.element_size() + d_x.numel() * 4
    return {**timing.bandwidth_record("ddimx_conv_in_bwd_data", ms, 1, nbytes, B=b, T=t_len, dtype="bf16" if dt == _lib.DDIMX_BF16 else "f32"),
            "frac_of_6.3TBps": nbytes / HBM_PRACTICAL / (ms * 1e-3)}


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 5, "B": [8, 32]})
    torch.manual_seed(0)
    m = timing.audio_model().train()
    for b in a.B:
        r = time_modes(m, b, a.T, a.rounds)
        r["data_only_saving_ms"] = r["full"]["fwd_bwd_ms"] - r["data_only"]["fwd_bwd_ms"]
        r["dx_cost_ms"] = r["full_dx"]["fwd_bwd_ms"] - r["full"]["fwd_bwd_ms"]
        print(json.dumps({"what": "fwd+bwd", "B": b, "T": a.T, "dtype": "bf16", "rounds": a.rounds, **r}), flush=True)
    for b in a.B:
        for dt in (_lib.DDIMX_BF16, _lib.DDIMX_F32):
            print(json.dumps(time_kernel(b, a.T, dt)), flush=True)


if __name__ == "__main__":
    main()
