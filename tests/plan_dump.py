"""Every launch plan and buffer size the library derives on the host, as one JSON-able dict: the plan table of exact_cases.py, the
edge-convolution plans of edge_cases.py and of the audio config, the weight-gradient and GroupNorm plans of the audio widths, and the workspace / tape sizes of the tiny and audio configs.  None of it
needs a GPU.  Run as a script it prints the dict as JSON (tests/test_host_cpu.py::test_launch_plans_ignore_the_environment starts it
in a child process whose environment differs from the parent's)."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import exact_util as X  # noqa: E402
import edge_cases as E  # noqa: E402
from exact_cases import CONV_CASES, DOWNUP_CASES, DTN, DUBWD_CASES, DUBWD_KEY_CASES, WGRAD_CASES, WGRAD_KEY_CASES  # noqa: E402
from ddim_audio_amd import configs  # noqa: E402

PLAN_KEYS = ("family", "var", "tiles_x", "tiles_y", "tiles_per_wg", "wgs_per_sample", "rounds", "th", "tw", "nthreads", "Hv", "Wv")


def _conv(out, tag, *args):
    p = X.conv_plan(*args)
    out[f"conv:{tag}"] = [p[k] for k in PLAN_KEYS]


def dump():
    out = {}
    for c in CONV_CASES:
        _conv(out, c["id"], c["dt"], X.CONV3, c["C"], c["C"], c["B"], c["H"], c["W"], c["flags"])
    for c in DOWNUP_CASES:
        _conv(out, c["id"], c["dt"], c["mode"], c["cin"], c["cout"], c["B"], c["H"], c["W"], c["flags"])
    for c in DUBWD_CASES + DUBWD_KEY_CASES:  # the data-gradient convs and the weight gradients of ddimx_downsample_bwd / ddimx_upsample_add_bwd
        dt, B = c["dt"], c["B"]
        if c["mode"] == X.DOWN4:
            _conv(out, c["id"], dt, X.UP4, c["cout"], c["cin"], B, c["H"] // 2, c["W"] // 2, X.P_BATCH | X.P_SKIP)
            out[f"wgrad:{c['id']}"] = X.wgrad_plan(dt, X.DOWN4, c["cin"], c["cout"], B, c["H"] // 2, c["W"] // 2)
        else:
            _conv(out, c["id"], dt, X.DOWN4, c["cout"], c["cin"], B, 2 * c["H"], 2 * c["W"], X.P_BATCH)
            out[f"wgrad:{c['id']}"] = X.wgrad_plan(dt, X.DOWN4, c["cout"], c["cin"], B, c["H"], c["W"])
    for c in WGRAD_CASES + WGRAD_KEY_CASES:
        out[f"wgrad:{c['id']}"] = X.wgrad_plan(c["dt"], X.CONV3, c["C"], c["C"], c["B"], c["H"], c["W"])
    for c in E.CASES:
        for key, p in E.plans(c).items():
            out[f"edge:{key}:{c['id']}"] = [p[k] for k in X.EDGE_KEYS]
    audio = configs.audio_config().model
    for dt in (X.F32, X.BF16):
        for B in (1, 8, 64):
            for T in (64, 1024, 4096):
                for key, op in E.PLAN_OPS.items():  # the edge launchers of the audio config: C0 = ch[0], the narrow side channels
                    p = X.edge_plan(op, dt, B, audio.ch[0], audio.channels, T, audio.f_size, 1 if key == "in" else 0)
                    out[f"edge:{key}:{DTN[dt]}-B{B}-T{T}"] = [p[k] for k in X.EDGE_KEYS]
                for l, C in enumerate(audio.ch):
                    H, W = T >> l, audio.f_size >> l
                    tag = f"{DTN[dt]}-L{l}-B{B}-T{T}"
                    out[f"wgrad:c3:{tag}"] = X.wgrad_plan(dt, X.CONV3, C, C, B, H, W)
                    if l > 0:
                        out[f"wgrad:du:{tag}"] = X.wgrad_plan(dt, X.DOWN4, audio.ch[l - 1], C, B, H, W)
                    y = X.gn_plan(dt, C, 1, H, W, 1)["y_np"]
                    out[f"gn:{tag}"] = X.gn_plan(dt, C, B, H, W, y)
    from ddim_audio_amd.model import Model
    for name, make in (("tiny", configs.tiny_config), ("audio", configs.audio_config)):
        for tensor in ("torch.FloatTensor", "torch.BFloat16Tensor"):
            m = Model(make(tensor))
            lib = m._ensure_handle()
            for B, T in ((2, 64), (8, 1024)):
                out[f"bytes:{name}:{tensor}:{B}x{T}"] = [lib.ddimx_workspace_bytes(m._handle, B, T), lib.ddimx_train_workspace_bytes(m._handle, B, T),
                                                         lib.ddimx_train_tape_bytes(m._handle, B, T)]
    return out


if __name__ == "__main__":
    print(json.dumps(dump(), sort_keys=True))
