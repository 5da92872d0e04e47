"""The kernels of csrc/edge_conv.hip one by one through the six edge exports, on the cases of tests/edge_cases.py (tests/test_edge_cpu.py
proves on the host that each case reaches the variant, tile count, loop trips and reduce path it is there for).

Every output -- y / eps / d_sum / d_x, d_w, d_b, the statistics slabs and the weight-gradient workspace at exactly
ddimx_edge_bwd_workspace_floats -- lives in a guarded allocation of 0xFF bytes (``Out`` of tests/kernel_harness.py), so a store past
the image is seen and a partial read before it is written poisons d_w; every input is an ``Ro`` whose bits are compared afterwards.
Operands are dyadic and sized per case so that any fp32 summation order is exact: fp32 outputs equal the fp64 reference bit for bit,
bf16 outputs equal its rounding to nearest even (criterion E of tests/exact_util.py), and the statistics partials equal the fp64 sums
of the stored values."""
import time

import pytest
import torch

from ddim_audio_amd import _lib
import edge_cases as E
import exact_util as X
import gn_kernel_ref as R
import gpu_util as G
from kernel_harness import Out, Ro, lib as L, refused, same, sync

pytestmark = pytest.mark.gpu
F32 = torch.float32
ACT = "act"  # a buffer in the activation dtype


def _np(H, W):
    return -(-H * W // 1024)


# export -> (buffers in argument order: (name, is output, dtype, elements), dims in argument order)
SPEC = {
    "ddimx_conv_in_fwd": ([("x", 0, F32, lambda B, C, n, H, W: B * n * H * W), ("w", 0, F32, lambda B, C, n, H, W: C * n * 9),
                           ("bias", 0, F32, lambda B, C, n, H, W: C), ("y", 1, ACT, lambda B, C, n, H, W: B * H * W * C),
                           ("stats", 1, F32, lambda B, C, n, H, W: B * _np(H, W) * C * 2)], ("B", "cio", "C0", "H", "W")),
    "ddimx_conv_in_fwd_groups": ([("x", 0, F32, lambda B, C, n, H, W: B * n * H * W), ("w", 0, F32, lambda B, C, n, H, W: C * n * 9),
                                  ("bias", 0, F32, lambda B, C, n, H, W: C), ("y", 1, ACT, lambda B, C, n, H, W: B * H * W * C),
                                  ("stats", 1, F32, lambda B, C, n, H, W: B * _np(H, W) * R.SLAB)], ("B", "cio", "C0", "H", "W")),
    "ddimx_conv_out_fwd": ([("a", 0, ACT, lambda B, C, n, H, W: B * H * W * C), ("b", 0, ACT, lambda B, C, n, H, W: B * H * W * C),
                            ("wp", 0, F32, lambda B, C, n, H, W: 9 * n * C), ("bias", 0, F32, lambda B, C, n, H, W: n),
                            ("eps", 1, F32, lambda B, C, n, H, W: B * n * H * W)], ("B", "C0", "cio", "H", "W")),
    "ddimx_conv_in_bwd": ([("dy", 0, ACT, lambda B, C, n, H, W: B * H * W * C), ("x", 0, F32, lambda B, C, n, H, W: B * n * H * W),
                           ("partial", 1, F32, None), ("d_w", 1, F32, lambda B, C, n, H, W: C * n * 9),
                           ("d_b", 1, F32, lambda B, C, n, H, W: C)], ("B", "cio", "C0", "H", "W")),
    "ddimx_conv_in_bwd_data": ([("dy", 0, ACT, lambda B, C, n, H, W: B * H * W * C), ("wp", 0, F32, lambda B, C, n, H, W: 9 * n * C),
                                ("d_x", 1, F32, lambda B, C, n, H, W: B * n * H * W)], ("B", "cio", "C0", "H", "W")),
    "ddimx_conv_out_bwd": ([("de", 0, F32, lambda B, C, n, H, W: B * n * H * W), ("a", 0, ACT, lambda B, C, n, H, W: B * H * W * C),
                            ("b", 0, ACT, lambda B, C, n, H, W: B * H * W * C), ("wp", 0, F32, lambda B, C, n, H, W: 9 * n * C),
                            ("d_sum", 1, ACT, lambda B, C, n, H, W: B * H * W * C), ("partial", 1, F32, None),
                            ("d_w", 1, F32, lambda B, C, n, H, W: n * C * 9), ("d_b", 1, F32, lambda B, C, n, H, W: n)],
                           ("B", "C0", "cio", "H", "W")),
}
EXPORT = {"out": "ddimx_conv_out_fwd", "outb": "ddimx_conv_out_bwd", "inbd": "ddimx_conv_in_bwd_data", "inb": "ddimx_conv_in_bwd"}
# the launchers whose plan each export checks before it launches anything
PLANS = {"ddimx_conv_in_fwd": (X.EDGE_IN,), "ddimx_conv_in_fwd_groups": (X.EDGE_IN,), "ddimx_conv_out_fwd": (X.EDGE_OUT,),
         "ddimx_conv_in_bwd": (X.EDGE_WGRAD,), "ddimx_conv_in_bwd_data": (X.EDGE_IN_BWD_DATA,),
         "ddimx_conv_out_bwd": (X.EDGE_OUT, X.EDGE_OUT_BWD_DATA, X.EDGE_WGRAD)}


def export_of(case):
    if case["op"] == "in":
        return "ddimx_conv_in_fwd_groups" if case["groups"] else "ddimx_conv_in_fwd"
    return EXPORT[case["op"]]


def invoke(export, dt, B, C0, cio, H, W, values=None, null=None):
    """One call of `export`: inputs from `values` (fp64, any shape; zeros where absent) as Ro, outputs as Out.  Buffers of a shape that
    cannot be allocated (a refusal case) hold 16 elements.  Returns (rc, {name: Ro | Out})."""
    bufs, dims = SPEC[export]
    tdt = G.TORCH_DT[dt] if dt in G.TORCH_DT else F32
    pos = [max(1, v) for v in (B, C0, cio, H, W)]
    held, args = {}, [dt]
    for name, is_out, dtype, count in bufs:
        if count is None:  # the weight-gradient workspace, at exactly the size the library asks for
            n = int(L().ddimx_edge_bwd_workspace_floats(dt, B, C0, cio, H, W))
            assert values is None or n > 0
        else:
            n = count(*pos)
        n = n if 0 < n <= 1 << 24 else 16
        dtype = tdt if dtype == ACT else dtype
        if is_out:
            held[name] = Out(n, dtype)
        else:
            v = values[name].reshape(-1) if values is not None else torch.zeros(n)
            assert v.numel() == n, (name, v.numel(), n)
            held[name] = Ro(v, dtype)
        args.append(None if name == null else held[name].ptr)
    d = dict(B=B, C0=C0, cio=cio, H=H, W=W)
    rc = getattr(L(), export)(*args, *(d[k] for k in dims), _lib.stream())
    return rc, held


def run(case, op_):
    """Runs the case's export on the operands `op_`; returns its outputs on the CPU in the layouts of edge_cases.reference, after
    checking the guards of every output and the bits of every input."""
    dt, B, C0, cio, H, W = (case[k] for k in ("dt", "B", "C0", "cio", "H", "W"))
    vals = dict(op_)
    if "w" in vals and case["op"] in ("out", "outb"):
        vals["wp"] = E.pack9(vals.pop("w"))
    elif case["op"] == "inbd":
        vals["wp"] = E.pack9_dgrad(vals.pop("w"))
    export = export_of(case)
    rc, held = invoke(export, dt, B, C0, cio, H, W, vals)
    _lib.check(rc)
    sync()
    out = {}
    for name, is_out, _, _ in SPEC[export][0]:
        if is_out:
            out[name] = held[name].read(f"{case['id']} {name}")
        else:
            held[name].check(f"{case['id']} {name}")
    shapes = dict(y=(B, H, W, C0), eps=(B, cio, H, W), d_sum=(B, H, W, C0), d_x=(B, cio, H, W),
                  d_w=(C0, cio, 3, 3) if case["op"] == "inb" else (cio, C0, 3, 3), d_b=(1, 1, 1, -1))
    return {k: v.view(shapes[k]) if k in shapes else v for k, v in out.items()}


OUT_DT = dict(y=None, d_sum=None, eps=X.F32, d_x=X.F32, d_w=X.F32, d_b=X.F32)  # None: the activation dtype
LAYOUT = dict(y="nhwc", d_sum="nhwc", eps="nchw", d_x="nchw", d_w="nchw", d_b="nhwc")

_REF = {}


def ref_of(case):
    """(operands, reference) of a case, computed once; the large cases are not kept."""
    if case["id"] in _REF:
        return _REF[case["id"]]
    op_ = E.operands(case)
    r = (op_, E.reference(case, op_))
    if case["B"] * case["H"] * case["W"] * case["C0"] <= 1 << 20:
        _REF[case["id"]] = r
    return r


def check_outputs(case, got, ref):
    for k, exact in ref.items():
        X.check(got[k], exact.reshape(got[k].shape), OUT_DT[k] if OUT_DT[k] is not None else case["dt"], f"{case['id']} {k}", layout=LAYOUT[k])


def check_stats(case, got):
    """Channel format: the fp64 sums of the stored values over each 1024-pixel part, bit for bit; group format: those folded to the 8
    groups, then 16 zeros."""
    B, C0, H, W = case["B"], case["C0"], case["H"], case["W"]
    chan = R.chan_stats(got["y"].double().view(B, H * W, C0), 1024)
    st = got["stats"].double()
    if case["groups"]:
        assert torch.equal(st.view(B, _np(H, W), R.SLAB), R.group_slabs(chan)), f"{case['id']}: group slabs"
    else:
        assert torch.equal(st.view(B, _np(H, W), C0, 2), chan), f"{case['id']}: channel slabs"


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c["id"])
def test_edge_case(case):
    op_, ref = ref_of(case)
    t0 = time.perf_counter()
    got = run(case, op_)
    check_outputs(case, got, ref)
    if case["op"] == "in":
        check_stats(case, got)
    print(f"[{case['id']}] {time.perf_counter() - t0:.2f} s after the reference")


def _solo(case, op_, b):
    c = dict(case)
    c["B"] = 1
    return c, {k: (v[b:b + 1] if v.shape[0] == case["B"] and k not in ("w", "bias") else v) for k, v in op_.items()}


@pytest.mark.parametrize("case", [c for c in E.CASES if c["batch"]], ids=lambda c: c["id"])
def test_batch_independence(case):
    """Sample b of the batch is bit-identical to the same sample run alone (statistics slabs included)."""
    op_, _ = ref_of(case)
    full = run(case, op_)
    key = {"in": "y", "out": "eps", "outb": "d_sum", "inbd": "d_x"}[case["op"]]
    for b in (0, case["B"] - 1):
        c1, o1 = _solo(case, op_, b)
        alone = run(c1, o1)
        same(full[key][b], alone[key][0], f"{case['id']} sample {b}")
        if case["op"] == "in":
            same(full["stats"].view(case["B"], -1)[b], alone["stats"].view(-1), f"{case['id']} statistics of sample {b}")


@pytest.mark.parametrize("case", [c for c in E.CASES if c["control"]], ids=lambda c: c["id"])
def test_negative_control(case):
    """One tap of the weights zeroed (the weight gradient: one plane of S) in what the kernel gets: the criterion reports it."""
    op_, ref = ref_of(case)
    op = case["op"]
    bad = {k: v.clone() for k, v in op_.items()}
    if op == "inb":
        bad["x"][:, -1] = 0
        key = "d_w"
    else:
        bad["w"][:, :, 1, 2] = 0
        key = {"in": "y", "out": "eps", "outb": "d_sum", "inbd": "d_x"}[op]
    got = run(case, bad)
    dt = OUT_DT[key] if OUT_DT[key] is not None else case["dt"]
    assert bool(X.mismatches(got[key], ref[key].reshape(got[key].shape), dt).any()), f"{case['id']}: a zeroed tap went unnoticed in {key}"
    if op == "outb":  # w does not enter d_w: its control is a plane of S = d_eps
        assert not bool(X.mismatches(got["d_w"], ref["d_w"], X.F32).any())
        bad = {k: v.clone() for k, v in op_.items()}
        bad["de"][:, -1] = 0
        got = run(case, bad)
        assert bool(X.mismatches(got["d_w"], ref["d_w"], X.F32).any()), f"{case['id']}: a zeroed plane of S went unnoticed in d_w"


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
VALID = dict(dt=X.F32, B=2, C0=32, cio=2, H=5, W=7)
BIG = 2 ** 31 - 1
COMMON = [dict(dt=2), dict(dt=-1), dict(B=0), dict(H=0), dict(W=0), dict(cio=0), dict(C0=0), dict(B=-1), dict(H=BIG), dict(W=BIG, H=1),
          dict(B=65535, C0=64, H=2 ** 20, W=2 ** 20)]
IN_RULES = [dict(C0=40), dict(C0=12), dict(C0=512), dict(C0=36, dt=X.BF16), dict(C0=256, cio=8), dict(B=65536, H=1, W=1),
            dict(H=2 ** 15, W=2 ** 15 + 1, B=1), dict(C0=16, H=2 ** 16, W=2 ** 15, B=1)]
OUT_RULES = [dict(cio=5), dict(C0=12), dict(C0=48), dict(C0=36), dict(B=2 ** 16, H=2 ** 15, W=2 ** 15)]
WGRAD_RULES = [dict(cio=5), dict(C0=68), dict(C0=64), dict(B=2 ** 16, H=2 ** 15, W=2 ** 15), dict(C0=16, B=2 ** 16, H=2 ** 15, W=2 ** 15)]
RULES = {
    "ddimx_conv_in_fwd": COMMON + IN_RULES,
    "ddimx_conv_in_fwd_groups": COMMON + IN_RULES + [dict(C0=4)],
    "ddimx_conv_out_fwd": COMMON + OUT_RULES,
    "ddimx_conv_in_bwd": COMMON + WGRAD_RULES,
    "ddimx_conv_in_bwd_data": COMMON + [dict(cio=5), dict(C0=6), dict(C0=12, dt=X.BF16), dict(B=2 ** 16, H=2 ** 15, W=2 ** 15),
                                        dict(C0=16, B=65536, H=1, W=1)],
    "ddimx_conv_out_bwd": COMMON + OUT_RULES + [dict(B=65536, H=1, W=1), dict(C0=16, B=65536, H=1, W=1)],
}


def _host_refuses(export, a):
    """The launcher's plan refuses these arguments (host only), so the export -- which asks the same function -- launches nothing."""
    for op in PLANS[export]:
        try:
            X.edge_plan(op, a["dt"], a["B"], a["C0"], a["cio"], a["H"], a["W"], 1 if export.endswith("groups") else 0)
        except RuntimeError:
            return True
    return False


@pytest.mark.parametrize("export", list(SPEC))
def test_refusals(export):
    """Every rule the export documents in include/ddimx.h, with otherwise valid arguments and guarded outputs: refused by name, nothing
    written.  A valid call of the same shape is accepted first."""
    rc, held = invoke(export, **VALID)
    _lib.check(rc)
    sync()
    for change in RULES[export]:
        a = {**VALID, **change}
        assert _host_refuses(export, a), (export, change)
        rc, held = invoke(export, **a)
        refused(rc, *(h for h in held.values() if isinstance(h, Out)), who=export)
    for name, _, _, _ in SPEC[export][0]:
        rc, held = invoke(export, **VALID, null=name)
        refused(rc, *(h for h in held.values() if isinstance(h, Out)), who=export)
    assert int(L().ddimx_edge_bwd_workspace_floats(X.F32, 2, 32, 5, 5, 7)) == -1
