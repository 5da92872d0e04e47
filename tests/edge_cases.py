"""Case table of the edge-convolution kernels (csrc/edge_conv.hip): tests/test_gpu_edge_kernels.py runs the cases, tests/test_edge_cpu.py
checks on the host that each reaches the branch it declares (the library's own ddimx_debug_edge_plan) and that its operand ranges
make every fp32 summation order exact.  No HIP here.

A case names the export it runs (`op`) and, per launcher behind that export, the plan it must get (`want`: plan key -> value;
exact_util.edge_plan's keys, with `trips` the most trips any block makes of its outer loop):

  in    ddimx_conv_in_fwd / _groups (groups = 1)   EDGE_IN
  out   ddimx_conv_out_fwd                         EDGE_OUT
  outb  ddimx_conv_out_bwd: d_sum, d_w, d_b        EDGE_OUT_BWD_DATA, EDGE_WGRAD (mode 1, G = a + b, S = d_eps)
  inbd  ddimx_conv_in_bwd_data                     EDGE_IN_BWD_DATA
  inb   ddimx_conv_in_bwd: d_w, d_b                EDGE_WGRAD (mode 0, G = dy, S = x)
"""
import torch.nn.functional as F

import exact_util as X

DTN = {X.F32: "f32", X.BF16: "bf16"}
DTS = (X.F32, X.BF16)
GENERIC, FIXED = 0, 1  # plan variants: the kernel for any width / the one for C0 = 32, Cio = 2


def pixb(dt):
    """Pixel columns of one weight-gradient strip."""
    return 64 if dt == X.BF16 else 32


def _case(op, dt, C0, cio, B, H, W, groups=0, control=False, batch=False, **want):
    name = f"{op}-{DTN[dt]}-C{C0}x{cio}-{B}x{H}x{W}" + ("-groups" if groups else "")
    return dict(id=name, op=op, dt=dt, C0=C0, cio=cio, B=B, H=H, W=W, groups=groups, control=control, batch=batch, want=want)


CASES = []
for _dt in DTS:
    _pb = pixb(_dt)
    # ---- conv_in forward -------------------------------------------------------------------------------------------------------------
    for _g in (0, 1):
        _first = _g == 0
        CASES += [  # MFMA variant.  trips: 32-pixel blocks of wave 0
            _case("in", _dt, 32, 2, 2, 1, 1, _g, **{"in": dict(variant=FIXED, tiles_x=1, trips=1)}),
            _case("in", _dt, 32, 2, 3, 1, 40, _g, **{"in": dict(variant=FIXED, tiles_x=1, trips=1)}),
            _case("in", _dt, 32, 2, 2, 40, 1, _g, **{"in": dict(variant=FIXED, tiles_x=1, trips=1)}),  # W = 1: the shift path, shift 0
            _case("in", _dt, 32, 2, 3, 5, 24, _g, control=_first, batch=_first, **{"in": dict(variant=FIXED, tiles_x=1, trips=1)}),
            # 1056 pixels: part 1 holds 32, waves 1-3 of its block own none
            _case("in", _dt, 32, 2, 2, 33, 32, _g, **{"in": dict(variant=FIXED, tiles_x=2, trips=8, last_part=32)}),
            _case("in", _dt, 32, 2, 2, 40, 256, _g, **{"in": dict(variant=FIXED, tiles_x=10, trips=8)}),
        ]
        for _cin, _c0 in ((1, 8), (1, 32), (3, 16), (4, 64), (4, 256)):
            _ctl = _first and (_cin, _c0) == (3, 16)
            CASES += [_case("in", _dt, _c0, _cin, 2, 7, 24, _g, control=_ctl, batch=_ctl, **{"in": dict(variant=GENERIC, tiles_x=1)}),
                      _case("in", _dt, _c0, _cin, 3, 33, 32, _g, **{"in": dict(variant=GENERIC, tiles_x=2, last_part=32)})]
    # ---- conv_out forward ------------------------------------------------------------------------------------------------------------
    CASES += [
        _case("out", _dt, 32, 2, 2, 1, 1, **{"out": dict(variant=FIXED, tiles_x=1, tiles_y=1)}),
        _case("out", _dt, 32, 2, 3, 1, 33, **{"out": dict(variant=FIXED, tiles_x=2, tiles_y=1)}),
        _case("out", _dt, 32, 2, 2, 9, 1, **{"out": dict(variant=FIXED, tiles_x=1, tiles_y=2)}),
        _case("out", _dt, 32, 2, 2, 8, 32, **{"out": dict(variant=FIXED, tiles_x=1, tiles_y=1, grid_x=2)}),  # exactly one tile
        _case("out", _dt, 32, 2, 3, 9, 33, control=True, batch=True, **{"out": dict(variant=FIXED, tiles_x=2, tiles_y=2)}),
    ]
    for _c0, _co in ((8, 1), (16, 3), (32, 1), (32, 4), (40, 4)):
        _ctl = (_c0, _co) == (16, 3)
        CASES += [_case("out", _dt, _c0, _co, 2, 9, 33, control=_ctl, batch=_ctl, **{"out": dict(variant=GENERIC, tiles_x=2, tiles_y=2)}),
                  _case("out", _dt, _c0, _co, 3, 1, 1, **{"out": dict(variant=GENERIC, tiles_x=1, tiles_y=1)})]
    # ---- conv_out backward: data gradient (d_w, d_b ride along in their tiled / strip form) -------------------------------------------------
    CASES += [
        # (1 x 1 runs with the strip cases of the weight gradient below)
        _case("outb", _dt, 32, 2, 3, 9, 33, control=True, batch=True, outbd=dict(variant=FIXED, trips=5),
              wgrad=dict(variant=FIXED)),
        _case("outb", _dt, 32, 2, 2, 40, 1, outbd=dict(variant=FIXED), wgrad=dict(variant=FIXED)),
    ]
    for _c0, _co in ((8, 1), (16, 3), (40, 4)):  # (8, 1), (40, 3 | 4): also the tiled weight gradient at NI = 1, 3, 4 in mode 1
        _ctl = (_c0, _co) == (16, 3)
        CASES.append(_case("outb", _dt, _c0, _co, 2, 9, 33, control=_ctl, batch=_ctl, outbd=dict(variant=GENERIC, trips=1),
                           wgrad=dict(variant=GENERIC, partial_blocks=6, trips=1, unrolled=False)))
    # ---- conv_in data gradient -------------------------------------------------------------------------------------------------------
    for _c0, _ni in ((8, 1), (16, 3), (64, 4)):
        _ctl = (_c0, _ni) == (16, 3)
        CASES.append(_case("inbd", _dt, _c0, _ni, 2, 9, 33, control=_ctl, batch=_ctl, inbd=dict(variant=GENERIC, trips=1)))
    # second trip of the grid-stride loop: 1 049 600 pixels against 4096 x 256.  The largest case of the module
    CASES.append(_case("inbd", _dt, 8, 3, 1, 4100, 256, inbd=dict(variant=GENERIC, grid_x=4096, trips=2)))
    CASES += [  # the tiled variant: conv_out's tile walk, on conv_out's shapes
        _case("inbd", _dt, 32, 2, 2, 1, 1, inbd=dict(variant=FIXED, tiles_x=1, tiles_y=1)),
        _case("inbd", _dt, 32, 2, 3, 1, 33, inbd=dict(variant=FIXED, tiles_x=2, tiles_y=1)),
        _case("inbd", _dt, 32, 2, 2, 9, 1, inbd=dict(variant=FIXED, tiles_x=1, tiles_y=2)),
        _case("inbd", _dt, 32, 2, 2, 8, 32, inbd=dict(variant=FIXED, tiles_x=1, tiles_y=1, grid_x=2)),  # exactly one tile
        _case("inbd", _dt, 32, 2, 3, 9, 33, control=True, batch=True, inbd=dict(variant=FIXED, tiles_x=2, tiles_y=2)),
    ]
    # ---- weight gradient, strip variant, both modes ----------------------------------------------------------------------------------
    for _op in ("inb", "outb"):
        _extra = {"outbd": dict(variant=FIXED)} if _op == "outb" else {}
        _first = _op == "inb"
        CASES += [
            _case(_op, _dt, 32, 2, 2, 1, 1, **_extra, wgrad=dict(variant=FIXED, tiles_x=1, tiles_y=1, trips=1, partial_blocks=2)),
            # two strip rows, the second a single row; two strip columns, the second a single column
            _case(_op, _dt, 32, 2, 2, 129, _pb + 1, control=_first, **_extra,
                  wgrad=dict(variant=FIXED, tiles_x=2, tiles_y=2, trips=4, partial_blocks=8)),
            # the second strip row has 33 rows: chunks of 32 rows and of 1 row
            _case(_op, _dt, 32, 2, 2, 161, 24, **_extra, wgrad=dict(variant=FIXED, tiles_x=1, tiles_y=2, trips=4, last_chunk=1)),
            # 36 partial blocks: one 8-deep trip of the reduce, then one single trip
            _case(_op, _dt, 32, 2, 3, 161, 6 * _pb, **_extra,
                  wgrad=dict(variant=FIXED, partial_blocks=36, unrolled=True, reduce_unrolled=1, reduce_tail=1)),
        ]
    # ---- weight gradient, tiled variant (mode 0; mode 1 runs in the conv_out backward cases above) ---------------------------------------
    for _c, _ni in ((8, 1), (16, 4), (40, 3)):
        CASES.append(_case("inb", _dt, _c, _ni, 2, 9, 33, control=(_c, _ni) == (16, 4),
                           wgrad=dict(variant=GENERIC, partial_blocks=6, trips=1, unrolled=False)))
    CASES += [
        # 3 x 19 x 19 = 1083 tiles on 1024 blocks, ragged both ways: 59 blocks run the tile loop twice
        _case("inb", _dt, 8, 1, 3, 300, 290, wgrad=dict(variant=GENERIC, tiles_x=19, tiles_y=19, partial_blocks=1024, trips=2, unrolled=True)),
        # the widest C at NI = 2 that fits the LDS: both items of a thread in use (9 x 60 = 540 > 288)
        _case("inb", _dt, 60, 2, 2, 17, 17, wgrad=dict(variant=GENERIC, tiles_x=2, tiles_y=2, partial_blocks=8, trips=1)),
    ]
# second trip of conv_out's generic data gradient: more than 4096 x 256 channel pieces.  fp32: 410 x 256 x 10 = 1 049 600; bf16
# has half the pieces per pixel: 820 is the smallest H (tests/test_edge_cpu.py proves both minimal)
SECOND_TRIP_H = {X.F32: 410, X.BF16: 820}
for _dt in DTS:
    CASES.append(_case("outb", _dt, 40, 3, 1, SECOND_TRIP_H[_dt], 256, outbd=dict(variant=GENERIC, grid_x=4096, trips=2),
                       wgrad=dict(variant=GENERIC, unrolled=True)))
WIDEST_TILED_C = 60

PLAN_OPS = {"in": X.EDGE_IN, "out": X.EDGE_OUT, "outbd": X.EDGE_OUT_BWD_DATA, "inbd": X.EDGE_IN_BWD_DATA, "wgrad": X.EDGE_WGRAD}


def plans(case):
    """{launcher: plan} of the launchers behind the case's export, each with the flags the table declares."""
    out = {}
    for key in case["want"]:
        p = X.edge_plan(PLAN_OPS[key], case["dt"], case["B"], case["C0"], case["cio"], case["H"], case["W"], case["groups"])
        p["unrolled"] = p["reduce_unrolled"] > 0
        if key == "in":
            p["last_part"] = case["H"] * case["W"] - 1024 * (p["tiles_x"] - 1)
        if key == "wgrad" and p["variant"] == FIXED:
            p["last_chunk"] = (case["H"] - 128 * (p["tiles_y"] - 1) - 1) % 32 + 1  # rows of the last strip row's last chunk
        out[key] = p
    return out


def plan_line(case):
    """The summary's line: variant, blocks, trips, partial blocks of every launcher of the case."""
    parts = []
    for key, p in plans(case).items():
        s = f"{key}: variant {p['variant']}, blocks {p['grid_x']}x{p['grid_y']}, trips {p['trips']}"
        if key == "wgrad":
            s += f", partial blocks {p['partial_blocks']} (reduce: {p['reduce_unrolled']} unrolled + {p['reduce_tail']} single trips)"
        parts.append(s)
    return f"{case['id']}: " + "; ".join(parts)


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def wgrad_ranges(case):
    """(kg, ks): G on k/8 with |k| <= kg, S on k/8 with |k| <= ks, the largest pair whose B H W products stay below 2^24 grid units
    (the grid of a product is 2^-6), so that the ranges shrink with the image."""
    n = case["B"] * case["H"] * case["W"]
    for kg, ks in ((8, 8), (4, 4), (2, 2), (2, 1)):
        if n * kg * ks < 2 ** 24:
            return kg, ks
    raise AssertionError(f"{case['id']}: too many pixels for an exact weight gradient")


def conv_in_ranges(case):
    """((kx, px), (kw, pw), (kb, pb)) of x, w and the bias.  The statistics need the sums of y and y^2 over a sample's group exact in
    fp32: the rich set where the expected sum of y^2 leaves a factor of four, the poor one for large images and wide groups."""
    n = case["H"] * case["W"] * (case["C0"] // 8 if case["C0"] >= 8 else 1)
    rich = (9 * case["cio"] * (60 / 9 / 16) * (2 / 16) + 88 / 256) * 256  # E[y^2] in units of the y^2 grid 2^-8
    if 4 * n * rich < 2 ** 24:
        return (4, 2), (2, 2), (16, 4)
    return (2, 1), (1, 1), (4, 2)


def pack9(w):
    """[O][I][3][3] -> the packed fp32 layout [9][O][I] of conv_out and its data gradient (ddimx_pack_conv(DDIMX_F32, ..))."""
    return w.permute(2, 3, 0, 1).reshape(9, w.shape[0], w.shape[1]).contiguous()


def pack9_dgrad(w):
    """[C0][Cin][3][3] -> [9][Cin][C0], transposed and flipped: the layout of ddimx_pack_conv_dgrad(DDIMX_F32, .., O = C0, I = Cin)."""
    return w.flip(2, 3).permute(2, 3, 1, 0).reshape(9, w.shape[1], w.shape[0]).contiguous()


def operands(case):
    """fp64 operands of a case, every one a number of the dtype it is stored in."""
    tag, op, B, C0, cio, H, W = case["id"], case["op"], case["B"], case["C0"], case["cio"], case["H"], case["W"]
    if op == "in":
        (kx, px), (kw, pw), (kb, pb) = conv_in_ranges(case)
        return dict(x=X.dyadic(tag + ".x", (B, cio, H, W), kx, px), w=X.dyadic(tag + ".w", (C0, cio, 3, 3), kw, pw),
                    bias=X.dyadic(tag + ".b", (C0,), kb, pb))
    if op == "out":
        return dict(a=X.dyadic(tag + ".a", (B, H, W, C0), 8, 3), b=X.dyadic(tag + ".b", (B, H, W, C0), 8, 3),
                    w=X.dyadic(tag + ".w", (cio, C0, 3, 3), 8, 6), bias=X.dyadic(tag + ".bias", (cio,), 512, 10))
    if op == "inbd":
        return dict(dy=X.dyadic(tag + ".dy", (B, H, W, C0), 15, 4), w=X.dyadic(tag + ".w", (C0, cio, 3, 3), 15, 5))
    kg, ks = wgrad_ranges(case)
    if op == "inb":
        return dict(dy=X.dyadic(tag + ".dy", (B, H, W, C0), kg, 3), x=X.dyadic(tag + ".x", (B, cio, H, W), ks, 3))
    assert op == "outb"
    return dict(de=X.dyadic(tag + ".de", (B, cio, H, W), ks, 3), a=X.dyadic(tag + ".a", (B, H, W, C0), kg // 2, 3),
                b=X.dyadic(tag + ".b", (B, H, W, C0), kg // 2, 3), w=X.dyadic(tag + ".w", (cio, C0, 3, 3), 8, 6))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_out_dgrad(den, w):
    """Gradient w.r.t. the input of Conv2d(C0 -> cout, k3, p1): den [B][H][W][cout], w [cout][C0][3][3] -> [B][H][W][C0]."""
    return X.conv3(den, w.transpose(0, 1).flip(2, 3))


def reference(case, op_=None):
    """fp64 values of every output of the case's export, in the layouts the kernels write (dtype: that of the operands, so the
    float32 evaluation of test_edge_cpu.py runs the same code)."""
    op_ = operands(case) if op_ is None else op_
    op = case["op"]
    if op == "in":
        return dict(y=X.conv3(nhwc(op_["x"]), op_["w"], op_["bias"]))
    if op == "out":
        return dict(eps=X.conv3(op_["a"] + op_["b"], op_["w"], op_["bias"]).permute(0, 3, 1, 2).contiguous())
    if op == "inbd":
        return dict(d_x=F.conv_transpose2d(op_["dy"].permute(0, 3, 1, 2), op_["w"], padding=1))
    if op == "inb":
        return dict(d_w=X.wgrad3(nhwc(op_["x"]), op_["dy"]), d_b=op_["dy"].sum((0, 1, 2)))
    den = nhwc(op_["de"])
    return dict(d_sum=conv_out_dgrad(den, op_["w"]), d_w=X.wgrad3(op_["a"] + op_["b"], den), d_b=den.sum((0, 1, 2)))
