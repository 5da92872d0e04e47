"""Case tables of the exact-operand tests (tests/test_gpu_exact.py and tests/test_gpu_train_exact.py run them, tests/test_exact_cpu.py
checks that each reaches the kernel family / variant / tiling it declares, and that its operand ranges make every summation order
exact)."""
import torch

import exact_util as X

DTN = {X.F32: "f32", X.BF16: "bf16"}


def _flags(fam, xf, act):
    f = X.P_XF(xf) | X.P_ACT(act)
    if fam == X.RING:
        return f  # ddimx_conv3x3_fwd: no fragment weights, no statistics
    if fam == X.WREG:
        return f | X.P_WFRAG | X.P_STATS | X.P_PREF(1)
    return f | X.P_WFRAG | X.P_STATS | X.P_GROUPS | X.P_PREF(2)


def _conv(dt, fam, C, B, H, W, xf, act, add=False, control=False, **want):
    return dict(id=f"{X.FAMILY[fam]}-{DTN[dt]}-C{C}-{B}x{H}x{W}-xf{xf}-act{act}{'-temb' if add else ''}", dt=dt, family=fam, C=C, B=B,
                H=H, W=W, xf=xf, act=act, add=add, control=control, flags=_flags(fam, xf, act), want=want)


CONV_CASES = []
for _dt in (X.F32, X.BF16):
    CONV_CASES += [
        _conv(_dt, X.RING, 32, 3, 13, 20, 1, 0, control=True, ragged_h=True, ragged_w=True),
        _conv(_dt, X.RING, 32, 1, 1040, 32, 0, 0, add=True, multi=_dt == X.F32),
        _conv(_dt, X.RING, 64, 1, 1040, 32, 2, 1, add=True, multi=True, short_last=_dt == X.F32),
        _conv(_dt, X.RING, 64, 2, 40, 64, 1, 1, ragged=False),
        _conv(_dt, X.RING, 96, 3, 13, 20, 1, 1, ragged_h=True),
        _conv(_dt, X.RING, 128, 3, 13, 20, 0, 0, var=1 if _dt == X.BF16 else 0, ragged_h=True),
        _conv(_dt, X.RING, 128, 1, 64, 256, 1, 0, add=True, var=0, multi=_dt == X.F32),
        _conv(_dt, X.RING, 192, 2, 40, 64, 2, 1, add=True, var=1 if _dt == X.BF16 else 0),
        _conv(_dt, X.RING, 192, 1, 1040, 32, 1, 0, var=0, multi=True, short_last=True),
        _conv(_dt, X.RING, 256, 3, 13, 20, 1, 0, control=_dt == X.BF16, var=1 if _dt == X.BF16 else 0, ragged_h=True),
        _conv(_dt, X.RING, 256, 1, 64, 256, 0, 0, add=True, var=0),
    ]
CONV_CASES += [
    _conv(X.BF16, X.WREG, 64, 2, 16, 64, 0, 0, control=True),
    _conv(X.BF16, X.WREG, 64, 2, 16, 64, 2, 1, add=True),
    _conv(X.BF16, X.WREG, 96, 2, 16, 32, 1, 1),
    _conv(X.BF16, X.WREG, 128, 2, 8, 64, 1, 0),
    _conv(X.BF16, X.WREG, 192, 2, 8, 32, 2, 1, add=True),
    _conv(X.BF16, X.WREG, 256, 2, 8, 16, 0, 0, control=True),
    _conv(X.BF16, X.WREG, 256, 2, 8, 16, 1, 1),
    _conv(X.BF16, X.WREG, 64, 1, 1048, 32, 1, 0, multi=True),   # tall: two tiles per workgroup, the weight ring wraps
    _conv(X.BF16, X.WREG, 96, 1, 1040, 32, 2, 1, add=True, multi=True),
    _conv(X.BF16, X.PIPE, 32, 2, 8, 32, 1, 1, control=True, multi=False),       # one tile
    _conv(X.BF16, X.PIPE, 32, 2, 48, 64, 2, 1, add=True, multi=True),            # several tiles per workgroup
    _conv(X.BF16, X.PIPE, 32, 3, 16 * 17, 32, 1, 1, multi=True, short_last=True),  # a second, shorter workgroup per sample
    _conv(X.BF16, X.PIPE, 32, 1, 64, 256, 2, 1, add=True, multi=True),            # full-width rows
    _conv(X.BF16, X.PIPE, 64, 2, 8, 32, 2, 1, add=True, control=True),
    _conv(X.BF16, X.PIPE, 64, 2, 24, 64, 1, 1, multi=True),
    _conv(X.BF16, X.PIPE, 64, 3, 8 * 9, 32, 2, 1, multi=True, short_last=True),
    _conv(X.BF16, X.PIPE, 64, 1, 40, 128, 1, 1, multi=True),
]

# Downsample (mode 1: input size) and Upsample + skip (mode 2: input size) at every (Cin, Cout) of the audio config
DOWN_PAIRS = [(32, 64, 32, 64), (64, 96, 16, 64), (96, 128, 16, 32), (128, 192, 16, 32), (192, 256, 8, 32)]
UP_PAIRS = [(256, 192, 8, 16), (192, 128, 8, 32), (128, 96, 8, 64), (96, 64, 8, 64), (64, 32, 16, 64)]


def _du(dt, fam, mode, cin, cout, B, H, W, control=False):
    flags = (X.P_WFRAG | X.P_STATS) if fam == X.WREG else 0
    if mode == X.UP4:
        flags |= X.P_SKIP
    name = "down" if mode == X.DOWN4 else "up"
    return dict(id=f"{name}-{X.FAMILY[fam]}-{DTN[dt]}-{cin}to{cout}-{B}x{H}x{W}", dt=dt, family=fam, mode=mode, cin=cin, cout=cout, B=B,
                H=H, W=W, control=control, flags=flags, want={})


DOWNUP_CASES = []
for _i, (_ci, _co, _h, _w) in enumerate(DOWN_PAIRS):
    DOWNUP_CASES += [_du(X.F32, X.RING, X.DOWN4, _ci, _co, 2, _h, _w), _du(X.BF16, X.RING, X.DOWN4, _ci, _co, 2, _h, _w, control=_i == 0),
                     _du(X.BF16, X.WREG, X.DOWN4, _ci, _co, 2, _h, _w, control=_i == 2)]
for _i, (_ci, _co, _h, _w) in enumerate(UP_PAIRS):
    DOWNUP_CASES += [_du(X.F32, X.RING, X.UP4, _ci, _co, 2, _h, _w), _du(X.BF16, X.RING, X.UP4, _ci, _co, 2, _h, _w),
                     _du(X.BF16, X.WREG, X.UP4, _ci, _co, 2, _h, _w, control=_i == 4)]


# bf16 ring forms of the deep levels in their large-tile variant (long spectrograms / the training walk reach it)
DOWNUP_CASES += [_du(X.BF16, X.RING, X.DOWN4, 128, 192, 1, 128, 128), _du(X.BF16, X.RING, X.DOWN4, 192, 256, 1, 64, 64),
                 _du(X.BF16, X.RING, X.UP4, 256, 192, 1, 32, 32)]
# ragged tiles and several tiles per workgroup (short / long spectrograms)
for _dt in (X.F32, X.BF16):
    DOWNUP_CASES += [_du(_dt, X.RING, X.DOWN4, 32, 64, 1, 26, 40), _du(_dt, X.RING, X.DOWN4, 32, 64, 1, 256, 256),
                     _du(_dt, X.RING, X.UP4, 64, 32, 1, 13, 20)]
DOWNUP_CASES += [_du(X.F32, X.RING, X.UP4, 64, 32, 1, 128, 128), _du(X.BF16, X.RING, X.UP4, 256, 192, 1, 64, 128),
                 _du(X.BF16, X.WREG, X.DOWN4, 32, 64, 1, 128, 256), _du(X.BF16, X.WREG, X.UP4, 256, 192, 1, 64, 64)]


# One case per further (family, mode, cin, cout, dtype, variant, ragged, multi-tile workgroup) key that the inference and training
# walks launch (tests/test_exact_cpu.py enumerates them): the smallest shape of the per-op entry point that reaches the key.
# (dtype, family, mode, cin, cout, B, H, W), H x W the input's size.
KEY_ROWS = [
    (X.F32, X.RING, X.CONV3, 32, 32, 1, 8, 32),  # var 0
    (X.BF16, X.RING, X.CONV3, 32, 32, 1, 1040, 64),  # var 0 multi
    (X.BF16, X.RING, X.CONV3, 64, 64, 1, 4, 8),  # var 0 ragged
    (X.BF16, X.RING, X.CONV3, 64, 64, 1, 1040, 8),  # var 0 ragged multi
    (X.F32, X.RING, X.CONV3, 96, 96, 1, 8, 16),  # var 0
    (X.F32, X.RING, X.CONV3, 96, 96, 1, 1040, 16),  # var 0 multi
    (X.F32, X.RING, X.CONV3, 96, 96, 1, 1040, 8),  # var 0 ragged multi
    (X.BF16, X.RING, X.CONV3, 96, 96, 1, 8, 32),  # var 0
    (X.BF16, X.RING, X.CONV3, 96, 96, 1, 1040, 32),  # var 0 multi
    (X.BF16, X.RING, X.CONV3, 96, 96, 1, 1040, 8),  # var 0 ragged multi
    (X.F32, X.RING, X.CONV3, 128, 128, 1, 8, 8),  # var 0
    (X.BF16, X.RING, X.CONV3, 128, 128, 1, 1040, 16),  # var 0 multi
    (X.BF16, X.RING, X.CONV3, 128, 128, 1, 8, 8),  # var 1
    (X.F32, X.RING, X.CONV3, 192, 192, 1, 4, 8),  # var 0 ragged
    (X.BF16, X.RING, X.CONV3, 192, 192, 1, 40, 96),  # var 0
    (X.BF16, X.RING, X.CONV3, 192, 192, 1, 4, 8),  # var 1 ragged
    (X.F32, X.RING, X.CONV3, 256, 256, 1, 8, 8),  # var 0
    (X.BF16, X.RING, X.CONV3, 256, 256, 1, 8, 8),  # var 1
    (X.F32, X.RING, X.DOWN4, 64, 96, 1, 128, 256),  # var 0 multi
    (X.BF16, X.RING, X.DOWN4, 64, 96, 1, 256, 256),  # var 0 multi
    (X.BF16, X.RING, X.DOWN4, 64, 96, 1, 4, 8),  # var 0 ragged
    (X.BF16, X.RING, X.DOWN4, 64, 96, 1, 1024, 40),  # var 0 ragged multi
    (X.F32, X.RING, X.DOWN4, 96, 128, 1, 64, 256),  # var 0 multi
    (X.BF16, X.RING, X.DOWN4, 96, 128, 1, 128, 256),  # var 0 multi
    (X.BF16, X.RING, X.DOWN4, 96, 128, 1, 4, 8),  # var 0 ragged
    (X.F32, X.RING, X.DOWN4, 128, 192, 1, 64, 256),  # var 0 multi
    (X.F32, X.RING, X.DOWN4, 128, 192, 1, 4, 8),  # var 0 ragged
    (X.BF16, X.RING, X.DOWN4, 128, 192, 1, 128, 256),  # var 0 multi
    (X.BF16, X.RING, X.DOWN4, 128, 192, 1, 4, 8),  # var 1 ragged
    (X.F32, X.RING, X.DOWN4, 192, 256, 1, 4, 8),  # var 0 ragged
    (X.BF16, X.RING, X.DOWN4, 192, 256, 1, 4, 8),  # var 1 ragged
    (X.BF16, X.RING, X.UP4, 64, 32, 1, 256, 256),  # var 0 multi
    (X.BF16, X.RING, X.UP4, 64, 32, 1, 1024, 40),  # var 0 ragged multi
    (X.F32, X.RING, X.UP4, 96, 64, 1, 32, 256),  # var 0 multi
    (X.BF16, X.RING, X.UP4, 96, 64, 1, 64, 256),  # var 0 multi
    (X.BF16, X.RING, X.UP4, 96, 64, 1, 4, 8),  # var 0 ragged
    (X.BF16, X.RING, X.UP4, 96, 64, 1, 1024, 8),  # var 0 ragged multi
    (X.F32, X.RING, X.UP4, 128, 96, 1, 16, 256),  # var 0 multi
    (X.BF16, X.RING, X.UP4, 128, 96, 1, 32, 256),  # var 0 multi
    (X.BF16, X.RING, X.UP4, 128, 96, 1, 4, 8),  # var 0 ragged
    (X.F32, X.RING, X.UP4, 192, 128, 1, 16, 256),  # var 0 multi
    (X.F32, X.RING, X.UP4, 192, 128, 1, 4, 12),  # var 0 ragged
    (X.BF16, X.RING, X.UP4, 192, 128, 1, 4, 8),  # var 0 ragged
    (X.F32, X.RING, X.UP4, 256, 192, 1, 4, 12),  # var 0 ragged
    (X.BF16, X.WREG, X.CONV3, 128, 128, 1, 264, 64),  # var 0 multi
    (X.BF16, X.WREG, X.DOWN4, 64, 96, 1, 64, 256),  # var 0 multi
    (X.BF16, X.WREG, X.DOWN4, 96, 128, 1, 64, 256),  # var 0 multi
    (X.BF16, X.WREG, X.DOWN4, 128, 192, 1, 32, 256),  # var 0 multi
    (X.BF16, X.WREG, X.DOWN4, 192, 256, 1, 32, 256),  # var 0 multi
    (X.BF16, X.WREG, X.UP4, 64, 32, 1, 64, 256),  # var 0 multi
    (X.BF16, X.WREG, X.UP4, 96, 64, 1, 32, 256),  # var 0 multi
    (X.BF16, X.WREG, X.UP4, 128, 96, 1, 32, 256),  # var 0 multi
    (X.BF16, X.WREG, X.UP4, 192, 128, 1, 16, 256),  # var 0 multi
]
_XA = [(0, 0), (1, 0), (2, 1), (1, 1)]
for _i, (_dt, _fam, _mode, _ci, _co, _b, _h, _w) in enumerate(KEY_ROWS):
    if _mode == X.CONV3:
        CONV_CASES.append(_conv(_dt, _fam, _ci, _b, _h, _w, *(_XA[_i % 4] if _fam == X.RING else (1, 0)), add=_i % 3 == 0))
    else:
        DOWNUP_CASES.append(_du(_dt, _fam, _mode, _ci, _co, _b, _h, _w))


def _wg(dt, C, B, H, W, xf, **want):
    return dict(id=f"wgrad-{DTN[dt]}-C{C}-{B}x{H}x{W}-xf{xf}", dt=dt, C=C, B=B, H=H, W=W, xf=xf, want=want)


WGRAD_CASES = []
for _dt in (X.F32, X.BF16):
    for _j, _c in enumerate((32, 64, 96, 128, 192, 256)):
        WGRAD_CASES += [_wg(_dt, _c, 2, 8, 16, (0, 1, 2, 3)[_j % 4], many=False),
                        _wg(_dt, _c, 2, 64, 128, (1, 2, 3, 0)[_j % 4], many=_c <= 128)]


def _dub(dt, mode, cin, cout, B, H, W, reduce):
    name = "down" if mode == X.DOWN4 else "up"
    return dict(id=f"{name}bwd-{DTN[dt]}-{cin}to{cout}-{B}x{H}x{W}", dt=dt, mode=mode, cin=cin, cout=cout, B=B, H=H, W=W, reduce=reduce)


DUBWD_CASES = []
for _dt in (X.F32, X.BF16):
    DUBWD_CASES += [_dub(_dt, X.DOWN4, 32, 64, 2, 16, 32, "ks4"), _dub(_dt, X.DOWN4, 32, 64, 2, 128, 128, "quad"),
                    _dub(_dt, X.DOWN4, 192, 256, 2, 8, 16, "ks4"),
                    _dub(_dt, X.UP4, 64, 32, 2, 8, 16, "ks4"), _dub(_dt, X.UP4, 64, 32, 2, 64, 64, "quad"),
                    _dub(_dt, X.UP4, 256, 192, 2, 4, 8, "ks4")]
# the data gradient of Upsample 192 -> 128 is a Downsample 128 -> 192 planned on the real batch: variant 1 with several tiles per
# workgroup, which no forward entry point reaches
DUBWD_CASES.append(_dub(X.BF16, X.UP4, 192, 128, 1, 64, 64, "quad"))


# ---- one weight-gradient case per key the training walk launches -------------------------------------------------------------------
# X.wgrad_key: kernel key (mode, ci, co, dtype, xf, ragged_h, ragged_w, multi, crossing, short_last) and reduce key (kind, unrolled,
# tail, disagree).  tests/test_exact_cpu.py enumerates the walk's keys and checks that every row below reaches the key it names.
WGRAD_WIDTHS = [(X.CONV3, _c, _c) for _c in (32, 64, 96, 128, 192, 256)] + \
               [(X.DOWN4, 32, 64), (X.DOWN4, 64, 96), (X.DOWN4, 96, 128), (X.DOWN4, 128, 192), (X.DOWN4, 192, 256)]
WG_FLAGS = "hwmcs"  # ragged_h, ragged_w, multi, crossing, short_last: a row names the ones that are set
WG_MAX_TILES = 1024


def wgrad_shapes_by_size(dt, mode, ci, co, max_b=4):
    """Every (B, Hd, Wd) that can give (dt, mode, ci, co) a plan of its own, smallest B Hd Wd first: the plan depends on the tile
    counts, and the key besides on whether the last tile row / column is whole, so one shape per (B, tiles_y, tiles_x, ragged_h,
    ragged_w) -- the smallest, whose ragged tiles keep one row / column -- is enough.  Wd <= 272: one tile past the widest level."""
    p = X.wgrad_plan(dt, mode, ci, co, 1, 1, 1)
    th, tw = p["th"], p["tw"]
    out = []
    for B in range(1, max_b + 1):
        for tx in range(1, 18):
            for ty in range(1, WG_MAX_TILES // (B * tx) + 1):
                out += [(B, ty * th - rh * (th - 1), tx * tw - rw * (tw - 1)) for rh in (0, 1) for rw in (0, 1)]
    return sorted(out, key=lambda s: (s[0] * s[1] * s[2],) + s)


def smallest_wgrad_shapes(dt, mode, ci, co, xf, kernel_keys=(), reduce_keys=()):
    """{key: (B, Hd, Wd)}: for each wanted kernel / reduce key of (dt, mode, ci, co) the smallest shape by B Hd Wd that the library's
    plan maps to it.  The tables below were found with it once and are frozen; nothing calls it at import."""
    want = set(kernel_keys) | set(reduce_keys)
    found = {}
    for B, H, W in wgrad_shapes_by_size(dt, mode, ci, co):
        for k in X.wgrad_key(dt, mode, ci, co, B, H, W, xf):
            if k in want and k not in found:
                found[k] = (B, H, W)
        if len(found) == len(want):
            break
    return found


def wg_flags(kernel_key):
    return "".join(f for f, on in zip(WG_FLAGS, kernel_key[5:]) if on)


_SILU = (X.XF_AFFINE_SILU, X.XF_SILU_AFFINE)
# (mode, ci, co, B, Hd, Wd, flags, transforms) with Hd x Wd the size of du; the plan does not depend on the dtype, so each row is
# a case in fp32 and in bf16.  3x3: the walk's two transforms (conv.0, conv.1 of the block) unless an older case has the key.
WGRAD_KEY_ROWS = [
    (X.CONV3, 32, 32, 1, 8, 16, "", _SILU),
    (X.CONV3, 32, 32, 1, 280, 176, "ms", _SILU),
    (X.CONV3, 32, 32, 1, 1544, 32, "m", _SILU),
    (X.CONV3, 32, 32, 2, 1544, 16, "mc", _SILU),
    (X.CONV3, 32, 32, 3, 344, 48, "mcs", _SILU),
    (X.CONV3, 64, 64, 1, 8, 16, "", (X.XF_SILU_AFFINE,)),
    (X.CONV3, 64, 64, 1, 280, 176, "ms", _SILU),
    (X.CONV3, 64, 64, 1, 1544, 32, "m", _SILU),
    (X.CONV3, 64, 64, 3, 344, 48, "mcs", _SILU),
    (X.CONV3, 96, 96, 1, 8, 1, "w", _SILU),
    (X.CONV3, 96, 96, 1, 1040, 1, "wm", _SILU),
    (X.CONV3, 96, 96, 2, 520, 1, "wmc", _SILU),
    (X.CONV3, 96, 96, 1, 80, 208, "m", _SILU),
    (X.CONV3, 96, 96, 2, 40, 208, "mc", _SILU),
    (X.CONV3, 128, 128, 1, 1, 16, "h", _SILU),
    (X.CONV3, 128, 128, 1, 8, 16, "", (X.XF_AFFINE_SILU,)),
    (X.CONV3, 128, 128, 3, 9, 272, "hm", _SILU),
    (X.CONV3, 128, 128, 1, 776, 16, "ms", _SILU),
    (X.CONV3, 128, 128, 1, 56, 224, "m", _SILU),
    (X.CONV3, 128, 128, 3, 24, 176, "mcs", _SILU),
    (X.CONV3, 192, 192, 1, 1, 16, "h", _SILU),
    (X.CONV3, 192, 192, 1, 8, 16, "", _SILU),
    (X.CONV3, 192, 192, 1, 32, 176, "m", _SILU),
    (X.CONV3, 192, 192, 4, 8, 176, "mc", _SILU),
    (X.CONV3, 192, 192, 3, 8, 240, "mcs", _SILU),
    (X.CONV3, 256, 256, 1, 1, 1, "hw", _SILU),
    (X.CONV3, 256, 256, 1, 8, 1, "w", _SILU),
    (X.CONV3, 256, 256, 2, 97, 1, "hwmc", _SILU),
    (X.CONV3, 256, 256, 1, 208, 1, "wm", _SILU),
    (X.CONV3, 256, 256, 2, 104, 1, "wmc", _SILU),
    (X.CONV3, 256, 256, 3, 72, 1, "wmcs", _SILU),
    (X.DOWN4, 32, 64, 1, 140, 176, "ms", (X.XF_NONE,)),
    (X.DOWN4, 32, 64, 1, 772, 32, "m", (X.XF_NONE,)),
    (X.DOWN4, 32, 64, 3, 172, 48, "mcs", (X.XF_NONE,)),
    (X.DOWN4, 64, 96, 1, 4, 1, "w", (X.XF_NONE,)),
    (X.DOWN4, 64, 96, 1, 4, 16, "", (X.XF_NONE,)),
    (X.DOWN4, 64, 96, 1, 772, 1, "wms", (X.XF_NONE,)),
    (X.DOWN4, 64, 96, 1, 776, 1, "wm", (X.XF_NONE,)),
    (X.DOWN4, 64, 96, 3, 260, 1, "wmcs", (X.XF_NONE,)),
    (X.DOWN4, 64, 96, 1, 772, 16, "ms", (X.XF_NONE,)),
    (X.DOWN4, 64, 96, 1, 388, 32, "m", (X.XF_NONE,)),
    (X.DOWN4, 64, 96, 3, 20, 208, "mcs", (X.XF_NONE,)),
    (X.DOWN4, 96, 128, 1, 4, 16, "", (X.XF_NONE,)),
    (X.DOWN4, 96, 128, 1, 24, 176, "m", (X.XF_NONE,)),
    (X.DOWN4, 96, 128, 2, 12, 176, "mc", (X.XF_NONE,)),
    (X.DOWN4, 128, 192, 1, 1, 16, "h", (X.XF_NONE,)),
    (X.DOWN4, 128, 192, 1, 4, 16, "", (X.XF_NONE,)),
    (X.DOWN4, 128, 192, 1, 24, 176, "m", (X.XF_NONE,)),
    (X.DOWN4, 128, 192, 2, 12, 176, "mc", (X.XF_NONE,)),
    (X.DOWN4, 192, 256, 1, 1, 1, "hw", (X.XF_NONE,)),
    (X.DOWN4, 192, 256, 1, 136, 1, "wm", (X.XF_NONE,)),
    (X.DOWN4, 192, 256, 2, 68, 1, "wmc", (X.XF_NONE,)),
]
# The reduce keys no row above reaches under the exact criterion: (mode, ci, co, B, Hd, Wd, transform, reduce key).  Two or more
# unrolled iterations of the 16-thread form need 241 slabs or more, which only the widths with one workgroup per (co, ci) group
# plan (32, 64, 32 -> 64); of the 4-thread form 61 to 63 slabs, which no walk of the sweep plans -- the last two rows of each
# form run it all the same.
WGRAD_REDUCE_ROWS = [
    (X.DOWN4, 32, 64, 1, 961, 1, X.XF_NONE, ("quad", 2, True, True)),
    (X.DOWN4, 32, 64, 3, 341, 1, X.XF_NONE, ("quad", 2, True, False)),
    (X.DOWN4, 32, 64, 4, 253, 1, X.XF_NONE, ("quad", 2, False, False)),
    (X.DOWN4, 96, 128, 1, 241, 1, X.XF_NONE, ("ks4", 2, True, True)),
    (X.CONV3, 32, 32, 1, 1921, 1, X.XF_AFFINE, ("quad", 2, True, True)),
    (X.CONV3, 32, 32, 4, 505, 1, X.XF_AFFINE, ("quad", 2, False, False)),
    (X.CONV3, 96, 96, 4, 249, 1, X.XF_AFFINE, ("quad", 1, False, False)),
    (X.CONV3, 128, 128, 3, 81, 1, X.XF_AFFINE, ("ks4", 1, True, False)),
    (X.CONV3, 128, 128, 1, 481, 1, X.XF_AFFINE, ("ks4", 2, True, True)),
]


def _wgk(dt, C, B, H, W, xf, flags, reduce=None):
    return dict(id=f"wgkey-{DTN[dt]}-C{C}-{B}x{H}x{W}-xf{xf}", dt=dt, C=C, B=B, H=H, W=W, xf=xf, flags=flags, reduce=reduce,
                sparse=xf in _SILU)


def _dubk(dt, i, ci, co, B, Hd, Wd, flags, reduce=None):
    """The stride-2 weight gradient (ci: the channels of the large side, co: of the small one) through ddimx_downsample_bwd (even
    rows of the tables) or ddimx_upsample_add_bwd (odd rows), which plan the same launch."""
    c = _dub(dt, X.DOWN4, ci, co, B, 2 * Hd, 2 * Wd, None) if i % 2 == 0 else _dub(dt, X.UP4, co, ci, B, Hd, Wd, None)
    return dict(c, flags=flags, reduce=reduce, wkey=(ci, co, B, Hd, Wd))


WGRAD_KEY_CASES, DUBWD_KEY_CASES = [], []
for _dt in (X.F32, X.BF16):
    for _i, (_mode, _ci, _co, _b, _h, _w, _f, _xfs) in enumerate(WGRAD_KEY_ROWS):
        if _mode == X.CONV3:
            WGRAD_KEY_CASES += [_wgk(_dt, _ci, _b, _h, _w, _xf, _f) for _xf in _xfs]
        else:
            DUBWD_KEY_CASES.append(_dubk(_dt, _i, _ci, _co, _b, _h, _w, _f))
    for _i, (_mode, _ci, _co, _b, _h, _w, _xf, _r) in enumerate(WGRAD_REDUCE_ROWS):
        if _mode == X.CONV3:
            WGRAD_KEY_CASES.append(_wgk(_dt, _ci, _b, _h, _w, _xf, None, _r))
        else:
            DUBWD_KEY_CASES.append(_dubk(_dt, _i, _ci, _co, _b, _h, _w, None, _r))


def case_wgrad_key(c):
    """(kernel key, reduce key) of the weight-gradient launch of a WGRAD_* or DUBWD_* case."""
    if "C" in c:
        return X.wgrad_key(c["dt"], X.CONV3, c["C"], c["C"], c["B"], c["H"], c["W"], c["xf"])
    if c["mode"] == X.DOWN4:
        return X.wgrad_key(c["dt"], X.DOWN4, c["cin"], c["cout"], c["B"], c["H"] // 2, c["W"] // 2, X.XF_NONE)
    return X.wgrad_key(c["dt"], X.DOWN4, c["cout"], c["cin"], c["B"], c["H"], c["W"], X.XF_NONE)


WG_HOT_TILES = 16


def wgrad_hot_tiles(case):
    """The tiles (numbered sample-major) on which a sparse 3x3 case keeps du: the first and the last tile of the first workgroup and
    of the last (the short) one; one tile of the last tile row and one of the last tile column (the ragged ones) with the first
    tile of that column's tile row, whose pixels follow the cut ones in memory; and the first and last tile of every workgroup
    whose range runs into the next sample, with the two tiles at the boundary."""
    p = X.wgrad_plan(case["dt"], X.CONV3, case["C"], case["C"], case["B"], case["H"], case["W"])
    ts = p["tiles_x"] * p["tiles_y"]
    ranges = X.wgrad_ranges(p, case["B"])
    hot = [ranges[0][0], ranges[0][1] - 1, ranges[-1][0], ranges[-1][1] - 1, ts - p["tiles_x"], p["tiles_x"] - 1, 0]
    for t0, t1 in ranges:
        for edge in range((t0 // ts + 1) * ts, t1, ts):
            hot += [t0, edge - 1, edge, t1 - 1]
    hot = sorted(set(hot))
    assert len(hot) <= WG_HOT_TILES, (case["id"], hot)
    return hot


def wgrad_tile_mask(case, tiles):
    """[B][H][W] bool: the pixels of the given tiles."""
    p = X.wgrad_plan(case["dt"], X.CONV3, case["C"], case["C"], case["B"], case["H"], case["W"])
    ts = p["tiles_x"] * p["tiles_y"]
    m = torch.zeros(case["B"], case["H"], case["W"], dtype=torch.bool)
    for t in tiles:
        b, ty, tx = t // ts, t % ts // p["tiles_x"], t % p["tiles_x"]
        m[b, ty * p["th"]:(ty + 1) * p["th"], tx * p["tw"]:(tx + 1) * p["tw"]] = True
    return m


def _regen(tag, x, s, h, xf, k, p):
    """Redraw the elements of NHWC x whose transformed value X.xf64(x, s, h, xf) lies within 2^-18 of a bf16 rounding midpoint (each
    round draws a whole tensor and takes its values at the elements still too close: only those are transformed again)."""
    idx = X.near_midpoint(X.xf64(x, s, h, xf)).nonzero(as_tuple=True)
    x = x.clone()
    for it in range(64):
        if idx[0].numel() == 0:
            return x
        v = X.dyadic(f"{tag}.re{it}", tuple(x.shape), k, p)[idx]
        x[idx] = v
        sv, hv = s[idx[0], idx[3]], h[idx[0], idx[3]]
        still = X.near_midpoint(X.silu64(v * sv + hv) if xf == X.XF_AFFINE_SILU else X.silu64(v) * sv + hv)
        idx = tuple(i[still] for i in idx)
    raise AssertionError(f"{tag}: could not keep the SiLU operands off the bf16 midpoints")


def conv_operands(case):
    """x on k/8, w on k/64 (|k| <= 8), scale on {0.5, 1, 1.5, 2}, shift on k/16 (|k| <= 16), bias / temb on k/1024 (|k| <= 512).
    a_ref: the conv's operand as the kernel multiplies it (bf16 mode: RNE of the SiLU)."""
    tag, C, B, H, W, xf = case["id"], case["C"], case["B"], case["H"], case["W"], case["xf"]
    x = X.dyadic(tag + ".x", (B, H, W, C), 8, 3)
    s, h = X.scales(tag + ".s", (B, C)), X.dyadic(tag + ".h", (B, C), 16, 4)
    silu = xf in (X.XF_AFFINE_SILU, X.XF_SILU_AFFINE)
    if silu and case["dt"] == X.BF16:
        x = _regen(tag + ".x", x, s, h, xf, 8, 3)
    a = X.xf64(x, s, h, xf)
    if silu and case["dt"] == X.BF16:
        a = X.rne(a)
    w = X.dyadic(tag + ".w", (C, C, 3, 3), 8, 6)
    extra = X.dyadic(tag + ".b", (C,), 512, 10)
    temb = X.dyadic(tag + ".t", (B, C), 512, 10)
    return dict(x=x, w=w, scale=s, shift=h, a_ref=a, bias=None if case["add"] else extra, add=temb if case["add"] else None)


def wgrad_operands(case):
    """a on k/8 (|k| <= 8) before the input transform, du on k/64 (|k| <= 8); dW sums B H W terms."""
    tag, C, B, H, W, xf = case["id"], case["C"], case["B"], case["H"], case["W"], case["xf"]
    a = X.dyadic(tag + ".a", (B, H, W, C), 8, 3)
    s, h = X.scales(tag + ".s", (B, C)), X.dyadic(tag + ".h", (B, C), 16, 4)
    if xf in (X.XF_AFFINE_SILU, X.XF_SILU_AFFINE) and case["dt"] == X.BF16:
        a = _regen(tag + ".a", a, s, h, xf, 8, 3)
    a_ref = X.xf64(a, s, h, xf)
    if xf in (X.XF_AFFINE_SILU, X.XF_SILU_AFFINE) and case["dt"] == X.BF16:
        a_ref = X.rne(a_ref)
    du = X.dyadic(tag + ".du", (B, H, W, C), 8, 6)
    if case.get("sparse"):  # the plan depends on the shape alone: du lives on the tiles that matter, `a` stays dense
        du = du * wgrad_tile_mask(case, wgrad_hot_tiles(case))[..., None]
    return dict(a=a, du=du, scale=s, shift=h, a_ref=a_ref)


def wgrad_delta(case, a_ref, du):
    """The bound of the kernel's inexact summation where SiLU makes the products inexact sums (None: criterion E): n 2^-23 sum |a||du|
    with n the number of pixels whose du is not zero (a zero term rounds nothing), + 2^-20 sum |a||du| in fp32, which keeps
    silu_f's own value."""
    if case["xf"] not in _SILU:
        return None
    n = int((du != 0).any(-1).sum())
    mag = X.wgrad3(a_ref.abs(), du.abs())
    return n * 2.0 ** -23 * mag + (2.0 ** -20 * mag if case["dt"] == X.F32 else 0.0)


def dubwd_ranges(case):
    """((kx, px), (kd, pd)): x on k 2^-px with |k| <= kx, dy on k 2^-pd with |k| <= kd -- the widest pair whose weight-gradient sums
    over the case's own pixel count stay below 2^24 units of the product grid."""
    n = case["B"] * case["H"] * case["W"] * (4 if case["mode"] == X.UP4 else 1)  # pixels of the large side
    for kx, kd in ((8, 8), (4, 4), (2, 2), (1, 1)):
        if X.budget_bits(n // 4, kx / 8, 3, kd / 64, 6) < 24:
            return (kx, 3), (kd, 6)
    raise AssertionError(f"{case['id']}: too many pixels for an exact weight gradient")


def dubwd_operands(case):
    """x [B][H][W][cin], dy (Downsample: [B][H/2][W/2][cout], Upsample: [B][2H][2W][cout]) and the layer's weight on k/64, |k| <= 8."""
    tag, cin, cout, B, H, W = case["id"], case["cin"], case["cout"], case["B"], case["H"], case["W"]
    (kx, px), (kd, pd) = dubwd_ranges(case)
    down = case["mode"] == X.DOWN4
    return dict(x=X.dyadic(tag + ".x", (B, H, W, cin), kx, px),
                dy=X.dyadic(tag + ".dy", (B, H // 2, W // 2, cout) if down else (B, 2 * H, 2 * W, cout), kd, pd),
                w=X.dyadic(tag + ".w", (cout, cin, 4, 4) if down else (cin, cout, 4, 4), 8, 6),
                add=X.dyadic(tag + ".add", (B, H, W, cin), 8, 6) if down else None)  # Downsample: joins dx in the epilogue


# ---- the training-only paths of conv_mfma_kernel ------------------------------------------------------------------------------------
# One row per (C, dtype, variant, ragged, multi-tile workgroup) key the training forward launches at T in {32 .. 8192}, B in {1 .. 64}
# (tests/test_exact_cpu.py enumerates them): the smallest H x W at which ddimx_conv3x3_fwd_ex reaches the key.  Only (128, bf16,
# variant 1, several tiles) needs the plan on the real batch (DDIMX_PLAN_BATCH); every other row passes plan_flags = 0.
# (dtype, C, H, W, variant, ragged, multi, batch plan)
TRAIN_KEY_ROWS = [
    (X.F32, 32, 8, 32, 0, False, False, False),
    (X.F32, 32, 1032, 32, 0, False, True, False),
    (X.BF16, 32, 16, 32, 0, False, False, False),
    (X.BF16, 32, 1040, 64, 0, False, True, False),
    (X.F32, 64, 8, 16, 0, False, False, False),
    (X.F32, 64, 1032, 16, 0, False, True, False),
    (X.BF16, 64, 8, 32, 0, False, False, False),
    (X.BF16, 64, 1032, 32, 0, False, True, False),
    (X.BF16, 64, 1, 4, 0, True, False, False),
    (X.BF16, 64, 1032, 4, 0, True, True, False),
    (X.F32, 96, 8, 16, 0, False, False, False),
    (X.F32, 96, 1032, 16, 0, False, True, False),
    (X.F32, 96, 1, 4, 0, True, False, False),
    (X.F32, 96, 1032, 4, 0, True, True, False),
    (X.BF16, 96, 8, 32, 0, False, False, False),
    (X.BF16, 96, 1032, 32, 0, False, True, False),
    (X.BF16, 96, 1, 4, 0, True, False, False),
    (X.BF16, 96, 1032, 4, 0, True, True, False),
    (X.F32, 128, 8, 8, 0, False, False, False),
    (X.F32, 128, 1032, 8, 0, False, True, False),
    (X.F32, 128, 1, 4, 0, True, False, False),
    (X.BF16, 128, 200, 16, 0, False, False, False),
    (X.BF16, 128, 1032, 16, 0, False, True, False),
    (X.BF16, 128, 200, 4, 0, True, False, False),
    (X.BF16, 128, 8, 8, 1, False, False, False),
    (X.BF16, 128, 264, 32, 1, False, True, True),
    (X.BF16, 128, 1, 4, 1, True, False, False),
    (X.F32, 192, 8, 8, 0, False, False, False),
    (X.F32, 192, 1, 4, 0, True, False, False),
    (X.BF16, 192, 200, 16, 0, False, False, False),
    (X.BF16, 192, 8, 16, 1, False, False, False),
    (X.BF16, 192, 1, 4, 1, True, False, False),
    (X.F32, 256, 8, 8, 0, False, False, False),
    (X.F32, 256, 1, 4, 0, True, False, False),
    (X.BF16, 256, 400, 8, 0, False, False, False),
    (X.BF16, 256, 8, 8, 1, False, False, False),
    (X.BF16, 256, 1, 4, 1, True, False, False),
]
# (xf, chan_add instead of bias): conv.0 of the block (xf 2, + temb), conv.1 (xf 3, + bias); xf 0 / 1 put the act = 2 store under
# criterion E with no SiLU operand
_TXF = [(2, True), (3, False), (0, False), (2, True), (3, False), (1, True)]


def _small_batch(H, W):
    return 2 if H * W <= 4096 else 1


def _tf(i, dt, C, H, W, var, ragged, multi, batch):
    xf, add = _TXF[i % len(_TXF)]
    B = 1 if batch else _small_batch(H, W)
    flags = X.P_XF(xf) | X.P_ACT(2) | X.P_STATS | (X.P_BATCH if batch else 0)
    return dict(id=f"act2-{DTN[dt]}-C{C}-{B}x{H}x{W}-xf{xf}{'-temb' if add else ''}{'-batch' if batch else ''}", dt=dt, family=X.RING, C=C,
                B=B, H=H, W=W, xf=xf, act=2, add=add, batch=batch, flags=flags, want=dict(var=var, ragged=ragged, multi=multi))


TRAIN_FWD_CASES = [_tf(_i, *_r) for _i, _r in enumerate(TRAIN_KEY_ROWS)]

# ddimx_conv3x3_dgrad_stats (ConvCfg::BWD): one row per key whose data-gradient conv takes the GroupNorm-backward statistics in its
# epilogue somewhere in the same sweep, at the smallest H x W where the export does (*nparts > 0), each in both bwd_modes; then the
# rows that give every one of the 15 instantiations (9 bf16, 6 fp32) a ragged and a whole-tile epilogue.
# (dtype, C, H, W, variant, ragged, multi)
DGRAD_KEY_ROWS = [
    (X.F32, 32, 8, 32, 0, False, False),
    (X.F32, 32, 1032, 32, 0, False, True),
    (X.BF16, 32, 16, 32, 0, False, False),
    (X.BF16, 32, 1040, 64, 0, False, True),
    (X.F32, 64, 8, 16, 0, False, False),
    (X.F32, 64, 1032, 16, 0, False, True),
    (X.BF16, 64, 8, 32, 0, False, False),
    (X.BF16, 64, 1032, 32, 0, False, True),
    (X.BF16, 64, 1, 4, 0, True, False),
    (X.F32, 96, 8, 16, 0, False, False),
    (X.F32, 96, 1032, 16, 0, False, True),
    (X.F32, 96, 1, 4, 0, True, False),
    (X.F32, 96, 1032, 4, 0, True, True),
    (X.BF16, 96, 8, 32, 0, False, False),
    (X.BF16, 96, 1032, 32, 0, False, True),
    (X.BF16, 96, 1, 4, 0, True, False),
    (X.F32, 128, 8, 8, 0, False, False),
    (X.F32, 128, 1032, 8, 0, False, True),
    (X.F32, 128, 1, 4, 0, True, False),
    (X.BF16, 128, 200, 16, 0, False, False),
    (X.BF16, 128, 1032, 16, 0, False, True),
    (X.BF16, 128, 200, 4, 0, True, False),
    (X.BF16, 128, 8, 8, 1, False, False),
    (X.BF16, 128, 1, 4, 1, True, False),
    (X.F32, 192, 8, 8, 0, False, False),
    (X.F32, 192, 1, 4, 0, True, False),
    (X.BF16, 192, 200, 16, 0, False, False),
    (X.BF16, 192, 8, 16, 1, False, False),
    (X.BF16, 192, 1, 4, 1, True, False),
    (X.F32, 256, 8, 8, 0, False, False),
    (X.F32, 256, 1, 4, 0, True, False),
    (X.BF16, 256, 400, 8, 0, False, False),
    (X.BF16, 256, 8, 8, 1, False, False),
    (X.BF16, 256, 1, 4, 1, True, False),
    # no training shape of the sweep: the ragged epilogue of the remaining instantiations
    (X.F32, 32, 1, 4, 0, True, False),
    (X.BF16, 32, 1, 4, 0, True, False),
    (X.F32, 64, 1, 4, 0, True, False),
    (X.BF16, 192, 200, 4, 0, True, False),
    (X.BF16, 256, 392, 4, 0, True, False),
]
BWD_INSTANTIATIONS = [(X.F32, _c, 0) for _c in (32, 64, 96, 128, 192, 256)] + [(X.BF16, _c, 0) for _c in (32, 64, 96, 128, 192, 256)] + \
                     [(X.BF16, _c, 1) for _c in (128, 192, 256)]
_DG_CONTROLS = {(X.F32, 96, 8, 16, 1), (X.BF16, 128, 8, 8, 2)}  # (dtype, C, H, W, bwd_mode)


def _dg(dt, C, H, W, var, ragged, multi, mode):
    B = _small_batch(H, W)
    row = f"dgrad-{DTN[dt]}-C{C}-{B}x{H}x{W}"
    return dict(id=f"{row}-bwd{mode}", row=row, dt=dt, family=X.RING, C=C, B=B, H=H, W=W, bwd_mode=mode, flags=X.P_BWD | X.P_STATS,
                control=(dt, C, H, W, mode) in _DG_CONTROLS, want=dict(var=var, ragged=ragged, multi=multi))


DGRAD_CASES = [_dg(*_r, _m) for _r in DGRAD_KEY_ROWS for _m in (1, 2)]  # (the two modes of a row share their operands)


def dgrad_operands(case):
    """du on k/64 (|k| <= 8), w [Co][Ci][3][3] on k/64 (|k| <= 8), aux on k/8 (|k| <= 8), aux_scale on {0.5, 1, 1.5, 2}, aux_shift on
    k/16 (|k| <= 16).  dg sums 9 C products on the 2^-12 grid: 9 * 256 * (1/8) * (1/8) * 2^12 < 2^18, any summation order is exact."""
    tag, C, B, H, W = case["row"], case["C"], case["B"], case["H"], case["W"]
    return dict(du=X.dyadic(tag + ".du", (B, H, W, C), 8, 6), w=X.dyadic(tag + ".w", (C, C, 3, 3), 8, 6),
                aux=X.dyadic(tag + ".aux", (B, H, W, C), 8, 3), scale=X.scales(tag + ".s", (B, C)), shift=X.dyadic(tag + ".h", (B, C), 16, 4))


def dgrad_exact(du, w):
    """The data gradient of y = conv3(x, w) for dy = du: the correlation with the channel-transposed, tap-flipped weights."""
    return X.conv3(du, w.transpose(0, 1).flip(2, 3))


# The plain epilogue of (128, bf16, variant 1, several tiles per workgroup): the training backward launches it at T = 4096, B = 1
# (there resid's partition has no room for the conv's slabs, so the data-gradient conv takes no statistics), and only a plan on the
# real batch reaches it -- ddimx_conv3x3_fwd_ex with DDIMX_PLAN_BATCH, as the (act = 2) row of TRAIN_KEY_ROWS.
BATCH_PLAIN_CASES = [dict(_conv(X.BF16, X.RING, 128, 1, 264, 32, 0, 0, var=1, ragged=False, multi=True), batch=True)]
for _c in BATCH_PLAIN_CASES:
    _c["id"] += "-batch"
    _c["flags"] |= X.P_BATCH
