"""ctypes binding of libddimx.so, derived from the C ABI's one description, include/ddimx.h: signatures, constants and struct
layouts are parsed from the header.  include/ddimx_distill.h, the second public header (loss weighting, distillation), is parsed
the same way; its functions are bound by ``load()`` too and listed in ``DISTILL_EXPORTS``, ``EXPORTS`` stays ddimx.h's.
include/ddimx_threshold.h, the third (x0 clipping and thresholding in the samplers), likewise: ``THRESHOLD_EXPORTS``; and
include/ddimx_sde.h, the fourth (the stochastic multistep update): ``SDE_EXPORTS``; and include/ddimx_brownian.h, the fifth (that
update on one Brownian path, with the constants of its plan row): ``BROWNIAN_EXPORTS``; and include/ddimx_window.h, the sixth (the
windowed multistep solver's fused update and blend): ``WINDOW_EXPORTS``; and include/ddimx_window_inpaint.h, the seventh (the windowed
inpainting step's residual and update): ``WINDOW_INPAINT_EXPORTS``; and include/ddimx_unic.h, the eighth (the multistep update with
the folded UniC corrector, with the stride of its table): ``UNIC_EXPORTS``; and include/ddimx_inpaint_solver.h, the ninth (the multistep
inpainting step's residual and update, with the stride of its table and its flags): ``INPAINT_SOLVER_EXPORTS``.  No fallback: if the library
is missing or a call fails, a RuntimeError is raised (the reference's ``main.py:212-223`` logs exceptions)."""
import ctypes
import os
import re
from ctypes import Structure, c_char_p, c_double, c_float, c_int, c_longlong, c_uint, c_ulonglong, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DDIMX_LIB", os.path.join(_HERE, "libddimx.so"))
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "ddimx.h")
_DISTILL_HEADER = os.path.join(os.path.dirname(_HERE), "include", "ddimx_distill.h")
_THRESHOLD_HEADER = os.path.join(os.path.dirname(_HERE), "include", "ddimx_threshold.h")
_SDE_HEADER = os.path.join(os.path.dirname(_HERE), "include", "ddimx_sde.h")
_BROWNIAN_HEADER = os.path.join(os.path.dirname(_HERE), "include", "ddimx_brownian.h")
_WINDOW_HEADER = os.path.join(os.path.dirname(_HERE), "include", "ddimx_window.h")
_WINDOW_INPAINT_HEADER = os.path.join(os.path.dirname(_HERE), "include", "ddimx_window_inpaint.h")
_UNIC_HEADER = os.path.join(os.path.dirname(_HERE), "include", "ddimx_unic.h")
_INPAINT_SOLVER_HEADER = os.path.join(os.path.dirname(_HERE), "include", "ddimx_inpaint_solver.h")

_SCALARS = {"int": c_int, "unsigned": c_uint, "long long": c_longlong, "unsigned long long": c_ulonglong, "float": c_float,
            "double": c_double}
_RETURNS = {"int": c_int, "long long": c_longlong, "const char*": c_char_p}


def parse_header(text):
    """(constants {name: int}, structs {name: _fields_ list}, functions {name: (restype, argtypes)}) of a header written like
    include/ddimx.h, in its order.  Every pointer and every handle is c_void_p, scalars map by _SCALARS / _RETURNS alone; whatever
    does not fit raises RuntimeError naming the declaration."""
    def bad(what, decl):
        return RuntimeError(f"ddimx.h: {what}: `{decl}`")

    def split(decl):  # "const float* x" / "int ch[DDIMX_MAX_LEVELS]" -> (ctypes class, name, array length or None)
        m = re.fullmatch(r"(.*?)\b(\w+)(?:\[(\w+)\])?", decl)
        if not m or not m.group(1):
            raise bad("cannot parse", decl)
        ctype, dim = m.group(1).strip(), m.group(3)
        if dim is not None:
            if dim not in consts and not dim.isdigit():
                raise bad("unknown array length", decl)
            dim = consts[dim] if dim in consts else int(dim)
        if "*" not in ctype and ctype not in handles and ctype not in _SCALARS:
            raise bad(f"unknown type `{ctype}`", decl)
        return _SCALARS.get(ctype, c_void_p), m.group(2), dim

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S).replace("\\\n", " ")
    consts, structs, funcs, handles = {}, {}, {}, set()
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):  # not NAME(..): function-like
        try:
            consts[name] = int(value, 0)
        except ValueError:
            raise bad("not an integer constant", f"#define {name} {value}") from None
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{|^\s*\}\s*$', "", text, flags=re.M)
    text = re.sub(r"\{[^}]*\}", lambda m: m.group().replace(";", "|"), text)  # a struct's fields end in `|`: one statement
    for stmt in text.split(";"):
        stmt = re.sub(r" ?([*\[\]]) ?", r"\1", " ".join(stmt.split()))
        if m := re.fullmatch(r"typedef struct ?\{(.*)\} ?(\w+)", stmt):
            fields = [split(f.strip()) for f in m.group(1).split("|") if f.strip()]
            structs[m.group(2)] = [(name, ctype if dim is None else ctype * dim) for ctype, name, dim in fields]
        elif m := re.fullmatch(r"typedef struct \w+\*(\w+)", stmt):
            handles.add(m.group(1))
        elif m := re.fullmatch(r"(.*?)\b(\w+) ?\((.*)\)", stmt):
            res, params = m.group(1).strip(), [p.strip() for p in m.group(3).split(",")]
            if res not in _RETURNS:
                raise bad(f"unknown return type `{res}`", stmt)
            args = [] if params == ["void"] else [split(p) for p in params]
            if any(dim is not None for _, _, dim in args):
                raise bad("array parameter", stmt)
            funcs[m.group(2)] = (_RETURNS[res], [ctype for ctype, _, _ in args])
        elif stmt:
            raise bad("cannot parse", stmt)
    return consts, structs, funcs


with open(_HEADER) as _f:
    _CONSTS, _STRUCTS, _FUNCS = parse_header(_f.read())
globals().update(_CONSTS)  # DDIMX_F32, DDIMX_BF16, DDIMX_ABI_VERSION, DDIMX_PLAN_*, ...: every object-like #define of the header
MAX_LEVELS = _CONSTS["DDIMX_MAX_LEVELS"]
EXPORTS = tuple(_FUNCS)
with open(_DISTILL_HEADER) as _f:
    _DISTILL_CONSTS, _, _DISTILL_FUNCS = parse_header(_f.read())
globals().update(_DISTILL_CONSTS)  # DDIMX_DISTILL_STRIDE
DISTILL_EXPORTS = tuple(_DISTILL_FUNCS)
with open(_THRESHOLD_HEADER) as _f:
    _, _, _THRESHOLD_FUNCS = parse_header(_f.read())
THRESHOLD_EXPORTS = tuple(_THRESHOLD_FUNCS)
with open(_SDE_HEADER) as _f:
    _, _, _SDE_FUNCS = parse_header(_f.read())
SDE_EXPORTS = tuple(_SDE_FUNCS)
with open(_BROWNIAN_HEADER) as _f:
    _BROWNIAN_CONSTS, _, _BROWNIAN_FUNCS = parse_header(_f.read())
globals().update(_BROWNIAN_CONSTS)  # DDIMXB_PLAN_STRIDE, DDIMXB_MAX_DEPTH, DDIMXB_ENTER_*, DDIMXB_PATH, DDIMXB_INCREMENT
BROWNIAN_EXPORTS = tuple(_BROWNIAN_FUNCS)
with open(_WINDOW_HEADER) as _f:
    _, _, _WINDOW_FUNCS = parse_header(_f.read())
WINDOW_EXPORTS = tuple(_WINDOW_FUNCS)
with open(_WINDOW_INPAINT_HEADER) as _f:
    _, _, _WINDOW_INPAINT_FUNCS = parse_header(_f.read())
WINDOW_INPAINT_EXPORTS = tuple(_WINDOW_INPAINT_FUNCS)
with open(_UNIC_HEADER) as _f:
    _UNIC_CONSTS, _, _UNIC_FUNCS = parse_header(_f.read())
globals().update(_UNIC_CONSTS)  # DDIMXU_STRIDE
UNIC_EXPORTS = tuple(_UNIC_FUNCS)
with open(_INPAINT_SOLVER_HEADER) as _f:
    _INPAINT_SOLVER_CONSTS, _, _INPAINT_SOLVER_FUNCS = parse_header(_f.read())
globals().update(_INPAINT_SOLVER_CONSTS)  # DDIMXI_STRIDE, DDIMXI_REPLACE, DDIMXI_GUIDED
INPAINT_SOLVER_EXPORTS = tuple(_INPAINT_SOLVER_FUNCS)


class DdimxConfig(Structure):
    _fields_ = _STRUCTS["ddimx_config"]


class DdimxTables(Structure):
    _fields_ = _STRUCTS["ddimx_tables"]

    def __init__(self, posenc=None, dft_hidden=None, dft_seq=None, temb_table=None):
        super().__init__(posenc, dft_hidden, dft_seq, temb_table)


_lib = None


def load():
    """Load libddimx.so once; raise loudly if it is missing (there is no CPU or eager fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -m ddim_audio_amd.build` "
                "(hipcc, gfx950). The HIP library is the only compute path of ddim_audio_amd.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(_FUNCS.items()) + list(_DISTILL_FUNCS.items()) + list(_THRESHOLD_FUNCS.items()) + list(_SDE_FUNCS.items())
                                  + list(_BROWNIAN_FUNCS.items()) + list(_WINDOW_FUNCS.items()) + list(_WINDOW_INPAINT_FUNCS.items())
                                  + list(_UNIC_FUNCS.items()) + list(_INPAINT_SOLVER_FUNCS.items())):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.ddimx_abi_version() != _CONSTS["DDIMX_ABI_VERSION"]:
            raise RuntimeError("libddimx ABI version mismatch")
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError("libddimx: " + load().ddimx_last_error().decode(errors="replace"))


def ptr(t):
    """Device pointer of a tensor (or None)."""
    return None if t is None else c_void_p(t.data_ptr())


def stream():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)
