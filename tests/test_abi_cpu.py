"""The ctypes binding is derived from include/ddimx.h (ddim_audio_amd/_lib.py::parse_header): the parser on a synthetic header,
its failure cases, and anchors on the real header at the places where a wrong rule would show.  Then the binding rule (_lib.py's
docstring) against a real shared object that has two functions only, and a sweep: every ``.ddimx*_...`` name that the Python
sources use is declared in some header.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_longlong, c_uint, c_ulonglong, c_void_p

import pytest

from ddim_audio_amd import _lib

SYNTHETIC = """
/* A header in the style of ddimx.h.  ddimx_in_a_comment(B, T) is no declaration; neither is
 * int ddimx_commented_out(int a); */
#ifndef DDIMX_H
#define DDIMX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define DDIMX_ABI_VERSION 7   /* object-like */
#define DDIMX_N 3
#define DDIMX_HEX 0x10
#define DDIMX_LONG \\
    12
#define DDIMX_SHIFT(x) ((x) << 8) /* function-like: skipped */
typedef struct {
    int a;              /* int ddimx_field_comment(void); */
    float eps;
    int ch[DDIMX_N];
    int two[2];
    const float* table;
} ddimx_thing;
typedef struct ddimx_ctx* ddimx_handle;

int ddimx_none(void);
const char* ddimx_text(void);
long long ddimx_bytes(ddimx_handle h, int B);
int ddimx_scalars(int a, unsigned b, long long c, unsigned long long d, float e, double f);
int ddimx_pointers(const float* a, void* const* b, const void* const* c, const char** d, ddimx_handle h, ddimx_handle* out,
                   const int64_t* t, double *spaced, unsigned long long* counter);
/* ddimx_three_lines(x, y) is declared below, over three lines */
int ddimx_three_lines(int dtype,
                      const void* x, float scale,
                      void* stream);
int ddimx_Capital_T(int a);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_a_synthetic_header():
    consts, structs, funcs = _lib.parse_header(SYNTHETIC)
    assert consts == {"DDIMX_ABI_VERSION": 7, "DDIMX_N": 3, "DDIMX_HEX": 16, "DDIMX_LONG": 12}
    assert list(structs) == ["ddimx_thing"]
    fields = structs["ddimx_thing"]
    assert [name for name, _ in fields] == ["a", "eps", "ch", "two", "table"]
    assert fields[0][1] is c_int and fields[1][1] is c_float and fields[4][1] is c_void_p
    assert (fields[2][1]._type_, fields[2][1]._length_) == (c_int, 3)
    assert (fields[3][1]._type_, fields[3][1]._length_) == (c_int, 2)
    assert list(funcs) == ["ddimx_none", "ddimx_text", "ddimx_bytes", "ddimx_scalars", "ddimx_pointers", "ddimx_three_lines",
                           "ddimx_Capital_T"]  # header order; nothing out of a comment
    assert funcs["ddimx_none"] == (c_int, [])
    assert funcs["ddimx_text"] == (c_char_p, [])
    assert funcs["ddimx_bytes"] == (c_longlong, [c_void_p, c_int])
    assert funcs["ddimx_scalars"] == (c_int, [c_int, c_uint, c_longlong, c_ulonglong, c_float, c_double])
    assert funcs["ddimx_pointers"] == (c_int, [c_void_p] * 9)
    assert funcs["ddimx_three_lines"] == (c_int, [c_int, c_void_p, c_float, c_void_p])
    assert funcs["ddimx_Capital_T"] == (c_int, [c_int])


@pytest.mark.parametrize("text, offender", [
    ("int ddimx_f(int a, short b);", "short b"),                                  # a scalar the table does not have
    ("int ddimx_f(int a, unsigned int b);", "unsigned int b"),                    # no second spelling either
    ("int ddimx_f(int);", "`int`"),                                               # no parameter name
    ("int ddimx_f(int a[4]);", "ddimx_f"),
    ("void ddimx_f(int a);", "ddimx_f"),                                          # unknown return types
    ("float ddimx_f(int a);", "ddimx_f"),
    ("unsigned long long ddimx_f(void);", "ddimx_f"),
    ("typedef struct { int a; int (*fn)(int); } ddimx_s;", "int (*fn)(int)"),     # struct fields it cannot place
    ("typedef struct { int a; short b; } ddimx_s;", "short b"),
    ("typedef struct { int a[DDIMX_UNKNOWN]; } ddimx_s;", "a[DDIMX_UNKNOWN]"),
    ("typedef struct { int a[2][3]; } ddimx_s;", "a[2][3]"),
    ("int ddimx_f(ddimx_handle h);", "ddimx_handle h"),                           # a handle nobody declared
    ("int ddimx_f(int a)\nint ddimx_g(int b);", "ddimx_g"),                       # a lost semicolon
    ("struct ddimx_s { int a; };", "ddimx_s"),                                    # a statement of another kind
    ("#define DDIMX_NAME \"text\"", "DDIMX_NAME"),                                # an object-like macro that is no integer
])
def test_parser_names_what_it_cannot_read(text, offender):
    with pytest.raises(RuntimeError) as err:
        _lib.parse_header(text)
    assert offender in str(err.value), str(err.value)


def test_real_header_anchors():
    """Positions chosen where a wrong rule would show: double against float, unsigned against int, 64-bit scalars, the two
    non-int return types, array fields and the float in ddimx_config."""
    lib = _lib.load()
    args = lambda name: getattr(lib, name).argtypes  # noqa: E731
    assert args("ddimx_gn_finalize")[4] is c_double and args("ddimx_gn_finalize")[7] is c_float
    assert args("ddimx_unet_fwd_forked")[-1] is c_uint
    assert args("ddimx_noise_fill")[3] is c_ulonglong and args("ddimx_noise_fill")[4] is c_uint
    adam = list(args("ddimx_adam_multi"))
    assert adam[9:14] == [c_float] * 5 and c_float not in adam[:9] + adam[14:]
    assert list(args("ddimx_gemm_nt")[12:15]) == [c_longlong] * 3 and c_longlong not in args("ddimx_gemm_nt")[:12]
    assert lib.ddimx_last_error.restype is c_char_p
    assert lib.ddimx_workspace_bytes.restype is c_longlong
    assert len(_lib.EXPORTS) == 151 and len(set(_lib.EXPORTS)) == 151
    assert _lib.EXPORTS[0] == "ddimx_abi_version" and _lib.EXPORTS[-1] == "ddimx_adam_multi_dyn"  # header order
    assert all(getattr(lib, name).restype in (c_int, c_longlong, c_char_p) for name in _lib.EXPORTS)
    assert ctypes.sizeof(_lib.DdimxConfig) == 136 and ctypes.sizeof(_lib.DdimxTables) == 32
    assert _lib.DdimxConfig.ch.offset == 12 and _lib.DdimxConfig.fnet_ln_eps.offset == 124
    assert _lib.DDIMX_INPAINT_STRIDE == 9 and _lib.DDIMX_PLAN_BWD == 32
    assert _lib.MAX_LEVELS == _lib.DDIMX_MAX_LEVELS == 8 and _lib.DDIMX_ABI_VERSION == lib.ddimx_abi_version()
    assert not hasattr(_lib, "DDIMX_PLAN_XF") and not hasattr(_lib, "DDIMX_H")  # function-like macro, include guard
    tab = _lib.DdimxTables()
    assert (tab.posenc, tab.dft_hidden, tab.dft_seq, tab.temb_table) == (None,) * 4


# ---- the binding rule against a real loader ------------------------------------------------------------------------------------------
TWO_FUNCTIONS = """
int ddimx_abi_version(void) { return %d; }
const char* ddimx_last_error(void) { return "none"; }
"""


def test_a_library_with_two_functions_loads_and_names_what_it_lacks(tmp_path, monkeypatch):
    """A libddimx.so from before every header but the first (and before most of that one): it loads, runs what it has, names the
    header of what it lacks, and has no attribute that no header declares."""
    from ddim_audio_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # build.py's compiler, or the system's
    cc = hipcc if os.path.exists(hipcc) else shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler (hipcc or cc)")
    src, so = tmp_path / "two.c", tmp_path / "libtwo.so"
    src.write_text(TWO_FUNCTIONS % _lib.DDIMX_ABI_VERSION)
    subprocess.run([cc, "-shared", "-fPIC", "-x", "c", str(src), "-o", str(so)], check=True, capture_output=True, text=True)
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    monkeypatch.setattr(_lib, "_lib", None)
    lib = _lib.load()
    assert _lib.load() is lib and os.path.basename(build.OUT) == "libddimx.so"
    assert lib.ddimx_abi_version() == _lib.DDIMX_ABI_VERSION and lib.ddimx_last_error() == b"none"
    with pytest.raises(RuntimeError) as err:
        lib.ddimxu_multistep_update
    msg = str(err.value)
    assert msg.startswith("ddimx_unic.h: ") and str(so) in msg and "has no ddimxu_multistep_update" in msg
    assert "built before this header existed" in msg and "rebuild (`python -m ddim_audio_amd.build`)" in msg
    with pytest.raises(RuntimeError, match=r"^ddimx\.h: .* has no ddimx_unet_fwd: "):
        lib.ddimx_unet_fwd
    with pytest.raises(AttributeError, match=r"no include/ddimx\*\.h declares ddimx_nonesuch"):
        lib.ddimx_nonesuch
    assert not hasattr(lib, "ddimx_nonesuch")


# names that stand behind a dot on purpose although no header declares them: {name: why}
UNDECLARED_ON_PURPOSE = {
    "ddimx_nonesuch": "the tests of the binding rule ask for it to see the AttributeError",
}


def test_every_name_called_on_the_library_is_declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = [os.path.join(root, "bench.py")]
    for sub in ("ddim_audio_amd", "tools", "tests"):
        files += [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(root, sub)) for f in fs if f.endswith(".py")]
    used = {}
    for path in files:
        with open(path) as f:
            for name in re.findall(r"\.(ddimx[a-z]*_\w+)\b", f.read()):
                used.setdefault(name, os.path.relpath(path, root))
    assert len(files) > 100 and len(used) > 100, "the sweep found its files"
    declared = {n for h in _lib.HEADERS.values() for n in h.funcs}
    stray = {n: where for n, where in used.items() if n not in declared and n not in UNDECLARED_ON_PURPOSE}
    assert not stray, stray
    assert set(UNDECLARED_ON_PURPOSE) <= set(used) and not set(UNDECLARED_ON_PURPOSE) & declared, "the list holds nothing stale"
