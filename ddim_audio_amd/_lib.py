"""ctypes binding of libddimx.so, derived from the C ABI's one description, the public headers: signatures, constants and struct
layouts are parsed from them.  Every ``include/ddimx*.h`` is a public header: include/ddimx.h first, the rest in sorted order, each
parsed by the same rule into ``HEADERS[file name]`` (``.consts``, ``.structs``, ``.funcs``).  Every object-like ``#define`` becomes
a name of this module, and each header's function names, in its order, are a tuple named after the file: ``EXPORTS`` is ddimx.h's,
``X_EXPORTS`` is ddimx_x.h's.  A new header registers nowhere; a function that two headers declare is refused at import.

The binding rule: ``load()`` opens the library and checks its ABI version, nothing else.  A function is bound on the first access
to its name on the loaded library: the header that declares it gives ``restype`` and ``argtypes``, and the function becomes an
attribute of the library object, so a later access costs an attribute lookup.  A name that no header declares is an
AttributeError -- there is no untyped call -- and a declared name that the .so lacks is a RuntimeError naming its header, so a
library built before a header existed loads and runs everything it has.

Feature headers.  Every other ``include/*.h`` -- a name that does not start with ``ddimx``, such as ``cmx_consistency.h`` -- is
parsed by the same ``parse_header`` into ``FEATURE_HEADERS[file name]``, in sorted order.  Its constants become names of this
module and its functions are bound by the same rule on first use (``_OWNER`` is consulted first, then the feature table); it gets
no ``*_EXPORTS`` tuple, and ``HEADERS`` and ``_OWNER`` do not know it.  A function declared in both tables, or by two feature
headers, is refused at import.  Why a second table: the contents of the public one -- the list of ``ddimx*.h``, every header's
function tuple, the set of ``*_EXPORTS`` names -- are held by tests as they were when those tests were written, so a feature
adds its header here; folding it into ``HEADERS`` is a later change that edits those tests with it.

The feature directory.  ``FEATURE_HEADERS`` itself is pinned by a test too (it is exactly ``cmx_consistency.h``), so from now on a
feature header goes into ``include/features/``: every ``include/features/*.h`` -- ``lkx_likelihood.h`` is the first -- is parsed by
the same ``parse_header`` into a third table, ``FEATURES[file name]``, in sorted order.  The rule is the second table's: constants
become names of this module, functions are bound on first use (after ``_OWNER`` and the feature table), there is no ``*_EXPORTS``
tuple, and a function that another header of any table declares is refused at import.  Folding the three tables into one is a
later change that edits the tests that pin the first two.

Feature directories: the last rule.  ``FEATURES`` is pinned as well (it is exactly ``lkx_likelihood.h``), so a feature header now
gets a sub-directory of its own: every ``include/features/*/*.h`` -- ``restore_pool/rpx_restore_pool.h`` is the first -- is parsed
by the same ``parse_header`` into a fourth table, ``FEATURE_DIRS["<dir>/<file>"]``, in sorted order.  The rule is the third
table's: constants become names of this module, functions are bound on first use (after the other three tables), there is no
``*_EXPORTS`` tuple, and a function that another header of any table declares is refused at import.  This table is never pinned:
a test asserts that its header is a MEMBER of ``FEATURE_DIRS`` (and of no other table), never what the whole table holds, so the
next feature adds a directory and no fifth table.  No fallback:
if the library is missing or a call fails, a RuntimeError is raised (the reference's ``main.py:212-223`` logs exceptions)."""
import collections
import ctypes
import glob
import os
import re
import threading
from ctypes import Structure, c_char_p, c_double, c_float, c_int, c_longlong, c_uint, c_ulonglong, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DDIMX_LIB", os.path.join(_HERE, "libddimx.so"))
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

_SCALARS = {"int": c_int, "unsigned": c_uint, "long long": c_longlong, "unsigned long long": c_ulonglong, "float": c_float,
            "double": c_double}
_RETURNS = {"int": c_int, "long long": c_longlong, "const char*": c_char_p}


def parse_header(text, header="ddimx.h"):
    """(constants {name: int}, structs {name: _fields_ list}, functions {name: (restype, argtypes)}) of a header written like
    include/ddimx.h, in its order.  Every pointer and every handle is c_void_p, scalars map by _SCALARS / _RETURNS alone; whatever
    does not fit raises RuntimeError naming the header and the declaration."""
    def bad(what, decl):
        return RuntimeError(f"{header}: {what}: `{decl}`")

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


Header = collections.namedtuple("Header", "consts structs funcs")


def _parse_all(texts):
    """``({file name: Header}, {function name: file name})`` of ``{file name: header text}``, in its order; a function that two
    headers declare raises RuntimeError naming both."""
    headers, owner = {}, {}
    for name, text in texts.items():
        headers[name] = Header(*parse_header(text, name))
        for fn in headers[name].funcs:
            if fn in owner:
                raise RuntimeError(f"{name}: {fn} is declared in {owner[fn]} too")
            owner[fn] = name
    return headers, owner


_texts = {}
for _path in sorted(glob.glob(os.path.join(_INCLUDE, "ddimx*.h")), key=lambda p: (os.path.basename(p) != "ddimx.h", p)):
    with open(_path) as _f:
        _texts[os.path.basename(_path)] = _f.read()
HEADERS, _OWNER = _parse_all(_texts)  # {file name: Header}, ddimx.h first; {function name: the file name that declares it}
for _name, _header in HEADERS.items():
    globals().update(_header.consts)  # DDIMX_F32, DDIMX_ABI_VERSION, DDIMXB_PLAN_STRIDE, ...: every object-like #define
    # ddimx.h: EXPORTS; ddimx_two_words.h: TWO_WORDS_EXPORTS
    globals()[(_name[len("ddimx_"):-len(".h")].upper() + "_EXPORTS").lstrip("_")] = tuple(_header.funcs)
_texts = {}
for _path in sorted(p for p in glob.glob(os.path.join(_INCLUDE, "*.h")) if not os.path.basename(p).startswith("ddimx")):
    with open(_path) as _f:
        _texts[os.path.basename(_path)] = _f.read()
FEATURE_HEADERS, _FEATURE_OWNER = _parse_all(_texts)  # the feature headers (the docstring has the rule) and their functions' owners
for _name, _header in FEATURE_HEADERS.items():
    globals().update(_header.consts)  # CMX_STRIDE, ...
    for _fn in _header.funcs:
        if _fn in _OWNER:
            raise RuntimeError(f"{_name}: {_fn} is declared in {_OWNER[_fn]} too")
_texts = {}
for _path in sorted(glob.glob(os.path.join(_INCLUDE, "features", "*.h"))):
    with open(_path) as _f:
        _texts[os.path.basename(_path)] = _f.read()
FEATURES, _FEATURES_OWNER = _parse_all(_texts)  # include/features/*.h (the docstring has the rule) and their functions' owners
for _name, _header in FEATURES.items():
    globals().update(_header.consts)  # LKX_STRIDE, ...
    for _fn in _header.funcs:
        for _other in (_OWNER, _FEATURE_OWNER):
            if _fn in _other:
                raise RuntimeError(f"features/{_name}: {_fn} is declared in {_other[_fn]} too")
_texts = {}
for _path in sorted(glob.glob(os.path.join(_INCLUDE, "features", "*", "*.h"))):
    with open(_path) as _f:
        _texts["/".join(_path.split(os.sep)[-2:])] = _f.read()
FEATURE_DIRS, _FEATURE_DIRS_OWNER = _parse_all(_texts)  # include/features/*/*.h (the docstring has the rule) and their functions' owners
for _name, _header in FEATURE_DIRS.items():
    globals().update(_header.consts)  # RPX_KNOWN_STRIDE, ...
    for _fn in _header.funcs:
        for _other in (_OWNER, _FEATURE_OWNER, _FEATURES_OWNER):
            if _fn in _other:
                raise RuntimeError(f"features/{_name}: {_fn} is declared in {_other[_fn]} too")
_CONSTS, _STRUCTS, _ = HEADERS["ddimx.h"]
MAX_LEVELS = _CONSTS["DDIMX_MAX_LEVELS"]


class DdimxConfig(Structure):
    _fields_ = _STRUCTS["ddimx_config"]


class DdimxTables(Structure):
    _fields_ = _STRUCTS["ddimx_tables"]

    def __init__(self, posenc=None, dft_hidden=None, dft_seq=None, temb_table=None):
        super().__init__(posenc, dft_hidden, dft_seq, temb_table)


class _Library:
    """libddimx.so behind the headers (the module's docstring has the rule).  ``__getattr__`` runs once per name."""

    def __init__(self, path):
        self._path, self._cdll, self._lock = path, ctypes.CDLL(path), threading.Lock()

    def __getattr__(self, name):
        header, table = _OWNER.get(name), HEADERS
        if header is None:
            header, table = _FEATURE_OWNER.get(name), FEATURE_HEADERS
        if header is None:
            header, table = _FEATURES_OWNER.get(name), FEATURES
        if header is None:
            header, table = _FEATURE_DIRS_OWNER.get(name), FEATURE_DIRS
        if header is None:
            raise AttributeError(f"no include/ddimx*.h declares {name}")
        with self._lock:  # steppers run on several threads: nobody is handed a function whose types are still being set
            if name not in vars(self):
                try:
                    fn = getattr(self._cdll, name)
                except AttributeError:
                    raise RuntimeError(f"{header}: {self._path} has no {name}: built before this header existed: rebuild "
                                       "(`python -m ddim_audio_amd.build`)") from None
                fn.restype, fn.argtypes = table[header].funcs[name]
                setattr(self, name, fn)
            return vars(self)[name]


_lib = None


def load():
    """Load libddimx.so once; raise loudly if it is missing (there is no CPU or eager fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -m ddim_audio_amd.build` "
                "(hipcc, gfx950). The HIP library is the only compute path of ddim_audio_amd.")
        lib = _Library(LIB_PATH)
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
