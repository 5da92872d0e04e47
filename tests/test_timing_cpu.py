"""tools/timing.py, the one copy of the timing tools' measuring method, as far as it runs without a device: the order of the legs,
the statistics, the bandwidth arithmetic, every tool's command line, and the refusal to run without a GPU.  Then the table of public
headers in ddim_audio_amd/_lib.py and the source list of ddim_audio_amd/build.py, which register nothing by hand.  CPU only."""
import importlib
import os
import sys
import types

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import timing  # noqa: E402
from ddim_audio_amd import _lib, build  # noqa: E402

TBL = {"T": 1024, "B": [8]}
# tool -> (flags, defaults, the usage line's words for them, one other line, what it parses to)
TOOLS = {
    "brownian": ((), dict(TBL, rounds=6), "[T=1024] [rounds=6] [B ...=8]", "512 3 2 4", dict(T=512, rounds=3, B=[2, 4])),
    "distill": ((), dict(T=1024, rounds=6, B=32, iters=3), "[T=1024] [rounds=6] [B=32] [iters=3]", "64 1 2 1", dict(T=64, rounds=1, B=2, iters=1)),
    "input_grad": ((), dict(T=1024, rounds=5, B=[8, 32]), "[T=1024] [rounds=5] [B ...=8 32]", "64 1 2", dict(T=64, rounds=1, B=[2])),
    "inpaint": ((), dict(T=1024, rounds=5, B=[8, 32]), "[T=1024] [rounds=5] [B ...=8 32]", "64 0", dict(T=64, rounds=0, B=[8, 32])),
    "inpaint_solver": (("unchanged",), dict(TBL, rounds=5, unchanged=False), "[T=1024] [rounds=5] [unchanged] [B ...=8]", "64 2 unchanged 2",
                       dict(T=64, rounds=2, unchanged=True, B=[2])),
    "invert": ((), dict(TBL, rounds=6), "[T=1024] [rounds=6] [B ...=8]", "2048", dict(T=2048, rounds=6, B=[8])),
    "noise": ((), dict(TBL, rounds=6), "[T=1024] [rounds=6] [B ...=8]", "64 1 2", dict(T=64, rounds=1, B=[2])),
    "pool": ((), dict(T=1024, rounds=6, what="abc"), "[T=1024] [rounds=6] [what=abc]", "64 1 what=a", dict(T=64, rounds=1, what="a")),
    "sde": ((), dict(TBL, rounds=6), "[T=1024] [rounds=6] [B ...=8]", "64 1 2 8 32", dict(T=64, rounds=1, B=[2, 8, 32])),
    "solver": ((), dict(TBL, rounds=6), "[T=1024] [rounds=6] [B ...=8]", "T=64 rounds=1 2", dict(T=64, rounds=1, B=[2])),
    "threshold": ((), dict(T=1024, rounds=8, B=8, legs="none,clip,dynamic"), "[T=1024] [rounds=8] [B=8] [legs=none,clip,dynamic]",
                  "64 1 2 legs=none", dict(T=64, rounds=1, B=2, legs="none")),
    "unic": (("unchanged",), dict(TBL, rounds=6, unchanged=False), "[T=1024] [rounds=6] [unchanged] [B ...=8]", "unchanged 64 1 2",
             dict(T=64, rounds=1, unchanged=True, B=[2])),
    "vpred": ((), dict(T=1024, rounds=8, B=8, legs="eps,v"), "[T=1024] [rounds=8] [B=8] [legs=eps,v]", "64 1 2 eps", dict(T=64, rounds=1, B=2, legs="eps")),
    "window": (("long",), dict(rounds=5, long=False, cases=[(1, 8), (4, 8)]), "[rounds=5] [long] [NxW ...=1x8 4x8]", "1x2 long 3",
               dict(rounds=3, long=True, cases=[(1, 2)])),
    "window_inpaint": (("unchanged",), dict(rounds=5, unchanged=False), "[rounds=5] [unchanged]", "1 unchanged", dict(rounds=1, unchanged=True)),
    "window_solver": (("long",), dict(rounds=5, long=False, cases=[(1, 8), (1, 32)]), "[rounds=5] [long] [NxW ...=1x8 1x32]", "2 1x2 2x3 long",
                      dict(rounds=2, long=True, cases=[(1, 2), (2, 3)])),
}


# ---- 1. the order of the legs, the statistics, the arithmetic ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5])
def test_leg_order_alternates_unless_fixed(n):
    names = tuple("abcde"[:n])
    assert [timing.leg_order(names, r) for r in range(4)] == [names, names[::-1], names, names[::-1]]
    assert [timing.leg_order(names, r, fixed=True) for r in range(4)] == [names] * 4
    assert timing.leg_order(dict.fromkeys(names), 1) == names[::-1]  # a mapping of legs, in its order
    assert timing.WARMUP_ROUNDS == 2


def test_summary_and_capture_counts():
    assert timing.summary([3.0, 1.0, 2.0, 10.0, 4.0]) == {"ms_per_step": 3.0, "spread_ms": 9.0}
    assert timing.summary([1.0, 2.0]) == {"ms_per_step": 1.5, "spread_ms": 1.0}
    assert timing.summary([7.0]) == {"ms_per_step": 7.0, "spread_ms": 0.0}
    # readings of stepper.captures after the warm-up rounds and at the end: a is replayed throughout, b captured once more while timed,
    # c never captures (eager)
    assert timing.capture_counts({"a": 2, "b": 1, "c": 0}, {"a": 2, "b": 2, "c": 0}) == {
        "a": {"captures": 2, "captures_while_timed": 0}, "b": {"captures": 2, "captures_while_timed": 1},
        "c": {"captures": 0, "captures_while_timed": 0}}


def test_bandwidth_record_on_two_hand_computed_cases():
    assert timing.HBM_PEAK == 8.0e12
    # 4 passes over 1e9 bytes in 1 ms: 4e9 bytes, 4 TB/s, half the peak
    r = timing.bandwidth_record("k", 1.0, 4, 1000000000, B=8, T=1024)
    assert list(r) == ["what", "B", "T", "ms", "bytes", "TB_per_s", "frac_of_8TBps"]
    assert r == {"what": "k", "B": 8, "T": 1024, "ms": 1.0, "bytes": 4000000000, "TB_per_s": 4.0, "frac_of_8TBps": 0.5}
    # 1 pass over 2^24 bytes in 8 us, printed in us
    r = timing.bandwidth_record("g", 0.008, 1, 1 << 24, unit="us", N=1, W=2)
    assert list(r) == ["what", "N", "W", "us", "bytes", "TB_per_s", "frac_of_8TBps"]
    assert r["us"] == 8.0 and r["bytes"] == 16777216
    assert r["TB_per_s"] == 16777216 / 0.008 / 1e9 and r["frac_of_8TBps"] == 16777216 / 8.0e12 / (0.008 * 1e-3)
    assert r["TB_per_s"] == pytest.approx(2.097152) and r["frac_of_8TBps"] == pytest.approx(0.262144)


# ---- 2. every tool: imports without a device, parses its usage line, refuses to run ------------------------------------------------
_PARSE_ARGS = timing.parse_args


class _Parsed(Exception):
    pass


def _parse(monkeypatch, tool, line):
    """What ``tool``'s main makes of the command line ``line``: main stops right behind its parse_args call."""
    mod = importlib.import_module(tool + "_time")
    seen = []

    def spy(argv, spec, flags=()):
        seen.append(_PARSE_ARGS(argv, spec, flags))
        raise _Parsed
    monkeypatch.setattr(timing, "parse_args", spy)
    with pytest.raises(_Parsed):
        mod.main(line.split())
    return mod, vars(seen[0])


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_tool_command_line(monkeypatch, tool):
    flags, defaults, usage, line, parsed = TOOLS[tool]
    mod, got = _parse(monkeypatch, tool, "")
    assert got == defaults
    assert f"usage: python tools/{tool}_time.py {usage}" in mod.__doc__, "the defaults are the usage line's"
    assert _parse(monkeypatch, tool, line)[1] == parsed
    for flag in flags:  # a word flag may stand anywhere
        words = line.replace(flag, "").split()
        for at in range(len(words) + 1):
            assert _parse(monkeypatch, tool, " ".join(words[:at] + [flag] + words[at:]))[1] == dict(parsed, **{flag: True})
    first = next(iter(defaults))  # T, or rounds for the tools without one: an integer or nothing
    for bad in ("abc", "1.5", "1e3"):
        with pytest.raises(SystemExit, match=first):
            _parse(monkeypatch, tool, bad)


def test_parser_refuses_what_is_left_over():
    with pytest.raises(SystemExit, match="left over"):
        timing.parse_args(["64", "1", "2", "3", "4"], {"T": 1024, "rounds": 6, "B": 32, "iters": 3})
    with pytest.raises(SystemExit, match="B"):
        timing.parse_args(["64", "1", "2", "x"], {"T": 1024, "rounds": 6, "B": [8]})


def test_nothing_runs_without_a_gpu():
    import torch
    assert not torch.cuda.is_available(), "this module is the CPU half; tests/test_gpu_timing_tools.py is the other"
    with pytest.raises(RuntimeError, match="GPU"):
        timing.require_gpu()
    for fn in (timing.audio_model, lambda: timing.time_legs({}, 1), lambda: timing.time_launches(lambda: None, 1, 1),
               lambda: timing.time_graph_replay(lambda: None, 1, 1)):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()
    for tool in TOOLS:  # imported above or here: no device work at import, and main refuses
        mod = importlib.import_module(tool + "_time")
        with pytest.raises(RuntimeError, match="GPU"):
            mod.main([])
    assert not torch.cuda.is_initialized()


# ---- 3. the table of public headers ------------------------------------------------------------------------------------------------
EXPORTS = {
    "DISTILL_EXPORTS": ("ddimxd_sqerr_loss_w", "ddimxd_sqerr_loss_w_bwd_mean", "ddimxd_distill_half", "ddimxd_distill_target"),
    "THRESHOLD_EXPORTS": ("ddimxq_quantile_work_bytes", "ddimxq_x0_quantile", "ddimxq_threshold_eps"),
    "SDE_EXPORTS": ("ddimxs_multistep_update",),
    "BROWNIAN_EXPORTS": ("ddimxb_multistep_update", "ddimxb_path_fill"),
    "WINDOW_EXPORTS": ("ddimxw_multistep_update", "ddimxw_blend"),
    "WINDOW_INPAINT_EXPORTS": ("ddimxwi_partials_floats", "ddimxwi_residual", "ddimxwi_update"),
    "WINDOW_INPAINT_SOLVER_EXPORTS": ("ddimxwis_residual", "ddimxwis_multistep_update"),
    "UNIC_EXPORTS": ("ddimxu_multistep_update",),
    "INPAINT_SOLVER_EXPORTS": ("ddimxi_residual", "ddimxi_multistep_update"),
}
# every integer constant of the binding as it was when each header was registered by hand
CONSTANTS = {
    "DDIMX_ABI_VERSION": 2, "DDIMX_MAX_LEVELS": 8, "DDIMX_F32": 0, "DDIMX_BF16": 1, "DDIMX_BWD_DATA_ONLY": 1, "DDIMX_PACK_COPY": 0,
    "DDIMX_PACK_CONV": 1, "DDIMX_PACK_CONVT": 2, "DDIMX_PACK_BIAS2": 3, "DDIMX_PACK_PERM_COLS": 4, "DDIMX_PACK_PERM_ROWS": 5,
    "DDIMX_PACK_CONV_F32": 6, "DDIMX_LAYOUT_WORKSPACE": 0, "DDIMX_LAYOUT_TRAIN_WORKSPACE": 1, "DDIMX_LAYOUT_TAPE": 2,
    "DDIMX_OP_LAYOUT_RESBLOCK": 0, "DDIMX_OP_LAYOUT_RESBLOCK_BWD": 1, "DDIMX_OP_LAYOUT_DOWNUP_BWD": 2, "DDIMX_PLAN_WFRAG": 1,
    "DDIMX_PLAN_SKIP": 2, "DDIMX_PLAN_STATS": 4, "DDIMX_PLAN_GROUPS": 8, "DDIMX_PLAN_BATCH": 16, "DDIMX_PLAN_BWD": 32,
    "DDIMX_FAMILY_RING": 0, "DDIMX_FAMILY_WREG": 1, "DDIMX_FAMILY_PIPE": 2, "DDIMX_EDGE_CONV_IN": 0, "DDIMX_EDGE_CONV_OUT": 1,
    "DDIMX_EDGE_CONV_OUT_BWD_DATA": 2, "DDIMX_EDGE_CONV_IN_BWD_DATA": 3, "DDIMX_EDGE_WGRAD": 4, "DDIMX_INPAINT_STRIDE": 9,
    "DDIMX_INPAINT_REPLACE": 1, "DDIMX_INPAINT_GUIDED": 2, "DDIMX_SOLVER_STRIDE": 8, "DDIMX_INVERT_STRIDE": 6, "DDIMX_NOISE_NORMALS": 0,
    "DDIMX_NOISE_WORDS": 1, "DDIMX_WINDOW_MAX_COVER": 8, "DDIMX_POOL_STRIDE": 8, "DDIMX_POOL_SLOT_WORDS": 8, "MAX_LEVELS": 8,
    "DDIMX_DISTILL_STRIDE": 12, "DDIMXB_MAX_DEPTH": 16, "DDIMXB_PLAN_STRIDE": 140, "DDIMXB_NOISE_TAG": 2, "DDIMXB_ENTER_ANCHOR": 0,
    "DDIMXB_ENTER_ROOT": 1, "DDIMXB_ENTER_LEFT": 2, "DDIMXB_ENTER_RIGHT": 3, "DDIMXB_PATH": 0, "DDIMXB_INCREMENT": 1, "DDIMXU_STRIDE": 9,
    "DDIMXI_STRIDE": 13, "DDIMXI_REPLACE": 1, "DDIMXI_GUIDED": 2,
}


def test_headers_are_found_not_registered():
    assert list(_lib.HEADERS) == ["ddimx.h", "ddimx_brownian.h", "ddimx_distill.h", "ddimx_inpaint_solver.h", "ddimx_sde.h",
                                  "ddimx_threshold.h", "ddimx_unic.h", "ddimx_window.h", "ddimx_window_inpaint.h",
                                  "ddimx_window_inpaint_solver.h"]
    assert sorted(_lib.HEADERS) == sorted(f for f in os.listdir(_lib._INCLUDE) if f.startswith("ddimx") and f.endswith(".h"))
    below = [os.path.join(d, f) for d, _, fs in os.walk(_lib._INCLUDE) if d != _lib._INCLUDE for f in fs if f.startswith("ddimx") and f.endswith(".h")]
    assert not below, "one kind of header: every ddimx*.h lies directly in include/"
    assert type(_lib.EXPORTS) is tuple and len(_lib.EXPORTS) == 151 and len(set(_lib.EXPORTS)) == 151
    assert _lib.EXPORTS == tuple(_lib.HEADERS["ddimx.h"].funcs)
    assert _lib.EXPORTS[0] == "ddimx_abi_version" and _lib.EXPORTS[-1] == "ddimx_adam_multi_dyn"
    for name, want in EXPORTS.items():
        got = getattr(_lib, name)
        assert type(got) is tuple and got == want, name
        assert got == tuple(_lib.HEADERS["ddimx_" + name[:-len("_EXPORTS")].lower() + ".h"].funcs)
    assert sorted(n for n in vars(_lib) if n.endswith("EXPORTS")) == sorted(["EXPORTS", *EXPORTS])
    assert type(_lib.EXPORTS + _lib.DISTILL_EXPORTS) is tuple  # what the entry point concatenates
    for name, value in CONSTANTS.items():
        assert getattr(_lib, name) == value, name
    for h in _lib.HEADERS.values():
        assert all(getattr(_lib, k) == v for k, v in h.consts.items())
    assert set(_lib.HEADERS["ddimx.h"].structs) == {"ddimx_config", "ddimx_tables"}


def test_a_bad_declaration_names_its_header():
    with pytest.raises(RuntimeError, match=r"^ddimx_new\.h: unknown return type `void`"):
        _lib.parse_header("#define DDIMXN_STRIDE 4\nvoid ddimxn_f(int a);", "ddimx_new.h")
    with pytest.raises(RuntimeError, match=r"^ddimx_new\.h: not an integer constant"):
        _lib.parse_header('#define DDIMXN_NAME "text"', "ddimx_new.h")
    with pytest.raises(RuntimeError, match=r"^ddimx\.h: "):
        _lib.parse_header("int ddimx_f(int a, short b);")


def test_functions_are_bound_on_first_use(monkeypatch):
    """load() touches ddimx_abi_version alone; a function is bound by its first access, once, with its header's types; a name that no
    header declares cannot be called; a function that two headers declare is refused when the table is built."""
    touched = []

    class FakeLib:
        def __getattr__(self, name):
            touched.append(name)
            fn = types.SimpleNamespace()
            if name == "ddimx_abi_version":
                fn = lambda: _lib.DDIMX_ABI_VERSION  # noqa: E731
            setattr(self, name, fn)
            return fn

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: FakeLib())
    monkeypatch.setattr(_lib, "LIB_PATH", __file__)  # a file that exists; the fake CDLL never opens it
    lib = _lib.load()
    assert touched == ["ddimx_abi_version"] and _lib.load() is lib
    fn = lib.ddimx_inpaint_update
    assert touched == ["ddimx_abi_version", "ddimx_inpaint_update"], "that one only"
    assert (fn.restype, fn.argtypes) == _lib.HEADERS["ddimx.h"].funcs["ddimx_inpaint_update"]
    assert lib.ddimx_inpaint_update is fn and lib.ddimx_abi_version() == _lib.DDIMX_ABI_VERSION
    assert len(touched) == 2, "a second access does not reach the library again"
    res, args = _lib.HEADERS["ddimx_unic.h"].funcs["ddimxu_multistep_update"]
    assert lib.ddimxu_multistep_update.restype is res and lib.ddimxu_multistep_update.argtypes == args and len(touched) == 3
    with monkeypatch.context() as mp:  # what the GPU tests do to count launches
        mp.setattr(lib, "ddimx_inpaint_update", "a wrapper")
        assert lib.ddimx_inpaint_update == "a wrapper"
    assert lib.ddimx_inpaint_update is fn and len(touched) == 3
    with pytest.raises(AttributeError, match=r"no include/ddimx\*\.h declares ddimx_nonesuch"):
        lib.ddimx_nonesuch
    assert not hasattr(lib, "ddimx_nonesuch") and not hasattr(lib, "ddimxu_update") and len(touched) == 3
    # the table: {file name: text} -> ({file name: Header}, {function: file name}); a second declaration names both headers
    one, two = "int ddimxn_f(int a);\nint ddimxn_g(void);", "#define DDIMXM_STRIDE 4\nint ddimxm_f(float a);"
    headers, owner = _lib._parse_all({"ddimx_n.h": one, "ddimx_m.h": two})
    assert list(headers) == ["ddimx_n.h", "ddimx_m.h"] and headers["ddimx_m.h"] == _lib.Header(*_lib.parse_header(two, "ddimx_m.h"))
    assert owner == {"ddimxn_f": "ddimx_n.h", "ddimxn_g": "ddimx_n.h", "ddimxm_f": "ddimx_m.h"}
    with pytest.raises(RuntimeError, match=r"^ddimx_m\.h: ddimxn_g is declared in ddimx_n\.h too"):
        _lib._parse_all({"ddimx_n.h": one, "ddimx_m.h": two + "\nint ddimxn_g(void);"})
    assert _lib._OWNER == {n: f for f, h in _lib.HEADERS.items() for n in h.funcs}
    assert len(_lib._OWNER) == sum(len(h.funcs) for h in _lib.HEADERS.values())


# ---- 4. the build's lists ----------------------------------------------------------------------------------------------------------
PARENT_SOURCES = """plan.cpp conv_dispatch.cpp blocks.cpp walk_infer.cpp walk_train.cpp ops.cpp samplers.cpp distill.cpp threshold.cpp sde.cpp
brownian.cpp window_solver.cpp window_inpaint.cpp unic.cpp inpaint_solver.cpp edge_conv.hip gn_kernels.hip fnet_pointwise.hip temb_kernels.hip
step_kernels.hip tail_kernels.hip pack_kernels.hip wgrad_reduce.hip gemm.hip fnet_dense.hip conv_inst_bf16_c3.hip conv_inst_bf16_du.hip
conv_inst_f32_c3.hip conv_inst_f32_du.hip conv_inst_bf16_c3b.hip conv_inst_bf16_wreg.hip conv_inst_bf16_pipe.hip conv_inst_f32_c3b.hip
wgrad_inst_bf16.hip wgrad_inst_f32.hip inpaint_kernels.hip solver_kernels.hip noise_kernels.hip window_kernels.hip invert_kernels.hip
pool_kernels.hip vpred_kernels.hip distill_kernels.hip threshold_kernels.hip sde_kernels.hip brownian_kernels.hip window_solver_kernels.hip
window_inpaint_kernels.hip unic_kernels.hip inpaint_solver_kernels.hip""".split()


def test_build_lists_what_is_there():
    assert len(PARENT_SOURCES) == 50 and set(build.SOURCES) == set(PARENT_SOURCES)
    assert build.SOURCES == sorted(build.SOURCES) and len(build.SOURCES) == 50
    assert set(build.EXTRA_FLAGS) <= set(build.SOURCES)
