import contextlib
import os
import sys
import time

if os.path.exists("/dev/kfd"):
    # GPU box: let the HIP runtime name a queue error / fault in the normal run's log (it prints its abort reason only at
    # log level >= 1).  Must be in the environment before libamdhip64 is loaded, i.e. before `import torch`.
    os.environ.setdefault("AMD_LOG_LEVEL", "1")

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

GOLDEN = os.path.join(REPO, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


_PROGRESS = None


def pytest_sessionstart(session):
    """GPU runs keep a crash trail that a later run never overwrites (the log of the one aborted run was lost):
    gpurun_out/crash/<time>_<pid>.txt gets one flushed line per test START, so after an abort from a runtime thread the file
    names the test that was running; faulthandler (pytest enables it: Python stacks of all threads on SIGSEGV / SIGABRT) goes
    to stderr, which tools/gpu_suite.sh redirects into a log with the same unique stem."""
    global _PROGRESS
    if not torch.cuda.is_available():
        return
    d = os.path.join(REPO, "gpurun_out", "crash")
    try:
        os.makedirs(d, exist_ok=True)
        _PROGRESS = open(os.path.join(d, time.strftime("%Y%m%d_%H%M%S") + f"_{os.getpid()}.txt"), "w")
        _PROGRESS.write(f"AMD_LOG_LEVEL={os.environ.get('AMD_LOG_LEVEL')} torch={torch.__version__} argv={sys.argv}\n")
        _PROGRESS.flush()
    except OSError:
        _PROGRESS = None


def pytest_runtest_logstart(nodeid, location):
    if _PROGRESS is not None:
        _PROGRESS.write(f"{time.strftime('%H:%M:%S')} START {nodeid}\n")
        _PROGRESS.flush()
        os.fsync(_PROGRESS.fileno())


def pytest_sessionfinish(session, exitstatus):
    if _PROGRESS is not None:
        _PROGRESS.write(f"{time.strftime('%H:%M:%S')} SESSION FINISHED exit={exitstatus}\n")
        _PROGRESS.close()


def pytest_collection_modifyitems(config, items):
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


@pytest.fixture(scope="session")
def golden():
    def load(name):
        return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return load


HOST_MATH_OPS = ("sqrt", "exp", "log", "sin", "cos")


@contextlib.contextmanager
def host_math(hook):
    """Route torch's float32 CPU sqrt / exp / log / sin / cos (``torch.op(x)`` and ``x.op()``) through ``hook(name, x, y) -> y``.

    The last bits of these ops come from MKL's vector math, whose code path depends on the CPU model; everything else the
    golden comparisons compute (+ - * /, cumprod, clamp, the numpy noise) is exactly rounded and CPU-independent."""
    saved = []
    for name in HOST_MATH_OPS:
        for owner in (torch, torch.Tensor):
            real = getattr(owner, name)

            def wrapped(x, *a, _real=real, _name=name, **k):
                y = _real(x, *a, **k)
                if (not a and not k and isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.device.type == "cpu"
                        and not x.requires_grad):
                    y = hook(_name, x, y)
                return y

            saved.append((owner, name, owner.__dict__.get(name)))
            setattr(owner, name, wrapped)
    try:
        yield
    finally:
        for owner, name, old in reversed(saved):
            if old is None:
                delattr(owner, name)
            else:
                setattr(owner, name, old)


def record_host_math(fn):
    """Run ``fn()`` and return {op: (input bits, output bits)} of every float32 CPU call of the ops above, sorted by input.
    Raises if one input gave two outputs (then a lookup by input would be ambiguous)."""
    seen = {n: {} for n in HOST_MATH_OPS}

    def hook(name, x, y):
        for i, o in zip(x.reshape(-1).view(torch.int32).tolist(), y.reshape(-1).view(torch.int32).tolist()):
            assert seen[name].setdefault(i, o) == o, (name, i)
        return y

    with host_math(hook):
        fn()
    out = {}
    for n, d in seen.items():
        keys = np.array(sorted(d), dtype=np.int32)
        out[n + "_in"], out[n + "_out"] = keys, np.array([d[k] for k in keys.tolist()], dtype=np.int32)
    return out


@pytest.fixture
def pinned_host_math():
    """For the tests that compare host float32 arithmetic with the golden vectors bit for bit: inside the test, the ops above
    return, for every input the golden computations fed them, the bits they gave where the golden vectors were made
    (tests/golden/host_math.npz, written by oracle/make_golden.py with ``record_host_math``).  The order and the exactly
    rounded arithmetic between those calls stay the code's own, so the comparisons remain bit for bit on any CPU."""
    t = np.load(os.path.join(GOLDEN, "host_math.npz"), allow_pickle=False)

    def hook(name, x, y):
        keys, vals = t[name + "_in"], t[name + "_out"]
        if keys.size == 0:
            return y
        xb = x.contiguous().reshape(-1).view(torch.int32).numpy()
        idx = np.minimum(np.searchsorted(keys, xb), keys.size - 1)
        hit = keys[idx] == xb
        if not hit.any():
            return y
        yb = y.contiguous().reshape(-1).view(torch.int32).numpy().copy()
        yb[hit] = vals[idx[hit]]
        return torch.from_numpy(yb).view(torch.float32).reshape(y.shape)

    with host_math(hook):
        yield


def rel_err(a, b):
    """(max-abs, rms) of a-b, both relative to the std of b."""
    a = torch.as_tensor(a, dtype=torch.float64).reshape(-1)
    b = torch.as_tensor(b, dtype=torch.float64).reshape(-1)
    s = float(b.std()) + 1e-30
    d = a - b
    return float(d.abs().max()) / s, float(d.square().mean().sqrt()) / s
