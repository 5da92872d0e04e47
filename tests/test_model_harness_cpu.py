"""tests/model_harness.py on the CPU: every builder of the feature GPU tests keeps the config it had (the expected edits are written
out here), the whole-network gate accepts and rejects on either side of its thresholds, the eager-steps switch restores what it
found, the sentinel holds its pattern, and no test module imports another."""
import copy
import glob
import os
import re

import pytest
import torch

from ddim_audio_amd import configs
import gpu_util as G
import model_harness as H

F32S, BF16S = "torch.cuda.FloatTensor", "torch.cuda.BFloat16Tensor"
DROPOUT = ("model", "transformers", "kwargs", "hidden_dropout_prob")
OPTIMIZER = ("optimization", "optimizer", "default", "optimizer")
KIND = ("model", "type")
WEIGHT = ("model", "loss_weight")

# (the builder it replaces, config_dict's keyword arguments, {path: value} of the edits it must make -- and no other)
ROWS = [
    ("_model of solver / noise / invert / window", {}, {}),
    ("test_gpu_inpaint._model", dict(dropout=0.1), {DROPOUT: 0.1}),
    ("test_gpu_input_grad._model, default", dict(dropout=0.0), {DROPOUT: 0.0}),
    ("test_gpu_input_grad._model, dropout", dict(dropout=0.1), {DROPOUT: 0.1}),
    ("test_gpu_train._train_model", dict(dropout=0.0, optimizer="Adam"), {DROPOUT: 0.0, OPTIMIZER: "Adam"}),
    ("test_gpu_train._train_model, dropout", dict(dropout=0.1, optimizer="Adam"), {DROPOUT: 0.1, OPTIMIZER: "Adam"}),
    ("_train_model of configs / zz_rccl", dict(dropout=0.0, optimizer="AdamW"), {DROPOUT: 0.0, OPTIMIZER: "AdamW"}),
    ("_train_model of configs, fp32 FNet", dict(dropout=0.0, optimizer="AdamW", fnet=F32S), {DROPOUT: 0.0, OPTIMIZER: "AdamW"}),
    ("_eval_model / make_model", {}, {}),
    ("make_model, fp32 FNet", dict(fnet=F32S), {}),
    ("make_model, bf16 FNet", dict(fnet=BF16S), {}),
    ("test_gpu_vpred._dict, v", dict(kind="v"), {KIND: "v"}),
    ("test_gpu_vpred._dict, simple", dict(kind="simple"), {KIND: "simple"}),
    ("test_gpu_vpred._dict, v, dropout", dict(kind="v", dropout=0.0), {KIND: "v", DROPOUT: 0.0}),
    ("test_gpu_vpred._dict, v, AdamW", dict(kind="v", optimizer="AdamW"), {KIND: "v", OPTIMIZER: "AdamW"}),
    ("test_gpu_vpred._v_train_model", dict(kind="v", dropout=0.0, optimizer="Adam"), {KIND: "v", DROPOUT: 0.0, OPTIMIZER: "Adam"}),
    ("test_gpu_distill._weighted_v_model", dict(kind="v", dropout=0.0, optimizer="Adam", loss_weight="min_snr"),
     {KIND: "v", DROPOUT: 0.0, OPTIMIZER: "Adam", WEIGHT: "min_snr"}),
    ("test_gpu_distill, AdamW with a weight", dict(kind="v", optimizer="AdamW", loss_weight="min_snr"),
     {KIND: "v", OPTIMIZER: "AdamW", WEIGHT: "min_snr"}),
    ("test_gpu_distill, the uniform weight", dict(kind="v", dropout=0.0, loss_weight="uniform"),
     {KIND: "v", DROPOUT: 0.0, WEIGHT: "uniform"}),
]


def _edited(d, edits):
    d = copy.deepcopy(d)
    for path, value in edits.items():
        at = d
        for key in path[:-1]:
            at = at[key]
        at[path[-1]] = value
    return d


@pytest.mark.parametrize("dtype_str", [F32S, BF16S], ids=H.MODE_IDS)
@pytest.mark.parametrize("name", ["tiny", "audio"])
@pytest.mark.parametrize("what,kw,edits", ROWS, ids=[r[0] for r in ROWS])
def test_config_dict_makes_the_listed_edits_and_no_other(what, kw, edits, name, dtype_str):
    base = (configs.tiny_dict if name == "tiny" else configs.audio_dict)(dtype_str, kw.get("fnet"))
    assert "loss_weight" not in base["model"] and base["model"]["type"] == "simple"
    assert H.config_dict(name, dtype_str, **kw) == _edited(base, edits)
    assert all(k in ("kind", "dropout", "optimizer", "loss_weight", "fnet") for k in kw)


def test_config_dict_fnet_is_the_second_argument_of_configs():
    assert H.config_dict("audio", BF16S, fnet=F32S) == configs.audio_dict(BF16S, F32S) != configs.audio_dict(BF16S)
    assert H.config_dict("tiny", BF16S) == configs.tiny_dict(BF16S) != configs.audio_dict(BF16S)


def test_constants():
    assert H.MODES == [(F32S, G.F32), (BF16S, G.BF16)] and H.MODE_IDS == ["f32", "bf16"]
    assert H.U == 2.0 ** -24 and H.TINY == 2.0 ** -126 and H.PATTERN == 0x7FC0BEEF
    a = H.alphas()
    assert a.shape == (1000,) and a.dtype == torch.float32 and torch.equal(a, H.alphas(configs.tiny_config()))


def test_backward_case_defaults_to_the_tiny_network_and_the_oracles_own_forward():
    """The callers from before the ``forward`` / ``name`` arguments pass neither: the defaults are what they had."""
    import inspect
    sig = inspect.signature(H.backward_case)
    assert list(sig.parameters) == ["mode", "shape", "tt", "build_model", "loss", "ref_loss", "forward", "name"]
    assert sig.parameters["forward"].default is None and sig.parameters["name"].default == "tiny"
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("build_model", "loss", "ref_loss", "forward", "name"))


# ---- gate: a reference of RMS exactly 2 (every element +-2), errors placed by hand ----------------------------------------------------
N = 4096
REF = torch.full((N,), 2.0, dtype=torch.float64) * torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(N // 2)
RMS = 2.0


def _got(max_rel, rms_rel=None):
    """REF with one element off by ``max_rel`` x RMS and, if asked, the others off by a constant such that the RMS error is
    ``rms_rel`` x RMS."""
    d = torch.zeros(N, dtype=torch.float64)
    d[7] = max_rel * RMS
    if rms_rel is not None:
        rest = ((rms_rel * RMS) ** 2 * N - float(d[7]) ** 2) / (N - 1)
        assert 0 <= rest <= (max_rel * RMS) ** 2
        d[torch.arange(N) != 7] = rest ** 0.5
    return REF + d


def test_gate_fp32_threshold():
    mx, er = H.gate(_got(1.9e-3), REF, G.F32, "inside")
    assert abs(mx - 1.9e-3) < 1e-9 and er < mx
    with pytest.raises(AssertionError, match="outside: max 2.100e-03 x rms"):
        H.gate(_got(2.1e-3), REF, G.F32, "outside")


def test_gate_bf16_thresholds():
    mx, er = H.gate(_got(0.59, 4.9e-2), REF, G.BF16, "inside")
    assert abs(mx - 0.59) < 1e-9 and abs(er - 4.9e-2) < 1e-9
    with pytest.raises(AssertionError, match="max 6.100e-01"):
        H.gate(_got(0.61, 4.9e-2), REF, G.BF16, "max outside")
    with pytest.raises(AssertionError, match="rms err 5.100e-02"):
        H.gate(_got(0.59, 5.1e-2), REF, G.BF16, "rms outside")
    H.gate(_got(2.1e-3), REF, G.BF16, "what fp32 rejects")


@pytest.mark.parametrize("dt", [G.F32, G.BF16], ids=H.MODE_IDS)
def test_gate_rejects_a_nan(dt):
    got = REF.clone()
    H.gate(got, REF, dt, "exact")
    got[11] = float("nan")
    with pytest.raises(AssertionError, match="a NaN"):
        H.gate(got, REF, dt, "a NaN")
    got[11] = float("inf")
    with pytest.raises(AssertionError, match="an inf"):
        H.gate(got, REF, dt, "an inf")


# ---- eager_steps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raises", [False, True], ids=["leaves", "raises"])
@pytest.mark.parametrize("before", [None, "1", "0"], ids=["absent", "1", "0"])
def test_eager_steps_sets_0_and_restores_what_it_found(monkeypatch, before, raises):
    if before is None:
        monkeypatch.delenv("DDIMX_GRAPH", raising=False)
    else:
        monkeypatch.setenv("DDIMX_GRAPH", before)
    try:
        with H.eager_steps():
            assert os.environ["DDIMX_GRAPH"] == "0"
            if raises:
                raise KeyError("inside")
    except KeyError:
        assert raises
    else:
        assert not raises
    assert os.environ.get("DDIMX_GRAPH") == before


def test_eager_steps_nest():
    with H.eager_steps():
        with H.eager_steps():
            assert os.environ["DDIMX_GRAPH"] == "0"
        assert os.environ["DDIMX_GRAPH"] == "0"


# ---- sentinel and bits --------------------------------------------------------------------------------------------------------------------
def test_sentinel_and_bits():
    s = H.sentinel(3, 20, device="cpu")
    assert s.shape == (3, 20) and s.dtype == torch.float32 and bool(torch.isnan(s).all())
    assert H.bits(s).dtype == torch.int32 and bool((H.bits(s) == H.PATTERN).all())
    s[1, 4] = float("nan")  # torch's own NaN is another pattern: a stray NaN store shows
    assert int((H.bits(s) != H.PATTERN).sum()) == 1
    assert H.bits(s).data_ptr() == s.data_ptr()


# ---- the import rule ----------------------------------------------------------------------------------------------------------------------
def test_no_test_module_imports_another():
    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, "*.py")))
    assert len(files) > 40
    bad = [(os.path.basename(f), line.rstrip()) for f in files for line in open(f) if re.match(r"^(from|import) test_", line)]
    assert not bad, bad


def test_nothing_assigns_to_the_product_loss_module_or_the_oracle():
    here = os.path.dirname(os.path.abspath(__file__))
    pat = re.compile(r"setattr\(\s*(\w+\.)*(losses|ref_cpu)\s*,|^\s*(\w+\.)*(losses|ref_cpu)\.\w+\s*=[^=]")
    bad = [(os.path.basename(f), line.rstrip()) for f in sorted(glob.glob(os.path.join(here, "test_*.py"))) for line in open(f)
           if pat.search(line) and os.path.basename(f) != os.path.basename(__file__)]
    assert not bad, bad
