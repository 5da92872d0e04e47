"""tests/model_harness.py on the CPU: every builder of the feature GPU tests keeps the config it had (the expected edits are written
out here), the whole-network gate accepts and rejects on either side of its thresholds, the eager-steps switch restores what it
found, the sentinel holds its pattern, the exact comparisons of two runs fail where they should and name the entry, the seeded
inputs are what the files that defined them had, and no test module imports another."""
import copy
import glob
import os
import re

import pytest
import torch

from ddim_audio_amd import configs, synth
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


# ---- exact comparisons of runs ------------------------------------------------------------------------------------------------------------
def _run(n=4):
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(2, 3, generator=g) for _ in range(n + 1)]
    return xs, [torch.randn(2, 3, generator=g) for _ in range(n)]


def _edited_run(run, which, i):
    xs, x0 = [v.clone() for v in run[0]], [v.clone() for v in run[1]]
    (xs, x0)[which][i][1, 2] += 1e-6
    return xs, x0


def test_same_run_passes_on_equal_runs_and_names_the_one_differing_entry():
    want = _run()
    H.same_run(([torch.zeros(2, 3)] + [v.clone() for v in want[0][1:]], [v.clone() for v in want[1]]), want, "xs[0] is the caller's")
    for i in range(1, 5):
        with pytest.raises(AssertionError, match=rf"case: xs\[{i}\]$"):
            H.same_run(_edited_run(want, 0, i), want, "case")
    for i in range(4):
        with pytest.raises(AssertionError, match=rf"case: x0_preds\[{i}\]$"):
            H.same_run(_edited_run(want, 1, i), want, "case")


def test_same_run_fails_on_a_length_mismatch_of_either_list_and_on_no_prediction():
    want = _run()
    with pytest.raises(AssertionError, match="short xs"):
        H.same_run((want[0][:-1], want[1]), want, "short xs")
    with pytest.raises(AssertionError, match="short x0"):
        H.same_run((want[0], want[1][:-1]), want, "short x0")
    with pytest.raises(AssertionError, match="long"):
        H.same_run((want[0] + want[0][-1:], want[1] + want[1][-1:]), want, "long")
    with pytest.raises(AssertionError, match="empty"):
        H.same_run((want[0][:1], []), (want[0][:1], []), "empty")


def test_same_list():
    want = _run()[1]
    H.same_list([v.clone() for v in want], want, "equal")
    H.same_list([], [], "both empty")
    for i in range(4):
        got = [v.clone() for v in want]
        got[i][0, 0] = -got[i][0, 0]
        with pytest.raises(AssertionError, match=rf"flat\[{i}\]$"):
            H.same_list(got, want, "flat")
    with pytest.raises(AssertionError, match="shorter"):
        H.same_list(want[:-1], want, "shorter")
    with pytest.raises(AssertionError, match="longer"):
        H.same_list(want + want[:1], want, "longer")


def test_differs_looks_at_the_last_sample_before_the_end_and_differs_anywhere_at_all_of_them():
    want = _run()
    assert not H.differs(want, want) and not H.differs_anywhere(want, want)
    early = _edited_run(want, 0, 1)   # only xs[1] differs: the runs met again before xs[-2]
    assert not H.differs(early, want) and H.differs_anywhere(early, want)
    late = _edited_run(want, 0, 3)    # xs[-2]
    assert H.differs(late, want) and H.differs_anywhere(late, want)
    first = _edited_run(want, 0, 0)   # xs[0] is the input: neither looks at it
    assert not H.differs(first, want) and not H.differs_anywhere(first, want)
    preds = _edited_run(want, 1, 2)   # nor at the predictions
    assert not H.differs(preds, want) and not H.differs_anywhere(preds, want)


def test_known_exact():
    g = torch.Generator().manual_seed(6)
    y = torch.randn(2, 1, 8, 4, generator=g)
    mask = torch.zeros(1, 1, 8, 1)
    mask[:, :, :3] = 1
    mask[:, :, 3] = 0.5  # a soft element is not known
    last = torch.where(torch.broadcast_to(mask, (2, 2, 8, 4)) == 1, torch.broadcast_to(y, (2, 2, 8, 4)), torch.randn(2, 2, 8, 4, generator=g))
    H.known_exact(last, y, mask)
    bad = last.clone()
    bad[1, 0, 2, 3] = torch.nextafter(bad[1, 0, 2, 3], torch.tensor(9.0))
    with pytest.raises(AssertionError, match="not y exactly"):
        H.known_exact(bad, y, mask)
    soft = last.clone()
    soft[0, 1, 3, 0] += 1  # outside the known region
    H.known_exact(soft, y, mask)
    with pytest.raises(AssertionError, match="no known element"):
        H.known_exact(last, y, torch.zeros(1, 1, 8, 1))
    with pytest.raises(AssertionError, match="no known element"):
        H.known_exact(last, y, torch.full((1, 1, 1, 1), 0.5))


def test_spread_and_pair_data():
    for n in (2, 6, 7, 9, 10, 12, 25):  # what test_gpu_solver.py, test_gpu_sde.py and test_gpu_unic.py each defined
        want = sorted({int(round(999 * (i / (n - 1)) ** 1.7)) for i in range(n)})
        assert H.spread(n) == want and len(want) == n and want[0] == 0 and want[-1] == 999
    assert H.spread(1) == [400]  # tests/pool_ref.py's, which those three never asked for
    steps = [b - a for a, b in zip(H.spread(10), H.spread(10)[1:])]
    assert steps == sorted(steps) and len(set(steps)) == len(steps), "uneven on purpose"
    x, y = H.pair_data("inp.empty", (2, 2, 4, 8))
    assert torch.equal(x, synth.gaussian("inp.empty.x", (2, 2, 4, 8))) and torch.equal(y, synth.gaussian("inp.empty.y", (2, 2, 4, 8)))
    assert not torch.equal(x, y)


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
