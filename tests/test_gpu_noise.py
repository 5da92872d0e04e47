"""Seeded device noise on the GPU (ddim_audio_amd.NoiseStream, ddimx_noise_fill) and the samplers that draw from it.

The Philox words against the numpy reference (tests/noise_ref.py) bit for bit; the normals against its float64 values within a
bound counted from the roundings; the moments of 2^22 normals within the six-sigma sampling error of exact ones; shard invariance
bit for bit; the replayed stochastic step against the eager one and against the materialised noise fed to the path that existed
before, bit for bit; against the CPU oracle; sample identity across batch splits; inpainting, ddpm_steps, graph ownership, and
the untouched default (torch's generator, eager)."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import _lib, synth
from ddim_audio_amd.dist import shard_bounds
from ddim_audio_amd.graphs import GraphOwner
from ddim_audio_amd.inpaint import InpaintStepper
from ddim_audio_amd.noise import NoiseStream
from ddim_audio_amd.sampler import DDIMStepper
from ddim_audio_amd.schedule import ddim_coefficients, inpaint_coefficients, make_schedule
from oracle import ref_cpu
import gpu_util as G
import model_harness as MH
from model_harness import MODE_IDS, TINY, U
import noise_ref as R

pytestmark = pytest.mark.gpu
MODES = [s for s, _ in MH.MODES]  # the dtype strings alone
SEEDS = [0, 0x1234, 2 ** 64 - 1]
FIRSTS = [0, 3, 2 ** 32 - 9]
SHAPES = [(1, 2, 8, 16), (5, 2, 32, 256), (8, 1, 1, 4)]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- 4. the words, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_words_equal_the_reference(seed, shape):
    for first in FIRSTS:
        ns = NoiseStream(seed, first)
        for k in (0, 7):
            for tag in (0, 1):
                got = _u32(ns.words(shape, k, G.dev(), tag=tag))
                assert got.shape == shape
                assert np.array_equal(got, R.words(seed, first, shape, k, tag)), (first, k, tag)


def test_draw_index_comes_from_the_device_counter():
    ns, shape = NoiseStream(0x1234, 3), (5, 2, 32, 256)
    ctr = torch.full((1,), 7, dtype=torch.int32, device=G.dev())
    a = ns.fill(torch.empty(shape, dtype=torch.int32, device=G.dev()), ctr, 0)
    b = ns.fill(torch.empty(shape, dtype=torch.int32, device=G.dev()), None, 7)
    assert torch.equal(a, b) and np.array_equal(_u32(a), R.words(0x1234, 3, shape, 7))
    c = ns.fill(torch.empty(shape, dtype=torch.int32, device=G.dev()), ctr, 2)
    assert np.array_equal(_u32(c), R.words(0x1234, 3, shape, 9)), "draw = draw_base + counter"
    za, zb = (ns.fill(torch.empty(shape, device=G.dev()), s, d) for s, d in ((ctr, 0), (None, 7)))
    assert torch.equal(za, zb) and torch.equal(za, ns.step_noise(shape, 7, G.dev()))


def test_fill_rejects_what_does_not_fit():
    lib, dev = _lib.load(), G.dev()
    buf = torch.empty(4096, device=dev)
    fill = lambda *a: lib.ddimx_noise_fill(_lib.ptr(buf), *a, _lib.stream())  # noqa: E731  (B, per, seed, first, step, base, tag, kind)
    assert fill(2, 16, 1, 0, None, 0, 0, 0) == 0
    for bad in ((0, 16, 1, 0, None, 0, 0, 0), (65536, 16, 1, 0, None, 0, 0, 0), (2, 18, 1, 0, None, 0, 0, 0), (2, 0, 1, 0, None, 0, 0, 0),
                (2, 16, 1, 2 ** 32 - 1, None, 0, 0, 0), (2, 16, 1, 0, None, 0, 0, 2), (2, 4 * (2 ** 32 + 1), 1, 0, None, 0, 0, 0)):
        assert fill(*bad) != 0, bad
    assert lib.ddimx_noise_fill(None, 2, 16, 1, 0, None, 0, 0, 0, _lib.stream()) != 0
    torch.cuda.synchronize()
    ns = NoiseStream(1, 2 ** 32 - 1)
    with pytest.raises(ValueError):
        ns.step_noise((2, 16), 0, dev)
    with pytest.raises(ValueError):
        NoiseStream(1).step_noise((2, 18), 0, dev)
    with pytest.raises(ValueError):
        NoiseStream(1).step_noise((2, 16), 2 ** 32, dev)
    with pytest.raises(ValueError):
        NoiseStream(1).fill(torch.empty((2, 16), dtype=torch.float16, device=dev))


# ---- 5. the normals, to a counted bound ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(1, 1, 1024, 1024)], ids=str)
@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_normals_within_the_rounding_bound(seed, shape):
    """|z_gpu - z_ref| <= 8 * 2^-24 * r + 2^-126 against the float64 normals of the same words, r the float64 radius of the pair.

    The 8 is counted, in units of 2^-24 relative to r (the sine and cosine are at most 1 in magnitude and v is exact, so every
    error scales with r): logf at most 1 ulp = 2 units, halved by the square root = 1 (the factor -2 is exact; u is exact);
    sqrtf's own rounding, at most 1 ulp = 2; sincospif at most 1 ulp = 2; the final product 1 (half an ulp of r * cs, which is at
    most r).  That is 6; 2 more cover the second-order terms.  The figure used for each of the three functions is 1 ulp (no HIP
    math documentation is installed with the ROCm this was written against that would give a larger one); the kernel calls the
    accurate forms, not the __-prefixed ones.  The test prints the largest error and its share of the bound before it asserts."""
    for first in FIRSTS[:2] if shape[-1] == 1024 else FIRSTS:
        ns = NoiseStream(seed, first)
        for k, tag in ((0, 1), (7, 0)):
            w = _u32(ns.words(shape, k, G.dev(), tag=tag))
            z = (ns.initial(shape, G.dev()) if tag == 1 else ns.step_noise(shape, k, G.dev())).cpu().numpy().astype(np.float64)
            want, r = R.normals64(w)
            err, bound = np.abs(z - want), 8 * U * r + TINY
            worst = float((err / bound).max())
            print(f"seed {seed:#x} first {first} draw {k} tag {tag} {shape}: max err {err.max():.3e}, max err / bound {worst:.3f}")
            assert np.isfinite(z).all() and (err <= bound).all(), (first, k, tag, worst)


# ---- 6. moments ---------------------------------------------------------------------------------------------------------------------
def test_moments_of_four_million_normals():
    """N = 2^22 values of step_noise(k = 7), seed 0x1234, first_sample 3.  The gates are the six-sigma sampling errors of exact
    normals: mean 1/sqrt(N), variance sqrt(2/N), fourth moment sqrt(96/N), correlation 1/sqrt(N).  The float64 reference values
    for exactly these parameters: mean 4.4e-4, variance 1.00083, fourth moment 3.0038, lag-1 -3.6e-4, lag-4 2e-5."""
    z = NoiseStream(0x1234, 3).step_noise((1, 1, 4096, 1024), 7, G.dev()).cpu().numpy().astype(np.float64).reshape(-1)
    n = z.size
    assert n == 2 ** 22
    mean, var = z.mean(), z.var()
    m4 = (z ** 4).mean()  # the raw fourth moment: its sampling variance is (E z^8 - 9) / N = 96 / N
    c = z - mean
    lag = {d: float((c[:-d] * c[d:]).mean() / var) for d in (1, 4)}
    print(f"mean {mean:.3e} var {var:.6f} m4 {m4:.5f} lag1 {lag[1]:.3e} lag4 {lag[4]:.3e} max |z| {np.abs(z).max():.3f}")
    assert abs(mean) <= 6 / np.sqrt(n)
    assert abs(var - 1) <= 6 * np.sqrt(2 / n)
    assert abs(m4 - 3) <= 6 * np.sqrt(96 / n)
    assert abs(lag[1]) <= 6 / np.sqrt(n) and abs(lag[4]) <= 6 / np.sqrt(n)
    assert np.abs(z).max() <= np.sqrt(48 * np.log(2.0)) * (1 + 8 * U)


# ---- 7. shard invariance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0, 8), (3, 5), (7, 8)])
def test_a_shard_is_the_rows_of_the_full_batch(lo, hi):
    ns, dev = NoiseStream(0xFEEDFACECAFE, 5), G.dev()
    full, part = (8, 2, 32, 256), (hi - lo, 2, 32, 256)
    sh = ns.shard(lo)
    assert torch.equal(ns.step_noise(full, 3, dev)[lo:hi], sh.step_noise(part, 3, dev))
    assert torch.equal(ns.initial(full, dev)[lo:hi], sh.initial(part, dev))
    assert torch.equal(ns.words(full, 3, dev)[lo:hi], sh.words(part, 3, dev))
    assert not torch.equal(ns.initial(part, dev), ns.step_noise(part, 0, dev)), "the tag separates x_T from the step noise"


# ---- 8. graph = eager = materialised ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.5, 1.0])
@pytest.mark.parametrize("name", ["tiny", "audio"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_replayed_step_equals_eager_and_materialised_noise(mode, name, eta):
    cfg, m = MH.build(name, mode, 5, mode="eval")
    a = MH.alphas(cfg)
    seq = list(range(0, 1000, 100))
    x = synth.gaussian("noise.replay", (4, 2, 32, cfg.model.f_size))  # B = 4: the captured graph forks into two shards
    ns = NoiseStream(0xC0FFEE, 2)
    xs, x0 = D.generalized_steps(x.cuda(), seq, m, a, None, eta=eta, noise=ns)
    assert len(xs) == 11 and len(x0) == 10
    # the stream run replays one captured graph
    xt = x.cuda()
    with torch.no_grad():
        st = DDIMStepper(m, xt, ddim_coefficients(seq, a, eta), noise=ns)
        try:
            for i in range(len(seq)):
                st.step()
                if i >= 1:
                    assert st.captures == 1 and st.graph is not None, i
                assert torch.equal(st.xt.cpu(), xs[i + 1]) and torch.equal(st.x0.cpu(), x0[i]), i
        finally:
            st.close()
    # (b) the path that exists without the stream (noise_fn: eager steps), fed the materialised tensors
    xt = x.cuda()
    with torch.no_grad():
        # (fork=False: eager steps on one stream, the same bits -- DESIGN section 9a)
        st = DDIMStepper(m, xt, ddim_coefficients(seq, a, eta), fork=False,
                         noise_fn=lambda ref: ns.step_noise(ref.shape, st.done, ref.device))
        try:
            for i in range(len(seq)):
                st.step()
                assert torch.equal(st.xt.cpu(), xs[i + 1]) and torch.equal(st.x0.cpu(), x0[i]), i
            assert st.captures == 0 and st.graph is None
        finally:
            st.close()
    # (a) the same call, eager
    with MH.eager_steps():
        e_xs, e_x0 = D.generalized_steps(x.cuda(), seq, m, a, None, eta=eta, noise=ns)
        for i in range(len(seq)):
            assert torch.equal(xs[i + 1], e_xs[i + 1]) and torch.equal(x0[i], e_x0[i]), i


def test_eta_zero_with_a_stream_makes_no_buffer_and_draws_nothing():
    cfg, m = MH.build("tiny", MODES[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = list(range(0, 1000, 200))
    x = synth.gaussian("noise.eta0", (4, 2, 32, 32))
    want_xs, want_x0 = D.generalized_steps(x.cuda(), seq, m, a, None, eta=0.0)
    xs, x0 = D.generalized_steps(x.cuda(), seq, m, a, None, eta=0.0, noise=NoiseStream(1))
    assert all(torch.equal(u, v) for u, v in zip(xs[1:] + x0, want_xs[1:] + want_x0))
    with torch.no_grad():
        st = DDIMStepper(m, x.cuda(), ddim_coefficients(seq, a, 0.0), noise=NoiseStream(1))
    assert st.noise_buf is None
    st.close()
    with pytest.raises(ValueError):
        DDIMStepper(m, x.cuda(), ddim_coefficients(seq, a, 1.0), noise=NoiseStream(1), noise_fn=torch.randn_like)


# ---- 9. against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_stream_sampler_matches_oracle_with_the_same_noise(eta):
    """test_gpu_configs.test_sampler_eta_nonzero_matches_oracle_with_the_drawn_noise with the noise from a NoiseStream on both sides
    (the same gates, rtol = atol = 2e-5)."""
    alphas = MH.alphas()
    fake = lambda x, t: 0.1 * x + 0.01 * t.float().view(-1, 1, 1, 1)  # noqa: E731  (a stand-in model, torch ops)
    seq = list(range(0, 1000, 125))
    x = synth.gaussian("eta.x", (2, 2, 8, 16))
    ns = NoiseStream(4321)
    xs, x0 = D.generalized_steps(x.cuda().clone(), seq, fake, alphas, None, eta=eta, noise=ns)
    exs, ex0 = ref_cpu.generalized_steps(x.clone(), seq, fake, alphas, None, eta=eta,
                                         noise_fn=lambda k, ref: ns.step_noise(ref.shape, k, G.dev()).cpu())
    assert len(xs) == len(exs) and len(x0) == len(ex0)
    for k, (u, v) in enumerate(zip(xs[1:], exs[1:])):
        assert torch.allclose(u, v, rtol=2e-5, atol=2e-5), k
    for k, (u, v) in enumerate(zip(x0, ex0)):
        assert torch.allclose(u, v, rtol=2e-5, atol=2e-5), k
    xs0, _ = D.generalized_steps(x.cuda().clone(), seq, fake, alphas, None, eta=0.0)
    assert not torch.allclose(xs0[-2], xs[-2], rtol=1e-3, atol=1e-3), "the noise really entered"


# ---- 10. a sample is (seed, global index), whatever the batch -----------------------------------------------------------------------
def test_sample_identity_across_batch_splits():
    """Rests on the forward's tested batch independence: the B = 8 run equals two B = 4 runs from ns and ns.shard(4)."""
    cfg, m = MH.build("audio", MODES[1], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = list(range(0, 1000, 167))
    assert len(seq) == 6
    dev = G.dev()

    def run(ns, b):
        x = ns.initial((b, 2, 64, 256), dev)
        return D.generalized_steps(x, seq, m, a, [-1], eta=1.0, noise=ns)[0][-1]

    ns = NoiseStream(0x5EED)
    full = run(ns, 8)
    halves = torch.cat([run(ns, 4), run(ns.shard(4), 4)])
    assert torch.isfinite(full).all() and torch.equal(full, halves)
    bounds = [shard_bounds(8, r, 3) for r in range(3)]
    ragged = torch.cat([run(ns.for_rank(8, r, 3), hi - lo) for r, (lo, hi) in enumerate(bounds)])
    assert torch.equal(full, ragged), "three ranks, 3 + 3 + 2 samples"
    other = run(NoiseStream(0x5EED + 1), 8)
    assert not torch.allclose(full, other, rtol=1e-3, atol=1e-3)


# ---- 11. inpainting -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_inpaint_with_a_stream(mode):
    cfg, m = MH.build("tiny", mode, 5, mode="eval")
    a = MH.alphas(cfg)
    shape = (4, 2, 32, 32)
    x, y = synth.gaussian("noise.inp.x", shape), synth.gaussian("noise.inp.y", shape)
    seq = [0, 200, 400, 600, 800]
    ns = NoiseStream(77, 1)
    # empty mask, no guidance: generalized_steps with the same stream, bit for bit
    want_xs, want_x0 = D.generalized_steps(x.cuda(), seq, m, a, None, eta=1.0, noise=ns)
    xs, x0 = D.inpaint_steps(x.cuda(), seq, m, a, None, y=y, mask=torch.zeros(1, 1, 1, 1), guidance=0.0, eta=1.0, noise=ns)
    for i in range(len(seq)):
        assert torch.equal(xs[i + 1], want_xs[i + 1]) and torch.equal(x0[i], want_x0[i]), i
    assert not torch.equal(xs[1], D.generalized_steps(x.cuda(), seq, m, a, [0], eta=0.0)[0][1])
    # a real mask with replacement: the known region of the final sample is y exactly
    mask = torch.ones(shape[0], 1, shape[2], 1)
    mask[:, :, 8:16] = 0
    rxs, _ = D.inpaint_steps(x.cuda(), seq, m, a, [-1], y=y, mask=mask, replace=True, eta=1.0, noise=ns)
    known = torch.broadcast_to(mask, shape) == 1
    assert torch.equal(rxs[-1][known], y[known]) and not torch.equal(rxs[-1][~known], y[~known])
    # guided, eta = 0.5: captured once, and graph = eager bit for bit
    kw = dict(y=y, mask=mask, guidance=0.3, replace=True, eta=0.5, noise=ns)
    g_xs, g_x0 = D.inpaint_steps(x.cuda(), seq, m, a, None, **kw)
    dev = G.dev()
    mk = torch.broadcast_to(mask, shape).to(dev).contiguous()
    yk = torch.where(mk == 0, torch.zeros((), device=dev), y.to(dev)).contiguous()
    with torch.no_grad():
        st = InpaintStepper(m, x.cuda(), yk, mk, inpaint_coefficients(seq, a, 0.5, 0.3), True, True, noise=ns)
        try:
            for i in range(len(seq)):
                st.step()
                assert torch.equal(st.xt.cpu(), g_xs[i + 1]), i
            assert st.captures == 1 and st.graph is not None and st.noise_buf is not None
        finally:
            st.close()
    with MH.eager_steps():
        e_xs, e_x0 = D.inpaint_steps(x.cuda(), seq, m, a, None, **kw)
        for i in range(len(seq)):
            assert torch.equal(g_xs[i + 1], e_xs[i + 1]) and torch.equal(g_x0[i], e_x0[i]), i


# ---- 12. ddpm_steps -----------------------------------------------------------------------------------------------------------------
def test_ddpm_steps_with_a_stream_equals_the_materialised_noise():
    cfg, m = MH.build("tiny", MODES[0], 5, mode="eval")
    betas = make_schedule(cfg.diffusion)[0]
    seq = list(range(0, 1000, 125))
    x = synth.gaussian("noise.ddpm", (3, 2, 16, 32))
    ns = NoiseStream(99, 4)
    xs, x0 = D.ddpm_steps(x.cuda(), seq, m, betas, None, noise=ns)
    wxs, wx0 = D.ddpm_steps(x.cuda(), seq, m, betas, None, noise_fn=lambda k, cur: ns.step_noise(cur.shape, k, cur.device))
    assert len(xs) == 9 and len(x0) == 8
    for i in range(8):
        assert torch.equal(xs[i + 1], wxs[i + 1]) and torch.equal(x0[i], wx0[i]), i
    assert torch.isfinite(xs[-1]).all()


# ---- 13. ownership ------------------------------------------------------------------------------------------------------------------
def test_noisy_stepper_recaptures_when_the_model_moves_on_and_close_keeps_the_buffer_until_the_graph_is_gone():
    """The pattern of test_gpu_solver's ownership test for a stepper that draws from a stream: after ``model.float()`` or a larger
    batch the next step runs eagerly and captures again, on the same trajectory bit for bit as a stepper that never captures."""
    cfg, m = MH.build("audio", MODES[1], 0, mode="eval")
    a = MH.alphas(cfg)
    seq = list(range(0, 1000, 100))
    coef = ddim_coefficients(seq, a, 1.0)
    x = synth.gaussian("noise.own", (5, 2, 64, 256)).cuda()
    ns = NoiseStream(31337, 6)

    def run(disturb, use_graph=True):
        xt = x.clone()
        with torch.no_grad():
            st = DDIMStepper(m, xt, coef, use_graph=use_graph, fork=use_graph, noise=ns)  # eager: one stream, the same bits
            for i in range(len(seq)):
                disturb(i, st)
                st.step()
            torch.cuda.synchronize()
            out = (xt.clone(), st.x0.clone(), st.captures)
            buf = st.noise_buf
            st.close()
        assert st.graph is None and st._ctx is None and st._refs is None
        assert st.noise_buf is buf and buf is not None, "the buffer outlives the graph: close() drops the graph, not the buffer"
        assert torch.equal(buf, ns.step_noise(buf.shape, len(seq) - 1, buf.device)), "... and still holds the last draw"
        return out

    ref = run(lambda i, st: None, use_graph=False)
    assert ref[2] == 0
    once = run(lambda i, st: None)
    assert once[2] == 1 and torch.equal(once[0], ref[0]) and torch.equal(once[1], ref[1])

    def move(i, st):
        if i == 4:
            assert st.graph is not None and st._ctx is not None
            m.float()  # nn.Module._apply: the model drops its packed weights, tables, workspaces, embedding table
            assert m._packed is None and m._workspace is None

    def grow(i, st):
        if i == 4:
            m.reserve(x.device, 9, 64, 0)  # what a forward of a larger batch does first: a new, larger workspace

    for disturb in (move, grow):
        got = run(disturb)
        assert got[2] == 2, "the stepper must re-capture after the model re-allocated its buffers"
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


# ---- 14. the default is untouched ---------------------------------------------------------------------------------------------------
def test_default_eta_path_keeps_torch_generator_and_never_captures(monkeypatch):
    cfg, m = MH.build("tiny", MODES[0], 5, mode="eval")
    a = MH.alphas(cfg)
    seq = list(range(0, 1000, 125))
    x = synth.gaussian("noise.default", (4, 2, 32, 32))
    captures = []
    real = GraphOwner._capture_graph
    monkeypatch.setattr(GraphOwner, "_capture_graph", lambda self, *a, **k: (captures.append(1), real(self, *a, **k))[1])
    torch.manual_seed(2024)
    xs, x0 = D.generalized_steps(x.cuda(), seq, m, a, None, eta=1.0)
    assert not captures
    torch.manual_seed(2024)
    xt = x.cuda()
    with torch.no_grad():
        st = DDIMStepper(m, xt, ddim_coefficients(seq, a, 1.0), noise_fn=torch.randn_like, fork=False)
        try:
            for i in range(len(seq)):
                st.step()
                assert torch.equal(st.xt.cpu(), xs[i + 1]) and torch.equal(st.x0.cpu(), x0[i]), i
            assert st.captures == 0 and st.noise_buf is None
        finally:
            st.close()
    assert not captures
    D.generalized_steps(x.cuda(), seq, m, a, [-1], eta=0.0)
    assert captures == [1], "the deterministic run does capture (the probe works)"
