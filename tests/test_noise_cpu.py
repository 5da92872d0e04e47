"""The seeded noise stream without a GPU: the numpy reference against Random123's known-answer vectors, and NoiseStream's host
logic (ranges, shard arithmetic, the rank split, the noise / noise_fn exclusion of the samplers)."""
import numpy as np
import pytest
import torch

import ddim_audio_amd as D
from ddim_audio_amd import dist
from ddim_audio_amd.noise import NoiseStream
import noise_ref as R

# Random123's kat_vectors for philox4x32-10: (counter, key, result)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_reference_known_answers(ctr, key, want):
    got = R.philox4x32_10(*ctr, *key)
    assert tuple(int(v) for v in got) == want


def test_reference_words_layout_and_vectorisation():
    """words(): element 4 q + j of sample b is word j of counter (q, first_sample + b, k, tag); arrays = one call per counter."""
    seed, first, k, tag = 0x0123456789ABCDEF, 5, 7, 1
    w = R.words(seed, first, (3, 2, 2, 4), k, tag).reshape(3, -1)
    for b in range(3):
        for q in range(4):
            one = R.philox4x32_10(q, first + b, k, tag, seed & 0xFFFFFFFF, seed >> 32)
            assert [int(v) for v in one] == [int(v) for v in w[b, 4 * q:4 * q + 4]]
    assert w.dtype == np.uint32


def test_reference_normals_f32_against_f64():
    """The float32 path stays within the GPU test's bound scale of the float64 one (it rounds the angle, so it is the coarser of the
    two float32 evaluations), and the tails end at sqrt(48 ln 2)."""
    w = R.words(0x1234, 3, (1, 1, 256, 1024), 7)
    z64, r = R.normals64(w)
    z32 = R.normals32(w).astype(np.float64)
    assert np.abs(z64).max() <= np.sqrt(48 * np.log(2.0))
    assert r.max() <= np.sqrt(48 * np.log(2.0)) and r.min() >= 0.0
    assert np.abs(z32 - z64).max() <= 4e-6
    # the extreme words: u = 1 gives radius 0, u = 2^-24 the cut
    z, r = R.normals64(np.array([[0xFFFFFFFF, 0, 0, 0x80000000]], dtype=np.uint32))
    assert r[0, 0] == 0.0 and z[0, 0] == 0.0 and z[0, 1] == 0.0
    assert abs(r[0, 2] - np.sqrt(48 * np.log(2.0))) < 1e-12 and abs(z[0, 2] + r[0, 2]) < 1e-12 and abs(z[0, 3]) < 1e-9


def test_noise_stream_resolves_and_validates():
    assert D.NoiseStream is NoiseStream
    ns = NoiseStream(2 ** 64 - 1, 2 ** 32 - 1)
    assert (ns.seed, ns.first_sample) == (2 ** 64 - 1, 2 ** 32 - 1)
    assert NoiseStream(np.int64(7)).seed == 7 and NoiseStream(0).first_sample == 0
    for bad in (-1, 2 ** 64, 1.0, "1", None, True):
        with pytest.raises(ValueError):
            NoiseStream(bad)
    for bad in (-1, 2 ** 32, 0.5, False):
        with pytest.raises(ValueError):
            NoiseStream(1, bad)


def test_shard_arithmetic_and_rank_split():
    ns = NoiseStream(0xABC, 10)
    s = ns.shard(4)
    assert (s.seed, s.first_sample) == (0xABC, 14) and ns.first_sample == 10, "shard returns a new stream"
    assert s.shard(3).first_sample == 17 and ns.shard(0).first_sample == 10
    with pytest.raises(ValueError):
        ns.shard(-1)
    with pytest.raises(ValueError):
        ns.shard(2 ** 32 - 10)  # first_sample would leave 32 bits
    with pytest.raises(ValueError):
        ns.shard(True)
    # ragged split: n = 10 over 4 ranks = 3, 3, 2, 2
    los = [ns.for_rank(10, r, 4).first_sample - 10 for r in range(4)]
    assert los == [dist.shard_bounds(10, r, 4)[0] for r in range(4)] == [0, 3, 6, 8]
    assert ns.for_rank(10).first_sample == 10, "no process group: one rank, the whole batch"


def _no_device_work(monkeypatch):
    """Any use of the library or of the GPU fails the test: the argument check has to come first."""
    from ddim_audio_amd import _lib

    def boom(*a, **k):
        raise AssertionError("device work before the argument check")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)


def test_noise_and_noise_fn_together_raise_before_any_device_work(monkeypatch):
    _no_device_work(monkeypatch)
    ns = NoiseStream(1)
    x = torch.zeros(2, 2, 8, 16)
    alphas = torch.linspace(0.999, 0.01, 1000)
    betas = torch.linspace(1e-4, 2e-2, 1000)
    seq = list(range(0, 1000, 125))
    fake = lambda a, t: a  # noqa: E731
    with pytest.raises(ValueError, match="not both"):
        D.generalized_steps(x, seq, fake, alphas, None, eta=1.0, noise=ns, noise_fn=torch.randn_like)
    with pytest.raises(ValueError, match="not both"):
        D.inpaint_steps(x, seq, fake, alphas, None, y=x, mask=torch.ones_like(x), eta=1.0, noise=ns, noise_fn=torch.randn_like)
    with pytest.raises(ValueError, match="not both"):
        D.ddpm_steps(x, seq, fake, betas, None, noise=ns, noise_fn=lambda k, cur: torch.randn_like(cur))
    with pytest.raises(TypeError):
        D.generalized_steps(x, seq, fake, alphas, None, eta=1.0, noise=torch.Generator())
