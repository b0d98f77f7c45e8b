"""The volume noise generator and the low-field degradation (no GPU): the integer streams next to a pure-Python restatement of the
hash, the table and its index arithmetic, the accuracy of the normals against the exact quantile, their moments, the Rician loop
through ``estimate_sigma_np``, the modes of the numpy specification, the refusals and the C entry's."""
import math
import os
import sys
from fractions import Fraction
from statistics import NormalDist

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mri_superresolution_amd import volume_denoise as D          # noqa: E402
from mri_superresolution_amd import volume_kspace as K           # noqa: E402
from mri_superresolution_amd import volume_lowfield as LF        # noqa: E402
from denoiseutil import phantom                                   # noqa: E402

M32 = 0xffffffff
QUANTILE_DEVIATION = 1.3e-5      # the largest | |z| - exact quantile | of this layout, measured over 2^22 words against inv_cdf
MOMENT_SEED = 1                  # the moments test asserts on this seed only


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- the integer streams

def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    return x ^ (x >> 16)


def noise_key(seed):
    return mix32((seed & M32) ^ mix32(((seed >> 32) + 0x9e3779b9) & M32))


def words(seed, i):
    key = noise_key(seed)
    return mix32(key ^ mix32((2 * i + 1) & M32)), mix32((key + 0x9e3779b9 + mix32((2 * i) & M32)) & M32)


def test_integer_streams_equal_a_scalar_restatement_of_the_hash():
    last = 2 ** 31 - 2                      # the last voxel of the largest volume
    for seed in (0, 1, 12345, 0xdeadbeef, 0x123456789abcdef0, 2 ** 64 - 1, 5 << 32):
        assert int(LF.noise_key_np(seed)) == noise_key(seed)
        for start, count in ((0, 5), (1000, 3), (2 ** 30 - 1, 3), (last - 3, 4)):
            h1, h2 = LF.hashed_words_np(seed, count, start)
            assert h1.dtype == h2.dtype == np.uint32 and h1.shape == h2.shape == (count,)
            for k in range(count):
                assert (int(h1[k]), int(h2[k])) == words(seed, start + k), (seed, start + k)
    assert int(LF.noise_key_np(0x123456789abcdef0)) != int(LF.noise_key_np(0x9abcdef0))      # the high word counts
    assert int(LF.noise_key_np(-1)) == noise_key(2 ** 64 - 1)                                # the low 64 bits of any integer
    with pytest.raises(ValueError, match="voxels"):
        LF.hashed_words_np(0, 2, last)


# ---------------------------------------------------------------- the table, the index, the fraction

def test_table_is_monotone_and_ends_at_zero():
    T, Dt, base = LF.normal_table()
    assert T.dtype == Dt.dtype == np.float32 and T.shape == (LF.KNOTS,) == (1665,) and Dt.shape == (1664,) and base.shape == (32,)
    assert np.all(T[1:] < T[:-1]) and np.all(Dt < 0) and np.array_equal(Dt, T[1:] - T[:-1])
    assert abs(float(T[-1])) <= 1e-6 and 6.3 < float(T[0]) < 6.4
    inv = NormalDist().inv_cdf
    a = LF.knot_positions()
    assert a[0] == 0 and a[1] == 1 and a[-1] == 2 ** 31 and np.all(np.diff(a) > 0)
    for k in (0, 1, 2, 63, 64, 700, 1663, 1664):
        assert T[k] == np.float32(-inv((int(a[k]) + 0.5) / 2.0 ** 32))
    assert np.array_equal(base, 64 * np.maximum(np.arange(32) - 7, 0))      # the closed form the kernel uses
    table = LF.device_table()
    assert table.dtype == np.float32 and table.shape == (2 * 1665,) and np.array_equal(bits(table[:1665]), bits(T))
    assert np.array_equal(bits(table[1665:-1]), bits(Dt)) and table[-1] == 0
    assert not T.flags.writeable and LF.normal_table()[0] is T


def edge_values():
    m = [0, 1, 2, 2 ** 31 - 1]
    for t in range(31):
        m += [2 ** t - 1, 2 ** t, 2 ** t + (2 ** t) // 3, 2 ** (t + 1) - 1]
    return np.array(sorted(set(x for x in m if 0 <= x < 2 ** 31)), dtype=np.int64)


def test_segment_index_equals_searchsorted_on_the_knots():
    a = LF.knot_positions()
    m = np.concatenate([np.random.default_rng(3).integers(0, 2 ** 31, 100000), edge_values()])
    k, shift = LF.segment_index(m)
    assert np.array_equal(k, np.searchsorted(a, m, side="right") - 1) and k.min() == 0 and k.max() == 1663
    assert np.array_equal(a[k + 1] - a[k], np.int64(1) << shift)           # a segment is 2^shift wide
    assert shift.min() == 0 and shift.max() == 24


def test_every_fraction_is_exact_in_float32():
    m = edge_values()
    k, shift = LF.segment_index(m)
    a = LF.knot_positions()
    for mi, ki, si in zip(m.tolist(), k.tolist(), shift.tolist()):
        frac = mi & ((1 << si) - 1)
        assert frac == mi - int(a[ki]) and frac < 2 ** 24
        f = np.ldexp(np.float32(frac), -si)
        assert f.dtype == np.float32 and Fraction(float(np.float32(frac))) == frac and Fraction(float(f)) == Fraction(frac, 1 << si)
    # the whole path on those words, both signs: T[k] + f D[k] in float32, then the sign bit
    T, Dt, _ = LF.normal_table()
    for sign in (0, 0x80000000):
        h = (m.astype(np.uint32) | np.uint32(sign))
        z = LF.normal_from_words_np(h)
        f = np.array([np.ldexp(np.float32(mi & ((1 << si) - 1)), -si) for mi, si in zip(m.tolist(), shift.tolist())], dtype=np.float32)
        want = T[k] + f * Dt[k]
        assert z.dtype == np.float32 and np.array_equal(bits(z), bits(want) ^ np.uint32(sign))
    assert LF.normal_from_words_np(np.array([0], dtype=np.uint32))[0] == T[0]       # the largest normal there is


def test_normals_follow_the_exact_quantile():
    """| |z| - (-Phi^-1((m + 0.5) / 2^32)) | <= twice the 1.3e-5 measured for this layout (S = 6, 1665 knots) over 2^22 words; the
    twofold margin covers the sampling of the maximum."""
    h = np.random.default_rng(11).integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32)
    z = LF.normal_from_words_np(h).astype(np.float64)
    inv = NormalDist().inv_cdf
    exact = np.array([-inv(((int(x) & 0x7fffffff) + 0.5) / 2.0 ** 32) for x in h])
    worst = float(np.abs(np.abs(z) - exact).max())
    print(f"largest deviation from the float64 quantile: {worst:.3e}")
    assert worst <= 2 * QUANTILE_DEVIATION
    assert np.array_equal(np.signbit(z), (h >> np.uint32(31)).astype(bool))


def test_moments_of_the_two_streams():
    """Bounds from the sample size alone: five standard errors of the mean, the variance and a correlation of N normals."""
    N = 1 << 20
    z1, z2 = LF.hashed_normals_np(MOMENT_SEED, N)
    assert z1.dtype == z2.dtype == np.float32 and z1.shape == z2.shape == (N,)
    a, b = z1.astype(np.float64), z2.astype(np.float64)
    corr = lambda x, y: float(np.corrcoef(x, y)[0, 1])      # noqa: E731
    figures = {"mean re": a.mean(), "mean im": b.mean(), "var re - 1": a.var() - 1, "var im - 1": b.var() - 1, "corr re im": corr(a, b),
               "corr re shifted": corr(a[:-1], a[1:]), "corr im shifted": corr(b[:-1], b[1:]), "corr re im shifted": corr(a[:-1], b[1:])}
    print(figures)
    for name, value in figures.items():
        bound = 5 * math.sqrt(2.0 / N) if name.startswith("var") else 5 / math.sqrt(N)
        assert abs(value) <= bound, (name, value, bound)
    assert abs(float((a ** 4).mean()) - 3) <= 5 * math.sqrt(96.0 / N)      # the fourth moment's standard error is sqrt(96 / N)


# ---------------------------------------------------------------- the Rician loop

def test_rician_air_gives_sigma_back():
    clean = phantom()
    air = clean == 0
    n = int(air.sum())
    assert n >= 10 ** 4
    sigma = 20.0
    noisy = LF.add_noise_np(clean, sigma, seed=7)
    assert noisy.dtype == np.float32 and noisy.shape == clean.shape and np.all(noisy >= 0)
    bound = 5 / (2 * math.sqrt(n))                               # five standard errors of a Rayleigh second moment, relative
    got, count = D.estimate_sigma_np(noisy, air.astype(np.uint8))
    mean = float(noisy[air].astype(np.float64).mean())
    print(f"sigma {float(got):.4f} from {count} air voxels, air mean {mean:.4f}, relative bound {bound:.4f}")
    assert count == n and abs(float(got) / sigma - 1) <= bound
    assert abs(mean / (sigma * math.sqrt(math.pi / 2)) - 1) <= bound
    # inside the head the noise is nearly Gaussian around sqrt(A^2 + sigma^2)
    core = clean == 900
    assert abs(float(noisy[core].astype(np.float64).mean()) - math.sqrt(900.0 ** 2 + sigma ** 2)) <= 5 * sigma / math.sqrt(int(core.sum()))


# ---------------------------------------------------------------- modes

def test_modes_seeds_and_frames():
    rng = np.random.default_rng(5)
    v = rng.uniform(-50.0, 4095.0, (3, 5, 7)).astype(np.float32)
    n_re, n_im = (rng.normal(0, 20, v.shape).astype(np.float32) for _ in range(2))
    assert np.array_equal(bits(LF.add_noise_np(v, 3.0, noise=(n_re, n_im), rician=False)), bits(v + n_re))
    re = v + n_re
    assert np.array_equal(bits(LF.add_noise_np(v, 0.0, noise=(n_re, n_im))), bits(np.sqrt(re * re + n_im * n_im)))
    assert np.array_equal(bits(LF.add_noise_np(v, 0.0, seed=3)), bits(np.sqrt(v * v)))              # sigma = 0: no special case
    z1, z2 = LF.hashed_normals_np(9, v.size)
    s = np.float32(12.5)
    re, im = v + (s * z1).reshape(v.shape), (s * z2).reshape(v.shape)
    assert np.array_equal(bits(LF.add_noise_np(v, 12.5, seed=9)), bits(np.sqrt(re * re + im * im)))
    assert np.array_equal(bits(LF.add_noise_np(v, 12.5, seed=9, rician=False)), bits(re))
    assert np.array_equal(bits(LF.add_noise_np(v, 12.5, seed=9)), bits(LF.add_noise_np(v.copy(), 12.5, seed=9)))
    assert not np.array_equal(LF.add_noise_np(v, 12.5, seed=9), LF.add_noise_np(v, 12.5, seed=10))
    # the index is the C-order index, whatever the memory order of the argument
    assert np.array_equal(bits(LF.add_noise_np(np.asfortranarray(v), 12.5, seed=9)), bits(LF.add_noise_np(v, 12.5, seed=9)))
    # NaN and Inf go through the arithmetic
    w = v.copy()
    w[0, 0, 0], w[1, 1, 1], w[2, 2, 2] = np.nan, np.inf, -np.inf
    got = LF.add_noise_np(w, 12.5, seed=9)
    assert np.isnan(got[0, 0, 0]) and got[1, 1, 1] == np.inf and got[2, 2, 2] == np.inf and np.isfinite(got).sum() == w.size - 3
    # the degradation: truncation, then the noise
    hr = rng.uniform(0.0, 1000.0, (8, 6, 10)).astype(np.float32)
    low = K.truncate2_np(hr, (0, 1, 2), "hamming")
    assert np.array_equal(bits(LF.simulate_lowfield_np(hr, window="hamming", sigma=5.0, seed=2)), bits(LF.add_noise_np(low, 5.0, seed=2)))
    assert np.array_equal(bits(LF.simulate_lowfield_np(hr, sigma=5.0, seed=2, truncate=False, rician=False)),
                          bits(LF.add_noise_np(hr, 5.0, seed=2, rician=False)))
    # the frames of 4-D scans: no seed twice, over frames and over scans
    seeds = LF.frame_seeds(0, 0, 4) + LF.frame_seeds(0, 1, 4) + LF.frame_seeds(1, 0, 4)
    assert len(set(seeds)) == 12 and all(0 <= x < 2 ** 64 for x in seeds) and LF.frame_seeds(0, 0, 4) == LF.frame_seeds(0, 0, 6)[:4]
    frames = [LF.add_noise_np(v, 12.5, seed=x) for x in LF.frame_seeds(3, 0, 3)]
    assert not any(np.array_equal(frames[i], frames[j]) for i in range(3) for j in range(i))


# ---------------------------------------------------------------- refusals, the entry

def test_refusals():
    import torch
    v = np.zeros((4, 4, 4), dtype=np.float32)
    for sigma in (-1.0, float("nan"), float("inf"), "x", None, True, 1e39):
        with pytest.raises(ValueError, match="sigma"):
            LF.add_noise_np(v, sigma)
    for seed in (1.5, "0", None, True):
        with pytest.raises(ValueError, match="seed"):
            LF.add_noise_np(v, 1.0, seed=seed)
    with pytest.raises(ValueError, match="float32"):
        LF.add_noise_np(v.astype(np.float64), 1.0)
    with pytest.raises(ValueError, match="float32"):
        LF.add_noise_np(v[0], 1.0)
    for noise in (v, (v,), (v, None), (v, v[:2]), (v, v.astype(np.float64))):
        with pytest.raises(ValueError, match="noise"):
            LF.add_noise_np(v, 1.0, noise=noise)
    with pytest.raises(ValueError, match="odd"):
        LF.simulate_lowfield_np(np.zeros((4, 5, 4), dtype=np.float32))
    for count in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="count"):
            LF.hashed_words_np(0, count)
    for call in (lambda: LF.add_noise(torch.zeros((4, 4, 4)), 1.0), lambda: LF.simulate_lowfield(torch.zeros((4, 4, 4))),
                 lambda: LF.sigma_for_snr(torch.zeros((4, 4, 4)), 10.0)):
        with pytest.raises(ValueError, match="CUDA tensor"):
            call()


def test_the_entry_is_declared_registered_and_built():
    from mri_superresolution_amd import _lib, build
    name = "mrisr_f32_volume_add_noise"
    header = open(os.path.join(REPO, "include", "mrisr.h")).read()
    lib = _lib.load()
    assert name in _lib.SIGNATURES and hasattr(lib, name) and f"int {name}(" in header
    assert "#define MRISR_NOISE_RICIAN 0" in header and "#define MRISR_NOISE_GAUSSIAN 1" in header
    assert (LF.MODE_RICIAN, LF.MODE_GAUSSIAN) == (0, 1)
    assert lib.mrisr_version() == _lib.ABI_VERSION >= 334
    assert "volume_noise.hip" in build.SOURCES and build.FILE_FLAGS["volume_noise.hip"] == ["-ffp-contract=off"]
    import re
    declared = set(re.findall(r"\b(mrisr_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib.SIGNATURES) and all(hasattr(lib, n) for n in declared)
    # the refusals of the entry need no GPU: no launch happens
    fn = getattr(lib, name)
    R, G = 0, 1
    assert fn(None, 4, 4, 4, R, 1.0, 0, 16, None, None, 4096, None) == -1
    assert fn(16, 4, 4, 4, R, 1.0, 0, 16, None, None, None, None) == -1
    assert fn(16, 4, 4, 4, R, 1.0, 0, None, None, None, 4096, None) == -1               # the generator needs its table
    assert fn(18, 4, 4, 4, R, 1.0, 0, 16, None, None, 4096, None) == -1                 # misaligned
    assert fn(16, 4, 4, 4, R, 1.0, 0, 16, None, None, 4098, None) == -1
    assert fn(16, 4, 4, 4, R, 1.0, 0, 18, None, None, 4096, None) == -1
    assert fn(16, 4, 4, 4, R, 1.0, 0, 16, 8192, 8194, 4096, None) == -1
    assert fn(16, 4, 4, 4, R, 1.0, 0, 16, 8192, None, 4096, None) == -1                 # one plane without the other
    assert fn(16, 4, 4, 4, G, 1.0, 0, 16, None, 8192, 4096, None) == -1
    assert fn(16, 4, 4, 4, 2, 1.0, 0, 16, None, None, 4096, None) == -1 and fn(16, 4, 4, 4, -1, 1.0, 0, 16, None, None, 4096, None) == -1
    for sigma in (-1.0, float("nan"), float("inf")):
        assert fn(16, 4, 4, 4, R, sigma, 0, 16, None, None, 4096, None) == -1
    assert fn(16, 4, 4, 4, R, 1.0, 0, 8192, None, None, 16 + 4 * 63, None) == -1         # overlapping without being equal
    assert fn(4096, 4, 4, 4, R, 1.0, 0, 8192, None, None, 4096 - 4 * 63, None) == -1
    assert fn(16, 4, 4, 4, R, 1.0, 0, None, 8192, 4096 + 4 * 63, 4096, None) == -1       # a plane overlapping dst
    assert fn(16, 0, 4, 4, R, 1.0, 0, 16, None, None, 4096, None) == -2 and fn(16, 4, 4, 32768, R, 1.0, 0, 16, None, None, 4096, None) == -2
    assert fn(16, 2048, 1024, 1024, R, 1.0, 0, 8, None, None, 1 << 40, None) == -2       # 2^31 voxels: one too many
    assert b"2^31" in lib.mrisr_last_error()
