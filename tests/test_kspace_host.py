"""Zero-filled x2 interpolation and k-space truncation (no GPU): the tables, the numpy specifications ``zerofill2_np`` / ``truncate2_np``
against an independent float64 FFT formulation, band-limited round trips, constants and refusals.

The bound on a float32 result is derived here, never measured: a pass over a line of ``m`` source samples computes, per output,
``sum_j t_j v_j`` with float32 table entries (one rounding each), float32 products (one each) and ``m`` float32 sums, so its error is
at most ``(m + 2) 2^-24 sum_j |t_j| |v_j|`` (the standard dot-product bound plus the table's rounding); what the input of a pass is
already off by goes through the pass as ``sum_j |t_j| e_j``.  Both are accumulated over the passes, per element."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd import volume_kspace as K      # noqa: E402

EXTENTS = (1, 2, 3, 8, 9, 31, 64)
EPS = 2.0 ** -24


# ---------------------------------------------------------------- the independent formulation: np.fft, float64

def fft_weights(n, window):
    """(n,) float64 in np.fft's order: w_|k| of the n-point grid, the Nyquist bin of an even n halved (it is split over +-n/2)."""
    k = np.abs(np.fft.fftfreq(n, 1.0 / n))
    w = np.ones(n) if window == "none" else 0.54 + 0.46 * np.cos(np.pi * k / ((n + 1) // 2))
    if n % 2 == 0:
        w[n // 2] *= 0.5
    return w


def zerofill_fft(v, axis, window):
    """One axis doubled: rfft-style zero padding of the spectrum with the ramp of the quarter-sample shift, in float64."""
    v = np.moveaxis(np.asarray(v, dtype=np.float64), axis, 0)
    n = v.shape[0]
    k = np.fft.fftfreq(n, 1.0 / n)                                   # signed integer frequencies
    tail = (slice(None),) + (None,) * (v.ndim - 1)
    spec = np.fft.fft(v, axis=0) * fft_weights(n, window)[tail]
    pad = np.zeros((2 * n,) + v.shape[1:], dtype=np.complex128)
    ramp = np.exp(-2j * np.pi * k * 0.25 / n)                        # output sample o sits at o / 2 - 1 / 4
    for b in range(n):
        pad[int(k[b]) % (2 * n)] += spec[b] * ramp[b]
        if n % 2 == 0 and b == n // 2:                               # the other half of the Nyquist bin, at +n/2
            pad[n // 2] += spec[b] * np.conj(ramp[b])
    out = np.fft.ifft(pad, axis=0) * 2.0
    assert np.abs(out.imag).max() <= 1e-9 * max(1.0, np.abs(out.real).max())
    return np.moveaxis(out.real, 0, axis)


def truncate_fft(v, axis, window):
    """One axis of even length N halved: the centre of the spectrum kept, coarse sample i at fine coordinate 2i + 1/2, in float64."""
    v = np.moveaxis(np.asarray(v, dtype=np.float64), axis, 0)
    N = v.shape[0]
    n = N // 2
    spec = np.fft.fft(v, axis=0)
    w = fft_weights(n, window)
    low = np.zeros((n,) + v.shape[1:], dtype=np.complex128)
    for k in range(-(n // 2), n // 2 + 1):                           # an even n: +n/2 and -n/2 both enter, each with half the weight
        low[k % n] += w[abs(k)] * spec[k % N] * np.exp(1j * np.pi * k / N)
    out = np.fft.ifft(low, axis=0) * (n / N)
    assert np.abs(out.imag).max() <= 1e-9 * max(1.0, np.abs(out.real).max())
    return np.moveaxis(out.real, 0, axis)


# ---------------------------------------------------------------- the derived bound

def matrix(mode, m, window):
    """The dense form of one pass over a line of m source samples, float64 of the float32 table (outputs x m)."""
    j = np.arange(m)
    if mode == "up":
        t = K.zerofill_table(m, window).astype(np.float64)
        mat = np.empty((2 * m, m))
        for i in range(m):
            mat[2 * i] = t[0][(i - j) % m]
            mat[2 * i + 1] = t[1][(i - j) % m]
        return mat
    t = K.truncate_table(m, window).astype(np.float64)
    return np.stack([t[(2 * i - j) % m] for i in range(m // 2)])


def along(mat, v, axis):
    return np.moveaxis(np.tensordot(mat, np.moveaxis(v, axis, 0), axes=(1, 0)), 0, axis)


def chain(mode, v32, axes, window, start=None):
    """-> (float32 result of the specification, float64 result of the FFT formulation, per-element bound on their difference).
    ``start``: what the float32 input is already off by (None: nothing) and the float64 input it stands for."""
    spec, exact = v32, (np.asarray(v32, dtype=np.float64) if start is None else start[1])
    bound = np.zeros(v32.shape) if start is None else start[0]
    for a in sorted(axes):
        m = spec.shape[a]
        mat = np.abs(matrix(mode, m, window))
        bound = along(mat, bound, a) + (m + 2) * EPS * along(mat, np.abs(spec).astype(np.float64), a)
        spec = (K.zerofill2_np if mode == "up" else K.truncate2_np)(spec, (a,), window)
        exact = (zerofill_fft if mode == "up" else truncate_fft)(exact, a, window)
    return spec, exact, bound


def values(shape, seed):
    return np.random.default_rng(seed).uniform(-3.0, 3.0, shape).astype(np.float32)


# ---------------------------------------------------------------- tables

@pytest.mark.parametrize("window", K.WINDOWS)
def test_tables_mirror_sum_and_smallest_sizes(window):
    for n in (1, 2, 3, 4, 7, 8, 9, 31, 64, 255, 512):
        t = K.zerofill_table(n, window, np.float64)
        assert t.shape == (2, n) and t.dtype == np.float64
        assert np.array_equal(t[0], t[1][(-np.arange(n)) % n]), n            # D_0[d] == D_1[(-d) mod n], before rounding
        assert np.abs(t.sum(axis=1) - 1.0).max() <= 8 * n * 2.0 ** -52, n
        t32 = K.zerofill_table(n, window)
        assert t32.dtype == np.float32 and np.array_equal(t32, t.astype(np.float32))
    for N in (2, 4, 6, 16, 18, 62, 128, 1024):
        t = K.truncate_table(N, window, np.float64)
        assert t.shape == (N,) and abs(t.sum() - 1.0) <= 8 * N * 2.0 ** -52, N
        assert np.array_equal(t, t[(-1 - np.arange(N)) % N])                 # symmetric about d = -1/2
        assert np.array_equal(K.truncate_table(N, window), t.astype(np.float32))
    assert K.zerofill_table(1, window).tolist() == [[1.0], [1.0]]
    assert K.truncate_table(2, "none").tolist() == [0.5, 0.5]


def test_table_entries_are_the_stated_cosine_sums():
    for n, window in ((5, "none"), (8, "hamming"), (9, "hamming")):
        ck = K.kspace_weights(n, window)
        k = np.arange(n // 2 + 1)
        assert ck[0] == 1.0 and (n % 2 or ck[-1] == (1.0 if window == "none" else 0.54 + 0.46 * np.cos(np.pi)))
        for s in (0, 1):
            want = [(ck * np.cos(2 * np.pi * k * (d - 0.25 + 0.5 * s) / n)).sum() / n for d in range(n)]
            assert np.allclose(K.zerofill_table(n, window, np.float64)[s], want, rtol=0, atol=1e-14)
        N = 2 * n
        want = [(ck * np.cos(2 * np.pi * k * (d + 0.5) / N)).sum() / N for d in range(N)]
        assert np.allclose(K.truncate_table(N, window, np.float64), want, rtol=0, atol=1e-14)


# ---------------------------------------------------------------- against the FFT formulation

def shapes_for(e):
    """Each axis alone on a small volume, and all three on the cube."""
    return [((e, 3, 2), (0,)), ((2, e, 3), (1,)), ((3, 2, e), (2,)), ((e, e, e), (0, 1, 2))]


@pytest.mark.parametrize("window", K.WINDOWS)
@pytest.mark.parametrize("e", EXTENTS)
def test_zerofill_agrees_with_the_fft_formulation(e, window):
    for shape, axes in shapes_for(e):
        spec, exact, bound = chain("up", values(shape, e + len(axes)), axes, window)
        assert spec.dtype == np.float32 and spec.shape == tuple(2 * d if a in axes else d for a, d in enumerate(shape))
        assert np.array_equal(spec, K.zerofill2_np(values(shape, e + len(axes)), axes, window))      # pass by pass == in one call
        off = np.abs(spec - exact)
        assert (off <= bound + 1e-12).all(), (shape, axes, float(off.max()), float(bound.max()))


@pytest.mark.parametrize("window", K.WINDOWS)
@pytest.mark.parametrize("e", EXTENTS)
def test_truncate_agrees_with_the_fft_formulation(e, window):
    for shape, axes in shapes_for(e):
        shape = tuple(2 * d if a in axes else d for a, d in enumerate(shape))      # lines of N = 2 e samples become e
        spec, exact, bound = chain("down", values(shape, e + len(axes)), axes, window)
        assert spec.dtype == np.float32 and spec.shape == tuple(d // 2 if a in axes else d for a, d in enumerate(shape))
        assert np.array_equal(spec, K.truncate2_np(values(shape, e + len(axes)), axes, window))
        off = np.abs(spec - exact)
        assert (off <= bound + 1e-12).all(), (shape, axes, float(off.max()), float(bound.max()))


def test_the_two_formulations_are_not_vacuous():
    """The bound is far below the signal, and a shifted grid is far outside it."""
    v = values((31, 3, 2), 5)
    spec, exact, bound = chain("up", v, (0,), "none")
    assert bound.max() < 1e-4 and np.abs(exact).max() > 1
    assert np.abs(spec[1:] - exact[:-1]).max() > 0.1


# ---------------------------------------------------------------- round trips, constants, refusals

def band_limited(shape, seed):
    """A sum of cosines with k < n / 2 per axis (n = half the extent), sampled on the fine grid, as float64."""
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in shape), indexing="ij")
    x = np.full(shape, 0.25)
    for _ in range(6):
        term = np.full(shape, rng.uniform(0.2, 1.0))
        for g, d in zip(grids, shape):
            top = (d // 2 - 1) // 2                                  # the largest k with k < n / 2
            term = term * np.cos(2 * np.pi * rng.integers(0, top + 1) * (g + rng.uniform(0, d)) / d)
        x = x + term
    return x


@pytest.mark.parametrize("window", ["none"])
@pytest.mark.parametrize("shape", [(16, 18, 10), (6, 62, 4)], ids=str)
def test_band_limited_volume_survives_truncation_and_zero_filling(shape, window):
    x64 = band_limited(shape, sum(shape))
    x32 = x64.astype(np.float32)
    low, low64, bound = chain("down", x32, (0, 1, 2), window, start=(np.abs(x32 - x64), x64))
    back, back64, bound = chain("up", low, (0, 1, 2), window, start=(bound, low64))
    assert np.abs(back64 - x64).max() < 1e-12                        # the formulation itself: exact for a band-limited input
    off = np.abs(back - x64)
    assert (off <= bound + 1e-12).all() and bound.max() < 1e-3, (float(off.max()), float(bound.max()))


@pytest.mark.parametrize("window", ["none"])
@pytest.mark.parametrize("shape", [(3, 9, 31), (1, 5, 7)], ids=str)
def test_zero_filling_then_truncation_is_the_identity_for_odd_extents(shape, window):
    y = values(shape, sum(shape))
    up, up64, bound = chain("up", y, (0, 1, 2), window)
    back, back64, bound = chain("down", up, (0, 1, 2), window, start=(bound, up64))
    assert np.abs(back64 - y).max() < 1e-12
    off = np.abs(back.astype(np.float64) - y)
    assert (off <= bound + 1e-12).all() and bound.max() < 1e-3, (float(off.max()), float(bound.max()))


@pytest.mark.parametrize("window", K.WINDOWS)
def test_a_constant_volume_stays_constant(window):
    for c in (1.5, -1000.25, 3e-5):
        c32 = np.float32(c)
        ulp = float(np.spacing(np.abs(c32)))
        for shape, axes in (((9, 3, 2), (0,)), ((2, 64, 3), (1,)), ((3, 2, 31), (2,)), ((8, 9, 31), (0, 1, 2))):
            up = K.zerofill2_np(np.full(shape, c32), axes, window)
            assert np.abs(up.astype(np.float64) - float(c32)).max() <= ulp * sum(shape[a] for a in axes)
            fine = tuple(2 * d if a in axes else d for a, d in enumerate(shape))
            down = K.truncate2_np(np.full(fine, c32), axes, window)
            assert down.shape == shape and np.abs(down.astype(np.float64) - float(c32)).max() <= ulp * sum(fine[a] for a in axes)


def test_refusals():
    v = np.zeros((4, 6, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="extent 3 of axis 2 is odd"):
        K.truncate2_np(v)
    assert K.truncate2_np(v, (0, 1)).shape == (2, 3, 3)
    for fn in (K.zerofill2_np, K.truncate2_np):
        with pytest.raises(ValueError, match="window"):
            fn(v, (0,), "hann")
        with pytest.raises(ValueError, match="axes"):
            fn(v, (0, 0))
        with pytest.raises(ValueError, match="float32"):
            fn(v.astype(np.float64), (0,))
    with pytest.raises(ValueError, match="window"):
        K.zerofill_table(8, "hann")
    with pytest.raises(ValueError):
        K.zerofill_table(513)
    with pytest.raises(ValueError, match="odd"):
        K.truncate_table(9)
    with pytest.raises(ValueError):
        K.truncate_table(1026)
    with pytest.raises(ValueError):
        K.zerofill2_np(np.zeros((513, 1, 1), dtype=np.float32), (0,))


def test_the_entry_is_declared_registered_and_built():
    from mri_superresolution_amd import _lib, build
    name = "mrisr_f32_volume_line_circulant"
    header = open(os.path.join(REPO, "include", "mrisr.h")).read()
    lib = _lib.load()
    assert name in _lib.SIGNATURES and hasattr(lib, name) and f"int {name}(" in header
    assert lib.mrisr_version() == _lib.ABI_VERSION >= 332
    assert "volume_kspace.hip" in build.SOURCES and build.FILE_FLAGS["volume_kspace.hip"] == ["-ffp-contract=off"]
    assert (K.MODE_UP2, K.MODE_DOWN2) == (0, 1) and "#define MRISR_CIRCULANT_DOWN2 1" in header
    # the refusals of the entry need no GPU: no launch happens
    fn = getattr(lib, name)
    assert fn(None, 2, 2, 2, 0, 0, None, None, None) == -1
    assert fn(16, 2, 2, 2, 3, 0, 16, 32, None) == -1 and fn(16, 2, 2, 2, 0, 2, 16, 32, None) == -1
    assert fn(16, 2, 2, 2, 0, 0, 16, 16, None) == -1                          # src == dst
    assert fn(16, 513, 1, 1, 0, 0, 16, 32, None) == -2 and fn(16, 1, 1, 1026, 2, 1, 16, 32, None) == -2
    assert fn(16, 2, 3, 2, 1, 1, 16, 32, None) == -2                          # an odd line cannot be halved
    assert fn(16, 0, 2, 2, 0, 0, 16, 32, None) == -2
