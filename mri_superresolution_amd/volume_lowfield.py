"""The low-field degradation of a volume (extension): k-space truncation (``volume_kspace.truncate2``) followed
by seeded complex Gaussian noise and the magnitude - Rician noise, the defining property of low-field MR - with a generator that
numpy restates bit for bit.

``add_noise``            ``re = v + sigma z1``, ``im = sigma z2``, ``out = sqrt(re re + im im)`` (``rician``) or ``re`` (Gaussian), per
                         voxel; ``z1, z2`` the two standard normals of the voxel's C-order index under ``seed``.  One launch
                         (``csrc/volume_noise.hip``), bit-equal to ``add_noise_np``, the same bits on every run, no host read,
                         HIP-graph capturable.  ``noise=(n_re, n_im)``: a replayed draw, ``re = v + n_re``, ``im = n_im``.
``simulate_lowfield``    ``truncate2`` over ``axes``, then ``add_noise``: a simulated low-field acquisition of a high-resolution volume.
``sigma_for_snr``        the sigma that gives a foreground signal-to-noise ratio: the median of the Otsu foreground over ``snr``.
``frame_seeds``          the seeds of the frames of 4-D scans: ``utils.lowfield.derive_seeds`` of (seed, scan index, frame index), so no
                         frame shares a draw with another.

The generator.  ``key = noise_key(seed)``; voxel ``i`` draws the words ``h1 = mix32(key ^ mix32(2i + 1))`` and ``h2 = mix32(key +
0x9e3779b9 + mix32(2i))`` - the hash of the 2-D path (``csrc/common.h``), all 32 bits of each used.  A word ``h`` becomes a standard
normal by a piecewise-linear inverse CDF on a hierarchical grid: the sign is bit 31, ``m = h & 0x7fffffff`` stands for the tail
probability ``p = (m + 0.5) / 2^32``.  The grid has one octave per position ``top`` of ``m``'s leading one, each cut into
``2^min(S, top)`` equal segments, and ``m = 0`` is a segment of its own: with ``S = 6``, 1664 segments and 1665 knots.  ``T[k] =
float32(-Phi^-1(p at knot k))`` comes from ``statistics.NormalDist().inv_cdf`` in float64 and is rounded once; ``D[k] = T[k + 1] -
T[k]`` is a float32 difference.  With ``shift = max(bit_length(m) - 1 - S, 0)`` the segment is ``k = base[bit_length(m)] + (m >>
shift)`` and the position inside it ``f = (m mod 2^shift) / 2^shift`` - at most 24 bits times a power of two, exact in float32 - and
``|z| = T[k] + f D[k]``, one rounded product and one rounded sum.  No logarithm, cosine or exponential is evaluated anywhere, which
is what makes the device equal to numpy (the 2-D path's Box-Muller through ``__logf`` / ``__cosf`` is not).  ``base[t] = 64 max(t -
7, 0)``; the kernel uses that closed form, the specification the array.  The largest deviation of ``|z|`` from the exact float64
quantile of ``p`` is 1.3e-5 (measured over 2^22 words); the largest ``|z|`` is ``T[0]`` = 6.338.

Every operation of ``add_noise_np`` is one float32 operation.  NaN and Inf go through the arithmetic; ``sigma = 0`` is no special
case (Rician: ``sqrt(v v)``).  There is no CPU path for tensors: CPU tensors raise.
"""
from __future__ import annotations

import functools
import logging
import math
from statistics import NormalDist

import numpy as np
import torch

from . import _lib as L
from ._volume_args import MAX_VOXELS, cuda_tensor, volume_np
from .volume_kspace import truncate2, truncate2_np

logger = logging.getLogger(__name__)

S = 6                      # an octave has at most 2^S segments
KNOTS = 1665               # 1 + (2^S - 1) + (31 - S) 2^S + 1
MODE_RICIAN, MODE_GAUSSIAN = 0, 1      # MRISR_NOISE_*: mode of mrisr_f32_volume_add_noise
_M32, _M64 = 0xffffffff, (1 << 64) - 1
_GOLDEN = 0x9e3779b9


# ---------------------------------------------------------------- the table

def knot_positions() -> np.ndarray:
    """int64[KNOTS]: the values of ``m`` at which the segments begin, ascending, and ``2^31`` for the last knot."""
    a = [0]
    for top in range(31):
        cut = min(S, top)
        a += [(1 << top) + (s << (top - cut)) for s in range(1 << cut)]
    return np.array(a + [1 << 31], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _normal_table():
    inv = NormalDist().inv_cdf
    T = np.array([-inv((int(a) + 0.5) / 4294967296.0) for a in knot_positions()], dtype=np.float64).astype(np.float32)     # rounded once
    D = (T[1:] - T[:-1]).astype(np.float32)
    # octave top = t - 1 begins at segment 1 + sum_{u < top} 2^min(S, u); m >> shift runs from 2^min(S, top) there
    base = np.array([0] + [1 + sum(1 << min(S, u) for u in range(t - 1)) - (1 << min(S, t - 1)) for t in range(1, 32)], dtype=np.int64)
    for a in (T, D, base):
        a.setflags(write=False)
    return T, D, base


def normal_table():
    """-> ``(T float32[1665], D float32[1664], base int64[32])`` of the module docstring, read-only; ``base`` is indexed by
    ``bit_length(m)`` (0 for ``m = 0``).  The specification and the device path use these same arrays."""
    return _normal_table()


def device_table() -> np.ndarray:
    """float32[2 * KNOTS]: ``T``, then ``D`` with one 0 appended - what ``mrisr_f32_volume_add_noise`` takes as ``table``."""
    T, D, _ = normal_table()
    return np.concatenate([T, D, np.zeros(1, dtype=np.float32)])


def segment_index(m):
    """``m``: integers in 0 .. 2^31 - 1 -> ``(k, shift)``: the segment of the grid and the number of bits of ``m`` below it."""
    m = np.asarray(m, dtype=np.int64)
    length = np.zeros(m.shape, dtype=np.int64)           # bit_length
    for b in (16, 8, 4, 2, 1):
        big = (m >> (length + b)) != 0
        length = np.where(big, length + b, length)
    length = np.where(m != 0, length + 1, 0)
    shift = np.maximum(length - 1 - S, 0)
    return normal_table()[2][length] + (m >> shift), shift


# ---------------------------------------------------------------- the generator in numpy

def _mix32_np(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def _seed64(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"the seed is an integer (its low 64 bits are used), got {seed!r}")
    return int(seed) & _M64


def noise_key_np(seed) -> np.uint32:
    """``noise_key`` of ``csrc/common.h``: the 32-bit generator key of a 64-bit seed."""
    s = _seed64(seed)
    lo, hi = np.array([s & _M32], dtype=np.uint32), np.array([s >> 32], dtype=np.uint32)
    return _mix32_np(lo ^ _mix32_np(hi + np.uint32(_GOLDEN)))[0]


def hashed_words_np(seed, count, start=0):
    """-> ``(h1, h2)``, uint32[count]: the two words of the voxels ``start .. start + count - 1`` (indices below 2^31 - 1)."""
    if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or count < 1 or start < 0 or start + count > MAX_VOXELS:
        raise ValueError(f"hashed_words_np: the voxels {start} .. {start} + {count!r} - 1 (a count of at least 1, indices below 2^31 - 1)")
    key = noise_key_np(seed)
    i = np.arange(start, start + count, dtype=np.int64).astype(np.uint32)
    two = i * np.uint32(2)
    h1 = _mix32_np(key ^ _mix32_np(two + np.uint32(1)))
    h2 = _mix32_np(np.uint32((int(key) + _GOLDEN) & _M32) + _mix32_np(two))      # the sums wrap at 32 bits
    return h1, h2


def normal_from_words_np(h) -> np.ndarray:
    """uint32 words -> float32 standard normals: the table's interpolation, operation by operation."""
    h = np.asarray(h, dtype=np.uint32)
    T, D, _ = normal_table()
    m = (h & np.uint32(0x7fffffff)).astype(np.int64)
    k, shift = segment_index(m)
    f = np.ldexp((m & ((np.int64(1) << shift) - 1)).astype(np.float32), -shift.astype(np.int32)).astype(np.float32)      # exact
    a = (T[k] + (f * D[k]).astype(np.float32)).astype(np.float32)
    return (a.view(np.uint32) ^ (h & np.uint32(0x80000000))).view(np.float32)


def hashed_normals_np(seed, count, start=0):
    """-> ``(z1, z2)``, float32[count]: the two standard normals of the voxels ``start .. start + count - 1``."""
    h1, h2 = hashed_words_np(seed, count, start)
    return normal_from_words_np(h1), normal_from_words_np(h2)


# ---------------------------------------------------------------- numpy specifications

def _check_sigma(sigma, what) -> np.float32:
    try:
        with np.errstate(over="ignore"):
            s = np.float32(sigma)
    except (TypeError, ValueError):
        s = np.float32("nan")
    if isinstance(sigma, bool) or not (np.isfinite(s) and s >= 0):
        raise ValueError(f"{what}: sigma must be finite and not negative (float32), got {sigma!r}")
    return s


def add_noise_np(v, sigma, seed=0, noise=None, rician=True) -> np.ndarray:
    """The specification: ``v`` float32 (X, Y, Z) -> the noisy float32 volume.  ``s = float32(sigma)``; per voxel of C-order index
    ``i``: ``re = v + s z1[i]``, ``im = s z2[i]`` (``hashed_normals_np(seed, v.size)``), ``out = sqrt(re re + im im)`` - or ``re`` with
    ``rician=False`` - every product, sum and the root one float32 operation.  ``noise = (n_re, n_im)``, float32 arrays of ``v``'s
    shape: ``re = v + n_re``, ``im = n_im``; ``sigma`` and ``seed`` are then not used."""
    v = np.ascontiguousarray(volume_np(v, "add_noise_np", limit=True))
    s = _check_sigma(sigma, "add_noise_np")
    with np.errstate(all="ignore"):
        if noise is not None:
            n_re, n_im = _noise_pair(noise, "add_noise_np")
            for n in (n_re, n_im):
                if np.asarray(n).dtype != np.float32 or np.shape(n) != v.shape:
                    raise ValueError(f"add_noise_np: the noise planes are float32 arrays of shape {v.shape}")
            re, im = v + np.asarray(n_re), np.asarray(n_im)
        else:
            z1, z2 = hashed_normals_np(seed, v.size)
            re, im = v + (s * z1).reshape(v.shape), (s * z2).reshape(v.shape)
        if not rician:
            return np.ascontiguousarray(re, dtype=np.float32)
        return np.sqrt(re * re + im * im).astype(np.float32)


def _noise_pair(noise, what):
    try:
        n_re, n_im = noise
    except (TypeError, ValueError):
        raise ValueError(f"{what}: noise is the pair (n_re, n_im)") from None
    if n_re is None or n_im is None:
        raise ValueError(f"{what}: noise is the pair (n_re, n_im), both given")
    return n_re, n_im


def simulate_lowfield_np(v, axes=(0, 1, 2), window="none", sigma=0.0, seed=0, truncate=True, rician=True) -> np.ndarray:
    """``add_noise_np(truncate2_np(v, axes, window), sigma, seed, rician=rician)``; ``truncate=False``: the noise alone."""
    v = volume_np(v, "simulate_lowfield_np")
    return add_noise_np(truncate2_np(v, axes, window) if truncate else v, sigma, seed, rician=rician)


def frame_seeds(seed, scan: int, frames: int) -> list:
    """The 64-bit seeds of the ``frames`` frames of scan number ``scan``: ``derive_seeds(seed, scan, range(frames))``."""
    from .utils.lowfield import derive_seeds
    return derive_seeds(_seed64(seed), int(scan), range(int(frames)))


# ---------------------------------------------------------------- device

_TABLES = {}


def _table(device) -> torch.Tensor:
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(device_table()).to(device)
    return _TABLES[key]


def add_noise(vol: torch.Tensor, sigma, seed=0, noise=None, rician=True, out: torch.Tensor = None) -> torch.Tensor:
    """vol: (X,Y,Z) float32 CUDA tensor -> the noisy volume, bit-equal to ``add_noise_np``.  One launch, no device-to-host read:
    HIP-graph capturable once the table is on the device (a first call outside the capture uploads it).  ``noise = (n_re, n_im)``:
    float32 CUDA volumes of ``vol``'s shape, the noise itself.  ``out``: the result goes to this tensor of ``vol``'s shape; it may be
    ``vol`` itself."""
    v = cuda_tensor(vol, (torch.float32,), "add_noise", ndim=3, limit=True)
    s = _check_sigma(sigma, "add_noise")
    seed = _seed64(seed)
    planes = (None, None)
    if noise is not None:
        planes = tuple(cuda_tensor(n, (torch.float32,), "add_noise", name="a noise plane", shape=v.shape) for n in _noise_pair(noise, "add_noise"))
    if out is None:
        out = torch.empty_like(v)
    else:
        cuda_tensor(out, (torch.float32,), "add_noise", name="out", shape=v.shape)
    if any(t.device != v.device for t in (out,) + tuple(p for p in planes if p is not None)):
        raise ValueError(f"add_noise: out and the noise planes must be on {v.device}")
    table = _table(v.device) if noise is None else None
    L.call("mrisr_f32_volume_add_noise", v.data_ptr(), *v.shape, MODE_RICIAN if rician else MODE_GAUSSIAN, float(s), seed, L.ptr(table),
           L.ptr(planes[0]), L.ptr(planes[1]), out.data_ptr(), L.stream_ptr(), nbytes=(8 if noise is None else 16) * v.numel())
    return out


def simulate_lowfield(vol: torch.Tensor, axes=(0, 1, 2), window="none", sigma=0.0, seed=0, truncate=True, rician=True) -> torch.Tensor:
    """vol: (X,Y,Z) float32 CUDA tensor, even extents on ``axes`` -> ``truncate2`` over ``axes``, then ``add_noise``: bit-equal to
    ``simulate_lowfield_np``.  ``truncate=False``: the noise alone, on a new tensor."""
    v = cuda_tensor(vol, (torch.float32,), "simulate_lowfield", ndim=3, limit=True)
    _check_sigma(sigma, "simulate_lowfield")
    if not truncate:
        return add_noise(v, sigma, seed, rician=rician)
    lr = truncate2(v, axes, window)
    return add_noise(lr, sigma, seed, rician=rician, out=lr)


def foreground_median(vol: torch.Tensor, mask=None, what="foreground_median"):
    """-> (median, count) of the foreground, as Python numbers: ``mask`` (uint8 or bool CUDA tensor) or the Otsu mask of ``vol``
    (``volume_eval.foreground_mask``); the median is ``volume_intensity.masked_percentiles``'s.  One device-to-host read."""
    from .volume_eval import foreground_mask
    from .volume_intensity import masked_percentiles
    v = cuda_tensor(vol, (torch.float32,), what, ndim=3)
    if mask is None:
        mask = foreground_mask(v)[0]
    median, count = masked_percentiles(v, mask, (50.0,))
    got = torch.cat([median.double(), count.double()]).cpu()
    return float(got[0]), int(got[1])


def sigma_for_snr(vol: torch.Tensor, snr, mask=None) -> float:
    """-> the sigma at which the median of the foreground is ``snr`` sigmas: ``foreground_median / snr``.  One device-to-host read;
    the result is logged."""
    v = cuda_tensor(vol, (torch.float32,), "sigma_for_snr", ndim=3)
    try:
        r = float(snr)
    except (TypeError, ValueError):
        r = float("nan")
    if isinstance(snr, bool) or not (math.isfinite(r) and r > 0):
        raise ValueError(f"sigma_for_snr: the signal-to-noise ratio must be finite and positive, got {snr!r}")
    median, count = foreground_median(v, mask, "sigma_for_snr")
    if count < 1 or not (math.isfinite(median) and median > 0):
        raise ValueError(f"sigma_for_snr: the foreground's median is {median!r} over {count} voxels: no signal to scale the noise to")
    sigma = median / r
    logger.info(f"sigma {sigma:.6g} = the foreground median {median:.6g} over {count} voxels / SNR {r:g}")
    return sigma
