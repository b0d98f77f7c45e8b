"""What an MR scanner does to resolution, in three dimensions (extension): zero-filled x2 interpolation and
k-space truncation, both as one dense circulant transform along one axis of a volume at a time.

``zerofill2``        doubles the chosen axes by padding k-space with zeros: periodic sinc (Dirichlet-kernel) interpolation onto the
                     project's half-pixel-centred x2 grid - output sample ``2i + s`` at source coordinate ``i - 0.25 + 0.5 s``, the
                     geometry of ``volume_eval.upscale2``, the U-Net and ``nifti.header_for_grid``.  The interpolation every vendor's
                     "interpolated matrix" is, and the baseline ``volume_eval.evaluate_volume(zerofill=...)`` adds.
``truncate2``        halves the chosen axes (even extents) by keeping the centre of k-space: the degradation of the 2-D training
                     path (``csrc/lowfield.hip``), here for volumes; ``evaluate_volume(degrade="kspace")`` makes its low-resolution
                     volume with it.
``zerofill_table``   the two rows ``D_0``, ``D_1`` of the doubling, ``truncate_table`` the one row ``T`` of the halving: float64 on the
                     host, rounded once to float32 - the only place a cosine is evaluated.  The device path uploads the same arrays.

Both borders are PERIODIC, as in k-space: a line's last samples bleed into its first (the interpolation baselines of
``volume_eval`` replicate the border instead).  Nothing is clipped: the ringing of a sharp edge may go below zero, as the ``cubic``
baseline's does.  There is no FFT, no plan and no workspace, so any extent is served: a line of ``n`` samples costs ``O(n)`` per
output (``csrc/volume_kspace.hip``).

The arithmetic is fixed: an output is ``0 + t_0 v[0] + t_1 v[1] + ...`` over the source index ``j`` ascending, every product and every
sum rounded to float32, no fma.  ``zerofill2_np`` and ``truncate2_np`` state it in numpy; the kernels are bit-equal to them.  There is
no CPU path for tensors: CPU tensors raise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._volume_args import check_shape, cuda_tensor, volume_np

WINDOWS = ("none", "hamming")
MAX_UP = 512          # the longest line zerofill2 doubles
MAX_DOWN = 1024       # the longest line truncate2 halves: the device path stages whole lines in LDS
MODE_UP2, MODE_DOWN2 = 0, 1      # MRISR_CIRCULANT_*: mode of mrisr_f32_volume_line_circulant


def _axes(axes) -> tuple:
    axes = tuple(axes)
    if not axes or len(set(axes)) != len(axes) or any(a not in (0, 1, 2) for a in axes):
        raise ValueError(f"axes must be a non-empty selection of 0, 1, 2 without repeats, got {axes}")
    return tuple(sorted(int(a) for a in axes))


def _check_window(window) -> str:
    if window not in WINDOWS:
        raise ValueError(f"window is 'none' or 'hamming', got {window!r}")
    return window


# ---------------------------------------------------------------- tables

def kspace_weights(n: int, window: str = "none") -> np.ndarray:
    """``c_k w_k`` for ``k = 0 .. n // 2`` of the ``n``-point grid, float64: ``c_0 = 1``, ``c_k = 2`` below Nyquist, ``c_{n/2} = 1``
    for even ``n`` (the Nyquist term is kept once, symmetrically); ``w_k = 0.54 + 0.46 cos(pi k / ceil(n / 2))`` for ``"hamming"``,
    1 for ``"none"``."""
    _check_window(window)
    k = np.arange(n // 2 + 1, dtype=np.float64)
    c = np.where(k == 0, 1.0, 2.0)
    if n % 2 == 0 and n > 0:
        c[n // 2] = 1.0
    if window == "hamming":
        c = c * (0.54 + 0.46 * np.cos(np.pi * k / ((n + 1) // 2)))
    return c


def _rows(n_grid, period, quarters, window, dtype, parts=4):
    """row[d] = (1 / period) sum_k c_k w_k cos(2 pi k (d + q / 4) / period) for every ``q`` of ``quarters``, the sum over ``k`` ascending
    in float64.  The phase ``k (4 d + q)`` is reduced modulo ``4 period`` in integers and folded onto the half circle before the
    cosine is taken, so mirrored entries - ``D_0[d]`` and ``D_1[-d]`` - are the same float64.  ``parts``: the offsets are ``q / parts``
    of a sample instead of quarters (``volume_unring.shift_table``)."""
    ck = kspace_weights(n_grid, window)
    d = np.arange(period, dtype=np.int64)
    full = parts * period
    rows = np.zeros((len(quarters), period), dtype=np.float64)
    for r, q in enumerate(quarters):
        for k, c in enumerate(ck):
            m = (k * (parts * d + q)) % full
            m = np.minimum(m, full - m)
            rows[r] += c * np.cos((2.0 * np.pi / full) * m.astype(np.float64))
    rows /= period
    return rows.astype(dtype)                                    # float32: rounded once


def zerofill_table(n: int, window: str = "none", dtype=np.float32) -> np.ndarray:
    """(2, n): ``D_s[d] = (1/n) sum_k c_k w_k cos(2 pi k (d - 0.25 + 0.5 s) / n)`` over ``k = 0 .. n // 2`` (``kspace_weights``),
    computed in float64 and rounded once to ``dtype``.  ``n`` in 1..512."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= MAX_UP:
        raise ValueError(f"zerofill_table: a line of {n!r} samples (1..{MAX_UP})")
    return _rows(int(n), int(n), (-1, 1), window, dtype)


def truncate_table(N: int, window: str = "none", dtype=np.float32) -> np.ndarray:
    """(N,): ``T[d] = (1/N) sum_k c_k w_k cos(2 pi k (d + 0.5) / N)`` over ``k = 0 .. n // 2`` with the weights of the ``n = N / 2``
    point grid, computed in float64 and rounded once to ``dtype``.  ``N`` even, in 2..1024."""
    if isinstance(N, bool) or not isinstance(N, (int, np.integer)) or not 1 <= N <= MAX_DOWN:
        raise ValueError(f"truncate_table: a line of {N!r} samples (2..{MAX_DOWN}, even)")
    if N % 2:
        raise ValueError(f"extent {N} is odd")
    return _rows(int(N) // 2, int(N), (2,), window, dtype)[0]


# ---------------------------------------------------------------- numpy specifications

def _circulant_np(m: np.ndarray, row: np.ndarray, step: int, count: int) -> np.ndarray:
    """``out[i] = sum_j row[(step i - j) mod len(row)] m[j]`` for ``i < count`` along axis 0: a loop over ``j`` ascending on whole
    float32 arrays, so every product and every sum is rounded to float32."""
    period = len(row)
    i = np.arange(count)
    tail = (1,) * (m.ndim - 1)
    out = np.zeros((count,) + m.shape[1:], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(period):
            out = out + row[(step * i - j) % period].reshape((count,) + tail) * m[j][None]
    return out


def zerofill2_np(v: np.ndarray, axes=(0, 1, 2), window: str = "none") -> np.ndarray:
    """Doubles ``axes`` in ascending order, each pass on the float32 result of the one before: along an axis of ``n`` samples (1..512)
    ``out[2i + s] = sum_j D_s[(i - j) mod n] v[j]`` with ``zerofill_table(n, window)``.  The border is periodic, as in k-space; values
    are not clipped."""
    v = volume_np(v, "zerofill2_np")
    _check_window(window)
    for a in _axes(axes):
        n = v.shape[a]
        table = zerofill_table(n, window)
        m = np.moveaxis(v, a, 0)
        u = np.empty((2 * n,) + m.shape[1:], dtype=np.float32)
        u[0::2] = _circulant_np(m, table[0], 1, n)
        u[1::2] = _circulant_np(m, table[1], 1, n)
        v = np.moveaxis(u, 0, a)
    return np.ascontiguousarray(v)


def truncate2_np(v: np.ndarray, axes=(0, 1, 2), window: str = "none") -> np.ndarray:
    """Halves ``axes`` in ascending order, each pass on the float32 result of the one before: along an axis of ``N = 2n`` samples
    (even, at most 1024) ``out[i] = sum_j T[(2i - j) mod N] v[j]`` with ``truncate_table(N, window)`` - the centre of k-space is
    kept.  The border is periodic.  An odd extent on one of the axes is a ``ValueError``."""
    v = volume_np(v, "truncate2_np")
    _check_window(window)
    axes = _axes(axes)
    for a in axes:
        if v.shape[a] % 2:
            raise ValueError(f"extent {v.shape[a]} of axis {a} is odd")
    for a in axes:
        N = v.shape[a]
        m = np.moveaxis(v, a, 0)
        v = np.moveaxis(_circulant_np(m, truncate_table(N, window), 2, N // 2), 0, a)
    return np.ascontiguousarray(v)


# ---------------------------------------------------------------- device

_TABLES = {}


def _table(mode, n, window, device) -> torch.Tensor:
    key = (mode, n, window, device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _TABLES:
        host = zerofill_table(n, window) if mode == MODE_UP2 else truncate_table(n, window)
        _TABLES[key] = torch.from_numpy(np.ascontiguousarray(host)).to(device)
    return _TABLES[key]


def _passes(vol, axes, window, out, mode, what):
    _check_window(window)
    axes = _axes(axes)
    v = cuda_tensor(vol, (torch.float32,), what, ndim=3, limit=True)
    up = mode == MODE_UP2
    shapes, shape = [], tuple(v.shape)
    for a in axes:
        if up and shape[a] > MAX_UP:
            raise ValueError(f"{what}: an axis of {shape[a]} voxels is longer than the limit of {MAX_UP}")
        if not up and shape[a] % 2:
            raise ValueError(f"extent {shape[a]} of axis {a} is odd")
        if not up and shape[a] > MAX_DOWN:
            raise ValueError(f"{what}: an axis of {shape[a]} voxels is longer than the limit of {MAX_DOWN}")
        shape = shape[:a] + (2 * shape[a] if up else shape[a] // 2,) + shape[a + 1:]
        check_shape(shape, f"{what}: the volume's shape")
        shapes.append(shape)
    if out is not None:
        cuda_tensor(out, (torch.float32,), what, name="out", shape=shapes[-1])
        if out.device != v.device or out.data_ptr() == v.data_ptr():
            raise ValueError(f"{what}: out must be another contiguous float32 tensor of shape {shapes[-1]} on {v.device}")
    # every table is on the device before the first launch: nothing is uploaded between two launches of one call
    tables = [_table(mode, (s[a] // 2) if up else 2 * s[a], window, v.device) for a, s in zip(axes, shapes)]
    for k, (a, s) in enumerate(zip(axes, shapes)):
        dst = out if out is not None and k == len(axes) - 1 else torch.empty(s, dtype=torch.float32, device=v.device)
        L.call("mrisr_f32_volume_line_circulant", v.data_ptr(), *v.shape, a, mode, tables[k].data_ptr(), dst.data_ptr(), L.stream_ptr(),
               nbytes=4 * (v.numel() + dst.numel()))
        v = dst
    return v


def zerofill2(vol: torch.Tensor, axes=(0, 1, 2), window: str = "none", out: torch.Tensor = None) -> torch.Tensor:
    """vol: (X,Y,Z) float32 CUDA tensor -> the volume with ``axes`` doubled by zero-filling k-space, bit-equal to ``zerofill2_np``.
    One launch per axis, no device-to-host read: HIP-graph capturable once the tables of its extents are cached (a first call
    outside the capture uploads them).  ``out``: the result goes to this tensor of the doubled shape (not ``vol``)."""
    return _passes(vol, axes, window, out, MODE_UP2, "zerofill2")


def truncate2(vol: torch.Tensor, axes=(0, 1, 2), window: str = "none", out: torch.Tensor = None) -> torch.Tensor:
    """vol: (X,Y,Z) float32 CUDA tensor with even extents on ``axes`` -> the volume with them halved by truncating k-space,
    bit-equal to ``truncate2_np``.  Launches, capture and ``out`` as ``zerofill2``."""
    return _passes(vol, axes, window, out, MODE_DOWN2, "truncate2")
