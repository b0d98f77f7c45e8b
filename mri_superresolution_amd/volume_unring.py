"""Gibbs-ringing removal for volumes (extension): Kellner's local subvoxel shifts (Kellner et al., MRM 2016),
one axis at a time, fused in one kernel per axis (``csrc/volume_unring.hip``).

A truncated k-space rings at every sharp interface with a period of one voxel pair; where the samples fall on the ringing depends
on the sub-voxel position of the grid.  So a line is re-sampled at ``2K`` sub-voxel offsets by periodic sinc interpolation, at every
sample the offset whose neighbourhood oscillates least is taken - the measure is the total variation in a small one-sided window -
and the sample is interpolated back to its own position.

``shift_table``      the ``2K`` rows of the re-sampling, ``shift_fractions`` their offsets: float64 on the host, rounded once to
                     float32 - the only place a cosine is evaluated (``volume_kspace._rows``).  The device path uploads the same arrays.
``unring_axis``      the operator along one axis; ``unring_axis_np`` states it in numpy and the kernel is bit-equal to it.
``kspace_split``     for several axes: the volume as a sum of one part per axis, ``G_a = B_a / sum_b B_b`` with ``B_a = prod_{b != a}
                     (1 + cos(2 pi k_b / n_b))`` in k-space, so that the part unringed along ``a`` holds what is low along the other
                     axes (for two axes Kellner's ``G_x = A_y / (A_x + A_y)``).  The only FFT (``torch.fft``: plumbing).
``unring``           ``sum_a unring_axis(kspace_split(vol)[a], a)``.

The border is PERIODIC, as in k-space.  The arithmetic of ``unring_axis`` is fixed: every product, difference and sum is one float32
operation, no fma, in the order ``unring_axis_np`` states.  There is no CPU path for tensors: CPU tensors raise.

Not built: zero-filled or partial-Fourier input (its ringing period is not one voxel), lines above 512 samples, a 2-D form for
``scripts/evaluate.py``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._volume_args import check_shape, cuda_tensor, out_like, volume_np
from .volume_kspace import _axes, _rows

MIN_LINE, MAX_LINE = 8, 512       # the lines unring_axis takes: the device path keeps two tiles of whole lines in LDS
MAX_SHIFTS = 32                   # K: 2K candidates besides the line itself
MAX_WINDOW = 4                    # 1 <= a <= b <= 4
WEIGHTINGS = ("kspace", "none")


def _check_line(n, what) -> int:
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not MIN_LINE <= n <= MAX_LINE:
        raise ValueError(f"{what}: a line of {n!r} samples ({MIN_LINE}..{MAX_LINE})")
    return int(n)


def _check_shifts(K, what) -> int:
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= MAX_SHIFTS:
        raise ValueError(f"{what}: K = {K!r} shifts (an integer in 1..{MAX_SHIFTS})")
    return int(K)


def _check_window(window, what) -> tuple:
    try:
        a, b = window
        ok = all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in (a, b)) and 1 <= a <= b <= MAX_WINDOW
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: window is (a, b) with 1 <= a <= b <= {MAX_WINDOW}, got {window!r}")
    return int(a), int(b)


def _check_weighting(weighting, axes, what) -> str:
    if weighting not in WEIGHTINGS:
        raise ValueError(f"{what}: weighting is 'kspace' or 'none', got {weighting!r}")
    if weighting == "none" and len(axes) > 1:
        raise ValueError(f"{what}: weighting 'none' is for one axis; {len(axes)} axes need the k-space split")
    return weighting


# ---------------------------------------------------------------- tables

def shift_order(K: int) -> list:
    """The candidates' numerators ``m`` in table order: ``+1, -1, +2, -2, ... +K, -K``."""
    K = _check_shifts(K, "shift_order")
    return [sign * m for m in range(1, K + 1) for sign in (1, -1)]


def shift_table(n: int, K: int = 20, dtype=np.float32) -> np.ndarray:
    """(2K, n): ``S_m[d] = (1/n) sum_k c_k cos(2 pi k (d + m / (2K)) / n)`` over ``k = 0 .. n // 2`` (``kspace_weights(n)``) for ``m`` in
    ``shift_order(K)``, computed in float64 and rounded once to ``dtype``.  ``sum_j S_m[(i - j) mod n] v[j]`` is the line's periodic
    sinc interpolant at ``i + m / (2K)``.  ``S_m[d]`` and ``S_-m[(-d) mod n]`` are the same float64."""
    n = _check_line(n, "shift_table")
    return _rows(n, n, shift_order(K), "none", dtype, parts=2 * K)


def shift_fractions(K: int = 20) -> np.ndarray:
    """(2K,) float32: ``m / (2K)`` for ``m`` in ``shift_order(K)``, the quotient taken in float64 and rounded once."""
    return (np.asarray(shift_order(K), dtype=np.float64) / (2.0 * K)).astype(np.float32)


# ---------------------------------------------------------------- numpy specification, one axis

def shifted_lines_np(v: np.ndarray, axis: int, K: int = 20) -> np.ndarray:
    """(2K, n, ...) float32, the line axis first: candidate ``m`` of every line, ``f_m[i] = 0 + S_m[(i - 0) mod n] v[0] + S_m[(i - 1)
    mod n] v[1] + ...`` over ``j`` ascending on whole float32 arrays - the arithmetic of ``volume_kspace._circulant_np``."""
    v = volume_np(v, "shifted_lines_np")
    m = np.moveaxis(v, axis, 0)
    n = _check_line(m.shape[0], "shifted_lines_np")
    table = shift_table(n, K)
    i = np.arange(n)
    out = np.zeros((2 * K, n) + m.shape[1:], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            out = out + table[:, (i - j) % n].reshape((2 * K, n, 1, 1)) * m[j][None, None]
    return out


def select_np(v: np.ndarray, shifted: np.ndarray, axis: int, K: int = 20, window=(1, 3), return_best: bool = False):
    """Steps 2 to 4 of ``unring_axis_np`` on the candidates ``shifted = shifted_lines_np(v, axis, K)``.  ``return_best``: also the
    variation that won at every sample, as a second array."""
    v = volume_np(v, "select_np")
    a, b = _check_window(window, "select_np")
    fractions = shift_fractions(K)
    m = np.moveaxis(v, axis, 0)
    if shifted.dtype != np.float32 or shifted.shape != (2 * K,) + m.shape:
        raise ValueError(f"select_np: the candidates must be float32 {(2 * K,) + m.shape}, got {shifted.dtype} {shifted.shape}")

    def variations(f):
        d = np.abs(f - np.roll(f, -1, axis=0))                      # d[t] = |f[t] - f[t + 1]|
        tvl = np.zeros_like(f)
        tvr = np.zeros_like(f)
        for k in range(a, b + 1):
            tvl = tvl + np.roll(d, k + 1, axis=0)                   # |f[i - k] - f[i - k - 1]|
            tvr = tvr + np.roll(d, -k, axis=0)                      # |f[i + k] - f[i + k + 1]|
        return tvl, tvr

    with np.errstate(invalid="ignore", over="ignore"):
        best, tvr = variations(m)
        value = m.copy()
        best = np.where(tvr < best, tvr, best)                      # candidate 0 on the right: the same value
        for f, s in zip(shifted, fractions):
            if s > 0:
                cand = f - (f - np.roll(f, 1, axis=0)) * s
            else:
                cand = f + (f - np.roll(f, -1, axis=0)) * s
            for tv in variations(f):
                win = tv < best
                best = np.where(win, tv, best)
                value = np.where(win, cand, value)
    assert value.dtype == np.float32
    value = np.ascontiguousarray(np.moveaxis(value, 0, axis))
    return (value, np.ascontiguousarray(np.moveaxis(best, 0, axis))) if return_best else value


def unring_axis_np(v: np.ndarray, axis: int, K: int = 20, window=(1, 3)) -> np.ndarray:
    """The operator along ``axis`` (0..2) of a float32 volume, lines of 8..512 samples, the border periodic.  Every operation is one
    float32 operation.  Along a line ``v[0..n)``:

    1. candidate 0 is ``f = v``; candidate ``m`` (``shift_order(K)``) is ``f_m = shifted_lines_np`` with row ``m`` of ``shift_table``;
    2. ``TVL[i] = 0 + sum_{k=a..b} |f[i-k] - f[i-k-1]|``, ``TVR[i] = 0 + sum_{k=a..b} |f[i+k] - f[i+k+1]|``, ``k`` ascending, indices
       modulo ``n``, ``(a, b) = window``;
    3. the candidate's value at ``i`` with ``s = shift_fractions(K)[m]``: ``v[i]`` for candidate 0, ``f[i] - (f[i] - f[i-1]) s`` for
       ``s > 0``, ``f[i] + (f[i] - f[i+1]) s`` for ``s < 0``;
    4. ``best`` starts as candidate 0's ``TVL`` and the value as ``v[i]``; then candidate 0's ``TVR``, then ``TVL`` and ``TVR`` of every
       ``m`` in table order are visited, and a visit replaces ``(best, value)`` only if ``tv < best``: the first minimum wins, a NaN never.

    A line that is constant, or whose window is flat at offset zero, returns its input bits."""
    if axis not in (0, 1, 2):
        raise ValueError(f"unring_axis_np: axis is 0, 1 or 2, got {axis!r}")
    K = _check_shifts(K, "unring_axis_np")
    _check_window(window, "unring_axis_np")
    return select_np(v, shifted_lines_np(v, axis, K), axis, K, window)


# ---------------------------------------------------------------- the k-space split

def split_weights(shape, axes=(0, 1, 2)) -> np.ndarray:
    """(len(axes), X, Y, Z) float64 on the FFT frequencies (extent 1 on an axis outside ``axes``): ``G_a = B_a / sum_b B_b`` with
    ``A_a(k) = 1 + cos(2 pi k / n_a)`` and ``B_a = prod_{b != a} A_b``; ``1 / len(axes)`` where the sum is 0 (two axes at Nyquist)."""
    shape = check_shape(shape, "split_weights: the volume's shape")
    axes = _axes(axes)
    A = {}
    for a in axes:
        n = shape[a]
        k = np.arange(n, dtype=np.int64)
        cos = np.cos(2.0 * np.pi * (k.astype(np.float64) / n))
        cos[2 * k == n] = -1.0
        form = [1, 1, 1]
        form[a] = n
        A[a] = (1.0 + cos).reshape(form)
    full = tuple(shape[a] if a in axes else 1 for a in range(3))
    B = []
    for a in axes:
        prod = np.ones(full)
        for b in axes:
            if b != a:
                prod = prod * A[b]
        B.append(np.broadcast_to(prod, full))
    total = sum(B)
    zero = total == 0
    return np.stack([np.where(zero, 1.0 / len(axes), b / np.where(zero, 1.0, total)) for b in B])


def kspace_split_np(v: np.ndarray, axes=(0, 1, 2)) -> np.ndarray:
    """(len(axes), X, Y, Z) float32: part ``a`` is the volume filtered with ``G_a`` (``split_weights``), in float64 ``np.fft``, rounded
    once.  The parts sum to the volume; a single axis gives the volume itself."""
    v = volume_np(v, "kspace_split_np", limit=True)
    axes = _axes(axes)
    if len(axes) == 1:
        return v[None].copy()
    spec = np.fft.fftn(v.astype(np.float64), axes=axes)
    return np.stack([np.fft.ifftn(spec * g, axes=axes).real for g in split_weights(v.shape, axes)]).astype(np.float32)


def unring_np(v: np.ndarray, axes=(0, 1, 2), K: int = 20, window=(1, 3), weighting: str = "kspace") -> np.ndarray:
    """``sum_a unring_axis_np(kspace_split_np(v, axes)[a], a)``, the axes ascending and the sums float32 adds; a single axis skips the
    split (``weighting="none"`` is accepted for one axis only)."""
    v = volume_np(v, "unring_np", limit=True)
    axes = _axes(axes)
    _check_weighting(weighting, axes, "unring_np")
    if len(axes) == 1:
        return unring_axis_np(v, axes[0], K, window)
    out = None
    for part, a in zip(kspace_split_np(v, axes), axes):
        u = unring_axis_np(part, a, K, window)
        with np.errstate(invalid="ignore", over="ignore"):
            out = u if out is None else out + u
    return out


# ---------------------------------------------------------------- device

_TABLES = {}
_WEIGHTS = {}


def _device_key(device):
    return device.type, device.index if device.index is not None else torch.cuda.current_device()


def _tables(n, K, device):
    key = (n, K) + _device_key(device)
    if key not in _TABLES:
        _TABLES[key] = (torch.from_numpy(shift_table(n, K)).to(device), torch.from_numpy(shift_fractions(K)).to(device))
    return _TABLES[key]


def unring_axis(vol: torch.Tensor, axis: int, K: int = 20, window=(1, 3), out: torch.Tensor = None) -> torch.Tensor:
    """vol: (X,Y,Z) float32 CUDA tensor with 8..512 voxels along ``axis`` -> the volume unringed along that axis, bit-equal to
    ``unring_axis_np``, NaN and Inf included.  One launch, no workspace, no device-to-host read: HIP-graph capturable once the tables
    of ``(extent, K)`` are cached (a first call outside the capture uploads them).  ``out``: the result goes to this tensor of the
    same shape (not ``vol``)."""
    what = "unring_axis"
    v = cuda_tensor(vol, (torch.float32,), what, ndim=3, limit=True)
    if axis not in (0, 1, 2):
        raise ValueError(f"{what}: axis is 0, 1 or 2, got {axis!r}")
    K = _check_shifts(K, what)
    a, b = _check_window(window, what)
    n = _check_line(int(v.shape[axis]), what)
    dst = out_like(out, v, (v,), what)
    table, fractions = _tables(n, K, v.device)
    L.call("mrisr_f32_volume_unring_axis", v.data_ptr(), *v.shape, int(axis), K, a, b, table.data_ptr(), fractions.data_ptr(),
           dst.data_ptr(), L.stream_ptr(), nbytes=8 * v.numel())
    return dst


def kspace_split(vol: torch.Tensor, axes=(0, 1, 2)) -> list:
    """vol: (X,Y,Z) float32 CUDA tensor -> one contiguous float32 part per axis of ``axes`` (ascending), ``irfftn(rfftn(vol) G_a)``
    with ``split_weights`` rounded once to float32 (the weights of the last shape stay on the device): ``kspace_split_np`` within the
    FFT's rounding.  A single axis gives ``[vol]``."""
    v = cuda_tensor(vol, (torch.float32,), "kspace_split", ndim=3, limit=True)
    axes = _axes(axes)
    if len(axes) == 1:
        return [v]
    shape = tuple(v.shape)
    key = (shape, axes) + _device_key(v.device)
    if key not in _WEIGHTS:
        _WEIGHTS.clear()                                             # the weights are as large as the spectra: only the last shape is kept
        g = split_weights(shape, axes)
        half = [slice(None)] * 4
        half[1 + axes[-1]] = slice(0, shape[axes[-1]] // 2 + 1)      # rfftn halves its last axis
        _WEIGHTS[key] = torch.from_numpy(np.ascontiguousarray(g[tuple(half)].astype(np.float32))).to(v.device)
    spec = torch.fft.rfftn(v, dim=axes)
    sizes = [shape[a] for a in axes]
    return [torch.fft.irfftn(spec * g, s=sizes, dim=axes).contiguous() for g in _WEIGHTS[key]]


def unring(vol: torch.Tensor, axes=(0, 1, 2), K: int = 20, window=(1, 3), weighting: str = "kspace") -> torch.Tensor:
    """vol: (X,Y,Z) float32 CUDA tensor -> ``sum_a unring_axis(kspace_split(vol, axes)[a], a)``, the axes ascending, the sums float32
    adds: bit-equal to that sum assembled by hand.  A single axis skips the split; ``weighting="none"`` is for one axis only."""
    what = "unring"
    v = cuda_tensor(vol, (torch.float32,), what, ndim=3, limit=True)
    axes = _axes(axes)
    _check_weighting(weighting, axes, what)
    K = _check_shifts(K, what)
    window = _check_window(window, what)
    for a in axes:
        _check_line(int(v.shape[a]), f"{what}: axis {a}")
    if len(axes) == 1:
        return unring_axis(v, axes[0], K, window)
    out = None
    for part, a in zip(kspace_split(v, axes), axes):
        u = unring_axis(part, a, K, window)
        out = u if out is None else out.add_(u)
    return out


def total_variation(vol: torch.Tensor) -> list:
    """The sum of ``|v[i + 1] - v[i]|`` along each axis of a CUDA volume, in float64 (what the scripts log; torch: plumbing)."""
    return [float(torch.diff(vol.double(), dim=a).abs().sum()) for a in range(3)]
