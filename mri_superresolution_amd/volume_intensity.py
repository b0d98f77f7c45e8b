"""Intensity standardisation between scans on the device (extension): MR intensities are in arbitrary units,
and two scanners or two sessions differ by a scale, an offset and usually a monotone contrast curve.  Nyul-Udupa landmark
standardisation takes a fixed set of percentiles of each scan's FOREGROUND and maps the source scan through the piecewise-linear
function that sends its landmarks onto the target's.

``landmarks_np``        the specification of the landmarks: ``np.percentile`` of the voxels inside a mask (NaN excluded), in
                        numpy's float32 path, restated in the explicit form the kernel implements
                        (``utils.imageops.percentile_bounds_np``'s rule).
``piecewise_map_np``    the specification of the map, float32, every operation rounded on its own.
``match_intensity_np``  the specification of the whole operation.
``masked_percentiles``, ``piecewise_map``, ``match_intensity``   the device path (``csrc/volume_intensity.hip``), equal to the
                        specification bit for bit.  There is no CPU path: CPU tensors raise.

Not built: histogram-exact (full CDF) matching.
"""
from __future__ import annotations

import logging
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from ._volume_args import cuda_tensor, mask_np, mask_tensor, volume_np
from .utils.imageops import np_percentile_f32

logger = logging.getLogger(__name__)

LANDMARKS = (1, 10, 20, 30, 40, 50, 60, 70, 80, 90, 99)
RANGE = (1, 99)
MAX_PERCENTILES = 16


class IntensityMatch(NamedTuple):
    percentiles: tuple               # the percentiles of the landmarks
    source_landmarks: np.ndarray     # (L,) float32
    target_landmarks: np.ndarray     # (L,) float32
    source_count: int                # voxels behind the source landmarks: inside the mask and not NaN
    target_count: int


def _check_percentiles(percentiles, least=2) -> tuple:
    """-> a tuple of ``least``..16 non-decreasing finite floats in [0, 100]."""
    try:
        q = tuple(float(x) for x in percentiles)
    except (TypeError, ValueError):
        raise ValueError(f"the percentiles are {least}..{MAX_PERCENTILES} numbers, got {percentiles!r}") from None
    if not least <= len(q) <= MAX_PERCENTILES or not all(np.isfinite(x) and 0.0 <= x <= 100.0 for x in q) \
            or any(b < a for a, b in zip(q, q[1:])):
        raise ValueError(f"the percentiles are {least}..{MAX_PERCENTILES} non-decreasing values in [0, 100], got {q}")
    return q


# ---------------------------------------------------------------- numpy specification

def masked_landmarks_np(vol, mask, q):
    """``landmarks_np`` for a checked ``vol`` and any number of percentiles ``q``."""
    keep = ~np.isnan(vol)
    if mask is not None:
        keep &= mask_np(mask, vol.shape, "landmarks_np") != 0
    s = np.sort(vol[keep].ravel())
    n = int(s.size)
    if n == 0:
        return np.full(len(q), np.nan, dtype=np.float32), 0
    return np.array([np_percentile_f32(s, p) for p in q], dtype=np.float32), n


def landmarks_np(vol, mask=None, percentiles=LANDMARKS):
    """-> (float32 (L,), int count): ``np.percentile(values, q)`` for every ``q`` of ``percentiles`` over
    ``values = vol[(mask != 0) & ~isnan(vol)]`` (``mask`` None: every voxel), ``count`` their number.  numpy's float32 path for a
    SCALAR ``q``, as ``utils.imageops.np_percentile_f32`` states it.  ``count == 0``: NaNs."""
    return masked_landmarks_np(volume_np(vol, "landmarks_np", ndim=None), mask, _check_percentiles(percentiles))


def _check_landmarks_np(lm, what):
    lm = np.asarray(lm)
    if lm.dtype != np.float32 or lm.ndim != 1 or not 2 <= lm.size <= MAX_PERCENTILES:
        raise ValueError(f"{what} are 2..{MAX_PERCENTILES} float32 values, got {lm.dtype} {lm.shape}")
    return lm


def piecewise_map_np(vol, src_landmarks, dst_landmarks) -> np.ndarray:
    """float32, the shape of ``vol``.  With ``s = src_landmarks`` and ``d = dst_landmarks`` (float32, equally many, 2..16), for every
    voxel ``v``: ``i = clip(#{j : s[j] <= v} - 1, 0, L - 2)`` (``np.searchsorted(s, v, side="right") - 1`` for sorted ``s``),
    ``w = s[i+1] - s[i]``, ``slope = 0 if w == 0 else (d[i+1] - d[i]) / w``, ``out = d[i] + (v - s[i]) * slope`` - float32, every
    operation rounded on its own.  Below ``s[0]`` and above ``s[L-1]`` the first and the last segment extend linearly: Nyul-Udupa's
    rule, no clamp.  A NaN voxel gives NaN; NaN landmarks give NaN everywhere."""
    vol = volume_np(vol, "piecewise_map_np", ndim=None)
    s, d = _check_landmarks_np(src_landmarks, "src_landmarks"), _check_landmarks_np(dst_landmarks, "dst_landmarks")
    if s.shape != d.shape:
        raise ValueError(f"as many source as target landmarks are expected, got {s.size} and {d.size}")
    with np.errstate(all="ignore"):
        w = s[1:] - s[:-1]
        slope = np.where(w == 0, np.float32(0), (d[1:] - d[:-1]) / np.where(w == 0, np.float32(1), w)).astype(np.float32)
        c = np.zeros(vol.shape, dtype=np.int64)
        for j in range(s.size):
            c += s[j] <= vol
        i = np.clip(c - 1, 0, s.size - 2)
        return d[i] + (vol - s[i]) * slope[i]


def _check_match(percentiles, sl, tl, sc, tc) -> IntensityMatch:
    if sc == 0 or tc == 0:
        raise ValueError(f"no voxels to take landmarks from: {sc} in the source, {tc} in the target (inside the masks, NaN excluded)")
    if (sl == sl[0]).all():
        raise ValueError(f"the source's landmarks are all {float(sl[0]):g} (a constant foreground): there is no map")
    return IntensityMatch(tuple(percentiles), sl, tl, int(sc), int(tc))


def match_intensity_np(source, target, source_mask=None, target_mask=None, percentiles=LANDMARKS):
    """-> (float32 array of ``source``'s shape, ``IntensityMatch``): ``piecewise_map_np(source, landmarks_np(source, source_mask),
    landmarks_np(target, target_mask))``.  ``ValueError`` when either side has no voxel to count or the source's landmarks are all
    equal (a constant foreground)."""
    q = _check_percentiles(percentiles)
    source, target = volume_np(source, "match_intensity_np", ndim=None), volume_np(target, "match_intensity_np", ndim=None)
    sl, sc = masked_landmarks_np(source, source_mask, q)
    tl, tc = masked_landmarks_np(target, target_mask, q)
    found = _check_match(q, sl, tl, sc, tc)
    return piecewise_map_np(source, sl, tl), found


# ---------------------------------------------------------------- device

def _check_landmarks(lm, n, what) -> torch.Tensor:
    if not isinstance(lm, torch.Tensor) or not lm.is_cuda:
        raise ValueError(f"{what} must be a CUDA tensor")
    if lm.dtype != torch.float32 or lm.dim() != 1 or not 2 <= lm.numel() <= MAX_PERCENTILES or not lm.is_contiguous() \
            or (n is not None and lm.numel() != n):
        raise ValueError(f"{what} are 2..{MAX_PERCENTILES} contiguous float32 values (equally many on both sides), got {lm.dtype} "
                         f"{tuple(lm.shape)}")
    return lm


def percentiles_workspace(nq: int, device) -> torch.Tensor:
    """An uninitialised workspace for ``masked_percentiles`` of ``nq`` quantiles: it may serve call after call on one stream."""
    nbytes = int(L.load().mrisr_f32_masked_percentiles_workspace_bytes(int(nq)))
    if nbytes == 0:
        raise ValueError(f"1..{MAX_PERCENTILES} percentiles are expected, got {nq}")
    return torch.empty(nbytes // 4, dtype=torch.int32, device=device)


def masked_percentiles(vol: torch.Tensor, mask=None, percentiles=LANDMARKS, workspace=None, out=None):
    """vol: contiguous float32 CUDA tensor; mask: a uint8 or bool CUDA tensor of its shape (non-zero = counted) or None -> (float32
    CUDA tensor (L,), int64 CUDA tensor (1,)): the landmarks and the count of ``landmarks_np``, equal by value.  One quantile alone
    is allowed here.  The ranks are derived on the device from the device-side count: 9 launches, no host read, no synchronisation
    (HIP-graph capturable when ``workspace`` - ``percentiles_workspace`` - is allocated before the capture).  ``out``: the pair of
    result tensors to write into (contiguous, on the volume's device: float32 (L,) and int64 (1,)), so that nothing is allocated."""
    v = cuda_tensor(vol, (torch.float32,), "masked_percentiles")
    q = _check_percentiles(percentiles, least=1)
    m = None if mask is None else mask_tensor(mask, v.shape, "masked_percentiles")
    if v.numel() > 0xffffffff:
        raise ValueError(f"masked_percentiles: at most 2^32 - 1 voxels, got {v.numel()}")
    ws = percentiles_workspace(len(q), v.device) if workspace is None else workspace
    need = int(L.load().mrisr_f32_masked_percentiles_workspace_bytes(len(q)))
    if not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.is_contiguous() and ws.numel() * ws.element_size() >= need
            and ws.data_ptr() % 16 == 0):
        raise ValueError(f"the workspace must be a contiguous 16-byte aligned CUDA tensor of at least {need} bytes")
    if out is None:
        out, count = torch.empty(len(q), dtype=torch.float32, device=v.device), torch.empty(1, dtype=torch.int64, device=v.device)
    else:
        out, count = out
        for t, dtype, n in ((out, torch.float32, len(q)), (count, torch.int64, 1)):
            if not (isinstance(t, torch.Tensor) and t.device == v.device and t.dtype == dtype and tuple(t.shape) == (n,) and t.is_contiguous()):
                raise ValueError(f"out is a pair of contiguous tensors on {v.device}: float32 ({len(q)},) and int64 (1,)")
    L.call("mrisr_f32_volume_masked_percentiles", v.data_ptr(), L.ptr(m), v.numel(), (L.C.c_double * len(q))(*q), len(q), out.data_ptr(),
           count.data_ptr(), ws.data_ptr(), L.stream_ptr())
    return out, count


def piecewise_map(vol: torch.Tensor, src_landmarks: torch.Tensor, dst_landmarks: torch.Tensor, out=None) -> torch.Tensor:
    """vol: contiguous float32 CUDA tensor; the landmarks: float32 CUDA tensors (L,), L in 2..16 -> the float32 CUDA tensor of
    ``piecewise_map_np``, bit for bit.  ``out``: such a tensor to overwrite; it may be ``vol`` itself.  One launch."""
    v = cuda_tensor(vol, (torch.float32,), "piecewise_map")
    s = _check_landmarks(src_landmarks, None, "src_landmarks")
    d = _check_landmarks(dst_landmarks, s.numel(), "dst_landmarks")
    if out is None:
        out = torch.empty_like(v)
    elif cuda_tensor(out, (torch.float32,), "piecewise_map").shape != v.shape:
        raise ValueError(f"out must have the shape {tuple(v.shape)}, got {tuple(out.shape)}")
    L.call("mrisr_f32_volume_piecewise_map", v.data_ptr(), v.numel(), s.data_ptr(), d.data_ptr(), s.numel(), out.data_ptr(), L.stream_ptr(),
           nbytes=8 * v.numel())
    return out


def match_intensity(source: torch.Tensor, target: torch.Tensor, source_mask=None, target_mask=None, percentiles=LANDMARKS):
    """The device path of ``match_intensity_np``, the same contract: -> (float32 CUDA tensor, ``IntensityMatch`` with host
    values), both bit-equal to the specification's.  Exactly ONE device-to-host read: both landmark vectors and both counts in one
    tensor, for the two checks (a count of 0, a constant foreground) and for logging."""
    q = _check_percentiles(percentiles)
    src, tgt = cuda_tensor(source, (torch.float32,), "match_intensity"), cuda_tensor(target, (torch.float32,), "match_intensity")
    ws = percentiles_workspace(len(q), src.device)
    sl, sc = masked_percentiles(src, source_mask, q, ws)
    tl, tc = masked_percentiles(tgt, target_mask, q, ws)
    n = len(q)
    host = torch.cat([sl.double(), tl.double(), sc.double(), tc.double()]).cpu().numpy()      # the one read (all values exact in double)
    found = _check_match(q, host[:n].astype(np.float32), host[n:2 * n].astype(np.float32), int(host[2 * n]), int(host[2 * n + 1]))
    return piecewise_map(src, sl, tl), found
