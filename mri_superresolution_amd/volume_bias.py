"""Bias-field matching between scans on the device (extension): a slowly varying multiplicative gain across the
head (B1 / coil sensitivity) is what a global monotone intensity map cannot touch.  The non-iterative low-pass-ratio method: a
masked Gaussian low-pass ``L = smooth(vol * m) / smooth(m)`` of each scan, and

  pairwise (differential bias correction)   ``field = L_ref / L_src``, ``out = src * field``
  single scan (homomorphic unsharp masking) ``field = L / median(L inside the mask)``, ``out = vol / field``

``gaussian_taps``, ``sigmas_for``   the taps of one axis (float64 weights, normalised, cast to float32) and the sigmas in voxels
                                    of a NIfTI affine.
``smooth_masked_np``, ``lowpass_np``, ``match_bias_np``, ``correct_bias_np``   the specification: float32, every product and every
                                    sum rounded on its own, the taps of a voxel added in ascending order, the passes over axis 2,
                                    then 1, then 0.
``smooth_masked``, ``match_bias``, ``correct_bias``   the device path (``csrc/volume_bias.hip``), equal to the specification bit
                                    for bit.  There is no CPU path: CPU tensors raise.  No device-to-host read; HIP-graph
                                    capturable with a ``BiasWorkspace`` made before the capture.

Not built: N4 / iterative histogram sharpening, a shrink factor (estimating the field on a coarser grid), the log-domain form, a
2-D form for ``scripts/evaluate.py``.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from ._volume_args import cuda_tensor, mask_np, mask_tensor, three_sigmas, volume_np
from .volume_intensity import masked_landmarks_np

MAX_RADIUS = 128
DEN_MIN = np.float32(1e-3)
MODE_PAIR, MODE_HUM, MODE_LOWPASS = 0, 1, 2      # MRISR_BIAS_*: mode of mrisr_f32_volume_bias_apply


def gaussian_taps(sigma_vox: float) -> np.ndarray:
    """float32 (2R+1,), ``R = ceil(3 sigma)``: ``exp(-0.5 (k / sigma)^2)`` in float64, divided by its float64 sum, cast to float32.
    ``sigma == 0``: ``[1]``.  ``ValueError`` for a negative or non-finite sigma and for ``R > MAX_RADIUS``."""
    sigma = float(sigma_vox)
    if not (math.isfinite(sigma) and sigma >= 0.0):
        raise ValueError(f"sigma must be finite and not negative, got {sigma_vox!r}")
    r = int(math.ceil(3.0 * sigma))
    if r > MAX_RADIUS:
        raise ValueError(f"sigma {sigma:g} voxels needs a radius of {r} taps, at most {MAX_RADIUS} are built")
    if r == 0:
        return np.ones(1, dtype=np.float32)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 * (k / sigma) ** 2)
    return (w / w.sum()).astype(np.float32)


def sigmas_for(affine, sigma_mm: float) -> tuple:
    """The sigma in voxels per axis of a grid with the index -> world ``affine`` (4 x 4): ``sigma_mm`` over the voxel sizes, the
    norms of the affine's columns."""
    a = np.asarray(affine, dtype=np.float64)
    if a.shape != (4, 4) or not np.isfinite(a).all():
        raise ValueError(f"sigmas_for takes a finite 4 x 4 affine, got shape {a.shape}")
    size = [float(np.linalg.norm(a[:3, i])) for i in range(3)]
    if not all(s > 0 for s in size) or not (math.isfinite(float(sigma_mm)) and float(sigma_mm) >= 0):
        raise ValueError(f"sigmas_for: voxel sizes {size} mm and sigma {sigma_mm!r} mm (positive sizes, a sigma that is not negative)")
    return tuple(float(sigma_mm) / s for s in size)


def _check_sigmas(sigmas_vox) -> list:
    return [gaussian_taps(x) for x in three_sigmas(sigmas_vox)]


def _check_limit(limit):
    hi = np.float32(limit)
    if not (np.isfinite(hi) and hi >= 1):
        raise ValueError(f"limit must be finite and at least 1, got {limit!r}")
    return np.float32(1) / hi, hi


# ---------------------------------------------------------------- numpy specification

def _check_pair_np(vol, mask, what):
    vol = volume_np(vol, what)
    return vol, mask_np(mask, vol.shape, what)


def _pass_np(x, w, axis):
    """One axis: for every voxel ``acc = 0``, then ``acc = acc + w[k] * x[i + k]`` for k ascending; taps outside contribute zero."""
    r = (w.size - 1) // 2
    n = x.shape[axis]
    pad = [(0, 0)] * 3
    pad[axis] = (r, r)
    xp = np.pad(x, pad)
    acc = np.zeros(x.shape, dtype=np.float32)
    index = [slice(None)] * 3
    with np.errstate(all="ignore"):
        for k in range(w.size):
            index[axis] = slice(k, k + n)
            acc = acc + w[k] * xp[tuple(index)]
    return acc


def _smooth_np(vol, keep, taps):
    a = np.where(keep, vol, np.float32(0)).astype(np.float32)
    b = keep.astype(np.float32)
    for axis in (2, 1, 0):
        a, b = _pass_np(a, taps[axis], axis), _pass_np(b, taps[axis], axis)
    return a, b


def smooth_masked_np(vol, mask, sigmas_vox):
    """-> (num, den), float32: the separable Gaussian of ``a = where(mask != 0 and not isnan(vol), vol, 0)`` and of the same
    predicate as 0 / 1, three passes over axis 2, 1, 0, intermediates float32 (module docstring)."""
    vol, mask = _check_pair_np(vol, mask, "smooth_masked_np")
    return _smooth_np(vol, (mask != 0) & ~np.isnan(vol), _check_sigmas(sigmas_vox))


def lowpass_np(num, den) -> np.ndarray:
    """``num / den`` (a correctly rounded float32 division) where ``den >= DEN_MIN``, NaN ("undefined") elsewhere."""
    with np.errstate(all="ignore"):
        return np.where(den >= DEN_MIN, num / np.where(den >= DEN_MIN, den, np.float32(1)), np.float32(np.nan)).astype(np.float32)


def _clamp_np(field, lo, hi):
    # by comparisons, so that a field that is not a number (inf / inf) has a place as well: the lower bound
    return np.where(field > hi, hi, np.where(field >= lo, field, lo)).astype(np.float32)


def match_bias_np(src, ref, src_mask, ref_mask, sigmas_vox, limit=4.0):
    """-> (out, field), float32.  One common mask ``m = src_mask & ref_mask``; ``field = L_ref / L_src`` where both low-passes are
    defined and positive, else 1, clamped to ``[1 / limit, limit]``; ``out = src * field`` on every voxel (NaN stays NaN)."""
    src, sm = _check_pair_np(src, src_mask, "match_bias_np")
    ref, rm = _check_pair_np(ref, ref_mask, "match_bias_np")
    if src.shape != ref.shape:
        raise ValueError(f"match_bias_np: the scans must share a grid, got shapes {src.shape} and {ref.shape}")
    taps = _check_sigmas(sigmas_vox)
    lo, hi = _check_limit(limit)
    m = (sm != 0) & (rm != 0)
    ls = lowpass_np(*_smooth_np(src, m & ~np.isnan(src), taps))
    lr = lowpass_np(*_smooth_np(ref, m & ~np.isnan(ref), taps))
    with np.errstate(all="ignore"):
        ok = (ls > 0) & (lr > 0)                  # NaN (undefined) compares false
        field = np.where(ok, lr / np.where(ok, ls, np.float32(1)), np.float32(1)).astype(np.float32)
        field = _clamp_np(field, lo, hi)
        return src * field, field


def correct_bias_np(vol, mask, sigmas_vox, limit=4.0):
    """-> (out, field), float32.  ``field = L / (p50 + 0)`` where the low-pass ``L`` is defined and positive, else 1, ``p50`` the 50th
    percentile of ``L`` over the voxels inside ``mask`` where it is defined (``volume_intensity.landmarks_np``'s rule); all ones
    when there is no such voxel.  Clamped to ``[1 / limit, limit]``; ``out = vol / field``."""
    vol, mask = _check_pair_np(vol, mask, "correct_bias_np")
    taps = _check_sigmas(sigmas_vox)
    lo, hi = _check_limit(limit)
    low = lowpass_np(*_smooth_np(vol, (mask != 0) & ~np.isnan(vol), taps))
    p50, count = masked_landmarks_np(low, mask, (50.0,))
    with np.errstate(all="ignore"):
        ok = (low > 0) & (count > 0)
        field = np.where(ok, low / (p50[0] + np.float32(0)), np.float32(1)).astype(np.float32)      # + 0: -0.0 and +0.0 are one median
        field = _clamp_np(field, lo, hi)
        return vol / field, field


# ---------------------------------------------------------------- device

class BiasWorkspace:
    """Everything ``match_bias`` / ``correct_bias`` need besides their outputs, for volumes of ``shape`` and the three sigmas: the
    taps on the device, the smoothing's intermediate, the sums of both scans, the low-pass and the percentile's workspace.  Made
    before a HIP-graph capture, it serves call after call on one stream.  Make one call with these sigmas before a capture, as a warm-up:
    the first call loads the code objects, and radii past about 60 raise the kernels' LDS limit on the current device at every call
    (a host-side attribute, not a stream operation)."""

    def __init__(self, shape, sigmas_vox, device):
        self.shape = tuple(int(d) for d in shape)
        if len(self.shape) != 3 or any(d < 1 for d in self.shape):
            raise ValueError(f"a volume has three positive extents, got {shape!r}")
        taps = _check_sigmas(sigmas_vox)
        self.sigmas = tuple(float(x) for x in sigmas_vox)
        self.radii = tuple((w.size - 1) // 2 for w in taps)
        self.taps = [torch.from_numpy(w).to(device) for w in taps]
        n = int(np.prod(self.shape))
        self.sums = torch.empty((6, n), dtype=torch.float32, device=device)       # tmp (2), num / den of the source, of the reference
        self.low = torch.empty(n, dtype=torch.float32, device=device)
        self.p50 = torch.empty(1, dtype=torch.float32, device=device)
        self.count = torch.empty(1, dtype=torch.int64, device=device)
        nbytes = int(L.load().mrisr_f32_masked_percentiles_workspace_bytes(1))
        self.select = torch.empty(nbytes // 4, dtype=torch.int32, device=device)


def _check_pair(vol, mask, what):
    vol = cuda_tensor(vol, (torch.float32,), what, ndim=3)
    return vol, mask_tensor(mask, vol.shape, what)


def _workspace(workspace, vol, sigmas_vox, what):
    if workspace is None:
        return BiasWorkspace(vol.shape, sigmas_vox, vol.device)
    if not isinstance(workspace, BiasWorkspace) or workspace.shape != tuple(vol.shape) or workspace.sums.device != vol.device \
            or workspace.sigmas != tuple(float(x) for x in sigmas_vox):
        raise ValueError(f"{what}: the workspace must be a BiasWorkspace for volumes of {tuple(vol.shape)} and these sigmas on {vol.device}")
    return workspace


def _smooth(vol, mask, mask2, ws, num, den):
    X, Y, Z = vol.shape
    L.call("mrisr_f32_volume_smooth_masked", vol.data_ptr(), mask.data_ptr(), L.ptr(mask2), X, Y, Z, ws.taps[0].data_ptr(), ws.radii[0],
           ws.taps[1].data_ptr(), ws.radii[1], ws.taps[2].data_ptr(), ws.radii[2], num.data_ptr(), den.data_ptr(), ws.sums[0].data_ptr(),
           L.stream_ptr(), nbytes=(45 if mask2 is None else 46) * vol.numel())      # 4 + 1 (+ 1) + 8, then twice 8 + 8 bytes a voxel


def _apply(mode, src, n, num, den, num_ref, den_ref, p50, count, limit, field, out):
    L.call("mrisr_f32_volume_bias_apply", L.ptr(src), n, num.data_ptr(), den.data_ptr(), L.ptr(num_ref), L.ptr(den_ref), L.ptr(p50),
           L.ptr(count), float(limit), mode, L.ptr(field), out.data_ptr(), L.stream_ptr())


def smooth_masked(vol: torch.Tensor, mask: torch.Tensor, sigmas_vox, workspace=None):
    """vol: contiguous float32 CUDA tensor (X, Y, Z); mask: uint8 or bool CUDA tensor of its shape -> (num, den), the float32 CUDA
    tensors of ``smooth_masked_np``, bit for bit.  Three launches (one per axis), both channels in each."""
    v, m = _check_pair(vol, mask, "smooth_masked")
    ws = _workspace(workspace, v, sigmas_vox, "smooth_masked")
    num, den = torch.empty_like(v), torch.empty_like(v)
    _smooth(v, m, None, ws, num, den)
    return num, den


def match_bias(src: torch.Tensor, ref: torch.Tensor, src_mask: torch.Tensor, ref_mask: torch.Tensor, sigmas_vox, limit=4.0,
               workspace=None, want_field=True):
    """The device path of ``match_bias_np``, bit for bit: -> (out, field), ``field`` None when ``want_field`` is false.  Seven
    launches (three per scan - both masks are read in the first pass of each, the common mask is never stored - and one that forms
    the field and applies it), no device-to-host read."""
    s, sm = _check_pair(src, src_mask, "match_bias")
    r, rm = _check_pair(ref, ref_mask, "match_bias")
    if s.shape != r.shape:
        raise ValueError(f"match_bias: the scans must share a grid, got shapes {tuple(s.shape)} and {tuple(r.shape)}")
    _check_limit(limit)
    ws = _workspace(workspace, s, sigmas_vox, "match_bias")
    _smooth(s, sm, rm, ws, ws.sums[2], ws.sums[3])
    _smooth(r, sm, rm, ws, ws.sums[4], ws.sums[5])
    out = torch.empty_like(s)
    field = torch.empty_like(s) if want_field else None
    _apply(MODE_PAIR, s, s.numel(), ws.sums[2], ws.sums[3], ws.sums[4], ws.sums[5], None, None, limit, field, out)
    return out, field


def correct_bias(vol: torch.Tensor, mask: torch.Tensor, sigmas_vox, limit=4.0, workspace=None, want_field=True):
    """The device path of ``correct_bias_np``, bit for bit: -> (out, field), ``field`` None when ``want_field`` is false.  The
    median of the low-pass is ``masked_percentiles``' exact selection, taken and used on the device: no device-to-host read."""
    v, m = _check_pair(vol, mask, "correct_bias")
    _check_limit(limit)
    if v.numel() > 0xffffffff:
        raise ValueError(f"correct_bias: at most 2^32 - 1 voxels, got {v.numel()}")
    ws = _workspace(workspace, v, sigmas_vox, "correct_bias")
    _smooth(v, m, None, ws, ws.sums[2], ws.sums[3])
    _apply(MODE_LOWPASS, None, v.numel(), ws.sums[2], ws.sums[3], None, None, None, None, limit, None, ws.low)
    L.call("mrisr_f32_volume_masked_percentiles", ws.low.data_ptr(), m.data_ptr(), v.numel(), (L.C.c_double * 1)(50.0), 1,
           ws.p50.data_ptr(), ws.count.data_ptr(), ws.select.data_ptr(), L.stream_ptr())
    out = torch.empty_like(v)
    field = torch.empty_like(v) if want_field else None
    _apply(MODE_HUM, v, v.numel(), ws.sums[2], ws.sums[3], None, None, ws.p50, ws.count, limit, field, out)
    return out, field
