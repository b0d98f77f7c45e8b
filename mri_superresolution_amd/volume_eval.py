"""Volume evaluation on the device (extension): is an enhanced volume closer to its ground truth than plain
interpolation, and does the three-plane blend beat one slice pass plus linear through-plane interpolation?

``downsample2``      the x2 degradation: mean over pairs along the chosen axes (``csrc/volume_eval.hip``), bit-equal to
                     ``downsample2_np``.  Output voxel ``i`` covers source voxels ``2i, 2i + 1`` - the model's half-pixel-centred
                     geometry (output ``o`` at input ``o / 2 - 1/4``).
``upscale2``         the x2 baselines, ``"linear"`` or ``"cubic"`` (Keys, A = -0.75), border replicated, one launch for all the
                     chosen axes, bit-equal to ``upscale2_np``.
``volume_metrics``   3-D Gaussian-window SSIM, MSE, RMSE, MAE and PSNR of a pair of volumes: one fused pass
                     (``csrc/volume_metrics.hip``) and one finalising launch; the (5,) float64 result stays on the device.
                     ``volume_metrics_np`` is its float64 specification.
                     With ``mask=`` the one pass also sums over the mask's voxels: (2, 5), whole volume and foreground.
``foreground_mask``  exact Otsu threshold on a 256-bin histogram plus an optional 3-D binary closing, all on the device
                     (``csrc/volume_mask.hip``), bit-equal to ``foreground_mask_np``.
``label_components`` connected components of a mask (``csrc/volume_label.hip``: union-find in LDS tiles, a merge launch across tile
                     borders, a flattening launch), bit-equal to ``label_components_np``; ``largest_component`` and ``fill_holes``
                     are the two clean-up steps built on it, which ``foreground_mask`` applies on request.
``evaluate_volume``  U-Net against the baselines on one ground-truth volume, optionally inside a foreground mask.

There is no CPU path: CPU tensors raise.  The ``*_np`` functions are the specifications the kernels are tested against.
"""
from __future__ import annotations

import logging
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from ._volume_args import check_classes, check_spacing, volume_np
from .utils.evalops import METRIC_COLUMNS
from .utils.imageops import _need_cuda
from .utils.losses import _check_window
from .volume import _up2_np, enhance_volume, enhance_volume_isotropic

logger = logging.getLogger(__name__)

METHODS = {"linear": L.RESAMPLE_LINEAR, "cubic": L.RESAMPLE_CUBIC}
CUBIC_WEIGHTS = (-0.03515625, 0.26171875, 0.87890625, -0.10546875)      # Keys, A = -0.75, at distances 1.75, 0.75, 0.25, 1.25


def _axes_mask(axes) -> int:
    axes = tuple(axes)
    if not axes or len(set(axes)) != len(axes) or any(a not in (0, 1, 2) for a in axes):
        raise ValueError(f"axes must be a non-empty selection of 0, 1, 2 without repeats, got {axes}")
    return sum(1 << int(a) for a in axes)


# ---------------------------------------------------------------- numpy specifications

def downsample2_np(v: np.ndarray, axes=(0, 1, 2)) -> np.ndarray:
    """Mean over pairs along ``axes``: for the axes in ascending order ``v = v[even] + v[odd]`` (float32), then one product with
    ``0.5 ** len(axes)`` (exact).  An odd extent on one of the axes is a ``ValueError``."""
    v = volume_np(v, "downsample2_np")
    mask = _axes_mask(axes)
    axes = [a for a in (0, 1, 2) if mask >> a & 1]
    for a in axes:
        if v.shape[a] % 2:
            raise ValueError(f"extent {v.shape[a]} of axis {a} is odd")
        m = np.moveaxis(v, a, 0)
        v = np.moveaxis(m[0::2] + m[1::2], 0, a)
    return np.ascontiguousarray(v * np.float32(0.5 ** len(axes)))


def _up2_cubic_np(e: np.ndarray, axis: int) -> np.ndarray:
    f32 = np.float32
    e = np.moveaxis(e, axis, 0)
    n = e.shape[0]
    idx = np.arange(n)
    tap = {d: e[np.clip(idx + d, 0, n - 1)] for d in (-2, -1, 0, 1, 2)}      # replicated border
    w = [f32(x) for x in CUBIC_WEIGHTS]
    u = np.empty((2 * n,) + e.shape[1:], dtype=f32)
    # every operation on float32 arrays rounds to float32: four products, summed in ascending tap order
    u[0::2] = ((w[0] * tap[-2] + w[1] * tap[-1]) + w[2] * tap[0]) + w[3] * tap[1]
    u[1::2] = ((w[3] * tap[-1] + w[2] * tap[0]) + w[1] * tap[1]) + w[0] * tap[2]
    return np.moveaxis(u, 0, axis)


def upscale2_np(v: np.ndarray, method: str, axes=(0, 1, 2)) -> np.ndarray:
    """Doubles ``axes`` in ascending order, each pass on the float32 result of the one before, border replicated.  ``"linear"``
    is ``volume._up2_np`` (``0.75 e[i] + 0.25 e[i -+ 1]``); ``"cubic"`` is Keys with A = -0.75: ``u[2i]`` from taps
    ``i-2 .. i+1`` with ``CUBIC_WEIGHTS``, ``u[2i+1]`` from taps ``i-1 .. i+2`` with the mirrored weights."""
    v = volume_np(v, "upscale2_np")
    if method not in METHODS:
        raise ValueError(f"Unknown interpolation method: {method}")
    mask = _axes_mask(axes)
    for a in (0, 1, 2):
        if mask >> a & 1:
            v = _up2_np(v, a) if method == "linear" else _up2_cubic_np(v, a)
    return np.ascontiguousarray(v)


def gaussian_window_np(window_size: int, sigma: float) -> np.ndarray:
    """The 1-D window of ``utils/losses.py:gaussian_window`` (float32 arithmetic), as float64."""
    coords = np.arange(window_size, dtype=np.float32) - np.float32(window_size // 2)
    g = np.exp(-(coords ** 2) / np.float32(2 * sigma ** 2)).astype(np.float32)
    return (g / g.sum(dtype=np.float32)).astype(np.float64)


def _blur_np(v: np.ndarray, g: np.ndarray) -> np.ndarray:
    h = len(g) // 2
    for a in range(3):
        n = v.shape[a]
        pad = [(0, 0)] * 3
        pad[a] = (h, h)
        p = np.pad(v, pad)                                      # zero padding
        idx = [slice(None)] * 3
        out = np.zeros_like(v)
        for k, gk in enumerate(g):
            idx[a] = slice(k, k + n)
            out += gk * p[tuple(idx)]
        v = out
    return v


def ssim_map_np(a: np.ndarray, b: np.ndarray, val_range: float, window_size: int = 11, sigma: float = 1.5) -> np.ndarray:
    """The reference's SSIM map (``utils/losses.py:27-70``) in three dimensions and float64: separable Gaussian window, zero
    padding, the size of the volume."""
    _check_window(window_size)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    g = gaussian_window_np(window_size, sigma)
    c1, c2 = (0.01 * val_range) ** 2, (0.03 * val_range) ** 2
    mu1, mu2 = _blur_np(a, g), _blur_np(b, g)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = _blur_np(a * a, g) - mu1_sq, _blur_np(b * b, g) - mu2_sq, _blur_np(a * b, g) - mu12
    return ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s11 + s22 + c2))


def volume_metrics_np(pred: np.ndarray, ref: np.ndarray, val_range: float, window_size: int = 11, sigma: float = 1.5,
                      mask: np.ndarray = None) -> np.ndarray:
    """(ssim, mse, rmse, mae, psnr) of two volumes in float64: the specification of ``volume_metrics``.  With ``mask`` (same shape,
    non-zero = foreground) every mean is taken over the mask's voxels, the SSIM mean over ``ssim_map_np(...)[mask != 0]`` - the map
    itself is the unmasked one; an empty mask gives five NaNs."""
    a, b = np.asarray(pred, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 3 or a.size == 0:
        raise ValueError(f"expected two non-empty volumes of one shape, got {a.shape} and {b.shape}")
    if not val_range > 0:
        raise ValueError(f"val_range must be positive, got {val_range}")
    d = a - b
    smap = ssim_map_np(a, b, val_range, window_size, sigma)
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != a.shape:
            raise ValueError(f"mask shape {mask.shape} is not the volumes' shape {a.shape}")
        sel = mask != 0
        if not sel.any():
            return np.full(5, np.nan)
        d, smap = d[sel], smap[sel]
    mse, mae = float(np.mean(d * d)), float(np.mean(np.abs(d)))
    ssim = float(np.mean(smap))
    psnr = 100.0 if mse < 1e-10 else 10.0 * np.log10(float(val_range) ** 2 / mse)
    return np.array([ssim, mse, np.sqrt(mse), mae, psnr], dtype=np.float64)


def otsu_bins_np(v: np.ndarray):
    """-> (lo, hi, bins): the extrema of the float32 volume and the histogram bin 0..255 of every voxel (int32), in float32 one
    rounded operation at a time: ``scale = 256 / (hi - lo)``, ``bin = min(255, int((v - lo) * scale))`` (truncated).  ``bins`` is
    ``None`` for a degenerate range: ``hi == lo``, or ``hi - lo`` or ``scale`` not finite in float32."""
    v = volume_np(v, "otsu_bins_np")
    f32 = np.float32
    lo, hi = f32(v.min()), f32(v.max())
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        width = f32(hi - lo)
        scale = f32(f32(256) / width) if width != 0 else f32(np.inf)
    if hi == lo or not np.isfinite(width) or not np.isfinite(scale):
        return lo, hi, None
    pos = (v - lo) * scale                                       # float32 array ops: each rounds to float32
    return lo, hi, np.minimum(255, pos.astype(np.int32))


def otsu_threshold_np(counts) -> int:
    """``t*`` of 256 bin counts, in bin-index space: exact integer prefix sums ``w_t``, ``m_t``; for ``t`` in 0..254 with
    ``0 < w_t < N``: ``mu0 = m_t / w_t``, ``mu1 = (M - m_t) / (N - w_t)``, ``d = mu1 - mu0``, ``s_t = (w_t (N - w_t)) (d d)`` in IEEE
    double, one operation at a time in this order; the smallest ``t`` with the largest ``s_t`` (-1 if no ``t`` qualifies)."""
    n = [int(c) for c in counts]
    N, M = sum(n), sum(k * c for k, c in enumerate(n))
    w = m = 0
    best, sbest = -1, -1.0
    for t in range(255):
        w += n[t]
        m += t * n[t]
        if not 0 < w < N:
            continue
        mu0 = float(m) / float(w)
        mu1 = float(M - m) / float(N - w)
        d = mu1 - mu0
        s = (float(w) * float(N - w)) * (d * d)
        if s > sbest:
            best, sbest = t, s
    return best


def _morph_np(m: np.ndarray, r: int, op) -> np.ndarray:
    for a in range(3):
        n = m.shape[a]
        out = m.copy()
        for d in range(1, r + 1):                                # taps outside the volume are ignored
            if d >= n:
                break
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[a], hi[a] = slice(0, n - d), slice(d, n)
            out[tuple(lo)] = op(out[tuple(lo)], m[tuple(hi)])
            out[tuple(hi)] = op(out[tuple(hi)], m[tuple(lo)])
        m = out
    return m


def dilate_np(m: np.ndarray, r: int) -> np.ndarray:
    """Max of the uint8 volume over the box ``|dx|, |dy|, |dz| <= r`` clipped to the volume."""
    return _morph_np(np.asarray(m, dtype=np.uint8), r, np.maximum)


def erode_np(m: np.ndarray, r: int) -> np.ndarray:
    """Min over the same clipped box: voxels outside the volume are ignored, so the border does not erode the mask."""
    return _morph_np(np.asarray(m, dtype=np.uint8), r, np.minimum)


def _check_radius(r):
    if not isinstance(r, (int, np.integer)) or isinstance(r, bool) or not 0 <= r <= 4:
        raise ValueError(f"close_radius must be an integer in 0..4, got {r!r}")
    return int(r)


def _check_connectivity(connectivity):
    if isinstance(connectivity, bool) or connectivity not in (6, 26):
        raise ValueError(f"connectivity must be 6 or 26, got {connectivity!r}")
    return int(connectivity)


def _check_plane_axis(axis, what="plane_axis"):
    """None -> -1, else the axis 0..2."""
    if axis is None:
        return -1
    if not isinstance(axis, (int, np.integer)) or isinstance(axis, bool) or axis not in (0, 1, 2):
        raise ValueError(f"{what} must be None, 0, 1 or 2, got {axis!r}")
    return int(axis)


def _check_fill(fill):
    """``fill_holes=`` of ``foreground_mask``: None -> None, "3d" -> -1, an axis -> that axis."""
    if fill is None:
        return None
    if isinstance(fill, str):
        if fill == "3d":
            return -1
        raise ValueError(f"fill_holes must be None, '3d', 0, 1 or 2, got {fill!r}")
    return _check_plane_axis(fill, "fill_holes")


def _check_mask_np(mask, what):
    mask = np.asarray(mask)
    if mask.ndim != 3 or mask.size == 0:
        raise ValueError(f"{what}: expected a non-empty mask (X,Y,Z), got {mask.shape}")
    return mask


def backward_offsets(connectivity: int, plane_axis: int = -1):
    """The neighbour offsets that come before the centre in C order (every pair of neighbours once): 13 of the 26, 3 of the 6;
    with ``plane_axis`` 0..2 only those with no step along that axis (4 of the 8, 2 of the 4)."""
    out = []
    for k in range(13):
        d = (k // 9 - 1, k // 3 % 3 - 1, k % 3 - 1)
        if connectivity == 6 and sum(c != 0 for c in d) != 1:
            continue
        if plane_axis >= 0 and d[plane_axis] != 0:
            continue
        out.append(d)
    return out


def label_components_np(mask: np.ndarray, connectivity: int = 26, plane_axis=None, invert: bool = False) -> np.ndarray:
    """The specification of ``label_components``: int32 labels of the non-zero voxels of ``mask`` (of its zero voxels with
    ``invert``), a voxel's label ``1 + the smallest C-order linear index of its component``, 0 elsewhere.  ``connectivity`` 6 or
    26; with ``plane_axis`` only neighbours inside the planes across that axis count.  Exact, without scipy: the edge list per
    neighbour offset, then rounds of hooking the larger root under the smaller (``np.minimum.at``) and pointer jumping until no
    edge joins two roots."""
    mask = _check_mask_np(mask, "label_components_np")
    conn, axis = _check_connectivity(connectivity), _check_plane_axis(plane_axis)
    fg = (mask != 0) != bool(invert)
    n = fg.size
    if n > 2 ** 31 - 2:
        raise ValueError(f"label_components_np: {n} voxels, labels are int32 (at most 2^31 - 2)")
    idx = np.arange(n, dtype=np.int64).reshape(fg.shape)
    hi, lo = [], []
    for d in backward_offsets(conn, axis):
        a = tuple(slice(max(0, -c), s - max(0, c)) for c, s in zip(d, fg.shape))       # the voxel
        b = tuple(slice(max(0, c), s - max(0, -c)) for c, s in zip(d, fg.shape))       # its neighbour at + d (earlier in C order)
        both = fg[a] & fg[b]
        hi.append(idx[a][both])
        lo.append(idx[b][both])
    hi, lo = np.concatenate(hi), np.concatenate(lo)
    parent = np.arange(n, dtype=np.int64)
    while hi.size:
        ra, rb = parent[hi], parent[lo]                         # roots: the forest is flat at this point
        open_ = ra != rb
        if not open_.any():
            break
        hi, lo, ra, rb = hi[open_], lo[open_], ra[open_], rb[open_]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:                                             # pointer jumping
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    return np.where(fg.reshape(-1), parent + 1, 0).astype(np.int32).reshape(fg.shape)


def largest_component_np(mask: np.ndarray, connectivity: int = 26):
    """-> (uint8 mask of the largest component - of several of one size the one with the smallest label -, float64 array
    [components, kept size, kept label]); an empty mask gives zeros and [0, 0, 0]."""
    lab = label_components_np(mask, connectivity)
    flat = lab.reshape(-1)
    roots = np.flatnonzero(flat == np.arange(1, flat.size + 1))
    if roots.size == 0:
        return np.zeros(lab.shape, dtype=np.uint8), np.zeros(3)
    sizes = np.bincount(flat, minlength=flat.size + 1)[roots + 1]
    k = int(np.argmax(sizes))                                   # the first of the largest: the smallest label
    return (lab == roots[k] + 1).astype(np.uint8), np.array([roots.size, sizes[k], roots[k] + 1], dtype=np.float64)


def fill_holes_np(mask: np.ndarray, axis=None):
    """-> (uint8 ``mask != 0`` plus every zero voxel whose 6-connected component of zero voxels owns no voxel on a face of the
    volume, the number of voxels filled): ``scipy.ndimage.binary_fill_holes``.  With ``axis`` 0..2 plane by plane across that
    axis: the zero voxels 4-connected inside the plane, the test "owns no voxel on an edge of its plane"."""
    mask = _check_mask_np(mask, "fill_holes_np")
    a = _check_plane_axis(axis, "axis")
    lab = label_components_np(mask, 6, axis, invert=True)
    border = np.zeros(lab.shape, dtype=bool)
    for ax in range(3):
        if ax != a:
            sl = [slice(None)] * 3
            for edge in (0, -1):
                sl[ax] = edge
                border[tuple(sl)] = True
    touches = np.zeros(lab.size + 1, dtype=bool)
    touches[lab[border]] = True
    filled = (lab != 0) & ~touches[lab]
    return ((mask != 0) | filled).astype(np.uint8), int(filled.sum())


def foreground_mask_np(v: np.ndarray, close_radius: int = 0, return_stats: bool = False, largest: bool = False, fill_holes=None):
    """The specification of ``foreground_mask``: ``mask = bin(v) > t*`` (uint8, 0 / 1) with the bins of ``otsu_bins_np`` and the
    ``t*`` of ``otsu_threshold_np`` on their counts - an integer comparison, exactly consistent with the histogram - then, for
    ``close_radius`` r in 1..4, the closing ``erode_np(dilate_np(mask, r), r)``.  A degenerate range gives ``t* = -1`` and a mask of
    ones.  ``return_stats``: -> (mask, dict(lo, hi, t, count, counts)), the count and the 256 counts those of the Otsu mask
    before the closing.  Then, on request: ``largest`` keeps the largest 26-connected component (``largest_component_np``), and
    ``fill_holes`` (``"3d"`` or an axis 0..2) fills the holes of what is left (``fill_holes_np``); with either the dict gains
    ``cleanup``: [components found, kept size, voxels filled], NaN for a step that is off."""
    r, fill = _check_radius(close_radius), _check_fill(fill_holes)
    lo, hi, bins = otsu_bins_np(v)
    if bins is None:
        t, counts = -1, np.zeros(256, dtype=np.int64)
        mask = np.ones(np.shape(v), dtype=np.uint8)
    else:
        counts = np.bincount(bins.reshape(-1), minlength=256).astype(np.int64)
        t = otsu_threshold_np(counts)
        mask = (bins > t).astype(np.uint8)
    stats = dict(lo=lo, hi=hi, t=t, count=int(mask.sum(dtype=np.int64)), counts=counts)
    if r:
        mask = erode_np(dilate_np(mask, r), r)
    if largest or fill is not None:
        cleanup = np.full(3, np.nan)
        if largest:
            mask, st3 = largest_component_np(mask, 26)
            cleanup[:2] = st3[:2]
        if fill is not None:
            mask, cleanup[2] = fill_holes_np(mask, None if fill < 0 else fill)
        stats["cleanup"] = cleanup
    return (mask, stats) if return_stats else mask


def otsu_threshold_value(lo: float, hi: float, t: int) -> float:
    """The threshold in intensity units, for logging only (no voxel is ever compared with it): the lower edge of bin ``t + 1``."""
    return float(lo) + (int(t) + 1) * (float(hi) - float(lo)) / 256.0


# ---------------------------------------------------------------- device

def _check_vol(vol, what):
    _need_cuda(vol, what)
    if vol.dtype != torch.float32 or vol.dim() != 3 or vol.numel() == 0:
        raise ValueError(f"{what}: expected a non-empty float32 volume (X,Y,Z), got {vol.dtype} {tuple(vol.shape)}")
    return vol.contiguous()


def downsample2(vol: torch.Tensor, axes=(0, 1, 2)) -> torch.Tensor:
    """vol: (X,Y,Z) float32 CUDA tensor -> the volume with ``axes`` halved (mean over pairs), bit-equal to ``downsample2_np``."""
    mask = _axes_mask(axes)
    v = _check_vol(vol, "downsample2")
    for a in (0, 1, 2):
        if mask >> a & 1 and v.shape[a] % 2:
            raise ValueError(f"extent {v.shape[a]} of axis {a} is odd")
    shape = tuple(d // 2 if mask >> a & 1 else d for a, d in enumerate(v.shape))
    out = torch.empty(shape, dtype=torch.float32, device=v.device)
    L.call("mrisr_f32_volume_down2", v.data_ptr(), *v.shape, mask, out.data_ptr(), L.stream_ptr(),
           nbytes=4 * (v.numel() + out.numel()))
    return out


def upscale2(vol: torch.Tensor, method: str, axes=(0, 1, 2)) -> torch.Tensor:
    """vol: (X,Y,Z) float32 CUDA tensor -> the volume with ``axes`` doubled, ``"linear"`` or ``"cubic"``, bit-equal to
    ``upscale2_np``."""
    if method not in METHODS:
        raise ValueError(f"Unknown interpolation method: {method}")
    mask = _axes_mask(axes)
    v = _check_vol(vol, "upscale2")
    shape = tuple(2 * d if mask >> a & 1 else d for a, d in enumerate(v.shape))
    out = torch.empty(shape, dtype=torch.float32, device=v.device)
    L.call("mrisr_f32_volume_up2", v.data_ptr(), *v.shape, mask, METHODS[method], out.data_ptr(), L.stream_ptr(),
           nbytes=4 * (v.numel() + out.numel()))
    return out


def _check_mask(mask, shape, what):
    """shape None: any non-empty (X,Y,Z)."""
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"{what}: the mask must be a tensor, got {type(mask).__name__}")
    _need_cuda(mask, what)
    bad_shape = mask.dim() != 3 or mask.numel() == 0 if shape is None else tuple(mask.shape) != tuple(shape)
    if mask.dtype not in (torch.uint8, torch.bool) or bad_shape:
        raise ValueError(f"{what}: expected a uint8 (or bool) mask of shape {'(X,Y,Z)' if shape is None else tuple(shape)}, "
                         f"got {mask.dtype} {tuple(mask.shape)}")
    return (mask.to(torch.uint8) if mask.dtype == torch.bool else mask).contiguous()


def otsu_mask(vol: torch.Tensor):
    """vol: (X,Y,Z) float32 CUDA tensor -> (mask uint8 (X,Y,Z), stats (4,) float64: lo, hi, t*, foreground count, counts (256,)
    int64), all on the device, bit-equal to ``foreground_mask_np(vol, 0, return_stats=True)``.  Five launches, no host
    synchronisation."""
    v = _check_vol(vol, "otsu_mask")
    lib = L.load()
    ws = torch.empty(int(lib.mrisr_f32_volume_otsu_workspace_bytes()) // 8, dtype=torch.int64, device=v.device)
    mask = torch.empty(v.shape, dtype=torch.uint8, device=v.device)
    stats = torch.empty(4, dtype=torch.float64, device=v.device)
    L.call("mrisr_f32_volume_otsu_mask", v.data_ptr(), *v.shape, mask.data_ptr(), stats.data_ptr(), ws.data_ptr(), L.stream_ptr(),
           nbytes=13 * v.numel())      # the volume three times (extrema, counts, mask), the mask written once
    return mask, stats, ws[:256]


def _morph(src, radius, op, dst, tmp):
    L.call("mrisr_u8_volume_morph", src.data_ptr(), *src.shape, int(radius), op, dst.data_ptr(), L.ptr(tmp), L.stream_ptr(),
           nbytes=6 * src.numel())    # three passes, each reads and writes the volume once
    return dst


def binary_dilate(mask: torch.Tensor, radius: int) -> torch.Tensor:
    """mask: (X,Y,Z) uint8 CUDA tensor -> its maximum over the clipped box of ``radius`` (0..4), bit-equal to ``dilate_np``."""
    m = _check_mask(mask, None, "binary_dilate")
    return _morph(m, _check_radius(radius), L.MORPH_DILATE, torch.empty_like(m), torch.empty_like(m))


def binary_erode(mask: torch.Tensor, radius: int) -> torch.Tensor:
    """The minimum over the same box, bit-equal to ``erode_np``."""
    m = _check_mask(mask, None, "binary_erode")
    return _morph(m, _check_radius(radius), L.MORPH_ERODE, torch.empty_like(m), torch.empty_like(m))


def binary_close(mask: torch.Tensor, radius: int) -> torch.Tensor:
    """Erosion of the dilation (``radius`` 0: the mask itself), three buffers in all; bit-equal to
    ``erode_np(dilate_np(mask, radius), radius)``."""
    m = _check_mask(mask, None, "binary_close")
    r = _check_radius(radius)
    if r == 0:
        return m
    grown, tmp = torch.empty_like(m), torch.empty_like(m)
    _morph(m, r, L.MORPH_DILATE, grown, tmp)
    return _morph(grown, r, L.MORPH_ERODE, torch.empty_like(m), tmp)


def _label_workspace(m):
    nbytes = int(L.load().mrisr_u8_volume_label_workspace_bytes(*m.shape))
    if nbytes == 0:
        raise ValueError(f"a mask of {tuple(m.shape)} has more than 2^31 - 2 voxels: labels are int32")
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=m.device)


def label_components(mask: torch.Tensor, connectivity: int = 26, plane_axis=None, invert: bool = False) -> torch.Tensor:
    """mask: (X,Y,Z) uint8 / bool CUDA tensor -> int32 CUDA tensor of labels, bit-equal to ``label_components_np``: a foreground
    voxel's label is 1 + the smallest C-order linear index of its component.  Three launches, no host synchronisation."""
    conn, axis = _check_connectivity(connectivity), _check_plane_axis(plane_axis)
    m = _check_mask(mask, None, "label_components")
    if m.numel() > 2 ** 31 - 2:
        raise ValueError(f"a mask of {tuple(m.shape)} has more than 2^31 - 2 voxels: labels are int32")
    labels = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    L.call("mrisr_u8_volume_label", m.data_ptr(), *m.shape, conn, axis, int(bool(invert)), labels.data_ptr(), L.stream_ptr())
    return labels


def _largest(m, conn):
    dst, stats = torch.empty_like(m), torch.empty(3, dtype=torch.float64, device=m.device)
    ws = _label_workspace(m)
    L.call("mrisr_u8_volume_keep_largest", m.data_ptr(), *m.shape, conn, dst.data_ptr(), stats.data_ptr(), ws.data_ptr(), L.stream_ptr())
    return dst, stats


def _fill(m, axis):
    dst, filled = torch.empty_like(m), torch.empty(1, dtype=torch.float64, device=m.device)
    ws = _label_workspace(m)
    L.call("mrisr_u8_volume_fill_holes", m.data_ptr(), *m.shape, axis, dst.data_ptr(), filled.data_ptr(), ws.data_ptr(), L.stream_ptr())
    return dst, filled


def largest_component(mask: torch.Tensor, connectivity: int = 26):
    """-> (uint8 CUDA mask of the largest component, (3,) float64 CUDA tensor: components, kept size, kept label), bit-equal to
    ``largest_component_np``.  No host synchronisation."""
    conn = _check_connectivity(connectivity)
    return _largest(_check_mask(mask, None, "largest_component"), conn)


def fill_holes(mask: torch.Tensor, axis=None):
    """-> (uint8 CUDA mask with its holes filled, 0-d float64 CUDA tensor: the voxels filled), bit-equal to ``fill_holes_np``; the
    volume's holes, or with ``axis`` 0..2 those of every plane across that axis.  No host synchronisation."""
    a = _check_plane_axis(axis, "axis")
    dst, filled = _fill(_check_mask(mask, None, "fill_holes"), a)
    return dst, filled[0]


def _clean_mask(m, largest, fill):
    """largest (26-connected), then fill (None, -1 or an axis) -> (mask, (3,) float64 CUDA tensor [components, kept size, filled]
    with NaN for a step that is off; None when both are off)."""
    if not largest and fill is None:
        return m, None
    cleanup = torch.full((3,), float("nan"), dtype=torch.float64, device=m.device)
    if largest:
        m, st3 = _largest(m, 26)
        cleanup[:2] = st3[:2]
    if fill is not None:
        m, filled = _fill(m, fill)
        cleanup[2:] = filled
    return m, cleanup


def foreground_mask(vol: torch.Tensor, close_radius: int = 0, largest: bool = False, fill_holes=None):
    """vol: (X,Y,Z) float32 CUDA tensor -> (mask uint8 CUDA tensor, stats (4,) float64 CUDA tensor: lo, hi, t*, and the foreground
    count of the Otsu mask before the closing).  Bit-equal to ``foreground_mask_np``.  No host synchronisation.

    ``largest`` keeps the largest 26-connected component of the closed mask, ``fill_holes`` (``"3d"`` or an axis 0..2) then fills
    its holes; with either, ``stats.cleanup`` is the (3,) float64 CUDA tensor [components found, kept size, voxels filled] (NaN
    for a step that is off) - a convenience of THIS object, ``None`` otherwise."""
    r, fill = _check_radius(close_radius), _check_fill(fill_holes)
    mask, stats, _ = otsu_mask(vol)
    mask, stats.cleanup = _clean_mask(binary_close(mask, r), bool(largest), fill)
    return mask, stats


def volume_metrics(pred: torch.Tensor, ref: torch.Tensor, val_range: float, window_size: int = 11, sigma: float = 1.5,
                   mask: torch.Tensor = None) -> torch.Tensor:
    """pred, ref: (X,Y,Z) float32 CUDA tensors -> (5,) float64 CUDA tensor, columns ``METRIC_COLUMNS`` (ssim, mse, rmse, mae,
    psnr; PSNR = 10 log10(val_range^2 / mse), 100 when mse < 1e-10).  No host synchronisation.

    With ``mask`` (uint8 or bool CUDA tensor of the same shape, non-zero = foreground): a (2, 5) tensor from the same single pass
    over the volumes - row 0 the whole volume, row 1 the mask's voxels (five NaNs for an empty mask).  The number of mask voxels
    is the 0-d float64 CUDA tensor ``result.mask_count``; ``result.packed`` is the (11,) tensor that holds both (one download)."""
    _check_window(window_size)
    a, b = _check_vol(pred, "volume_metrics"), _check_vol(ref, "volume_metrics")
    if a.shape != b.shape:
        raise ValueError(f"shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
    if not (val_range > 0 and sigma > 0):
        raise ValueError(f"val_range and sigma must be positive, got {val_range} and {sigma}")
    st = L.stream_ptr()
    if mask is not None:
        m = _check_mask(mask, a.shape, "volume_metrics")
        sums = torch.zeros(7, dtype=torch.float64, device=a.device)
        packed = torch.empty(11, dtype=torch.float64, device=a.device)
        L.call("mrisr_f32_volume_metrics_masked", a.data_ptr(), b.data_ptr(), m.data_ptr(), *a.shape, float(val_range), float(sigma),
               int(window_size), sums.data_ptr(), st, nbytes=9 * a.numel())      # the two fp32 volumes and the mask once
        L.call("mrisr_volume_metrics_finalize_masked", sums.data_ptr(), *a.shape, float(val_range), packed.data_ptr(), st)
        out = packed[:10].view(2, 5)
        out.mask_count, out.packed = packed[10], packed      # a convenience of THIS object: any op on it returns a plain tensor
        return out
    sums = torch.zeros(3, dtype=torch.float64, device=a.device)
    out = torch.empty(5, dtype=torch.float64, device=a.device)
    L.call("mrisr_f32_volume_metrics", a.data_ptr(), b.data_ptr(), *a.shape, float(val_range), float(sigma), int(window_size),
           sums.data_ptr(), st, nbytes=8 * a.numel())      # the two fp32 volumes once
    L.call("mrisr_volume_metrics_finalize", sums.data_ptr(), *a.shape, float(val_range), out.data_ptr(), st)
    return out


class VolumeScores(OrderedDict):
    """What ``evaluate_volume`` returns: ``{method: metrics tensor}`` in method order.  With a mask it also carries ``mask``
    (the uint8 CUDA tensor every method was scored with), ``mask_count`` (its voxel count, 0-d float64 CUDA tensor) and
    ``mask_stats`` (``foreground_mask``'s (4,) float64 CUDA tensor lo, hi, t*, count for ``"otsu"``); all three ``None`` otherwise.
    ``mask_cleanup``: the (3,) float64 CUDA tensor [components found, kept size, voxels filled] of the mask's clean-up (NaN for a
    step that is off), ``None`` when neither ``mask_largest`` nor ``mask_fill_holes`` is on.  ``tissue_dice``: ``{method: (K,) float64
    numpy array}`` with ``evaluate_volume(tissue_dice=K)``, else ``None``.  ``tissue_surface``: ``{method: volume_surface.SurfaceDistances}`` with
    ``evaluate_volume(tissue_surface=True)``, else ``None``.  ``tissue_edges``: ``{method: volume_sharpness.EdgeSharpness}`` with
    ``evaluate_volume(tissue_edges=True)``, else ``None``."""

    def __init__(self):
        super().__init__()
        self.mask = self.mask_count = self.mask_stats = self.mask_cleanup = self.tissue_dice = self.tissue_surface = None
        self.tissue_edges = None


_DEGRADE_WARNED = False


def _warn_degrade_ignored(degrade):
    global _DEGRADE_WARNED
    if not _DEGRADE_WARNED:
        logger.warning(f"degrade={degrade!r} is ignored: the low-resolution volume is given.")
        _DEGRADE_WARNED = True


def evaluate_volume(model, ref: torch.Tensor, lr: torch.Tensor = None, isotropic: bool = False, axis: int = 2, val_range: float = None,
                    batch_size: int = 16, use_amp: bool = False, use_graph: bool = True, graph_cache: dict = None, mask=None,
                    mask_close: int = 0, mask_largest: bool = False, mask_fill_holes=None, tissue_dice: int = 0, tissue_surface: bool = False,
                    spacing=None, tissue_edges: bool = False, edge_radius: float = 4.0, edge_bin: float = 0.5, zerofill: str = None,
                    degrade: str = "mean") -> "VolumeScores":
    """Scores the U-Net and the interpolation baselines against the ground truth ``ref`` (float32 CUDA volume).

    The doubled axes are all three with ``isotropic``, else the two in-plane axes of the slices across ``axis``.  ``lr=None``
    derives the low-resolution volume with ``downsample2`` over them (a trailing voxel of ``ref`` is cropped, and logged, where
    an extent is odd); a given ``lr`` must have exactly half of ``ref``'s extents on the doubled axes.  ``val_range=None`` is
    ``ref.max() - ref.min()`` (of the cropped volume).  Returns ``{method: (5,) float64 CUDA tensor}`` in the order ``unet``
    (``enhance_volume`` or ``enhance_volume_isotropic``, float32), ``unet_axis2_linear`` (``isotropic`` only:
    ``enhance_volume_isotropic(planes=(2,))``, the single-pass alternative to the blend), ``linear``, ``cubic`` (``upscale2`` of
    the same ``lr`` over the same axes), then ``zerofill`` on request (below).

    ``mask``: ``None``, ``"otsu"`` (``foreground_mask`` of the cropped REFERENCE volume with ``close_radius=mask_close``, taken once
    and shared by every method) or a uint8 / bool CUDA tensor of ``ref``'s shape (it gets the reference's crop; ``mask_close`` is
    applied to it as well, with a log line).  With a mask every value is the (2, 5) tensor of ``volume_metrics(mask=...)`` - row 0 the whole
    volume, row 1 the foreground - and the returned ``VolumeScores`` carries ``.mask``, ``.mask_count`` and ``.mask_stats``.
    Without one nothing changes.  ``mask_largest`` / ``mask_fill_holes`` (``"3d"`` or an axis 0..2) clean the mask after the closing,
    ``"otsu"`` and a given tensor alike (``foreground_mask``'s ``largest`` / ``fill_holes``); ``.mask_cleanup`` then holds what they
    found.  Both need a mask.

    ``tissue_dice`` K in 2..6 (0: off; needs a mask): the reference and every method's output are segmented into K tissue classes
    inside the mask (``volume_tissue.segment_tissue``, the reference once) and ``.tissue_dice`` is ``{method: (K,) float64 numpy array}``,
    the Dice overlap of the method's classes with the reference's.  A last method ``reference`` - the reference scored against itself,
    Dice 1 for every class it has - is then added as the check of the whole path.

    ``tissue_surface`` (needs ``tissue_dice``): ``.tissue_surface`` is ``{method: SurfaceDistances}``, the surface distances per class
    between the tissue interfaces of the label volumes already made for Dice (``volume_surface.surface_distances`` with
    ``background=False``: the mask's outer rim is the same on both sides), in the unit of ``spacing``, the three voxel sizes (None: 1).

    ``tissue_edges`` (needs ``tissue_dice``): ``.tissue_edges`` is ``{method: EdgeSharpness}``, the 10 % - 90 % width and the contrast of
    every method's output across the ``tissue_dice - 1`` interfaces between the tissue classes of the REFERENCE's label volume
    (``volume_sharpness``): the signed distances to them are taken once, with ``spacing``, and each output and the ``reference`` row get
    one ``edge_profile`` pass with ``edge_radius`` and ``edge_bin`` in the unit of ``spacing``.

    ``zerofill`` (``"none"`` or ``"hamming"``, the k-space window; None: off): a method ``zerofill`` (``zerofill_hamming``) is scored
    after ``cubic`` - ``volume_kspace.zerofill2`` of the same ``lr`` over the same axes, what a scanner's interpolated matrix shows -
    with everything the other rows get.  ``degrade`` (``"mean"``, ``"kspace"`` or ``"kspace_hamming"``): with a k-space setting the
    low-resolution volume derived from ``ref`` is ``volume_kspace.truncate2`` of it, the degradation of the 2-D training path, in place
    of ``downsample2``; a given ``lr`` is taken as it is, with one warning.  Both defaults leave a run as it was."""
    # the checks that need no data come first, the device check after them
    if not isinstance(ref, torch.Tensor) or ref.dtype != torch.float32 or ref.dim() != 3 or ref.numel() == 0:
        raise ValueError(f"expected a non-empty float32 volume (X,Y,Z), got {getattr(ref, 'dtype', type(ref))} "
                         f"{tuple(getattr(ref, 'shape', ()))}")
    if axis not in (0, 1, 2):
        raise ValueError(f"axis must be 0, 1 or 2, got {axis}")
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    if val_range is not None and not val_range > 0:
        raise ValueError(f"val_range must be positive, got {val_range}")
    if zerofill is not None or degrade != "mean":
        from .volume_kspace import truncate2, zerofill2
        if zerofill not in (None, "none", "hamming"):
            raise ValueError(f"zerofill must be None, 'none' or 'hamming', got {zerofill!r}")
        if degrade not in ("mean", "kspace", "kspace_hamming"):
            raise ValueError(f"degrade must be 'mean', 'kspace' or 'kspace_hamming', got {degrade!r}")
    if tissue_dice != 0:
        from .volume_tissue import TissueWorkspace, dice, label_confusion, segment_tissue
        check_classes(tissue_dice)
        if mask is None:
            raise ValueError("tissue_dice needs a mask")
    if tissue_surface:
        from .volume_surface import SurfaceWorkspace, surface_distances
        if not tissue_dice:
            raise ValueError("tissue_surface needs tissue_dice")
        spacing = (1.0, 1.0, 1.0) if spacing is None else spacing
        check_spacing(spacing)
    if tissue_edges:
        from .volume_sharpness import EdgeWorkspace, check_bins, edge_sharpness, signed_distances
        if not tissue_dice:
            raise ValueError("tissue_edges needs tissue_dice")
        spacing = (1.0, 1.0, 1.0) if spacing is None else spacing
        check_spacing(spacing)
        edge_bins = check_bins(edge_radius, edge_bin)[2]
    if spacing is not None and not (tissue_surface or tissue_edges):
        raise ValueError("spacing needs tissue_surface")
    if mask is None:
        if mask_close != 0:
            raise ValueError("mask_close needs a mask")
        if mask_largest or mask_fill_holes is not None:
            raise ValueError("mask_largest and mask_fill_holes need a mask")
    else:
        _check_radius(mask_close)
        fill = _check_fill(mask_fill_holes)
        if isinstance(mask, str):
            if mask != "otsu":
                raise ValueError(f"mask must be None, 'otsu' or a tensor, got {mask!r}")
        elif not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool) or tuple(mask.shape) != tuple(ref.shape):
            raise ValueError(f"mask must be None, 'otsu' or a uint8 / bool tensor of the reference's shape {tuple(ref.shape)}, got "
                             f"{getattr(mask, 'dtype', type(mask).__name__)} {tuple(getattr(mask, 'shape', ()))}")
    axes = (0, 1, 2) if isotropic else tuple(a for a in (0, 1, 2) if a != axis)
    if lr is not None:
        want = tuple(d // 2 if a in axes else d for a, d in enumerate(ref.shape))
        if lr.dtype != torch.float32 or tuple(lr.shape) != want or any(ref.shape[a] % 2 for a in axes):
            raise ValueError(f"lr must be a float32 volume with exactly half of the reference's extents {tuple(ref.shape)} on the "
                             f"axes {axes} ({want}), got {lr.dtype} {tuple(lr.shape)}")
        _need_cuda(lr, "evaluate_volume")
    crop = tuple(d - d % 2 if a in axes else d for a, d in enumerate(ref.shape))
    if 0 in crop:
        raise ValueError(f"nothing is left of the reference volume {tuple(ref.shape)} after cropping to even extents")
    _need_cuda(ref, "evaluate_volume")
    if isinstance(mask, torch.Tensor):
        _need_cuda(mask, "evaluate_volume")
    if lr is None:
        if crop != tuple(ref.shape):
            logger.warning(f"Reference volume {tuple(ref.shape)} has an odd extent on a doubled axis: cropped to {crop}.")
            ref = ref[:crop[0], :crop[1], :crop[2]]
            if isinstance(mask, torch.Tensor):
                mask = mask[:crop[0], :crop[1], :crop[2]]
        ref = ref.contiguous()
        lr = downsample2(ref, axes) if degrade == "mean" else truncate2(ref, axes, "hamming" if degrade == "kspace_hamming" else "none")
    else:
        if degrade != "mean":
            _warn_degrade_ignored(degrade)
        ref, lr = ref.contiguous(), lr.contiguous()
    if val_range is None:
        val_range = float((ref.max() - ref.min()).item())
    if not val_range > 0:
        raise ValueError(f"the data range must be positive, got {val_range} (a constant reference volume?)")
    graphs = graph_cache if graph_cache is not None else {}
    common = dict(batch_size=batch_size, use_amp=use_amp, use_graph=use_graph, graph_cache=graphs)
    results = VolumeScores()
    score = {}                                                    # the mask, once per volume, for every method
    if mask is not None:
        if isinstance(mask, str):
            score["mask"], results.mask_stats = foreground_mask(ref, mask_close, bool(mask_largest), mask_fill_holes)
            results.mask_cleanup = results.mask_stats.cleanup
        else:
            if mask_close:
                logger.info(f"Closing the given mask with radius {mask_close}.")
            closed = binary_close(_check_mask(mask, ref.shape, "evaluate_volume"), mask_close)
            score["mask"], results.mask_cleanup = _clean_mask(closed, bool(mask_largest), fill)
        results.mask = score["mask"]
    if tissue_dice:
        tissue_ws = TissueWorkspace(ref.shape, tissue_dice, ref.device)
        ref_labels = segment_tissue(ref, score["mask"], tissue_dice, workspace=tissue_ws).labels.clone()
        results.tissue_dice = {}
    if tissue_surface:
        surface_ws = SurfaceWorkspace(ref.shape, tissue_dice, ref.device)
        results.tissue_surface = {}
    if tissue_edges:
        edge_ws = EdgeWorkspace(tissue_dice - 1, edge_bins, ref.device)
        ref_sdist = signed_distances(ref_labels, tissue_dice, spacing)
        results.tissue_edges = {}

    def scored(method, out):
        results[method] = volume_metrics(out, ref, val_range, **score)
        if tissue_dice:
            labels = segment_tissue(out.contiguous(), score["mask"], tissue_dice, workspace=tissue_ws).labels
            results.tissue_dice[method] = dice(label_confusion(labels, ref_labels, score["mask"], tissue_dice))
            if tissue_surface:
                results.tissue_surface[method] = surface_distances(labels, ref_labels, tissue_dice, spacing, False, surface_ws)
            if tissue_edges:
                results.tissue_edges[method] = edge_sharpness(out.contiguous(), radius=edge_radius, bin_width=edge_bin, workspace=edge_ws,
                                                              sdist=ref_sdist)

    if isotropic:
        scored("unet", enhance_volume_isotropic(model, lr, **common))
        scored("unet_axis2_linear", enhance_volume_isotropic(model, lr, planes=(2,), **common))
    else:
        scored("unet", enhance_volume(model, lr, axis=axis, **common))
    for method in ("linear", "cubic"):
        scored(method, upscale2(lr, method, axes))
    if zerofill is not None:
        scored("zerofill" if zerofill == "none" else f"zerofill_{zerofill}", zerofill2(lr, axes, zerofill))
    if tissue_dice:
        scored("reference", ref)
    if mask is not None:
        results.mask_count = results["unet"].mask_count
    return results
