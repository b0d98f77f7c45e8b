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
``evaluate_volume``  U-Net against the baselines on one ground-truth volume, optionally inside a foreground mask.

There is no CPU path: CPU tensors raise.  The ``*_np`` functions are the specifications the kernels are tested against.
"""
from __future__ import annotations

import logging
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
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

def _check_np(v, what):
    v = np.asarray(v)
    if v.dtype != np.float32 or v.ndim != 3 or v.size == 0:
        raise ValueError(f"{what}: expected a non-empty float32 volume (X,Y,Z), got {v.dtype} {v.shape}")
    return v


def downsample2_np(v: np.ndarray, axes=(0, 1, 2)) -> np.ndarray:
    """Mean over pairs along ``axes``: for the axes in ascending order ``v = v[even] + v[odd]`` (float32), then one product with
    ``0.5 ** len(axes)`` (exact).  An odd extent on one of the axes is a ``ValueError``."""
    v = _check_np(v, "downsample2_np")
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
    v = _check_np(v, "upscale2_np")
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
    v = _check_np(v, "otsu_bins_np")
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


def foreground_mask_np(v: np.ndarray, close_radius: int = 0, return_stats: bool = False):
    """The specification of ``foreground_mask``: ``mask = bin(v) > t*`` (uint8, 0 / 1) with the bins of ``otsu_bins_np`` and the
    ``t*`` of ``otsu_threshold_np`` on their counts - an integer comparison, exactly consistent with the histogram - then, for
    ``close_radius`` r in 1..4, the closing ``erode_np(dilate_np(mask, r), r)``.  A degenerate range gives ``t* = -1`` and a mask of
    ones.  ``return_stats``: -> (mask, dict(lo, hi, t, count, counts)), the count and the 256 counts those of the Otsu mask
    before the closing."""
    r = _check_radius(close_radius)
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


def foreground_mask(vol: torch.Tensor, close_radius: int = 0):
    """vol: (X,Y,Z) float32 CUDA tensor -> (mask uint8 CUDA tensor, stats (4,) float64 CUDA tensor: lo, hi, t*, and the foreground
    count of the Otsu mask before the closing).  Bit-equal to ``foreground_mask_np``.  No host synchronisation."""
    r = _check_radius(close_radius)
    mask, stats, _ = otsu_mask(vol)
    return binary_close(mask, r), stats


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
    ``mask_stats`` (``foreground_mask``'s (4,) float64 CUDA tensor lo, hi, t*, count for ``"otsu"``); all three ``None`` otherwise."""

    def __init__(self):
        super().__init__()
        self.mask = self.mask_count = self.mask_stats = None


def evaluate_volume(model, ref: torch.Tensor, lr: torch.Tensor = None, isotropic: bool = False, axis: int = 2, val_range: float = None,
                    batch_size: int = 16, use_amp: bool = False, use_graph: bool = True, graph_cache: dict = None, mask=None,
                    mask_close: int = 0) -> "VolumeScores":
    """Scores the U-Net and the interpolation baselines against the ground truth ``ref`` (float32 CUDA volume).

    The doubled axes are all three with ``isotropic``, else the two in-plane axes of the slices across ``axis``.  ``lr=None``
    derives the low-resolution volume with ``downsample2`` over them (a trailing voxel of ``ref`` is cropped, and logged, where
    an extent is odd); a given ``lr`` must have exactly half of ``ref``'s extents on the doubled axes.  ``val_range=None`` is
    ``ref.max() - ref.min()`` (of the cropped volume).  Returns ``{method: (5,) float64 CUDA tensor}`` in the order ``unet``
    (``enhance_volume`` or ``enhance_volume_isotropic``, float32), ``unet_axis2_linear`` (``isotropic`` only:
    ``enhance_volume_isotropic(planes=(2,))``, the single-pass alternative to the blend), ``linear``, ``cubic`` (``upscale2`` of
    the same ``lr`` over the same axes).

    ``mask``: ``None``, ``"otsu"`` (``foreground_mask`` of the cropped REFERENCE volume with ``close_radius=mask_close``, taken once
    and shared by every method) or a uint8 / bool CUDA tensor of ``ref``'s shape (it gets the reference's crop; ``mask_close`` is
    applied to it as well, with a log line).  With a mask every value is the (2, 5) tensor of ``volume_metrics(mask=...)`` - row 0 the whole
    volume, row 1 the foreground - and the returned ``VolumeScores`` carries ``.mask``, ``.mask_count`` and ``.mask_stats``.
    Without one nothing changes."""
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
    if mask is None:
        if mask_close != 0:
            raise ValueError("mask_close needs a mask")
    else:
        _check_radius(mask_close)
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
        lr = downsample2(ref, axes)
    else:
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
            score["mask"], results.mask_stats = foreground_mask(ref, mask_close)
        else:
            if mask_close:
                logger.info(f"Closing the given mask with radius {mask_close}.")
            score["mask"] = binary_close(_check_mask(mask, ref.shape, "evaluate_volume"), mask_close)
        results.mask = score["mask"]
    if isotropic:
        results["unet"] = volume_metrics(enhance_volume_isotropic(model, lr, **common), ref, val_range, **score)
        results["unet_axis2_linear"] = volume_metrics(enhance_volume_isotropic(model, lr, planes=(2,), **common), ref, val_range, **score)
    else:
        results["unet"] = volume_metrics(enhance_volume(model, lr, axis=axis, **common), ref, val_range, **score)
    for method in ("linear", "cubic"):
        results[method] = volume_metrics(upscale2(lr, method, axes), ref, val_range, **score)
    if mask is not None:
        results.mask_count = results["unet"].mask_count
    return results
