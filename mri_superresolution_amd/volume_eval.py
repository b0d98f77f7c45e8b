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
``evaluate_volume``  U-Net against the baselines on one ground-truth volume.

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


def volume_metrics_np(pred: np.ndarray, ref: np.ndarray, val_range: float, window_size: int = 11, sigma: float = 1.5) -> np.ndarray:
    """(ssim, mse, rmse, mae, psnr) of two volumes in float64: the specification of ``volume_metrics``."""
    a, b = np.asarray(pred, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 3 or a.size == 0:
        raise ValueError(f"expected two non-empty volumes of one shape, got {a.shape} and {b.shape}")
    if not val_range > 0:
        raise ValueError(f"val_range must be positive, got {val_range}")
    d = a - b
    mse, mae = float(np.mean(d * d)), float(np.mean(np.abs(d)))
    ssim = float(np.mean(ssim_map_np(a, b, val_range, window_size, sigma)))
    psnr = 100.0 if mse < 1e-10 else 10.0 * np.log10(float(val_range) ** 2 / mse)
    return np.array([ssim, mse, np.sqrt(mse), mae, psnr], dtype=np.float64)


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


def volume_metrics(pred: torch.Tensor, ref: torch.Tensor, val_range: float, window_size: int = 11, sigma: float = 1.5) -> torch.Tensor:
    """pred, ref: (X,Y,Z) float32 CUDA tensors -> (5,) float64 CUDA tensor, columns ``METRIC_COLUMNS`` (ssim, mse, rmse, mae,
    psnr; PSNR = 10 log10(val_range^2 / mse), 100 when mse < 1e-10).  No host synchronisation."""
    _check_window(window_size)
    a, b = _check_vol(pred, "volume_metrics"), _check_vol(ref, "volume_metrics")
    if a.shape != b.shape:
        raise ValueError(f"shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
    if not (val_range > 0 and sigma > 0):
        raise ValueError(f"val_range and sigma must be positive, got {val_range} and {sigma}")
    st = L.stream_ptr()
    sums = torch.zeros(3, dtype=torch.float64, device=a.device)
    out = torch.empty(5, dtype=torch.float64, device=a.device)
    L.call("mrisr_f32_volume_metrics", a.data_ptr(), b.data_ptr(), *a.shape, float(val_range), float(sigma), int(window_size),
           sums.data_ptr(), st, nbytes=8 * a.numel())      # the two fp32 volumes once
    L.call("mrisr_volume_metrics_finalize", sums.data_ptr(), *a.shape, float(val_range), out.data_ptr(), st)
    return out


def evaluate_volume(model, ref: torch.Tensor, lr: torch.Tensor = None, isotropic: bool = False, axis: int = 2, val_range: float = None,
                    batch_size: int = 16, use_amp: bool = False, use_graph: bool = True, graph_cache: dict = None) -> "OrderedDict":
    """Scores the U-Net and the interpolation baselines against the ground truth ``ref`` (float32 CUDA volume).

    The doubled axes are all three with ``isotropic``, else the two in-plane axes of the slices across ``axis``.  ``lr=None``
    derives the low-resolution volume with ``downsample2`` over them (a trailing voxel of ``ref`` is cropped, and logged, where
    an extent is odd); a given ``lr`` must have exactly half of ``ref``'s extents on the doubled axes.  ``val_range=None`` is
    ``ref.max() - ref.min()`` (of the cropped volume).  Returns ``{method: (5,) float64 CUDA tensor}`` in the order ``unet``
    (``enhance_volume`` or ``enhance_volume_isotropic``, float32), ``unet_axis2_linear`` (``isotropic`` only:
    ``enhance_volume_isotropic(planes=(2,))``, the single-pass alternative to the blend), ``linear``, ``cubic`` (``upscale2`` of
    the same ``lr`` over the same axes)."""
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
    if lr is None:
        if crop != tuple(ref.shape):
            logger.warning(f"Reference volume {tuple(ref.shape)} has an odd extent on a doubled axis: cropped to {crop}.")
            ref = ref[:crop[0], :crop[1], :crop[2]]
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
    results = OrderedDict()
    if isotropic:
        results["unet"] = volume_metrics(enhance_volume_isotropic(model, lr, **common), ref, val_range)
        results["unet_axis2_linear"] = volume_metrics(enhance_volume_isotropic(model, lr, planes=(2,), **common), ref, val_range)
    else:
        results["unet"] = volume_metrics(enhance_volume(model, lr, axis=axis, **common), ref, val_range)
    for method in ("linear", "cubic"):
        results[method] = volume_metrics(upscale2(lr, method, axes), ref, val_range)
    return results
