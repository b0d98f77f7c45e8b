"""Rician non-local-means denoising of volumes on the device (extension): noise is the defining property of
low-field MR, and the Rician bias lifts the dark regions of a magnitude image.  The 3-D non-local-means filter (Buades; Coupe et
al. 2008) with the Rician correction on the squared signal (Wiest-Daessle et al. 2008), sigma from the air around the head, whose
magnitude follows a Rayleigh distribution.  Patch radius 1 (27 voxels), search radius ``R`` in 1..5.

``WEIGHT_TABLE``                       ``float32(exp(-(k + 0.5) / 256))``, k = 0..4095, float64 on the host: the device never
                                       evaluates an exponential, which is what lets it equal numpy bit for bit.
``patch_distance_np``, ``denoise_np``, ``noise_params_np``, ``estimate_sigma_np``, ``background_mask_np``   the specification:
                                       float32, every product, sum, division and square root rounded on its own (no fma), the
                                       candidates of a voxel in ascending ``(t0, t1, t2)`` order.
``denoise``, ``noise_params``, ``estimate_noise``, ``background_mask``, ``denoise_volume``   the device path
                                       (``csrc/volume_denoise.hip``); ``denoise`` equals ``denoise_np`` bit for bit.  There is no CPU
                                       path: CPU tensors raise.  The filter's parameters live in a device float32[4] tensor
                                       ``params = (inv_h2, two_sigma2, sigma, beta)``, so nothing needs a host read.

Not built: the block-wise / preselection speed-ups, a patch radius other than 1, spatially varying sigma, a 2-D form for
``scripts/evaluate.py``.
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import torch

from . import _lib as L
from ._volume_args import cuda_tensor, mask_np, mask_tensor, out_like, volume_np
from .volume_eval import binary_dilate, dilate_np, foreground_mask, foreground_mask_np

MAX_RADIUS = 5
TABLE_SIZE = 4096
PATCH_VOXELS = 27
MIN_BACKGROUND = 1000          # denoise_volume(check=True): fewer background voxels are no estimate of sigma
WEIGHT_TABLE = np.exp(-(np.arange(TABLE_SIZE, dtype=np.float64) + 0.5) / 256.0).astype(np.float32)
WEIGHT_TABLE.setflags(write=False)


def _check_radius(radius) -> int:
    if not isinstance(radius, (int, np.integer)) or isinstance(radius, bool) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"the search radius is an integer in 1..{MAX_RADIUS}, got {radius!r}")
    return int(radius)


def _check_beta(beta) -> float:
    beta = float(beta)
    if not (math.isfinite(beta) and beta > 0):
        raise ValueError(f"beta must be finite and positive, got {beta!r}")
    return beta


def _check_volume_np(v, what):
    return np.ascontiguousarray(volume_np(v, what))


def offsets(radius: int):
    """Every ``t != 0`` with ``|t_i| <= radius`` in ascending ``(t0, t1, t2)`` order: ``(2 radius + 1)^3 - 1`` candidates."""
    r = range(-radius, radius + 1)
    return [t for t in itertools.product(r, r, r) if t != (0, 0, 0)]


# ---------------------------------------------------------------- numpy specification

def _box3_np(a, axis):
    """``(a[i - 1] + a[i]) + a[i + 1]`` along ``axis``: the result is two shorter there."""
    n = a.shape[axis]
    s = [[slice(None)] * 3 for _ in range(3)]
    for k in range(3):
        s[k][axis] = slice(k, n - 2 + k)
    return (a[tuple(s[0])] + a[tuple(s[1])]) + a[tuple(s[2])]


def _distance_np(padded, shape, reach, t):
    """``padded``: the volume edge-replicated by ``reach >= max|t_i| + 1`` on every side -> ``d`` of ``patch_distance_np``."""
    n0, n1, n2 = shape
    a = padded[reach - 1:reach + n0 + 1, reach - 1:reach + n1 + 1, reach - 1:reach + n2 + 1]
    b = padded[reach - 1 + t[0]:reach + n0 + 1 + t[0], reach - 1 + t[1]:reach + n1 + 1 + t[1], reach - 1 + t[2]:reach + n2 + 1 + t[2]]
    with np.errstate(all="ignore"):
        diff = a - b
        return _box3_np(_box3_np(_box3_np(diff * diff, 2), 1), 0)


def patch_distance_np(v, t) -> np.ndarray:
    """float32, the shape of ``v``: the squared distance of the 3 x 3 x 3 patches around ``p`` and ``p + t``.  ``c(p)`` clamps every
    coordinate into the volume (edge replication); ``sq(p) = (v[c(p)] - v[c(p + t)])^2``,
    ``row(p) = (sq(p - e2) + sq(p)) + sq(p + e2)``, ``plane(p) = (row(p - e1) + row(p)) + row(p + e1)``,
    ``d(p) = (plane(p - e0) + plane(p)) + plane(p + e0)``.  The nested loop over the patch, the separable box sum and a running
    window of three plane sums along axis 0 all add in this order, so all three give these bits."""
    v = _check_volume_np(v, "patch_distance_np")
    t = tuple(int(x) for x in t)
    if len(t) != 3:
        raise ValueError(f"an offset has three components, got {t!r}")
    reach = max(abs(x) for x in t) + 1
    return _distance_np(np.pad(v, reach, mode="edge"), v.shape, reach, t)


def _check_scalar_f32(x, what):
    x = np.float32(x)
    if np.isnan(x) or x < 0:
        raise ValueError(f"{what} must not be negative, got {x!r}")
    return x


def weight_np(x) -> np.ndarray:
    """``WEIGHT_TABLE[int(x * 256)]`` where ``0 <= x < 16``, else 0 (NaN and inf compare false); ``x`` float32, ``x * 256`` exact."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        ok = (x >= 0) & (x < 16)
        k = np.where(ok, x * np.float32(256), np.float32(0)).astype(np.int32)
    return np.where(ok, WEIGHT_TABLE[k], np.float32(0))


def denoise_np(v, inv_h2, two_sigma2, radius=3, rician=True) -> np.ndarray:
    """float32, the shape of ``v``.  ``val = v * v`` if ``rician`` else ``v``.  For every voxel ``p`` and every candidate
    ``t`` of ``offsets(radius)`` in order: ``x = d(p) * inv_h2``; the weight is ``w = WEIGHT_TABLE[int(x * 256)]`` if
    ``0 <= x < 16`` (NaN and inf compare false; ``x * 256`` is exact) and ``p + t`` lies inside the volume, else 0; then
    ``num = num + w * val[p + t]``, ``den = den + w``, ``wmax = max(wmax, w)`` - a candidate of weight 0 adds nothing (its value may
    be inf or NaN; for a number, adding ``+-0`` to a sum that began at ``+0`` changes no bit).  The centre enters last with
    ``wc = wmax if wmax > 0 else 1``: ``num = num + wc * val[p]``, ``den = den + wc``; ``m = num / den``.  ``rician``:
    ``u = m - two_sigma2``, ``out = sqrt(u) if u > 0 else 0``; else ``out = m``.  A voxel whose own value is not finite is copied
    through.  ``inv_h2`` and ``two_sigma2`` are float32 and not negative (``noise_params_np``)."""
    v = _check_volume_np(v, "denoise_np")
    radius = _check_radius(radius)
    inv_h2, two_sigma2 = _check_scalar_f32(inv_h2, "inv_h2"), _check_scalar_f32(two_sigma2, "two_sigma2")
    n0, n1, n2 = v.shape
    reach = radius + 1
    padded = np.pad(v, reach, mode="edge")
    with np.errstate(all="ignore"):
        val_padded = padded * padded if rician else padded
        i0, i1, i2 = np.ogrid[0:n0, 0:n1, 0:n2]
        num = np.zeros(v.shape, dtype=np.float32)
        den = np.zeros(v.shape, dtype=np.float32)
        wmax = np.zeros(v.shape, dtype=np.float32)
        for t in offsets(radius):
            x = _distance_np(padded, v.shape, reach, t) * inv_h2
            inside = ((i0 + t[0] >= 0) & (i0 + t[0] < n0)) & ((i1 + t[1] >= 0) & (i1 + t[1] < n1)) & ((i2 + t[2] >= 0) & (i2 + t[2] < n2))
            w = np.where(inside, weight_np(x), np.float32(0))
            there = val_padded[reach + t[0]:reach + t[0] + n0, reach + t[1]:reach + t[1] + n1, reach + t[2]:reach + t[2] + n2]
            num = num + np.where(w > 0, w * np.where(w > 0, there, np.float32(0)), np.float32(0))
            den = den + w
            wmax = np.maximum(wmax, w)
        finite = np.isfinite(v)
        centre = np.where(finite, v * v if rician else v, np.float32(0))
        wc = np.where(wmax > 0, wmax, np.float32(1))
        num = num + wc * centre
        den = den + wc
        m = num / den
        if rician:
            u = m - two_sigma2
            m = np.where(u > 0, np.sqrt(np.where(u > 0, u, np.float32(0))), np.float32(0))
        return np.where(finite, m, v).astype(np.float32)


def noise_params_np(sigma, beta=1.0):
    """-> float32 ``(inv_h2, two_sigma2, sigma)``: ``s = float32(sigma)``, ``two_sigma2 = (s * s) * 2``,
    ``h2 = (two_sigma2 * float32(beta)) * 27``, ``inv_h2 = 1 / h2`` (inf for ``sigma == 0``: every weight is then 0)."""
    s = _check_scalar_f32(sigma, "sigma")
    b = np.float32(_check_beta(beta))
    with np.errstate(all="ignore"):
        two_sigma2 = (s * s) * np.float32(2)
        h2 = (two_sigma2 * b) * np.float32(PATCH_VOXELS)
        return np.float32(1) / h2, two_sigma2, s


def estimate_sigma_np(v, background):
    """-> (float32 sigma, int count).  Over the finite voxels where ``background != 0``: ``S`` the float64 sum of ``float64(v)^2``,
    ``n`` their count, ``sigma = float32(sqrt(S / (2 n)))`` - the maximum-likelihood estimate of a Rayleigh distribution, the
    magnitude of pure complex Gaussian noise.  ``n == 0``: sigma 0."""
    v = _check_volume_np(v, "estimate_sigma_np")
    keep = (mask_np(background, v.shape, "estimate_sigma_np") != 0) & np.isfinite(v)
    n = int(keep.sum())
    if n == 0:
        return np.float32(0), 0
    x = v[keep].astype(np.float64)
    return np.float32(math.sqrt(float(np.sum(x * x)) / (2.0 * n))), n


def _check_margin(margin) -> int:
    if not isinstance(margin, (int, np.integer)) or isinstance(margin, bool) or not 0 <= margin <= 4:
        raise ValueError(f"the margin is an integer in 0..4, got {margin!r}")
    return int(margin)


def background_mask_np(v, margin=3) -> np.ndarray:
    """uint8 0 / 1: the complement of ``dilate_np(foreground_mask_np(v), margin)`` - the air, ``margin`` voxels away from the head."""
    v = _check_volume_np(v, "background_mask_np")
    return (dilate_np(foreground_mask_np(v), _check_margin(margin)) == 0).astype(np.uint8)


# ---------------------------------------------------------------- device

_TABLES = {}


def _table(device) -> torch.Tensor:
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(WEIGHT_TABLE.copy()).to(device)
    return _TABLES[key]


def _check_volume(vol, what) -> torch.Tensor:
    return cuda_tensor(vol, (torch.float32,), what, ndim=3)


def _check_params(params, device, what) -> torch.Tensor:
    if not isinstance(params, torch.Tensor) or not params.is_cuda or params.dtype != torch.float32 or tuple(params.shape) != (4,) \
            or not params.is_contiguous() or params.device != device:
        raise ValueError(f"{what}: params is a contiguous float32 CUDA tensor of 4 values on {device} (noise_params, estimate_noise)")
    return params


def noise_params(sigma, beta=1.0, device="cuda") -> torch.Tensor:
    """float32[4] on ``device``: ``(inv_h2, two_sigma2, sigma, beta)`` by ``noise_params_np`` - a host computation and one upload."""
    inv_h2, two_sigma2, s = noise_params_np(sigma, beta)
    return torch.tensor([inv_h2, two_sigma2, s, np.float32(beta)], dtype=torch.float32).to(device)


def denoise(vol: torch.Tensor, params: torch.Tensor, radius=3, rician=True, out=None) -> torch.Tensor:
    """vol: contiguous float32 CUDA tensor (n0, n1, n2); params: ``(inv_h2, two_sigma2, ...)`` on the device -> ``denoise_np``, bit
    for bit.  One launch (``mrisr_f32_volume_nlm``), no device-to-host read.  ``out``: another tensor like ``vol``."""
    v = _check_volume(vol, "denoise")
    radius = _check_radius(radius)
    p = _check_params(params, v.device, "denoise")
    out = out_like(out, v, (v,), "denoise")
    L.call("mrisr_f32_volume_nlm", v.data_ptr(), *v.shape, radius, int(bool(rician)), p.data_ptr(), _table(v.device).data_ptr(),
           out.data_ptr(), L.stream_ptr(), nbytes=8 * v.numel())
    return out


def estimate_noise(vol: torch.Tensor, background: torch.Tensor, beta=1.0, params=None, sigma=None):
    """-> (params float32[4], count int64[1]), both on the device: ``estimate_sigma_np`` of ``vol`` over ``background`` (sigma within
    one float32 ulp: the float64 sums are added in another order), then ``noise_params_np(sigma, beta)`` bit for bit.  ``sigma``
    given (> 0): no sums, that sigma, count 0.  Per-workgroup partial sums in fixed slots, added in slot order: the same bits on
    every run.  Two launches, no device-to-host read."""
    v = _check_volume(vol, "estimate_noise")
    beta = _check_beta(beta)
    given = 0.0
    if sigma is not None:
        given = float(np.float32(sigma))
        if not (math.isfinite(given) and given > 0):
            raise ValueError(f"sigma must be finite and positive, got {sigma!r}")
        bg = None
    else:
        bg = mask_tensor(background, v.shape, "estimate_noise")
    params = torch.empty(4, dtype=torch.float32, device=v.device) if params is None else _check_params(params, v.device, "estimate_noise")
    count = torch.empty(1, dtype=torch.int64, device=v.device)
    ws = torch.empty(int(L.load().mrisr_f32_volume_noise_workspace_bytes()) // 8, dtype=torch.int64, device=v.device)
    L.call("mrisr_f32_volume_noise_params", v.data_ptr(), L.ptr(bg), v.numel(), beta, given, params.data_ptr(), count.data_ptr(),
           ws.data_ptr(), L.stream_ptr(), nbytes=5 * v.numel() if bg is not None else None)
    return params, count


def background_mask(vol: torch.Tensor, margin=3) -> torch.Tensor:
    """uint8 CUDA tensor, ``background_mask_np`` bit for bit: the Otsu foreground dilated by ``margin``, complemented."""
    v = _check_volume(vol, "background_mask")
    margin = _check_margin(margin)
    return binary_dilate(foreground_mask(v)[0], margin) == 0


def denoise_volume(vol: torch.Tensor, sigma=None, beta=1.0, radius=3, rician=True, margin=3, check=True, return_noise=False):
    """The whole filter on one volume -> the denoised volume (with ``return_noise``: and a dict ``sigma``, ``count``,
    ``background`` - floats / ints after a check, else the device tensors).  ``sigma`` None: estimated from the air
    (``background_mask``, ``estimate_noise``).  ``check`` makes one device-to-host read (sigma and the count) and raises
    ``ValueError`` when sigma was estimated from fewer than 1000 voxels or is not a positive finite number - a skull-stripped or
    zero-padded scan has no air to measure, and the remedy is to give ``--sigma``.  ``check=False``: no read, HIP-graph capturable
    on one stream; a sigma of 0 then returns the non-negative input (rician) or the input (gaussian)."""
    v = _check_volume(vol, "denoise_volume")
    radius, beta = _check_radius(radius), _check_beta(beta)
    bg = None
    if sigma is None:
        bg = background_mask(v, margin)
        params, count = estimate_noise(v, bg, beta)
    else:
        params, count = estimate_noise(v, None, beta, sigma=sigma)
    noise = {"sigma": params[2], "count": count[0], "background": bg}
    if check:
        got = torch.cat([params[2:3].double(), count.double()]).cpu()
        s, n = float(got[0]), int(got[1])
        if sigma is None and n < MIN_BACKGROUND:
            raise ValueError(f"only {n} background voxels (fewer than {MIN_BACKGROUND}) to estimate the noise from - a skull-stripped or "
                             "zero-padded scan has no air: give the noise level with --sigma")
        if not (math.isfinite(s) and s > 0):
            raise ValueError(f"the estimated noise level is {s:g} (the background is empty or zero-filled): give it with --sigma")
        noise.update(sigma=s, count=n)
    out = denoise(v, params, radius, rician)
    return (out, noise) if return_noise else out
