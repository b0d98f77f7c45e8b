"""Reslicing of whole volumes between voxel grids through an affine, on the device (extension): the
operation that brings a scan onto another scan's grid - another spacing, field of view, axis order or rotation - from the two
NIfTI affines alone.

``reslice_np``        the specification: every rounding fixed, so that the kernel (``csrc/volume_reslice.hip``) is bit-equal to it.
``reslice_mask_np``   its ``nearest`` rule on uint8 volumes.
``reslice``           (X,Y,Z) float32 CUDA tensor, (3, 4) matrix -> the volume on the destination grid; one launch.
``reslice_mask``      the same for uint8 / bool masks (``nearest``).
``reslice_like``      ``reslice`` with the matrix of two index -> world affines (``utils.nifti.grid_matrix``).

The matrix ``m`` maps a destination voxel index ``(i, j, k)`` to a continuous source voxel index.  Voxels are cells with their
centres at the integer indices (the half-pixel convention of ``utils.nifti.upscaled_affine``): the volume covers
``[-0.5, n - 0.5]`` along an axis of extent ``n``; a destination voxel whose centre falls outside is ``fill``, one inside is
interpolated with the border replicated.  There is no CPU path: CPU tensors raise.  The affines are taken as they are here;
``volume_register`` estimates a rigid transform between two scans.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._volume_args import MAX_VOXELS, check_matrix, check_shape, cuda_tensor, matrix_arg, volume_np      # noqa: F401  (MAX_VOXELS: this module's documented limit)
from .utils.nifti import grid_matrix

METHODS = {"nearest": L.RESAMPLE_NEAREST, "linear": L.RESAMPLE_LINEAR, "cubic": L.RESAMPLE_CUBIC}


# ---------------------------------------------------------------- numpy specification

def source_coordinates_np(m, out_shape, src_shape):
    """-> (p, inside): the three float64 coordinate arrays ``p_a = ((m[a,0] i + m[a,1] j) + m[a,2] k) + m[a,3]``, one rounded
    operation at a time (numpy never fuses), and the inside test ``-0.5 <= p_a <= n_a - 0.5`` on all three axes."""
    m = check_matrix(m)
    i, j, k = (np.arange(n, dtype=np.float64).reshape([-1 if a == b else 1 for b in range(3)]) for a, n in enumerate(out_shape))
    p = [np.broadcast_to(((m[a, 0] * i + m[a, 1] * j) + m[a, 2] * k) + m[a, 3], out_shape) for a in range(3)]
    inside = np.ones(out_shape, dtype=bool)
    for a in range(3):
        inside &= (p[a] >= -0.5) & (p[a] <= src_shape[a] - 0.5)
    return p, inside


def keys_weight_np(x: np.ndarray) -> np.ndarray:
    """Keys' cubic kernel with A = -0.75 at the float32 distances ``x >= 0``, every operation rounded to float32."""
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    near = ((f32(1.25) * x - f32(2.25)) * x) * x + f32(1)
    far = ((f32(-0.75) * x + f32(3.75)) * x - f32(6)) * x + f32(3)
    return np.where(x <= f32(1), near, far).astype(f32)


def taps_np(p, n, method):
    """p: the float64 coordinates of the inside voxels along one axis -> ([index arrays], [float32 weight arrays])."""
    f32 = np.float32
    f = np.floor(p)
    t = (p - f).astype(f32)                                      # the difference is exact in double
    fi = f.astype(np.int64)
    if method == "linear":
        return [np.clip(fi + d, 0, n - 1) for d in (0, 1)], [f32(1) - t, t]
    return ([np.clip(fi + d, 0, n - 1) for d in (-1, 0, 1, 2)],
            [keys_weight_np(f32(1) + t), keys_weight_np(t), keys_weight_np(f32(1) - t), keys_weight_np(f32(2) - t)])


def weighted_sum_np(w, v):
    acc = w[0] * v[0]                                            # float32 arrays: every product and sum rounds to float32
    for wd, vd in zip(w[1:], v[1:]):
        acc = acc + wd * vd
    return acc


def sample_np(volumes, p, method):
    """The sampler of every volume tool.  ``volumes``: float32 volumes of one shape ``(X, Y, Z)``; ``p``: the three float64 coordinate
    arrays of the selected voxels (all inside, or clamped into the volume) -> one float32 array per volume: ``taps_np`` along
    every axis, computed once for all volumes, the taps reduced along z, then y, then x with ``weighted_sum_np``."""
    (ix, wx), (iy, wy), (iz, wz) = (taps_np(pa, n, method) for pa, n in zip(p, volumes[0].shape))
    return [weighted_sum_np(wx, [weighted_sum_np(wy, [weighted_sum_np(wz, [v[xa, yb, zc] for zc in iz]) for yb in iy]) for xa in ix])
            for v in volumes]


def reslice_np(v: np.ndarray, m, out_shape, method: str = "linear", fill: float = 0.0) -> np.ndarray:
    """The specification of ``reslice``.  ``v``: float32 (X, Y, Z); ``m``: (3, 4) float64, destination index -> source index.

    Coordinate and inside test: ``source_coordinates_np``; a voxel outside is ``fill`` and nothing of it is converted to an
    integer.  ``nearest``: index ``clip(floor(p_a + 0.5), 0, n_a - 1)``.  ``linear``: ``f_a = floor(p_a)``,
    ``t_a = float32(p_a - f_a)``, weights ``(1 - t_a, t_a)`` in float32 on the taps ``f_a, f_a + 1``.  ``cubic``: taps
    ``f_a - 1 .. f_a + 2``, weights ``keys_weight_np`` at the distances ``1 + t, t, 1 - t, 2 - t`` (not renormalised; exactly
    (0, 1, 0, 0) at ``t = 0``).  Taps are clamped to the volume.  Reduction along z, then y, then x, each stage
    ``((w0 v0 + w1 v1) + w2 v2) + w3 v3`` in float32."""
    v = volume_np(v, "reslice_np")
    if method not in METHODS:
        raise ValueError(f"Unknown interpolation method: {method}")
    out_shape = check_shape(out_shape, "out_shape")
    p, inside = source_coordinates_np(m, out_shape, v.shape)
    out = np.full(out_shape, np.float32(fill), dtype=np.float32)
    pin = [pa[inside] for pa in p]
    if method == "nearest":
        q = [np.clip(np.floor(pa + 0.5).astype(np.int64), 0, n - 1) for pa, n in zip(pin, v.shape)]
        out[inside] = v[q[0], q[1], q[2]]
        return out
    out[inside] = sample_np([v], pin, method)[0]
    return out


def reslice_mask_np(mask: np.ndarray, m, out_shape, fill: int = 0) -> np.ndarray:
    """The ``nearest`` rule of ``reslice_np`` on a uint8 volume."""
    mask = np.asarray(mask)
    if mask.dtype != np.uint8 or mask.ndim != 3 or mask.size == 0:
        raise ValueError(f"reslice_mask_np: expected a non-empty uint8 volume (X,Y,Z), got {mask.dtype} {mask.shape}")
    out_shape = check_shape(out_shape, "out_shape")
    p, inside = source_coordinates_np(m, out_shape, mask.shape)
    out = np.full(out_shape, _check_fill_u8(fill), dtype=np.uint8)
    q = [np.clip(np.floor(pa[inside] + 0.5).astype(np.int64), 0, n - 1) for pa, n in zip(p, mask.shape)]
    out[inside] = mask[q[0], q[1], q[2]]
    return out


def _check_fill_u8(fill) -> int:
    if isinstance(fill, bool) or int(fill) != fill or not 0 <= int(fill) <= 255:
        raise ValueError(f"the fill of a uint8 volume must be an integer in 0..255, got {fill!r}")
    return int(fill)


# ---------------------------------------------------------------- device

def reslice(vol: torch.Tensor, m, out_shape, method: str = "linear", fill: float = 0.0) -> torch.Tensor:
    """vol: contiguous (X,Y,Z) float32 CUDA tensor; m: (3, 4) matrix, destination index -> source index (host, float64) -> the
    float32 CUDA volume of ``out_shape``, bit-equal to ``reslice_np``.  One launch, no host synchronisation."""
    if method not in METHODS:
        raise ValueError(f"Unknown interpolation method: {method}")
    v = cuda_tensor(vol, (torch.float32,), "reslice", ndim=3, limit=True)
    out_shape = check_shape(out_shape, "out_shape")
    out = torch.empty(out_shape, dtype=torch.float32, device=v.device)
    L.call("mrisr_f32_volume_reslice", v.data_ptr(), *v.shape, out.data_ptr(), *out_shape, matrix_arg(m), METHODS[method], float(fill),
           L.stream_ptr(), nbytes=4 * (v.numel() + out.numel()))
    return out


def reslice_mask(mask: torch.Tensor, m, out_shape, fill: int = 0) -> torch.Tensor:
    """mask: contiguous (X,Y,Z) uint8 or bool CUDA tensor -> the uint8 CUDA volume of ``out_shape`` under the ``nearest`` rule,
    bit-equal to ``reslice_mask_np``.  One launch, no host synchronisation."""
    k = cuda_tensor(mask, (torch.uint8, torch.bool), "reslice_mask", ndim=3, limit=True)
    if k.dtype == torch.bool:
        k = k.view(torch.uint8)
    out_shape = check_shape(out_shape, "out_shape")
    out = torch.empty(out_shape, dtype=torch.uint8, device=k.device)
    L.call("mrisr_u8_volume_reslice_nearest", k.data_ptr(), *k.shape, out.data_ptr(), *out_shape, matrix_arg(m), _check_fill_u8(fill),
           L.stream_ptr(), nbytes=k.numel() + out.numel())
    return out


def reslice_like(vol: torch.Tensor, src_affine, dst_affine, dst_shape, method: str = "linear", fill: float = 0.0) -> torch.Tensor:
    """``vol`` on the grid ``(dst_affine, dst_shape)``: ``reslice`` with ``grid_matrix(src_affine, dst_affine)``; the two affines
    map voxel indices to world coordinates (``NiftiHeader.affine()``).  A uint8 / bool ``vol`` goes through ``reslice_mask``."""
    m = grid_matrix(src_affine, dst_affine)
    if isinstance(vol, torch.Tensor) and vol.dtype in (torch.uint8, torch.bool):
        if method != "nearest":
            raise ValueError(f"a uint8 volume is resliced with 'nearest', got {method!r}")
        return reslice_mask(vol, m, dst_shape, fill)
    return reslice(vol, m, dst_shape, method, fill)


def covered_share(src_shape, m, out_shape, device="cuda") -> torch.Tensor:
    """0-d float64 CUDA tensor: the share of the destination voxels whose centre lies inside the source volume - ``reslice_mask``
    of an all-ones mask, counted on the device."""
    ones = torch.ones(check_shape(src_shape, "src_shape"), dtype=torch.uint8, device=device)
    hit = reslice_mask(ones, m, out_shape)
    return hit.count_nonzero().to(torch.float64) / hit.numel()
