"""Whole-volume inference on the device (extension): a float32 volume in HBM -> the x2 volume in HBM.

Per chunk of ``batch_size`` slices: exact 0.5 / 99.5 percentile window of every slice (``csrc/percentile.hip``) -> normalise
-> forward -> clamp and restore to the slice's own intensity window, written straight into the output volume.  The window is
per slice, as in the reference's extraction (``utils/extraction_utils.py:118-131``); a constant slice enters the network as
zeros (``utils/preprocessing.py:143-153``) and comes back at its value.  Nothing leaves the device in between.

``enhance_volume`` doubles the two in-plane axes of the slices across one axis; ``enhance_volume_isotropic`` doubles all three:
the passes across axes 0, 1 and 2, each interpolated along its own slice axis, averaged (``csrc/volume_blend.hip``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from .utils import imageops


def _check_volume(model, vol, axis, batch_size, out_dtype, what):
    imageops._need_cuda(vol, what)
    if vol.dtype != torch.float32 or vol.dim() != 3 or vol.numel() == 0:
        raise ValueError(f"expected a non-empty float32 volume (X,Y,Z), got {vol.dtype} {tuple(vol.shape)}")
    if axis not in (0, 1, 2):
        raise ValueError(f"axis must be 0, 1 or 2, got {axis}")
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    if out_dtype not in (torch.float32, torch.int16):
        raise ValueError(f"out_dtype must be torch.float32 or torch.int16, got {out_dtype}")
    if model.training:
        raise RuntimeError(f"{what} runs the eval forward: call model.eval() first")


def _enhance_slice_major(model, vol, axis, batch_size, use_amp, use_graph, out_dtype, q_lo, q_hi, graph_cache) -> torch.Tensor:
    """The pass across ``axis`` of a checked volume as the contiguous slice-major buffer ``[S][2R][2C]``: S the extent of
    ``axis``, R and C those of the two other axes in ascending order."""
    slices = vol.movedim(axis, 0).contiguous()
    s, h, w = slices.shape
    out = torch.empty((s, 2 * h, 2 * w), dtype=out_dtype, device=vol.device)
    model.set_compute_dtype(torch.float16 if use_amp else torch.float32)   # as scripts/infer.py: the reference's autocast is fp16
    graphs = graph_cache if graph_cache is not None else {}
    with torch.no_grad():
        for i0 in range(0, s, batch_size):
            chunk = slices[i0:i0 + batch_size]
            x, lohi = imageops.normalise_percentile_f32(chunk, q_lo, q_hi, return_bounds=True)
            if use_graph and chunk.shape[0] == batch_size:
                key = (tuple(x.shape), bool(use_amp))
                if key not in graphs:
                    graphs[key] = model.graphed_forward(x)
                y = graphs[key](x)
            else:
                y = model(x)
            imageops.restore_window(y.to(torch.float32), lohi, out_dtype, out=out[i0:i0 + chunk.shape[0]].unsqueeze(1))
    return out


def enhance_volume(model, vol: torch.Tensor, axis: int = 2, batch_size: int = 16, use_amp: bool = False, use_graph: bool = True,
                   out_dtype=torch.float32, q_lo: float = 0.5, q_hi: float = 99.5, graph_cache: dict = None) -> torch.Tensor:
    """vol: (X,Y,Z) float32 CUDA tensor of finite values.  Slices are taken across ``axis`` (default 2: the reference's
    ``data[:, :, idx]``, rows along axis 0 - the orientation the model was trained in); returns the volume with the two other
    axes doubled, float32 or int16 (``out_dtype``), as a view of a slice-major buffer.  Full chunks replay
    ``model.graphed_forward`` when ``use_graph``; the last partial chunk runs eagerly.  ``graph_cache``: a dict that keeps the
    captured forwards from call to call (the timepoints of a 4-D scan); it belongs to one model with unchanged weights."""
    _check_volume(model, vol, axis, batch_size, out_dtype, "enhance_volume")
    return _enhance_slice_major(model, vol, axis, batch_size, use_amp, use_graph, out_dtype, q_lo, q_hi, graph_cache).movedim(0, axis)


def up2_blend(plane: torch.Tensor, axis: int, acc: torch.Tensor, mode: int, count: int = 1, out: torch.Tensor = None):
    """One launch of ``mrisr_f32_volume_up2_blend``: ``plane`` is the contiguous float32 slice-major result ``[S][R][C]`` of
    the pass across ``axis``, ``acc`` the contiguous float32 (2X,2Y,2Z) accumulator (None for a single-plane FINISH), ``mode``
    ``_lib.VOLBLEND_*``; FINISH writes the mean of ``count`` planes into ``out`` (float32, where it may be ``acc``, or int16)."""
    imageops._need_cuda(plane, "up2_blend")
    if plane.dtype != torch.float32 or plane.dim() != 3 or not plane.is_contiguous() or axis not in (0, 1, 2):
        raise ValueError(f"expected a contiguous float32 plane [S][R][C] and an axis of 0, 1, 2, got {plane.dtype} {tuple(plane.shape)}, {axis}")
    s, r, c = plane.shape
    if r % 2 or c % 2:
        raise ValueError(f"the in-plane extents of {tuple(plane.shape)} are not doubled ones")
    dims = [r // 2, c // 2]
    dims.insert(axis, s)
    full = tuple(2 * d for d in dims)
    for t, name, dtypes in ((acc, "acc", (torch.float32,)), (out, "out", (torch.float32, torch.int16))):
        if t is not None and (t.dtype not in dtypes or tuple(t.shape) != full or not t.is_contiguous() or t.device != plane.device):
            raise ValueError(f"{name} must be a contiguous {' or '.join(str(d) for d in dtypes)} tensor {full} on {plane.device}")
    L.call("mrisr_f32_volume_up2_blend", plane.data_ptr(), int(axis), *dims, L.ptr(acc), int(mode), int(count),
           L.WINDOW_I16 if out is not None and out.dtype == torch.int16 else L.WINDOW_F32, L.ptr(out), L.stream_ptr())


def enhance_volume_isotropic(model, vol: torch.Tensor, planes=(0, 1, 2), batch_size: int = 16, use_amp: bool = False,
                             use_graph: bool = True, out_dtype=torch.float32, graph_cache: dict = None) -> torch.Tensor:
    """Multi-planar x2 of every axis: vol (X,Y,Z) float32 CUDA -> (2X,2Y,2Z) float32 or int16.  For every axis of ``planes``
    (ascending) the slices across it are enhanced as ``enhance_volume`` does (per-slice window, restored to scanner intensities),
    the remaining axis is doubled with the half-pixel-centred linear rule and the results are averaged - one launch of
    ``csrc/volume_blend.hip`` per plane, ``combine_planes_np`` restated.  One ``graph_cache`` serves all planes and calls."""
    _check_volume(model, vol, 0, batch_size, out_dtype, "enhance_volume_isotropic")
    planes = tuple(planes)
    if not planes or len(set(planes)) != len(planes) or any(a not in (0, 1, 2) for a in planes):
        raise ValueError(f"planes must be a non-empty selection of 0, 1, 2 without repeats, got {planes}")
    planes = tuple(sorted(int(a) for a in planes))
    graphs = graph_cache if graph_cache is not None else {}
    full = tuple(2 * d for d in vol.shape)
    acc = torch.empty(full, dtype=torch.float32, device=vol.device) if len(planes) > 1 or out_dtype == torch.float32 else None
    out = acc if out_dtype == torch.float32 else torch.empty(full, dtype=out_dtype, device=vol.device)
    for i, axis in enumerate(planes):
        plane = _enhance_slice_major(model, vol, axis, batch_size, use_amp, use_graph, torch.float32, 0.5, 99.5, graphs)
        if i == len(planes) - 1:
            up2_blend(plane, axis, acc, L.VOLBLEND_FINISH, len(planes), out)
        else:
            up2_blend(plane, axis, acc, L.VOLBLEND_SET if i == 0 else L.VOLBLEND_ADD)
        del plane      # stream-ordered allocator: the next plane's buffer may take this one's memory
    return out


def _up2_np(e: np.ndarray, axis: int) -> np.ndarray:
    f32 = np.float32
    e = np.moveaxis(e, axis, 0)
    prev, nxt = np.concatenate([e[:1], e[:-1]]), np.concatenate([e[1:], e[-1:]])
    centre = f32(0.75) * e                                            # every operation on float32 arrays rounds to float32
    u = np.empty((2 * e.shape[0],) + e.shape[1:], dtype=f32)
    u[0::2] = centre + f32(0.25) * prev
    u[1::2] = centre + f32(0.25) * nxt
    return np.moveaxis(u, 0, axis)


def combine_planes_np(planes: dict, out_dtype=np.float32) -> np.ndarray:
    """The numpy restatement of the multi-planar blend, the specification ``csrc/volume_blend.hip`` is
    tested against.  ``planes``: ``{axis: E_axis}`` with ``E_axis`` the float32 ``enhance_volume(axis=axis)`` result of one
    (X,Y,Z) volume (axis kept, the two others doubled).  Each is doubled along its axis - ``u[2i] = 0.75 e[i] + 0.25 e[max(i-1, 0)]``,
    ``u[2i+1] = 0.75 e[i] + 0.25 e[min(i+1, S-1)]``, float32, product, product, sum - the results are summed in ascending axis
    order and divided once by ``float32(len(planes))`` (no division for one plane); int16 is ``np.rint`` of that, saturated."""
    axes = sorted(planes)
    if not axes or any(a not in (0, 1, 2) for a in axes):
        raise ValueError(f"planes must be keyed by a non-empty selection of 0, 1, 2, got {list(planes)}")
    if np.dtype(out_dtype) not in (np.dtype(np.float32), np.dtype(np.int16)):
        raise ValueError(f"out_dtype must be float32 or int16, got {out_dtype}")
    total = None
    for a in axes:
        e = np.asarray(planes[a])
        if e.dtype != np.float32 or e.ndim != 3 or e.size == 0:
            raise ValueError(f"plane {a}: expected a non-empty float32 volume, got {e.dtype} {e.shape}")
        u = _up2_np(e, a)
        if total is not None and u.shape != total.shape:
            raise ValueError(f"plane {a} doubles to {u.shape}, the planes before it to {total.shape}")
        total = u if total is None else total + u
    if len(axes) > 1:
        total = total / np.float32(len(axes))
    if np.dtype(out_dtype) == np.dtype(np.int16):
        return np.clip(np.rint(total), -32768, 32767).astype(np.int16)
    return total
