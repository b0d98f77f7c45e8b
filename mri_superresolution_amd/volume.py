"""Whole-volume inference on the device (extension): a float32 volume in HBM -> the x2 volume in HBM.

Per chunk of ``batch_size`` slices: exact 0.5 / 99.5 percentile window of every slice (``csrc/percentile.hip``) -> normalise
-> forward -> clamp and restore to the slice's own intensity window, written straight into the output volume.  The window is
per slice, as in the reference's extraction (``utils/extraction_utils.py:118-131``); a constant slice enters the network as
zeros (``utils/preprocessing.py:143-153``) and comes back at its value.  Nothing leaves the device in between.
"""
from __future__ import annotations

import torch

from .utils import imageops


def enhance_volume(model, vol: torch.Tensor, axis: int = 2, batch_size: int = 16, use_amp: bool = False, use_graph: bool = True,
                   out_dtype=torch.float32, q_lo: float = 0.5, q_hi: float = 99.5, graph_cache: dict = None) -> torch.Tensor:
    """vol: (X,Y,Z) float32 CUDA tensor of finite values.  Slices are taken across ``axis`` (default 2: the reference's
    ``data[:, :, idx]``, rows along axis 0 - the orientation the model was trained in); returns the volume with the two other
    axes doubled, float32 or int16 (``out_dtype``), as a view of a slice-major buffer.  Full chunks replay
    ``model.graphed_forward`` when ``use_graph``; the last partial chunk runs eagerly.  ``graph_cache``: a dict that keeps the
    captured forwards from call to call (the timepoints of a 4-D scan); it belongs to one model with unchanged weights."""
    imageops._need_cuda(vol, "enhance_volume")
    if vol.dtype != torch.float32 or vol.dim() != 3 or vol.numel() == 0:
        raise ValueError(f"expected a non-empty float32 volume (X,Y,Z), got {vol.dtype} {tuple(vol.shape)}")
    if axis not in (0, 1, 2):
        raise ValueError(f"axis must be 0, 1 or 2, got {axis}")
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    if out_dtype not in (torch.float32, torch.int16):
        raise ValueError(f"out_dtype must be torch.float32 or torch.int16, got {out_dtype}")
    if model.training:
        raise RuntimeError("enhance_volume runs the eval forward: call model.eval() first")
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
    return out.movedim(0, axis)
