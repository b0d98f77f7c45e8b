"""Device-side pre- and post-processing of the inference driver (reference ``scripts/infer.py:97-130, 276-333``).

``normalise_percentile_u8``  8-bit grayscale image(s) on the GPU -> (B,1,H,W) fp32 in [0,1]: clip to the 0.5 / 99.5
                             percentiles and rescale (``infer.py:107-117``), as two HIP kernels (256-bin histogram ->
                             per-image look-up table; ``csrc/image.hip``), numpy's float32 arithmetic step by step.
``normalise_percentile_f32`` the same window for FLOAT images (12- to 16-bit or float MRI volumes; extension): an exact radix
                             select of the percentiles (``csrc/percentile.hip``), then clip and rescale; a constant image
                             becomes zeros (reference ``utils/preprocessing.py:143-153``).  ``percentile_bounds_f32`` is the
                             selection alone, ``restore_window`` the way back to the input's intensity scale, and
                             ``percentile_bounds_np`` the numpy restatement the kernels are tested against.
``to_uint8``                 clamp(0,1) -> ``(x * 255).astype(uint8)`` (``infer.py:276,331``), one HIP kernel.
``match_histograms``         skimage.exposure.match_histograms for one channel (``infer.py:285-313``) with torch CUDA
                             primitives (unique / cumsum / searchsorted) in float64 - plumbing, no HIP kernel: it runs only
                             when a target image is given.

There is no CPU path: CPU tensors raise.  The numpy restatements these are tested against live in ``scripts/infer.py``
(``normalise_percentile``, ``match_histograms_np``) and are themselves "parity unpinned" against skimage, which is absent.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L


def _need_cuda(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what} runs on an MI355X through libmrisr.so only; got a CPU tensor (no CPU fallback)")


def normalise_percentile_u8(img_u8: torch.Tensor, q_lo: float = 0.5, q_hi: float = 99.5, return_bounds: bool = False):
    """img_u8: (H,W) or (B,H,W) uint8 CUDA tensor -> (B,1,H,W) float32; every image with its own percentiles."""
    _need_cuda(img_u8, "normalise_percentile_u8")
    if img_u8.dtype != torch.uint8 or img_u8.dim() not in (2, 3):
        raise ValueError(f"expected a uint8 tensor (H,W) or (B,H,W), got {img_u8.dtype} {tuple(img_u8.shape)}")
    x = img_u8.contiguous()
    if x.dim() == 2:
        x = x.unsqueeze(0)
    b, h, w = x.shape
    n = h * w
    st = L.stream_ptr()
    hist = torch.zeros(b * 256, dtype=torch.int32, device=x.device)
    out = torch.empty((b, 1, h, w), dtype=torch.float32, device=x.device)
    lohi = torch.empty((b, 2), dtype=torch.float32, device=x.device)
    L.call("mrisr_u8_histogram", x.data_ptr(), n, b, hist.data_ptr(), st)
    L.call("mrisr_u8_percentile_normalise", x.data_ptr(), hist.data_ptr(), n, b, float(q_lo), float(q_hi),
           out.data_ptr(), lohi.data_ptr(), st)
    return (out, lohi) if return_bounds else out


def _f32_batch(x: torch.Tensor, what: str) -> torch.Tensor:
    _need_cuda(x, what)
    if x.dtype != torch.float32 or x.dim() not in (2, 3) or x.numel() == 0:
        raise ValueError(f"expected a non-empty float32 tensor (H,W) or (B,H,W), got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    return x.unsqueeze(0) if x.dim() == 2 else x


_WORKSPACES = {}       # (device, batch) -> selection workspace: the library clears what it needs, so one serves every call


def _percentile_workspace(device, batch):
    key = (str(device), int(batch))
    if key not in _WORKSPACES:
        nbytes = int(L.load().mrisr_f32_percentile_workspace_bytes(int(batch)))
        if nbytes == 0:
            raise ValueError(f"batch of {batch} images is outside 1..65535")
        _WORKSPACES[key] = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
    return _WORKSPACES[key]


def percentile_bounds_f32(x: torch.Tensor, q_lo: float = 0.5, q_hi: float = 99.5, workspace=None) -> torch.Tensor:
    """x: (H,W) or (B,H,W) float32 CUDA tensor of FINITE values -> (B,2) float32 ``(np.percentile(x[b], q_lo),
    np.percentile(x[b], q_hi))``, exactly, without a host synchronisation (9 launches; capturable in a HIP graph).
    ``workspace``: an int32 CUDA tensor of ``mrisr_f32_percentile_workspace_bytes(B)`` bytes to use instead of the cached one
    (all calls on one device and batch size share that one: they must be on one stream)."""
    x = _f32_batch(x, "percentile_bounds_f32")
    b, n = x.shape[0], x.shape[1] * x.shape[2]
    ws = _percentile_workspace(x.device, b) if workspace is None else workspace
    lohi = torch.empty((b, 2), dtype=torch.float32, device=x.device)
    L.call("mrisr_f32_percentile_bounds", x.data_ptr(), n, b, float(q_lo), float(q_hi), lohi.data_ptr(), ws.data_ptr(), L.stream_ptr())
    return lohi


def normalise_percentile_f32(x: torch.Tensor, q_lo: float = 0.5, q_hi: float = 99.5, return_bounds: bool = False):
    """x: (H,W) or (B,H,W) float32 CUDA tensor -> (B,1,H,W) float32 in [0,1]: every image clipped to its own percentiles and
    rescaled; an image whose two percentiles are equal becomes zeros."""
    x = _f32_batch(x, "normalise_percentile_f32")
    b, h, w = x.shape
    lohi = percentile_bounds_f32(x, q_lo, q_hi)
    out = torch.empty((b, 1, h, w), dtype=torch.float32, device=x.device)
    L.call("mrisr_f32_window_normalise", x.data_ptr(), lohi.data_ptr(), h * w, b, out.data_ptr(), L.stream_ptr())
    return (out, lohi) if return_bounds else out


def restore_window(y: torch.Tensor, lohi: torch.Tensor, dtype=torch.float32, out=None) -> torch.Tensor:
    """The inverse of the window: y (B,1,H,W) or (B,H,W) float32 CUDA tensor, lohi (B,2) -> ``clamp(y, 0, 1) * (hi - lo) + lo``
    in float32 as a tensor of y's shape, float32 or int16 (rounded half to even, saturated).  ``out``: a contiguous tensor of
    that shape and dtype to write into."""
    _need_cuda(y, "restore_window")
    _need_cuda(lohi, "restore_window")
    if y.dtype != torch.float32 or y.dim() not in (3, 4) or (y.dim() == 4 and y.shape[1] != 1) or y.numel() == 0:
        raise ValueError(f"expected a non-empty float32 tensor (B,1,H,W) or (B,H,W), got {y.dtype} {tuple(y.shape)}")
    if lohi.dtype != torch.float32 or tuple(lohi.shape) != (y.shape[0], 2):
        raise ValueError(f"expected float32 bounds {(y.shape[0], 2)}, got {lohi.dtype} {tuple(lohi.shape)}")
    if dtype not in (torch.float32, torch.int16):
        raise ValueError(f"restore_window writes float32 or int16, not {dtype}")
    y = y.contiguous()
    if out is None:
        out = torch.empty(y.shape, dtype=dtype, device=y.device)
    elif out.dtype != dtype or tuple(out.shape) != tuple(y.shape) or not out.is_contiguous() or out.device != y.device:
        raise ValueError(f"out must be a contiguous {dtype} tensor {tuple(y.shape)} on {y.device}")
    L.call("mrisr_f32_window_restore", y.data_ptr(), lohi.contiguous().data_ptr(), y.numel() // y.shape[0], y.shape[0],
           L.WINDOW_I16 if dtype == torch.int16 else L.WINDOW_F32, out.data_ptr(), L.stream_ptr())
    return out


def np_percentile_f32(sorted_values: np.ndarray, q: float) -> np.float32:
    """``np.percentile(values, q)`` of a non-empty float32 array for a SCALAR ``q``, from the sorted values, in the explicit form
    the kernels implement (csrc/volume_common.h).  For a float32 array numpy carries the quantile and the virtual index in float32:
    ``v = float32(n - 1) * (float32(q) / float32(100))``; the order statistics are ``k = min(floor(v), n - 1)`` (float32(n - 1) may
    round up past the last index when n > 2^24) and ``min(k + 1, n - 1)``, the weight ``t = v - floor(v)``, and ``_lerp`` interpolates
    in float32: ``a + (b - a) * t``, and ``b - (b - a) * (1 - t)`` where ``t >= 0.5``.  (It is not the float64 interpolation
    rounded, and a float64 array of ``q`` takes a float64 path: both differ in the last place.)"""
    f32 = np.float32
    s, n = sorted_values, sorted_values.size
    v = f32(n - 1) * (f32(q) / f32(100))
    prev = np.floor(v)
    k = min(int(prev), n - 1)
    lo, hi, t = s[k], s[min(k + 1, n - 1)], f32(v - prev)
    d = f32(hi - lo)
    return f32(hi - f32(d * f32(f32(1) - t))) if t >= f32(0.5) else f32(lo + f32(d * t))


def percentile_bounds_np(a: np.ndarray, q_lo: float = 0.5, q_hi: float = 99.5) -> np.ndarray:
    """``(np.percentile(a, q_lo), np.percentile(a, q_hi))`` of one float32 image as float32: ``np_percentile_f32`` twice."""
    a = np.asarray(a)
    if a.dtype != np.float32 or a.size == 0:
        raise ValueError(f"expected a non-empty float32 array, got {a.dtype} {a.shape}")
    s = np.sort(a.ravel())
    return np.array([np_percentile_f32(s, q_lo), np_percentile_f32(s, q_hi)], dtype=np.float32)


def to_uint8(x: torch.Tensor) -> torch.Tensor:
    """float32 CUDA tensor -> uint8 tensor of the same shape: clamp(0,1), times 255, truncated."""
    _need_cuda(x, "to_uint8")
    xf = x.detach().to(torch.float32).contiguous()
    out = torch.empty(xf.shape, dtype=torch.uint8, device=xf.device)
    L.call("mrisr_f32_to_u8", xf.data_ptr(), out.data_ptr(), xf.numel(), L.stream_ptr())
    return out


def _interp(x: torch.Tensor, xp: torch.Tensor, fp: torch.Tensor) -> torch.Tensor:
    """np.interp(x, xp, fp) for increasing xp (float64 in, float64 out)."""
    i = torch.searchsorted(xp, x, right=True).clamp_(1, xp.numel() - 1) if xp.numel() > 1 else torch.zeros_like(x, dtype=torch.long)
    if xp.numel() == 1:
        return fp[0].expand_as(x).clone()
    x0, x1, f0, f1 = xp[i - 1], xp[i], fp[i - 1], fp[i]
    t = ((x - x0) / (x1 - x0)).clamp_(0.0, 1.0)       # clamps reproduce np.interp's constant extension at both ends
    return f0 + t * (f1 - f0)


def match_histograms(image: torch.Tensor, reference: torch.Tensor) -> torch.Tensor:
    """Maps every value of ``image`` to the ``reference`` value of equal empirical CDF (skimage's algorithm for a
    single channel: unique values + counts -> quantiles -> np.interp).  Both CUDA tensors of any shape; returns
    float64 like skimage / np.interp do."""
    _need_cuda(image, "match_histograms")
    _need_cuda(reference, "match_histograms")
    src_vals, src_idx, src_counts = torch.unique(image.reshape(-1), return_inverse=True, return_counts=True)
    ref_vals, ref_counts = torch.unique(reference.reshape(-1), return_counts=True)
    src_q = src_counts.cumsum(0).double() / image.numel()
    ref_q = ref_counts.cumsum(0).double() / reference.numel()
    return _interp(src_q, ref_q, ref_vals.double())[src_idx].reshape(image.shape)
