"""Device-side pieces of the evaluation harness (reference ``scripts/test_comparison.py:92-134, 164-202``).

``upscale2_u8``    the x2 interpolation baselines on 8-bit images (cv2 INTER_LINEAR / INTER_CUBIC / bilinear + 3x3
                   sharpening as ``scripts/evaluate.py:upscale_array`` restates them), one HIP launch per method for a whole
                   batch (``csrc/evalops.hip``), exact integer arithmetic: bit-equal to the host function.
``image_metrics``  SSIM, MSE, RMSE, MAE, PSNR per image pair: the fused SSIM + L1 tile pass with a squared-error
                   accumulator and one finalising launch (``csrc/loss.hip``); the (B,5) float64 result stays on the device.
``unit_from_u8``   uint8 -> ``v / 255`` in float32 (ToTensor).

There is no CPU path: CPU tensors raise.  Scale factors other than 2 stay with the host function.
"""
from __future__ import annotations

import torch

from .. import _lib as L
from .imageops import _need_cuda
from .losses import _check_window, _planes

METHODS = {"bilinear": L.UP2_BILINEAR, "bicubic": L.UP2_BICUBIC, "sharp_bilinear": L.UP2_SHARP_BILINEAR}
METRIC_COLUMNS = ("ssim", "mse", "rmse", "mae", "psnr")


def upscale2_u8(img_u8: torch.Tensor, method: str, as_float: bool = True) -> torch.Tensor:
    """img_u8: (h,w) or (B,h,w) uint8 CUDA tensor -> (B,1,2h,2w) float32 in [0,1] (``as_float``) or (B,2h,2w) uint8."""
    if method not in METHODS:
        raise ValueError(f"Unknown interpolation method: {method}")
    _need_cuda(img_u8, "upscale2_u8")
    if img_u8.dtype != torch.uint8 or img_u8.dim() not in (2, 3):
        raise ValueError(f"expected a uint8 tensor (h,w) or (B,h,w), got {img_u8.dtype} {tuple(img_u8.shape)}")
    x = img_u8.contiguous()
    if x.dim() == 2:
        x = x.unsqueeze(0)
    b, h, w = x.shape
    if as_float:
        out = torch.empty((b, 1, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
        ptrs = (None, out.data_ptr())
    else:
        out = torch.empty((b, 2 * h, 2 * w), dtype=torch.uint8, device=x.device)
        ptrs = (out.data_ptr(), None)
    # algorithmic traffic: the source bytes once, the output once
    L.call("mrisr_u8_upscale2", x.data_ptr(), *ptrs, b, h, w, METHODS[method], L.stream_ptr(),
           nbytes=b * h * w * (1 + 4 * out.element_size()))
    return out


def unit_from_u8(t: torch.Tensor) -> torch.Tensor:
    """uint8 CUDA tensor -> float32 tensor of the same shape, ``t / 255``."""
    _need_cuda(t, "unit_from_u8")
    if t.dtype != torch.uint8:
        raise ValueError(f"expected a uint8 tensor, got {t.dtype}")
    x = t.contiguous()
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    L.call("mrisr_u8_to_unit_f32", x.data_ptr(), out.data_ptr(), x.numel(), L.stream_ptr())
    return out


def image_metrics(pred: torch.Tensor, ref: torch.Tensor, window_size: int = 11, sigma: float = 1.5,
                  val_range: float = 1.0) -> torch.Tensor:
    """pred, ref: (B,1,H,W) CUDA tensors -> (B,5) float64 CUDA tensor, columns ``METRIC_COLUMNS``
    (ssim, mse, rmse, mae, psnr; PSNR = 10 log10(val_range^2 / mse), 100 when mse < 1e-10).  No host synchronisation."""
    _check_window(window_size)
    a, b = _planes(pred), _planes(ref)
    if a.shape != b.shape:
        raise ValueError(f"shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
    if a.shape[1] != 1:
        raise ValueError(f"expected single-channel images (B,1,H,W), got {tuple(a.shape)}")
    n, _, h, w = a.shape
    st = L.stream_ptr()
    sums = torch.zeros(n * 3, dtype=torch.float64, device=a.device)
    out = torch.empty((n, 5), dtype=torch.float64, device=a.device)
    L.call("mrisr_image_metrics", a.data_ptr(), b.data_ptr(), sums.data_ptr(), n, h, w, float(val_range), float(sigma),
           int(window_size), st, nbytes=n * h * w * 8)        # the two fp32 images once
    L.call("mrisr_metrics_finalize", sums.data_ptr(), n, h, w, float(val_range), out.data_ptr(), st)
    return out
