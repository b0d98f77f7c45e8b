"""Low-field MRI simulation: low-resolution images drawn from high-resolution ones (extension).

The reference's degradation model is ``utils/preprocessing.py:225-293`` ``simulate_low_field_mri`` (FFT -> keep the
centre of k-space -> complex Gaussian noise over all of k-space -> IFFT -> magnitude -> min/max renormalisation) followed by
``utils/extraction_utils.py:136-163`` (clip to [0,1], 2x ``INTER_AREA`` downsampling, ``astype(np.uint8)``).

``simulate_low_field_u8``    the device path (``csrc/lowfield.hip``): a batch of uint8 HR images in HBM -> uint8 LR images,
                             noise from explicit image-space planes or from per-image 64-bit seeds.  CPU tensors raise.
``simulate_low_field_f32``   the float form (``mrisr_lowfield_simulate_f32``): float32 images in [0,1] of ANY size -> the
                             renormalised, clipped float32 plane at full size - what the slice extraction
                             (``utils/extraction.py``) resizes afterwards.  ``simulate_low_field_f32_host`` restates it.
``simulate_low_field_host``  float64 NumPy restatement of the two reference functions, in their FFT form: what the tests
                             compare the device path against.
``image_noise_from_kspace``  the image-space noise ``ifft2(ifftshift(N))`` of a k-space noise array ``N``.
``derive_seeds``             per-sample seeds of ``DevicePairLoader(simulate_lr=...)``.

The reference's k-space noise has per-component standard deviation ``(noise_std / 255) sqrt(R C) / 10``; ``ifft2`` scales by
``1 / (R C)`` and sums ``R C`` terms, so in image space it is white complex Gaussian noise of per-component standard
deviation ``noise_std / 2550``.  ``INTER_AREA`` at exactly half scale is the 2x2 mean (even sizes only); parity with cv2's
own code path is not claimed.  Deviation: an image whose simulated magnitude is constant (the reference divides 0 by 0)
comes out as its own minimum everywhere.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from .imageops import _need_cuda

_TABLES = {}       # (n, crop_factor, device) -> (re, im) device tensors
_M64 = (1 << 64) - 1


def dirichlet_table(n: int, crop_factor: float) -> Tuple[np.ndarray, np.ndarray]:
    """float32 (re, im) of the Dirichlet row of an axis of length ``n`` through the library's host helper (no GPU needed)."""
    re, im = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.float32)
    L.check(L.load().mrisr_lowfield_dirichlet(int(n), float(crop_factor), re.ctypes.data, im.ctypes.data), "mrisr_lowfield_dirichlet")
    return re, im


def dirichlet_table_any(n: int, crop_factor: float) -> Tuple[np.ndarray, np.ndarray]:
    """The same for any ``n >= 2``, odd sizes included (``mrisr_lowfield_dirichlet_any``)."""
    re, im = np.empty(max(int(n), 0), dtype=np.float32), np.empty(max(int(n), 0), dtype=np.float32)
    L.check(L.load().mrisr_lowfield_dirichlet_any(int(n), float(crop_factor), re.ctypes.data, im.ctypes.data), "mrisr_lowfield_dirichlet_any")
    return re, im


def _device_table(n, crop_factor, device, any_size=False):
    key = (int(n), float(crop_factor), str(device), bool(any_size))
    if key not in _TABLES:
        re, im = (dirichlet_table_any if any_size else dirichlet_table)(n, crop_factor)
        _TABLES[key] = (torch.from_numpy(re).to(device), torch.from_numpy(im).to(device))
    return _TABLES[key]


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def derive_seeds(seed: int, epoch: Optional[int], sample_ids: Sequence[int]) -> list:
    """One 64-bit seed per sample from ``(seed, epoch, sample index)``; ``epoch=None`` (a loader that neither shuffles nor
    augments: validation) leaves the epoch out, so that every epoch sees the same images."""
    base = _splitmix64(int(seed) & _M64)
    if epoch is not None:
        base = _splitmix64(base ^ _splitmix64((int(epoch) + 1) & _M64))
    return [_splitmix64(base ^ _splitmix64((int(i) << 1 | 1) & _M64)) for i in sample_ids]


def image_noise_from_kspace(noise_real: np.ndarray, noise_imag: np.ndarray) -> np.ndarray:
    """Complex image-space noise of the (shifted) k-space noise arrays the reference adds (preprocessing.py:278-284)."""
    n = np.asarray(noise_real, dtype=np.float64) + 1j * np.asarray(noise_imag, dtype=np.float64)
    return np.fft.ifft2(np.fft.ifftshift(n, axes=(-2, -1)), axes=(-2, -1))


def _noise_args(what, b, h, w, dev, noise_std, seeds, noise):
    """-> (sigma, n_re, n_im, seed tensor): the noise operands of either entry point from ``noise_std / seeds / noise``."""
    if noise_std < 0:
        raise ValueError(f"noise_std {noise_std} is negative")
    sigma = float(noise_std) / 2550.0
    n_re = n_im = seed_t = None
    if noise is not None:
        n_re, n_im = noise
        for t in (n_re, n_im):
            _need_cuda(t, what)
            if t.dtype != torch.float32 or tuple(t.shape) != (b, h, w):
                raise ValueError(f"noise planes must be float32 {(b, h, w)}, got {t.dtype} {tuple(t.shape)}")
        n_re, n_im = n_re.contiguous(), n_im.contiguous()
    elif sigma > 0:
        if seeds is None:
            seeds = torch.randint(0, 2 ** 62, (b,), dtype=torch.int64).tolist()
        elif isinstance(seeds, int):
            seeds = derive_seeds(seeds, None, range(b))
        if isinstance(seeds, torch.Tensor):
            seed_t = seeds.to(device=dev, dtype=torch.int64).contiguous()
        else:
            seed_t = torch.from_numpy(np.array([int(s) & _M64 for s in seeds], dtype=np.uint64).view(np.int64)).to(dev)
        if seed_t.numel() != b:
            raise ValueError(f"{seed_t.numel()} seeds for a batch of {b}")
    return sigma, n_re, n_im, seed_t


def simulate_low_field_u8(high_u8: torch.Tensor, kspace_crop_factor: float = 0.5, noise_std: float = 5.0, seeds=None,
                          noise=None, return_float: bool = False, _return_magnitude: bool = False):
    """high_u8: (H,W) or (B,H,W) uint8 CUDA tensor, H and W even -> (B,H/2,W/2) uint8 LR images (with ``return_float`` also
    the unquantised LR plane, float32 in [0,1]).

    ``noise``: ``(n_re, n_im)`` float32 CUDA tensors (B,H,W), explicit image-space noise (``image_noise_from_kspace`` of a
    reference draw); else ``seeds``: an int (image b gets ``derive_seeds(seeds, None, [b])``), a sequence or an int64 tensor
    of B seeds; with neither, fresh seeds from torch's generator.  ``noise_std=0`` adds no noise and ignores the seeds."""
    _need_cuda(high_u8, "simulate_low_field_u8")
    if high_u8.dtype != torch.uint8 or high_u8.dim() not in (2, 3):
        raise ValueError(f"expected a uint8 tensor (H,W) or (B,H,W), got {high_u8.dtype} {tuple(high_u8.shape)}")
    x = high_u8.contiguous()
    if x.dim() == 2:
        x = x.unsqueeze(0)
    b, h, w = x.shape
    dev = x.device
    sigma, n_re, n_im, seed_t = _noise_args("simulate_low_field_u8", b, h, w, dev, noise_std, seeds, noise)
    # shape / crop_factor rules are the library's (MRISR_E_SHAPE / MRISR_E_ARG raise through _lib.check)
    rr, ri = _device_table(h, kspace_crop_factor, dev)
    cr, ci = _device_table(w, kspace_crop_factor, dev)
    ws = torch.empty(int(L.load().mrisr_lowfield_workspace_bytes(b, h, w)) // 4, dtype=torch.float32, device=dev)
    out = torch.empty((b, h // 2, w // 2), dtype=torch.uint8, device=dev)
    out_f = torch.empty((b, h // 2, w // 2), dtype=torch.float32, device=dev) if return_float else None
    L.call("mrisr_lowfield_simulate", x.data_ptr(), b, h, w, float(kspace_crop_factor), rr.data_ptr(), ri.data_ptr(),
           cr.data_ptr(), ci.data_ptr(), sigma, L.ptr(n_re), L.ptr(n_im), L.ptr(seed_t), ws.data_ptr(), out.data_ptr(),
           L.ptr(out_f), L.stream_ptr())
    res = (out, out_f) if return_float else out
    if _return_magnitude:          # tests: the magnitude plane |Y + n| of pass 1
        return res, ws[:b * h * w].view(b, h, w)
    return res


def simulate_low_field_f32(x: torch.Tensor, kspace_crop_factor: float = 0.5, noise_std: float = 5.0, seeds=None, noise=None,
                           _return_magnitude: bool = False):
    """x: (H,W) or (B,H,W) float32 CUDA tensor in [0,1], any H, W >= 2 -> (B,H,W) float32: the simulated plane
    (preprocessing.py:225-293) clipped to [0,1] (extraction_utils.py:147), at full size.  ``noise`` / ``seeds`` /
    ``noise_std`` as in ``simulate_low_field_u8``; the same seed draws the same noise in both."""
    _need_cuda(x, "simulate_low_field_f32")
    if x.dtype != torch.float32 or x.dim() not in (2, 3):
        raise ValueError(f"expected a float32 tensor (H,W) or (B,H,W), got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    if x.dim() == 2:
        x = x.unsqueeze(0)
    b, h, w = x.shape
    dev = x.device
    sigma, n_re, n_im, seed_t = _noise_args("simulate_low_field_f32", b, h, w, dev, noise_std, seeds, noise)
    rr, ri = _device_table(h, kspace_crop_factor, dev, any_size=True)
    cr, ci = _device_table(w, kspace_crop_factor, dev, any_size=True)
    ws = torch.empty(int(L.load().mrisr_lowfield_workspace_bytes(b, h, w)) // 4, dtype=torch.float32, device=dev)
    out = torch.empty((b, h, w), dtype=torch.float32, device=dev)
    L.call("mrisr_lowfield_simulate_f32", x.data_ptr(), b, h, w, float(kspace_crop_factor), rr.data_ptr(), ri.data_ptr(),
           cr.data_ptr(), ci.data_ptr(), sigma, L.ptr(n_re), L.ptr(n_im), L.ptr(seed_t), ws.data_ptr(), out.data_ptr(),
           L.stream_ptr())
    if _return_magnitude:          # tests: the magnitude plane |Y + n| of pass 1
        return out, ws[:b * h * w].view(b, h, w)
    return out


def simulate_low_field_f32_host(x: np.ndarray, kspace_crop_factor: float = 0.5, noise_std: float = 5.0, kspace_noise=None,
                                rng: Optional[np.random.Generator] = None):
    """float64 restatement of the reference for one (H,W) image in [0,1] of any size; the dict of ``simulate_low_field_host``
    without the 2x2 mean: ``simulated`` (preprocessing.py:225-293), ``magnitude`` (:287) and ``clipped``
    (extraction_utils.py:147).

    A float32 array is handed to ``np.fft.fft2`` as it is, as the reference hands it its float32 normalised slice: numpy >= 2
    runs that one transform in single precision (earlier versions in double), everything after it is complex128 either way.
    Any other dtype is taken as float64 - the plain float64 restatement the device path is compared against."""
    data = np.asarray(x)
    if data.dtype != np.float32:
        data = data.astype(np.float64)
    if data.ndim != 2 or min(data.shape) < 2:
        raise ValueError(f"expected an (H,W) image of at least 2 x 2, got {data.shape}")
    orig_min, orig_max = data.min(), data.max()                                   # :246
    kspace = np.fft.fftshift(np.fft.fft2(data))                                   # :249-250
    rows, cols = kspace.shape
    crop_r, crop_c = int(rows * kspace_crop_factor), int(cols * kspace_crop_factor)     # :257-258
    mask = np.zeros((rows, cols), dtype=np.complex128)
    mask[rows // 2 - crop_r // 2:rows // 2 + crop_r // 2, cols // 2 - crop_c // 2:cols // 2 + crop_c // 2] = 1   # :261-268
    low = kspace * mask
    if kspace_noise is not None:
        low = low + np.asarray(kspace_noise[0], dtype=np.float64) + 1j * np.asarray(kspace_noise[1], dtype=np.float64)   # :280
    elif noise_std > 0:
        scaled = (noise_std / 255.0) * np.sqrt(rows * cols) / 10                  # :274
        rng = rng or np.random.default_rng()
        low = low + rng.normal(0, scaled, low.shape) + 1j * rng.normal(0, scaled, low.shape)
    magnitude = np.abs(np.fft.ifft2(np.fft.ifftshift(low)))                       # :283-287
    if magnitude.max() > magnitude.min():
        simulated = (magnitude - magnitude.min()) / (magnitude.max() - magnitude.min())   # :290
        simulated = simulated * (orig_max - orig_min) + orig_min                  # :291
    else:                                                                         # deviation: 0 / 0 in the reference
        simulated = np.full_like(magnitude, float(orig_min))
    return {"simulated": simulated, "magnitude": magnitude, "clipped": np.clip(simulated, 0, 1)}   # extraction_utils.py:147


def simulate_low_field_host(high_u8: np.ndarray, kspace_crop_factor: float = 0.5, noise_std: float = 5.0,
                            kspace_noise=None, rng: Optional[np.random.Generator] = None):
    """float64 restatement of the reference for one (H,W) uint8 image, H and W even; returns a dict:

    ``simulated``  preprocessing.py:225-293 on ``high_u8 / 255`` (before the clip)
    ``magnitude``  its ``np.abs(noisy_image)`` (:287)
    ``lr``         extraction_utils.py:147-157: clip to [0,1], then the 2x2 mean (``INTER_AREA`` at exactly half scale)
    ``lr_u8``      :162 ``np.clip(lr * 255, 0, 255).astype(np.uint8)``

    ``kspace_noise``: ``(noise_real, noise_imag)`` as the reference draws them (:278-279, already scaled); else drawn from
    ``rng`` with the reference's standard deviation; ``noise_std=0`` adds none."""
    u8 = np.asarray(high_u8)
    if u8.dtype != np.uint8 or u8.ndim != 2 or u8.shape[0] % 2 or u8.shape[1] % 2:
        raise ValueError(f"expected an even-sized (H,W) uint8 image, got {u8.dtype} {u8.shape}")
    data = u8.astype(np.float64) / 255.0
    orig_min, orig_max = data.min(), data.max()                                   # :246
    kspace = np.fft.fftshift(np.fft.fft2(data))                                   # :249-250
    rows, cols = kspace.shape
    crop_r, crop_c = int(rows * kspace_crop_factor), int(cols * kspace_crop_factor)     # :257-258
    mask = np.zeros((rows, cols), dtype=np.complex128)
    mask[rows // 2 - crop_r // 2:rows // 2 + crop_r // 2, cols // 2 - crop_c // 2:cols // 2 + crop_c // 2] = 1   # :261-268
    low = kspace * mask
    if kspace_noise is not None:
        low = low + np.asarray(kspace_noise[0], dtype=np.float64) + 1j * np.asarray(kspace_noise[1], dtype=np.float64)   # :280
    elif noise_std > 0:
        scaled = (noise_std / 255.0) * np.sqrt(rows * cols) / 10                  # :274
        rng = rng or np.random.default_rng()
        low = low + rng.normal(0, scaled, low.shape) + 1j * rng.normal(0, scaled, low.shape)
    magnitude = np.abs(np.fft.ifft2(np.fft.ifftshift(low)))                       # :283-287
    if magnitude.max() > magnitude.min():
        simulated = (magnitude - magnitude.min()) / (magnitude.max() - magnitude.min())   # :290
        simulated = simulated * (orig_max - orig_min) + orig_min                  # :291
    else:                                                                         # deviation: 0 / 0 in the reference
        simulated = np.full_like(magnitude, orig_min)
    clipped = np.clip(simulated, 0, 1)                                            # extraction_utils.py:147
    lr = clipped.reshape(rows // 2, 2, cols // 2, 2).mean((1, 3))                 # :153-157 at exactly half scale
    return {"simulated": simulated, "magnitude": magnitude, "lr": lr, "lr_u8": np.clip(lr * 255, 0, 255).astype(np.uint8)}   # :162


def simulate_low_field_circulant(high_u8: np.ndarray, kspace_crop_factor: float = 0.5, image_noise=None):
    """The same in the circulant form the kernel uses, in float64: ``Y = P_r x P_c^T`` with the complex Dirichlet rows,
    ``image_noise`` (complex, ``image_noise_from_kspace``) added in image space.  Returns the dict of
    ``simulate_low_field_host``."""
    u8 = np.asarray(high_u8)
    data = u8.astype(np.float64) / 255.0
    rows, cols = data.shape

    def circ(n):
        a = int(n * kspace_crop_factor) // 2
        d = np.arange(n)
        p = np.exp(2j * np.pi * np.outer(d, np.arange(-a, a)) / n).sum(1) / n
        return p[(d[:, None] - d[None, :]) % n]

    y = circ(rows) @ data @ circ(cols).T
    if image_noise is not None:
        y = y + image_noise
    magnitude = np.abs(y)
    if magnitude.max() > magnitude.min():
        simulated = (magnitude - magnitude.min()) / (magnitude.max() - magnitude.min()) * (data.max() - data.min()) + data.min()
    else:
        simulated = np.full_like(magnitude, data.min())
    lr = np.clip(simulated, 0, 1).reshape(rows // 2, 2, cols // 2, 2).mean((1, 3))
    return {"simulated": simulated, "magnitude": magnitude, "lr": lr, "lr_u8": np.clip(lr * 255, 0, 255).astype(np.uint8)}
