"""Paired-slice extraction on the device (extension): a float volume in HBM -> the paired HR / LR uint8
slices ``scripts/train.py`` reads, the reference's ``scripts/extract_paired_slices.py`` + ``utils/extraction_utils.py:74-164``.

Per selected slice ``data[:, :, idx]`` (rows along axis 0):

    HR  percentile window 0.5 / 99.5 -> [0,1]  ->  letter-box resize to ``target_size`` (LANCZOS4)  ->  uint8 by truncation
    LR  the same normalised plane  ->  low-field simulation at the scan's own size (``utils/lowfield.py``), clip  ->
        letter-box resize to half the target (AREA)  ->  uint8 by truncation

``extract_pairs``            the device path: one batch of all selected slices through ``csrc/percentile.hip``,
                             ``csrc/lowfield.hip`` and ``csrc/resample.hip``; nothing returns to the host in between.
``resample_letterbox_f32``   the resize alone (``mrisr_f32_resample_letterbox``), tap tables cached per axis.
``extract_pairs_host``, ``resample_letterbox_host``, ``resample_taps_np``: float64 / NumPy restatements the tests compare
against; ``slice_indices``, ``bids_identifier``, ``pair_filename``, ``letterbox_geometry``: the reference's bookkeeping.

Tap rules (``mrisr_resample_taps``; output sample d, ``scale = src / dst``, ``s = (d + 0.5) scale - 0.5``): LINEAR 2 taps, CUBIC
4 taps (Keys, A = -0.75), LANCZOS4 8 taps at ``floor(s) - 3 .. floor(s) + 4`` with ``sinc(x) sinc(x / 4)`` normalised to sum 1,
indices clamped to the image (replicated border); AREA for ``dst <= src``: source sample i weighs
``|[i, i + 1] n [d scale, (d + 1) scale]| / min(scale, src - d scale)``.

Deviations: AREA with ``dst > src`` uses the LINEAR taps; a constant slice becomes zeros on the HR side too (the reference's
HR chain leaves the constant in place, its LR chain gives zeros); the constant-magnitude rule of ``utils/lowfield.py``.
cv2 is absent, so parity with ``cv2.resize``'s own code path is not claimed anywhere: everything in the chain except
``cv2.resize`` itself is pinned to the reference by ``tests/golden/extraction.npz``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from . import imageops, lowfield
from .imageops import _need_cuda

LINEAR, CUBIC, AREA, LANCZOS4 = L.RESAMPLE_LINEAR, L.RESAMPLE_CUBIC, L.RESAMPLE_AREA, L.RESAMPLE_LANCZOS4
MAX_TAPS = 16
_WORD = frozenset("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789")
_MODALITIES = frozenset({"BOLD", "DWI", "FLAIR", "PD", "PDw", "T1w", "T2w"})      # the name suffixes kept as a modality
_TAPS = {}       # (method, src, dst, device) -> (index int16 [dst][K], weight float32 [dst][K]) device tensors


# ---------------------------------------------------------------- bookkeeping (host)
def slice_indices(num_slices: int, n_slices: int = 10, lower: float = 0.2, upper: float = 0.8) -> np.ndarray:
    """``n_slices`` equally spaced slice numbers between ``int(lower * num_slices)`` and ``int(upper * num_slices)``
    (extraction_utils.py:112-115).  ``ValueError`` if one is outside the volume (the reference would crash there)."""
    idx = np.linspace(int(lower * num_slices), int(upper * num_slices), n_slices, dtype=int)
    if idx.size and (idx.min() < 0 or idx.max() >= num_slices):
        raise ValueError(f"slice indices {idx.min()}..{idx.max()} outside a volume of {num_slices} slices "
                         f"(lower {lower}, upper {upper})")
    return idx


def bids_identifier(path: str) -> str:
    """Subject identifier of a scan's file name: its ``key-value`` entities joined by ``_`` plus a trailing standard modality
    suffix; a name without entities stays as it is, minus ``.nii`` / ``.nii.gz``."""
    name = os.path.basename(path)
    name = name[:-7] if name.endswith(".nii.gz") else name[:-4] if name.endswith(".nii") else name
    # an entity is a run of ASCII letters / digits, one dash, another such run; scanned left to right without overlap, so in
    # "a-b-c" only a-b counts and "a--b" holds none
    pairs = []
    for token in "".join(ch if ch in _WORD or ch == "-" else " " for ch in name).split():
        parts, i = token.split("-"), 0
        while i + 1 < len(parts):
            if parts[i] and parts[i + 1]:
                pairs.append(parts[i] + "-" + parts[i + 1])
                i += 2
            else:
                i += 1
    if not pairs:
        return name
    _, underscore, suffix = name.rpartition("_")
    if underscore and suffix in _MODALITIES:
        pairs.append(suffix)
    return "_".join(pairs)


def pair_filename(subject: str, idx: int, timepoint: Optional[int] = None) -> str:
    """``subject[_T{timepoint}]_s{idx:03d}.png``: the same name in both directories."""
    mid = f"_T{timepoint}" if timepoint is not None else ""
    return f"{subject}{mid}_s{int(idx):03d}.png"


def letterbox_geometry(h: int, w: int, target_w: int, target_h: int) -> Tuple[int, int, int, int]:
    """-> ``(new_w, new_h, x_off, y_off)`` of an (h, w) image inside a (target_h, target_w) canvas (preprocessing.py:39-55)."""
    scale = min(target_w / w, target_h / h)
    new_w, new_h = int(w * scale), int(h * scale)
    return new_w, new_h, (target_w - new_w) // 2, (target_h - new_h) // 2


# ---------------------------------------------------------------- tap tables
def _sinc(x):
    x = np.asarray(x, dtype=np.float64)
    px = np.pi * np.where(x == 0, 1.0, x)
    return np.where(x == 0, 1.0, np.where(x == np.floor(x), 0.0, np.sin(px) / px))      # exact zeros at the integers


def _keys(x, a=-0.75):
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(x <= 1, ((a + 2) * x - (a + 3)) * x * x + 1, np.where(x < 2, ((a * x - 5 * a) * x + 8 * a) * x - 4 * a, 0.0))


def resample_taps_np(method: int, src: int, dst: int) -> Tuple[np.ndarray, np.ndarray]:
    """float64 restatement of ``mrisr_resample_taps``: ``(index int64 [dst][K], weight float64 [dst][K])``."""
    if method not in (LINEAR, CUBIC, AREA, LANCZOS4):
        raise ValueError(f"unknown resampling method {method}")
    if method == AREA and dst > src:
        method = LINEAR
    d = np.arange(dst, dtype=np.int64)
    scale = src / dst
    if method == AREA:
        lo, hi = (d * src) / dst, ((d + 1) * src) / dst
        first = np.floor(lo).astype(np.int64)
        k = int((np.ceil(hi).astype(np.int64) - first).max())
        i = first[:, None] + np.arange(k)[None, :]
        ov = np.minimum(i + 1.0, hi[:, None]) - np.maximum(i.astype(np.float64), lo[:, None])
        w = np.where(ov > 0, ov / np.minimum(scale, src - lo)[:, None], 0.0)
    else:
        k = {LINEAR: 2, CUBIC: 4, LANCZOS4: 8}[method]
        s = (d + 0.5) * scale - 0.5
        fl = np.floor(s)
        off = np.arange(k) - (k // 2 - 1)
        i = fl.astype(np.int64)[:, None] + off[None, :]
        x = (s - fl)[:, None] - off[None, :]
        if method == LINEAR:
            w = 1.0 - np.abs(x)
        elif method == CUBIC:
            w = _keys(x)
        else:
            w = np.where(np.abs(x) < 4, _sinc(x) * _sinc(x / 4), 0.0)
            w = w / w.sum(1, keepdims=True)
    if k > MAX_TAPS:
        raise ValueError(f"{src} -> {dst} needs {k} taps per sample (at most {MAX_TAPS})")
    return np.clip(i, 0, src - 1), w


def resample_taps(method: int, src: int, dst: int) -> Tuple[np.ndarray, np.ndarray]:
    """The library's tables (host helper, no GPU needed): ``(index int16 [dst][K], weight float32 [dst][K])``."""
    index = np.zeros((max(int(dst), 0), MAX_TAPS), dtype=np.int16)
    weight = np.zeros((max(int(dst), 0), MAX_TAPS), dtype=np.float32)
    k = C.c_int(0)
    L.check(L.load().mrisr_resample_taps(int(method), int(src), int(dst), MAX_TAPS, C.addressof(k), index.ctypes.data,
                                         weight.ctypes.data), "mrisr_resample_taps")
    return np.ascontiguousarray(index[:, :k.value]), np.ascontiguousarray(weight[:, :k.value])


def _device_taps(method, src, dst, device):
    key = (int(method), int(src), int(dst), str(device))
    if key not in _TAPS:
        index, weight = resample_taps(method, src, dst)
        _TAPS[key] = (torch.from_numpy(index).to(device), torch.from_numpy(weight).to(device))
    return _TAPS[key]


# ---------------------------------------------------------------- the resize
def _to_u8(v: np.ndarray) -> np.ndarray:
    return np.clip(v * 255, 0, 255).astype(np.uint8)          # extraction_utils.py:131,162: truncation


def resample_letterbox_host(img: np.ndarray, target_size: Sequence[int], method: int = LANCZOS4, pad_value: float = 0.0,
                            clip: bool = False, as_uint8: bool = False) -> np.ndarray:
    """float64 restatement of the whole resize for one (H,W) image: columns, then rows, with the tables of
    ``resample_taps_np``; the block on a ``(target_h, target_w)`` canvas of ``pad_value`` (``target_size`` is (width, height))."""
    x = np.asarray(img, dtype=np.float64)
    h, w = x.shape
    tw, th = int(target_size[0]), int(target_size[1])
    new_w, new_h, x_off, y_off = letterbox_geometry(h, w, tw, th)
    if new_w < 1 or new_h < 1:
        raise ValueError(f"{h} x {w} does not fit {th} x {tw}")
    xi, xw = resample_taps_np(method, w, new_w)
    yi, yw = resample_taps_np(method, h, new_h)
    t = (x[:, xi] * xw[None]).sum(2)                   # (h, new_w)
    block = (t[yi] * yw[:, :, None]).sum(1)            # (new_h, new_w)
    if clip:
        block = np.clip(block, 0, 1)
    canvas = np.full((th, tw), float(pad_value), dtype=np.float64)
    canvas[y_off:y_off + new_h, x_off:x_off + new_w] = block
    return _to_u8(canvas) if as_uint8 else canvas


def resample_letterbox_f32(x: torch.Tensor, target_size: Sequence[int], method: int = LANCZOS4, pad_value: float = 0.0,
                           clip: bool = False, as_uint8: bool = False) -> torch.Tensor:
    """x: (H,W) or (B,H,W) float32 CUDA tensor -> (B, target_h, target_w) float32, or uint8 (``clamp(v * 255, 0, 255)``
    truncated) with ``as_uint8``: every image resized to fit ``target_size`` = (width, height) with its aspect ratio kept and
    centred on a canvas of ``pad_value``.  One launch; bitwise reproducible.  CPU tensors raise."""
    _need_cuda(x, "resample_letterbox_f32")
    if x.dtype != torch.float32 or x.dim() not in (2, 3) or x.numel() == 0:
        raise ValueError(f"expected a non-empty float32 tensor (H,W) or (B,H,W), got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    if x.dim() == 2:
        x = x.unsqueeze(0)
    b, h, w = x.shape
    tw, th = int(target_size[0]), int(target_size[1])
    new_w, new_h, x_off, y_off = letterbox_geometry(h, w, tw, th)
    return _resample_block(x, (new_h, new_w), (th, tw), (y_off, x_off), method, pad_value, clip, as_uint8)


def _resample_block(x, new_hw, canvas_hw, off_yx, method, pad_value, clip, as_uint8):
    """The entry point with explicit geometry (shape rules are the library's)."""
    b, h, w = x.shape
    if new_hw[0] < 1 or new_hw[1] < 1:
        raise ValueError(f"{h} x {w} does not fit {canvas_hw[0]} x {canvas_hw[1]}")
    yi, yw = _device_taps(method, h, new_hw[0], x.device)
    xi, xw = _device_taps(method, w, new_hw[1], x.device)
    out = torch.empty((b, canvas_hw[0], canvas_hw[1]), dtype=torch.uint8 if as_uint8 else torch.float32, device=x.device)
    L.call("mrisr_f32_resample_letterbox", x.data_ptr(), b, h, w, yi.data_ptr(), yw.data_ptr(), yi.shape[1], int(new_hw[0]),
           xi.data_ptr(), xw.data_ptr(), xi.shape[1], int(new_hw[1]), int(canvas_hw[0]), int(canvas_hw[1]), int(off_yx[0]),
           int(off_yx[1]), float(pad_value), int(bool(clip)), None if as_uint8 else out.data_ptr(),
           out.data_ptr() if as_uint8 else None, L.stream_ptr())
    return out


# ---------------------------------------------------------------- the chain
def normalise_slice_np(slice_f32: np.ndarray) -> np.ndarray:
    """The percentile window of one float32 slice in numpy's float32 arithmetic (preprocessing.py:139-163 and :336-343, which
    agree once the window clips): zeros for a slice whose two percentiles are equal."""
    a = np.asarray(slice_f32, dtype=np.float32)
    lo, hi = imageops.percentile_bounds_np(a, 0.5, 99.5)
    if hi == lo:
        return np.zeros_like(a)
    return ((np.clip(a, lo, hi) - lo) / np.float32(hi - lo)).astype(np.float32)


def extract_pairs_host(volume: np.ndarray, n_slices: int = 10, lower_percent: float = 0.2, upper_percent: float = 0.8,
                       target_size: Sequence[int] = (256, 256), kspace_crop_factor: float = 0.5, noise_std: float = 5.0,
                       kspace_noise=None, rng: Optional[np.random.Generator] = None) -> dict:
    """The whole chain in NumPy for an (X,Y,Z) volume: float32 for the window (as the reference), float64 after it.

    ``kspace_noise``: one ``(noise_real, noise_imag)`` pair per selected slice (a replayed reference draw), else drawn from
    ``rng``.  Returns ``indices``; per slice the lists ``hr_plane`` / ``lr_plane`` (what the reference hands to ``cv2.resize``:
    the normalised slice, the simulated and clipped slice), ``hr`` / ``lr`` (float64 canvases), ``hr_u8`` / ``lr_u8``; and
    ``hr_dsize`` / ``lr_dsize`` (width, height of the resized block) with ``hr_interpolation`` / ``lr_interpolation``."""
    vol = np.asarray(volume)
    if vol.ndim != 3:
        raise ValueError(f"expected an (X,Y,Z) volume, got {vol.shape}")
    tw, th = int(target_size[0]), int(target_size[1])
    lr_size = (tw // 2, th // 2)
    idx = slice_indices(vol.shape[2], n_slices, lower_percent, upper_percent)
    h, w = vol.shape[:2]
    out = {"indices": idx, "hr_plane": [], "lr_plane": [], "hr": [], "lr": [], "hr_u8": [], "lr_u8": [],
           "hr_dsize": letterbox_geometry(h, w, tw, th)[:2], "lr_dsize": letterbox_geometry(h, w, *lr_size)[:2],
           "hr_interpolation": LANCZOS4, "lr_interpolation": AREA}
    for k, i in enumerate(idx):
        norm = normalise_slice_np(vol[:, :, i].astype(np.float32))
        sim = lowfield.simulate_low_field_f32_host(norm, kspace_crop_factor, noise_std,
                                                   None if kspace_noise is None else kspace_noise[k], rng)["clipped"]
        hr = resample_letterbox_host(norm, (tw, th), LANCZOS4)
        lr = resample_letterbox_host(sim, lr_size, AREA)
        out["hr_plane"].append(norm)
        out["lr_plane"].append(sim)
        out["hr"].append(hr)
        out["lr"].append(lr)
        out["hr_u8"].append(_to_u8(hr))
        out["lr_u8"].append(_to_u8(lr))
    return out


def extract_pairs(volume: torch.Tensor, n_slices: int = 10, lower_percent: float = 0.2, upper_percent: float = 0.8,
                  target_size: Sequence[int] = (256, 256), kspace_crop_factor: float = 0.5, noise_std: float = 5.0, seeds=None,
                  noise=None):
    """volume: (X,Y,Z) float32 CUDA tensor of finite values -> ``(indices, hr_u8 (S, th, tw), lr_u8 (S, th // 2, tw // 2))``:
    the slice numbers (NumPy) and the paired uint8 images on the device, from ONE batch of the selected slices
    ``volume[:, :, idx]``.  ``seeds`` / ``noise`` (image-space planes (S,X,Y)) / ``noise_std`` as in
    ``lowfield.simulate_low_field_f32``."""
    _need_cuda(volume, "extract_pairs")
    if volume.dtype != torch.float32 or volume.dim() != 3 or volume.numel() == 0:
        raise ValueError(f"expected a non-empty float32 volume (X,Y,Z), got {volume.dtype} {tuple(volume.shape)}")
    tw, th = int(target_size[0]), int(target_size[1])
    idx = slice_indices(volume.shape[2], n_slices, lower_percent, upper_percent)
    sel = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(volume.device)
    slices = volume.index_select(2, sel).permute(2, 0, 1).contiguous()
    norm = imageops.normalise_percentile_f32(slices)[:, 0]
    hr = resample_letterbox_f32(norm, (tw, th), LANCZOS4, as_uint8=True)
    sim = lowfield.simulate_low_field_f32(norm, kspace_crop_factor, noise_std, seeds=seeds, noise=noise)
    lr = resample_letterbox_f32(sim, (tw // 2, th // 2), AREA, as_uint8=True)
    return idx, hr, lr
