"""The argument checks of the volume tools (``volume_*.py``), once.  Every check raises ``ValueError`` with a
message that begins with the caller's ``what`` and returns the checked argument.  This module imports no ``volume_*`` module, so
that every one of them may import it; a check that a single tool uses stays in that tool.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L

MAX_VOXELS = 2 ** 31 - 1
MAX_EXTENT = 1024                  # the longest axis of the distance transform: the device path stages whole lines in LDS
MIN_CLASSES, MAX_CLASSES = 2, 6    # tissue classes
NO_CPU = "runs on an MI355X through libmrisr.so only (no CPU fallback)"


# ---------------------------------------------------------------- shapes, matrices, scalars

def check_shape(shape, what) -> tuple:
    shape = tuple(int(d) for d in shape)
    if len(shape) != 3 or any(d < 1 for d in shape):
        raise ValueError(f"{what} must be three positive extents, got {shape}")
    if shape[0] * shape[1] * shape[2] > MAX_VOXELS:
        raise ValueError(f"{what} {shape} has more than 2^31 - 1 voxels")
    return shape


def check_matrix(m) -> np.ndarray:
    m = np.asarray(m, dtype=np.float64)
    if m.shape != (3, 4) or not np.isfinite(m).all():
        raise ValueError(f"the grid matrix must be (3, 4) and finite, got shape {m.shape}: {m.tolist()}")
    return np.ascontiguousarray(m)


def matrix_arg(m):
    m = check_matrix(m)
    return (L.C.c_double * 12)(*m.reshape(-1).tolist())


def check_extents(shape, what):
    if len(shape) != 3:
        raise ValueError(f"{what}: expected a volume (X, Y, Z), got {tuple(shape)}")
    if max(shape) > MAX_EXTENT:
        raise ValueError(f"{what}: an axis of {max(shape)} voxels is longer than the limit of {MAX_EXTENT}")


def check_weights(weights, what="weights") -> tuple:
    """-> three float32 values, finite and positive."""
    try:
        with np.errstate(over="ignore"):
            w = tuple(np.float32(x) for x in weights)
    except (TypeError, ValueError):
        w = ()
    if len(w) != 3 or not all(np.isfinite(x) and x > 0 for x in w):
        raise ValueError(f"{what} are three finite positive numbers (float32), got {weights!r}")
    return w


def check_spacing(spacing) -> tuple:
    """-> the weights of the distance transform: ``float32(s * s)`` per axis, the product taken in float64."""
    try:
        s = tuple(float(x) for x in spacing)
    except (TypeError, ValueError):
        s = ()
    if len(s) != 3 or not all(math.isfinite(x) and x > 0 for x in s):
        raise ValueError(f"spacing is three finite positive voxel sizes, got {spacing!r}")
    return check_weights(tuple(x * x for x in s), "the squared voxel sizes")


def check_classes(classes) -> int:
    if isinstance(classes, bool) or not isinstance(classes, (int, np.integer)) or not MIN_CLASSES <= classes <= MAX_CLASSES:
        raise ValueError(f"classes must be an integer in {MIN_CLASSES}..{MAX_CLASSES}, got {classes!r}")
    return int(classes)


def three_sigmas(sigmas_vox) -> list:
    """-> the three sigmas as floats; the caller makes its taps of them and bounds their radius."""
    try:
        s = [float(x) for x in sigmas_vox]
    except (TypeError, ValueError):
        raise ValueError(f"three sigmas in voxels are expected, got {sigmas_vox!r}") from None
    if len(s) != 3:
        raise ValueError(f"three sigmas in voxels are expected, got {sigmas_vox!r}")
    return s


# ---------------------------------------------------------------- numpy arrays

def _noun(ndim):
    return "volume (X, Y, Z)" if ndim == 3 else "array"


def volume_np(v, what, ndim=3, limit=False) -> np.ndarray:
    """A non-empty float32 array; ``ndim`` 3: a volume, None: any shape.  ``limit``: ``check_shape``'s bound on the voxel count."""
    v = np.asarray(v)
    if v.dtype != np.float32 or v.size == 0 or (ndim is not None and v.ndim != ndim):
        raise ValueError(f"{what}: expected a non-empty float32 {_noun(ndim)}, got {v.dtype} {v.shape}")
    if limit:
        check_shape(v.shape, f"{what}: the volume's shape")
    return v


def u8_np(a, shape, what, ndim=None) -> np.ndarray:
    """A non-empty uint8 or bool array - a mask, labels - of ``shape`` (None: any), viewed as uint8.  Here ``what`` names the array."""
    a = np.asarray(a)
    if a.dtype not in (np.uint8, np.bool_) or a.size == 0 or (shape is not None and a.shape != tuple(shape)) \
            or (ndim is not None and a.ndim != ndim):
        raise ValueError(f"{what} must be a non-empty uint8 or bool {_noun(ndim)}" + (f" of shape {tuple(shape)}" if shape is not None else "")
                         + f", got {a.dtype} {a.shape}")
    return a.view(np.uint8)


def mask_np(mask, shape, what) -> np.ndarray:
    return u8_np(mask, shape, f"{what}: the mask")


# ---------------------------------------------------------------- CUDA tensors

def cuda_tensor(t, dtypes, what, name=None, ndim=None, shape=None, limit=False) -> torch.Tensor:
    """A non-empty contiguous CUDA tensor of one of ``dtypes``; ``ndim`` 3: a volume; ``shape``: exactly that shape; ``name``: the
    argument the message speaks of; ``limit``: ``check_shape``'s bound on the voxel count.  Nothing is copied."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        got = "a CPU tensor" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what} {NO_CPU}: {'expected' if name is None else name + ' must be'} a CUDA tensor, got {got}")
    if t.dtype not in dtypes or t.numel() == 0 or not t.is_contiguous() or (ndim is not None and t.dim() != ndim) \
            or (shape is not None and tuple(t.shape) != tuple(shape)):
        kinds = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise ValueError(f"{what}: {'expected' if name is None else name + ' must be'} a non-empty contiguous {kinds} "
                         f"{'volume (X, Y, Z)' if ndim == 3 else 'tensor'}" + (f" of shape {tuple(shape)}" if shape is not None else "")
                         + f", got {t.dtype} {tuple(t.shape)}{'' if t.is_contiguous() else ', not contiguous'}")
    if limit:
        check_shape(t.shape, f"{what}: the volume's shape")
    return t


def cuda_device(device, what) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{what} {NO_CPU}: expected a CUDA device")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())      # a tensor's device carries its index
    return device


def mask_tensor(mask, shape, what) -> torch.Tensor:
    """A contiguous uint8 or bool CUDA tensor of ``shape``, viewed as uint8 without a copy."""
    return cuda_tensor(mask, (torch.uint8, torch.bool), what, name="the mask", shape=shape).view(torch.uint8)


def out_like(out, like, others, what) -> torch.Tensor:
    """``out`` None: a new tensor like ``like``; else ``out``, which must be like it and none of ``others``."""
    if out is None:
        return torch.empty_like(like)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != like.shape or not out.is_contiguous() \
            or out.device != like.device or any(out.data_ptr() == o.data_ptr() for o in others):
        raise ValueError(f"{what}: out must be another contiguous float32 tensor of shape {tuple(like.shape)} on {like.device}")
    return out
