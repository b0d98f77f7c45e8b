"""Rigid registration of whole volumes on the device (extension): the transform between two scans of one
head is ESTIMATED - six parameters, by maximising the normalised mutual information of their joint histogram - instead of being
taken from the two NIfTI headers.

``joint_histogram_np``  the specification of the similarity measure's first half: every rounding fixed through ``reslice_np`` and
                        ``source_coordinates_np``, so that the kernel (``csrc/volume_register.hip``) equals it as integers.
``nmi_np``              normalised mutual information ``(H_f + H_m) / H_fm`` of a joint histogram.
``rigid_world``         the 4 x 4 fixed world -> moving world matrix of the parameters ``(tx, ty, tz mm; rx, ry, rz degrees)``.
``candidate_matrix``    the (3, 4) fixed voxel index -> moving voxel index matrix of the parameters and the two affines.
``compass_search``      the search: ONE function for the specification and the device path, only ``cost_batch`` differs.
``register_rigid_np``   the specification of the whole operation (numpy cost).
``joint_histogram``, ``nmi``, ``register_rigid``   the device path.  There is no CPU path: CPU tensors raise.

Not built: affine or deformable transforms, smoothing of the histogram (Parzen windows), masks in the cost, a coarse global
search - the capture range is what a start from the headers (``p0 = 0``) allows.
"""
from __future__ import annotations

import logging
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from .utils.nifti import _check_affine, grid_matrix
from .volume_reslice import _check_matrix, _check_tensor, reslice_np, source_coordinates_np

logger = logging.getLogger(__name__)

BINS = (16, 32, 64)
STRIDES = (1, 2, 4, 8)
MAX_CANDIDATES = 16
MIN_SAMPLES_PER_AXIS = 8
MAX_ITERATIONS = 1000      # per level: a bound on the search loop, far above what a registration takes


class RigidResult(NamedTuple):
    p: np.ndarray                # (6,) float64: tx, ty, tz in mm, rx, ry, rz in degrees
    world: np.ndarray            # (4, 4): fixed world -> moving world
    matrix: np.ndarray           # (3, 4): fixed voxel index -> continuous moving voxel index (``reslice``'s matrix)
    value: float                 # the normalised mutual information reached, at the last level's stride
    n_evaluations: int
    trace: list                  # one dict per ``cost_batch`` call (``compass_search``)


# ---------------------------------------------------------------- numpy specification

def _check_range(r, bins, what):
    """-> (float32 lo, float32 scale).  ``scale = float32(bins) / (hi - lo)``, everything float32."""
    lo, hi = (float(x) for x in r)
    f32 = np.float32
    with np.errstate(all="ignore"):
        lo32, hi32 = f32(lo), f32(hi)
        scale = f32(bins) / (hi32 - lo32)
    if not (np.isfinite(lo) and np.isfinite(hi) and np.isfinite(lo32) and np.isfinite(hi32) and hi32 > lo32 and np.isfinite(scale)):
        raise ValueError(f"{what} must be finite in float32 with hi > lo (and a finite bins / (hi - lo)), got ({lo}, {hi})")
    return lo32, scale


def _check_bins_stride(bins, stride):
    if bins not in BINS:
        raise ValueError(f"bins must be one of {BINS}, got {bins}")
    if stride not in STRIDES:
        raise ValueError(f"stride must be one of {STRIDES}, got {stride}")


def bin_np(v: np.ndarray, lo32, scale, bins: int) -> np.ndarray:
    """The bin of the float32 values ``v`` (no NaN): ``min(bins - 1, max(0, int((v - lo) * scale)))`` in float32, one rounded
    operation at a time; the clamp is applied to the float before the conversion (the same bins wherever the conversion is defined,
    and a defined bin for +-infinity and products beyond the integers)."""
    with np.errstate(all="ignore"):
        x = (np.asarray(v, dtype=np.float32) - lo32) * scale
    return np.minimum(np.clip(x, np.float32(0), np.float32(bins)).astype(np.int64), bins - 1)


def strided_matrix(m, stride: int) -> np.ndarray:
    """``m`` with its first three columns times ``stride`` (exact for a power of two): sample index -> moving voxel index."""
    ms = _check_matrix(m).copy()
    ms[:, :3] *= float(stride)
    return _check_matrix(ms)


def joint_histogram_np(fixed, moving, m, bins, stride, fixed_range, moving_range) -> np.ndarray:
    """int64 (bins, bins).  The samples are ``fixed[::s, ::s, ::s]``; with ``m' = strided_matrix(m, s)`` their moving values are
    ``reslice_np(moving, m', sampled shape, "linear")`` and the inside test is ``source_coordinates_np(m', ...)``.  A sample counts
    when it is inside and neither value is NaN: ``H[bin_np(fixed value), bin_np(moving value)] += 1``."""
    fixed, moving = np.asarray(fixed), np.asarray(moving)
    for v, what in ((fixed, "fixed"), (moving, "moving")):
        if v.dtype != np.float32 or v.ndim != 3 or v.size == 0:
            raise ValueError(f"joint_histogram_np: {what} must be a non-empty float32 volume (X,Y,Z), got {v.dtype} {v.shape}")
    _check_bins_stride(bins, stride)
    flo, fscale = _check_range(fixed_range, bins, "fixed_range")
    mlo, mscale = _check_range(moving_range, bins, "moving_range")
    ms = strided_matrix(m, stride)
    fs = fixed[::stride, ::stride, ::stride]
    mv = reslice_np(moving, ms, fs.shape, "linear")
    _, inside = source_coordinates_np(ms, fs.shape, moving.shape)
    ok = inside & ~np.isnan(fs) & ~np.isnan(mv)
    cell = bin_np(fs[ok], flo, fscale, bins) * bins + bin_np(mv[ok], mlo, mscale, bins)
    return np.bincount(cell, minlength=bins * bins).astype(np.int64).reshape(bins, bins)


def _entropy_np(counts: np.ndarray, n: int) -> float:
    p = counts[counts > 0].astype(np.float64) / float(n)
    return float(-np.sum(p * np.log(p)))


def nmi_np(H, min_count=0):
    """-> (float64 value, int64 count).  ``N = sum H``; ``N < max(min_count, 1)``: ``-inf``.  Else ``P = H / N``, the entropies
    ``-sum p ln p`` over the positive cells of the row sums (``H_f``), the column sums (``H_m``) and the cells in C order
    (``H_fm``): ``(H_f + H_m) / H_fm``, and ``0.0`` where ``H_fm == 0``.  No smoothing of the histogram."""
    H = np.asarray(H)
    if H.ndim != 2 or H.shape[0] != H.shape[1] or H.dtype.kind not in "iu" or (H < 0).any() or int(min_count) < 0:
        raise ValueError(f"nmi_np takes a square histogram of non-negative integers and a non-negative min_count, got {H.dtype} {H.shape}")
    H = H.astype(np.int64)
    n = int(H.sum())
    if n < max(int(min_count), 1):
        return float("-inf"), np.int64(n)
    hf, hm, hfm = _entropy_np(H.sum(axis=1), n), _entropy_np(H.sum(axis=0), n), _entropy_np(H.reshape(-1), n)
    return (0.0 if hfm == 0.0 else (hf + hm) / hfm), np.int64(n)


def volume_centre(fixed_affine, shape) -> np.ndarray:
    """(3,) world position of the fixed volume's centre voxel coordinate ``(n - 1) / 2``."""
    a = _check_affine(fixed_affine, "fixed_affine")
    return a[:3, :3] @ ((np.asarray(shape[:3], dtype=np.float64) - 1) / 2) + a[:3, 3]


def rotation_np(rx, ry, rz) -> np.ndarray:
    """``Rz Ry Rx`` of the angles in degrees."""
    ax, ay, az = np.deg2rad([float(rx), float(ry), float(rz)])
    mx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    my = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    mz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return (mz @ my @ mx) + 0.0      # + 0.0: no negative zeros, so that p = 0 gives the identity to the last bit


def _check_p(p) -> np.ndarray:
    p = np.asarray(p, dtype=np.float64)
    if p.shape != (6,) or not np.isfinite(p).all():
        raise ValueError(f"the rigid parameters are six finite numbers (tx, ty, tz, rx, ry, rz), got {p.tolist()}")
    return p


def rigid_world(p, centre) -> np.ndarray:
    """(4, 4): fixed world -> moving world, ``x -> R (x - c) + c + t`` with ``R = Rz Ry Rx`` (degrees) and ``c = centre``."""
    p, c = _check_p(p), np.asarray(centre, dtype=np.float64).reshape(3)
    w = np.eye(4)
    w[:3, :3] = rotation_np(*p[3:])
    w[:3, 3] = (c - w[:3, :3] @ c) + p[:3]
    return w


def candidate_matrix(p, fixed_affine, moving_affine, centre) -> np.ndarray:
    """(3, 4): the first three rows of ``inv(A_mov) W(p) A_fix``, solved as ``grid_matrix`` solves it; ``p = 0`` gives
    ``grid_matrix(A_mov, A_fix)`` to the last bit."""
    return grid_matrix(moving_affine, rigid_world(p, centre) @ _check_affine(fixed_affine, "fixed_affine"))


def corner_displacement(world_a, world_b, fixed_affine, shape) -> float:
    """The worst distance in mm, over the eight corner voxels of the fixed volume, between their images under two fixed world ->
    moving world matrices."""
    a = _check_affine(fixed_affine, "fixed_affine")
    n = np.asarray(shape[:3], dtype=np.float64) - 1
    corners = np.array([[i, j, k, 1.0] for i in (0.0, n[0]) for j in (0.0, n[1]) for k in (0.0, n[2])]).T
    world = a @ corners
    d = (np.asarray(world_a) @ world - np.asarray(world_b) @ world)[:3]
    return float(np.sqrt((d * d).sum(axis=0)).max())


# ---------------------------------------------------------------- the search

def compass_search(cost_batch, p0, levels, max_iterations=MAX_ITERATIONS):
    """Maximises ``cost_batch`` over the six parameters -> ``(p, value, n_evaluations, trace)``.

    ``cost_batch(ps, stride)``: ``ps`` a (K, 6) float64 array, K <= 16 -> K values (``-inf``: not enough samples).  A level is
    ``(stride, step[6], min_translation_step)``.  At each level: evaluate ``p`` (one call, K = 1); then, while
    ``step[0] >= min_translation_step``, score the 12 candidates ``p +- step[a] e_a`` - axis ascending, ``+`` before ``-`` - in
    ONE call; move to the first argmax only if it is strictly greater than the best so far, otherwise halve all six steps.
    ``trace``: one dict per call - ``level``, ``stride``, ``kind`` (``"start"`` / ``"probe"``), ``p`` (the point probed around),
    ``step``, ``values``, ``accepted`` (index of the candidate taken, or None), ``best`` (after the call)."""
    p = _check_p(p0).copy()
    trace, n_eval, best = [], 0, float("-inf")
    for li, (stride, step, min_t) in enumerate(levels):
        step = np.asarray(step, dtype=np.float64).copy()
        if step.shape != (6,) or not (step > 0).all() or not np.isfinite(step).all() or not min_t > 0:
            raise ValueError(f"level {li}: six positive steps and a positive stop, got {step.tolist()} and {min_t}")
        best = float(np.asarray(cost_batch(p[None].copy(), stride), dtype=np.float64).reshape(1)[0])
        n_eval += 1
        trace.append({"level": li, "stride": stride, "kind": "start", "p": tuple(p), "step": tuple(step), "values": (best,),
                      "accepted": None, "best": best})
        for _ in range(max_iterations):
            if not step[0] >= min_t:
                break
            cands = np.repeat(p[None], 12, axis=0)
            for a in range(6):
                cands[2 * a, a] += step[a]
                cands[2 * a + 1, a] -= step[a]
            vals = np.asarray(cost_batch(cands, stride), dtype=np.float64).reshape(12)
            n_eval += 12
            j = int(np.argmax(vals))                                  # the first of equal maxima
            entry = {"level": li, "stride": stride, "kind": "probe", "p": tuple(p), "step": tuple(step),
                     "values": tuple(float(v) for v in vals), "accepted": None}
            if vals[j] > best:
                p, best = cands[j].copy(), float(vals[j])
                entry["accepted"] = j
            else:
                step = step / 2
            entry["best"] = best
            trace.append(entry)
    return p, best, n_eval, trace


def voxel_size(fixed_affine) -> float:
    """The mean column norm of the affine's 3 x 3 block (mm)."""
    a = _check_affine(fixed_affine, "fixed_affine")
    return float(np.mean(np.linalg.norm(a[:3, :3], axis=0)))


def default_levels(fixed_affine):
    v = voxel_size(fixed_affine)
    return [(4, (2 * v,) * 3 + (2.0,) * 3, 0.5 * v), (2, (0.5 * v,) * 3 + (0.5,) * 3, v / 16)]


def effective_stride(shape, stride: int) -> int:
    """``stride``, halved while it leaves fewer than 8 samples on an axis (logged)."""
    if stride not in STRIDES:
        raise ValueError(f"stride must be one of {STRIDES}, got {stride}")
    s = stride
    while s > 1 and any(-(-int(n) // s) < MIN_SAMPLES_PER_AXIS for n in shape[:3]):
        s //= 2
    if s != stride:
        logger.info(f"stride {stride} leaves fewer than {MIN_SAMPLES_PER_AXIS} samples on an axis of {tuple(shape[:3])}: using {s}")
    return s


def sample_count(shape, stride: int) -> int:
    return int(np.prod([-(-int(n) // stride) for n in shape[:3]]))


def _prepare(fixed_shape, fixed_affine, moving_affine, bins, levels, p0):
    if bins not in BINS:
        raise ValueError(f"bins must be one of {BINS}, got {bins}")
    fa, ma = _check_affine(fixed_affine, "fixed_affine"), _check_affine(moving_affine, "moving_affine")
    levels = default_levels(fa) if levels is None else list(levels)
    levels = [(effective_stride(fixed_shape, int(s)), step, min_t) for s, step, min_t in levels]
    p0 = np.zeros(6) if p0 is None else _check_p(p0)
    return fa, ma, levels, p0, volume_centre(fa, fixed_shape)


def _result(search, fa, ma, centre) -> RigidResult:
    p, value, n_eval, trace = search
    return RigidResult(p, rigid_world(p, centre), candidate_matrix(p, fa, ma, centre), value, n_eval, trace)


def register_rigid_np(fixed, fixed_affine, moving, moving_affine, bins=64, levels=None, p0=None) -> RigidResult:
    """The specification of ``register_rigid``: ``compass_search`` over ``nmi_np(joint_histogram_np(...))``.  The ranges are the
    (NaN-ignoring) minimum and maximum of each volume; ``min_count`` is a quarter of the level's sample count; ``levels``
    defaults to ``default_levels(fixed_affine)``, every stride through ``effective_stride``."""
    fixed, moving = np.asarray(fixed), np.asarray(moving)
    fa, ma, levels, p0, centre = _prepare(fixed.shape, fixed_affine, moving_affine, bins, levels, p0)
    franges = (float(np.nanmin(fixed)), float(np.nanmax(fixed)))
    mranges = (float(np.nanmin(moving)), float(np.nanmax(moving)))

    def cost_batch(ps, stride):
        min_count = sample_count(fixed.shape, stride) // 4
        return [nmi_np(joint_histogram_np(fixed, moving, candidate_matrix(p, fa, ma, centre), bins, stride, franges, mranges),
                       min_count)[0] for p in ps]
    return _result(compass_search(cost_batch, p0, levels), fa, ma, centre)


# ---------------------------------------------------------------- device

def _matrices_arg(ms):
    ms = np.asarray(ms, dtype=np.float64)
    if ms.ndim == 2:
        ms = ms[None]
    if ms.ndim != 3 or ms.shape[1:] != (3, 4) or not 1 <= ms.shape[0] <= MAX_CANDIDATES or not np.isfinite(ms).all():
        raise ValueError(f"1..{MAX_CANDIDATES} finite (3, 4) matrices are expected, got shape {ms.shape}")
    return ms.shape[0], (L.C.c_double * (12 * ms.shape[0]))(*ms.reshape(-1).tolist())


def joint_histogram(fixed: torch.Tensor, moving: torch.Tensor, ms, bins, stride, fixed_range, moving_range, out=None) -> torch.Tensor:
    """fixed, moving: contiguous (X,Y,Z) float32 CUDA tensors; ms: (K, 3, 4) or (3, 4), K <= 16 (host, float64) -> the int64 CUDA
    tensor (K, bins, bins), equal to ``joint_histogram_np`` of every matrix.  ``out``: such a tensor to overwrite.  A memset and
    one launch, no host synchronisation."""
    f, mv = _check_tensor(fixed, (torch.float32,), "joint_histogram"), _check_tensor(moving, (torch.float32,), "joint_histogram")
    _check_bins_stride(bins, stride)
    _check_range(fixed_range, bins, "fixed_range")
    _check_range(moving_range, bins, "moving_range")
    k, arg = _matrices_arg(ms)
    if out is None:
        out = torch.empty((k, bins, bins), dtype=torch.int64, device=f.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == (k, bins, bins)
              and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous int64 CUDA tensor of shape {(k, bins, bins)}")
    L.call("mrisr_f32_volume_joint_histogram", f.data_ptr(), *f.shape, mv.data_ptr(), *mv.shape, arg, k, int(stride), int(bins),
           float(fixed_range[0]), float(fixed_range[1]), float(moving_range[0]), float(moving_range[1]), out.data_ptr(), L.stream_ptr())
    return out


def nmi(hist: torch.Tensor, min_count=0):
    """hist: contiguous int64 CUDA tensor (K, bins, bins) or (bins, bins) -> (values float64 (K,), counts int64 (K,)), CUDA tensors,
    by ``nmi_np``'s rules.  One launch, no host synchronisation."""
    if not isinstance(hist, torch.Tensor) or not hist.is_cuda:
        raise ValueError("nmi runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor")
    h = hist[None] if hist.dim() == 2 else hist
    if h.dtype != torch.int64 or h.dim() != 3 or h.shape[1] != h.shape[2] or h.shape[1] not in BINS or not h.is_contiguous() \
            or not 1 <= h.shape[0] <= MAX_CANDIDATES or int(min_count) < 0:
        raise ValueError(f"nmi: expected a contiguous int64 tensor (K <= {MAX_CANDIDATES}, bins, bins) with bins in {BINS} and a "
                         f"non-negative min_count, got {hist.dtype} {tuple(hist.shape)}")
    values = torch.empty(h.shape[0], dtype=torch.float64, device=h.device)
    counts = torch.empty(h.shape[0], dtype=torch.int64, device=h.device)
    L.call("mrisr_joint_histogram_nmi", h.data_ptr(), h.shape[0], h.shape[1], int(min_count), values.data_ptr(), counts.data_ptr(),
           L.stream_ptr())
    return values, counts


def volume_range(v: torch.Tensor):
    """(lo, hi) host floats of a CUDA volume, NaN ignored: one read (not on the hot path)."""
    finite = torch.where(torch.isnan(v), v.new_tensor(float("inf")), v).amin(), torch.where(torch.isnan(v), v.new_tensor(float("-inf")), v).amax()
    lo, hi = torch.stack(finite).cpu().tolist()
    return lo, hi


def register_rigid(fixed: torch.Tensor, fixed_affine, moving: torch.Tensor, moving_affine, bins=64, levels=None, p0=None) -> RigidResult:
    """The device path of ``register_rigid_np``: the same ``compass_search`` over a ``cost_batch`` that launches
    ``joint_histogram`` and ``nmi`` for the K candidates and reads their K values back - ONE device-to-host read per search
    iteration (``trace[i]["host_reads"] == 1``).  The ranges of the two volumes are read once per registration."""
    f, mv = _check_tensor(fixed, (torch.float32,), "register_rigid"), _check_tensor(moving, (torch.float32,), "register_rigid")
    fa, ma, levels, p0, centre = _prepare(f.shape, fixed_affine, moving_affine, bins, levels, p0)
    franges, mranges = volume_range(f), volume_range(mv)
    hist = torch.empty((MAX_CANDIDATES, bins, bins), dtype=torch.int64, device=f.device)
    reads = []

    def cost_batch(ps, stride):
        ms = np.stack([candidate_matrix(p, fa, ma, centre) for p in ps])
        values, _ = nmi(joint_histogram(f, mv, ms, bins, stride, franges, mranges, out=hist[:len(ps)]), sample_count(f.shape, stride) // 4)
        host = values.cpu().numpy()                                  # the one synchronisation of this iteration
        reads.append(1)
        return host
    search = compass_search(cost_batch, p0, levels)
    for entry, n in zip(search[3], reads):
        entry["host_reads"] = n
    assert len(search[3]) == len(reads)
    return _result(search, fa, ma, centre)
