"""Rigid registration of whole volumes on the device (extension): the transform between two scans of one
head is ESTIMATED - six parameters, by maximising the normalised mutual information of their joint histogram - instead of being
taken from the two NIfTI headers.

``joint_histogram_np``  the specification of the similarity measure's first half: every rounding fixed through ``reslice_np`` and
                        ``source_coordinates_np``, so that the kernel (``csrc/volume_register.hip``) equals it as integers.
``nmi_np``              normalised mutual information ``(H_f + H_m) / H_fm`` of a joint histogram.
``rigid_world``         the 4 x 4 fixed world -> moving world matrix of the parameters ``(tx, ty, tz mm; rx, ry, rz degrees)``.
``candidate_matrix``    the (3, 4) fixed voxel index -> moving voxel index matrix of the parameters and the two affines.
``compass_search``      the search: ONE function for the specification and the device path, only ``cost_batch`` differs.
``mask_moments_np``, ``mask_centre_world``, ``rotation_grid``, ``coarse_start``   the start from far apart (``init="global"``): the
                        two masks' centres of mass brought together under every rotation of a coarse grid, all scored at stride 4.
``register_rigid_np``   the specification of the whole operation (numpy cost).
``joint_histogram``, ``nmi``, ``mask_moments``, ``register_rigid``   the device path.  There is no CPU path: CPU tensors raise.

A fixed-side mask in the cost (``fixed_mask`` / ``mask_cost=True``): a sample counts only where the mask is non-zero.

Not built: affine or deformable transforms, smoothing of the histogram (Parzen windows), a moving-side mask in the cost,
principal-axes starts.  With ``init="header"`` the capture range is what a start from the headers (``p0 = 0``) allows.
"""
from __future__ import annotations

import itertools
import logging
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from .utils.nifti import check_affine, grid_matrix
from ._volume_args import NO_CPU, check_matrix, cuda_tensor, u8_np
from .volume_reslice import reslice_np, source_coordinates_np

logger = logging.getLogger(__name__)

BINS = (16, 32, 64)
STRIDES = (1, 2, 4, 8)
MAX_CANDIDATES = 16
MIN_SAMPLES_PER_AXIS = 8
MAX_ITERATIONS = 1000      # per level: a bound on the search loop, far above what a registration takes
MAX_GRID = 1000            # rotations of a coarse grid
COARSE_STRIDE = 4


class RigidResult(NamedTuple):
    p: np.ndarray                # (6,) float64: tx, ty, tz in mm, rx, ry, rz in degrees
    world: np.ndarray            # (4, 4): fixed world -> moving world
    matrix: np.ndarray           # (3, 4): fixed voxel index -> continuous moving voxel index (``reslice``'s matrix)
    value: float                 # the normalised mutual information reached, at the last level's stride
    n_evaluations: int
    trace: list                  # one dict per ``cost_batch`` call (``compass_search``), after the ``coarse`` entry of ``init="global"``


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
    ms = check_matrix(m).copy()
    ms[:, :3] *= float(stride)
    return check_matrix(ms)


def joint_histogram_np(fixed, moving, m, bins, stride, fixed_range, moving_range, fixed_mask=None) -> np.ndarray:
    """int64 (bins, bins).  The samples are ``fixed[::s, ::s, ::s]``; with ``m' = strided_matrix(m, s)`` their moving values are
    ``reslice_np(moving, m', sampled shape, "linear")`` and the inside test is ``source_coordinates_np(m', ...)``.  A sample counts
    when it is inside and neither value is NaN: ``H[bin_np(fixed value), bin_np(moving value)] += 1``.  ``fixed_mask`` (uint8 or
    bool, the fixed shape): a sample counts only if ``fixed_mask[::s, ::s, ::s]`` is non-zero there as well."""
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
    if fixed_mask is not None:
        ok &= u8_np(fixed_mask, fixed.shape, "fixed_mask")[::stride, ::stride, ::stride] != 0
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
    a = check_affine(fixed_affine, "fixed_affine")
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
    return grid_matrix(moving_affine, rigid_world(p, centre) @ check_affine(fixed_affine, "fixed_affine"))


def corner_displacement(world_a, world_b, fixed_affine, shape) -> float:
    """The worst distance in mm, over the eight corner voxels of the fixed volume, between their images under two fixed world ->
    moving world matrices."""
    a = check_affine(fixed_affine, "fixed_affine")
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
    a = check_affine(fixed_affine, "fixed_affine")
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


# ---------------------------------------------------------------- the start from far apart

def mask_moments_np(mask) -> np.ndarray:
    """int64 (4,): ``(N, sum i, sum j, sum k)`` over the non-zero voxels ``(i, j, k)`` of a uint8 or bool volume."""
    mask = np.asarray(mask)
    if mask.dtype not in (np.uint8, np.bool_) or mask.ndim != 3 or mask.size == 0:
        raise ValueError(f"mask_moments_np takes a non-empty uint8 or bool volume (X,Y,Z), got {mask.dtype} {mask.shape}")
    nz = mask != 0
    per_axis = [nz.sum(axis=tuple(b for b in range(3) if b != a), dtype=np.int64) for a in range(3)]
    return np.array([per_axis[0].sum()] + [(c * np.arange(len(c), dtype=np.int64)).sum() for c in per_axis], dtype=np.int64)


def mask_centre_world(moments, affine) -> np.ndarray:
    """(3,) float64: the world position ``A[:3, :3] @ (sums / N) + A[:3, 3]`` of a mask's centre of mass from its moments."""
    mo = np.asarray(moments)
    if mo.shape != (4,) or mo.dtype.kind not in "iu":
        raise ValueError(f"the moments of a mask are four integers (N, sum i, sum j, sum k), got {mo.dtype} {mo.shape}")
    if int(mo[0]) <= 0:
        raise ValueError("the mask is empty: it has no centre of mass")
    a = check_affine(affine, "affine")
    return a[:3, :3] @ (mo[1:].astype(np.float64) / float(mo[0])) + a[:3, 3]


def rotation_grid(limit_deg, step_deg) -> np.ndarray:
    """(n^3, 3) float64: the angle triples ``(rx, ry, rz)`` over ``np.arange(-limit, limit + 1e-9, step)`` per axis, in the order of
    ``itertools.product`` (``rx`` slowest).  At most 1000 triples."""
    limit, step = float(limit_deg), float(step_deg)
    if not (np.isfinite(limit) and np.isfinite(step) and step > 0 and limit >= 0):
        raise ValueError(f"a rotation grid takes a non-negative limit and a positive step in degrees, got {limit_deg} and {step_deg}")
    if 2 * limit / step + 1 >= 12:                       # before np.arange: no huge allocation for a tiny step
        raise ValueError(f"a rotation grid of +-{limit} degrees in steps of {step} has more than {MAX_GRID} rotations")
    angles = np.arange(-limit, limit + 1e-9, step)
    if len(angles) ** 3 > MAX_GRID:
        raise ValueError(f"a rotation grid of +-{limit} degrees in steps of {step} has {len(angles) ** 3} rotations (at most {MAX_GRID})")
    return np.array(list(itertools.product(angles, repeat=3)), dtype=np.float64).reshape(-1, 3)


def coarse_start(cost_batch_many, centre_fixed, centre_moving, c, grid, stride):
    """The best of a grid of rotations, each with the translation that brings the two centres of mass together ->
    ``(p0, value, entry)``.  ONE function for the specification and the device path, only ``cost_batch_many`` differs.

    For every rotation ``R = rotation_np(*grid[n])`` the candidate is ``p = (t, rx, ry, rz)`` with
    ``t = centre_moving - (R (centre_fixed - c) + c)``: under ``rigid_world(p, c)`` the fixed centre lands on the moving one.
    ``cost_batch_many(ps, stride)``: ``ps`` (n, 6), any n -> n values.  The first argmax wins; a best value of ``-inf`` (no
    candidate had enough samples) raises.  ``entry``: ``kind`` ``"coarse"``, ``stride``, ``n_candidates``, ``values``,
    ``accepted`` (the index taken), ``best``."""
    cf, cm, c = (np.asarray(x, dtype=np.float64).reshape(3) for x in (centre_fixed, centre_moving, c))
    grid = np.asarray(grid, dtype=np.float64)
    if grid.ndim != 2 or grid.shape[1] != 3 or not 1 <= len(grid) <= MAX_GRID or not np.isfinite(grid).all():
        raise ValueError(f"the grid is 1..{MAX_GRID} finite angle triples, got shape {grid.shape}")
    ps = np.array([np.concatenate([cm - (rotation_np(*r) @ (cf - c) + c), r]) for r in grid])
    vals = np.asarray(cost_batch_many(ps.copy(), stride), dtype=np.float64).reshape(len(ps))
    j = int(np.argmax(vals))                                          # the first of equal maxima
    best = float(vals[j])
    if best == float("-inf"):
        raise ValueError(f"none of the {len(ps)} coarse candidates at stride {stride} had enough samples inside the moving volume")
    entry = {"kind": "coarse", "stride": stride, "n_candidates": len(ps), "values": tuple(float(v) for v in vals), "accepted": j,
             "best": best}
    return _check_p(ps[j]), best, entry


def global_levels(fixed_affine, init_step):
    """The levels after a coarse start: ``default_levels`` with the first level's rotation step at half the grid's."""
    v = voxel_size(fixed_affine)
    return [(4, (2 * v,) * 3 + (float(init_step) / 2,) * 3, 0.5 * v), (2, (0.5 * v,) * 3 + (0.5,) * 3, v / 16)]


def _prepare(fixed_shape, fixed_affine, moving_affine, bins, levels, p0, init="header", init_limit=40.0, init_step=20.0):
    """-> (A_fix, A_mov, levels, p0, centre, grid): ``grid`` the rotations of ``init="global"``, else None."""
    if bins not in BINS:
        raise ValueError(f"bins must be one of {BINS}, got {bins}")
    if init not in ("header", "global"):
        raise ValueError(f"init must be 'header' or 'global', got {init!r}")
    fa, ma = check_affine(fixed_affine, "fixed_affine"), check_affine(moving_affine, "moving_affine")
    grid = None
    if init == "global":
        if p0 is not None:
            raise ValueError("init='global' finds its own start: p0 goes with init='header'")
        grid = rotation_grid(init_limit, init_step)
        levels = global_levels(fa, init_step) if levels is None else list(levels)
    levels = default_levels(fa) if levels is None else list(levels)
    levels = [(effective_stride(fixed_shape, int(s)), step, min_t) for s, step, min_t in levels]
    p0 = np.zeros(6) if p0 is None else _check_p(p0)
    return fa, ma, levels, p0, volume_centre(fa, fixed_shape), grid


def _result(search, fa, ma, centre, coarse=None) -> RigidResult:
    p, value, n_eval, trace = search
    if coarse is not None:
        n_eval, trace = n_eval + coarse["n_candidates"], [coarse] + trace
    return RigidResult(p, rigid_world(p, centre), candidate_matrix(p, fa, ma, centre), value, n_eval, trace)


def register_rigid_np(fixed, fixed_affine, moving, moving_affine, bins=64, levels=None, p0=None, fixed_mask=None, moving_mask=None,
                      mask_cost=False, init="header", init_limit=40.0, init_step=20.0) -> RigidResult:
    """The specification of ``register_rigid``: ``compass_search`` over ``nmi_np(joint_histogram_np(...))``.  The ranges are the
    (NaN-ignoring) minimum and maximum of each volume; ``min_count`` is a quarter of the level's sample count; ``levels``
    defaults to ``default_levels(fixed_affine)``, every stride through ``effective_stride``.

    ``init="global"``: the search starts from ``coarse_start`` - the centres of mass of the two masks (a missing one is
    ``volume_eval.foreground_mask_np`` of its volume: Otsu, no closing), the rotations ``rotation_grid(init_limit, init_step)``,
    all scored at ``effective_stride(shape, 4)`` - and ``levels`` defaults to ``global_levels(fixed_affine, init_step)``; the
    trace begins with the ``coarse`` entry and ``n_evaluations`` includes the grid.  ``mask_cost=True``: every evaluation counts
    only the samples inside ``fixed_mask`` (computed as above when missing) and ``min_count`` is a quarter of
    ``count_nonzero(fixed_mask[::s, ::s, ::s])``.  The moving mask serves only its centre of mass."""
    from .volume_eval import foreground_mask_np
    fixed, moving = np.asarray(fixed), np.asarray(moving)
    fa, ma, levels, p0, centre, grid = _prepare(fixed.shape, fixed_affine, moving_affine, bins, levels, p0, init, init_limit, init_step)
    franges = (float(np.nanmin(fixed)), float(np.nanmax(fixed)))
    mranges = (float(np.nanmin(moving)), float(np.nanmax(moving)))
    if fixed_mask is None and (mask_cost or grid is not None):
        fixed_mask = foreground_mask_np(fixed)
    if fixed_mask is not None:
        fixed_mask = u8_np(fixed_mask, fixed.shape, "fixed_mask")
    cost_mask = fixed_mask if mask_cost else None

    def min_count(stride):
        if cost_mask is None:
            return sample_count(fixed.shape, stride) // 4
        return int(np.count_nonzero(cost_mask[::stride, ::stride, ::stride])) // 4

    def cost_batch(ps, stride):
        return [nmi_np(joint_histogram_np(fixed, moving, candidate_matrix(p, fa, ma, centre), bins, stride, franges, mranges, cost_mask),
                       min_count(stride))[0] for p in ps]
    coarse = None
    if grid is not None:
        moving_mask = foreground_mask_np(moving) if moving_mask is None else u8_np(moving_mask, moving.shape, "moving_mask")
        cf, cm = mask_centre_world(mask_moments_np(fixed_mask), fa), mask_centre_world(mask_moments_np(moving_mask), ma)
        p0, _, coarse = coarse_start(cost_batch, cf, cm, centre, grid, effective_stride(fixed.shape, COARSE_STRIDE))
    return _result(compass_search(cost_batch, p0, levels), fa, ma, centre, coarse)


# ---------------------------------------------------------------- device

def _matrices_arg(ms):
    ms = np.asarray(ms, dtype=np.float64)
    if ms.ndim == 2:
        ms = ms[None]
    if ms.ndim != 3 or ms.shape[1:] != (3, 4) or not 1 <= ms.shape[0] <= MAX_CANDIDATES or not np.isfinite(ms).all():
        raise ValueError(f"1..{MAX_CANDIDATES} finite (3, 4) matrices are expected, got shape {ms.shape}")
    return ms.shape[0], (L.C.c_double * (12 * ms.shape[0]))(*ms.reshape(-1).tolist())


def _check_tensor(t, what):
    return cuda_tensor(t, (torch.float32,), what, ndim=3, limit=True)


def _check_mask_tensor(mask, shape, what):
    """uint8 alone (no bool); two steps, so that the extent limit is checked before the shape, as it always was."""
    m = cuda_tensor(mask, (torch.uint8,), what, name="the mask", ndim=3, limit=True)
    return m if shape is None else cuda_tensor(m, (torch.uint8,), what, name="the mask", shape=shape)


def joint_histogram(fixed: torch.Tensor, moving: torch.Tensor, ms, bins, stride, fixed_range, moving_range, fixed_mask=None,
                    out=None) -> torch.Tensor:
    """fixed, moving: contiguous (X,Y,Z) float32 CUDA tensors; ms: (K, 3, 4) or (3, 4), K <= 16 (host, float64) -> the int64 CUDA
    tensor (K, bins, bins), equal to ``joint_histogram_np`` of every matrix.  ``fixed_mask``: a contiguous uint8 CUDA tensor of the
    fixed shape (the masked entry; ``None``: the unmasked one).  ``out``: such a tensor to overwrite.  A memset and one launch, no
    host synchronisation."""
    f, mv = _check_tensor(fixed, "joint_histogram"), _check_tensor(moving, "joint_histogram")
    _check_bins_stride(bins, stride)
    _check_range(fixed_range, bins, "fixed_range")
    _check_range(moving_range, bins, "moving_range")
    k, arg = _matrices_arg(ms)
    if out is None:
        out = torch.empty((k, bins, bins), dtype=torch.int64, device=f.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == (k, bins, bins)
              and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous int64 CUDA tensor of shape {(k, bins, bins)}")
    tail = (arg, k, int(stride), int(bins), float(fixed_range[0]), float(fixed_range[1]), float(moving_range[0]), float(moving_range[1]),
            out.data_ptr(), L.stream_ptr())
    if fixed_mask is None:
        L.call("mrisr_f32_volume_joint_histogram", f.data_ptr(), *f.shape, mv.data_ptr(), *mv.shape, *tail)
    else:
        fm = _check_mask_tensor(fixed_mask, f.shape, "joint_histogram")
        L.call("mrisr_f32_volume_joint_histogram_masked", f.data_ptr(), *f.shape, fm.data_ptr(), mv.data_ptr(), *mv.shape, *tail)
    return out


def nmi(hist: torch.Tensor, min_count=0):
    """hist: contiguous int64 CUDA tensor (K, bins, bins) or (bins, bins) -> (values float64 (K,), counts int64 (K,)), CUDA tensors,
    by ``nmi_np``'s rules.  One launch, no host synchronisation."""
    if not isinstance(hist, torch.Tensor) or not hist.is_cuda:
        raise ValueError(f"nmi {NO_CPU}: expected a CUDA tensor")
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


def mask_moments(mask: torch.Tensor) -> torch.Tensor:
    """mask: contiguous (X,Y,Z) uint8 CUDA tensor -> the int64 CUDA tensor (4,) ``(N, sum i, sum j, sum k)`` over its non-zero
    voxels, equal to ``mask_moments_np``.  A memset and one launch, no host synchronisation."""
    m = _check_mask_tensor(mask, None, "mask_moments")
    out = torch.empty(4, dtype=torch.int64, device=m.device)
    L.call("mrisr_u8_volume_mask_moments", m.data_ptr(), *m.shape, out.data_ptr(), L.stream_ptr())
    return out


def volume_range(v: torch.Tensor):
    """(lo, hi) host floats of a CUDA volume, NaN ignored: one read (not on the hot path)."""
    finite = torch.where(torch.isnan(v), v.new_tensor(float("inf")), v).amin(), torch.where(torch.isnan(v), v.new_tensor(float("-inf")), v).amax()
    lo, hi = torch.stack(finite).cpu().tolist()
    return lo, hi


def register_rigid(fixed: torch.Tensor, fixed_affine, moving: torch.Tensor, moving_affine, bins=64, levels=None, p0=None, fixed_mask=None,
                   moving_mask=None, mask_cost=False, init="header", init_limit=40.0, init_step=20.0) -> RigidResult:
    """The device path of ``register_rigid_np``: the same ``compass_search`` over a ``cost_batch`` that launches
    ``joint_histogram`` and ``nmi`` for the K candidates and reads their K values back - ONE device-to-host read per search
    iteration (``trace[i]["host_reads"] == 1``).  The ranges of the two volumes are read once per registration.

    ``init="global"`` (``register_rigid_np``): missing masks are ``volume_eval.foreground_mask`` of their volumes; the 8 moments of
    the two masks are read at once; the grid's candidates go out in chunks of 16 (``joint_histogram`` + ``nmi`` each) into one
    values tensor that is read once - the ``coarse`` entry of the trace has ``host_reads == 1`` too.  ``mask_cost=True``: the masked
    histogram entry everywhere; the masked sample counts behind ``min_count`` are read once, before the search."""
    from .volume_eval import foreground_mask
    f, mv = _check_tensor(fixed, "register_rigid"), _check_tensor(moving, "register_rigid")
    fa, ma, levels, p0, centre, grid = _prepare(f.shape, fixed_affine, moving_affine, bins, levels, p0, init, init_limit, init_step)
    franges, mranges = volume_range(f), volume_range(mv)
    if fixed_mask is None and (mask_cost or grid is not None):
        fixed_mask = foreground_mask(f)[0]
    if fixed_mask is not None:
        fixed_mask = _check_mask_tensor(fixed_mask, f.shape, "register_rigid")
    cost_mask = fixed_mask if mask_cost else None
    coarse_stride = effective_stride(f.shape, COARSE_STRIDE)
    strides = sorted({s for s, _, _ in levels} | ({coarse_stride} if grid is not None else set()))
    if cost_mask is None:
        min_counts = {s: sample_count(f.shape, s) // 4 for s in strides}
    else:                                                            # one read for all the distinct strides, before the loop
        counted = torch.stack([torch.count_nonzero(cost_mask[::s, ::s, ::s]) for s in strides]).cpu().tolist()
        min_counts = {s: int(n) // 4 for s, n in zip(strides, counted)}
    hist = torch.empty((MAX_CANDIDATES, bins, bins), dtype=torch.int64, device=f.device)
    reads = []

    def launch(ps, stride):
        ms = np.stack([candidate_matrix(p, fa, ma, centre) for p in ps])
        return nmi(joint_histogram(f, mv, ms, bins, stride, franges, mranges, fixed_mask=cost_mask, out=hist[:len(ps)]), min_counts[stride])[0]

    def cost_batch(ps, stride):
        host = launch(ps, stride).cpu().numpy()                      # the one synchronisation of this iteration
        reads.append(1)
        return host

    def cost_batch_many(ps, stride):
        values = torch.empty(len(ps), dtype=torch.float64, device=f.device)
        for at in range(0, len(ps), MAX_CANDIDATES):                 # nmi has read hist before the next chunk's memset: one stream
            values[at:at + MAX_CANDIDATES] = launch(ps[at:at + MAX_CANDIDATES], stride)
        host = values.cpu().numpy()                                  # the one synchronisation of the coarse stage
        reads.append(1)
        return host
    coarse = None
    if grid is not None:
        moving_mask = foreground_mask(mv)[0] if moving_mask is None else _check_mask_tensor(moving_mask, mv.shape, "register_rigid")
        moments = torch.stack([mask_moments(fixed_mask), mask_moments(moving_mask)]).cpu().numpy()      # one read of the 8 integers
        cf, cm = mask_centre_world(moments[0], fa), mask_centre_world(moments[1], ma)
        p0, _, coarse = coarse_start(cost_batch_many, cf, cm, centre, grid, coarse_stride)
    result = _result(compass_search(cost_batch, p0, levels), fa, ma, centre, coarse)
    assert len(result.trace) == len(reads)
    for entry, n in zip(result.trace, reads):
        entry["host_reads"] = n
    return result
