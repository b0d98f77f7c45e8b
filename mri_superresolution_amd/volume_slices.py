"""Slice-to-volume motion correction of the reconstruction from orthogonal stacks (``volume_stacks.py``; extension, DESIGN.md section
7): everything with a pose per slice.  A 2-D multi-slice stack is acquired slice by slice and the head moves in between, so every
slice gets a rigid pose of its own; ``motion=MotionOptions(...)`` of ``volume_stacks.combine_stacks_np`` / ``combine_stacks`` (default
off) registers the slices of every stack to the current estimate and rebuilds the estimate, in rounds.

``slice_geometries``   the two matrices of ``stack_geometry`` per slice, from (S, 6) poses about the slices' centres (S <= 256).
``stack_residual_slices_np``, ``simulate_stack_slices_np``, ``stack_update_slices_np``   the two projections with a matrix per slice; the
                      update weights the slices near a voxel by ``1 - |z - s|``, leaves gaps uncovered and normalises overlaps.
``slice_cost_np``, ``ncc_from_sums``, ``slice_compass_search``, ``register_slices_np``   the cost of up to 13 candidate poses of every
                      slice (six float64 sums each), its NCC, and the compass search of ``volume_register`` for all slices at once.
``stack_residual_slices``, ``stack_update_slices``, ``slice_cost``, ``register_slices``   the device path (``csrc/volume_slices.hip``): the
                      projections bit for bit; the sums within 1e-12 and the same bits on every run; one device-to-host read per
                      search iteration.  Measured quality and speed: README, DESIGN.md section 7.

The forward model, the step of an update, the reconstruction loops (``_reconstruct_np``, ``_reconstruct``, ``_iterate``) and the
checks are those of ``volume_stacks``, which this module imports; ``volume_stacks`` imports this one inside its functions alone.
What is not built is listed there.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from ._volume_args import check_shape, cuda_tensor, out_like
from .utils.nifti import check_affine, grid_matrix
from .volume_reslice import taps_np, weighted_sum_np
from .volume_stacks import (StackGeometry, _check_clamp, _check_geometry, _check_pair, _check_same_count, _check_slice_axis,
                            _check_stack_count, _check_stacks, _check_step, _check_tensor, _check_volume_np, _coordinate_np, _index_axes,
                            _matrix_rows, _profile_args, _project_rows_np, _reconstruct, _reconstruct_np, _residual_np,
                            _simulated_np, _slots, _step_args, _step_np, _table_rows, _update_bytes, voxel_sizes)

MAX_SLICES = 256                 # per-slice poses: the slices of one stack
MAX_CANDIDATES = 13              # poses of a slice scored in one launch: a point and its 12 compass neighbours
COST_STRIDES = (1, 2, 4)


# ---------------------------------------------------------------- geometry and specification

def _in_plane(axis):
    return tuple(a for a in range(3) if a != axis)


def _check_table(table, slices, what) -> np.ndarray:
    t = np.asarray(table, dtype=np.float64)
    if t.shape != (slices, 3, 4) or not np.isfinite(t).all():
        raise ValueError(f"{what}: the per-slice matrices must be ({slices}, 3, 4) and finite, got shape {t.shape}")
    return np.ascontiguousarray(t)


def _check_slice_count(slices, what) -> int:
    if not 1 <= slices <= MAX_SLICES:
        raise ValueError(f"{what}: per-slice poses take stacks of 1..{MAX_SLICES} slices, got {slices}")
    return int(slices)


def slice_centres(affine, stack_shape, slice_axis) -> np.ndarray:
    """(S, 3) float64: the world position of the centre of every slice - index ``(n - 1) / 2`` in the plane, ``s`` along the axis."""
    a, shape = check_affine(affine, "affine"), check_shape(stack_shape, "stack_shape")
    idx = np.tile((np.asarray(shape, dtype=np.float64) - 1.0) / 2.0, (shape[slice_axis], 1))
    idx[:, slice_axis] = np.arange(shape[slice_axis], dtype=np.float64)
    return idx @ a[:3, :3].T + a[:3, 3]


def slice_geometries(affine, affine_out, stack_shape, slice_axis, params, world=None):
    """-> ``(to_output, from_output)``, both (S, 3, 4) float64: ``stack_geometry``'s two matrices with a rigid pose per slice.
    ``params`` (S, 6): ``(tx, ty, tz, rx, ry, rz)`` of slice ``s`` in mm and degrees; ``W_s = volume_register.rigid_world(params[s],
    centre_s)`` about the world position of the slice's centre is folded as ``stack_geometry`` folds ``world``:
    ``out_s = W_s @ world @ affine_out``, ``M_s = grid_matrix(out_s, affine)``, ``N_s = grid_matrix(affine, out_s)``.  ``params = 0``
    gives the stack's own matrices to the last bit, S times.  More than 256 slices: ``ValueError``."""
    from .volume_register import rigid_world
    a, out = check_affine(affine, "affine"), check_affine(affine_out, "affine_out")
    shape = check_shape(stack_shape, "stack_shape")
    S = _check_slice_count(shape[_check_slice_axis(slice_axis)], "slice_geometries")
    params = np.asarray(params, dtype=np.float64)
    if params.shape != (S, 6) or not np.isfinite(params).all():
        raise ValueError(f"slice_geometries: the parameters are ({S}, 6) and finite, got shape {params.shape}")
    if world is not None:
        out = check_affine(world, "world") @ out
    centres = slice_centres(a, shape, int(slice_axis))
    to_output, from_output = np.empty((S, 3, 4)), np.empty((S, 3, 4))
    for s in range(S):
        out_s = rigid_world(params[s], centres[s]) @ out
        to_output[s], from_output[s] = grid_matrix(out_s, a), grid_matrix(a, out_s)
    return to_output, from_output


def _slice_rows(g, shape, to_output_s, what):
    """The rows the voxels of a stack of ``shape`` project through: those of ``to_output_s[s]`` (S, 3, 4, checked) in slice ``s``."""
    table = _check_table(to_output_s, _check_slice_count(shape[g.slice_axis], what), what)
    grid = [1, 1, 1]
    grid[g.slice_axis] = shape[g.slice_axis]
    return _table_rows(table, grid)


def simulate_stack_slices_np(x, geometry: StackGeometry, stack_shape, to_output_s, fill: float = 0.0) -> np.ndarray:
    """``simulate_stack_np`` with the voxels of slice ``s`` going through ``to_output_s[s]`` (S, 3, 4) in place of ``M``."""
    x, g = _check_volume_np(x, "simulate_stack_slices_np"), _check_geometry(geometry, "simulate_stack_slices_np")
    shape = check_shape(stack_shape, "stack_shape")
    rows = _slice_rows(g, shape, to_output_s, "simulate_stack_slices_np")
    return _simulated_np(*_project_rows_np(x, g, rows, _index_axes(shape), shape), fill)[0]


def stack_residual_slices_np(x, y, geometry: StackGeometry, to_output_s):
    """``stack_residual_np`` -> ``(r, (S, n))`` with the voxels of slice ``s`` using ``to_output_s[s]`` (S, 3, 4) in place of ``M``:
    the same operations voxel by voxel, so equal tables reproduce ``stack_residual_np`` bit for bit."""
    x, y = _check_volume_np(x, "stack_residual_slices_np"), _check_volume_np(y, "stack_residual_slices_np")
    g = _check_geometry(geometry, "stack_residual_slices_np")
    return _residual_np(x, y, g, _slice_rows(g, y.shape, to_output_s, "stack_residual_slices_np"))


def _not_built_with_motion(reg_lambda, what):
    if float(reg_lambda) != 0.0:
        raise NotImplementedError(f"{what}: the regulariser (reg_lambda > 0) together with per-slice poses is not built")


def stack_update_slices_np(x, residuals, geometries, from_output_s, step: float = 1.0, clamp=0.0, reg_lambda: float = 0.0):
    """-> ``(x', cnt)``: ``stack_update_np`` with a pose per slice.  ``from_output_s[k]`` (S_k, 3, 4): ``N_{k,s}``.  For every output
    voxel ``q`` and stack ``k`` ascending, from ``acc = +0``, ``wk = +0`` (float32) and for ``s = 0 .. S_k - 1`` ascending:
    ``p = N_{k,s} q`` (the coordinate rule of ``stack_residual_np``); ``z = p[slice_axis]``, ``d = |z - s|`` in float64; the slice is
    skipped unless ``d < 1`` and both in-plane coordinates lie in ``[-0.5, n - 0.5]``; else ``w = float32(1 - d)`` (the difference in
    float64), ``g`` = the bilinear gather of slice ``s`` of the residual at the two in-plane coordinates (``taps_np(..., "linear")``,
    ``weighted_sum_np``, the higher in-plane axis reduced first), ``acc = acc + w g``, ``wk = wk + w``.  The stack covers the voxel
    when ``wk >= 0.5``: ``sum = sum + acc / wk``, ``cnt += 1``.  The step, the clamp and the uncovered voxels: ``stack_update_np``.

    With equal matrices this is ``stack_update_np`` up to rounding: ``wk`` sums to 1 between two slices, the border slice alone is
    replicated, and ``wk < 0.5`` is the inside test along the slice axis.  With motion, gaps between slices stay uncovered and
    overlapping slices are normalised.  ``reg_lambda > 0`` is not built here: ``NotImplementedError``."""
    _not_built_with_motion(reg_lambda, "stack_update_slices_np")
    x = _check_volume_np(x, "stack_update_slices_np")
    residuals, geometries, tables = list(residuals), list(geometries), list(from_output_s)
    _check_stack_count(len(residuals), "stack_update_slices_np")
    if len(geometries) != len(residuals) or len(tables) != len(residuals):
        raise ValueError(f"stack_update_slices_np: {len(residuals)} stacks, {len(geometries)} geometries and {len(tables)} tables")
    step, lo = _check_step(step), _check_clamp(clamp)
    q = _index_axes(x.shape)
    total, cnt = np.zeros(x.shape, dtype=np.float32), np.zeros(x.shape, dtype=np.uint8)
    with np.errstate(all="ignore"):
        for k, (r, g, table) in enumerate(zip(residuals, geometries, tables)):
            what = f"stack_update_slices_np: stack {k}"
            r, g = _check_volume_np(r, what), _check_geometry(g, what)
            axis, (a, b) = g.slice_axis, _in_plane(g.slice_axis)
            table = _check_table(table, _check_slice_count(r.shape[axis], what), what)
            acc, wk = np.zeros(x.shape, dtype=np.float32), np.zeros(x.shape, dtype=np.float32)
            for s in range(r.shape[axis]):
                rows = _matrix_rows(table[s])
                d = np.abs(np.broadcast_to(_coordinate_np(rows[axis], q), x.shape) - float(s))
                ok = d < 1.0
                if not ok.any():
                    continue
                pa, pb = (np.broadcast_to(_coordinate_np(rows[c], q), x.shape) for c in (a, b))
                ok = ok & (pa >= -0.5) & (pa <= r.shape[a] - 0.5) & (pb >= -0.5) & (pb <= r.shape[b] - 0.5)
                if not ok.any():
                    continue
                w = (1.0 - d[ok]).astype(np.float32)
                (ia, wa), (ib, wb) = taps_np(pa[ok], r.shape[a], "linear"), taps_np(pb[ok], r.shape[b], "linear")
                plane = np.take(r, s, axis=axis)
                val = weighted_sum_np(wa, [weighted_sum_np(wb, [plane[u, v] for v in ib]) for u in ia])
                acc[ok] = acc[ok] + w * val
                wk[ok] = wk[ok] + w
            hit = wk >= np.float32(0.5)
            total[hit] = total[hit] + acc[hit] / wk[hit]
            cnt[hit] += 1
    return _step_np(x, total, cnt, step, lo), cnt


def _check_cost_args(shape, axis, cand_to_output, stride, what):
    S = _check_slice_count(shape[axis], what)
    cand = np.asarray(cand_to_output, dtype=np.float64)
    if cand.ndim != 4 or cand.shape[0] != S or not 1 <= cand.shape[1] <= MAX_CANDIDATES or cand.shape[2:] != (3, 4) \
            or not np.isfinite(cand).all():
        raise ValueError(f"{what}: the candidates are ({S}, 1..{MAX_CANDIDATES}, 3, 4) and finite, got shape {cand.shape}")
    if stride not in COST_STRIDES:
        raise ValueError(f"{what}: stride must be one of {COST_STRIDES}, got {stride!r}")
    return np.ascontiguousarray(cand), int(stride)


def strided_slice_count(shape, slice_axis, stride) -> int:
    """The voxels of one slice whose two in-plane indices are multiples of ``stride``."""
    a, b = _in_plane(slice_axis)
    return -(-int(shape[a]) // stride) * -(-int(shape[b]) // stride)


def slice_cost_np(x, y, geometry: StackGeometry, cand_to_output, stride: int = 1) -> np.ndarray:
    """-> (S, C, 6) float64.  For slice ``s`` and candidate ``c`` (``C <= 13``): over the voxels of the slice whose two in-plane indices
    are multiples of ``stride`` (1, 2 or 4), simulated as ``m = acc / wsum`` through ``cand_to_output[s, c]`` with the profile
    (``stack_residual_np``'s forward model) and kept where ``wsum >= 0.5``: ``n, sum y, sum m, sum y^2, sum m^2, sum y m`` - the
    products formed in float64 (exact), the sums correctly rounded (``math.fsum``)."""
    x, y = _check_volume_np(x, "slice_cost_np"), _check_volume_np(y, "slice_cost_np")
    g = _check_geometry(geometry, "slice_cost_np")
    cand, stride = _check_cost_args(y.shape, g.slice_axis, cand_to_output, stride, "slice_cost_np")
    S, C = cand.shape[:2]
    a, b = _in_plane(g.slice_axis)
    ia, ib = np.arange(0, y.shape[a], stride), np.arange(0, y.shape[b], stride)
    shape = (S, C, ia.size, ib.size)
    q = [None, None, None]
    q[g.slice_axis] = np.arange(S, dtype=np.float64).reshape(S, 1, 1, 1)
    q[a], q[b] = ia.astype(np.float64).reshape(1, 1, -1, 1), ib.astype(np.float64).reshape(1, 1, 1, -1)
    acc, wsum = _project_rows_np(x, g, _table_rows(cand, (S, C, 1, 1)), q, shape)
    m, ok = _simulated_np(acc, wsum)
    m = m.astype(np.float64)
    ys = np.moveaxis(y, g.slice_axis, 0)[:, ::stride, ::stride].astype(np.float64)      # (S, rows, cols), the lower in-plane axis first
    out = np.zeros((S, C, 6))
    for s in range(S):
        for c in range(C):
            keep = ok[s, c]
            yv, mv = ys[s][keep], m[s, c][keep]
            out[s, c] = (yv.size, math.fsum(yv), math.fsum(mv), math.fsum(yv * yv), math.fsum(mv * mv), math.fsum(yv * mv))
    return out


def ncc_from_sums(sums, min_count=1) -> np.ndarray:
    """The normalised cross-correlation of ``y`` and ``m`` from ``(..., 6)`` sums ``n, sum y, sum m, sum y^2, sum m^2, sum y m``, in
    float64: ``cov / sqrt(var_y var_m)`` with ``var_y = sum y^2 - (sum y)^2 / n`` and so on; ``-inf`` where ``n < min_count`` (an
    array broadcasts), ``n < 1`` or a variance is not positive.  The specification path and the device path share it."""
    sums = np.asarray(sums, dtype=np.float64)
    n, sy, sm, syy, smm, sym = (sums[..., e] for e in range(6))
    with np.errstate(all="ignore"):
        nn = np.maximum(n, 1.0)
        vy, vm, cov = syy - sy * sy / nn, smm - sm * sm / nn, sym - sy * sm / nn
        ok = (n >= min_count) & (n >= 1) & (vy > 0) & (vm > 0)
        return np.where(ok, cov / np.sqrt(np.where(ok, vy * vm, 1.0)), -np.inf)


def slice_compass_search(cost_batch, p0, levels, limits, active=None, max_iterations=1000):
    """``volume_register.compass_search`` for all the slices of a stack at once -> ``(params (S, 6), best (S,), start (S,), trace)``.
    Every slice has its own point, step vector and best value; ONE ``cost_batch(cands (S, C, 6), stride) -> (S, C)`` call per
    iteration covers them all.  A level is ``(stride, step[6], min_translation_step)``.  At each level every slice's point is scored
    (``C = 1``; ``start`` is that of the first level); then, while a live slice is left, the 12 candidates ``p +- step[a] e_a`` of
    every slice - axis ascending, ``+`` before ``-`` - are scored in one call; a candidate beyond ``limits = (mm, deg)`` in any
    component scores ``-inf``; a slice moves to its first argmax only if that is strictly greater than its best, otherwise its six
    steps halve.  A slice is live while it is active and its translation step is at least the level's stop; the others resubmit
    their point 12 times and ignore the values.  Inactive slices (``active`` (S,) bool, None: all active) keep ``p0``.  ``trace``:
    one dict per call - ``level``, ``stride``, ``kind``, ``p``, ``step``, ``values``, ``accepted`` (per slice, -1: none), ``best``."""
    p = np.array(p0, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 6 or not np.isfinite(p).all():
        raise ValueError(f"slice_compass_search: the start is (S, 6) and finite, got shape {p.shape}")
    S = p.shape[0]
    active = np.ones(S, dtype=bool) if active is None else np.asarray(active, dtype=bool).reshape(S).copy()
    lim = np.array([float(limits[0])] * 3 + [float(limits[1])] * 3)
    if not (lim > 0).all():
        raise ValueError(f"slice_compass_search: the limits are two positive numbers (mm, degrees), got {limits!r}")
    best, start, trace, rows = np.full(S, -np.inf), None, [], np.arange(S)
    for li, (stride, step0, min_t) in enumerate(levels):
        step0 = np.asarray(step0, dtype=np.float64)
        if step0.shape != (6,) or not (step0 > 0).all() or not np.isfinite(step0).all() or not min_t > 0:
            raise ValueError(f"level {li}: six positive steps and a positive stop, got {step0.tolist()} and {min_t}")
        step = np.tile(step0, (S, 1))
        best = np.asarray(cost_batch(p[:, None, :].copy(), stride), dtype=np.float64).reshape(S).copy()
        start = best.copy() if start is None else start
        trace.append({"level": li, "stride": stride, "kind": "start", "p": p.copy(), "step": step.copy(), "values": best[:, None].copy(),
                      "accepted": np.full(S, -1), "best": best.copy()})
        for _ in range(max_iterations):
            live = active & (step[:, 0] >= min_t)
            if not live.any():
                break
            cands = np.repeat(p[:, None, :], 12, axis=1)
            for a in range(6):
                cands[live, 2 * a, a] += step[live, a]
                cands[live, 2 * a + 1, a] -= step[live, a]
            vals = np.asarray(cost_batch(cands.copy(), stride), dtype=np.float64).reshape(S, 12)
            vals = np.where((np.abs(cands) > lim).any(axis=2), -np.inf, vals)
            j = np.argmax(vals, axis=1)                                   # the first of equal maxima
            move = live & (vals[rows, j] > best)
            entry = {"level": li, "stride": stride, "kind": "probe", "p": p.copy(), "step": step.copy(), "values": vals,
                     "accepted": np.where(move, j, -1)}
            p[move], best[move] = cands[move, j[move]], vals[move, j[move]]
            step[live & ~move] /= 2
            entry["best"] = best.copy()
            trace.append(entry)
    return p, best, start, trace


def in_plane_voxel_size(affine, slice_axis) -> float:
    """The mean of the two in-plane voxel sizes of a stack, in mm."""
    return float(np.mean(voxel_sizes(affine)[list(_in_plane(slice_axis))]))


def default_slice_levels(affine, slice_axis):
    """``[(2, 2v x 3 + 2 deg x 3, v / 2), (1, v / 2 x 3 + 0.5 deg x 3, v / 8)]`` with ``v = in_plane_voxel_size``."""
    v = in_plane_voxel_size(affine, slice_axis)
    return [(2, (2 * v,) * 3 + (2.0,) * 3, 0.5 * v), (1, (0.5 * v,) * 3 + (0.5,) * 3, v / 8)]


def active_slices(sums, min_contrast) -> np.ndarray:
    """(S,) bool from the (S, 6) sums of the slices' current poses: a slice is active when the standard deviation of its ``y`` is at
    least ``min_contrast`` times that of the pooled stack (air and the crown of the head fall below) and positive."""
    sums = np.asarray(sums, dtype=np.float64)
    n, sy, syy = sums[:, 0], sums[:, 1], sums[:, 3]
    with np.errstate(all="ignore"):
        sd = np.sqrt(np.maximum(syy - sy * sy / np.maximum(n, 1.0), 0.0) / np.maximum(n, 1.0))
        N, SY, SYY = n.sum(), sy.sum(), syy.sum()
        pooled = math.sqrt(max(SYY - SY * SY / max(N, 1.0), 0.0) / max(N, 1.0))
    return (n > 0) & (sd > 0) & (sd >= float(min_contrast) * pooled)


def slice_corner_displacement(params_a, params_b, affine, stack_shape, slice_axis) -> np.ndarray:
    """(S,) float64: per slice, the largest distance in mm, over the four corner voxels of the slice, between their positions under
    the poses ``params_a[s]`` and ``params_b[s]`` (``rigid_world`` about the slice's centre)."""
    from .volume_register import rigid_world
    a, shape = check_affine(affine, "affine"), check_shape(stack_shape, "stack_shape")
    centres = slice_centres(a, shape, slice_axis)
    pa, pb = np.asarray(params_a, dtype=np.float64), np.asarray(params_b, dtype=np.float64)
    u, v = _in_plane(slice_axis)
    out = np.zeros(shape[slice_axis])
    for s in range(shape[slice_axis]):
        idx = np.zeros((4, 4))
        idx[:, 3], idx[:, slice_axis] = 1.0, s
        idx[:, u], idx[:, v] = [0, 0, shape[u] - 1, shape[u] - 1], [0, shape[v] - 1, 0, shape[v] - 1]
        world = a @ idx.T
        d = ((rigid_world(pa[s], centres[s]) - rigid_world(pb[s], centres[s])) @ world)[:3]
        out[s] = np.sqrt((d * d).sum(axis=0)).max()
    return out


class MotionOptions(NamedTuple):
    """What ``combine_stacks(_np)(..., motion=...)`` needs to move single slices: the grids - the geometries alone do not say where a
    slice's centre lies in the world - and the search's settings."""
    affines: tuple                   # per stack: index -> world (4, 4)
    affine_out: np.ndarray           # the output grid's index -> world
    worlds: tuple = None             # per stack: None or the (4, 4) ``world`` folded into its geometry
    rounds: int = 2
    limit_mm: float = 10.0
    limit_deg: float = 10.0
    min_contrast: float = 0.1
    levels: tuple = None             # per stack: the search levels; None: ``default_slice_levels``


class SliceMotion(NamedTuple):
    params: np.ndarray               # (S, 6) float64: tx, ty, tz (mm), rx, ry, rz (degrees) per slice
    active: np.ndarray               # (S,) bool: the slices that were searched
    start: np.ndarray                # (S,) float64: the cost (NCC) at the start, at the first level's stride
    end: np.ndarray                  # (S,) float64: the cost after the search, at the last level's stride
    trace: list


def _check_motion(motion, count, reg_lambda, what) -> MotionOptions:
    _not_built_with_motion(reg_lambda, what)
    if not isinstance(motion, MotionOptions):
        raise ValueError(f"{what}: motion is a MotionOptions, got {type(motion).__name__}")
    affines = tuple(check_affine(a, "affine") for a in motion.affines)
    worlds = (None,) * count if motion.worlds is None else tuple(motion.worlds)
    levels = (None,) * count if motion.levels is None else tuple(motion.levels)
    if len(affines) != count or len(worlds) != count or len(levels) != count:
        raise ValueError(f"{what}: motion needs one affine (and world, and list of levels) per stack ({count})")
    if isinstance(motion.rounds, bool) or not isinstance(motion.rounds, (int, np.integer)) or motion.rounds < 0:
        raise ValueError(f"{what}: motion rounds is an integer that is not negative, got {motion.rounds!r}")
    if not (motion.limit_mm > 0 and motion.limit_deg > 0 and 0 <= motion.min_contrast < np.inf):
        raise ValueError(f"{what}: the motion limits must be positive and min_contrast not negative")
    return motion._replace(affines=affines, affine_out=check_affine(motion.affine_out, "affine_out"), worlds=worlds, levels=levels)


def _register_slices(sums_of, shape, axis, affine, affine_out, world, params0, levels, limits, min_contrast) -> SliceMotion:
    """The search of ``register_slices_np`` / ``register_slices``: ``sums_of(cand_to_output (S, C, 3, 4), stride) -> (S, C, 6)``."""
    S = _check_slice_count(shape[axis], "register_slices")
    p0 = np.zeros((S, 6)) if params0 is None else np.array(params0, dtype=np.float64)
    levels = default_slice_levels(affine, axis) if levels is None else list(levels)

    def sums(cands, stride):
        tables = [slice_geometries(affine, affine_out, shape, axis, cands[:, c], world)[0] for c in range(cands.shape[1])]
        return sums_of(np.stack(tables, axis=1), stride)

    active = active_slices(sums(p0[:, None, :], levels[0][0])[:, 0], min_contrast)

    def cost_batch(cands, stride):
        return ncc_from_sums(sums(cands, stride), 0.25 * strided_slice_count(shape, axis, stride))

    params, best, start, trace = slice_compass_search(cost_batch, p0, levels, limits, active)
    return SliceMotion(params, active, start, best, trace)


def register_slices_np(x, y, geometry: StackGeometry, affine, affine_out, params0=None, world=None, levels=None, limits=(10.0, 10.0),
                       min_contrast: float = 0.1) -> SliceMotion:
    """The specification of ``register_slices``: the pose of every slice of the stack ``y`` against the estimate ``x``.  The current
    poses (``params0``, None: zeros) are scored first (``slice_cost_np`` at the first level's stride); ``active_slices`` of those sums
    picks the slices to search; ``slice_compass_search`` maximises ``ncc_from_sums(slice_cost_np(...), min_count)`` over the poses,
    ``min_count`` a quarter of a slice's strided voxel count, the candidates turned into matrices by ``slice_geometries``."""
    x, y = _check_volume_np(x, "register_slices_np"), _check_volume_np(y, "register_slices_np")
    g = _check_geometry(geometry, "register_slices_np")
    return _register_slices(lambda cand, stride: slice_cost_np(x, y, g, cand, stride), y.shape, g.slice_axis, affine, affine_out, world,
                            params0, levels, limits, min_contrast)


def _motion_rounds(motion, stacks_shapes, geometries, register, rebuild):
    """The rounds of ``combine_stacks(_np)`` with motion.  ``register(k, params_k, levels_k) -> SliceMotion`` against the current
    estimate; ``rebuild(to_output_s, from_output_s)`` makes the estimate from scratch.  -> ``(params per stack, motion_cost, last)``:
    ``motion_cost[round][k] = (mean cost of the active slices at the start, at the end)``; ``last``: the final round's SliceMotion."""
    K = len(geometries)
    params = [np.zeros((shape[g.slice_axis], 6)) for shape, g in zip(stacks_shapes, geometries)]
    costs, last = [], [None] * K
    for _ in range(motion.rounds):
        row = []
        for k in range(K):
            last[k] = register(k, params[k], motion.levels[k])
            act = last[k].active
            finite = act & np.isfinite(last[k].start) & np.isfinite(last[k].end)
            row.append((float(last[k].start[finite].mean()) if finite.any() else float("nan"),
                        float(last[k].end[finite].mean()) if finite.any() else float("nan")))
        params = [m.params for m in last]
        costs.append(row)
        tables = [slice_geometries(motion.affines[k], motion.affine_out, stacks_shapes[k], geometries[k].slice_axis, params[k], motion.worlds[k])
                  for k in range(K)]
        rebuild([t[0] for t in tables], [t[1] for t in tables])
    return params, np.asarray(costs, dtype=np.float64).reshape(motion.rounds, K, 2), last


def _slice_steps_np(stacks, geometries, to_output_s, from_output_s, step, clamp):
    """The two steps of ``volume_stacks._reconstruct_np`` with a pose per slice (``volume_stacks._steps_np``)."""
    def residual(x, k):
        return stack_residual_slices_np(x, stacks[k], geometries[k], to_output_s[k])

    def update(x, volumes, first):
        return stack_update_slices_np(x, volumes, geometries, from_output_s, 1.0 if first else step, clamp)

    return residual, update


def _motion_np(motion, state, stacks, geometries, shape_out, iterations, step, clamp, fill):
    """The motion rounds of ``combine_stacks_np``.  ``state``: the list ``_reconstruct_np`` returned, whose first entry is the current
    estimate; every rebuild replaces its entries.  -> ``(params per stack, motion_cost, last)``."""
    def register(k, params, levels):
        return register_slices_np(state[0], stacks[k], geometries[k], motion.affines[k], motion.affine_out, params, motion.worlds[k],
                                  levels, (motion.limit_mm, motion.limit_deg), motion.min_contrast)

    def rebuild(to_output_s, from_output_s):
        state[:] = _reconstruct_np(stacks, shape_out, iterations, fill, *_slice_steps_np(stacks, geometries, to_output_s, from_output_s, step, clamp))

    return _motion_rounds(motion, [y.shape for y in stacks], geometries, register, rebuild)


# ---------------------------------------------------------------- device

def _table_tensor(table, slices, device, what) -> torch.Tensor:
    """A (slices, 12) float64 table on ``device``: a numpy (slices, 3, 4) array is checked and uploaded, a tensor taken as given."""
    if isinstance(table, torch.Tensor):
        t = cuda_tensor(table, (torch.float64,), what, name="the table of per-slice matrices", shape=(slices, 12))
        if t.device != device:
            raise ValueError(f"{what}: the table of per-slice matrices must lie on {device}")
        return t
    return torch.from_numpy(_check_table(table, slices, what).reshape(slices, 12)).to(device)


def _residual_slices(x, y, g, table, r, slots_ptr, stats_row):
    L.call("mrisr_f32_volume_stack_residual_slices", x.data_ptr(), *x.shape, y.data_ptr(), *y.shape, table.data_ptr(), y.shape[g.slice_axis],
           g.slice_axis, *_profile_args(g), r.data_ptr(), slots_ptr, L.ptr(stats_row), L.stream_ptr(), nbytes=4 * (x.numel() + 2 * y.numel()))


def _update_slices(x, volumes, geometries, tables, step, lo, out, cover, slots, stats_rows):
    views = (L.StackSlicesView * len(volumes))()
    for view, v, g, t in zip(views, volumes, geometries, tables):
        view.data, (view.nx, view.ny, view.nz), view.slice_axis = v.data_ptr(), v.shape, g.slice_axis
        view.from_output, view.slices = t.data_ptr(), v.shape[g.slice_axis]
    L.call("mrisr_f32_volume_stack_update_slices", x.data_ptr(), *x.shape, views, len(volumes), *_step_args(step, lo), out.data_ptr(),
           L.ptr(cover), L.ptr(slots), L.ptr(stats_rows), L.stream_ptr(), nbytes=_update_bytes(x, volumes))


def stack_residual_slices(x: torch.Tensor, y: torch.Tensor, geometry: StackGeometry, to_output_s, out=None):
    """The device path of ``stack_residual_slices_np`` -> ``(r, S, n)`` as ``stack_residual``: ``r`` bit for bit.  ``to_output_s``: a
    numpy (S, 3, 4) array (uploaded) or a float64 CUDA tensor (S, 12).  CPU tensors raise."""
    x, y = _check_pair(x, y, "stack_residual_slices")
    g = _check_geometry(geometry, "stack_residual_slices")
    table = _table_tensor(to_output_s, _check_slice_count(y.shape[g.slice_axis], "stack_residual_slices"), x.device, "stack_residual_slices")
    r = out_like(out, y, (x, y), "stack_residual_slices")
    row = torch.empty(2, dtype=torch.int64, device=x.device)
    _residual_slices(x, y, g, table, r, _slots(x.device, 1).data_ptr(), row)
    return r, row[:1].view(torch.float64)[0], row[1]


def stack_update_slices(x: torch.Tensor, residuals, geometries, from_output_s, step: float = 1.0, clamp=0.0, out=None, cover: bool = False,
                        reg_lambda: float = 0.0):
    """The device path of ``stack_update_slices_np`` -> ``(x', cnt)``, bit for bit; ``cnt`` (uint8) only with ``cover=True``.  ONE
    launch for all the stacks, no device-to-host read.  ``from_output_s``: per stack a numpy (S_k, 3, 4) array or a float64 CUDA
    tensor (S_k, 12).  ``out``: a tensor like ``x`` - ``x`` itself updates in place.  ``reg_lambda > 0``: not built."""
    _not_built_with_motion(reg_lambda, "stack_update_slices")
    x = _check_tensor(x, "stack_update_slices")
    volumes, geometries = _check_stacks(residuals, geometries, x.device, "stack_update_slices")
    tables = list(from_output_s)
    _check_same_count(volumes, tables, "stack_update_slices", "tables")
    tables = [_table_tensor(t, _check_slice_count(v.shape[g.slice_axis], "stack_update_slices"), x.device, f"stack_update_slices: stack {k}")
              for k, (t, v, g) in enumerate(zip(tables, volumes, geometries))]
    step, lo = _check_step(step), _check_clamp(clamp)
    out = x if out is x else out_like(out, x, volumes, "stack_update_slices")
    cnt = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if cover else None
    _update_slices(x, volumes, geometries, tables, step, lo, out, cnt, None, None)
    return out, cnt


class SliceCostWorkspace:
    """The buffers of ``slice_cost`` for stacks of up to ``slices`` slices and ``candidates`` poses each: the candidates' matrices, the
    fixed slots of the sums and the result.  Made once, it serves call after call on one stream; nothing in it needs initialising."""

    def __init__(self, device, slices: int = MAX_SLICES, candidates: int = MAX_CANDIDATES):
        self.slices, self.candidates = _check_slice_count(slices, "SliceCostWorkspace"), int(candidates)
        if not 1 <= self.candidates <= MAX_CANDIDATES:
            raise ValueError(f"SliceCostWorkspace: 1..{MAX_CANDIDATES} candidates, got {candidates}")
        self.cand = torch.empty(self.slices * self.candidates * 12, dtype=torch.float64, device=device)
        self.slots = torch.empty(int(L.load().mrisr_f32_volume_slice_cost_workspace_bytes(self.slices, self.candidates)) // 8,
                                 dtype=torch.float64, device=device)
        self.out = torch.empty(self.slices * self.candidates * 6, dtype=torch.float64, device=device)


def slice_cost(x: torch.Tensor, y: torch.Tensor, geometry: StackGeometry, cand_to_output, stride: int = 1, workspace=None) -> torch.Tensor:
    """The device path of ``slice_cost_np`` -> a float64 CUDA tensor (S, C, 6) (a view of the workspace's result buffer): the counts
    equal, the sums those of a fixed order of addition - within 1e-12 (relative) of the specification's, the same bits on every run.
    ``cand_to_output``: numpy (S, C, 3, 4), uploaded into the workspace.  Two launches (the S C pairs; the slots), no atomics, no
    device-to-host read.  CPU tensors raise."""
    x, y = _check_pair(x, y, "slice_cost")
    g = _check_geometry(geometry, "slice_cost")
    cand, stride = _check_cost_args(y.shape, g.slice_axis, cand_to_output, stride, "slice_cost")
    S, C = cand.shape[:2]
    ws = SliceCostWorkspace(x.device, S, C) if workspace is None else workspace
    if not isinstance(ws, SliceCostWorkspace) or ws.slices < S or ws.candidates < C or ws.cand.device != x.device:
        raise ValueError(f"slice_cost: the workspace must be a SliceCostWorkspace for {S} slices and {C} candidates on {x.device}")
    table, out = ws.cand[:S * C * 12], ws.out[:S * C * 6]
    table.copy_(torch.from_numpy(cand.reshape(-1)))
    L.call("mrisr_f32_volume_slice_cost", x.data_ptr(), *x.shape, y.data_ptr(), *y.shape, table.data_ptr(), S, C, g.slice_axis,
           *_profile_args(g), stride, ws.slots.data_ptr(), out.data_ptr(), L.stream_ptr())
    return out.view(S, C, 6)


def register_slices(x: torch.Tensor, y: torch.Tensor, geometry: StackGeometry, affine, affine_out, params0=None, world=None, levels=None,
                    limits=(10.0, 10.0), min_contrast: float = 0.1, workspace=None) -> SliceMotion:
    """The device path of ``register_slices_np``: the same search on the host (``slice_compass_search``, ``ncc_from_sums``) over the
    sums of ``slice_cost`` - per search iteration one upload of the candidates' matrices, two launches and ONE device-to-host read of
    ``S C 6`` doubles.  The poses are close to the specification's, not bit-equal (the sums differ at 1e-12)."""
    x, y = _check_tensor(x, "register_slices"), _check_tensor(y, "register_slices")
    g = _check_geometry(geometry, "register_slices")
    ws = SliceCostWorkspace(x.device) if workspace is None else workspace
    return _register_slices(lambda cand, stride: slice_cost(x, y, g, cand, stride, ws).cpu().numpy(), tuple(y.shape), g.slice_axis, affine,
                            affine_out, world, params0, levels, limits, min_contrast)


def _slice_launchers(ws, stacks, geometries, step, lo):
    """``volume_stacks._launchers`` with the per-slice kernels on the tables of the workspace -> ``(residual, update, alternate)``; the update
    runs in place, so ``alternate`` is False."""
    to_tables = [t[:y.shape[g.slice_axis]] for t, y, g in zip(ws.to_tables, stacks, geometries)]
    from_tables = [t[:y.shape[g.slice_axis]] for t, y, g in zip(ws.from_tables, stacks, geometries)]

    def residual(x, k):
        _residual_slices(x, stacks[k], geometries[k], to_tables[k], ws.residuals[k], ws.region(k), None)

    def update(x, out, rows):
        if rows is None:
            _update_slices(x, stacks, geometries, from_tables, 1.0, lo, out, ws.cover, None, None)
        else:
            _update_slices(x, ws.residuals, geometries, from_tables, step, lo, out, None, ws.slots, rows)

    return residual, update, False


def _rebuild_slices(ws, stacks, geometries, to_output_s, from_output_s, iterations, step, lo, fill, graph):
    """The estimate from scratch with a pose per slice: the tables go into the workspace, then ``volume_stacks._reconstruct`` with
    the per-slice launchers -> the initial estimate."""
    for k, (y, g) in enumerate(zip(stacks, geometries)):
        S = _check_slice_count(y.shape[g.slice_axis], "combine_stacks")
        ws.to_tables[k][:S].copy_(torch.from_numpy(_check_table(to_output_s[k], S, "combine_stacks").reshape(S, 12)))
        ws.from_tables[k][:S].copy_(torch.from_numpy(_check_table(from_output_s[k], S, "combine_stacks").reshape(S, 12)))
    return _reconstruct(ws, iterations, fill, graph, *_slice_launchers(ws, stacks, geometries, step, lo))


def _motion(motion, ws, initial, stacks, geometries, iterations, step, lo, fill, graph):
    """The motion rounds of ``combine_stacks`` on the estimate in ``ws`` -> ``(the last rebuild's initial estimate - ``initial`` without
    a round -, (params per stack, motion_cost, last))``."""
    first_estimate = [initial]

    def register(k, params, levels):
        return register_slices(ws.x, stacks[k], geometries[k], motion.affines[k], motion.affine_out, params, motion.worlds[k], levels,
                               (motion.limit_mm, motion.limit_deg), motion.min_contrast, workspace=ws.cost)

    def rebuild(to_output_s, from_output_s):
        first_estimate[0] = _rebuild_slices(ws, stacks, geometries, to_output_s, from_output_s, iterations, step, lo, fill, graph)

    extra = _motion_rounds(motion, [tuple(y.shape) for y in stacks], geometries, register, rebuild)
    return first_estimate[0], extra
