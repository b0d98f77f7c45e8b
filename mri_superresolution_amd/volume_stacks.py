"""Super-resolution reconstruction from orthogonal thick-slice stacks on the device (extension): a low-field
head protocol delivers an axial, a coronal and a sagittal stack of one head, each fine in its own plane and 4 - 5 mm through it.
Iterative back-projection (Irani-Peleg) fuses them into one isotropic volume: every iteration simulates each stack from the
current estimate through its slice profile, then back-projects the mean of the residuals.  Both directions are gathers under the
rules of ``volume_reslice.reslice_np`` (``linear``), so the result is deterministic and specified bit for bit.

Stack ``k`` is a float32 volume ``y_k`` with an index -> world affine, a slice axis ``s_k`` and a slice profile of ``T`` samples at
the float64 offsets ``o_t`` along ``s_k`` (in stack-index units) with the float32 weights ``w_t``; ``StackGeometry`` holds them next
to ``M_k`` (stack index -> output index) and ``N_k`` (output index -> stack index), both ``utils.nifti.grid_matrix``.

``slice_profile``, ``default_profile_samples``, ``default_slice_axis``, ``default_output_grid``, ``stack_geometry``   the host side.
``simulate_stack_np``   the forward model alone: a stack from a volume (the tests make their stacks with it).
``regulariser_coeffs``   the weights of the regulariser's neighbour differences from the output grid's voxel sizes.
``stack_residual_np``, ``stack_update_np``, ``combine_stacks_np``   the specification: float32, every product, sum, difference and
                      division rounded on its own (no fma), the orders written in the docstrings.
``stack_residual``, ``stack_update``, ``combine_stacks``   the device path (``csrc/volume_stacks.hip``), equal to the specification
                      bit for bit (the float64 sums of squared residuals: within one spacing, the same bits on every run).  There
                      is no CPU path: CPU tensors raise.  An iteration of ``combine_stacks`` is ``K + 1`` launches; it reads the
                      device once, at its end; the loop is HIP-graph capturable with a ``StackWorkspace`` made before the capture.

Quality (the specification on the CPU, ``tests/stackutil.py``: a 32 x 36 x 40 phantom, three orthogonal stacks, box profile, 10
iterations, no noise): the RMSE against the truth over the initial estimate's is 0.0196, 0.0707 and 0.1058 at thickness factors 2, 3
and 4, falling at every iteration (the stacks are made with this forward model on grids that share the output's voxel edges, the
most favourable case).  With noise of sigma 20 the plain iteration is best after 2 iterations (0.54 of the initial estimate's), is
0.63, 0.66 and 0.62 at iteration 5 and 0.72, 0.79 and 0.76 at iteration 20 (semi-convergence); at sigma 40 it is above 1.19 from
iteration 10 on - worse than the initial estimate.

The regulariser (``reg_lambda``, ``reg_delta``, ``reg_coeffs`` of ``stack_update_np``, ``combine_stacks_np``, ``stack_update`` and
``combine_stacks``; default off) ends that: a Huber prior on the six face neighbours, ``x' = x + step (m + lambda sum_n c_a
clip(x[n] - x[c], -delta, delta))`` over the covered neighbours inside the grid, read before the update (Jacobi).  With lambda =
0.03 and delta = inf the ratio at sigma 20 is 0.578, 0.591 and 0.566 at iteration 10 and 0.579, 0.592 and 0.568 at iteration 20
(sigma 40: 0.89, 0.94, 0.93 at iteration 20): it settles and can be run to convergence - on noisy data use ``--regularise`` rather
than stopping early.  The prior costs detail on clean stacks (0.33, 0.31, 0.30 at iteration 10 against 0.02, 0.07, 0.11); the clip
gives most of it back (lambda = 0.05: 0.158, 0.160, 0.173 with delta = 30 against 0.508, 0.466, 0.439 with delta = inf).  The full
table is in the README.

Speed on an MI355X (``tools/stacks_bench.py --regularise``, 2026-10-20, 256^3 output, three 256 x 256 x 64 stacks, T = 4): 0.44 ms
an iteration - 0.071 ms a residual launch, 0.19 ms the update - against 9.7 ms with torch's ``affine_grid`` + ``grid_sample``;
regularised 0.50 ms an iteration, 0.23 ms the update launch (1.23 times the plain one), against 10.1 ms with torch.

Slice-to-volume motion correction (``motion=MotionOptions(...)`` of ``combine_stacks_np`` / ``combine_stacks``; default off): a 2-D
multi-slice stack is acquired slice by slice and the head moves in between, so every slice gets a rigid pose of its own.
``slice_geometries``   the two matrices of ``stack_geometry`` per slice, from (S, 6) poses about the slices' centres (S <= 256).
``stack_residual_slices_np``, ``simulate_stack_slices_np``, ``stack_update_slices_np``   the two projections with a matrix per slice; the
                      update weights the slices near a voxel by ``1 - |z - s|``, leaves gaps uncovered and normalises overlaps.
``slice_cost_np``, ``ncc_from_sums``, ``slice_compass_search``, ``register_slices_np``   the cost of up to 13 candidate poses of every
                      slice (six float64 sums each), its NCC, and the compass search of ``volume_register`` for all slices at once.
``stack_residual_slices``, ``stack_update_slices``, ``slice_cost``, ``register_slices``   the device path (``csrc/volume_slices.hip``): the
                      projections bit for bit; the sums within 1e-12 and the same bits on every run; one device-to-host read per
                      search iteration.  Measured quality and speed: README, DESIGN.md section 7.

Not built: a 26-neighbour or true total-variation prior; an automatic choice of lambda; the regulariser together with per-slice
poses (``NotImplementedError``); leave-one-stack-out targets for the slice registration (the estimate includes the stack itself);
interleaved acquisition order; outlier slice rejection; motion smoothness over time; an exact adjoint (scatter) back-projection;
intensity or bias matching between stacks inside the loop; more than 8 stacks.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from ._volume_args import check_matrix, check_shape, cuda_tensor, matrix_arg, out_like, volume_np
from .utils.nifti import check_affine, grid_matrix, respaced_grid
from .volume_reslice import taps_np, weighted_sum_np

MAX_STACKS = 8
MAX_SAMPLES = 16
MAX_SLICES = 256                 # per-slice poses: the slices of one stack
MAX_CANDIDATES = 13              # poses of a slice scored in one launch: a point and its 12 compass neighbours
COST_STRIDES = (1, 2, 4)
PROFILES = ("box", "gaussian")
DEFAULT_ITERATIONS = 8
FWHM_PER_SIGMA = 2.0 * math.sqrt(2.0 * math.log(2.0))


class StackGeometry(NamedTuple):
    to_output: np.ndarray        # M (3, 4) float64: stack voxel index -> continuous output voxel index
    from_output: np.ndarray      # N (3, 4) float64: output voxel index -> continuous stack voxel index
    slice_axis: int              # 0..2: the thick axis of the stack
    offsets: np.ndarray          # (T,) float64: the profile's samples along the slice axis, in stack-index units
    weights: np.ndarray          # (T,) float32: their weights, normalised in float64 before the rounding


class StackResult(NamedTuple):
    volume: object               # (X, Y, Z) float32: the estimate after the last iteration
    initial: object              # the initial estimate: the mean of the covering stacks' linear reslices
    rms: np.ndarray              # (iterations, K) float64: the RMS of stack k's residual against the estimate BEFORE the iteration's update
    counts: np.ndarray           # (iterations, K) int64: the voxels of stack k that entered it (weight sum >= 0.5)
    coverage: np.ndarray         # (K + 1,) int64: the output voxels covered by 0, 1, ..., K stacks
    motion: object = None        # with motion: per stack the (S, 6) float64 poses of its slices (tx, ty, tz mm, rx, ry, rz degrees)
    motion_cost: object = None   # with motion: (rounds, K, 2) float64, the mean NCC of the active slices at a round's start and end
    motion_detail: object = None # with motion: per stack the last round's SliceMotion (active flags, per-slice costs)


# ---------------------------------------------------------------- host side: profiles and grids

def slice_profile(profile: str = "box", samples: int = 1, rho: float = 1.0):
    """-> ``(offsets, weights)``: ``samples`` (1..16) points of the slice profile along the slice axis, in stack-index units, float64,
    and their float32 weights - computed in float64, normalised to sum 1, then rounded.  ``rho`` is the slice thickness over the
    spacing along the slice axis (1: contiguous slices).  ``box``: ``o_t = ((t + 0.5) / T - 0.5) rho``, equal weights.
    ``gaussian``: the FWHM is the thickness, ``T`` samples evenly over ``[-rho, rho]`` (one sample: the centre alone)."""
    if profile not in PROFILES:
        raise ValueError(f"Unknown slice profile: {profile!r} (box or gaussian)")
    if not isinstance(samples, (int, np.integer)) or isinstance(samples, bool) or not 1 <= samples <= MAX_SAMPLES:
        raise ValueError(f"profile samples is an integer in 1..{MAX_SAMPLES}, got {samples!r}")
    rho = float(rho)
    if not (np.isfinite(rho) and rho > 0):
        raise ValueError(f"the thickness over the spacing must be finite and positive, got {rho!r}")
    T = int(samples)
    t = np.arange(T, dtype=np.float64)
    if profile == "box":
        offsets = ((t + 0.5) / T - 0.5) * rho
        w = np.ones(T, dtype=np.float64)
    else:
        offsets = np.zeros(1) if T == 1 else (2.0 * t / (T - 1) - 1.0) * rho
        sigma = rho / FWHM_PER_SIGMA
        w = np.exp(-0.5 * (offsets / sigma) ** 2)
    w = 0.5 * (w + w[::-1])                                          # symmetric to the last bit
    offsets = 0.5 * (offsets - offsets[::-1])
    return np.ascontiguousarray(offsets), np.ascontiguousarray((w / w.sum()).astype(np.float32))


def default_profile_samples(profile: str, thickness_mm: float, out_voxel_mm: float) -> int:
    """``clamp(ceil(span / out_voxel_mm), 1, 16)``: a sample per output voxel over the profile's span in mm - the thickness of a
    ``box``, twice the thickness of a ``gaussian``."""
    if profile not in PROFILES:
        raise ValueError(f"Unknown slice profile: {profile!r} (box or gaussian)")
    span = float(thickness_mm) * (2.0 if profile == "gaussian" else 1.0)
    if not (np.isfinite(span) and span > 0 and np.isfinite(out_voxel_mm) and out_voxel_mm > 0):
        raise ValueError(f"thickness {thickness_mm!r} mm and output voxel size {out_voxel_mm!r} mm must be finite and positive")
    return int(min(MAX_SAMPLES, max(1, math.ceil(span / float(out_voxel_mm) - 1e-9))))


def voxel_sizes(affine) -> np.ndarray:
    """(3,) float64: the norms of the three columns of an index -> world affine, in mm."""
    a = check_affine(affine, "affine")
    return np.linalg.norm(a[:3, :3], axis=0)


def default_slice_axis(affine) -> int:
    """The axis with the largest voxel size.  Two largest sizes within 1e-6 of each other (relative) leave no answer: ``ValueError``
    naming ``--slice_axis``."""
    s = voxel_sizes(affine)
    order = np.argsort(s)
    if not np.isfinite(s).all() or s[order[2]] <= 0 or s[order[2]] - s[order[1]] <= 1e-6 * s[order[2]]:
        raise ValueError(f"the voxel sizes {s.tolist()} mm do not single out a slice axis: give it with --slice_axis")
    return int(order[2])


def default_output_grid(affines, shapes, spacing=None):
    """-> ``(affine_out, shape_out)``: a grid with the first stack's orientation, isotropic at the smallest voxel size of any stack
    (or at ``spacing`` mm), whose extent is the bounding box - along the first stack's axes - of the corners of all the stacks.
    The box is cut on the first stack's grid and handed to ``utils.nifti.respaced_grid``, which keeps the corner of its first cell."""
    affines = [check_affine(a, "affine") for a in affines]
    shapes = [check_shape(s, "shape") for s in shapes]
    if not affines or len(affines) != len(shapes):
        raise ValueError(f"default_output_grid takes one shape per affine, got {len(affines)} and {len(shapes)}")
    if spacing is None:
        spacing = float(min(voxel_sizes(a).min() for a in affines))
    spacing = float(spacing)
    if not (np.isfinite(spacing) and spacing > 0):
        raise ValueError(f"the output spacing must be finite and positive, got {spacing!r}")
    first = affines[0]
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for a, n in zip(affines, shapes):
        m = grid_matrix(first, a)                                    # that stack's index -> the first stack's index
        for corner in np.ndindex(2, 2, 2):
            c = m @ np.array([(-0.5 if b == 0 else n[d] - 0.5) for d, b in enumerate(corner)] + [1.0])
            lo, hi = np.minimum(lo, c), np.maximum(hi, c)
    box = first.copy()
    box[:3, 3] = first[:3, :3] @ (lo + 0.5) + first[:3, 3]           # index -0.5 of the box is the low corner
    extent = tuple(max(1, int(np.ceil(hi[d] - lo[d] - 1e-6))) for d in range(3))
    return respaced_grid(box, extent, (spacing,) * 3)


def _check_geometry(g, what) -> StackGeometry:
    if not isinstance(g, StackGeometry):
        raise ValueError(f"{what}: a stack's geometry is a StackGeometry (stack_geometry), got {type(g).__name__}")
    m, n = check_matrix(g.to_output), check_matrix(g.from_output)
    if isinstance(g.slice_axis, bool) or not isinstance(g.slice_axis, (int, np.integer)) or not 0 <= g.slice_axis <= 2:
        raise ValueError(f"{what}: the slice axis is 0, 1 or 2, got {g.slice_axis!r}")
    o, w = np.asarray(g.offsets), np.asarray(g.weights)
    if o.dtype != np.float64 or w.dtype != np.float32 or o.ndim != 1 or o.shape != w.shape or not 1 <= o.size <= MAX_SAMPLES:
        raise ValueError(f"{what}: a profile is 1..{MAX_SAMPLES} float64 offsets and as many float32 weights, got {o.dtype} {o.shape} "
                         f"and {w.dtype} {w.shape}")
    if not (np.isfinite(o).all() and np.isfinite(w).all()):
        raise ValueError(f"{what}: a profile sample is not finite")
    return StackGeometry(m, n, int(g.slice_axis), np.ascontiguousarray(o), np.ascontiguousarray(w))


def stack_geometry(affine, affine_out, slice_axis=None, profile: str = "box", thickness_mm=None, samples=None, world=None) -> StackGeometry:
    """The geometry of a stack with the index -> world ``affine`` against the output grid ``affine_out``.  ``slice_axis``: None takes
    ``default_slice_axis``.  ``thickness_mm``: None takes the spacing along the slice axis (``rho = 1``).  ``samples``: None takes
    ``default_profile_samples`` at the smallest output voxel size.  ``world`` (4 x 4): a rigid transform, reference world -> this
    stack's world (``volume_register.RigidResult.world`` with the reference as the fixed scan), folded into both matrices."""
    a, out = check_affine(affine, "affine"), check_affine(affine_out, "affine_out")
    axis = default_slice_axis(a) if slice_axis is None else slice_axis
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not 0 <= axis <= 2:
        raise ValueError(f"the slice axis is 0, 1 or 2, got {slice_axis!r}")
    spacing = float(voxel_sizes(a)[axis])
    thickness = spacing if thickness_mm is None else float(thickness_mm)
    if not (np.isfinite(thickness) and thickness > 0):
        raise ValueError(f"the slice thickness must be finite and positive, got {thickness_mm!r}")
    if samples is None:
        samples = default_profile_samples(profile, thickness, float(voxel_sizes(out).min()))
    offsets, weights = slice_profile(profile, samples, thickness / spacing)
    if world is not None:
        w = check_affine(world, "world")
        out = w @ out                                                # output index -> this stack's world
    return StackGeometry(grid_matrix(out, a), grid_matrix(a, out), int(axis), offsets, weights)


# ---------------------------------------------------------------- numpy specification

def _check_volume_np(v, what):
    return volume_np(v, what, limit=True)


def _check_step(step) -> np.float32:
    s = np.float32(step)
    if not np.isfinite(s):
        raise ValueError(f"step must be finite, got {step!r}")
    return s


def _check_clamp(clamp):
    if clamp is None:
        return None
    lo = np.float32(clamp)
    if not np.isfinite(lo):
        raise ValueError(f"clamp must be finite or None, got {clamp!r}")
    return lo


def _check_iterations(iterations) -> int:
    if not isinstance(iterations, (int, np.integer)) or isinstance(iterations, bool) or iterations < 0:
        raise ValueError(f"iterations is an integer that is not negative, got {iterations!r}")
    return int(iterations)


def _check_stack_count(n, what):
    if not 1 <= n <= MAX_STACKS:
        raise ValueError(f"{what}: 1..{MAX_STACKS} stacks are combined, got {n}")


def regulariser_coeffs(affine_out) -> np.ndarray:
    """(3,) float32: ``(h_min / h_a)^2`` of the output grid's voxel sizes ``h``, computed in float64 and rounded once - the weights of
    the regulariser's neighbour differences along the three axes; an isotropic grid gives ``(1, 1, 1)``."""
    h = voxel_sizes(affine_out)
    if not (np.isfinite(h).all() and (h > 0).all()):
        raise ValueError(f"the voxel sizes {h.tolist()} mm must be finite and positive")
    return ((h.min() / h) ** 2).astype(np.float32)


def _check_regulariser(step, reg_lambda, reg_delta, reg_coeffs):
    """-> ``(lambda, delta, coeffs)`` in float32 (coeffs: (3,), None gives ones); ``ValueError`` for what the rule cannot take."""
    with np.errstate(all="ignore"):
        lam, delta = np.float32(reg_lambda), np.float32(reg_delta)
    if not (np.isfinite(lam) and lam >= 0):
        raise ValueError(f"reg_lambda must be finite and not negative, got {reg_lambda!r}")
    if not delta > 0:                                                # a NaN compares false
        raise ValueError(f"reg_delta must be positive (inf: the quadratic prior), got {reg_delta!r}")
    if reg_coeffs is None:
        c = np.ones(3, dtype=np.float32)
    else:
        with np.errstate(all="ignore"):
            c = np.asarray(reg_coeffs, dtype=np.float32)
        if c.shape != (3,) or not (np.isfinite(c).all() and (c > 0).all()):
            raise ValueError(f"reg_coeffs are three finite positive numbers, got {reg_coeffs!r}")
    bound = float(step) * float(lam) * ((float(c[0]) + float(c[1])) + float(c[2]))
    if not bound <= 0.5:
        raise ValueError(f"step * reg_lambda * (c_0 + c_1 + c_2) = {bound:.6g} breaks the stability bound <= 0.5 of the explicit "
                         f"diffusion step (unit coefficients, step 1: reg_lambda <= 1/6)")
    return lam, delta, np.ascontiguousarray(c)


def _regulariser_np(x, cnt, delta, coeffs):
    """``reg`` of ``stack_update_np`` for every voxel, float32: axes ascending, the lower neighbour before the upper one."""
    reg = np.zeros(x.shape, dtype=np.float32)
    covered = cnt > 0
    for a in range(3):
        for side in (-1, 1):
            here = [slice(None)] * 3
            there = [slice(None)] * 3
            here[a], there[a] = (slice(1, None), slice(None, -1)) if side < 0 else (slice(None, -1), slice(1, None))
            here, there = tuple(here), tuple(there)
            d = x[there] - x[here]
            psi = np.where(d > delta, delta, np.where(d < -delta, -delta, d))      # a NaN falls through and stays
            reg[here] = np.where(covered[there], reg[here] + coeffs[a] * psi, reg[here])
    return reg


def _index_axes(shape):
    return [np.arange(n, dtype=np.float64).reshape([-1 if a == b else 1 for b in range(3)]) for a, n in enumerate(shape)]


def _matrix_rows(m):
    """The entries of a (3, 4) matrix as ``rows[a][c]``; ``_table_rows`` gives arrays in their place: one matrix per grid point."""
    return [[m[a, c] for c in range(4)] for a in range(3)]


def _table_rows(table, shape):
    """``rows[a][c]`` of a table of matrices ``(..., 3, 4)`` whose leading axes are reshaped to ``shape`` (to broadcast on a grid)."""
    return [[table[..., a, c].reshape(shape) for c in range(4)] for a in range(3)]


def _coordinate_np(row, q):
    return ((row[0] * q[0] + row[1] * q[1]) + row[2] * q[2]) + row[3]


def _gather_rows_np(v, rows, q, shape):
    """-> ``(values at the inside points, inside)``: ``p_a = ((m[a,0] q0 + m[a,1] q1) + m[a,2] q2) + m[a,3]`` in float64, the
    inside test and the linear gather of ``reslice_np`` (taps clamped, reduction along z, then y, then x)."""
    p = [np.broadcast_to(_coordinate_np(rows[a], q), shape) for a in range(3)]
    inside = np.ones(shape, dtype=bool)
    for a in range(3):
        inside &= (p[a] >= -0.5) & (p[a] <= v.shape[a] - 0.5)
    if not inside.any():
        return np.zeros(0, dtype=np.float32), inside
    (ix, wx), (iy, wy), (iz, wz) = (taps_np(pa[inside], n, "linear") for pa, n in zip(p, v.shape))
    rx = []
    for xa in ix:
        ry = [weighted_sum_np(wz, [v[xa, yb, zc] for zc in iz]) for yb in iy]
        rx.append(weighted_sum_np(wy, ry))
    return weighted_sum_np(wx, rx), inside


def _gather_np(v, m, q, shape):
    return _gather_rows_np(v, _matrix_rows(m), q, shape)


def _project_rows_np(x, g, rows, q0, shape):
    """-> ``(acc, wsum)`` of ``stack_residual_np`` on the grid points ``q0`` (three broadcastable index arrays) of ``shape``."""
    acc, wsum = np.zeros(shape, dtype=np.float32), np.zeros(shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        for o, w in zip(g.offsets, g.weights):
            q = list(q0)
            q[g.slice_axis] = q0[g.slice_axis] + o
            val, inside = _gather_rows_np(x, rows, q, shape)
            if val.size:
                acc[inside] = acc[inside] + w * val
                wsum[inside] = wsum[inside] + w
    return acc, wsum


def _project_np(x, g, shape):
    """-> ``(acc, wsum)`` of ``stack_residual_np`` on a stack of ``shape``."""
    return _project_rows_np(x, g, _matrix_rows(g.to_output), _index_axes(shape), shape)


def simulate_stack_np(x, geometry: StackGeometry, stack_shape, fill: float = 0.0) -> np.ndarray:
    """The forward model alone: the float32 stack of ``stack_shape`` that the volume ``x`` gives, ``acc / wsum`` of
    ``stack_residual_np`` where ``wsum >= 0.5`` and ``fill`` elsewhere."""
    x = _check_volume_np(x, "simulate_stack_np")
    g = _check_geometry(geometry, "simulate_stack_np")
    shape = check_shape(stack_shape, "stack_shape")
    acc, wsum = _project_np(x, g, shape)
    ok = wsum >= np.float32(0.5)
    out = np.full(shape, np.float32(fill), dtype=np.float32)
    with np.errstate(all="ignore"):
        out[ok] = acc[ok] / wsum[ok]
    return out


def stack_residual_np(x, y, geometry: StackGeometry):
    """-> ``(r, (S, n))``.  For every stack voxel ``(i, j, k)`` and ``t`` ascending: ``q = (i, j, k)`` in float64 with
    ``q[s] = float64(i_s) + o_t`` (one rounded add); ``p_a = ((M[a,0] q0 + M[a,1] q1) + M[a,2] q2) + M[a,3]``; a sample with
    ``-0.5 <= p_a <= n_a - 0.5`` on all axes of ``x`` adds: ``acc = acc + w_t * val`` with ``val`` the linear gather of
    ``reslice_np`` and ``wsum = wsum + w_t``, float32 from +0, every product and sum rounded; a sample outside adds nothing.
    ``r = y - acc / wsum`` where ``wsum >= 0.5`` and +0 elsewhere.  ``n`` counts the voxels that passed that test and ``S`` is the
    sum of ``float64(r)^2`` over them (each square is exact), correctly rounded (``math.fsum``)."""
    x, y = _check_volume_np(x, "stack_residual_np"), _check_volume_np(y, "stack_residual_np")
    g = _check_geometry(geometry, "stack_residual_np")
    acc, wsum = _project_np(x, g, y.shape)
    ok = wsum >= np.float32(0.5)
    r = np.zeros(y.shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        r[ok] = y[ok] - acc[ok] / wsum[ok]
    r64 = r[ok].astype(np.float64)
    return r, (math.fsum(r64 * r64), int(ok.sum()))


def stack_update_np(x, residuals, geometries, step: float = 1.0, clamp=0.0, reg_lambda: float = 0.0, reg_delta: float = math.inf,
                    reg_coeffs=None):
    """-> ``(x', cnt)``.  For every output voxel and ``k`` ascending: ``p = N_k (i, j, k)`` (the coordinate rule above); inside
    stack ``k``: ``sum = sum + g`` with ``g`` the linear gather of ``residuals[k]`` (border replicated) and ``cnt += 1``.
    ``x' = x + step * (sum / float32(cnt))`` where ``cnt > 0``, every operation rounded to float32, then ``clamp`` where that is
    below ``clamp`` (None: no clamp; a NaN stays); ``x' = x`` where no stack covers the voxel - neither stepped nor clamped.
    ``cnt`` is uint8.

    ``reg_lambda > 0`` adds a Huber prior on the six face neighbours.  With ``m = sum / float32(cnt)``, at a voxel ``c`` with
    ``cnt > 0``: ``reg = +0``; for ``a`` in 0, 1, 2 and ``side`` in -1, +1, the neighbour ``n = c + side e_a`` - skipped when it lies
    outside the grid or no stack covers it (``cnt[n] == 0``: it holds the fill, not anatomy) - adds ``d = x[n] - x[c]``,
    ``psi = delta if d > delta else (-delta if d < -delta else d)`` (a NaN stays), ``reg = reg + c_a * psi``; then
    ``x' = x + step * (m + reg_lambda * reg)``, every operation one rounded float32 operation, and the clamp.  All neighbours are
    read from ``x`` before the update (Jacobi).  ``reg_delta = inf`` is the quadratic prior; ``reg_coeffs`` (None: ones) are the
    ``c_a``, ``regulariser_coeffs`` of the output grid.  ``step * reg_lambda * (c_0 + c_1 + c_2) <= 0.5`` must hold (the limit of
    an explicit diffusion step).  ``reg_lambda = 0`` is the rule above, the same operations as without the keywords."""
    x = _check_volume_np(x, "stack_update_np")
    residuals, geometries = list(residuals), list(geometries)
    _check_stack_count(len(residuals), "stack_update_np")
    if len(geometries) != len(residuals):
        raise ValueError(f"stack_update_np: {len(residuals)} stacks and {len(geometries)} geometries")
    step, lo = _check_step(step), _check_clamp(clamp)
    lam, delta, coeffs = _check_regulariser(step, reg_lambda, reg_delta, reg_coeffs)
    q = _index_axes(x.shape)
    total, cnt = np.zeros(x.shape, dtype=np.float32), np.zeros(x.shape, dtype=np.uint8)
    with np.errstate(all="ignore"):
        for k, (r, g) in enumerate(zip(residuals, geometries)):
            r, g = _check_volume_np(r, f"stack_update_np: stack {k}"), _check_geometry(g, f"stack_update_np: stack {k}")
            val, inside = _gather_np(r, g.from_output, q, x.shape)
            if val.size:
                total[inside] = total[inside] + val
                cnt[inside] += 1
        out = x.copy()
        hit = cnt > 0
        if lam > 0:
            new = x[hit] + step * (total[hit] / cnt[hit].astype(np.float32) + lam * _regulariser_np(x, cnt, delta, coeffs)[hit])
        else:
            new = x[hit] + step * (total[hit] / cnt[hit].astype(np.float32))
        if lo is not None:
            new = np.where(new < lo, lo, new)
        out[hit] = new
    return out, cnt


def _rms_table(sums, counts):
    sums, counts = np.asarray(sums, dtype=np.float64), np.asarray(counts, dtype=np.int64)
    with np.errstate(all="ignore"):
        return np.where(counts > 0, np.sqrt(sums / np.maximum(counts, 1)), 0.0)


# ---------------------------------------------------------------- slice-to-volume motion: geometry and specification

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
    if isinstance(slice_axis, bool) or not isinstance(slice_axis, (int, np.integer)) or not 0 <= slice_axis <= 2:
        raise ValueError(f"the slice axis is 0, 1 or 2, got {slice_axis!r}")
    S = _check_slice_count(shape[slice_axis], "slice_geometries")
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


def _project_slices_np(x, g, shape, to_output_s):
    grid = [1, 1, 1]
    grid[g.slice_axis] = shape[g.slice_axis]
    return _project_rows_np(x, g, _table_rows(to_output_s, grid), _index_axes(shape), shape)


def simulate_stack_slices_np(x, geometry: StackGeometry, stack_shape, to_output_s, fill: float = 0.0) -> np.ndarray:
    """``simulate_stack_np`` with the voxels of slice ``s`` going through ``to_output_s[s]`` (S, 3, 4) in place of ``M``."""
    x, g = _check_volume_np(x, "simulate_stack_slices_np"), _check_geometry(geometry, "simulate_stack_slices_np")
    shape = check_shape(stack_shape, "stack_shape")
    table = _check_table(to_output_s, _check_slice_count(shape[g.slice_axis], "simulate_stack_slices_np"), "simulate_stack_slices_np")
    acc, wsum = _project_slices_np(x, g, shape, table)
    ok = wsum >= np.float32(0.5)
    out = np.full(shape, np.float32(fill), dtype=np.float32)
    with np.errstate(all="ignore"):
        out[ok] = acc[ok] / wsum[ok]
    return out


def stack_residual_slices_np(x, y, geometry: StackGeometry, to_output_s):
    """``stack_residual_np`` -> ``(r, (S, n))`` with the voxels of slice ``s`` using ``to_output_s[s]`` (S, 3, 4) in place of ``M``:
    the same operations voxel by voxel, so equal tables reproduce ``stack_residual_np`` bit for bit."""
    x, y = _check_volume_np(x, "stack_residual_slices_np"), _check_volume_np(y, "stack_residual_slices_np")
    g = _check_geometry(geometry, "stack_residual_slices_np")
    table = _check_table(to_output_s, _check_slice_count(y.shape[g.slice_axis], "stack_residual_slices_np"), "stack_residual_slices_np")
    acc, wsum = _project_slices_np(x, g, y.shape, table)
    ok = wsum >= np.float32(0.5)
    r = np.zeros(y.shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        r[ok] = y[ok] - acc[ok] / wsum[ok]
    r64 = r[ok].astype(np.float64)
    return r, (math.fsum(r64 * r64), int(ok.sum()))


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
        out = x.copy()
        hit = cnt > 0
        new = x[hit] + step * (total[hit] / cnt[hit].astype(np.float32))
        if lo is not None:
            new = np.where(new < lo, lo, new)
        out[hit] = new
    return out, cnt


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
    ok = wsum >= np.float32(0.5)
    with np.errstate(all="ignore"):
        m = np.where(ok, acc / np.where(ok, wsum, np.float32(1)), np.float32(0)).astype(np.float64)
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


def _check_motion(motion, count, what) -> MotionOptions:
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


def _reconstruct_np(stacks, geometries, shape_out, iterations, step, clamp, fill, on_iteration=None, reg=(0.0, math.inf, None), tables=None):
    """The initial estimate and ``iterations`` updates -> ``(x, initial, sums, counts, cnt)``.  ``tables``: None, or the per-slice
    ``(to_output_s, from_output_s)`` lists, which select the ``*_slices_np`` forms of both steps."""
    x0 = np.full(shape_out, np.float32(fill), dtype=np.float32)
    if tables is None:
        x, cnt = stack_update_np(x0, stacks, geometries, 1.0, clamp)
    else:
        x, cnt = stack_update_slices_np(x0, stacks, geometries, tables[1], 1.0, clamp)
    initial = x.copy()
    if on_iteration is not None:
        on_iteration(0, x)
    sums, counts = np.zeros((iterations, len(stacks))), np.zeros((iterations, len(stacks)), dtype=np.int64)
    for it in range(iterations):
        res = []
        for k, (y, g) in enumerate(zip(stacks, geometries)):
            r, (sums[it, k], counts[it, k]) = stack_residual_np(x, y, g) if tables is None else stack_residual_slices_np(x, y, g, tables[0][k])
            res.append(r)
        if tables is None:
            x = stack_update_np(x, res, geometries, step, clamp, *reg)[0]
        else:
            x = stack_update_slices_np(x, res, geometries, tables[1], step, clamp)[0]
        if on_iteration is not None:
            on_iteration(it + 1, x)
    return x, initial, sums, counts, cnt


def combine_stacks_np(stacks, geometries, shape_out, iterations: int = DEFAULT_ITERATIONS, step: float = 1.0, clamp=0.0, fill: float = 0.0,
                      on_iteration=None, reg_lambda: float = 0.0, reg_delta: float = math.inf, reg_coeffs=None, motion=None) -> StackResult:
    """The specification of ``combine_stacks``.  The initial estimate is ``stack_update_np`` of a volume of ``fill`` with ``step = 1``
    and the stacks themselves in place of the residuals: the mean, over the stacks that cover a voxel, of their linear reslices; a
    voxel no stack covers is ``fill`` to the end.  Then ``iterations`` times: ``r_k = stack_residual_np(x, y_k, g_k)`` for every
    stack, ``x = stack_update_np(x, r, g, step, clamp)``.  ``on_iteration(it, x)`` is called with the initial estimate (``it = 0``)
    and after every update.  ``reg_lambda``, ``reg_delta``, ``reg_coeffs``: the regulariser of ``stack_update_np``, in the updates of
    the iterations alone - the initial estimate is never regularised.

    ``motion`` (a ``MotionOptions``; None: everything above, the same operations as without the keyword): slice-to-volume motion
    correction.  The reconstruction above is round 0.  Then ``motion.rounds`` times: (1) every stack's slices are registered to the
    current estimate (``register_slices_np``, from the poses of the round before; the estimate includes the stack itself -
    leave-one-out is not built); (2) the estimate is rebuilt from scratch - initial estimate, then ``iterations`` - with
    ``stack_update_slices_np`` / ``stack_residual_slices_np`` on the new ``slice_geometries``.  ``volume``, ``initial``, ``rms``,
    ``counts`` and ``coverage`` are the last rebuild's; ``on_iteration`` sees round 0 alone.  With ``reg_lambda > 0``:
    ``NotImplementedError`` (not built)."""
    stacks, geometries = [_check_volume_np(y, "combine_stacks_np") for y in stacks], list(geometries)
    _check_stack_count(len(stacks), "combine_stacks_np")
    if len(geometries) != len(stacks):
        raise ValueError(f"combine_stacks_np: {len(stacks)} stacks and {len(geometries)} geometries")
    shape_out, iterations = check_shape(shape_out, "shape_out"), _check_iterations(iterations)
    _check_regulariser(_check_step(step), reg_lambda, reg_delta, reg_coeffs)
    if motion is not None:
        _not_built_with_motion(reg_lambda, "combine_stacks_np")
        motion = _check_motion(motion, len(stacks), "combine_stacks_np")
        geometries = [_check_geometry(g, f"combine_stacks_np: stack {k}") for k, g in enumerate(geometries)]
    state = list(_reconstruct_np(stacks, geometries, shape_out, iterations, step, clamp, fill, on_iteration, (reg_lambda, reg_delta, reg_coeffs)))
    extra = ()
    if motion is not None:
        def register(k, params, levels):
            return register_slices_np(state[0], stacks[k], geometries[k], motion.affines[k], motion.affine_out, params, motion.worlds[k],
                                      levels, (motion.limit_mm, motion.limit_deg), motion.min_contrast)

        def rebuild(to_output_s, from_output_s):
            state[:] = _reconstruct_np(stacks, geometries, shape_out, iterations, step, clamp, fill, tables=(to_output_s, from_output_s))

        extra = _motion_rounds(motion, [y.shape for y in stacks], geometries, register, rebuild)
    x, initial, sums, counts, cnt = state
    return StackResult(x, initial, _rms_table(sums, counts), counts, np.bincount(cnt.reshape(-1), minlength=len(stacks) + 1).astype(np.int64),
                       *extra)


# ---------------------------------------------------------------- device

def _check_tensor(t, what) -> torch.Tensor:
    return cuda_tensor(t, (torch.float32,), what, ndim=3, limit=True)


def _region_bytes() -> int:
    return int(L.load().mrisr_f32_volume_stack_workspace_bytes(1))


def _slots(device, count) -> torch.Tensor:
    return torch.empty(count * _region_bytes() // 8, dtype=torch.int64, device=device)


def _residual(x, y, g, r, slots_ptr, stats_row):
    T = g.offsets.size
    L.call("mrisr_f32_volume_stack_residual", x.data_ptr(), *x.shape, y.data_ptr(), *y.shape, matrix_arg(g.to_output), g.slice_axis,
           (L.C.c_double * T)(*g.offsets.tolist()), (L.C.c_float * T)(*g.weights.tolist()), T, r.data_ptr(), slots_ptr,
           L.ptr(stats_row), L.stream_ptr(), nbytes=4 * (x.numel() + 2 * y.numel()))


def _views_arg(volumes, geometries):
    views = (L.StackView * len(volumes))()
    for view, v, g in zip(views, volumes, geometries):
        view.data, (view.nx, view.ny, view.nz) = v.data_ptr(), v.shape
        view.m[:] = g.from_output.reshape(-1).tolist()
    return views


def _update(x, volumes, geometries, step, lo, out, cover, slots, stats_rows):
    L.call("mrisr_f32_volume_stack_update", x.data_ptr(), *x.shape, _views_arg(volumes, geometries), len(volumes), float(step),
           int(lo is not None), 0.0 if lo is None else float(lo), out.data_ptr(), L.ptr(cover), L.ptr(slots), L.ptr(stats_rows),
           L.stream_ptr(), nbytes=4 * (2 * x.numel() + sum(v.numel() for v in volumes)))


def _update_reg(x, volumes, geometries, step, lo, reg, coverage, out, cover, slots, stats_rows):
    lam, delta, coeffs = reg
    L.call("mrisr_f32_volume_stack_update_reg", x.data_ptr(), *x.shape, _views_arg(volumes, geometries), len(volumes), float(step),
           int(lo is not None), 0.0 if lo is None else float(lo), float(lam), float(delta), (L.C.c_float * 3)(*coeffs.tolist()),
           coverage.data_ptr(), out.data_ptr(), L.ptr(cover), L.ptr(slots), L.ptr(stats_rows), L.stream_ptr(),
           nbytes=4 * (2 * x.numel() + sum(v.numel() for v in volumes)) + x.numel())


def stack_residual(x: torch.Tensor, y: torch.Tensor, geometry: StackGeometry, out=None):
    """The device path of ``stack_residual_np`` -> ``(r, S, n)``: ``r`` bit for bit; ``S`` (0-d float64) within one spacing of the
    specification's sum and the same bits on every run, ``n`` (0-d int64) equal - both stay on the device.  Two launches (the
    residual; one wave that adds the fixed slots), no device-to-host read.  ``out``: another tensor like ``y``."""
    x, y = _check_tensor(x, "stack_residual"), _check_tensor(y, "stack_residual")
    if x.device != y.device:
        raise ValueError(f"stack_residual: the estimate and the stack must share a device, got {x.device} and {y.device}")
    g = _check_geometry(geometry, "stack_residual")
    r = out_like(out, y, (x, y), "stack_residual")
    row = torch.empty(2, dtype=torch.int64, device=x.device)
    _residual(x, y, g, r, _slots(x.device, 1).data_ptr(), row)
    return r, row[:1].view(torch.float64)[0], row[1]


def _check_stacks(volumes, geometries, device, what):
    volumes, geometries = list(volumes), list(geometries)
    _check_stack_count(len(volumes), what)
    if len(geometries) != len(volumes):
        raise ValueError(f"{what}: {len(volumes)} stacks and {len(geometries)} geometries")
    volumes = [_check_tensor(v, f"{what}: stack {k}") for k, v in enumerate(volumes)]
    if any(v.device != device for v in volumes):
        raise ValueError(f"{what}: every stack must lie on {device}")
    return volumes, [_check_geometry(g, f"{what}: stack {k}") for k, g in enumerate(geometries)]


def stack_update(x: torch.Tensor, residuals, geometries, step: float = 1.0, clamp=0.0, out=None, cover: bool = False,
                 reg_lambda: float = 0.0, reg_delta: float = math.inf, reg_coeffs=None, coverage=None):
    """The device path of ``stack_update_np`` -> ``(x', cnt)``, bit for bit; ``cnt`` (uint8) only with ``cover=True``, else None.
    ONE launch for all the stacks, no device-to-host read.  ``out``: a tensor like ``x`` - ``x`` itself updates in place.
    ``reg_lambda > 0``: the regularised kernel, which reads the neighbours of a voxel - ``out`` must not be ``x`` - and the coverage
    counts of these stacks: ``coverage`` (uint8, like ``x``; ``cnt`` of an earlier call) is taken as given, None costs one launch of
    the plain kernel into scratch."""
    x = _check_tensor(x, "stack_update")
    volumes, geometries = _check_stacks(residuals, geometries, x.device, "stack_update")
    step, lo = _check_step(step), _check_clamp(clamp)
    reg = _check_regulariser(step, reg_lambda, reg_delta, reg_coeffs)
    if coverage is not None and (not isinstance(coverage, torch.Tensor) or coverage.dtype != torch.uint8 or coverage.shape != x.shape
                                 or coverage.device != x.device or not coverage.is_contiguous()):
        raise ValueError(f"stack_update: coverage must be a contiguous uint8 tensor of shape {tuple(x.shape)} on {x.device}")
    if reg[0] > 0 and isinstance(out, torch.Tensor) and out.data_ptr() == x.data_ptr():
        raise ValueError("stack_update: with reg_lambda > 0 the neighbours are read before the update: out must be another tensor than x")
    out = x if out is x else out_like(out, x, volumes, "stack_update")
    cnt = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if cover else None
    if reg[0] > 0:
        if coverage is None:
            coverage = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
            _update(x, volumes, geometries, 1.0, None, torch.empty_like(x), coverage, None, None)
        _update_reg(x, volumes, geometries, step, lo, reg, coverage, out, cnt, None, None)
    else:
        _update(x, volumes, geometries, step, lo, out, cnt, None, None)
    return out, cnt


class StackWorkspace:
    """Everything ``combine_stacks`` needs besides the stacks, for this output shape, these stack shapes and this iteration count:
    the estimate, one residual volume per stack, the coverage counts, the fixed slots of the sums (one region per stack) and the
    stats buffer - one (double, int64) row per iteration and stack.  Made before a HIP-graph capture, it serves call after call on
    one stream.  ``regularised``: it also holds a second estimate - the regularised update reads the neighbours of a voxel and cannot
    run in place, so the iterations alternate between the two.  ``motion``: it also holds, per stack, the two tables of per-slice
    matrices (``MAX_SLICES`` x 12 doubles each) and the buffers of the slice cost (``SliceCostWorkspace``)."""

    def __init__(self, shape_out, stack_shapes, device, iterations: int = DEFAULT_ITERATIONS, regularised: bool = False, motion: bool = False):
        self.shape_out = check_shape(shape_out, "shape_out")
        self.stack_shapes = tuple(check_shape(s, "stack shape") for s in stack_shapes)
        _check_stack_count(len(self.stack_shapes), "StackWorkspace")
        self.iterations = _check_iterations(iterations)
        self.key = (self.shape_out, self.stack_shapes, self.iterations)
        self.x = torch.empty(self.shape_out, dtype=torch.float32, device=device)
        self.x2 = torch.empty_like(self.x) if regularised else None
        self.residuals = [torch.empty(s, dtype=torch.float32, device=device) for s in self.stack_shapes]
        self.cover = torch.empty(self.shape_out, dtype=torch.uint8, device=device)
        self.slots = _slots(device, len(self.stack_shapes))
        self.stats = torch.zeros((max(self.iterations, 1), len(self.stack_shapes), 2), dtype=torch.int64, device=device)
        self.to_tables = self.from_tables = self.cost = None
        if motion:
            self.to_tables = [torch.zeros((MAX_SLICES, 12), dtype=torch.float64, device=device) for _ in self.stack_shapes]
            self.from_tables = [torch.zeros((MAX_SLICES, 12), dtype=torch.float64, device=device) for _ in self.stack_shapes]
            self.cost = SliceCostWorkspace(device)

    def region(self, k) -> int:
        return self.slots.data_ptr() + k * _region_bytes()


def _iterate(ws, stacks, geometries, first, count, step, lo, reg=None):
    """``count`` iterations from row ``first``, ``K + 1`` launches each: the residual of every stack against the estimate, then the
    update in place, whose first wave adds the residuals' slots into the iteration's stats rows.  Nothing is allocated.  ``reg``
    (``_check_regulariser``): the regularised update, from ``ws.x`` into ``ws.x2`` in the even iterations and back in the odd ones,
    with the coverage counts in ``ws.cover``."""
    for it in range(first, first + count):
        x, out = (ws.x, ws.x) if reg is None else ((ws.x, ws.x2) if it % 2 == 0 else (ws.x2, ws.x))
        for k, (y, g) in enumerate(zip(stacks, geometries)):
            _residual(x, y, g, ws.residuals[k], ws.region(k), None)
        if reg is None:
            _update(x, ws.residuals, geometries, step, lo, out, None, ws.slots, ws.stats[it])
        else:
            _update_reg(x, ws.residuals, geometries, step, lo, reg, ws.cover, out, None, ws.slots, ws.stats[it])


def combine_stacks(stacks, geometries, shape_out, iterations: int = DEFAULT_ITERATIONS, step: float = 1.0, clamp=0.0, fill: float = 0.0,
                   workspace=None, graph: bool = False, check: bool = False, reg_lambda: float = 0.0, reg_delta: float = math.inf,
                   reg_coeffs=None, motion=None) -> StackResult:
    """The device path of ``combine_stacks_np``: ``volume`` and ``initial`` (CUDA tensors) bit for bit, ``counts`` and ``coverage``
    equal, ``rms`` from sums within one spacing.  An iteration is ``K + 1`` launches; the one device-to-host read - the stats rows
    and the coverage counts - is the last thing done.  ``graph``: the iteration loop is captured into a HIP graph and replayed
    (after one eager iteration as a warm-up, which loads the code objects) - the same bits as the eager loop.  ``workspace``: a
    ``StackWorkspace`` of these shapes and this iteration count.  ``check``: a volume that is not finite everywhere raises - the
    flag travels in the same read.  ``reg_lambda``, ``reg_delta``, ``reg_coeffs``: the regulariser of ``stack_update_np``; with
    ``reg_lambda > 0`` the iterations run the regularised kernel between the two estimates of a ``StackWorkspace(...,
    regularised=True)`` - still ``K + 1`` launches and one read; with 0 the kernels and the bits are those without the keywords.

    ``motion`` (a ``MotionOptions``; None: the launches and the bits of a call without the keyword): the rounds of
    ``combine_stacks_np`` with ``register_slices`` - one launch pair and ONE device-to-host read of ``S C 6`` doubles per search
    iteration - and the per-slice kernels of ``csrc/volume_slices.hip``; the workspace is a ``StackWorkspace(..., motion=True)``.  Every
    round's rebuild is ``K + 1`` launches an iteration on tables that lie in the workspace, and with ``graph`` is captured and
    replayed on its own - the same bits as eager.  The poses are not bit-compared with the specification's (near-ties of the cost at
    1e-12 may resolve differently).  With ``reg_lambda > 0``: ``NotImplementedError`` (not built)."""
    if not stacks:
        raise ValueError(f"combine_stacks: 1..{MAX_STACKS} stacks are combined, got 0")
    first = _check_tensor(list(stacks)[0], "combine_stacks: stack 0")
    stacks, geometries = _check_stacks(stacks, geometries, first.device, "combine_stacks")
    shape_out, iterations = check_shape(shape_out, "shape_out"), _check_iterations(iterations)
    step, lo = _check_step(step), _check_clamp(clamp)
    reg = _check_regulariser(step, reg_lambda, reg_delta, reg_coeffs)
    reg = reg if reg[0] > 0 else None
    if motion is not None:
        _not_built_with_motion(reg_lambda, "combine_stacks")
        motion = _check_motion(motion, len(stacks), "combine_stacks")
    if workspace is None:
        workspace = StackWorkspace(shape_out, [y.shape for y in stacks], first.device, iterations, regularised=reg is not None,
                                   motion=motion is not None)
    ws = workspace
    if not isinstance(ws, StackWorkspace) or ws.key != (shape_out, tuple(tuple(y.shape) for y in stacks), iterations) \
            or ws.x.device != first.device:
        raise ValueError(f"combine_stacks: the workspace must be a StackWorkspace for an output of {shape_out}, these stack shapes and "
                         f"{iterations} iterations on {first.device}")
    if reg is not None and ws.x2 is None:
        raise ValueError("combine_stacks: reg_lambda > 0 needs a workspace with the second estimate: StackWorkspace(..., regularised=True)")
    if motion is not None and ws.cost is None:
        raise ValueError("combine_stacks: motion needs a workspace with the tables and the cost buffers: StackWorkspace(..., motion=True)")
    K = len(stacks)
    ws.x.fill_(float(fill))
    _update(ws.x, stacks, geometries, 1.0, lo, ws.x, ws.cover, None, None)
    initial = ws.x.clone()
    if graph and iterations:
        _iterate(ws, stacks, geometries, 0, 1, step, lo, reg)
        ws.x.copy_(initial)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _iterate(ws, stacks, geometries, 0, iterations, step, lo, reg)
        g.replay()
    else:
        _iterate(ws, stacks, geometries, 0, iterations, step, lo, reg)
    extra = ()
    if motion is not None:
        first_estimate = [initial]

        def register(k, params, levels):
            return register_slices(ws.x, stacks[k], geometries[k], motion.affines[k], motion.affine_out, params, motion.worlds[k], levels,
                                   (motion.limit_mm, motion.limit_deg), motion.min_contrast, workspace=ws.cost)

        def rebuild(to_output_s, from_output_s):
            first_estimate[0] = _rebuild_slices(ws, stacks, geometries, to_output_s, from_output_s, iterations, step, lo, fill, graph)

        extra = _motion_rounds(motion, [tuple(y.shape) for y in stacks], geometries, register, rebuild)
        initial = first_estimate[0]
    volume = (ws.x2 if reg is not None and iterations % 2 else ws.x).clone()       # the estimate an odd count of regularised updates left
    tail = [torch.stack([(ws.cover == c).sum() for c in range(K + 1)])]
    if check:
        tail.append(torch.isfinite(volume).all().to(torch.int64).reshape(1))
    host = torch.cat([ws.stats.reshape(-1)] + tail).cpu().numpy()       # the one device-to-host read
    rows = host[:ws.stats.numel()].reshape(ws.stats.shape)[:iterations]
    sums, counts = rows[..., 0].copy().view(np.float64), rows[..., 1].copy()
    coverage = host[ws.stats.numel():ws.stats.numel() + K + 1].copy()
    if check and not host[-1]:
        raise ValueError("combine_stacks: the reconstructed volume is not finite everywhere")
    return StackResult(volume, initial, _rms_table(sums, counts), counts, coverage, *extra)


# ---------------------------------------------------------------- device: slice-to-volume motion

def _table_tensor(table, slices, device, what) -> torch.Tensor:
    """A (slices, 12) float64 table on ``device``: a numpy (slices, 3, 4) array is checked and uploaded, a tensor taken as given."""
    if isinstance(table, torch.Tensor):
        t = cuda_tensor(table, (torch.float64,), what, name="the table of per-slice matrices", shape=(slices, 12))
        if t.device != device:
            raise ValueError(f"{what}: the table of per-slice matrices must lie on {device}")
        return t
    return torch.from_numpy(_check_table(table, slices, what).reshape(slices, 12)).to(device)


def _profile_args(g):
    T = g.offsets.size
    return (L.C.c_double * T)(*g.offsets.tolist()), (L.C.c_float * T)(*g.weights.tolist()), T


def _residual_slices(x, y, g, table, r, slots_ptr, stats_row):
    L.call("mrisr_f32_volume_stack_residual_slices", x.data_ptr(), *x.shape, y.data_ptr(), *y.shape, table.data_ptr(), y.shape[g.slice_axis],
           g.slice_axis, *_profile_args(g), r.data_ptr(), slots_ptr, L.ptr(stats_row), L.stream_ptr(), nbytes=4 * (x.numel() + 2 * y.numel()))


def _update_slices(x, volumes, geometries, tables, step, lo, out, cover, slots, stats_rows):
    views = (L.StackSlicesView * len(volumes))()
    for view, v, g, t in zip(views, volumes, geometries, tables):
        view.data, (view.nx, view.ny, view.nz), view.slice_axis = v.data_ptr(), v.shape, g.slice_axis
        view.from_output, view.slices = t.data_ptr(), v.shape[g.slice_axis]
    L.call("mrisr_f32_volume_stack_update_slices", x.data_ptr(), *x.shape, views, len(volumes), float(step), int(lo is not None),
           0.0 if lo is None else float(lo), out.data_ptr(), L.ptr(cover), L.ptr(slots), L.ptr(stats_rows), L.stream_ptr(),
           nbytes=4 * (2 * x.numel() + sum(v.numel() for v in volumes)))


def stack_residual_slices(x: torch.Tensor, y: torch.Tensor, geometry: StackGeometry, to_output_s, out=None):
    """The device path of ``stack_residual_slices_np`` -> ``(r, S, n)`` as ``stack_residual``: ``r`` bit for bit.  ``to_output_s``: a
    numpy (S, 3, 4) array (uploaded) or a float64 CUDA tensor (S, 12).  CPU tensors raise."""
    x, y = _check_tensor(x, "stack_residual_slices"), _check_tensor(y, "stack_residual_slices")
    if x.device != y.device:
        raise ValueError(f"stack_residual_slices: the estimate and the stack must share a device, got {x.device} and {y.device}")
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
    if len(tables) != len(volumes):
        raise ValueError(f"stack_update_slices: {len(volumes)} stacks and {len(tables)} tables")
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
    x, y = _check_tensor(x, "slice_cost"), _check_tensor(y, "slice_cost")
    if x.device != y.device:
        raise ValueError(f"slice_cost: the estimate and the stack must share a device, got {x.device} and {y.device}")
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


def _iterate_slices(ws, stacks, geometries, count, step, lo):
    """``_iterate`` with the per-slice kernels on the tables of the workspace: ``K + 1`` launches an iteration, nothing allocated."""
    to_tables = [t[:y.shape[g.slice_axis]] for t, y, g in zip(ws.to_tables, stacks, geometries)]
    from_tables = [t[:y.shape[g.slice_axis]] for t, y, g in zip(ws.from_tables, stacks, geometries)]
    for it in range(count):
        for k, (y, g) in enumerate(zip(stacks, geometries)):
            _residual_slices(ws.x, y, g, to_tables[k], ws.residuals[k], ws.region(k), None)
        _update_slices(ws.x, ws.residuals, geometries, from_tables, step, lo, ws.x, None, ws.slots, ws.stats[it])


def _rebuild_slices(ws, stacks, geometries, to_output_s, from_output_s, iterations, step, lo, fill, graph):
    """The estimate from scratch with a pose per slice: the tables go into the workspace, then the initial estimate and
    ``iterations`` updates (captured and replayed with ``graph``) -> the initial estimate."""
    for k, (y, g) in enumerate(zip(stacks, geometries)):
        S = _check_slice_count(y.shape[g.slice_axis], "combine_stacks")
        ws.to_tables[k][:S].copy_(torch.from_numpy(_check_table(to_output_s[k], S, "combine_stacks").reshape(S, 12)))
        ws.from_tables[k][:S].copy_(torch.from_numpy(_check_table(from_output_s[k], S, "combine_stacks").reshape(S, 12)))
    from_tables = [t[:y.shape[g.slice_axis]] for t, y, g in zip(ws.from_tables, stacks, geometries)]
    ws.x.fill_(float(fill))
    _update_slices(ws.x, stacks, geometries, from_tables, 1.0, lo, ws.x, ws.cover, None, None)
    initial = ws.x.clone()
    if graph and iterations:
        _iterate_slices(ws, stacks, geometries, 1, step, lo)
        ws.x.copy_(initial)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _iterate_slices(ws, stacks, geometries, iterations, step, lo)
        g.replay()
    else:
        _iterate_slices(ws, stacks, geometries, iterations, step, lo)
    return initial
