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

Slice-to-volume motion correction (``motion=volume_slices.MotionOptions(...)`` of ``combine_stacks_np`` / ``combine_stacks``; default
off) and everything with a pose per slice live in ``volume_slices.py``, which imports this module; the two ``combine_stacks`` reach it
through an import inside the function, under ``if motion is not None``.

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
from .volume_reslice import sample_np

MAX_STACKS = 8
MAX_SAMPLES = 16
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


def _check_slice_axis(axis, prefix="") -> int:
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not 0 <= axis <= 2:
        raise ValueError(f"{prefix}the slice axis is 0, 1 or 2, got {axis!r}")
    return int(axis)


def _check_geometry(g, what) -> StackGeometry:
    if not isinstance(g, StackGeometry):
        raise ValueError(f"{what}: a stack's geometry is a StackGeometry (stack_geometry), got {type(g).__name__}")
    m, n = check_matrix(g.to_output), check_matrix(g.from_output)
    axis = _check_slice_axis(g.slice_axis, f"{what}: ")
    o, w = np.asarray(g.offsets), np.asarray(g.weights)
    if o.dtype != np.float64 or w.dtype != np.float32 or o.ndim != 1 or o.shape != w.shape or not 1 <= o.size <= MAX_SAMPLES:
        raise ValueError(f"{what}: a profile is 1..{MAX_SAMPLES} float64 offsets and as many float32 weights, got {o.dtype} {o.shape} "
                         f"and {w.dtype} {w.shape}")
    if not (np.isfinite(o).all() and np.isfinite(w).all()):
        raise ValueError(f"{what}: a profile sample is not finite")
    return StackGeometry(m, n, axis, np.ascontiguousarray(o), np.ascontiguousarray(w))


def stack_geometry(affine, affine_out, slice_axis=None, profile: str = "box", thickness_mm=None, samples=None, world=None) -> StackGeometry:
    """The geometry of a stack with the index -> world ``affine`` against the output grid ``affine_out``.  ``slice_axis``: None takes
    ``default_slice_axis``.  ``thickness_mm``: None takes the spacing along the slice axis (``rho = 1``).  ``samples``: None takes
    ``default_profile_samples`` at the smallest output voxel size.  ``world`` (4 x 4): a rigid transform, reference world -> this
    stack's world (``volume_register.RigidResult.world`` with the reference as the fixed scan), folded into both matrices."""
    a, out = check_affine(affine, "affine"), check_affine(affine_out, "affine_out")
    axis = default_slice_axis(a) if slice_axis is None else _check_slice_axis(slice_axis)
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
    return StackGeometry(grid_matrix(out, a), grid_matrix(a, out), axis, offsets, weights)


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


def _check_same_count(stacks, others, what, things="geometries"):
    if len(others) != len(stacks):
        raise ValueError(f"{what}: {len(stacks)} stacks and {len(others)} {things}")


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
    return sample_np([v], [pa[inside] for pa in p], "linear")[0], inside


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


def _simulated_np(acc, wsum, fill=0.0):
    """-> ``(m, ok)``: the simulated values of a projection, ``acc / wsum`` where ``wsum >= 0.5`` (``ok``) and ``fill`` elsewhere."""
    ok = wsum >= np.float32(0.5)
    m = np.full(acc.shape, np.float32(fill), dtype=np.float32)
    with np.errstate(all="ignore"):
        m[ok] = acc[ok] / wsum[ok]
    return m, ok


def _residual_np(x, y, g, rows):
    """``stack_residual_np`` through ``rows`` -> ``(r, (S, n))``."""
    m, ok = _simulated_np(*_project_rows_np(x, g, rows, _index_axes(y.shape), y.shape))
    r = np.zeros(y.shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        r[ok] = y[ok] - m[ok]
    r64 = r[ok].astype(np.float64)
    return r, (math.fsum(r64 * r64), int(ok.sum()))


def _step_np(x, total, cnt, step, lo, prior=None):
    """The tail of every update: ``x + step * (total / float32(cnt) [+ prior])`` where ``cnt > 0``, clamped from below at ``lo`` (None:
    no clamp); ``x`` where no stack covers the voxel."""
    out = x.copy()
    hit = cnt > 0
    with np.errstate(all="ignore"):
        m = total[hit] / cnt[hit].astype(np.float32)
        new = x[hit] + step * (m if prior is None else m + prior[hit])
        if lo is not None:
            new = np.where(new < lo, lo, new)
    out[hit] = new
    return out


def simulate_stack_np(x, geometry: StackGeometry, stack_shape, fill: float = 0.0) -> np.ndarray:
    """The forward model alone: the float32 stack of ``stack_shape`` that the volume ``x`` gives, ``acc / wsum`` of
    ``stack_residual_np`` where ``wsum >= 0.5`` and ``fill`` elsewhere."""
    x = _check_volume_np(x, "simulate_stack_np")
    g = _check_geometry(geometry, "simulate_stack_np")
    shape = check_shape(stack_shape, "stack_shape")
    return _simulated_np(*_project_rows_np(x, g, _matrix_rows(g.to_output), _index_axes(shape), shape), fill)[0]


def stack_residual_np(x, y, geometry: StackGeometry):
    """-> ``(r, (S, n))``.  For every stack voxel ``(i, j, k)`` and ``t`` ascending: ``q = (i, j, k)`` in float64 with
    ``q[s] = float64(i_s) + o_t`` (one rounded add); ``p_a = ((M[a,0] q0 + M[a,1] q1) + M[a,2] q2) + M[a,3]``; a sample with
    ``-0.5 <= p_a <= n_a - 0.5`` on all axes of ``x`` adds: ``acc = acc + w_t * val`` with ``val`` the linear gather of
    ``reslice_np`` and ``wsum = wsum + w_t``, float32 from +0, every product and sum rounded; a sample outside adds nothing.
    ``r = y - acc / wsum`` where ``wsum >= 0.5`` and +0 elsewhere.  ``n`` counts the voxels that passed that test and ``S`` is the
    sum of ``float64(r)^2`` over them (each square is exact), correctly rounded (``math.fsum``)."""
    x, y = _check_volume_np(x, "stack_residual_np"), _check_volume_np(y, "stack_residual_np")
    g = _check_geometry(geometry, "stack_residual_np")
    return _residual_np(x, y, g, _matrix_rows(g.to_output))


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
    _check_same_count(residuals, geometries, "stack_update_np")
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
        prior = lam * _regulariser_np(x, cnt, delta, coeffs) if lam > 0 else None
    return _step_np(x, total, cnt, step, lo, prior), cnt


def _rms_table(sums, counts):
    sums, counts = np.asarray(sums, dtype=np.float64), np.asarray(counts, dtype=np.int64)
    with np.errstate(all="ignore"):
        return np.where(counts > 0, np.sqrt(sums / np.maximum(counts, 1)), 0.0)


def _steps_np(stacks, geometries, step, clamp, reg=(0.0, math.inf, None)):
    """The two steps of ``_reconstruct_np`` with one matrix per stack."""
    def residual(x, k):
        return stack_residual_np(x, stacks[k], geometries[k])

    def update(x, volumes, first):
        return stack_update_np(x, volumes, geometries, 1.0, clamp) if first else stack_update_np(x, volumes, geometries, step, clamp, *reg)

    return residual, update


def _reconstruct_np(stacks, shape_out, iterations, fill, residual, update, on_iteration=None):
    """The initial estimate and ``iterations`` updates -> ``(x, initial, sums, counts, cnt)``, over a pair of steps (``_steps_np``, or
    ``volume_slices._slice_steps_np`` with a pose per slice): ``residual(x, k) -> (r, (S, n))`` of stack ``k``; ``update(x, volumes,
    first) -> (x', cnt)`` - ``first``: the initial estimate, from the stacks themselves with step 1 and never regularised."""
    x, cnt = update(np.full(shape_out, np.float32(fill), dtype=np.float32), stacks, True)
    initial = x.copy()
    if on_iteration is not None:
        on_iteration(0, x)
    sums, counts = np.zeros((iterations, len(stacks))), np.zeros((iterations, len(stacks)), dtype=np.int64)
    for it in range(iterations):
        res = []
        for k in range(len(stacks)):
            r, (sums[it, k], counts[it, k]) = residual(x, k)
            res.append(r)
        x = update(x, res, False)[0]
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

    ``motion`` (a ``volume_slices.MotionOptions``; None: everything above, the same operations as without the keyword): slice-to-volume motion
    correction.  The reconstruction above is round 0.  Then ``motion.rounds`` times: (1) every stack's slices are registered to the
    current estimate (``volume_slices.register_slices_np``, from the poses of the round before; the estimate includes the stack itself -
    leave-one-out is not built); (2) the estimate is rebuilt from scratch - initial estimate, then ``iterations`` - with
    ``stack_update_slices_np`` / ``stack_residual_slices_np`` on the new ``slice_geometries``.  ``volume``, ``initial``, ``rms``,
    ``counts`` and ``coverage`` are the last rebuild's; ``on_iteration`` sees round 0 alone.  With ``reg_lambda > 0``:
    ``NotImplementedError`` (not built)."""
    stacks, geometries = [_check_volume_np(y, "combine_stacks_np") for y in stacks], list(geometries)
    _check_stack_count(len(stacks), "combine_stacks_np")
    _check_same_count(stacks, geometries, "combine_stacks_np")
    shape_out, iterations = check_shape(shape_out, "shape_out"), _check_iterations(iterations)
    _check_regulariser(_check_step(step), reg_lambda, reg_delta, reg_coeffs)
    if motion is not None:
        from . import volume_slices
        motion = volume_slices._check_motion(motion, len(stacks), reg_lambda, "combine_stacks_np")
        geometries = [_check_geometry(g, f"combine_stacks_np: stack {k}") for k, g in enumerate(geometries)]
    state = list(_reconstruct_np(stacks, shape_out, iterations, fill, *_steps_np(stacks, geometries, step, clamp, (reg_lambda, reg_delta, reg_coeffs)),
                                 on_iteration))
    extra = ()
    if motion is not None:
        extra = volume_slices._motion_np(motion, state, stacks, geometries, shape_out, iterations, step, clamp, fill)
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


def _profile_args(g):
    T = g.offsets.size
    return (L.C.c_double * T)(*g.offsets.tolist()), (L.C.c_float * T)(*g.weights.tolist()), T


def _residual(x, y, g, r, slots_ptr, stats_row):
    L.call("mrisr_f32_volume_stack_residual", x.data_ptr(), *x.shape, y.data_ptr(), *y.shape, matrix_arg(g.to_output), g.slice_axis,
           *_profile_args(g), r.data_ptr(), slots_ptr, L.ptr(stats_row), L.stream_ptr(), nbytes=4 * (x.numel() + 2 * y.numel()))


def _views_arg(volumes, geometries):
    views = (L.StackView * len(volumes))()
    for view, v, g in zip(views, volumes, geometries):
        view.data, (view.nx, view.ny, view.nz) = v.data_ptr(), v.shape
        view.m[:] = g.from_output.reshape(-1).tolist()
    return views


def _step_args(step, lo):
    """``step, use_clamp, lo`` of the update entry points."""
    return float(step), int(lo is not None), 0.0 if lo is None else float(lo)


def _update_bytes(x, volumes) -> int:
    return 4 * (2 * x.numel() + sum(v.numel() for v in volumes))


def _update(x, volumes, geometries, step, lo, out, cover, slots, stats_rows):
    L.call("mrisr_f32_volume_stack_update", x.data_ptr(), *x.shape, _views_arg(volumes, geometries), len(volumes), *_step_args(step, lo),
           out.data_ptr(), L.ptr(cover), L.ptr(slots), L.ptr(stats_rows), L.stream_ptr(), nbytes=_update_bytes(x, volumes))


def _update_reg(x, volumes, geometries, step, lo, reg, coverage, out, cover, slots, stats_rows):
    lam, delta, coeffs = reg
    L.call("mrisr_f32_volume_stack_update_reg", x.data_ptr(), *x.shape, _views_arg(volumes, geometries), len(volumes), *_step_args(step, lo),
           float(lam), float(delta), (L.C.c_float * 3)(*coeffs.tolist()), coverage.data_ptr(), out.data_ptr(), L.ptr(cover), L.ptr(slots),
           L.ptr(stats_rows), L.stream_ptr(), nbytes=_update_bytes(x, volumes) + x.numel())


def _check_pair(x, y, what):
    """The estimate and a stack of one entry: two float32 CUDA volumes on one device."""
    x, y = _check_tensor(x, what), _check_tensor(y, what)
    if x.device != y.device:
        raise ValueError(f"{what}: the estimate and the stack must share a device, got {x.device} and {y.device}")
    return x, y


def stack_residual(x: torch.Tensor, y: torch.Tensor, geometry: StackGeometry, out=None):
    """The device path of ``stack_residual_np`` -> ``(r, S, n)``: ``r`` bit for bit; ``S`` (0-d float64) within one spacing of the
    specification's sum and the same bits on every run, ``n`` (0-d int64) equal - both stay on the device.  Two launches (the
    residual; one wave that adds the fixed slots), no device-to-host read.  ``out``: another tensor like ``y``."""
    x, y = _check_pair(x, y, "stack_residual")
    g = _check_geometry(geometry, "stack_residual")
    r = out_like(out, y, (x, y), "stack_residual")
    row = torch.empty(2, dtype=torch.int64, device=x.device)
    _residual(x, y, g, r, _slots(x.device, 1).data_ptr(), row)
    return r, row[:1].view(torch.float64)[0], row[1]


def _check_stacks(volumes, geometries, device, what):
    volumes, geometries = list(volumes), list(geometries)
    _check_stack_count(len(volumes), what)
    _check_same_count(volumes, geometries, what)
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
            from .volume_slices import MAX_SLICES, SliceCostWorkspace
            self.to_tables = [torch.zeros((MAX_SLICES, 12), dtype=torch.float64, device=device) for _ in self.stack_shapes]
            self.from_tables = [torch.zeros((MAX_SLICES, 12), dtype=torch.float64, device=device) for _ in self.stack_shapes]
            self.cost = SliceCostWorkspace(device)

    def region(self, k) -> int:
        return self.slots.data_ptr() + k * _region_bytes()


def _launchers(ws, stacks, geometries, step, lo, reg=None):
    """-> ``(residual, update, alternate)`` for ``_iterate`` and ``_reconstruct``, with one matrix per stack.  ``residual(x, k)``: the
    residual of stack ``k`` against ``x`` into ``ws.residuals[k]`` and region ``k`` of the slots.  ``update(x, out, rows)``: the update
    from the residuals, whose first wave adds those slots into the stats ``rows``; ``rows`` None: the initial estimate - the stacks
    themselves, step 1, the coverage counts into ``ws.cover``.  ``reg`` (``_check_regulariser``): the regularised update, which reads
    ``ws.cover`` and cannot run in place, so the iterations alternate between the two estimates."""
    def residual(x, k):
        _residual(x, stacks[k], geometries[k], ws.residuals[k], ws.region(k), None)

    def update(x, out, rows):
        if rows is None:
            _update(x, stacks, geometries, 1.0, lo, out, ws.cover, None, None)
        elif reg is None:
            _update(x, ws.residuals, geometries, step, lo, out, None, ws.slots, rows)
        else:
            _update_reg(x, ws.residuals, geometries, step, lo, reg, ws.cover, out, None, ws.slots, rows)

    return residual, update, reg is not None


def _iterate(ws, first, count, residual, update, alternate):
    """``count`` iterations from row ``first``, ``K + 1`` launches each: the residual of every stack against the estimate, then the
    update.  Nothing is allocated.  ``alternate``: from ``ws.x`` into ``ws.x2`` in the even iterations and back in the odd ones; else
    in place."""
    for it in range(first, first + count):
        x, out = (ws.x, ws.x) if not alternate else ((ws.x, ws.x2) if it % 2 == 0 else (ws.x2, ws.x))
        for k in range(len(ws.residuals)):
            residual(x, k)
        update(x, out, ws.stats[it])


def _reconstruct(ws, iterations, fill, graph, residual, update, alternate):
    """The estimate from scratch in the workspace -> the initial estimate (a clone): fill, the initial update with the coverage
    counts, then ``iterations`` of ``_iterate`` - with ``graph`` captured into a HIP graph and replayed, after one eager iteration as
    a warm-up (it loads the code objects) whose result is undone."""
    ws.x.fill_(float(fill))
    update(ws.x, ws.x, None)
    initial = ws.x.clone()
    if graph and iterations:
        _iterate(ws, 0, 1, residual, update, alternate)
        ws.x.copy_(initial)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _iterate(ws, 0, iterations, residual, update, alternate)
        g.replay()
    else:
        _iterate(ws, 0, iterations, residual, update, alternate)
    return initial


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

    ``motion`` (a ``volume_slices.MotionOptions``; None: the launches and the bits of a call without the keyword): the rounds of
    ``combine_stacks_np`` with ``volume_slices.register_slices`` - one launch pair and ONE device-to-host read of ``S C 6`` doubles per search
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
        from . import volume_slices
        motion = volume_slices._check_motion(motion, len(stacks), reg_lambda, "combine_stacks")
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
    initial = _reconstruct(ws, iterations, fill, graph, *_launchers(ws, stacks, geometries, step, lo, reg))
    extra = ()
    if motion is not None:
        initial, extra = volume_slices._motion(motion, ws, initial, stacks, geometries, iterations, step, lo, fill, graph)
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

