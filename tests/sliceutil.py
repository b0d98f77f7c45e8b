"""Helpers shared by the slice-motion tests: orthogonal stacks of the phantom of ``stackutil`` whose slices were acquired under
per-slice rigid poses drawn from a fixed seed (``simulate_stack_slices_np``), the corner-displacement measures of a recovered
motion, and small stacks with hand-made poses (a gap, an overlap, a slice pushed out of the volume) for the bit comparisons."""
import functools

import numpy as np

from mri_superresolution_amd import volume_slices as V
from mri_superresolution_amd import volume_stacks as S
from stackutil import oblique_affine, phantom, rmse, thick_grid

AMPLITUDE_VOX, AMPLITUDE_DEG = 1.5, 3.0


@functools.lru_cache(maxsize=None)
def structured_phantom(shape=(32, 36, 40), blobs=40, seed=7):
    """A head ellipsoid of 300 filled with ``blobs`` Gaussian blobs (sigma 1.5 - 4 voxels, amplitude +-100..400) at random places:
    no symmetry and no periodic detail, so a slice has one pose that fits.  Not negative; read-only."""
    rng = np.random.default_rng(seed)
    x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    c = [(n - 1) / 2.0 for n in shape]
    r = np.sqrt(sum(((x[a] - c[a]) / (0.45 * shape[a])) ** 2 for a in range(3)))
    head = 1.0 / (1.0 + np.exp((r - 1.0) / 0.03))
    v = 300.0 * head
    for _ in range(blobs):
        centre = [rng.uniform(0.15 * n, 0.85 * n) for n in shape]
        sigma, amp = rng.uniform(1.5, 4.0), rng.uniform(100.0, 400.0) * rng.choice([-1.0, 1.0])
        v = v + head * amp * np.exp(-0.5 * sum((x[a] - centre[a]) ** 2 for a in range(3)) / sigma ** 2)
    out = np.maximum(v, 0.0).astype(np.float32)
    out.setflags(write=False)
    return out


def injected_params(slices, voxel, seed, amplitude_vox=AMPLITUDE_VOX, amplitude_deg=AMPLITUDE_DEG):
    """(slices, 6): translations uniform within +-amplitude_vox voxels (of ``voxel`` mm), rotations within +-amplitude_deg."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, (slices, 6))
    p[:, :3] *= amplitude_vox * voxel
    p[:, 3:] *= amplitude_deg
    return p


def moved_stacks(truth, factor, seed=0, noise=0.0, moved=True, affine_out=None):
    """Three stacks of ``truth``, thick along axis 0, 1 and 2 by ``factor``, every slice under a pose of its own ->
    ``(stacks, geometries, affines, params)``; ``moved=False``: all poses zero (the stacks of ``stackutil.orthogonal_stacks``)."""
    affine_out = np.eye(4) if affine_out is None else affine_out
    rng = np.random.default_rng(seed + 1000)
    stacks, geometries, affines, params = [], [], [], []
    for axis in range(3):
        a, shape = thick_grid(truth.shape, axis, factor, affine_out)
        g = S.stack_geometry(a, affine_out, axis, "box", samples=factor)
        p = injected_params(shape[axis], V.in_plane_voxel_size(a, axis), seed + axis) if moved else np.zeros((shape[axis], 6))
        y = V.simulate_stack_slices_np(truth, g, shape, V.slice_geometries(a, affine_out, shape, axis, p)[0])
        if noise:
            y = (y + rng.normal(0.0, noise, shape)).astype(np.float32)
        stacks.append(y)
        geometries.append(g)
        affines.append(a)
        params.append(p)
    return stacks, geometries, affines, params


def rms_corner_displacement(params_a, params_b, affines, shapes, geometries, actives=None):
    """The RMS, over the (active) slices of all stacks, of ``slice_corner_displacement`` between two sets of poses, in mm."""
    d = []
    for k, (pa, pb) in enumerate(zip(params_a, params_b)):
        dk = V.slice_corner_displacement(pa, pb, affines[k], shapes[k], geometries[k].slice_axis)
        d.append(dk if actives is None else dk[np.asarray(actives[k], dtype=bool)])
    d = np.concatenate(d)
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0


def motion_options(affines, affine_out=None, **kw):
    return V.MotionOptions(tuple(affines), np.eye(4) if affine_out is None else affine_out, **kw)


@functools.lru_cache(maxsize=None)
def quality_case(factor, noise=0.0, moved=True, rounds=1, iterations=4, structured=True, limit_mm=10.0, limit_deg=10.0):
    """The specification on the CPU, once per case: the phantom's moved stacks combined without and with motion correction ->
    a dict of the truth-RMSEs and the corner displacements."""
    truth = structured_phantom() if structured else phantom()
    stacks, geometries, affines, params = moved_stacks(truth, factor, seed=0, noise=noise, moved=moved)
    shapes = [y.shape for y in stacks]
    plain = S.combine_stacks_np(stacks, geometries, truth.shape, iterations)
    fixed = S.combine_stacks_np(stacks, geometries, truth.shape, iterations, motion=motion_options(affines, rounds=rounds, limit_mm=limit_mm, limit_deg=limit_deg))
    actives = [m.active for m in fixed.motion_detail]
    zeros = [np.zeros_like(p) for p in params]
    return {"rmse_plain": rmse(plain.volume, truth), "rmse_fixed": rmse(fixed.volume, truth),
            "injected": rms_corner_displacement(params, zeros, affines, shapes, geometries, actives),
            "residual": rms_corner_displacement(fixed.motion, params, affines, shapes, geometries, actives),
            "recovered": rms_corner_displacement(fixed.motion, zeros, affines, shapes, geometries, actives),
            "largest": max(float(np.abs(p[a]).max()) if a.any() else 0.0 for p, a in zip(fixed.motion, actives)),
            "active": [int(a.sum()) for a in actives], "slices": [s[g.slice_axis] for s, g in zip(shapes, geometries)],
            "motion_cost": fixed.motion_cost, "stop": min(lv[-1][2] for lv in (V.default_slice_levels(a, g.slice_axis)
                                                                             for a, g in zip(affines, geometries)))}


# ---------------------------------------------------------------- small stacks with hand-made poses (bit comparisons)

SMALL_OUT = (18, 20, 23)


def small_stack(axis, slices, oblique=False, seed=0):
    """-> ``(y, geometry, affine)``: a random stack with ``slices`` slices along ``axis`` that covers most of the ``SMALL_OUT`` grid
    (identity affine); in-plane extents odd and no multiple of a brick."""
    rng = np.random.default_rng(100 * axis + slices + seed)
    shape = [17, 19, 21]
    shape[axis] = slices
    voxel = [1.0, 1.0, 1.0]
    voxel[axis] = (SMALL_OUT[axis] - 2.0) / slices
    a = oblique_affine(SMALL_OUT, shape, voxel, (6.0, -8.0, 11.0) if oblique else (0.0, 0.0, 0.0), (0.3, -0.2, 0.4))
    g = S.stack_geometry(a, np.eye(4), axis, "box", samples=min(4, max(1, int(round(voxel[axis])))))
    return rng.uniform(0.0, 900.0, shape).astype(np.float32), g, a


def hand_poses(slices, axis, spacing):
    """(slices, 6): poses that open a gap between two slices, overlap two, tilt one and push the last out of the volume."""
    p = np.zeros((slices, 6))
    if slices >= 5:
        p[1, axis] = -0.45 * spacing          # 1 moves away from 2: a gap opens between them
        p[3, axis] = -0.9 * spacing           # 3 lands nearly on 2: they overlap
        p[2, 3:] = (4.0, -3.0, 5.0)           # a tilted slice
        p[2, :3] = (0.7, -0.4, 0.2)
        p[slices - 1, :3] = 500.0             # far outside the output grid
    elif slices == 1:
        p[0] = (0.6, -0.3, 0.4, 3.0, -2.0, 4.0)
    return p
