"""The far pair of the global-start registration tests (host and GPU): the phantom of tests/registerutil.py on two grids whose world
origins differ by centimetres, the second one turned by 24 / -19 / 27 degrees - the worst corner starts 39.7 voxels off under the
headers.  No air-and-noise background beyond the phantom's own: the Otsu masks cover 24.6 % and 20.9 % of the two volumes."""
import functools

import numpy as np

import registerutil as U
from mri_superresolution_amd import volume_register as G
from mri_superresolution_amd.volume_eval import foreground_mask_np

FIXED_SHAPE, MOVING_SHAPE = (40, 48, 36), (52, 56, 50)
FIXED_AFFINE = U.FIXED_AFFINE
MOVING_AFFINE = np.array([[-1.2, 0.0, 0.0, 31.0], [0.0, 1.0, 0.0, -28.0], [0.0, 0.0, 1.1, -27.0], [0.0, 0.0, 0.0, 1.0]])
P_FAR = np.array([13.0, -9.0, 8.0, 24.0, -19.0, 27.0])      # mm, degrees
BINS = 32


def true_world():
    return G.rigid_world(P_FAR, G.volume_centre(FIXED_AFFINE, FIXED_SHAPE))


@functools.lru_cache(maxsize=None)
def far_pair():
    """-> (fixed, moving) float32, read-only.  A point x of the fixed world lies at W x in the moving world, W = true_world()."""
    rng = np.random.default_rng(7)
    fixed = 1000.0 * U.phantom(U.grid_world(FIXED_AFFINE, FIXED_SHAPE)) + rng.normal(0, 8.0, FIXED_SHAPE)
    inv = np.linalg.inv(true_world())
    w = U.grid_world(MOVING_AFFINE, MOVING_SHAPE)
    back = np.tensordot(inv[:3, :3], w, axes=1) + inv[:3, 3].reshape(3, 1, 1, 1)
    moving = 800.0 * np.sqrt(U.phantom(back)) + rng.normal(0, 8.0, MOVING_SHAPE)
    fixed, moving = fixed.astype(np.float32), moving.astype(np.float32)
    fixed.setflags(write=False)
    moving.setflags(write=False)
    return fixed, moving


@functools.lru_cache(maxsize=None)
def far_masks():
    """The Otsu masks of the pair (``foreground_mask_np``, no closing), read-only."""
    masks = tuple(foreground_mask_np(v) for v in far_pair())
    for m in masks:
        m.setflags(write=False)
    return masks


@functools.lru_cache(maxsize=None)
def specification_result(init, mask_cost):
    """``register_rigid_np`` on the far pair: computed once per process and setting, only read."""
    fixed, moving = far_pair()
    fmask, mmask = far_masks()
    return G.register_rigid_np(fixed, FIXED_AFFINE, moving, MOVING_AFFINE, bins=BINS, fixed_mask=fmask, moving_mask=mmask,
                               mask_cost=mask_cost, init=init)


def corner_error_voxels(world):
    """The worst corner displacement against the truth, in units of the SMALLEST fixed voxel size."""
    smallest = float(np.linalg.norm(FIXED_AFFINE[:3, :3], axis=0).min())
    return G.corner_displacement(world, true_world(), FIXED_AFFINE, FIXED_SHAPE) / smallest
