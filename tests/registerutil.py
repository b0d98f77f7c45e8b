"""The synthetic pair of the registration tests (host and GPU): a blob phantom defined in world coordinates, sampled on two
different grids, the second one moved by a known rigid transform, contrast-inverted through a square root and given noise."""
import functools

import numpy as np

from mri_superresolution_amd import volume_register as G

FIXED_SHAPE, MOVING_SHAPE = (40, 48, 36), (36, 46, 42)
# anisotropic on both sides; the moving grid runs backwards along x
FIXED_AFFINE = np.array([[1.0, 0.0, 0.0, -19.5], [0.0, 0.9, 0.0, -21.0], [0.0, 0.0, 1.25, -22.0], [0.0, 0.0, 0.0, 1.0]])
MOVING_AFFINE = np.array([[-1.2, 0.0, 0.0, 22.0], [0.0, 1.0, 0.0, -23.0], [0.0, 0.0, 1.1, -23.5], [0.0, 0.0, 0.0, 1.0]])
P_TRUE = np.array([2.3, -1.6, 1.2, 4.0, -3.0, 5.0])      # mm, degrees: a few voxels, a few degrees
BINS = 32


def phantom(world):
    """world: (3, ...) mm -> intensities in 0..1: an ellipsoidal head with blobs of several sizes, no symmetry."""
    x, y, z = world
    v = 0.55 * np.exp(-((x / 15.0) ** 4 + (y / 17.0) ** 4 + (z / 16.0) ** 4))
    for cx, cy, cz, s, a in ((6, 4, -3, 5.0, 0.45), (-7, -6, 5, 4.0, 0.35), (2, -9, -8, 3.0, -0.3), (-4, 8, 2, 6.0, 0.25),
                             (9, -2, 7, 2.5, 0.3), (-10, 3, -9, 3.5, -0.25)):
        v = v + a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (2 * s * s))
    return np.clip(v, 0.0, None)


def grid_world(affine, shape):
    idx = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij"))
    return np.tensordot(affine[:3, :3], idx, axes=1) + affine[:3, 3].reshape(3, 1, 1, 1)


def true_world():
    return G.rigid_world(P_TRUE, G.volume_centre(FIXED_AFFINE, FIXED_SHAPE))


@functools.lru_cache(maxsize=None)
def synthetic_pair():
    """-> (fixed, moving) float32.  A point x of the fixed world lies at W x in the moving world, W = true_world()."""
    rng = np.random.default_rng(20240607)
    fixed = 1000.0 * phantom(grid_world(FIXED_AFFINE, FIXED_SHAPE)) + rng.normal(0, 8.0, FIXED_SHAPE)
    inv = np.linalg.inv(true_world())
    w = grid_world(MOVING_AFFINE, MOVING_SHAPE)
    back = np.tensordot(inv[:3, :3], w, axes=1) + inv[:3, 3].reshape(3, 1, 1, 1)
    moving = 800.0 * (1.0 - np.sqrt(phantom(back))) + rng.normal(0, 8.0, MOVING_SHAPE)      # inverted, nonlinear
    fixed, moving = fixed.astype(np.float32), moving.astype(np.float32)
    fixed.setflags(write=False)
    moving.setflags(write=False)
    return fixed, moving


@functools.lru_cache(maxsize=None)
def specification_result():
    """``register_rigid_np`` on the pair: computed once per process, only read."""
    fixed, moving = synthetic_pair()
    return G.register_rigid_np(fixed, FIXED_AFFINE, moving, MOVING_AFFINE, bins=BINS)


def corner_error_voxels(world):
    """The worst corner displacement against the truth, in units of the SMALLEST fixed voxel size."""
    smallest = float(np.linalg.norm(FIXED_AFFINE[:3, :3], axis=0).min())
    return G.corner_displacement(world, true_world(), FIXED_AFFINE, FIXED_SHAPE) / smallest
