"""What the edge-sharpness tests share: a phantom of three nested spheres with known labels, blurred by a known Gaussian, and a
brute-force restatement of the profile."""
import functools
import math

import numpy as np

PHANTOM_SHAPE = (40, 44, 48)
PHANTOM_RADII = (18.3, 13.6, 8.4)          # in voxels about the centre: the outer faces of the classes 1..3
PHANTOM_MEANS = (300.0, 600.0, 900.0)      # classes 1..3, the darkest outermost; air is 0
PHANTOM_SIGMAS = (0.0, 0.75, 1.0, 1.5, 2.0)
PHANTOM_NOISE = 30.0


@functools.lru_cache(maxsize=None)
def truth(shape=PHANTOM_SHAPE):
    """uint8 labels, read-only: 0 outside, 1..3 from the outside in."""
    grids = np.meshgrid(*(np.arange(n, dtype=np.float64) - (n - 1) / 2.0 for n in shape), indexing="ij")
    r = np.sqrt(sum(g * g for g in grids))
    labels = np.zeros(shape, dtype=np.uint8)
    for label, radius in enumerate(PHANTOM_RADII, start=1):
        labels[r <= radius] = label
    labels.setflags(write=False)
    return labels


def gaussian_blur(vol, sigma):
    """float64: a separable Gaussian truncated at ``ceil(4 sigma)`` voxels and normalised, the border replicated; sigma 0: a copy."""
    v = np.asarray(vol, dtype=np.float64)
    if sigma == 0:
        return v.copy()
    h = int(math.ceil(4.0 * sigma))
    g = np.exp(-0.5 * (np.arange(-h, h + 1) / float(sigma)) ** 2)
    g /= g.sum()
    for axis in range(3):
        pad = [(0, 0)] * 3
        pad[axis] = (h, h)
        p = np.pad(v, pad, mode="edge")
        n = v.shape[axis]
        out = np.zeros_like(v)
        idx = [slice(None)] * 3
        for t, gt in enumerate(g):
            idx[axis] = slice(t, t + n)
            out += gt * p[tuple(idx)]
        v = out
    return v


@functools.lru_cache(maxsize=None)
def phantom(sigma=0.0, noise=0.0, seed=11, shape=PHANTOM_SHAPE):
    """float32, read-only and cached: the intensities ``PHANTOM_MEANS`` of ``truth(shape)`` blurred by ``gaussian_blur(sigma)``, plus
    Gaussian noise of standard deviation ``noise`` from a fixed seed."""
    clean = np.concatenate([[0.0], PHANTOM_MEANS])[truth(shape)]
    v = gaussian_blur(clean, sigma)
    if noise:
        v = v + np.random.default_rng(seed).normal(0.0, noise, shape)
    v = v.astype(np.float32)
    v.setflags(write=False)
    return v


def brute_profile(vol, sdist, radius, bin_width):
    """The definition of the profile voxel by voxel in Python: -> (count, sum_v, sum_s, sum_vv), (J, nb) each."""
    r32, w32 = np.float32(radius), np.float32(bin_width)
    nb = int(math.ceil(2.0 * float(radius) / float(bin_width)))
    J = sdist.shape[0]
    count = np.zeros((J, nb), dtype=np.int64)
    parts = [[[[] for _ in range(nb)] for _ in range(J)] for _ in range(3)]
    for j in range(J):
        for idx in np.ndindex(*vol.shape):
            s, v = sdist[(j,) + idx], vol[idx]
            if not np.isfinite(s) or not np.isfinite(v):
                continue
            b = math.floor(np.float32(np.float32(s + r32) / w32))
            if 0 <= b < nb:
                count[j, b] += 1
                parts[0][j][b].append(float(v))
                parts[1][j][b].append(float(s))
                parts[2][j][b].append(float(v) * float(v))
    sums = [np.array([[math.fsum(cell) for cell in row] for row in part]) for part in parts]
    return count, sums[0], sums[1], sums[2]
