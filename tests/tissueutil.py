"""What the tissue-classification tests share: a phantom with known labels and small random sweep problems."""
import functools

import numpy as np

PHANTOM_SHAPE = (24, 28, 32)
PHANTOM_MEANS = (300.0, 520.0, 740.0)      # classes 1..3, the darkest outermost; air is 0
PHANTOM_SIGMA = 60.0                       # at this level beta = 0 already scores below beta = 1 on every class
PHANTOM_RADII = (0.92, 0.66, 0.38)         # of the half extents: the outer faces of the three shells


@functools.lru_cache(maxsize=None)
def _phantom(shape, sigma, seed):
    grids = np.meshgrid(*(np.linspace(-1.0, 1.0, n) for n in shape), indexing="ij")
    r = np.sqrt(sum(g * g for g in grids))
    truth = np.zeros(shape, dtype=np.uint8)
    for label, radius in enumerate(PHANTOM_RADII, start=1):
        truth[r <= radius] = label
    clean = np.concatenate([[0.0], PHANTOM_MEANS])[truth]
    noise = np.random.default_rng(seed).normal(0.0, sigma, shape)
    vol = np.where(truth != 0, clean + noise, np.abs(noise) * 0.1).astype(np.float32)
    mask = (truth != 0).astype(np.uint8)
    for a in (vol, truth, mask):
        a.setflags(write=False)
    return vol, mask, truth


def phantom(shape=PHANTOM_SHAPE, sigma=PHANTOM_SIGMA, seed=7):
    """-> (vol float32, mask uint8, truth uint8), read-only and cached: three nested ellipsoidal shells (labels 1..3 from the outside
    in) with the intensities ``PHANTOM_MEANS`` plus Gaussian noise of ``sigma`` from a fixed seed, and faint air outside; the mask is
    the object."""
    return _phantom(tuple(shape), float(sigma), int(seed))


def sweep_problem(shape, K, seed, mask_kind="random"):
    """-> (q uint8, mask uint8, labels uint8 in 1..K inside the mask, cost int32 (K, 256)): a random instance for one sweep."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, shape, dtype=np.uint8)
    if mask_kind == "empty":
        mask = np.zeros(shape, dtype=np.uint8)
    elif mask_kind == "ones":
        mask = np.ones(shape, dtype=np.uint8)
    else:
        mask = (rng.random(shape) < 0.7).astype(np.uint8) * rng.integers(1, 256, shape, dtype=np.uint8)      # holes; any non-zero byte
    labels = np.where(mask != 0, rng.integers(1, K + 1, shape), 0).astype(np.uint8)
    cost = rng.integers(0, 1 << 20, (K, 256)).astype(np.int32)
    cost[rng.integers(0, K), rng.integers(0, 256)] = 1 << 30                                               # the cap appears
    return q, mask, labels, cost


def noisy_volume(shape, seed):
    """A float32 volume with values well outside and exactly on the percentile range, negatives included."""
    rng = np.random.default_rng(seed)
    v = rng.normal(100.0, 60.0, shape).astype(np.float32)
    flat = v.reshape(-1)
    flat[::7] = -flat[::7]
    flat[::11] *= 8.0
    return v
