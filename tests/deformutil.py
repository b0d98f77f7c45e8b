"""Helpers shared by the deformable-registration tests: the bit comparison, tensors at chosen alignments, messy volumes and fields,
and the phantom of the quality test with its true field."""
import functools

import numpy as np

PHANTOM_SHAPE = (24, 28, 32)
AMPLITUDE = 1.5          # voxels: the amplitude of the phantom's true field


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    """Equal uint32 views wherever there is a number, NaNs in the same places (a NaN's sign and payload are nobody's rule)."""
    if not (a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))):
        return False
    number = ~np.isnan(a)
    return np.array_equal(bits(a)[number], bits(b)[number])


def on_device(a, offset=0):
    """``a`` as a CUDA tensor whose base pointer lies ``offset`` floats past a 16-byte boundary."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 8, dtype=torch.float32, device="cuda")
    shift = (-(buf.data_ptr() // 4) % 4 + offset) % 4
    t = buf[shift:shift + a.size].view(a.shape)
    assert (t.data_ptr() // 4) % 4 == offset % 4
    t.copy_(torch.from_numpy(a))
    return t


def messy_volume(shape, seed, specials=True):
    """Intensities of mixed sign and magnitude; with ``specials`` a few NaN, +-inf and huge voxels."""
    rng = np.random.default_rng(seed)
    v = (rng.normal(0, 300, shape) * rng.choice([1e-3, 1.0, 1.0, 40.0], shape)).astype(np.float32)
    if specials and v.size >= 8:
        flat = v.reshape(-1)
        at = rng.choice(v.size, size=min(5, v.size // 4), replace=False)
        flat[at] = np.array([np.nan, np.inf, -np.inf, 1e30, -0.0], dtype=np.float32)[:at.size]
    return v


def messy_field(shape, seed):
    """(3,) + shape: integers (t = 0), displacements that land exactly on -0.5 and n - 0.5, ones that push outside, NaN, +-inf, 1e9
    and ordinary fractions, mixed voxel by voxel."""
    rng = np.random.default_rng(seed)
    u = np.empty((3,) + tuple(shape), dtype=np.float32)
    for a, n in enumerate(shape):
        i = np.arange(n, dtype=np.float64).reshape([-1 if a == b else 1 for b in range(3)]) + np.zeros(shape)
        kind = rng.integers(0, 10, shape)
        frac = rng.uniform(-2.5, 2.5, shape)
        whole = rng.integers(-2, 3, shape).astype(np.float64)
        ua = np.where(kind < 5, frac, whole)
        ua = np.where(kind == 6, -0.5 - i, ua)                 # p = -0.5 exactly: inside
        ua = np.where(kind == 7, n - 0.5 - i, ua)              # p = n - 0.5 exactly: inside
        ua = np.where(kind == 8, rng.choice([-1.0, 1.0], shape) * (n + rng.uniform(0, 3, shape)), ua)      # outside
        ua = ua.astype(np.float32)
        special = rng.random(shape) < 0.03
        ua[special] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e9, -1e9], dtype=np.float32), int(special.sum()))
        u[a] = ua
    return u


def smooth_field(shape, seed, amplitude=1.2):
    """An ordinary field: low-frequency sines of ``amplitude`` voxels."""
    rng = np.random.default_rng(seed)
    x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    u = [amplitude * np.sin(2 * np.pi * (x[(a + 1) % 3] / max(shape[(a + 1) % 3], 2) + rng.random())) *
         np.cos(np.pi * x[(a + 2) % 3] / max(shape[(a + 2) % 3], 2)) for a in range(3)]
    return np.stack(u).astype(np.float32)


def _phantom_at(x, y, z, shape):
    """The continuous phantom at the float64 coordinates: a smooth-edged ellipsoid with five Gaussian blobs."""
    c = [(n - 1) / 2.0 for n in shape]
    r = np.sqrt(((x - c[0]) / (0.40 * shape[0])) ** 2 + ((y - c[1]) / (0.40 * shape[1])) ** 2 + ((z - c[2]) / (0.40 * shape[2])) ** 2)
    body = 600.0 / (1.0 + np.exp((r - 1.0) / 0.08))
    blobs = [((-0.35, 0.10, 0.05), 3.0, 300.0), ((0.30, -0.25, 0.20), 2.5, -250.0), ((0.05, 0.30, -0.35), 3.5, 200.0),
             ((0.00, 0.00, 0.00), 4.0, 250.0), ((0.25, 0.25, 0.30), 2.0, -200.0)]
    for (o, s, amp) in blobs:
        q = [c[a] + o[a] * 0.8 * shape[a] / 2 for a in range(3)]
        body = body + amp * np.exp(-((x - q[0]) ** 2 + (y - q[1]) ** 2 + (z - q[2]) ** 2) / (2 * s * s)) / (1.0 + np.exp((r - 1.0) / 0.08))
    return body


@functools.lru_cache(maxsize=None)
def phantom(noise=0.0, seed=0, shape=PHANTOM_SHAPE):
    """-> (fixed, moving, true field, object mask) on ``shape``: ``moving`` is the phantom, ``fixed(x)`` the phantom at
    ``x + u(x)`` with ``u`` a sinusoidal field of ``AMPLITUDE`` voxels - evaluated analytically, so ``u`` is the true field.  The
    arrays are shared between tests: do not write to them."""
    x, y, z = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    u = np.stack([AMPLITUDE * np.sin(2 * np.pi * y / shape[1]) * np.cos(np.pi * z / shape[2]),
                  AMPLITUDE * np.sin(2 * np.pi * z / shape[2] + 0.5) * np.cos(np.pi * x / shape[0]),
                  AMPLITUDE * np.sin(2 * np.pi * x / shape[0] + 1.0) * np.cos(np.pi * y / shape[1])])
    moving = _phantom_at(x, y, z, shape)
    fixed = _phantom_at(x + u[0], y + u[1], z + u[2], shape)
    if noise:
        rng = np.random.default_rng(seed)
        moving = moving + rng.normal(0, noise, shape)
        fixed = fixed + rng.normal(0, noise, shape)
    mask = _phantom_at(x, y, z, shape) > 100.0
    out = (fixed.astype(np.float32), moving.astype(np.float32), u.astype(np.float32), mask)
    for a in out:
        a.setflags(write=False)
    return out


def quality(fixed, moving, truth, mask, result):
    """-> (RMS intensity difference inside the object after / before, RMS end-point error / RMS of the true field, both inside the
    object, minimum Jacobian determinant)."""
    before = np.sqrt(np.mean((moving.astype(np.float64) - fixed)[mask] ** 2))
    after = np.sqrt(np.mean((np.asarray(result.warped, dtype=np.float64) - fixed)[mask] ** 2))
    err = np.sqrt(np.mean(np.sum((np.asarray(result.field, dtype=np.float64) - truth) ** 2, axis=0)[mask]))
    ref = np.sqrt(np.mean(np.sum(truth.astype(np.float64) ** 2, axis=0)[mask]))
    return after / before, err / ref, result.jacobian[0]
