"""What the denoising tests share: the bit views, a device tensor off a 16-byte boundary, the noisy phantom and an independent
restatement of the filter (a loop over voxels and candidates, every patch distance by the 27-term nested sum)."""
import numpy as np

from mri_superresolution_amd import volume_denoise as D

SHAPE = (32, 32, 32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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


def radius_grid(shape=SHAPE):
    """-> (g, r): the coordinates ``index - 15.5`` per axis (3, ...) and their norm."""
    g = np.indices(shape).astype(np.float64) - 15.5
    return g, np.sqrt((g ** 2).sum(axis=0))


def phantom(shape=SHAPE):
    """The clean volume: 600 inside r < 13, +300 inside r < 8, -200 where |g0| < 2 and r < 13, 0 elsewhere."""
    g, r = radius_grid(shape)
    return (600.0 * (r < 13) + 300.0 * (r < 8) - 200.0 * ((np.abs(g[0]) < 2) & (r < 13))).astype(np.float32)


def rician(clean, sigma, seed=0):
    """``sqrt((clean + N(0, sigma))^2 + N(0, sigma)^2)`` from ``default_rng(seed)``, float32."""
    rng = np.random.default_rng(seed)
    re = clean + rng.normal(0.0, sigma, clean.shape)
    im = rng.normal(0.0, sigma, clean.shape)
    return np.sqrt(re ** 2 + im ** 2).astype(np.float32)


def messy_volume(shape, seed):
    """Positive noise around 200 +- 80 with a few NaN, +-inf, 0.0, -0.0 and negative values planted (as many as the size allows)."""
    rng = np.random.default_rng(seed)
    v = (200.0 + 80.0 * rng.standard_normal(shape)).astype(np.float32)
    flat = v.reshape(-1)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, -35.0, np.nan, -120.5]
    if flat.size >= 4 * len(special):
        where = rng.choice(flat.size, len(special), replace=False)
        flat[where] = np.array(special, dtype=np.float32)
    return v


def denoise_loops(v, inv_h2, two_sigma2, radius, rician_mode):
    """``denoise_np`` restated voxel by voxel and candidate by candidate: the 27 squared differences of a patch pair gathered
    through clamped indices and added as ((sq + sq) + sq) along axis 2, then 1, then 0."""
    f = np.float32
    n = v.shape
    inv_h2, two_sigma2 = f(inv_h2), f(two_sigma2)
    out = np.empty_like(v)
    d3 = np.arange(-1, 2)
    with np.errstate(all="ignore"):
        for p in np.ndindex(*n):
            if not np.isfinite(v[p]):
                out[p] = v[p]
                continue
            num, den, wmax = f(0), f(0), f(0)
            ia = [np.clip(p[a] + d3, 0, n[a] - 1) for a in range(3)]
            pa = v[np.ix_(*ia)]
            for t in D.offsets(radius):
                ib = [np.clip(p[a] + t[a] + d3, 0, n[a] - 1) for a in range(3)]
                diff = pa - v[np.ix_(*ib)]
                sq = diff * diff
                rows = (sq[:, :, 0] + sq[:, :, 1]) + sq[:, :, 2]
                planes = (rows[:, 0] + rows[:, 1]) + rows[:, 2]
                d = (planes[0] + planes[1]) + planes[2]
                x = d * inv_h2
                q = tuple(p[a] + t[a] for a in range(3))
                if not (x < 16 and all(0 <= q[a] < n[a] for a in range(3))):
                    continue
                w = D.WEIGHT_TABLE[int(x * f(256))]
                val = v[q] * v[q] if rician_mode else v[q]
                num, den, wmax = num + w * val, den + w, max(wmax, w)
            wc = wmax if wmax > 0 else f(1)
            val = v[p] * v[p] if rician_mode else v[p]
            m = (num + wc * val) / (den + wc)
            if rician_mode:
                u = m - two_sigma2
                m = np.sqrt(u) if u > 0 else f(0)
            out[p] = m
    return out
