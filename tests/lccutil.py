"""Helpers of the tests of the force across contrasts: the other-contrast moving scan of the phantom, an independent slow
restatement of the specification and the registrations shared between the tests."""
import functools
import math

import numpy as np

import deformutil as du

SCHEDULE = dict(levels=2, iterations=(15, 10), sigma_vox=1.5)


def other_contrast(moving):
    """``(900 - 0.7 moving) gain``, ``gain = 1 + 0.35 x0 - 0.25 x1 x2`` with ``x_a = linspace(-1, 1, n_a)``: an inverted contrast
    under a smooth gain, float32."""
    x = [np.linspace(-1.0, 1.0, n).reshape([-1 if a == b else 1 for b in range(3)]) for a, n in enumerate(moving.shape)]
    gain = 1.0 + 0.35 * x[0] - 0.25 * x[1] * x[2]
    return ((900.0 - 0.7 * moving.astype(np.float64)) * gain).astype(np.float32)


@functools.lru_cache(maxsize=None)
def contrast_phantom(noise=0.0):
    """-> (fixed, moving of the other contrast, true field, object mask); shared between tests: do not write to them."""
    fixed, moving, truth, mask = du.phantom(noise)
    other = other_contrast(moving)
    other.setflags(write=False)
    return fixed, other, truth, mask


@functools.lru_cache(maxsize=None)
def reference(kind, force, noise=0.0):
    """The specification's registration of the contrast phantom, computed once: ``kind`` is "deformable" or "diffeomorphic"."""
    from mri_superresolution_amd import volume_deform as vd
    fixed, moving = contrast_phantom(noise)[:2]
    fn = vd.register_deformable_np if kind == "deformable" else vd.register_diffeomorphic_np
    return fn(fixed, moving, force=force, lcc_radius=2, **SCHEDULE)


def slow_lcc_force(fixed, moving, u, radius, max_step=2.0, den_min=np.float32(1e-9)):
    """``lcc_force_np`` restated voxel by voxel: explicit loops over the window in the stated order, scalar float64 / float32
    arithmetic.  Only ``warp_np`` and ``gradient_np`` are taken from the package (they have tests of their own)."""
    from mri_superresolution_amd import volume_deform as vd
    X, Y, Z = fixed.shape
    r = radius
    warped = vd.warp_np(moving, u, "linear", np.nan)
    g = vd.gradient_np(fixed)
    valid = np.isfinite(warped) & np.isfinite(fixed)
    chan = np.zeros((6, X, Y, Z), dtype=np.float64)
    for i, j, k in np.ndindex(X, Y, Z):
        if valid[i, j, k]:
            F, M = np.float64(fixed[i, j, k]), np.float64(warped[i, j, k])
            chan[:, i, j, k] = (1.0, F, M, F * F, M * M, F * M)
    s2 = np.zeros_like(chan)
    s1 = np.zeros_like(chan)
    s0 = np.zeros_like(chan)
    for c in range(6):
        for i, j, k in np.ndindex(X, Y, Z):
            acc = np.float64(0.0)
            for kk in range(max(k - r, 0), min(k + r, Z - 1) + 1):
                acc = acc + chan[c, i, j, kk]
            s2[c, i, j, k] = acc
        for i, j, k in np.ndindex(X, Y, Z):
            acc = np.float64(0.0)
            for jj in range(max(j - r, 0), min(j + r, Y - 1) + 1):
                acc = acc + s2[c, i, jj, k]
            s1[c, i, j, k] = acc
        for i, j, k in np.ndindex(X, Y, Z):
            acc = np.float64(0.0)
            for ii in range(max(i - r, 0), min(i + r, X - 1) + 1):
                acc = acc + s1[c, ii, j, k]
            s0[c, i, j, k] = acc
    with np.errstate(all="ignore"):
        v = u + np.float32(0)                       # where nothing is added the specification still adds +0.0
    ms = np.float32(max_step)
    weights = []
    with np.errstate(all="ignore"):
        for i, j, k in np.ndindex(X, Y, Z):
            n, sF, sM, sFF, sMM, sFM = s0[:, i, j, k]
            if not valid[i, j, k] or n < 2:
                continue
            F, M = np.float64(fixed[i, j, k]), np.float64(warped[i, j, k])
            mF, mM = sF / n, sM / n
            A = sFM - mM * sF
            B = sFF - mF * sF
            C = sMM - mM * sM
            if not (B > 0 and C > 0 and A != 0):
                continue
            d64 = (M - mM) * (B / A) - (F - mF)
            w64 = (A * A) / (B * C)
            if w64 > 1.0:
                w64 = np.float64(1.0)
            if not (np.isfinite(d64) and np.isfinite(w64)):
                continue
            d, w = np.float32(d64), np.float32(w64)
            weights.append(float(w))
            ga = [g[a][i, j, k] for a in range(3)]
            g2 = (ga[0] * ga[0] + ga[1] * ga[1]) + ga[2] * ga[2]
            den = g2 + d * d
            s = d / den if den > den_min else np.float32(0)
            s = s * w
            for a in range(3):
                x = -(s * ga[a])
                x = ms if x > ms else (-ms if x < -ms else x)
                if not np.isnan(x):
                    v[a][i, j, k] = u[a][i, j, k] + np.float32(x)
    return v, (math.fsum(weights), len(weights))
