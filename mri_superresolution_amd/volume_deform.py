"""Deformable registration of volumes on the device (extension): what is left between two scans of one head
after the best rigid fit - gradient non-linearity, susceptibility / B0 distortion - is non-rigid.  Thirion's demons with an
additive update and a Gaussian ("diffusion-like") regularisation of the field, coarse to fine, with fixed iteration counts and no
line search.  The cost is an intensity difference: standardise the intensities and match the bias first.

A field ``u`` is float32 ``(3, X, Y, Z)`` in voxels of the common grid: ``fixed(x)`` is compared with ``moving(x + u(x))``.

``warp_np``, ``gradient_np``, ``demons_force_np``, ``smooth_field_np``, ``jacobian_stats_np``, ``register_deformable_np``   the
                      specification: float32, every product, sum, difference and division rounded on its own (no fma), the orders
                      written in the docstrings.
``compose_np``, ``demons_update_np``, ``exp_field_np``, ``register_diffeomorphic_np``   the specification of the diffeomorphic
                      variant (Vercauteren): the update is scaled by ``2^-K``, squared ``K`` times into a small diffeomorphism
                      (``compose_np(w, w)``) and COMPOSED with the field, ``u = smooth(compose(u, exp(upd)))``, not added - an additive
                      field may fold, a composition of diffeomorphisms does not (up to the smoothing and the interpolation).
``warp_matrix_np``    one interpolation through a grid matrix and a field: ``moving`` at ``M (x + u(x))``.
``pyramid_shapes``    the shapes of the levels, coarse to fine.
``warp``, ``demons_force``, ``smooth_field``, ``jacobian_stats``, ``register_deformable``   the device path
                      (``csrc/volume_deform.hip``), equal to the specification bit for bit (the float64 sum of squared
                      differences: within one spacing, the same bits on every run).  There is no CPU path: CPU tensors raise.
                      ``register_deformable`` reads the device once, at its end; its iteration loop - four launches per
                      iteration - is HIP-graph capturable with a ``DeformWorkspace`` made before the capture.
``compose``, ``demons_update``, ``exp_field``, ``warp_matrix``, ``register_diffeomorphic``   the device path of the second group, under
                      the same rules; an iteration of ``register_diffeomorphic`` is ``5 + exp_steps`` launches (``DiffeoWorkspace``).

``lcc_force_np``, ``lcc_update_np``   the specification of the force ACROSS CONTRASTS (``force="lcc"`` of the two registrations): the
                      intensity difference means something only between scans of one contrast, and between 64 mT and 3 T one tissue
                      can be brighter than its neighbour in one scan and darker in the other.  Every window of ``(2 r + 1)^3`` voxels
                      gets its own affine relation between the scans - six window sums in float64 in a fixed order, a regression
                      of the warped scan on the fixed one - and only its residual, in units of the fixed scan,
                      ``d = (M - mM) (B / A) - (F - mF)``, drives Thirion's rule, scaled by the squared local correlation
                      ``w = min(A A / (B C), 1)``.  On the phantom of ``tests/deformutil.py`` with the moving scan replaced by
                      ``(900 - 0.7 moving) gain`` (two levels, 15 + 10 iterations, sigma 1.5, r = 2) the end-point error over the
                      true field's RMS is 0.833 with ``"lcc"`` (minimum determinant 0.721) and 1.826 with ``"ssd"``, which moves
                      the field away from the truth; with noise of sigma 10: 0.831 (0.734) and 1.826.
``lcc_force``, ``lcc_update``   their device path (``csrc/volume_lcc.hip``): the warp with a NaN fill, then ONE fused launch, bit for
                      bit; ``force="lcc"`` makes an iteration 5 launches (``6 + exp_steps`` diffeomorphic).  Speed on an MI355X
                      (``tools/lcc_bench.py``, 2026-10-20, 256^3, r = 2, sigma 1.5): 1.04 ms an iteration against 0.55 ms with ``"ssd"`` and
                      12.8 ms with torch operators; the force kernel 0.52 ms, 0.19 of a device copy of its bytes.

Not built: log-domain demons with a stored velocity, an inverse field, affine; for the force: a symmetric force using the gradient of
the moving scan, a mutual-information force, masks in the force, an ``lcc`` radius above 4.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from ._volume_args import check_matrix, check_shape, cuda_tensor, matrix_arg, out_like, three_sigmas, volume_np
from .volume_bias import gaussian_taps
from .volume_eval import downsample2, downsample2_np, upscale2, upscale2_np
from .volume_reslice import sample_np

MAX_RADIUS = 16
DEN_MIN = np.float32(1e-9)                 # MRISR_DEFORM_DEN_MIN: below it a voxel has neither a gradient nor a difference
METHODS = {"linear": L.RESAMPLE_LINEAR, "cubic": L.RESAMPLE_CUBIC}
MIN_EXTENT = 16                            # pyramid_shapes: an extent below this is not halved
DEFAULT_ITERATIONS = (40, 20, 10)          # coarse -> fine
MAX_LCC_RADIUS = 4
FORCES = ("ssd", "lcc")


class DeformResult(NamedTuple):
    field: object          # (3, X, Y, Z) float32
    warped: object         # moving at x + field(x)
    stats: list            # one (sum of d^2, n) row per iteration, coarse level first; force="lcc": (sum of the confidences, n_ok)
    jacobian: tuple        # (minimum determinant of I + grad field, count of determinants <= 0)
    schedule: tuple        # ((shape, iterations), ...) coarse -> fine: the rows of stats belong to the levels in this order


# ---------------------------------------------------------------- numpy specification

def _check_volume_np(v, what):
    return volume_np(v, what, limit=True)


def _check_field_np(u, shape, what):
    u = np.asarray(u)
    if u.dtype != np.float32 or u.shape != (3,) + tuple(shape):
        raise ValueError(f"{what}: the field must be float32 of shape {(3,) + tuple(shape)}, got {u.dtype} {u.shape}")
    return u


def _check_field4_np(u, what):
    u = np.asarray(u)
    if u.dtype != np.float32 or u.ndim != 4 or u.shape[0] != 3 or u.size == 0:
        raise ValueError(f"{what}: expected a non-empty float32 field (3,X,Y,Z), got {u.dtype} {u.shape}")
    check_shape(u.shape[1:], f"{what}: the volume's shape")
    return u


def _check_pair_np(fixed, moving, what):
    fixed, moving = _check_volume_np(fixed, what), _check_volume_np(moving, what)
    if fixed.shape != moving.shape:
        raise ValueError(f"{what}: the scans must share a grid, got shapes {fixed.shape} and {moving.shape}")
    return np.ascontiguousarray(fixed), np.ascontiguousarray(moving)


def _check_method(method):
    if method not in METHODS:
        raise ValueError(f"Unknown interpolation method: {method} (linear or cubic)")
    return method


def _check_max_step(max_step) -> np.float32:
    m = np.float32(max_step)
    if not (np.isfinite(m) and m >= 0):
        raise ValueError(f"max_step must be finite and not negative, got {max_step!r}")
    return m


def _field_coordinates_np(u):
    """The three float64 arrays ``float64(i_a) + float64(u_a)`` of a field ``u`` (3, X, Y, Z): one double addition each."""
    with np.errstate(invalid="ignore"):
        return [np.arange(n, dtype=np.float64).reshape([-1 if a == b else 1 for b in range(3)]) + u[a].astype(np.float64)
                for a, n in enumerate(u.shape[1:])]


def _sample_inside_np(moving, p, shape, method, fill):
    """-> ``(out, inside)``: ``moving`` sampled at the coordinates ``p`` (on a grid of ``shape``) that pass the inside test
    ``-0.5 <= p_a <= n_a - 0.5`` on all three axes of ``moving`` (a NaN fails it), ``fill`` elsewhere."""
    inside = np.ones(shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        for pa, n in zip(p, moving.shape):
            inside &= (pa >= -0.5) & (pa <= n - 0.5)
    out = np.full(shape, np.float32(fill), dtype=np.float32)
    if inside.any():
        with np.errstate(all="ignore"):
            out[inside] = sample_np([moving], [pa[inside] for pa in p], method)[0]
    return out, inside


def _warp_np(moving, u, method, fill):
    return _sample_inside_np(moving, _field_coordinates_np(u), moving.shape, method, fill)


def warp_np(moving, u, method: str = "linear", fill: float = 0.0) -> np.ndarray:
    """``moving`` at ``x + u(x)``, float32.  Coordinate ``p_a = float64(i_a) + float64(u_a)``, one double addition; then
    ``volume_reslice.reslice_np``'s rules: inside test ``-0.5 <= p_a <= n_a - 0.5`` on all axes, outside -> ``fill`` and nothing
    is converted to an integer, ``taps_np``, clamped taps, reduction along z, then y, then x.  A NaN or infinite displacement is
    outside."""
    moving = _check_volume_np(moving, "warp_np")
    u = _check_field_np(u, moving.shape, "warp_np")
    return _warp_np(moving, u, _check_method(method), fill)[0]


def _gradient_axis_np(f, axis):
    n = f.shape[axis]
    g = np.zeros(f.shape, dtype=np.float32)
    if n == 1:
        return g
    m, gm = np.moveaxis(f, axis, 0), np.moveaxis(g, axis, 0)
    with np.errstate(all="ignore"):
        gm[1:-1] = np.float32(0.5) * (m[2:] - m[:-2])
        gm[0] = m[1] - m[0]
        gm[-1] = m[-1] - m[-2]
    return g


def gradient_np(f) -> np.ndarray:
    """float32 ``(3, X, Y, Z)``: along every axis ``0.5 * (f[i + 1] - f[i - 1])`` inside, the one-sided difference
    ``f[1] - f[0]`` / ``f[n - 1] - f[n - 2]`` at the two ends, 0 along an axis of extent 1."""
    f = _check_volume_np(f, "gradient_np")
    return np.stack([_gradient_axis_np(f, a) for a in range(3)])


def _thirion_np(d, g, max_step, keep, weight=None):
    """Thirion's rule -> the three update components: ``den = ((g0 g0 + g1 g1) + g2 g2) + d d``; ``s = d / den`` where
    ``den > DEN_MIN``, else 0; with a ``weight``, ``s = s weight``; ``upd_a = -(s g_a)`` clamped to ``[-max_step, max_step]`` by
    comparisons, 0 outside ``keep`` and where it is not a number.  Every operation float32; call under ``np.errstate``."""
    g2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
    den = g2 + d * d
    has = den > DEN_MIN
    s = np.where(has, d / np.where(has, den, np.float32(1)), np.float32(0)).astype(np.float32)
    if weight is not None:
        s = s * weight
    upd = []
    for a in range(3):
        x = -(s * g[a])
        x = np.where(x > max_step, max_step, np.where(x < -max_step, -max_step, x))
        upd.append(np.where(keep & ~np.isnan(x), x, np.float32(0)).astype(np.float32))
    return upd


def _demons_update_np(fixed, moving, u, max_step, fill, what):
    """-> ``(u, upd, stats)``: the checked field, the three cleaned update components and the (sum of d^2, count) row, as
    ``demons_force_np`` states them."""
    fixed, moving = _check_pair_np(fixed, moving, what)
    u = _check_field_np(u, fixed.shape, what)
    ms = _check_max_step(max_step)
    warped, inside = _warp_np(moving, u, "linear", fill)
    with np.errstate(all="ignore"):
        d = warped - fixed
        upd = _thirion_np(d, gradient_np(fixed), ms, inside)
    keep = inside & np.isfinite(d)
    dd = d[keep].astype(np.float64)
    return u, upd, (math.fsum(dd * dd), int(keep.sum()))


def demons_force_np(fixed, moving, u, max_step: float = 2.0, fill: float = 0.0):
    """-> ``(v, stats)``.  ``d = warp_np(moving, u, "linear", fill) - fixed``; ``g = gradient_np(fixed)``;
    ``g2 = (g0 g0 + g1 g1) + g2 g2``; ``den = g2 + d d``; ``s = d / den`` where ``den > DEN_MIN``, else 0;
    ``upd_a = -(s g_a)``, clamped to ``[-max_step, max_step]`` by comparisons, 0 where the voxel is outside the moving volume or
    ``upd_a`` is not a number; ``v_a = u_a + upd_a``.  ``stats = (S, n)``: over the inside voxels with a finite ``d``, ``n`` their
    count and ``S`` the sum of ``float64(d)^2`` (each square is exact), correctly rounded (``math.fsum``)."""
    u, upd, stats = _demons_update_np(fixed, moving, u, max_step, fill, "demons_force_np")
    v = np.empty_like(u)
    with np.errstate(all="ignore"):
        for a in range(3):
            v[a] = u[a] + upd[a]
    return v, stats


def _check_scale(scale) -> np.float32:
    s = np.float32(scale)
    if not (np.isfinite(s) and s > 0):
        raise ValueError(f"scale must be finite and positive, got {scale!r}")
    return s


def demons_update_np(fixed, moving, u, max_step: float = 2.0, fill: float = 0.0, scale: float = 1.0):
    """-> ``(w, stats)``: ``upd_a`` and ``stats`` exactly as in ``demons_force_np`` (same operations, same order), then
    ``w_a = upd_a * float32(scale)``, one rounded float32 product - exact for the ``2^-K`` the exponential passes - instead of
    ``u_a + upd_a``.  The field ``u`` only says where ``moving`` is read."""
    sc = _check_scale(scale)
    u, upd, stats = _demons_update_np(fixed, moving, u, max_step, fill, "demons_update_np")
    with np.errstate(all="ignore"):
        return np.stack([x * sc for x in upd]), stats


def _check_lcc_radius(radius) -> int:
    if not isinstance(radius, (int, np.integer)) or isinstance(radius, bool) or not 1 <= radius <= MAX_LCC_RADIUS:
        raise ValueError(f"lcc_radius is an integer in 1..{MAX_LCC_RADIUS}, got {radius!r}")
    return int(radius)


def _check_force(force, lcc_radius):
    if force not in FORCES:
        raise ValueError(f"Unknown force: {force!r} (ssd or lcc)")
    return force, _check_lcc_radius(lcc_radius)


def _window_sums_np(c, r):
    """float64 ``(..., X, Y, Z)``: the sums over the cube of ``r`` voxels either side, clipped to the grid: along axis 2, then 1, then
    0, each over ascending index into a sum that starts at ``+0.0`` (a clipped voxel adds ``+0.0``, which changes no bit of it)."""
    for axis in (-1, -2, -3):
        n = c.shape[axis]
        pad = [(0, 0)] * c.ndim
        pad[axis] = (r, r)
        cp = np.pad(c, pad)
        acc = np.zeros(c.shape, dtype=np.float64)
        index = [slice(None)] * c.ndim
        for k in range(2 * r + 1):
            index[axis] = slice(k, k + n)
            acc = acc + cp[tuple(index)]
        c = acc
    return c


def _lcc_update_np(fixed, moving, u, radius, max_step, what):
    """-> ``(u, upd, stats)``: the checked field, the three cleaned update components and the (sum of w, count) row, as
    ``lcc_force_np`` states them."""
    fixed, moving = _check_pair_np(fixed, moving, what)
    u = _check_field_np(u, fixed.shape, what)
    r = _check_lcc_radius(radius)
    ms = _check_max_step(max_step)
    warped = _warp_np(moving, u, "linear", np.nan)[0]
    valid = np.isfinite(warped) & np.isfinite(fixed)
    with np.errstate(all="ignore"):
        F = np.where(valid, fixed, np.float32(0)).astype(np.float64)
        M = np.where(valid, warped, np.float32(0)).astype(np.float64)
        n, sF, sM, sFF, sMM, sFM = _window_sums_np(np.stack([valid.astype(np.float64), F, M, F * F, M * M, F * M]), r)
        mF, mM = sF / n, sM / n
        A = sFM - mM * sF
        B = sFF - mF * sF
        C = sMM - mM * sM
        d64 = (M - mM) * (B / A) - (F - mF)
        q = (A * A) / (B * C)
        w64 = np.where(q > 1.0, 1.0, q)
        ok = valid & (n >= 2) & (B > 0) & (C > 0) & (A != 0) & np.isfinite(d64) & np.isfinite(w64)
        d = np.where(ok, d64, 0.0).astype(np.float32)
        w = np.where(ok, w64, 0.0).astype(np.float32)
        upd = _thirion_np(d, gradient_np(fixed), ms, ok, w)
    return u, upd, (math.fsum(w[ok].astype(np.float64)), int(ok.sum()))


def lcc_force_np(fixed, moving, u, radius: int = 2, max_step: float = 2.0):
    """-> ``(v, stats)``: the force across contrasts, the counterpart of ``demons_force_np``.
    ``warped = warp_np(moving, u, "linear", NaN)``; a voxel is valid where ``warped`` and ``fixed`` are finite (outside the moving
    volume is invalid through the fill).  Channels ``1, F, M, F F, M M, F M`` in float64 (``F = float64(fixed)``,
    ``M = float64(warped)``; the products are exact), ``+0.0`` at an invalid voxel.  Window sums ``n, sF, sM, sFF, sMM, sFM`` over
    the cube of ``radius`` voxels either side, clipped to the grid: along axis 2, then those along axis 1, then those along axis 0,
    each over ascending index into a sum that starts at ``+0.0``, every addition rounded on its own.  In float64, one rounded
    operation each: ``mF = sF / n``, ``mM = sM / n``, ``A = sFM - mM sF``, ``B = sFF - mF sF``, ``C = sMM - mM sM``,
    ``d64 = (M - mM) (B / A) - (F - mF)`` - the residual of the local regression of M on F in units of the fixed scan; a negative
    ``A`` is an inverted contrast and no special case - and ``w64 = (A A) / (B C)``, replaced by 1 where it is above 1: the squared
    local correlation.  ``ok``: valid, ``n >= 2``, ``B > 0``, ``C > 0``, ``A != 0``, ``d64`` and ``w64`` finite.
    ``d = float32(d64)``, ``w = float32(w64)``, both 0 where not ``ok``; then ``demons_force_np``'s rule in float32 with ONE more
    product: ``g = gradient_np(fixed)``, ``den = ((g0 g0 + g1 g1) + g2 g2) + d d``, ``s = d / den`` where ``den > DEN_MIN``, else 0,
    ``s = s w``, ``upd_a = -(s g_a)`` clamped to ``[-max_step, max_step]`` by comparisons, 0 where it is not a number or the voxel is
    not ``ok``; ``v_a = u_a + upd_a``.  ``stats = (S, n_ok)``: the correctly rounded sum (``math.fsum``) of ``float64(w)`` over the
    ``ok`` voxels and their count; ``1 - S / n_ok`` is what the logs print.  ``radius``: an integer 1..4."""
    u, upd, stats = _lcc_update_np(fixed, moving, u, radius, max_step, "lcc_force_np")
    v = np.empty_like(u)
    with np.errstate(all="ignore"):
        for a in range(3):
            v[a] = u[a] + upd[a]
    return v, stats


def lcc_update_np(fixed, moving, u, radius: int = 2, max_step: float = 2.0, scale: float = 1.0):
    """-> ``(w, stats)``: ``upd_a`` and ``stats`` exactly as in ``lcc_force_np``, then ``w_a = upd_a * float32(scale)`` - what
    ``demons_update_np`` is to ``demons_force_np``."""
    sc = _check_scale(scale)
    u, upd, stats = _lcc_update_np(fixed, moving, u, radius, max_step, "lcc_update_np")
    with np.errstate(all="ignore"):
        return np.stack([x * sc for x in upd]), stats


def compose_np(u, v) -> np.ndarray:
    """``v_a + U_a``, float32 ``(3, X, Y, Z)``: ``U_a`` is ``u_a`` interpolated linearly at ``p = float64(i) + float64(v)`` (the coordinate
    of ``warp_np``), so that ``warp(warp(m, u), v)`` samples ``m`` at ``x + compose_np(u, v)(x)``, up to interpolation.  Each ``p_a``
    is clamped into ``[0, n_a - 1]`` by comparisons, ``p < 0 -> 0``, ``p > n_a - 1 -> n_a - 1``: a displacement field continues
    constantly past the faces (a zero fill would pull the field to zero at the border).  Then ``taps_np`` / ``weighted_sum_np``
    along z, then y, then x - the taps once for all three components - and one float32 add.

    An infinite displacement in ``v`` is clamped like any other, onto a face; the sum ``v_a + U_a`` is then infinite in that
    component.  A displacement that is not a number fails both comparisons and stays: such a voxel gets NaN in ALL THREE components
    (where it points is unknown), and nothing of it is converted to an integer."""
    u, v = _check_field4_np(u, "compose_np"), _check_field4_np(v, "compose_np")
    if u.shape != v.shape:
        raise ValueError(f"compose_np: the fields must share a grid, got shapes {u.shape} and {v.shape}")
    with np.errstate(invalid="ignore"):
        p = [np.where(pa < 0.0, 0.0, np.where(pa > n - 1.0, n - 1.0, pa)) for pa, n in zip(_field_coordinates_np(v), u.shape[1:])]
    number = ~(np.isnan(p[0]) | np.isnan(p[1]) | np.isnan(p[2]))
    out = np.full(u.shape, np.float32(np.nan), dtype=np.float32)
    if number.any():
        with np.errstate(all="ignore"):
            for a, ua in enumerate(sample_np(list(u), [pa[number] for pa in p], "linear")):
                out[a][number] = v[a][number] + ua
    return out


MAX_EXP_STEPS = 8


def _check_exp_steps(steps) -> int:
    if not isinstance(steps, (int, np.integer)) or isinstance(steps, bool) or not 0 <= steps <= MAX_EXP_STEPS:
        raise ValueError(f"exp_steps is an integer in 0..{MAX_EXP_STEPS}, got {steps!r}")
    return int(steps)


def exp_field_np(w, steps: int) -> np.ndarray:
    """The exponential of the velocity field ``w`` by scaling and squaring: ``w = w * float32(2^-steps)``, then ``steps`` times
    ``w = compose_np(w, w)``.  ``steps`` in 0..8; 0 returns ``w``."""
    w = _check_field4_np(w, "exp_field_np")
    steps = _check_exp_steps(steps)
    with np.errstate(all="ignore"):
        w = w * np.float32(2.0 ** -steps)
    for _ in range(steps):
        w = compose_np(w, w)
    return w


def warp_matrix_np(moving, m, u, method: str = "linear", fill: float = 0.0) -> np.ndarray:
    """``moving`` (a float32 volume of any shape) at ``M (x + u(x))``, on the grid of the field ``u`` (3, X, Y, Z): ONE interpolation
    through a field and the ``(3, 4)`` float64 matrix ``m``, fixed index -> moving index (the matrix ``reslice`` takes).
    ``q_a = float64(i_a) + float64(u_a)``; ``p_a = ((m[a,0] q_0 + m[a,1] q_1) + m[a,2] q_2) + m[a,3]`` in float64, the order of
    ``source_coordinates_np``; then ``reslice_np``'s inside test (on ``moving``'s extents), taps and reduction.  Bit for bit
    ``reslice_np`` for a zero field and ``warp_np`` for the identity matrix.  A NaN or infinite displacement is outside."""
    moving = _check_volume_np(moving, "warp_matrix_np")
    m = check_matrix(m)
    u = _check_field4_np(u, "warp_matrix_np")
    _check_method(method)
    q = _field_coordinates_np(u)
    with np.errstate(invalid="ignore"):
        p = [((m[a, 0] * q[0] + m[a, 1] * q[1]) + m[a, 2] * q[2]) + m[a, 3] for a in range(3)]
    return _sample_inside_np(moving, p, u.shape[1:], method, fill)[0]


def _check_sigmas(sigmas_vox) -> list:
    s = three_sigmas(sigmas_vox)
    taps = [gaussian_taps(x) for x in s]
    for x, w in zip(s, taps):
        if (w.size - 1) // 2 > MAX_RADIUS:
            raise ValueError(f"sigma {x:g} voxels needs a radius of {(w.size - 1) // 2} taps, at most {MAX_RADIUS} are built for a field")
    return taps


def _pass_np(x, w, axis):
    """One axis of a ``(3, X, Y, Z)`` field (``axis`` 0..2 of the volume): ``acc = 0``, then ``acc = acc + w[k] * x[clamp(i + k - r)]``
    for k ascending - the border replicated."""
    r = (w.size - 1) // 2
    n = x.shape[axis + 1]
    pad = [(0, 0)] * 4
    pad[axis + 1] = (r, r)
    xp = np.pad(x, pad, mode="edge")
    acc = np.zeros(x.shape, dtype=np.float32)
    index = [slice(None)] * 4
    with np.errstate(all="ignore"):
        for k in range(w.size):
            index[axis + 1] = slice(k, k + n)
            acc = acc + w[k] * xp[tuple(index)]
    return acc


def smooth_field_np(v, sigmas_vox) -> np.ndarray:
    """A separable Gaussian of each component of the field ``v`` over axis 2, then 1, then 0 of the volume: taps
    ``volume_bias.gaussian_taps``, added in ascending order to a sum that starts at 0, every product and sum float32; the border is
    replicated (``np.pad(mode="edge")``).  ``ValueError`` for a radius past 16 taps."""
    v = _check_field4_np(v, "smooth_field_np")
    taps = _check_sigmas(sigmas_vox)
    for axis in (2, 1, 0):
        v = _pass_np(v, taps[axis], axis)
    return v


def jacobian_stats_np(u):
    """-> ``(min det, count of det <= 0)`` of ``J = I + grad u``: ``J[a][b] = gradient_np(u_a)[b]``, ``J[a][a] = 1 + J[a][a]``,
    ``det = (J00 (J11 J22 - J12 J21) - J01 (J10 J22 - J12 J20)) + J02 (J10 J21 - J11 J20)`` - the expansion along the first row, every
    operation float32.  A determinant that is not a number enters neither; the minimum of none is +inf; ``-0.0`` is returned as 0."""
    u = _check_field4_np(u, "jacobian_stats_np")
    with np.errstate(all="ignore"):
        J = [list(gradient_np(u[a])) for a in range(3)]
        for a in range(3):
            J[a][a] = np.float32(1) + J[a][a]
        c0 = J[1][1] * J[2][2] - J[1][2] * J[2][1]
        c1 = J[1][0] * J[2][2] - J[1][2] * J[2][0]
        c2 = J[1][0] * J[2][1] - J[1][1] * J[2][0]
        det = (J[0][0] * c0 - J[0][1] * c1) + J[0][2] * c2
        m = np.where(np.isnan(det), np.float32(np.inf), det).min() + np.float32(0)
        return float(m), int((det <= 0).sum())


def pyramid_shapes(shape, levels: int) -> list:
    """The shapes of the levels, coarse to fine: ``shape`` is halved while every extent is even and at least 16, at most
    ``levels - 1`` times."""
    shape = check_shape(shape, "shape")
    if not isinstance(levels, (int, np.integer)) or isinstance(levels, bool) or levels < 1:
        raise ValueError(f"levels is a positive integer, got {levels!r}")
    shapes = [shape]
    while len(shapes) < levels and all(d % 2 == 0 and d >= MIN_EXTENT for d in shapes[0]):
        shapes.insert(0, tuple(d // 2 for d in shapes[0]))
    return shapes


def _schedule(shape, levels, iterations) -> tuple:
    """((shape, iterations), ...) coarse -> fine.  ``iterations``: one count for every level, or ``levels`` counts coarse -> fine, of
    which a shorter pyramid uses the last (finest) ones."""
    shapes = pyramid_shapes(shape, levels)
    if isinstance(iterations, (int, np.integer)) and not isinstance(iterations, bool):
        its = [int(iterations)] * len(shapes)
    else:
        its = [int(i) for i in iterations]
        if len(its) != levels:
            raise ValueError(f"iterations: one count or one per level ({levels}), coarse to fine, got {iterations!r}")
        its = its[len(its) - len(shapes):]
    if any(i < 0 for i in its):
        raise ValueError(f"iterations must not be negative, got {iterations!r}")
    return tuple(zip(shapes, its))


def _register_np(fixed, moving, levels, iterations, sigma_vox, max_step, fill, method, force, lcc_radius, what, step) -> DeformResult:
    """The frame of the two specifications, the counterpart of ``_register``: the checks, the pyramid, the hand-over between levels
    and the final warp around ``step(f, m, u, sigmas) -> (u', stats row)``, one iteration on one level."""
    fixed, moving = _check_pair_np(fixed, moving, what)
    _check_force(force, lcc_radius)
    schedule = _schedule(fixed.shape, levels, iterations)
    sigmas = (float(sigma_vox),) * 3
    _check_sigmas(sigmas), _check_max_step(max_step), _check_method(method)
    pyramid = [(fixed, moving)]
    for _ in schedule[1:]:
        pyramid.insert(0, tuple(downsample2_np(v) for v in pyramid[0]))
    u = np.zeros((3,) + schedule[0][0], dtype=np.float32)
    stats = []
    for level, ((shape, its), (f, m)) in enumerate(zip(schedule, pyramid)):
        if level:
            u = np.stack([upscale2_np(np.ascontiguousarray(u[a]), "linear") * np.float32(2) for a in range(3)])
        for _ in range(its):
            u, row = step(f, m, u, sigmas)
            stats.append(row)
    return DeformResult(u, warp_np(moving, u, method, fill), stats, jacobian_stats_np(u), schedule)


def register_deformable_np(fixed, moving, levels: int = 3, iterations=DEFAULT_ITERATIONS, sigma_vox: float = 1.5, max_step: float = 2.0,
                           fill: float = 0.0, method: str = "linear", force: str = "ssd", lcc_radius: int = 2) -> DeformResult:
    """The specification of ``register_deformable``.  The volumes of a level are repeated ``downsample2_np`` of the scans
    (``pyramid_shapes``); the field starts at zero on the coarsest level; an iteration is
    ``u = smooth_field_np(demons_force_np(fixed_l, moving_l, u, max_step, fill)[0], (sigma_vox,) * 3)`` (sigma in voxels of the level);
    the field goes to the next level as ``upscale2_np(u_a, "linear") * 2`` per component; ``warped = warp_np(moving, field, method,
    fill)`` once at the end.  Identical scans leave the field exactly zero.  ``force="lcc"``: the iteration takes
    ``lcc_force_np(fixed_l, moving_l, u, lcc_radius, max_step)`` instead and the rows of ``stats`` are its ``(S, n_ok)``."""
    def step(f, m, u, sigmas):
        v, row = lcc_force_np(f, m, u, lcc_radius, max_step) if force == "lcc" else demons_force_np(f, m, u, max_step, fill)
        return smooth_field_np(v, sigmas), row

    return _register_np(fixed, moving, levels, iterations, sigma_vox, max_step, fill, method, force, lcc_radius,
                        "register_deformable_np", step)


def register_diffeomorphic_np(fixed, moving, levels: int = 3, iterations=DEFAULT_ITERATIONS, sigma_vox: float = 1.5, max_step: float = 2.0,
                              fill: float = 0.0, method: str = "linear", exp_steps: int = 2, force: str = "ssd",
                              lcc_radius: int = 2) -> DeformResult:
    """The specification of ``register_diffeomorphic``: ``register_deformable_np`` with the iteration
    ``w = demons_update_np(fixed_l, moving_l, u, max_step, fill, 2^-exp_steps)[0]``; ``exp_steps`` times ``w = compose_np(w, w)``;
    ``u = smooth_field_np(compose_np(u, w), (sigma_vox,) * 3)``.  Thirion's update is at most half a voxel, so with the default
    ``exp_steps = 2`` the sub-steps are at most an eighth.  Identical scans leave the field exactly zero.  ``force="lcc"``:
    ``lcc_update_np(fixed_l, moving_l, u, lcc_radius, max_step, 2^-exp_steps)`` instead, rows ``(S, n_ok)``."""
    scale = np.float32(2.0 ** -_check_exp_steps(exp_steps))

    def step(f, m, u, sigmas):
        w, row = lcc_update_np(f, m, u, lcc_radius, max_step, scale) if force == "lcc" else demons_update_np(f, m, u, max_step, fill, scale)
        for _ in range(exp_steps):
            w = compose_np(w, w)
        return smooth_field_np(compose_np(u, w), sigmas), row

    return _register_np(fixed, moving, levels, iterations, sigma_vox, max_step, fill, method, force, lcc_radius,
                        "register_diffeomorphic_np", step)


# ---------------------------------------------------------------- device

def _check_volume(vol, what) -> torch.Tensor:
    return cuda_tensor(vol, (torch.float32,), what, ndim=3, limit=True)


def _check_field(u, shape, device, what) -> torch.Tensor:
    u = cuda_tensor(u, (torch.float32,), what)
    if tuple(u.shape) != (3,) + tuple(shape) or u.device != device:
        raise ValueError(f"{what}: the field must have shape {(3,) + tuple(shape)} on {device}, got {tuple(u.shape)} on {u.device}")
    return u


def _check_field4(u, what) -> torch.Tensor:
    u = cuda_tensor(u, (torch.float32,), what)
    if u.dim() != 4 or u.shape[0] != 3:
        raise ValueError(f"{what}: a field is (3, X, Y, Z), got shape {tuple(u.shape)}")
    check_shape(u.shape[1:], f"{what}: the volume's shape")
    return u


def _check_pair(fixed, moving, what):
    f, m = _check_volume(fixed, what), _check_volume(moving, what)
    if f.shape != m.shape or f.device != m.device:
        raise ValueError(f"{what}: the scans must share a grid and a device, got shapes {tuple(f.shape)} and {tuple(m.shape)}")
    return f, m


def _slots(device) -> torch.Tensor:
    return torch.empty(int(L.load().mrisr_f32_volume_deform_workspace_bytes()) // 8, dtype=torch.int64, device=device)


def warp(moving: torch.Tensor, u: torch.Tensor, method: str = "linear", fill: float = 0.0, out=None) -> torch.Tensor:
    """moving: contiguous float32 CUDA tensor (X, Y, Z); u: (3, X, Y, Z) -> ``warp_np``, bit for bit.  One launch, no device-to-host
    read.  ``out``: another tensor like ``moving``."""
    m = _check_volume(moving, "warp")
    u = _check_field(u, m.shape, m.device, "warp")
    _check_method(method)
    out = out_like(out, m, (m, u), "warp")
    L.call("mrisr_f32_volume_warp", m.data_ptr(), u.data_ptr(), *m.shape, METHODS[method], float(fill), out.data_ptr(), L.stream_ptr(),
           nbytes=20 * m.numel())
    return out


def _force(fixed, moving, u, max_step, fill, v, slots, stats_row):
    L.call("mrisr_f32_volume_demons_force", fixed.data_ptr(), moving.data_ptr(), u.data_ptr(), *fixed.shape, float(max_step), float(fill),
           v.data_ptr(), slots.data_ptr(), L.ptr(stats_row), L.stream_ptr(), nbytes=32 * fixed.numel())      # 5 floats read, 3 written


def _lcc(fixed, moving, u, radius, max_step, scale, update, warped, v, slots, stats_row):
    """Two launches: ``moving`` at ``x + u`` with a NaN fill into ``warped``, then the fused force."""
    L.call("mrisr_f32_volume_warp", moving.data_ptr(), u.data_ptr(), *fixed.shape, METHODS["linear"], float("nan"), warped.data_ptr(),
           L.stream_ptr(), nbytes=20 * fixed.numel())
    L.call("mrisr_f32_volume_lcc_force", fixed.data_ptr(), warped.data_ptr(), u.data_ptr(), *fixed.shape, int(radius), float(max_step),
           float(scale), int(update), v.data_ptr(), slots.data_ptr(), L.ptr(stats_row), L.stream_ptr(),
           nbytes=(20 if update else 32) * fixed.numel())                 # 2 (+ 3) floats read, 3 written


def _smooth_pass(src, dst, shape, axis, taps, radius, slots=None, stats_row=None):
    L.call("mrisr_f32_volume_field_smooth", src.data_ptr(), dst.data_ptr(), *shape, axis, taps.data_ptr(), radius, L.ptr(slots),
           L.ptr(stats_row), L.stream_ptr(), nbytes=24 * int(np.prod(shape)))


def demons_force(fixed: torch.Tensor, moving: torch.Tensor, u: torch.Tensor, max_step: float = 2.0, fill: float = 0.0, out=None):
    """The device path of ``demons_force_np`` -> ``(v, S, n)``: ``v`` bit for bit; ``S`` (0-d float64) within one spacing of the
    specification's sum and the same bits on every run, ``n`` (0-d int64) equal - both stay on the device.  Two launches (the
    force; one wave that adds the fixed slots), no device-to-host read.  ``out``: another tensor like ``u``."""
    f, m = _check_pair(fixed, moving, "demons_force")
    u = _check_field(u, f.shape, f.device, "demons_force")
    _check_max_step(max_step)
    v = out_like(out, u, (u, f, m), "demons_force")
    row = torch.empty(2, dtype=torch.int64, device=f.device)
    _force(f, m, u, max_step, fill, v, _slots(f.device), row)
    return v, row[:1].view(torch.float64)[0], row[1]


def smooth_field(v: torch.Tensor, sigmas_vox, out=None) -> torch.Tensor:
    """v: contiguous float32 CUDA field (3, X, Y, Z) -> ``smooth_field_np``, bit for bit.  Three launches (axis 2, 1, 0), all three
    components in each.  ``out``: another tensor like ``v``."""
    v = _check_field4(v, "smooth_field")
    shape = tuple(v.shape[1:])
    taps = [torch.from_numpy(w).to(v.device) for w in _check_sigmas(sigmas_vox)]
    out = out_like(out, v, (v,), "smooth_field")
    tmp = torch.empty_like(v)
    for src, dst, axis in ((v, out, 2), (out, tmp, 1), (tmp, out, 0)):
        _smooth_pass(src, dst, shape, axis, taps[axis], (taps[axis].numel() - 1) // 2)
    return out


def _jacobian(u, shape, min_det, count, slots):
    L.call("mrisr_f32_volume_jacobian_stats", u.data_ptr(), *shape, min_det.data_ptr(), count.data_ptr(), slots.data_ptr(), L.stream_ptr())


def jacobian_stats(u: torch.Tensor):
    """u: contiguous float32 CUDA field (3, X, Y, Z) -> ``(min det, count of det <= 0)`` of ``jacobian_stats_np`` as a 0-d float32 and a
    0-d int64 tensor on the device.  Two launches, no device-to-host read."""
    u = _check_field4(u, "jacobian_stats")
    shape = tuple(u.shape[1:])
    min_det = torch.empty(1, dtype=torch.float32, device=u.device)
    count = torch.empty(1, dtype=torch.int64, device=u.device)
    _jacobian(u, shape, min_det, count, _slots(u.device))
    return min_det[0], count[0]


class DeformWorkspace:
    """Everything ``register_deformable`` needs besides the two scans, for volumes of ``shape`` and this schedule: the volumes of the
    coarser levels, the two field buffers (every level's field is a view of their beginning), the taps on the device, the fixed slots
    of the sums and the stats buffer - one (double, int64) row per iteration and a last row for the Jacobian numbers.  Made before
    a HIP-graph capture, it serves call after call on one stream.  ``force="lcc"``: also the volume the moving scan is warped into
    before the force, and the key carries the force and its radius (a workspace of the default force compares as it always did)."""

    def __init__(self, shape, device, levels=3, iterations=DEFAULT_ITERATIONS, sigma_vox=1.5, force="ssd", lcc_radius=2):
        self.schedule = _schedule(shape, levels, iterations)
        self.force, self.lcc_radius = _check_force(force, lcc_radius)
        self.force_key = ("lcc", self.lcc_radius) if self.force == "lcc" else ()
        self.key = (tuple(self.schedule), float(sigma_vox)) + self.force_key
        w = _check_sigmas((float(sigma_vox),) * 3)[0]
        self.radius = (w.size - 1) // 2
        self.taps = torch.from_numpy(w).to(device)
        n = int(np.prod(self.schedule[-1][0]))
        self.fields = [torch.empty(3 * n, dtype=torch.float32, device=device) for _ in range(2)]
        self.volumes = [tuple(torch.empty(s, dtype=torch.float32, device=device) for _ in range(2)) for s, _ in self.schedule[:-1]]
        self.rows = sum(its for _, its in self.schedule)
        self.stats = torch.zeros((self.rows + 1, 2), dtype=torch.int64, device=device)
        self.slots = _slots(device)
        self.warped = torch.empty(n, dtype=torch.float32, device=device) if self.force == "lcc" else None

    def field(self, which, level) -> torch.Tensor:
        shape = self.schedule[level][0]
        return self.fields[which][:3 * int(np.prod(shape))].view(3, *shape)

    def scratch(self, level) -> torch.Tensor:
        shape = self.schedule[level][0]
        return self.warped[:int(np.prod(shape))].view(*shape)


def _iterate(ws, level, fixed, moving, iterations, row, max_step, fill):
    """``iterations`` iterations on one level, four launches each: the force (field 0 -> field 1), then the passes over axis 2
    (1 -> 0; its first workgroup adds the force's slots into the stats row), 1 (0 -> 1) and 0 (1 -> 0).  Nothing is allocated.
    A workspace of ``force="lcc"``: five launches, the warp into the scratch volume and the fused force in place of the force."""
    shape = ws.schedule[level][0]
    a, b = ws.field(0, level), ws.field(1, level)
    for it in range(iterations):
        if ws.force == "lcc":
            _lcc(fixed, moving, a, ws.lcc_radius, max_step, 1.0, 0, ws.scratch(level), b, ws.slots, None)
        else:
            _force(fixed, moving, a, max_step, fill, b, ws.slots, None)
        _smooth_pass(b, a, shape, 2, ws.taps, ws.radius, ws.slots, ws.stats[row + it])
        _smooth_pass(a, b, shape, 1, ws.taps, ws.radius)
        _smooth_pass(b, a, shape, 0, ws.taps, ws.radius)


def register_deformable(fixed: torch.Tensor, moving: torch.Tensor, levels: int = 3, iterations=DEFAULT_ITERATIONS, sigma_vox: float = 1.5,
                        max_step: float = 2.0, fill: float = 0.0, method: str = "linear", workspace=None, graph: bool = False,
                        force: str = "ssd", lcc_radius: int = 2) -> DeformResult:
    """The device path of ``register_deformable_np``: ``field`` and ``warped`` (CUDA tensors) bit for bit, ``stats`` and ``jacobian``
    as there (the sums within one spacing).  The pyramid is ``downsample2`` / ``upscale2``; an iteration is four launches; the one
    device-to-host read, of the stats rows and the Jacobian numbers, is the last thing done.  ``graph``: the iteration loop of every
    level is captured into a HIP graph and replayed (after one eager iteration as a warm-up, which loads the code objects) - the
    same bits as the eager loop.  ``force="lcc"``: the force across contrasts (``lcc_force_np``), five launches per iteration, the
    rows of ``stats`` are ``(S, n_ok)``; ``workspace`` must have been made with the same ``force`` and ``lcc_radius``."""
    return _register(fixed, moving, levels, iterations, sigma_vox, max_step, fill, method, workspace, graph, "register_deformable",
                     DeformWorkspace, (), _iterate, force, lcc_radius)


def _register(fixed, moving, levels, iterations, sigma_vox, max_step, fill, method, workspace, graph, what, ws_type, ws_extra, iterate,
              force="ssd", lcc_radius=2):
    """The frame of ``register_deformable`` and ``register_diffeomorphic``: the pyramid, the hand-over between levels, the (captured)
    loop ``iterate`` of every level, the final warp and the one read.  ``ws_type(shape, device, levels, iterations, sigma_vox,
    *ws_extra, force=force, lcc_radius=lcc_radius)`` is the workspace it needs."""
    force, lcc_radius = _check_force(force, lcc_radius)
    force_key = ("lcc", lcc_radius) if force == "lcc" else ()
    f, m = _check_pair(fixed, moving, what)
    _check_max_step(max_step), _check_method(method)
    if workspace is None:
        workspace = ws_type(f.shape, f.device, levels, iterations, sigma_vox, *ws_extra, force=force, lcc_radius=lcc_radius)
    ws = workspace
    if not isinstance(ws, ws_type) or ws.key != (tuple(_schedule(f.shape, levels, iterations)), float(sigma_vox)) + tuple(ws_extra) \
            + force_key or ws.slots.device != f.device:
        raise ValueError(f"{what}: the workspace must be a {ws_type.__name__} for volumes of {tuple(f.shape)}, this schedule, "
                         f"sigma and force on {f.device}")
    pyramid = [(f, m)]
    for pair in reversed(ws.volumes):
        for dst, src in zip(pair, pyramid[0]):
            dst.copy_(downsample2(src))
        pyramid.insert(0, pair)
    ws.field(0, 0).zero_()
    if graph and ws.rows:
        iterate(ws, 0, *pyramid[0], 1, 0, max_step, fill)
        ws.field(0, 0).zero_()
    row = 0
    for level, ((shape, its), (fl, ml)) in enumerate(zip(ws.schedule, pyramid)):
        if level:
            coarse = ws.field(0, level - 1)
            up = [upscale2(coarse[a], "linear") for a in range(3)]      # all three before the finer field overwrites the coarse one
            for a in range(3):
                torch.mul(up[a], 2.0, out=ws.field(0, level)[a])
        if graph and its:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                iterate(ws, level, fl, ml, its, row, max_step, fill)
            g.replay()
        else:
            iterate(ws, level, fl, ml, its, row, max_step, fill)
        row += its
    field = ws.field(0, len(ws.schedule) - 1).clone()
    warped = warp(m, field, method, fill)
    last = ws.stats[ws.rows]
    _jacobian(field, f.shape, last[:1].view(torch.float32), last[1:], ws.slots)
    host = ws.stats.cpu().numpy()                                       # the one device-to-host read
    stats = [(float(s), int(n)) for s, n in zip(host[:ws.rows, 0].copy().view(np.float64), host[:ws.rows, 1])]
    jacobian = (float(host[ws.rows, :1].copy().view(np.float32)[0]), int(host[ws.rows, 1]))
    return DeformResult(field, warped, stats, jacobian, ws.schedule)


# ---------------------------------------------------------------- device: the diffeomorphic variant

def _compose(u, v, out, shape):
    L.call("mrisr_f32_volume_field_compose", u.data_ptr(), v.data_ptr(), *shape, out.data_ptr(), L.stream_ptr(),
           nbytes=36 * int(np.prod(shape)))                                                                   # 6 floats read, 3 written


def _update(fixed, moving, u, max_step, fill, scale, w, slots, stats_row):
    L.call("mrisr_f32_volume_demons_update", fixed.data_ptr(), moving.data_ptr(), u.data_ptr(), *fixed.shape, float(max_step), float(fill),
           float(scale), w.data_ptr(), slots.data_ptr(), L.ptr(stats_row), L.stream_ptr(), nbytes=32 * fixed.numel())


def compose(u: torch.Tensor, v: torch.Tensor, out=None) -> torch.Tensor:
    """u, v: contiguous float32 CUDA fields (3, X, Y, Z) -> ``compose_np(u, v)``, bit for bit.  One launch: the coordinates and the
    eight taps of a voxel once for all three components.  ``u`` and ``v`` may be one tensor (squaring); ``out``: another tensor."""
    u = _check_field4(u, "compose")
    v = _check_field(v, u.shape[1:], u.device, "compose")
    out = out_like(out, u, (u, v), "compose")
    _compose(u, v, out, tuple(u.shape[1:]))
    return out


def demons_update(fixed: torch.Tensor, moving: torch.Tensor, u: torch.Tensor, max_step: float = 2.0, fill: float = 0.0, scale: float = 1.0,
                  out=None):
    """The device path of ``demons_update_np`` -> ``(w, S, n)`` as ``demons_force`` returns them: the same kernel, writing
    ``upd * scale``.  ``out``: another tensor like ``u``."""
    f, m = _check_pair(fixed, moving, "demons_update")
    u = _check_field(u, f.shape, f.device, "demons_update")
    _check_max_step(max_step)
    scale = _check_scale(scale)
    w = out_like(out, u, (u, f, m), "demons_update")
    row = torch.empty(2, dtype=torch.int64, device=f.device)
    _update(f, m, u, max_step, fill, scale, w, _slots(f.device), row)
    return w, row[:1].view(torch.float64)[0], row[1]


def _lcc_entry(what, fixed, moving, u, radius, max_step, scale, update, out):
    f, m = _check_pair(fixed, moving, what)
    u = _check_field(u, f.shape, f.device, what)
    radius = _check_lcc_radius(radius)
    _check_max_step(max_step)
    v = out_like(out, u, (u, f, m), what)
    row = torch.empty(2, dtype=torch.int64, device=f.device)
    _lcc(f, m, u, radius, max_step, scale, update, torch.empty_like(f), v, _slots(f.device), row)
    return v, row[:1].view(torch.float64)[0], row[1]


def lcc_force(fixed: torch.Tensor, moving: torch.Tensor, u: torch.Tensor, radius: int = 2, max_step: float = 2.0, out=None):
    """The device path of ``lcc_force_np`` -> ``(v, S, n)`` as ``demons_force`` returns them: ``v`` bit for bit, ``S`` (0-d float64,
    the sum of the confidences) within one spacing of the specification's and the same bits on every run, ``n`` (0-d int64) equal.
    Three launches (the warp with a NaN fill, the fused force, one wave that adds the slots), no device-to-host read."""
    return _lcc_entry("lcc_force", fixed, moving, u, radius, max_step, 1.0, 0, out)


def lcc_update(fixed: torch.Tensor, moving: torch.Tensor, u: torch.Tensor, radius: int = 2, max_step: float = 2.0, scale: float = 1.0,
               out=None):
    """The device path of ``lcc_update_np`` -> ``(w, S, n)``: the same kernel, writing ``upd * scale``."""
    return _lcc_entry("lcc_update", fixed, moving, u, radius, max_step, _check_scale(scale), 1, out)


def exp_field(w: torch.Tensor, steps: int, out=None) -> torch.Tensor:
    """w: contiguous float32 CUDA field (3, X, Y, Z) -> ``exp_field_np(w, steps)``, bit for bit: the product with ``2^-steps``, then
    ``steps`` launches of ``compose`` between two buffers.  ``steps`` is a host integer: nothing is read from the device."""
    w = _check_field4(w, "exp_field")
    steps = _check_exp_steps(steps)
    out = out_like(out, w, (w,), "exp_field")
    shape = tuple(w.shape[1:])
    other = torch.empty_like(w) if steps else None
    src = out if steps % 2 == 0 else other           # the last of the squarings lands in out
    torch.mul(w, 2.0 ** -steps, out=src)
    for _ in range(steps):
        dst = other if src is out else out
        _compose(src, src, dst, shape)
        src = dst
    return out


def warp_matrix(moving: torch.Tensor, m, u: torch.Tensor, method: str = "linear", fill: float = 0.0, out=None) -> torch.Tensor:
    """moving: contiguous float32 CUDA volume of any shape; m: (3, 4) matrix (host, float64), index on the field's grid -> index in
    ``moving``; u: (3, X, Y, Z) -> ``warp_matrix_np``, bit for bit: the (X, Y, Z) volume ``moving`` at ``M (x + u(x))``, one
    interpolation, one launch, the matrix by value (no upload, no synchronisation)."""
    mv = _check_volume(moving, "warp_matrix")
    u = _check_field4(u, "warp_matrix")
    if u.device != mv.device:
        raise ValueError(f"warp_matrix: the field must lie on {mv.device}, got {u.device}")
    _check_method(method)
    out = out_like(out, u[0], (mv, u), "warp_matrix")
    L.call("mrisr_f32_volume_warp_matrix", mv.data_ptr(), *mv.shape, u.data_ptr(), *u.shape[1:], matrix_arg(m), METHODS[method], float(fill),
           out.data_ptr(), L.stream_ptr(), nbytes=4 * (mv.numel() + 4 * out.numel()))
    return out


class DiffeoWorkspace(DeformWorkspace):
    """``DeformWorkspace`` for ``register_diffeomorphic``: two more field buffers, for the update and its squarings."""

    def __init__(self, shape, device, levels=3, iterations=DEFAULT_ITERATIONS, sigma_vox=1.5, exp_steps=2, force="ssd", lcc_radius=2):
        self.exp_steps = _check_exp_steps(exp_steps)
        super().__init__(shape, device, levels, iterations, sigma_vox, force, lcc_radius)
        self.key = self.key[:2] + (self.exp_steps,) + self.force_key
        self.fields += [torch.empty_like(self.fields[0]) for _ in range(2 if self.exp_steps else 1)]


def _iterate_diffeo(ws, level, fixed, moving, iterations, row, max_step, fill):
    """``iterations`` iterations on one level, ``5 + exp_steps`` launches each: the scaled update (field 0 -> 2), its squarings
    (2 -> 3 -> 2 ...), the composition with the field (0 and the last of those -> 1), then the passes over axis 2 (1 -> 0; its first
    workgroup adds the update's slots into the stats row), 1 (0 -> 1) and 0 (1 -> 0).  Nothing is allocated."""
    shape = ws.schedule[level][0]
    a, b = ws.field(0, level), ws.field(1, level)
    scale = 2.0 ** -ws.exp_steps
    for it in range(iterations):
        w = ws.field(2, level)
        if ws.force == "lcc":
            _lcc(fixed, moving, a, ws.lcc_radius, max_step, scale, 1, ws.scratch(level), w, ws.slots, None)
        else:
            _update(fixed, moving, a, max_step, fill, scale, w, ws.slots, None)
        for _ in range(ws.exp_steps):
            sq = ws.field(3, level) if w.data_ptr() == ws.fields[2].data_ptr() else ws.field(2, level)
            _compose(w, w, sq, shape)
            w = sq
        _compose(a, w, b, shape)
        _smooth_pass(b, a, shape, 2, ws.taps, ws.radius, ws.slots, ws.stats[row + it])
        _smooth_pass(a, b, shape, 1, ws.taps, ws.radius)
        _smooth_pass(b, a, shape, 0, ws.taps, ws.radius)


def register_diffeomorphic(fixed: torch.Tensor, moving: torch.Tensor, levels: int = 3, iterations=DEFAULT_ITERATIONS, sigma_vox: float = 1.5,
                           max_step: float = 2.0, fill: float = 0.0, method: str = "linear", exp_steps: int = 2, workspace=None,
                           graph: bool = False, force: str = "ssd", lcc_radius: int = 2) -> DeformResult:
    """The device path of ``register_diffeomorphic_np``, under the rules of ``register_deformable``: ``field`` and ``warped`` bit for
    bit, the sums within one spacing, one device-to-host read at the end; an iteration is ``5 + exp_steps`` launches; ``graph``
    captures the loop of every level.  ``workspace``: a ``DiffeoWorkspace`` of this schedule, sigma and ``exp_steps``.
    ``force="lcc"``: ``lcc_update_np``'s update, ``6 + exp_steps`` launches per iteration, rows ``(S, n_ok)``."""
    exp_steps = _check_exp_steps(exp_steps)
    return _register(fixed, moving, levels, iterations, sigma_vox, max_step, fill, method, workspace, graph, "register_diffeomorphic",
                     DiffeoWorkspace, (exp_steps,), _iterate_diffeo, force, lcc_radius)
