"""Bias-field matching, the specification (no GPU): volume_bias.gaussian_taps, smooth_masked_np against a float64 evaluation of the
same separable sums, the low-pass of a constant, what the two forms achieve on the phantom of tests/biasutil.py, the edge cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import biasutil as B                                             # noqa: E402
from mri_superresolution_amd import volume_bias as V             # noqa: E402
from mri_superresolution_amd.utils.nifti import downscaled_affine      # noqa: E402

EPS = 2.0 ** -24


def test_gaussian_taps():
    for sigma in (0.3, 1.0, 2.5, 4.0, 25.0, 42.6):
        w = V.gaussian_taps(sigma)
        r = int(np.ceil(3 * sigma))
        assert w.dtype == np.float32 and w.shape == (2 * r + 1,)
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= (2 * r + 1) * EPS
        assert np.array_equal(w, w[::-1]) and w[r] == w.max() and (w > 0).all()
        k = np.arange(-r, r + 1, dtype=np.float64)
        e = np.exp(-0.5 * (k / sigma) ** 2)
        assert np.array_equal(w, (e / e.sum()).astype(np.float32))
    assert np.array_equal(V.gaussian_taps(0), np.ones(1, dtype=np.float32))
    assert V.gaussian_taps(128 / 3).size == 257
    for bad in (43.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            V.gaussian_taps(bad)
    assert V.MAX_RADIUS == 128 and V.DEN_MIN == np.float32(1e-3) and V.DEN_MIN.dtype == np.float32


def test_sigmas_for_an_affine():
    affine = np.diag([1.0, 2.0, 0.5, 1.0])
    assert V.sigmas_for(affine, 25.0) == (25.0, 12.5, 50.0)
    rot = np.array([[0.0, -2.0, 0.0, 3.0], [1.5, 0.0, 0.0, -7.0], [0.0, 0.0, 3.0, 1.0], [0, 0, 0, 1]])
    assert np.allclose(V.sigmas_for(rot, 6.0), (4.0, 3.0, 2.0))
    assert np.allclose(V.sigmas_for(downscaled_affine(affine, (0, 1)), 4.0), (2.0, 1.0, 8.0))
    with pytest.raises(ValueError):
        V.sigmas_for(np.eye(3), 1.0)
    with pytest.raises(ValueError):
        V.sigmas_for(np.diag([1.0, 0.0, 1.0, 1.0]), 1.0)


def dense_smooth_f64(x, taps):
    """The same separable sums with float64 products and sums of the float32 taps: the banded matrix of every axis."""
    x = x.astype(np.float64)
    for axis in (2, 1, 0):
        w = taps[axis].astype(np.float64)
        r, n = (w.size - 1) // 2, x.shape[axis]
        m = np.zeros((n, n))
        for i in range(n):
            for k in range(-r, r + 1):
                if 0 <= i + k < n:
                    m[i, i + k] = w[k + r]
        x = np.moveaxis(np.tensordot(m, np.moveaxis(x, axis, 0), axes=(1, 0)), 0, axis)
    return x


@pytest.mark.parametrize("shape,sigmas", [((9, 12, 17), (1.0, 2.0, 1.5)), ((5, 16, 8), (4.0, 0.0, 2.5)), ((6, 7, 40), (0.5, 1.0, 12.0))])
def test_smooth_masked_np_against_float64(shape, sigmas):
    rng = np.random.default_rng(sum(shape))
    vol = rng.uniform(0.0, 1000.0, shape).astype(np.float32)
    vol.reshape(-1)[rng.choice(vol.size, 7, replace=False)] = np.nan
    mask = (rng.random(shape) < 0.7).astype(np.uint8) * rng.choice(np.array([1, 2, 255], dtype=np.uint8), shape)
    num, den = V.smooth_masked_np(vol, mask, sigmas)
    assert num.dtype == den.dtype == np.float32 and num.shape == den.shape == shape
    taps = [V.gaussian_taps(s) for s in sigmas]
    keep = (mask != 0) & ~np.isnan(vol)
    want_num = dense_smooth_f64(np.where(keep, vol, 0), taps)
    want_den = dense_smooth_f64(keep.astype(np.float32), taps)
    # per pass one rounding for the tap weight, one per product and at most T per sum: 3 (T + 2) 2^-24, relative, on non-negative
    # input, when every axis has T taps; with unequal axes the same count is the sum over the axes, which is no larger
    bound = sum(t.size + 2 for t in taps) * EPS
    assert bound <= 3 * (max(t.size for t in taps) + 2) * EPS
    for got, want in ((num, want_num), (den, want_den)):
        assert (np.abs(got.astype(np.float64) - want) <= bound * np.abs(want)).all()
    # a bool mask is the same mask
    num2, den2 = V.smooth_masked_np(vol, mask != 0, sigmas)
    assert B.same_bits(num, num2) and B.same_bits(den, den2)


def test_lowpass_of_a_constant_inside_an_arbitrary_mask():
    shape, sigmas, value = (14, 18, 22), (2.0, 1.5, 2.5), np.float32(812.25)
    rng = np.random.default_rng(3)
    mask = np.zeros(shape, dtype=np.uint8)
    mask[2:9, 3:12, 4:15] = 1
    mask[10:13, 14:17, 17:21] = rng.random((3, 3, 4)) < 0.6
    num, den = V.smooth_masked_np(np.full(shape, value, dtype=np.float32), mask, sigmas)
    low = V.lowpass_np(num, den)
    defined = den >= V.DEN_MIN
    assert defined.any() and (~defined).any()
    assert np.isnan(low[~defined]).all() and not np.isnan(low[defined]).any()
    T = max(V.gaussian_taps(s).size for s in sigmas)
    # the bound of the sums, 3 (T + 2) 2^-24, for their quotient as well
    bound = 3 * (T + 2) * EPS
    assert (np.abs(low[defined].astype(np.float64) - float(value)) <= bound * float(value)).all()
    assert np.array_equal(low[defined], (num[defined] / den[defined]).astype(np.float32))


def test_phantom_pairwise_and_single_scan():
    src, ref, field, sm, rm = B.phantom()
    assert src.shape == B.SHAPE
    inside = (sm != 0) & (rm != 0)
    before = B.relative_rms(src, ref, inside)
    assert 0.10 < before < 0.15
    for sigma in (4.0, 8.0):
        out, est = V.match_bias_np(src, ref, sm, rm, (sigma,) * 3)
        after = B.relative_rms(out, ref, inside)
        print(f"pairwise sigma {sigma}: {before:.4f} -> {after:.4f}")
        assert after < 0.5 * before
        assert np.array_equal(out, src * est)
    only = sm != 0
    cv_before = B.variation(field, only)
    out, est = V.correct_bias_np(src, sm, (6.0,) * 3)
    cv_after = B.variation(field / est, only)
    print(f"single scan sigma 6: {cv_before:.4f} -> {cv_after:.4f}")
    assert cv_after < 0.75 * cv_before
    assert np.array_equal(out, src / est)


def test_edge_cases():
    src, ref, _, sm, rm = B.phantom()
    sig = (2.0, 2.0, 2.0)
    # an all-zero mask: a field of ones, the source bit for bit
    zero = np.zeros_like(sm)
    for out, est in (V.match_bias_np(src, ref, zero, rm, sig), V.match_bias_np(src, ref, sm, zero, sig), V.correct_bias_np(src, zero, sig)):
        assert (est == 1).all() and B.same_bits(out, src)
    # NaN voxels are left out of the smooth and stay NaN
    holes = src.copy()
    where = np.zeros(src.shape, dtype=bool)
    where[20, 24, 10:20] = True
    holes[where] = np.nan
    num, den = V.smooth_masked_np(holes, sm, sig)
    assert not np.isnan(num).any() and not np.isnan(den).any()
    masked_out = sm.copy()
    masked_out[where] = 0
    filled = np.where(where, np.float32(5), src)
    num2, den2 = V.smooth_masked_np(filled, masked_out, sig)
    assert B.same_bits(num, num2) and B.same_bits(den, den2)
    for out, est in (V.match_bias_np(holes, ref, sm, rm, sig), V.correct_bias_np(holes, sm, sig)):
        assert np.isnan(out[where]).all() and not np.isnan(out[~where]).any() and not np.isnan(est).any()
    # limit clamps
    out, est = V.match_bias_np(src, (10 * ref).astype(np.float32), sm, rm, sig, limit=2.0)
    assert est.max() == np.float32(2.0) and est.min() >= np.float32(0.5)
    out, est = V.match_bias_np((10 * src).astype(np.float32), ref, sm, rm, sig, limit=2.0)
    assert est.min() == np.float32(0.5) and est.max() <= np.float32(2.0)
    out, est = V.correct_bias_np(src, sm, sig, limit=1.0)
    assert (est == 1).all() and B.same_bits(out, src)
    # shapes and dtypes
    with pytest.raises(ValueError):
        V.match_bias_np(src, ref[:-1], sm, rm[:-1], sig)
    with pytest.raises(ValueError):
        V.match_bias_np(src, ref, sm[:-1], rm, sig)
    with pytest.raises(ValueError):
        V.match_bias_np(src.astype(np.float64), ref, sm, rm, sig)
    with pytest.raises(ValueError):
        V.correct_bias_np(src, sm.astype(np.int32), sig)
    with pytest.raises(ValueError):
        V.correct_bias_np(src[0], sm[0], sig)
    with pytest.raises(ValueError):
        V.correct_bias_np(src, sm, (2.0, 2.0))
    with pytest.raises(ValueError):
        V.correct_bias_np(src, sm, sig, limit=0.5)
    with pytest.raises(ValueError):
        V.smooth_masked_np(src, sm, (50.0, 1.0, 1.0))


def test_device_functions_refuse_cpu_tensors():
    import torch
    src, ref, _, sm, rm = B.phantom()
    s, r, a, b = (torch.from_numpy(x) for x in (src, ref, sm, rm))
    with pytest.raises(ValueError, match="no CPU fallback"):
        V.smooth_masked(s, a, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="no CPU fallback"):
        V.match_bias(s, r, a, b, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="no CPU fallback"):
        V.correct_bias(s, a, (1.0, 1.0, 1.0))


def test_library_declares_the_entry_points():
    from mri_superresolution_amd import _lib
    lib = _lib.load()
    for name in ("mrisr_f32_volume_smooth_masked", "mrisr_f32_volume_bias_apply"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.mrisr_version() == _lib.ABI_VERSION >= 319
    assert (_lib.BIAS_PAIR, _lib.BIAS_HUM, _lib.BIAS_LOWPASS) == (V.MODE_PAIR, V.MODE_HUM, V.MODE_LOWPASS)
