"""The numpy specification of the intensity standardisation (mri_superresolution_amd/volume_intensity.py): the landmarks pinned to
scalar np.percentile calls, the properties of the piecewise-linear map, the whole operation on the registration tests' phantom,
and the argument errors.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import registerutil as U                                             # noqa: E402
from test_percentile_host import CLASSES, input_class                # noqa: E402
from mri_superresolution_amd import volume_intensity as I            # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)
SHAPES = [(1, 1, 1), (1, 1, 2), (1, 1, 3), (7, 5, 3), (1, 1, 201), (24, 40, 3), (32, 30, 20)]


def volume(name, shape, seed=0):
    return np.ascontiguousarray(input_class(name, (shape[0] * shape[1], shape[2]), seed).reshape(shape))


def masks(shape, seed=0):
    """name -> mask (or None) of the cases the GPU tests use as well."""
    rng = np.random.default_rng([seed, *shape])
    n = int(np.prod(shape))
    one = np.zeros(n, dtype=np.uint8)
    one[n // 2] = 1
    odd = np.where(rng.random(n) < 0.5, rng.choice(np.array([2, 255], dtype=np.uint8), n), 0).astype(np.uint8)
    return {"none": None, "ones": np.ones(shape, dtype=np.uint8), "half": (rng.random(shape) < 0.5).astype(np.uint8),
            "one_voxel": one.reshape(shape), "values_2_255": odd.reshape(shape)}


def scalar_percentiles(values, percentiles):
    return np.array([np.percentile(values, float(q)) for q in percentiles], dtype=np.float32)


@pytest.mark.parametrize("name", CLASSES)
def test_landmarks_equal_scalar_np_percentile(name):
    for shape in SHAPES:
        v = volume(name, shape)
        for mname, m in masks(shape).items():
            values = v.reshape(-1) if m is None else v[m != 0]
            if values.size == 0:
                continue
            for qs in (I.LANDMARKS, I.RANGE, (0, 100), (0, 0.5, 50, 50, 99.5, 100)):
                got, count = I.landmarks_np(v, m, qs)
                want = scalar_percentiles(values, qs)
                assert np.percentile(values, 50.0).dtype == np.float32
                assert got.dtype == np.float32 and count == values.size
                assert np.array_equal(got, want), (name, shape, mname, qs, got, want)


def test_landmarks_and_window_bounds_are_one_rule():
    """landmarks_np and utils/imageops.percentile_bounds_np state np.percentile's float32 rule through one function: bit-equal to
    each other on every array, and to np.percentile with a scalar q wherever the array is finite (with infinities in it the
    interpolation meets inf - inf).  -0.0 is in the arrays of 2, 3 and 257 elements.  The array of one element holds -3.5: of a
    lone -0.0 the rule gives -0.0 + 0.0 * t = +0.0 at every q, here and in the kernels, where numpy 2.2 returns -0.0 - the one
    divergence, in the sign of a zero, which the last assertion records."""
    from mri_superresolution_amd.utils.imageops import percentile_bounds_np
    pool = np.array([-0.0, -np.inf, np.inf, -3.5, -3.5, 0.0, 2.25, -1e-30, 7.0, 7.0, 7.0, -4096.0, 1.0 + 2.0 ** -23], dtype=np.float32)
    bits = lambda x: np.asarray(x, dtype=np.float32).view(np.uint32)                 # noqa: E731
    for n in (1, 2, 3, 257):
        with_inf = pool[np.arange(n) % pool.size] if n > 1 else pool[3:4].copy()
        with_inf[13:] *= np.float32(0.5) ** (np.arange(13, n) // 13).astype(np.float32)      # 257: the pool at several scales
        finite = np.where(np.isinf(with_inf), np.copysign(np.float32(3e38), with_inf), with_inf)
        for a in (with_inf, finite):
            a = np.random.default_rng(n).permutation(a)
            for q_lo, q_hi in ((0, 100), (0.5, 99.5), (50, 50)):
                with np.errstate(invalid="ignore"):
                    got = I.landmarks_np(a, None, (q_lo, q_hi))[0]
                    bounds = percentile_bounds_np(a, q_lo, q_hi)
                assert got.dtype == bounds.dtype == np.float32
                assert (bits(got) == bits(bounds)).all(), (n, q_lo, q_hi, got, bounds)
                if np.isfinite(a).all():
                    want = [np.percentile(a, float(q_lo)), np.percentile(a, float(q_hi))]
                    assert (bits(got) == bits(want)).all(), (n, q_lo, q_hi, got, want)
    lone = np.array([-0.0], dtype=np.float32)
    assert (bits(I.landmarks_np(lone, None, (0, 100))[0]) == 0).all() and I.landmarks_np(lone, None, (0, 100))[0][0] == np.percentile(lone, 0.0)


def test_landmarks_exclude_nan_and_empty_mask_gives_nan():
    v = volume("normal", (7, 5, 3)).copy()
    v[0, 0, 0] = v[3, 2, 1] = v[6, 4, 2] = np.nan
    for m in masks(v.shape).values():
        keep = ~np.isnan(v) if m is None else (m != 0) & ~np.isnan(v)
        got, count = I.landmarks_np(v, m)
        assert count == int(keep.sum())
        if count:
            assert np.array_equal(got, scalar_percentiles(v[keep], I.LANDMARKS))
    got, count = I.landmarks_np(v, np.zeros(v.shape, dtype=np.uint8))
    assert count == 0 and got.shape == (11,) and got.dtype == np.float32 and np.isnan(got).all()
    got, count = I.landmarks_np(np.full((2, 2, 2), np.nan, dtype=np.float32), None, (50, 60))
    assert count == 0 and np.isnan(got).all()
    # a bool mask is a mask
    m = masks(v.shape)["half"]
    assert np.array_equal(I.landmarks_np(v, m.astype(bool))[0], I.landmarks_np(v, m)[0])


def phantom_landmarks():
    fixed, _ = U.synthetic_pair()
    return I.landmarks_np(fixed, fixed > 100.0)[0]


def samples_around(s, rng, n=4000):
    """Voxels below, on, next to, between and above the landmarks."""
    lo, hi = float(s[0]), float(s[-1])
    span = max(hi - lo, 1.0)
    x = rng.uniform(lo - 0.3 * span, hi + 0.3 * span, n).astype(np.float32)
    near = np.concatenate([s, np.nextafter(s, np.float32(-np.inf)), np.nextafter(s, np.float32(np.inf))]).astype(np.float32)
    return np.concatenate([x, near])


def test_map_sends_landmarks_onto_landmarks_exactly():
    """A voxel on s[i] lies in segment i, where v - s[i] is 0: it maps to d[i] exactly, for every i that HAS a segment
    (i <= L - 2).  The last landmark is clipped into segment L - 2 and maps to d[L-2] + w * ((d[L-1] - d[L-2]) / w): the quotient,
    the product and the sum round once each (half an eps32 relative each, the first two of |D| <= 2 max|d|, the last of about
    |d[L-1]|), 2.5 eps32 max|d| in all; 3 eps32 max|d| is asserted."""
    rng = np.random.default_rng(1)
    for L in (2, 3, 11, 16):
        s = np.sort(rng.uniform(0, 4000, L)).astype(np.float32)
        d = np.sort(rng.uniform(-50, 900, L)).astype(np.float32)
        out = I.piecewise_map_np(s, s, d)
        assert out.dtype == np.float32 and np.array_equal(out[:-1], d[:-1])
        assert abs(float(out[-1]) - float(d[-1])) <= 3 * EPS32 * float(np.abs(d).max())
    # duplicates: a voxel on a repeated landmark takes the LAST of its copies (side="right")
    s = np.array([0, 1, 1, 1, 5], dtype=np.float32)
    d = np.array([10, 20, 30, 40, 50], dtype=np.float32)
    assert np.array_equal(I.piecewise_map_np(s, s, d), np.array([10, 40, 40, 40, 50], dtype=np.float32))      # 40 + 4 * 2.5


def test_map_is_non_decreasing_for_non_decreasing_targets():
    rng = np.random.default_rng(2)
    cases = [(phantom_landmarks(), np.sort(rng.uniform(0, 800, 11)).astype(np.float32))]
    for L in (2, 5, 11, 16):
        cases.append((np.sort(rng.uniform(0, 4000, L)).astype(np.float32), np.sort(rng.uniform(0, 900, L)).astype(np.float32)))
    for s, d in cases:
        x = np.sort(samples_around(s, rng))
        out = I.piecewise_map_np(x, s, d)
        assert (np.diff(out) >= 0).all(), (s, d)


def test_zero_width_segments_give_finite_outputs():
    d = np.array([10, 20, 30, 40, 50], dtype=np.float32)
    x = np.array([-3, 0, 0.5, 1, 2, 4.5, 5, 9], dtype=np.float32)
    for s in ([0, 0, 1, 4, 5], [0, 1, 1, 4, 5], [0, 1, 4, 5, 5], [0, 0, 0, 5, 5], [1, 1], [2, 2, 2]):
        s = np.array(s, dtype=np.float32)
        out = I.piecewise_map_np(x, s, d[:s.size])
        assert out.dtype == np.float32 and np.isfinite(out).all(), (s, out)
    # first segment of zero width: everything below the doubled landmark sits on d[0]
    out = I.piecewise_map_np(x, np.array([0, 0, 1, 4, 5], dtype=np.float32), d)
    assert out[0] == 10 and out[1] == 20 and out[2] == 25


def test_power_of_two_scaling_commutes_with_every_rounding():
    rng = np.random.default_rng(3)
    for s in (phantom_landmarks(), np.sort(rng.uniform(1, 4000, 16)).astype(np.float32), np.array([3, 3, 7, 7, 20], dtype=np.float32)):
        x = samples_around(s, rng)
        a, b = I.piecewise_map_np(np.float32(4) * x, np.float32(4) * s, s), I.piecewise_map_np(x, s, s)
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
        d = np.sort(rng.uniform(0, 900, s.size)).astype(np.float32)
        a, b = I.piecewise_map_np(np.float32(0.25) * x, np.float32(0.25) * s, d), I.piecewise_map_np(x, s, d)
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_identity_map_is_within_two_roundings():
    """out = s[i] + (x - s[i]) * 1 (the slope w / w is exactly 1): two roundings, the difference's and the sum's, of at most half an
    ulp each; the difference may reach 2 M, M = max(|x|, max|s|), so the two errors are below eps32 M and eps32 M / 2."""
    rng = np.random.default_rng(4)
    worst = 0.0
    for s in (phantom_landmarks(), np.sort(rng.uniform(-2000, 4000, 16)).astype(np.float32),
              np.sort(10.0 ** rng.uniform(-3, 6, 11)).astype(np.float32)):
        assert (np.diff(s) > 0).all()
        x = samples_around(s, rng)
        out = I.piecewise_map_np(x, s, s)
        bound = 2 * EPS32 * np.maximum(np.abs(x.astype(np.float64)), float(np.abs(s).max()))
        err = np.abs(out.astype(np.float64) - x.astype(np.float64))
        worst = max(worst, float((err / (bound / 2)).max()))
        assert (err <= bound).all()
    print(f"identity map: worst error {worst:.3f} eps32 of max(|x|, max|s|)")


def distorted_pair():
    """The phantom of the registration tests, its foreground, and the phantom seen through a strictly increasing curve."""
    fixed, _ = U.synthetic_pair()
    mask = (fixed > 100.0).astype(np.uint8)
    x = np.clip(fixed.astype(np.float64), 0.0, None)
    source = (700.0 * (x / float(fixed.max())) ** 0.7 + 0.05 * x + 40.0).astype(np.float32)
    return source, fixed, mask


def test_match_intensity_lowers_the_error_inside_the_mask():
    source, target, mask = distorted_pair()
    out, found = I.match_intensity_np(source, target, mask, mask)
    inside = mask != 0
    before = float(np.abs(source.astype(np.float64) - target)[inside].mean())
    after = float(np.abs(out.astype(np.float64) - target)[inside].mean())
    print(f"mean absolute error inside the mask: {before:.4f} before, {after:.4f} after matching")
    assert after < before
    assert out.dtype == np.float32 and out.shape == source.shape
    assert found.percentiles == tuple(float(q) for q in I.LANDMARKS) and found.source_count == found.target_count == int(inside.sum())
    assert np.array_equal(found.source_landmarks, I.landmarks_np(source, mask)[0])
    assert np.array_equal(found.target_landmarks, I.landmarks_np(target, mask)[0])
    assert np.array_equal(out, I.piecewise_map_np(source, found.source_landmarks, found.target_landmarks))
    # the source's landmarks land on the target's (the last one through the last segment: within its roundings)
    mapped = I.piecewise_map_np(found.source_landmarks, found.source_landmarks, found.target_landmarks)
    assert np.array_equal(mapped[:-1], found.target_landmarks[:-1])
    assert abs(float(mapped[-1]) - float(found.target_landmarks[-1])) <= 3 * EPS32 * float(np.abs(found.target_landmarks).max())
    out2, found2 = I.match_intensity_np(source, target, mask, mask, I.RANGE)
    assert found2.percentiles == (1.0, 99.0) and found2.source_landmarks.shape == (2,)


def test_argument_errors():
    v = volume("normal", (7, 5, 3))
    ok = np.ones(v.shape, dtype=np.uint8)
    for bad in ((50,), (), tuple(range(17)), (10, 5), (-1, 50), (50, 101), (1, float("nan")), (1, float("inf")), "ab", 5):
        with pytest.raises(ValueError):
            I.landmarks_np(v, None, bad)
        with pytest.raises(ValueError):
            I.match_intensity_np(v, v, None, None, bad)
    assert I._check_percentiles((50,), least=1) == (50.0,)
    assert len(I._check_percentiles(tuple(range(16)))) == 16
    for vol in (v.astype(np.float64), np.zeros((0, 3), dtype=np.float32), v.astype(np.int16)):
        with pytest.raises(ValueError):
            I.landmarks_np(vol)
        with pytest.raises(ValueError):
            I.piecewise_map_np(vol, np.float32([0, 1]), np.float32([0, 1]))
        with pytest.raises(ValueError):
            I.match_intensity_np(vol, v)
        with pytest.raises(ValueError):
            I.match_intensity_np(v, vol)
    for m in (ok[:-1], ok.astype(np.int32), ok.astype(np.float32), ok.reshape(-1)):
        with pytest.raises(ValueError):
            I.landmarks_np(v, m)
    for s, d in ((np.float32([0]), np.float32([0])), (np.float32([0, 1]), np.float32([0, 1, 2])), (np.float64([0, 1]), np.float32([0, 1])),
                 (np.float32([[0, 1]]), np.float32([[0, 1]])), (np.zeros(17, np.float32), np.zeros(17, np.float32))):
        with pytest.raises(ValueError):
            I.piecewise_map_np(v, s, d)
    zero = np.zeros(v.shape, dtype=np.uint8)
    with pytest.raises(ValueError, match="no voxels"):
        I.match_intensity_np(v, v, zero, None)
    with pytest.raises(ValueError, match="no voxels"):
        I.match_intensity_np(v, v, None, zero)
    with pytest.raises(ValueError, match="constant foreground"):
        I.match_intensity_np(np.full(v.shape, 3.5, dtype=np.float32), v)
    # the device path has no CPU fallback
    import torch
    t = torch.from_numpy(v)
    for call in (lambda: I.masked_percentiles(t), lambda: I.piecewise_map(t, torch.zeros(2), torch.ones(2)), lambda: I.match_intensity(t, t)):
        with pytest.raises(ValueError, match="MI355X"):
            call()
