"""Reslicing between voxel grids (host): exact identities of the specification reslice_np - they catch a matrix used in the wrong
direction -, its consistency with the x2 baselines of volume_eval.py, the grid helpers of utils/nifti.py and the refusals of the
entry points that need no device."""
import itertools
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd import _lib                                      # noqa: E402
from mri_superresolution_amd import volume_reslice as R                       # noqa: E402
from mri_superresolution_amd.utils.nifti import (NiftiHeader, downscaled_affine, grid_matrix, header_for_grid, read_nifti,   # noqa: E402
                                                 respaced_grid, upscaled_affine, write_nifti)
from mri_superresolution_amd.volume_eval import upscale2_np                   # noqa: E402

METHODS = ("nearest", "linear", "cubic")
IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


def values(shape, seed):
    v = np.random.default_rng(seed).uniform(-3000.0, 3000.0, shape)
    v[..., ::2] = np.rint(v[..., ::2])
    # no -0: a zero weight times a finite tap is +-0, and (+0) + (-0) = +0, so an exact gather returns -0 as +0
    return v.astype(np.float32) + np.float32(0)


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("method", METHODS)
def test_identity_returns_the_volume(method):
    v = values((5, 4, 7), 1)
    assert same_bits(R.reslice_np(v, IDENTITY, v.shape, method), v)


@pytest.mark.parametrize("method", METHODS)
def test_permutations_with_flips_are_transposes_and_flips(method):
    """Destination index d -> source index: source axis perm[a] ... the matrix row a picks the destination axis perm[a], reversed
    where flip[a] is set: out[d] = v[s] with s_a = d_perm[a] or n_a - 1 - d_perm[a]."""
    v = values((3, 4, 5), 2)
    for perm in itertools.permutations(range(3)):
        for flips in itertools.product((False, True), repeat=3):
            m = np.zeros((3, 4))
            for a in range(3):
                m[a, perm[a]] = -1.0 if flips[a] else 1.0
                m[a, 3] = v.shape[a] - 1 if flips[a] else 0.0
            w = np.flip(v, [a for a in range(3) if flips[a]])
            # w has the source's axes; destination axis perm[a] runs along source axis a: out = transpose with axes inv(perm)
            inv = [perm.index(b) for b in range(3)]
            want = np.ascontiguousarray(np.transpose(w, inv))
            got = R.reslice_np(v, m, want.shape, method, fill=-7.0)
            assert same_bits(got, want), (perm, flips)


@pytest.mark.parametrize("method", METHODS)
def test_integer_translation_shifts_and_fills(method):
    v = values((4, 5, 6), 3)
    shift = (2, -1, 3)                                            # p = d + shift
    m = np.hstack([np.eye(3), np.array(shift, dtype=np.float64)[:, None]])
    got = R.reslice_np(v, m, v.shape, method, fill=-5.5)
    want = np.full(v.shape, np.float32(-5.5))
    d = np.indices(v.shape)
    s = [d[a] + shift[a] for a in range(3)]
    ok = np.all([(s[a] >= 0) & (s[a] <= v.shape[a] - 1) for a in range(3)], axis=0)      # the inside test at integer p
    want[ok] = v[s[0][ok], s[1][ok], s[2][ok]]
    assert 0 < ok.sum() < ok.size
    assert same_bits(got, want)


def test_linear_reproduces_a_ramp_exactly():
    """v = 3x - 2y + 5z + 7 with a matrix of multiples of 1/4: coordinates, fractions, weights, products and sums are all small
    multiples of 1/16 - exact in float32.  Checked wherever both taps of every axis are unclamped: 0 <= p_a <= n_a - 1."""
    n = (6, 7, 8)
    x, y, z = np.indices(n)
    v = (3 * x - 2 * y + 5 * z + 7).astype(np.float32)
    m = np.array([[0.75, 0.25, 0.0, -0.5], [-0.25, 0.5, 0.25, 1.25], [0.0, -0.5, 0.75, 3.0]])
    shape = (7, 9, 8)
    got = R.reslice_np(v, m, shape, "linear", fill=np.nan)
    p, inside = R.source_coordinates_np(m, shape, n)
    free = inside & np.all([(p[a] >= 0) & (p[a] <= n[a] - 1) for a in range(3)], axis=0)
    assert free.sum() > 50
    want = 3 * p[0] - 2 * p[1] + 5 * p[2] + 7
    assert np.array_equal(got[free].astype(np.float64), want[free])
    assert np.isnan(got[~inside]).all() and not np.isnan(got[inside]).any()


def test_inside_test_is_closed_at_both_ends():
    v = values((3, 2, 2), 4)
    m = np.array([[0.5, 0, 0, -0.5], [0, 1, 0, 0], [0, 0, 1, 0.0]])      # p_x = -0.5, 0, .., 2.5, 3.0
    got = R.reslice_np(v, m, (8, 2, 2), "linear", fill=99.0)
    assert same_bits(got[0], v[0]) and same_bits(got[6], v[2]) and (got[7] == 99.0).all()
    near = R.reslice_np(v, m, (8, 2, 2), "nearest", fill=99.0)
    assert same_bits(near[0], v[0]) and same_bits(near[6], v[2]) and (near[7] == 99.0).all()      # floor(2.5 + 0.5) clipped to 2


def test_cubic_weights():
    w = [R.keys_weight_np(np.float32(x)) for x in (1.0, 0.0, 1.0, 2.0)]
    assert [float(x) for x in w] == [0.0, 1.0, 0.0, 0.0]
    quarter = [float(R.keys_weight_np(np.float32(x))) for x in (1.75, 0.75, 0.25, 1.25)]
    assert quarter == [-0.03515625, 0.26171875, 0.87890625, -0.10546875]          # volume_eval.CUBIC_WEIGHTS


def half_pixel_matrix():
    return np.hstack([0.5 * np.eye(3), np.full((3, 1), -0.25)])


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (6, 5, 4)], ids=str)
def test_half_pixel_matrix_agrees_with_upscale2(shape):
    v = values(shape, 5)
    big = tuple(2 * d for d in shape)
    peak = np.abs(v).max()
    lin = R.reslice_np(v, half_pixel_matrix(), big, "linear", fill=np.nan)
    # both are convex sums of at most 8 values with exact weights: 8 float32 ulps of max|v|
    assert np.abs(lin.astype(np.float64) - upscale2_np(v, "linear")).max() <= 8 * np.spacing(np.float32(peak))
    cub = R.reslice_np(v, half_pixel_matrix(), big, "cubic", fill=np.nan)
    assert np.abs(cub.astype(np.float64) - upscale2_np(v, "cubic")).max() <= 1e-5 * peak


def test_refusals_of_the_specification():
    v = values((2, 2, 2), 6)
    bad = IDENTITY.copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError):
        R.reslice_np(v, bad, (2, 2, 2))
    bad[1, 2] = np.inf
    with pytest.raises(ValueError):
        R.reslice_np(v, bad, (2, 2, 2))
    with pytest.raises(ValueError):
        R.reslice_np(v, IDENTITY, (2, 2, 2), "area")
    with pytest.raises(ValueError):
        R.reslice_np(v, IDENTITY, (2, 0, 2))
    with pytest.raises(ValueError):
        R.reslice_np(v[:0], IDENTITY, (2, 2, 2))
    with pytest.raises(ValueError):
        R.reslice_mask_np(v, IDENTITY, (2, 2, 2))               # float32 is no mask
    mask = (v > 0).astype(np.uint8)
    assert np.array_equal(R.reslice_mask_np(mask, IDENTITY, (2, 2, 2)), mask)
    assert np.array_equal(R.reslice_mask_np(mask, IDENTITY, (3, 2, 2), fill=7)[2], np.full((2, 2), 7, dtype=np.uint8))


# ---------------------------------------------------------------- grid helpers

AFFINE = np.array([[0.9, 0.1, 0.0, -30.0], [-0.1, 1.1, 0.2, 5.0], [0.0, 0.3, 2.0, 7.0], [0.0, 0.0, 0.0, 1.0]])
AXES = [(0, 1), (0, 2), (1, 2), (0, 1, 2)]


@pytest.mark.parametrize("axes", AXES, ids=str)
def test_downscaled_affine_inverts_upscaled_affine(axes):
    assert np.abs(downscaled_affine(upscaled_affine(AFFINE, axes), axes) - AFFINE).max() <= 1e-12
    assert np.abs(upscaled_affine(downscaled_affine(AFFINE, axes), axes) - AFFINE).max() <= 1e-12


@pytest.mark.parametrize("axes", AXES, ids=str)
def test_respaced_grid_at_half_spacing_is_the_upscaled_grid(axes):
    shape = (5, 6, 7)
    spacing = [np.linalg.norm(AFFINE[:3, a]) / 2 if a in axes else (None if a else 0) for a in range(3)]
    aff, new = respaced_grid(AFFINE, shape, spacing)
    assert new == tuple(2 * d if a in axes else d for a, d in enumerate(shape))
    assert np.abs(aff - upscaled_affine(AFFINE, axes)).max() <= 1e-12


def test_respaced_grid_keeps_the_first_corner():
    shape = (11, 13, 9)
    aff, new = respaced_grid(AFFINE, shape, (0.7, 1.3, 0.45))
    corner = np.array([-0.5, -0.5, -0.5, 1.0])
    assert np.abs(aff @ corner - AFFINE @ corner).max() <= 1e-12
    sizes = [np.linalg.norm(AFFINE[:3, a]) for a in range(3)]
    assert new == tuple(int(np.ceil(n * s / w - 1e-6)) for n, s, w in zip(shape, sizes, (0.7, 1.3, 0.45)))
    assert np.allclose([np.linalg.norm(aff[:3, a]) for a in range(3)], (0.7, 1.3, 0.45), rtol=1e-12)
    # the respaced volume is resliced through grid_matrix: a pure scaling about that corner
    m = grid_matrix(AFFINE, aff)
    assert np.abs(m[:, :3] - np.diag([w / s for w, s in zip((0.7, 1.3, 0.45), sizes)])).max() <= 1e-12
    assert np.abs(m @ corner + 0.5).max() <= 1e-12


def test_grid_matrix_maps_destination_to_source_and_refuses_singular_affines():
    dst = upscaled_affine(AFFINE, (0, 1, 2))
    m = grid_matrix(AFFINE, dst)
    assert m.shape == (3, 4) and m.dtype == np.float64
    assert np.abs(m - half_pixel_matrix()).max() <= 1e-12       # NOT the inverse direction (diag 2, offset + 1/2)
    singular = AFFINE.copy()
    singular[:3, 2] = singular[:3, 1]
    with pytest.raises(ValueError):
        grid_matrix(singular, AFFINE)
    with pytest.raises(ValueError):
        grid_matrix(np.diag([1.0, 1.0, 0.0, 1.0]), AFFINE)
    nan = AFFINE.copy()
    nan[0, 0] = np.nan
    with pytest.raises(ValueError):
        grid_matrix(nan, AFFINE)


@pytest.mark.parametrize("endian", ["<", ">"])
def test_header_for_grid_round_trips_through_a_file(tmp_path, endian):
    data = values((4, 5, 3), 7)
    old = NiftiHeader.new((9, 9, 9, 2), (1.0, 1.0, 1.0, 2.5), endian=endian)
    old.set("qform_code", 1)
    old.set("descrip", b"kept")
    hdr = header_for_grid(old, data.shape, AFFINE)
    assert hdr.get("dim")[:5] == [4, 4, 5, 3, 2] and hdr.endian == endian
    assert hdr.get("qform_code") == 0 and hdr.get("sform_code") == 1 and hdr.get("descrip").rstrip(b"\0") == b"kept"
    assert hdr.get("pixdim")[1:5] == pytest.approx([float(np.linalg.norm(AFFINE[:3, a])) for a in range(3)] + [2.5], rel=1e-6)
    assert old.get("dim")[1:4] == [9, 9, 9]                      # a copy
    old.set("sform_code", 2)
    assert header_for_grid(old, data.shape, AFFINE).get("sform_code") == 2
    path = str(tmp_path / "grid.nii.gz")
    both = np.stack([data, data + 1], axis=3)
    write_nifti(path, both, hdr)
    back, got = read_nifti(path)
    assert back.shape == (4, 5, 3, 2) and same_bits(np.ascontiguousarray(back[..., 0]), data)
    assert np.array_equal(got.affine(), AFFINE.astype(np.float32).astype(np.float64))      # srow_* are float32 fields
    hdr3 = header_for_grid(NiftiHeader.new((2, 2, 2)), data.shape, AFFINE)
    write_nifti(path, data, hdr3)
    assert read_nifti(path)[1].shape == data.shape


# ---------------------------------------------------------------- the library's refusals (no launch, no device needed)

def test_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    for name in ("mrisr_f32_volume_reslice", "mrisr_u8_volume_reslice_nearest"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.mrisr_version() == _lib.ABI_VERSION >= 315
    assert _lib.RESAMPLE_NEAREST not in (_lib.RESAMPLE_LINEAR, _lib.RESAMPLE_CUBIC, _lib.RESAMPLE_AREA, _lib.RESAMPLE_LANCZOS4)
    m = (_lib.C.c_double * 12)(*IDENTITY.reshape(-1))
    assert lib.mrisr_f32_volume_reslice(None, 2, 2, 2, None, 2, 2, 2, m, _lib.RESAMPLE_LINEAR, 0.0, None) == -1      # null pointers
    assert lib.mrisr_u8_volume_reslice_nearest(None, 2, 2, 2, None, 2, 2, 2, m, 0, None) == -1
