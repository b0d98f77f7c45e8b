"""CPU-only tests of the surface distances (mri_superresolution_amd/volume_surface.py, numpy part): the distance transform against
brute force, the boundary on hand-made cases, the three distances on shifted boxes, the argument checks of both paths and of the C
entries."""
import math

import numpy as np
import pytest

from mri_superresolution_amd import volume_surface as S


def _random_sites(shape, seed, density=0.1):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _pairs(shape, sites):
    """-> (voxel coordinates (N, 1, 3), site coordinates (1, M, 3)) as int64."""
    grid = np.stack(np.meshgrid(*(np.arange(n) for n in shape), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    return grid[:, None, :], grid[sites.reshape(-1) != 0][None, :, :]


# ---------------------------------------------------------------- edt_sq_np

def test_unit_weights_equal_the_integer_brute_force():
    shape = (5, 6, 7)
    sites = _random_sites(shape, 1)
    v, s = _pairs(shape, sites)
    want = ((v - s) ** 2).sum(axis=2).min(axis=1).reshape(shape)
    got = S.edt_sq_np(sites)
    assert got.dtype == np.float32 and got.shape == shape
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))


def test_anisotropic_weights_stay_within_three_roundings_of_float64():
    shape = (5, 6, 7)
    sites = _random_sites(shape, 2)
    w = tuple(np.float32(x) for x in (0.64, 1.0, 6.25))
    v, s = _pairs(shape, sites)
    want = (((v - s) ** 2).astype(np.float64) * np.array([float(x) for x in w])).sum(axis=2).min(axis=1).reshape(shape)
    got = S.edt_sq_np(sites, 0, w).astype(np.float64)
    # every term passes through at most three roundings (its product, two sums) and all terms are non-negative
    assert (np.abs(got - want) <= 4.0 * 2.0 ** -24 * want).all()
    assert (got != want).any()                                           # the roundings are there: 0.64 is not a float32


def test_no_site_all_sites_one_corner_and_value():
    shape = (3, 4, 5)
    assert np.isposinf(S.edt_sq_np(np.zeros(shape, np.uint8))).all()
    assert not S.edt_sq_np(np.ones(shape, np.uint8)).any()
    corner = np.zeros(shape, np.uint8)
    corner[2, 0, 4] = 7
    i, j, k = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    want = ((i - 2) ** 2 + j ** 2 + (k - 4) ** 2).astype(np.float32)
    assert np.array_equal(S.edt_sq_np(corner), want)                     # value 0: any non-zero byte is a site
    assert np.array_equal(S.edt_sq_np(corner, 7), want)
    assert np.isposinf(S.edt_sq_np(corner, 3)).all()
    assert np.array_equal(S.edt_sq_np(corner, 7, (4, 1, 0.25)), (4 * (i - 2) ** 2 + j ** 2 + 0.25 * (k - 4) ** 2).astype(np.float32))
    table = S.distance_table_np(5, np.float32(0.64))
    assert table.dtype == np.float32 and table.tolist() == [float(np.float32(0.64) * np.float32(d * d)) for d in range(5)]


# ---------------------------------------------------------------- boundary_np

def test_boundary_volume_face_both_modes_and_a_sheet():
    full = np.full((3, 3, 3), 2, dtype=np.uint8)
    out = S.boundary_np(full)
    assert out[1, 1, 1] == 0 and out.sum() == 2 * 26                     # the faces of the volume count as background
    assert not S.boundary_np(full, background=False).any()               # no other tissue anywhere
    two = np.zeros((4, 4, 6), dtype=np.uint8)
    two[:, :, 1:3], two[:, :, 3:5] = 1, 2                                # air, two slabs, air along axis 2
    inter = S.boundary_np(two, background=False)
    assert (inter[:, :, 2] == 1).all() and (inter[:, :, 3] == 2).all() and inter.sum() == 16 * 3
    assert np.array_equal(S.boundary_np(two), two)                       # every voxel touches the rim, air or the other slab
    deep = np.zeros((5, 5, 7), dtype=np.uint8)
    deep[:, :, 0:3], deep[:, :, 3:7] = 1, 3
    edge = S.boundary_np(deep)
    assert edge[2, 2, 1] == 0 and edge[2, 2, 2] == 1 and edge[2, 2, 3] == 3 and edge[2, 2, 4] == 0 and edge[0, 2, 1] == 1
    sheet = np.zeros((5, 5, 5), dtype=np.uint8)
    sheet[2] = 3                                                          # one voxel thick: all of it is boundary
    assert np.array_equal(S.boundary_np(sheet), sheet) and not S.boundary_np(sheet, background=False).any()
    assert S.boundary_np(sheet).dtype == np.uint8


# ---------------------------------------------------------------- surface_distances_np

def _boxes(shift=3):
    a, b = np.zeros((16, 16, 16), dtype=np.uint8), np.zeros((16, 16, 16), dtype=np.uint8)
    a[2:10, 4:12, 4:12] = 1
    b[2 + shift:10 + shift, 4:12, 4:12] = 1
    return a, b


def test_shifted_boxes_and_spacing():
    a, b = _boxes()
    r = S.surface_distances_np(a, b)
    surface = 8 ** 3 - 6 ** 3
    assert r.counts.dtype == np.int64 and r.counts.tolist() == [[surface, surface], [0, 0], [0, 0]]
    assert r.hd[0] == 3.0 and 0.0 < r.assd[0] < r.hd95[0] <= 3.0
    assert np.isnan(r.assd[1:]).all() and np.isnan(r.hd95[1:]).all() and np.isnan(r.hd[1:]).all()
    r2 = S.surface_distances_np(a, b, spacing=(2, 1, 1))
    assert r2.hd[0] == 6.0 and r2.assd[0] > r.assd[0]
    # the definition, by brute force over the two surfaces
    pa, pb = np.argwhere(S.boundary_np(a) == 1), np.argwhere(S.boundary_np(b) == 1)
    d = np.sqrt(((pa[:, None, :] - pb[None, :, :]) ** 2).sum(axis=2).astype(np.float32))
    dab, dba = d.min(axis=1), d.min(axis=0)
    assert r.assd[0] == (math.fsum(map(float, dab)) + math.fsum(map(float, dba))) / (len(dab) + len(dba))
    assert r.hd95[0] == max(float(np.percentile(dab, 95)), float(np.percentile(dba, 95)))


def test_identical_volumes_score_zero_and_an_absent_class_is_nan():
    rng = np.random.default_rng(4)
    a = rng.integers(0, 4, (6, 7, 8), dtype=np.uint8)
    for background in (True, False):
        r = S.surface_distances_np(a, a, 3, (1, 2, 3), background)
        assert r.assd.tolist() == r.hd95.tolist() == r.hd.tolist() == [0.0, 0.0, 0.0]
        assert (r.counts[:, 0] == r.counts[:, 1]).all() and r.counts.min() > 0
    b = np.where(a == 3, 2, a).astype(np.uint8)                          # class 3 is absent from b
    r = S.surface_distances_np(a, b, 3)
    assert r.counts[2].tolist() == [int((S.boundary_np(a) == 3).sum()), 0] and r.counts[2, 0] > 0
    assert np.isnan([r.assd[2], r.hd95[2], r.hd[2]]).all() and np.isfinite(r.assd[:2]).all() and np.isfinite(r.hd[:2]).all()


def test_argument_checks():
    a, b = _boxes()
    for spacing in ((1, 0, 1), (1, -1, 1), (1, np.inf, 1), (1, np.nan, 1), (1, 1), "abc", (1e30, 1, 1)):
        with pytest.raises(ValueError, match="voxel sizes"):
            S.surface_distances_np(a, b, 3, spacing)
    high = a.copy()
    high[0, 0, 0] = 4
    with pytest.raises(ValueError, match="label above 3"):
        S.surface_distances_np(high, b, 3)
    assert S.surface_distances_np(high, b, 4).counts.shape == (4, 2)
    for bad in (dict(classes=1), dict(classes=7), dict(classes=3.0)):
        with pytest.raises(ValueError, match="classes"):
            S.surface_distances_np(a, b, **bad)
    with pytest.raises(ValueError, match="uint8"):
        S.surface_distances_np(a.astype(np.int32), b)
    with pytest.raises(ValueError, match="shape"):
        S.surface_distances_np(a, b[:, :, :8])
    with pytest.raises(ValueError, match="volume"):
        S.boundary_np(a[0])
    with pytest.raises(ValueError, match="volume"):
        S.edt_sq_np(a[0])
    with pytest.raises(ValueError, match="limit of 1024"):
        S.edt_sq_np(np.zeros((1, 1, 1025), np.uint8))
    for weights in ((1, 1), (0, 1, 1), (1, np.inf, 1)):
        with pytest.raises(ValueError, match="weights"):
            S.edt_sq_np(a, 0, weights)
    for value in (-1, 256, 1.0, True):
        with pytest.raises(ValueError, match="value"):
            S.edt_sq_np(a, value)


def test_device_entries_refuse_cpu_tensors():
    import torch
    a = torch.from_numpy(_boxes()[0])
    for call in (lambda: S.label_boundary(a), lambda: S.distance_transform_sq(a), lambda: S.surface_distances(a, a),
                 lambda: S.SurfaceWorkspace(a.shape, 3, "cpu")):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="limit of 1024"):
        S.SurfaceWorkspace((4, 1025, 4), 3, "cuda")


# ---------------------------------------------------------------- the C side, without a GPU

def test_library_declares_the_entry_points_and_checks_their_arguments():
    import ctypes
    import os
    from mri_superresolution_amd import _lib
    lib = _lib.load()
    names = ("mrisr_u8_volume_label_boundary", "mrisr_u8_volume_edt_sq", "mrisr_f32_volume_surface_workspace_bytes",
             "mrisr_f32_volume_surface_gather")
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mrisr.h")) as f:
        header = f.read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and f" {name}(" in header
    assert lib.mrisr_version() == _lib.ABI_VERSION >= 324
    assert lib.mrisr_f32_volume_surface_workspace_bytes() % 8 == 0 and lib.mrisr_f32_volume_surface_workspace_bytes() > 0
    ARG, SHAPE = -1, -2
    buf = (ctypes.c_uint64 * 64)()                       # host memory: nothing is launched when a check fails
    p = ctypes.addressof(buf)
    q, r, w = p + 64, p + 128, p + 256
    assert lib.mrisr_u8_volume_label_boundary(None, 1, 1, 1, 1, 3, q, None, None) == ARG
    assert lib.mrisr_u8_volume_label_boundary(p, 1, 1, 1, 1, 3, None, None, None) == ARG
    assert lib.mrisr_u8_volume_label_boundary(p, 1, 1, 1, 1, 3, p, None, None) == ARG
    assert b"two buffers" in lib.mrisr_last_error()
    assert lib.mrisr_u8_volume_label_boundary(p, 1, 1, 1, 2, 3, q, None, None) == ARG
    assert lib.mrisr_u8_volume_label_boundary(p, 1, 1, 1, 1, 0, q, None, None) == ARG
    assert lib.mrisr_u8_volume_label_boundary(p, 1, 1, 1, 1, 3, q, w + 4, None) == ARG
    assert lib.mrisr_u8_volume_label_boundary(p, 0, 1, 1, 1, 3, q, None, None) == SHAPE
    assert lib.mrisr_u8_volume_label_boundary(p, 1, 1, 32768, 1, 3, q, None, None) == SHAPE
    assert lib.mrisr_u8_volume_edt_sq(None, 1, 1, 1, 0, 1.0, 1.0, 1.0, r, 7, 0, None) == ARG
    assert lib.mrisr_u8_volume_edt_sq(p, 1, 1, 1, 0, 1.0, 1.0, 1.0, None, 7, 0, None) == ARG
    assert lib.mrisr_u8_volume_edt_sq(p, 1, 1, 1, 0, 1.0, 1.0, 1.0, r + 2, 7, 0, None) == ARG
    assert lib.mrisr_u8_volume_edt_sq(p, 1, 1, 1, 256, 1.0, 1.0, 1.0, r, 7, 0, None) == ARG
    assert lib.mrisr_u8_volume_edt_sq(p, 1, 1, 1, 0, 1.0, 0.0, 1.0, r, 7, 0, None) == ARG
    assert lib.mrisr_u8_volume_edt_sq(p, 1, 1, 1, 0, 1.0, 1.0, float("inf"), r, 7, 0, None) == ARG
    assert b"weights" in lib.mrisr_last_error()
    assert lib.mrisr_u8_volume_edt_sq(p, 1, 1, 1, 0, 1.0, 1.0, 1.0, r, 7, 2, None) == ARG
    assert lib.mrisr_u8_volume_edt_sq(p, 1, 1, 1, 0, 1.0, 1.0, 1.0, r, 0, 0, None) == ARG
    assert lib.mrisr_u8_volume_edt_sq(p, 1, 1, 1, 0, 1.0, 1.0, 1.0, r, 8, 0, None) == ARG
    assert b"passes" in lib.mrisr_last_error()
    assert lib.mrisr_u8_volume_edt_sq(p, 1, 0, 1, 0, 1.0, 1.0, 1.0, r, 7, 0, None) == SHAPE
    for extents in ((1025, 1, 1), (1, 1025, 1), (1, 1, 1025)):
        assert lib.mrisr_u8_volume_edt_sq(p, *extents, 0, 1.0, 1.0, 1.0, r, 7, 0, None) == SHAPE
        assert b"1024" in lib.mrisr_last_error()
    assert lib.mrisr_f32_volume_surface_gather(None, q, 1, 4, r, q + 8, w, w + 64, None) == ARG
    assert lib.mrisr_f32_volume_surface_gather(p, q, 1, 4, r, q + 8, None, w + 64, None) == ARG
    assert lib.mrisr_f32_volume_surface_gather(p, q, 1, 4, r, q + 8, w, None, None) == ARG
    assert lib.mrisr_f32_volume_surface_gather(p, q, 1, 4, r, q + 8, w, w + 68, None) == ARG
    assert lib.mrisr_f32_volume_surface_gather(p, q, 1, 4, p, q + 8, w, w + 64, None) == ARG
    assert lib.mrisr_f32_volume_surface_gather(p, q, 1, 4, r, q, w, w + 64, None) == ARG
    assert b"of their own" in lib.mrisr_last_error()
    assert lib.mrisr_f32_volume_surface_gather(p, q, 0, 4, r, q + 8, w, w + 64, None) == ARG
    assert lib.mrisr_f32_volume_surface_gather(p, q, 1, 0, r, q + 8, w, w + 64, None) == SHAPE
    assert lib.mrisr_f32_volume_surface_gather(p, q, 1, 1 << 32, r, q + 8, w, w + 64, None) == SHAPE


# ---------------------------------------------------------------- the command lines

def test_command_lines_parse_the_new_option():
    from scripts import evaluate_volume as eval_cli
    assert eval_cli.parse_args(["--reference", "r.nii"]).tissue_surface is False
    assert eval_cli.parse_args(["--reference", "r.nii", "--mask", "otsu", "--tissue_dice", "3", "--tissue_surface"]).tissue_surface is True
    eval_cli.check_options(None, None, "linear", "header", "none", "none", tissue_dice=3, mask="otsu", tissue_surface=True)
    with pytest.raises(ValueError, match="--tissue_surface goes with --tissue_dice"):
        eval_cli.check_options(None, None, "linear", "header", "none", "none", mask="otsu", tissue_surface=True)
    assert eval_cli.surface_columns(3) == ["assd_1", "assd_2", "assd_3", "hd95_1", "hd95_2", "hd95_3"] and eval_cli.surface_columns(0) == []
