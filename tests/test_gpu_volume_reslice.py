"""Reslicing between voxel grids (GPU): csrc/volume_reslice.hip against its numpy specifications reslice_np / reslice_mask_np, bit
for bit - the kernel restates them operation by operation -, the refusals of the two entry points and of the wrappers."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd import _lib as L                                # noqa: E402
from mri_superresolution_amd import volume_reslice as R                      # noqa: E402
from mri_superresolution_amd.utils.nifti import grid_matrix, upscaled_affine  # noqa: E402

E_ARG, E_SHAPE, E_UNSUPPORTED = -1, -2, -5      # include/mrisr.h
METHODS = ("nearest", "linear", "cubic")
# source -> destination.  The kernel's brick is 2 x 2 x 64 voxels (x, y, z): (9, 11, 70) is 5 x 6 x 2 bricks with a remainder of
# 1, 1 and 6 voxels - adjusted from the (9, 10, 70) of the proposal, whose y extent is a whole number of bricks (bricks of
# 4 x 4 x 16 or 8 x 8 x 4 would leave a remainder on every axis of it as well)
SHAPES = [((1, 1, 1), (2, 3, 4)), ((2, 3, 5), (3, 5, 7)), ((5, 4, 3), (4, 4, 4)), ((11, 7, 37), (9, 11, 70))]
MATRICES = ("identity", "permute_flip", "half_pixel", "respace", "rotation", "boundary")


def values(shape, seed):
    """+-3000; every other voxel along z at an integer step."""
    v = np.random.default_rng(seed).uniform(-3000.0, 3000.0, shape)
    v[..., ::2] = np.rint(v[..., ::2])
    # no -0: a zero weight times a finite tap is +-0, and (+0) + (-0) = +0, so an exact gather returns -0 as +0
    return v.astype(np.float32) + np.float32(0)


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def rotation(deg_x, deg_y, deg_z):
    ax, ay, az = np.deg2rad([deg_x, deg_y, deg_z])
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return rz @ ry @ rx


def matrix(name, src, dst):
    """(3, 4) float64: destination index -> source index."""
    n, d = np.array(src, dtype=np.float64), np.array(dst, dtype=np.float64)
    m = np.zeros((3, 4))
    if name == "identity":
        m[:, :3] = np.eye(3)
    elif name == "permute_flip":                                 # source axis a runs along destination axis perm[a]; x and z reversed
        for a, (b, flip) in enumerate(zip((2, 0, 1), (True, False, True))):
            m[a, b], m[a, 3] = (-1.0, n[a] - 1) if flip else (1.0, 0.0)
    elif name == "half_pixel":                                   # the x2 geometry of upscaled_affine
        m[:, :3], m[:, 3] = 0.5 * np.eye(3), -0.25
    elif name == "respace":                                      # non-dyadic voxel sizes, the first corner kept
        s = np.array([0.3, 1.7, 0.3])
        m[:, :3], m[:, 3] = np.diag(s), 0.5 * s - 0.5
    elif name == "rotation":
        # 10 / 20 / 30 degrees about the centres; the destination's field of view is 1.3 times the source's, moved by a fifth of
        # the source's extent along x, a seventh along y and a ninth back along z: part of it sees the source, part does not
        lin = rotation(10, 20, 30) @ np.diag(1.3 * n / d)
        m[:, :3] = lin
        m[:, 3] = (n - 1) / 2 + n * np.array([0.2, 1 / 7, -1 / 9]) - lin @ ((d - 1) / 2)
    elif name == "boundary":
        # dyadic steps, so that the coordinates are exact: x starts exactly on p = -0.5, y starts exactly on p = n - 0.5 and
        # walks down, z ends exactly on p = n - 0.5
        m[0, 0], m[0, 3] = 0.5, -0.5
        m[1, 1], m[1, 3] = -0.5, n[1] - 0.5
        m[2, 2], m[2, 3] = 0.25, n[2] - 0.5 - 0.25 * (d[2] - 1)
    else:
        raise KeyError(name)
    return m


@pytest.fixture(scope="module")
def cases():
    """{(src, dst, matrix name): (v, mask, m, {method: specification}, specification of the mask)}: computed once, only read."""
    out = {}
    for src, dst in SHAPES:
        v = values(src, seed=sum(src) + sum(dst))
        mask = (np.random.default_rng(sum(dst)).integers(0, 4, src) % 3).astype(np.uint8)      # values 0, 1, 2
        for name in MATRICES:
            m = matrix(name, src, dst)
            want = {method: R.reslice_np(v, m, dst, method, fill=-1234.5) for method in METHODS}
            out[src, dst, name] = (v, mask, m, want, R.reslice_mask_np(mask, m, dst, fill=9))
    return out


@pytest.mark.parametrize("name", MATRICES)
@pytest.mark.parametrize("shapes", SHAPES, ids=str)
def test_reslice_is_bit_equal_to_the_specification(cases, shapes, name):
    src, dst = shapes
    v, mask, m, want, want_mask = cases[src, dst, name]
    x = torch.from_numpy(v).cuda()
    for method in METHODS:
        got = R.reslice(x, m, dst, method, fill=-1234.5).cpu().numpy()
        assert same_bits(got, want[method]), (method, src, dst, name, int((got != want[method]).sum()))
    got_mask = R.reslice_mask(torch.from_numpy(mask).cuda(), m, dst, fill=9).cpu().numpy()
    assert got_mask.dtype == np.uint8 and np.array_equal(got_mask, want_mask)
    # the uint8 kernel against the float nearest kernel on the same values
    as_float = R.reslice(torch.from_numpy(mask.astype(np.float32)).cuda(), m, dst, "nearest", fill=9.0).cpu().numpy()
    assert np.array_equal(as_float, got_mask.astype(np.float32))


@pytest.mark.parametrize("shapes", SHAPES, ids=str)
def test_the_cases_exercise_what_they_are_for(cases, shapes):
    """On the specification's output, on the CPU: the rotation both fills and interpolates at least a fifth of the voxels, the
    boundary matrix puts voxels exactly on p = -0.5 and p = n - 0.5 and they count as inside, the identities hold."""
    src, dst = shapes
    v, _, m, want, _ = cases[src, dst, "rotation"]
    _, inside = R.source_coordinates_np(m, dst, src)
    assert inside.mean() >= 0.2 and (~inside).mean() >= 0.2, (src, dst, inside.mean())
    for method in METHODS:
        assert ((want[method] == np.float32(-1234.5)) == ~inside).all()
    m = cases[src, dst, "boundary"][2]
    p, inside = R.source_coordinates_np(m, dst, src)
    assert (p[0] == -0.5).any() and (p[1] == src[1] - 0.5).any() and (p[2] == src[2] - 0.5).any()
    assert inside[(p[0] == -0.5) & (p[1] == src[1] - 0.5) & (p[2] == src[2] - 0.5)].all()
    assert (p[0] == -0.5).sum() * dst[0] == inside.size            # the whole first x plane
    v, _, _, want, _ = cases[src, dst, "identity"]
    both = tuple(slice(0, min(a, b)) for a, b in zip(src, dst))
    assert all(same_bits(np.ascontiguousarray(want[k][both]), np.ascontiguousarray(v[both])) for k in METHODS)


def test_refusals_launch_nothing():
    v = values((4, 6, 5), seed=9)
    x = torch.from_numpy(v).cuda()
    k = torch.ones((4, 6, 5), dtype=torch.uint8, device="cuda")
    out = torch.full((4, 6, 5), 9.0, dtype=torch.float32, device="cuda")
    out8 = torch.full((4, 6, 5), 9, dtype=torch.uint8, device="cuda")
    lib, st = L.load(), L.stream_ptr()

    def mat(**entries):
        m = np.hstack([np.eye(3), np.zeros((3, 1))])
        for pos, val in entries.items():
            m[int(pos[1]), int(pos[2])] = val
        return (L.C.c_double * 12)(*m.reshape(-1))

    def f32(m, method=L.RESAMPLE_LINEAR, src=(4, 6, 5), dst=(4, 6, 5)):
        return lib.mrisr_f32_volume_reslice(x.data_ptr(), *src, out.data_ptr(), *dst, m, method, 0.0, st)

    def u8(m, src=(4, 6, 5), dst=(4, 6, 5)):
        return lib.mrisr_u8_volume_reslice_nearest(k.data_ptr(), *src, out8.data_ptr(), *dst, m, 0, st)

    good = mat()
    assert f32(mat(e12=float("nan"))) == E_ARG and u8(mat(e12=float("nan"))) == E_ARG
    assert f32(mat(e03=float("inf"))) == E_ARG and u8(mat(e20=float("-inf"))) == E_ARG
    for method in (0, L.RESAMPLE_AREA, L.RESAMPLE_LANCZOS4, 6, -1):
        assert method not in R.METHODS.values() and f32(good, method) == E_ARG
    assert f32(good, dst=(4, 0, 5)) == E_SHAPE and f32(good, src=(0, 6, 5)) == E_SHAPE and f32(good, dst=(4, 6, -1)) == E_SHAPE
    assert u8(good, dst=(0, 6, 5)) == E_SHAPE and u8(good, src=(4, 6, 0)) == E_SHAPE
    # more than 2^31 - 1 voxels on either side: the code volume_label.hip uses for that
    assert f32(good, dst=(2048, 2048, 512)) == E_UNSUPPORTED and f32(good, src=(32768, 32768, 2)) == E_UNSUPPORTED
    assert u8(good, dst=(2048, 2048, 512)) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == 9.0).all() and (out8 == 9).all()              # nothing was launched
    assert f32(good) == 0 and u8(good) == 0
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), v) and (out8 == 1).all()


def test_wrappers_refuse_what_is_not_a_contiguous_device_volume():
    v = values((4, 6, 5), seed=10)
    x = torch.from_numpy(v).cuda()
    m = matrix("identity", v.shape, v.shape)
    with pytest.raises(ValueError):
        R.reslice(torch.from_numpy(v), m, v.shape)                                # CPU
    with pytest.raises(ValueError):
        R.reslice(x.transpose(0, 2), m, v.shape)                                  # not contiguous
    with pytest.raises(ValueError):
        R.reslice(x.double(), m, v.shape)                                         # wrong dtype
    with pytest.raises(ValueError):
        R.reslice(x[None], m, v.shape)
    with pytest.raises(ValueError):
        R.reslice(x, m, v.shape, "area")
    with pytest.raises(ValueError):
        R.reslice(x, m, (4, 0, 5))
    with pytest.raises(ValueError):
        R.reslice(x, np.full((3, 4), np.nan), v.shape)
    with pytest.raises(ValueError):
        R.reslice(x, np.eye(4), v.shape)
    k = (x > 0)
    with pytest.raises(ValueError):
        R.reslice_mask(k.cpu(), m, v.shape)
    with pytest.raises(ValueError):
        R.reslice_mask(k.transpose(0, 1), m, v.shape)
    with pytest.raises(ValueError):
        R.reslice_mask(x, m, v.shape)                                             # float32 is no mask
    with pytest.raises(ValueError):
        R.reslice_mask(k, m, v.shape, fill=256)
    with pytest.raises(ValueError):
        R.reslice_like(x.cpu(), np.eye(4), np.eye(4), v.shape)
    with pytest.raises(ValueError):
        R.reslice_like(x, np.diag([1.0, 0.0, 1.0, 1.0]), np.eye(4), v.shape)      # singular source affine
    assert torch.equal(R.reslice_mask(k, m, v.shape), k.to(torch.uint8))          # bool masks are taken
    # reslice_like: onto the x2 grid of upscaled_affine = the half-pixel matrix
    aff = np.array([[0.0, -2.0, 0.0, 10.0], [4.0, 0.0, 0.0, -4.0], [0.0, 0.0, 0.5, 3.0], [0.0, 0.0, 0.0, 1.0]])
    big = tuple(2 * d for d in v.shape)
    up = upscaled_affine(aff, (0, 1, 2))
    assert np.abs(grid_matrix(aff, up) - matrix("half_pixel", v.shape, big)).max() <= 1e-15
    got = R.reslice_like(x, aff, up, big, "cubic").cpu().numpy()
    assert same_bits(got, R.reslice_np(v, grid_matrix(aff, up), big, "cubic"))
    share = R.covered_share(v.shape, matrix("half_pixel", v.shape, big), big)
    assert share.is_cuda and float(share) == 1.0
