"""Registration from far apart (host): the numpy specification of the masked joint histogram, the mask moments, the rotation grid
and the coarse start of mri_superresolution_amd/volume_register.py; the whole registration on the far pair of
tests/farpairutil.py, where the start from the headers fails; and the refusals of the two new C entries that need no GPU."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import farpairutil as F                                                      # noqa: E402
import registerutil as U                                                     # noqa: E402
from mri_superresolution_amd import _lib                                     # noqa: E402
from mri_superresolution_amd import volume_register as G                     # noqa: E402

E_ARG, E_SHAPE, E_UNSUPPORTED = -1, -2, -5      # include/mrisr.h
RANGES = ((100.0, 700.0), (200.0, 300.0))


def small_pair(seed):
    rng = np.random.default_rng(seed)
    fixed = rng.uniform(-50, 950, (7, 9, 6)).astype(np.float32)
    moving = rng.uniform(0, 500, (6, 5, 8)).astype(np.float32)
    fixed[1, 2, 3] = np.nan
    fixed[4, 4, 4] = np.nan
    moving[2, 2, 3] = np.nan
    m = np.hstack([G.rotation_np(10, 20, 30) @ np.diag([0.8, 0.5, 1.2]), np.array([[0.4], [1.1], [-0.7]])])
    return fixed, moving, m


@pytest.mark.parametrize("stride", [1, 2, 4])
@pytest.mark.parametrize("bins", [16, 64])
def test_masked_histogram_equals_the_unmasked_one_on_filtered_samples(bins, stride):
    """Masking a sample out is the same as making it uncountable: the masked histogram equals the unmasked histogram of a fixed
    volume whose masked-out voxels were set to NaN by hand."""
    fixed, moving, m = small_pair(bins + stride)
    rng = np.random.default_rng(5)
    mask = rng.choice(np.array([0, 0, 1, 2, 255], dtype=np.uint8), fixed.shape)
    mask[0, 0, 0], mask[4, 4, 4] = 0, 1                    # a lattice point of every stride out, a NaN voxel in
    filtered = fixed.copy()
    filtered[mask == 0] = np.nan
    want = G.joint_histogram_np(filtered, moving, m, bins, stride, *RANGES)
    got = G.joint_histogram_np(fixed, moving, m, bins, stride, *RANGES, fixed_mask=mask)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(G.joint_histogram_np(fixed, moving, m, bins, stride, *RANGES, fixed_mask=mask != 0), want)      # bool
    plain = G.joint_histogram_np(fixed, moving, m, bins, stride, *RANGES)
    if stride == 1:
        assert 0 < got.sum() < plain.sum()
    assert (got <= plain).all()


def test_all_ones_all_zero_and_refused_masks():
    fixed, moving, m = small_pair(1)
    plain = G.joint_histogram_np(fixed, moving, m, 16, 1, *RANGES)
    assert np.array_equal(G.joint_histogram_np(fixed, moving, m, 16, 1, *RANGES, fixed_mask=None), plain)
    assert np.array_equal(G.joint_histogram_np(fixed, moving, m, 16, 1, *RANGES, fixed_mask=np.ones(fixed.shape, dtype=np.uint8)), plain)
    assert np.array_equal(G.joint_histogram_np(fixed, moving, m, 16, 1, *RANGES, fixed_mask=np.full(fixed.shape, 7, dtype=np.uint8)), plain)
    empty = G.joint_histogram_np(fixed, moving, m, 16, 1, *RANGES, fixed_mask=np.zeros(fixed.shape, dtype=np.uint8))
    assert empty.shape == (16, 16) and not empty.any()
    assert G.nmi_np(empty, 0) == (float("-inf"), 0)
    for bad in (np.ones(fixed.shape, dtype=np.float32), np.ones(fixed.shape, dtype=np.int32), np.ones(moving.shape, dtype=np.uint8),
                np.ones(fixed.shape[:2], dtype=np.uint8)):
        with pytest.raises(ValueError):
            G.joint_histogram_np(fixed, moving, m, 16, 1, *RANGES, fixed_mask=bad)


def test_mask_moments_np_against_argwhere():
    rng = np.random.default_rng(3)
    for shape in ((1, 1, 1), (3, 5, 70), (37, 41, 19)):
        mask = rng.choice(np.array([0, 0, 1, 2, 255], dtype=np.uint8), shape)
        idx = np.argwhere(mask != 0)
        got = G.mask_moments_np(mask)
        assert got.dtype == np.int64 and got.shape == (4,)
        assert got.tolist() == [len(idx)] + idx.sum(axis=0, dtype=np.int64).tolist()
        assert np.array_equal(G.mask_moments_np(mask != 0), got)
    assert G.mask_moments_np(np.zeros((2, 3, 4), dtype=np.uint8)).tolist() == [0, 0, 0, 0]
    assert G.mask_moments_np(np.ones((2, 3, 4), dtype=np.uint8)).tolist() == [24, 12, 24, 36]
    for bad in (np.ones((2, 3), dtype=np.uint8), np.ones((2, 3, 4), dtype=np.float32), np.ones((0, 3, 4), dtype=np.uint8)):
        with pytest.raises(ValueError):
            G.mask_moments_np(bad)


def test_mask_centre_world():
    a = np.array([[0.0, 2.0, 0.0, 5.0], [-1.0, 0.0, 0.0, 7.0], [0.0, 0.0, 0.5, -3.0], [0.0, 0.0, 0.0, 1.0]])
    mo = np.array([4, 6, 10, 2], dtype=np.int64)           # centre of mass (1.5, 2.5, 0.5)
    c = G.mask_centre_world(mo, a)
    assert c.dtype == np.float64 and np.array_equal(c, a[:3, :3] @ np.array([1.5, 2.5, 0.5]) + a[:3, 3])
    with pytest.raises(ValueError):
        G.mask_centre_world(np.zeros(4, dtype=np.int64), a)
    with pytest.raises(ValueError):
        G.mask_centre_world(G.mask_moments_np(np.zeros((3, 3, 3), dtype=np.uint8)), np.eye(4))
    with pytest.raises(ValueError):
        G.mask_centre_world(np.ones(3, dtype=np.int64), a)


def test_rotation_grid_order_and_refusals():
    g = G.rotation_grid(40.0, 20.0)
    assert g.shape == (125, 3) and g.dtype == np.float64
    axis = np.arange(-40.0, 40.0 + 1e-9, 20.0)
    assert np.array_equal(g, np.array(list(itertools.product(axis, axis, axis))))
    assert tuple(g[0]) == (-40, -40, -40) and tuple(g[1]) == (-40, -40, -20) and tuple(g[5]) == (-40, -20, -40)      # rx slowest
    assert tuple(g[62]) == (0, 0, 0) and tuple(g[-1]) == (40, 40, 40)
    assert np.array_equal(G.rotation_grid(0.0, 5.0), np.zeros((1, 3)))
    assert len(G.rotation_grid(30.0, 15.0)) == 125 and len(G.rotation_grid(45.0, 10.0)) == 1000
    assert len(G.rotation_grid(25.0, 20.0)) == 27          # the limit is no multiple of the step: -25, -5, 15
    for limit, step in ((40.0, 0.0), (40.0, -5.0), (-1.0, 5.0), (50.0, 10.0), (40.0, 1e-9), (float("nan"), 5.0), (40.0, float("inf"))):
        with pytest.raises(ValueError):
            G.rotation_grid(limit, step)


def test_coarse_start_candidates_and_first_argmax():
    c, cf, cm = np.array([1.0, -2.0, 3.0]), np.array([4.0, 0.5, -1.0]), np.array([-20.0, 11.0, 6.0])
    grid = G.rotation_grid(20.0, 20.0)
    seen = []

    def cost(ps, stride):
        seen.append((np.array(ps), stride))
        vals = np.zeros(len(ps))
        vals[[7, 19]] = 1.5                                 # two equal maxima: the first wins
        vals[3] = float("-inf")
        return vals

    p0, value, entry = G.coarse_start(cost, cf, cm, c, grid, 4)
    (ps, stride), = seen
    assert stride == 4 and ps.shape == (27, 6) and np.array_equal(ps[:, 3:], grid)
    for p in ps:                                            # W(p) takes the fixed centre of mass onto the moving one
        w = G.rigid_world(p, c)
        assert np.allclose(w[:3, :3] @ cf + w[:3, 3], cm, atol=1e-12)
    assert np.array_equal(p0, ps[7]) and value == 1.5
    assert entry == {"kind": "coarse", "stride": 4, "n_candidates": 27, "values": tuple(cost(ps, 4).tolist()), "accepted": 7, "best": 1.5}
    with pytest.raises(ValueError):
        G.coarse_start(lambda ps, s: [float("-inf")] * len(ps), cf, cm, c, grid, 4)
    with pytest.raises(ValueError):
        G.coarse_start(cost, cf, cm, c, np.zeros((0, 3)), 4)


def test_header_start_without_a_mask_is_the_registration_as_it_was():
    fixed, moving = U.synthetic_pair()
    want = U.specification_result()
    got = G.register_rigid_np(fixed, U.FIXED_AFFINE, moving, U.MOVING_AFFINE, bins=U.BINS, fixed_mask=None, moving_mask=None,
                              mask_cost=False, init="header", init_limit=40.0, init_step=20.0)
    assert got.p.tobytes() == want.p.tobytes() and got.value == want.value and got.n_evaluations == want.n_evaluations
    assert got.world.tobytes() == want.world.tobytes() and got.matrix.tobytes() == want.matrix.tobytes()
    assert got.trace == want.trace and got.trace[0]["kind"] == "start"
    with pytest.raises(ValueError):
        G.register_rigid_np(fixed, U.FIXED_AFFINE, moving, U.MOVING_AFFINE, bins=U.BINS, init="centre")
    with pytest.raises(ValueError):
        G.register_rigid_np(fixed, U.FIXED_AFFINE, moving, U.MOVING_AFFINE, bins=U.BINS, init="global", p0=np.zeros(6))


def test_the_far_pair_is_what_it_claims():
    fixed, moving = F.far_pair()
    fmask, mmask = F.far_masks()
    assert fixed.shape == F.FIXED_SHAPE and moving.shape == F.MOVING_SHAPE and fixed.dtype == moving.dtype == np.float32
    assert fmask.mean() == pytest.approx(0.246, abs=0.001) and mmask.mean() == pytest.approx(0.209, abs=0.001)
    assert F.corner_error_voxels(np.eye(4)) == pytest.approx(39.7, abs=0.05)


def test_the_start_from_the_headers_fails_on_the_far_pair():
    """The case that shows the feature is needed: ``register_rigid_np`` as shipped ends 35.5 voxels off (254 evaluations)."""
    r = F.specification_result("header", False)
    err = F.corner_error_voxels(r.world)
    print(f"header start: {err:.3f} voxels off, p = {r.p.tolist()}, {r.n_evaluations} evaluations")
    assert err > 20.0 and r.trace[0]["kind"] == "start"


@pytest.mark.parametrize("mask_cost", [True, False])
def test_the_global_start_registers_the_far_pair(mask_cost):
    """At most ONE fixed voxel (the smallest voxel size) at the worst corner, with the mask in the cost and without.  The
    specification reaches 0.085 voxels masked (475 evaluations) and 0.307 unmasked (427)."""
    r = F.specification_result("global", mask_cost)
    err = F.corner_error_voxels(r.world)
    print(f"global start, mask_cost={mask_cost}: {err:.3f} voxels off, p = {r.p.tolist()}, {r.n_evaluations} evaluations")
    assert err <= 1.0
    coarse = r.trace[0]
    assert coarse["kind"] == "coarse" and coarse["stride"] == 4 and coarse["n_candidates"] == 125 == len(coarse["values"])
    assert coarse["best"] == coarse["values"][coarse["accepted"]] == max(coarse["values"])
    assert coarse["accepted"] == coarse["values"].index(coarse["best"])
    assert all(t["kind"] in ("start", "probe") for t in r.trace[1:]) and r.trace[1]["kind"] == "start"
    assert r.n_evaluations == 125 + sum(len(t["values"]) for t in r.trace[1:])
    # the search starts where the coarse stage ended, with half the grid's step on the rotations
    v = G.voxel_size(F.FIXED_AFFINE)
    assert r.trace[1]["step"] == (2 * v,) * 3 + (10.0,) * 3 and r.trace[1]["stride"] == 4
    grid = G.rotation_grid(40.0, 20.0)
    assert r.trace[1]["p"][3:] == tuple(grid[coarse["accepted"]])
    assert [t["stride"] for t in r.trace if t["kind"] == "start"] == [4, 2]


def test_computed_masks_equal_given_masks():
    """Missing masks are the Otsu masks of the volumes: the same result as handing them in."""
    fixed, moving = F.far_pair()
    want = F.specification_result("global", True)
    got = G.register_rigid_np(fixed, F.FIXED_AFFINE, moving, F.MOVING_AFFINE, bins=F.BINS, mask_cost=True, init="global")
    assert got.p.tobytes() == want.p.tobytes() and got.trace == want.trace


def test_library_has_the_new_entries_and_they_refuse_without_a_gpu():
    """Every refusal below returns before any HIP call: the pointers are never dereferenced."""
    lib = _lib.load()
    for name in ("mrisr_f32_volume_joint_histogram_masked", "mrisr_u8_volume_mask_moments"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.mrisr_version() == _lib.ABI_VERSION >= 317
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])

    def mats(k=1, **entries):
        ms = np.stack([eye] * max(k, 1))
        for pos, val in entries.items():
            ms[-1, int(pos[1]), int(pos[2])] = val
        return (ctypes.c_double * ms.size)(*ms.reshape(-1))

    def jh(m=None, k=1, stride=1, bins=16, fr=(0.0, 1.0), mr=(0.0, 1.0), fshape=(4, 6, 5), mshape=(4, 6, 5), fp=a, kp=a, mp=a, hp=a):
        return lib.mrisr_f32_volume_joint_histogram_masked(fp, *fshape, kp, mp, *mshape, mats(k) if m is None else m, k, stride, bins,
                                                           *fr, *mr, hp, None)

    inf, nan = float("inf"), float("nan")
    assert jh(kp=None) == E_ARG and b"null" in lib.mrisr_last_error() and b"masked" in lib.mrisr_last_error()
    assert jh(fp=None) == E_ARG and jh(mp=None) == E_ARG and jh(hp=None) == E_ARG and jh(m=ctypes.POINTER(ctypes.c_double)()) == E_ARG
    assert jh(m=mats(e12=nan)) == E_ARG and jh(m=mats(k=3, e03=inf), k=3) == E_ARG and jh(m=mats(e00=1e308), stride=8) == E_ARG
    for k in (0, -1, 17):
        assert jh(k=k, m=mats(17)) == E_ARG
    for stride in (0, 3, 16, -2):
        assert jh(stride=stride) == E_ARG
    for bins in (0, 8, 17, 128, -16):
        assert jh(bins=bins) == E_ARG
    for r in ((0.0, 0.0), (1.0, 0.5), (nan, 1.0), (0.0, inf), (-inf, 0.0), (0.0, 1e300), (0.0, 1e-45)):
        assert jh(fr=r) == E_ARG and jh(mr=r) == E_ARG, r
    assert jh(fshape=(4, 0, 5)) == E_SHAPE and jh(mshape=(0, 6, 5)) == E_SHAPE and jh(fshape=(4, 6, -1)) == E_SHAPE
    assert jh(fshape=(2048, 2048, 512)) == E_UNSUPPORTED and jh(mshape=(32768, 32768, 2)) == E_UNSUPPORTED
    assert b"2^31 - 1" in lib.mrisr_last_error()

    mm = lib.mrisr_u8_volume_mask_moments
    assert mm(None, 2, 2, 2, a, None) == E_ARG and b"null" in lib.mrisr_last_error()
    assert mm(a, 2, 2, 2, None, None) == E_ARG
    assert mm(a, 2, 2, 2, a + (-a) % 8 + 4, None) == E_ARG and b"misaligned" in lib.mrisr_last_error()
    for shape in ((0, 2, 2), (2, -1, 2), (2, 2, 0), (32768, 2, 2), (2, 32768, 2), (2, 2, 32768)):
        assert mm(a, *shape, a + (-a) % 8, None) == E_SHAPE, shape
    assert mm(a, 2048, 2048, 512, a + (-a) % 8, None) == E_UNSUPPORTED and b"2^31 - 1" in lib.mrisr_last_error()
    assert mm(a, 32767, 32767, 32767, a + (-a) % 8, None) == E_UNSUPPORTED


def test_cpu_tensors_raise():
    import torch
    v = torch.zeros((4, 4, 4), dtype=torch.float32)
    with pytest.raises(ValueError):
        G.mask_moments(torch.ones((4, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        G.register_rigid(v, np.eye(4), v, np.eye(4), init="global", mask_cost=True)
