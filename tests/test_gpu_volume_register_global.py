"""Registration from far apart (GPU): the masked joint histogram of csrc/volume_register.hip against joint_histogram_np as integers,
the mask moments against mask_moments_np as integers, the wrappers' refusals, and register_rigid(init="global") on the far pair
of tests/farpairutil.py against the truth and against register_rigid_np."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import farpairutil as F                                                      # noqa: E402
import registerutil as U                                                     # noqa: E402
from mri_superresolution_amd import _lib as L                                # noqa: E402
from mri_superresolution_amd import volume_register as G                     # noqa: E402
from mri_superresolution_amd.volume_reslice import source_coordinates_np     # noqa: E402

# fixed, moving.  The kernel's brick is 8 x 8 x 16 samples (x, y, z): no fixed axis is a multiple of it at any stride
SHAPES = [((19, 21, 37), (9, 11, 70)), ((1, 9, 40), (6, 5, 8)), ((33, 8, 17), (20, 13, 9))]
MASKS = ("zero", "ones", "random", "nan_only")
FIXED_RANGE, MOVING_RANGE = (-1500.0, 1500.0), (-1000.0, 1200.0)
# NaN voxels of the fixed volumes (those that fit): on the stride-4 lattice and off it
NAN_VOXELS = [(0, 0, 0), (0, 4, 8), (0, 4, 32), (16, 4, 12), (0, 3, 5), (0, 7, 16), (8, 0, 4), (2, 2, 2)]


def values(shape, seed, nan_voxels=()):
    """+-3000, smooth along x plus noise (tests/test_gpu_volume_register.py)."""
    rng = np.random.default_rng(seed)
    x = np.linspace(-1, 1, shape[0]).reshape(-1, 1, 1)
    v = (2500.0 * np.sin(2 * x + rng.uniform(-1, 1, (1,) + tuple(shape[1:]))) + rng.uniform(-500.0, 500.0, shape)).astype(np.float32)
    for at in nan_voxels:
        if all(a < n for a, n in zip(at, shape)):
            v[at] = np.nan
    return v


def rotation(src, dst, shift=0.0):
    """10 / 20 / 30 degrees about the centres, part of the fixed grid outside the moving volume."""
    n, d = np.array(src, dtype=np.float64), np.array(dst, dtype=np.float64)
    lin = G.rotation_np(10, 20, 30) @ np.diag(1.3 * n / d)
    return np.hstack([lin, ((n - 1) / 2 + n * np.array([0.2, 1 / 7, -1 / 9]) - lin @ ((d - 1) / 2) + shift)[:, None]])


def flip(src, dst):
    """The moving axes reversed and stretched over the fixed extents: every sample inside."""
    n, d = np.array(src, dtype=np.float64), np.array(dst, dtype=np.float64)
    s = (n - 1) / np.maximum(d - 1, 1)
    return np.hstack([np.diag(-s), (n - 1)[:, None]])


def outside(src):
    m = np.hstack([np.eye(3), np.zeros((3, 1))])
    m[0, 3] = src[0] + 10.0
    return m


def batch16(src, dst):
    """16 mixed matrices: rotation, flip, wholly outside, then shifted rotations and flips in turn."""
    ms = [rotation(src, dst), flip(src, dst), outside(src)]
    while len(ms) < 16:
        ms.append(rotation(src, dst, 0.37 * len(ms)) if len(ms) % 2 else flip(src, dst) + np.eye(3, 4, 3) * 0.21 * len(ms))
    return np.stack(ms)


def mask_of(kind, fixed, seed):
    if kind == "zero":
        return np.zeros(fixed.shape, dtype=np.uint8)
    if kind == "ones":
        return np.ones(fixed.shape, dtype=np.uint8)
    if kind == "nan_only":                                  # only voxels that can never count
        return np.isnan(fixed).astype(np.uint8) * 3
    rng = np.random.default_rng(seed)
    m = np.where(rng.uniform(size=fixed.shape) < 0.3, rng.choice(np.array([1, 2, 255], dtype=np.uint8), fixed.shape), 0).astype(np.uint8)
    m[:8, :8, :16] = 0                                      # the first brick at stride 1: a workgroup with nothing to count
    return m


@pytest.fixture(scope="module")
def cases():
    """shapes -> (fixed, moving, {mask kind: mask}), host arrays, computed once and only read."""
    out = {}
    for f, m in SHAPES:
        fixed, moving = values(f, sum(f), NAN_VOXELS), values(m, sum(m) + 100, [(1, 1, 1)])
        out[(f, m)] = (fixed, moving, {kind: mask_of(kind, fixed, sum(f) + 7) for kind in MASKS})
    return out


@pytest.mark.parametrize("bins", [16, 64])
@pytest.mark.parametrize("stride", [1, 2, 4])
@pytest.mark.parametrize("shapes", SHAPES, ids=str)
def test_masked_histograms_equal_the_specification(cases, shapes, stride, bins):
    fshape, mshape = shapes
    fixed, moving, masks = cases[shapes]
    f, mv = torch.from_numpy(fixed).cuda(), torch.from_numpy(moving).cuda()
    ms = batch16(mshape, fshape)
    plain = G.joint_histogram(f, mv, ms, bins, stride, FIXED_RANGE, MOVING_RANGE).cpu().numpy()
    for kind in MASKS:
        mask = torch.from_numpy(masks[kind]).cuda()
        want = np.stack([G.joint_histogram_np(fixed, moving, m, bins, stride, FIXED_RANGE, MOVING_RANGE, fixed_mask=masks[kind]) for m in ms])
        # K = 16 into a stale buffer ...
        out = torch.full((16, bins, bins), 7, dtype=torch.int64, device="cuda")
        got = G.joint_histogram(f, mv, ms, bins, stride, FIXED_RANGE, MOVING_RANGE, fixed_mask=mask, out=out)
        assert got is out and np.array_equal(got.cpu().numpy(), want), (kind, shapes, stride, bins)
        # ... and K = 1 for the rotation, the flip and the matrix wholly outside
        for c in range(3):
            one = G.joint_histogram(f, mv, ms[c], bins, stride, FIXED_RANGE, MOVING_RANGE, fixed_mask=mask)
            assert one.dtype == torch.int64 and tuple(one.shape) == (1, bins, bins)
            assert np.array_equal(one[0].cpu().numpy(), want[c]), (kind, c, shapes, stride, bins)
        if kind in ("zero", "nan_only"):
            assert not want.any()
        if kind == "ones":                                  # bit for bit the unmasked entry's output
            assert np.array_equal(got.cpu().numpy(), plain)
        assert not want[2].any()


def test_the_cases_exercise_what_they_are_for(cases):
    """On the specification, on the CPU: samples are masked out, outside and NaN; masked-in NaN samples exist at every stride; the
    random mask has every value and leaves the first brick's workgroup with an entirely zero mask while others count."""
    for shapes in SHAPES:
        fshape, mshape = shapes
        fixed, moving, masks = cases[shapes]
        rnd = masks["random"]
        assert set(np.unique(rnd)) == {0, 1, 2, 255} and 0.15 <= (rnd != 0).mean() <= 0.35
        assert not rnd[:8, :8, :16].any() and rnd[:, :, 16:].any()               # stride 1: brick (0, 0, 0) is empty, others are not
        assert masks["nan_only"].any() and np.isnan(fixed[masks["nan_only"] != 0]).all()
        for stride in (1, 2, 4):
            assert np.isnan(fixed[::stride, ::stride, ::stride]).any()           # a NaN sample at every stride
            assert masks["nan_only"][::stride, ::stride, ::stride].any()
        for m in (rotation(mshape, fshape), flip(mshape, fshape)):
            _, inside = source_coordinates_np(m, fshape, mshape)
            plain = G.joint_histogram_np(fixed, moving, m, 16, 1, FIXED_RANGE, MOVING_RANGE)
            masked = G.joint_histogram_np(fixed, moving, m, 16, 1, FIXED_RANGE, MOVING_RANGE, fixed_mask=rnd)
            assert 0 < masked.sum() < plain.sum()                                 # some samples masked out, some counted
        _, inside = source_coordinates_np(rotation(mshape, fshape), fshape, mshape)
        assert 0.05 <= inside.mean() <= 0.95                                      # some outside
        assert source_coordinates_np(flip(mshape, fshape), fshape, mshape)[1].all()
        assert not source_coordinates_np(outside(mshape), fshape, mshape)[1].any()
    # NaN samples inside: the flip keeps every sample inside, so the NaN voxels are what its total lacks
    fixed, moving, _ = cases[SHAPES[0]]
    assert G.joint_histogram_np(fixed, moving, flip(SHAPES[0][1], SHAPES[0][0]), 16, 1, FIXED_RANGE, MOVING_RANGE).sum() < fixed.size


def moments_case(shape, kind, offset=0):
    """-> (device mask, host mask); ``offset``: the mask starts this many bytes into an allocation (no 16-byte alignment)."""
    n = int(np.prod(shape))
    if kind == "ones":
        host = np.ones(shape, dtype=np.uint8)
    else:
        host = np.random.default_rng(n + offset).choice(np.array([0, 0, 1, 2, 255], dtype=np.uint8), shape)
    dev = torch.zeros(n + offset + 16, dtype=torch.uint8, device="cuda")
    dev[:offset] = 9                                        # bytes before and after the mask are never counted
    dev[offset + n:] = 9
    dev[offset:offset + n] = torch.from_numpy(host.reshape(-1)).cuda()
    return dev[offset:offset + n].view(shape), host


@pytest.mark.parametrize("shape,kind,offset", [((1, 1, 1), "random", 0), ((1, 1, 1), "ones", 5), ((3, 5, 70), "random", 0),
                                               ((3, 5, 70), "random", 3), ((37, 41, 19), "random", 0), ((37, 41, 19), "random", 13),
                                               ((640, 512, 50), "ones", 0), ((32767, 2, 2), "random", 0), ((2, 32767, 2), "random", 1),
                                               ((2, 2, 32767), "ones", 0)], ids=str)
def test_mask_moments_equal_the_specification(shape, kind, offset):
    dev, host = moments_case(shape, kind, offset)
    assert dev.is_contiguous() and dev.data_ptr() % 16 == offset % 16
    got = G.mask_moments(dev)
    assert got.dtype == torch.int64 and tuple(got.shape) == (4,) and got.is_cuda
    want = G.mask_moments_np(host)
    assert got.cpu().numpy().tolist() == want.tolist(), (shape, kind, offset)
    if shape == (640, 512, 50):
        assert want[1] > 2 ** 32                            # past 32 bits
    # into the same stream again: the call zeroes its output
    assert G.mask_moments(dev).cpu().numpy().tolist() == want.tolist()


def test_wrappers_refuse():
    f = torch.from_numpy(np.random.default_rng(0).uniform(0, 1, (4, 6, 5)).astype(np.float32)).cuda()      # a range to register in
    mask = torch.ones((4, 6, 5), dtype=torch.uint8, device="cuda")
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    ok = dict(fixed=f, moving=f, ms=eye, bins=16, stride=1, fixed_range=(0.0, 1.0), moving_range=(0.0, 1.0), fixed_mask=mask)
    assert G.joint_histogram(**ok).sum().item() == f.numel()
    wide = torch.ones((4, 6, 10), dtype=torch.uint8, device="cuda")
    bad_masks = (mask.cpu(), mask.bool(), mask.float(), mask.int(), torch.ones((4, 6, 6), dtype=torch.uint8, device="cuda"),
                 torch.ones((5, 6, 4), dtype=torch.uint8, device="cuda").transpose(0, 2), wide[:, :, ::2], mask.cpu().numpy())
    for bad in bad_masks:
        with pytest.raises(ValueError):
            G.joint_histogram(**{**ok, "fixed_mask": bad})
    for bad in (mask.cpu(), mask.bool(), mask.float(), wide[:, :, ::2], mask[0], mask.cpu().numpy()):
        with pytest.raises(ValueError):
            G.mask_moments(bad)
    out4 = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    for bad in ((0, 6, 5), (4, 32768, 5), (4, 6, -1)):           # MRISR_E_SHAPE before the memset
        assert L.load().mrisr_u8_volume_mask_moments(mask.data_ptr(), *bad, out4.data_ptr(), L.stream_ptr()) == -2
    assert out4.cpu().tolist() == [-7] * 4
    for bad in bad_masks[:5]:
        with pytest.raises(ValueError):
            G.register_rigid(f, np.eye(4), f, np.eye(4), bins=16, fixed_mask=bad, mask_cost=True)
    with pytest.raises(ValueError):
        G.register_rigid(f, np.eye(4), f, np.eye(4), bins=16, init="somewhere")
    with pytest.raises(ValueError):
        G.register_rigid(f, np.eye(4), f, np.eye(4), bins=16, init="global", p0=np.zeros(6))
    with pytest.raises(ValueError):
        G.register_rigid(f, np.eye(4), f, np.eye(4), bins=16, init="global", init_step=0.0)


@pytest.mark.parametrize("mask_cost", [True, False])
def test_register_rigid_global_on_the_far_pair(mask_cost):
    """The far pair starts 39.7 voxels off.  At most ONE fixed voxel (the smallest voxel size) at the worst corner, with the mask in
    the cost and without; the coarse stage is one read and equals the specification's within 1e-9 (the NMI of a histogram that is
    equal as integers: tests/test_gpu_volume_register.py bounds the difference by 1e-11 relative)."""
    fixed, moving = F.far_pair()
    fmask, mmask = F.far_masks()
    want = F.specification_result("global", mask_cost)
    f, mv = torch.tensor(fixed).cuda(), torch.tensor(moving).cuda()                      # copies: the pair is read-only
    got = G.register_rigid(f, F.FIXED_AFFINE, mv, F.MOVING_AFFINE, bins=F.BINS, mask_cost=mask_cost, init="global")
    err = F.corner_error_voxels(got.world)
    print(f"mask_cost={mask_cost}: corner displacement {err:.3f} voxels (specification {F.corner_error_voxels(want.world):.3f}), "
          f"p = {got.p.tolist()} (specification {want.p.tolist()}), {got.n_evaluations} evaluations")
    assert err <= 1.0
    coarse = got.trace[0]
    assert coarse["kind"] == "coarse" and coarse["host_reads"] == 1 and coarse["n_candidates"] == 125 == len(coarse["values"])
    assert coarse["stride"] == 4
    assert all(t["kind"] in ("start", "probe") and t["host_reads"] == 1 for t in got.trace[1:])
    assert got.n_evaluations == 125 + sum(len(t["values"]) for t in got.trace[1:])
    for a, b in zip(coarse["values"], want.trace[0]["values"]):
        assert a == b if b == float("-inf") else abs(a - b) <= 1e-9, (a, b)
    assert coarse["accepted"] == want.trace[0]["accepted"] and got.trace[1]["p"] == want.trace[1]["p"]
    # the masks computed on the device are the specification's: handing them in changes nothing
    again = G.register_rigid(f, F.FIXED_AFFINE, mv, F.MOVING_AFFINE, bins=F.BINS, fixed_mask=torch.tensor(fmask).cuda(),
                             moving_mask=torch.tensor(mmask).cuda(), mask_cost=mask_cost, init="global")
    assert again.p.tobytes() == got.p.tobytes() and again.trace[0]["values"] == coarse["values"]


def test_the_header_start_is_what_it_was():
    """``init="header"``, ``mask_cost=False``: the registration of tests/test_gpu_volume_register.py, whatever masks are handed in -
    the same parameters as the call without the new arguments, and no coarse entry."""
    fixed, moving = U.synthetic_pair()
    f, mv = torch.tensor(fixed).cuda(), torch.tensor(moving).cuda()
    before = G.register_rigid(f, U.FIXED_AFFINE, mv, U.MOVING_AFFINE, bins=U.BINS)
    got = G.register_rigid(f, U.FIXED_AFFINE, mv, U.MOVING_AFFINE, bins=U.BINS, fixed_mask=torch.zeros_like(f, dtype=torch.uint8),
                           moving_mask=None, mask_cost=False, init="header", init_limit=40.0, init_step=20.0)
    assert got.p.tobytes() == before.p.tobytes() and got.value == before.value and got.n_evaluations == before.n_evaluations
    assert [t["kind"] for t in got.trace] == [t["kind"] for t in before.trace] and got.trace[0]["kind"] == "start"
    assert all(t["host_reads"] == 1 for t in got.trace)
    want = U.specification_result()
    v = G.voxel_size(U.FIXED_AFFINE)
    assert (np.abs(got.p[:3] - want.p[:3]) <= v / 16 + 1e-12).all() and (np.abs(got.p[3:] - want.p[3:]) <= 1 / 16 + 1e-12).all()
    assert U.corner_error_voxels(got.world) <= 1.0
