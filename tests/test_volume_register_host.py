"""Rigid registration (host): the numpy specification of mri_superresolution_amd/volume_register.py - the joint histogram against
a plain triple loop, normalised mutual information, the rigid parametrisation, the compass search's order and tie rule, and the
whole registration on a synthetic pair."""
import math
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import registerutil as U                                                     # noqa: E402
from mri_superresolution_amd import _lib                                     # noqa: E402
from mri_superresolution_amd import volume_register as G                     # noqa: E402
from mri_superresolution_amd.utils.nifti import grid_matrix                  # noqa: E402
from mri_superresolution_amd.volume_reslice import reslice_np, source_coordinates_np      # noqa: E402


def loop_histogram(fixed, moving, m, bins, stride, frange, mrange):
    """The definition, one sample at a time in Python floats and numpy float32 scalars."""
    f32 = np.float32
    H = np.zeros((bins, bins), dtype=np.int64)

    def bin_of(v, r):
        lo, hi = f32(r[0]), f32(r[1])
        scale = f32(bins) / (hi - lo)
        x = (f32(v) - lo) * scale
        return min(bins - 1, max(0, int(x))) if np.isfinite(x) else (bins - 1 if x > 0 else 0)

    for i in range(0, fixed.shape[0], stride):
        for j in range(0, fixed.shape[1], stride):
            for k in range(0, fixed.shape[2], stride):
                p = [((m[a, 0] * i + m[a, 1] * j) + m[a, 2] * k) + m[a, 3] for a in range(3)]
                if not all(-0.5 <= p[a] <= moving.shape[a] - 0.5 for a in range(3)):
                    continue
                # the moving value of this one voxel through reslice_np: a 1 x 1 x 1 destination whose matrix is the point
                point = np.zeros((3, 4))
                point[:, 3] = p
                mv = reslice_np(moving, point, (1, 1, 1), "linear")[0, 0, 0]
                fv = fixed[i, j, k]
                if np.isnan(fv) or np.isnan(mv):
                    continue
                H[bin_of(fv, frange), bin_of(mv, mrange)] += 1
    return H


def tilted(src, dst):
    """A rotation of 10 / 20 / 30 degrees about the centres with part of the destination outside (tests/test_gpu_volume_reslice.py)."""
    n, d = np.array(src, dtype=np.float64), np.array(dst, dtype=np.float64)
    lin = G.rotation_np(10, 20, 30) @ np.diag(1.3 * n / d)
    return np.hstack([lin, ((n - 1) / 2 + n * np.array([0.2, 1 / 7, -1 / 9]) - lin @ ((d - 1) / 2))[:, None]])


@pytest.mark.parametrize("stride", [1, 2, 4])
@pytest.mark.parametrize("bins", [16, 64])
def test_joint_histogram_matches_a_triple_loop(bins, stride):
    rng = np.random.default_rng(bins + stride)
    fixed = rng.uniform(-50, 950, (7, 9, 6)).astype(np.float32)
    moving = rng.uniform(0, 500, (6, 5, 8)).astype(np.float32)
    fixed[1, 2, 3] = np.nan
    fixed[4, 4, 4] = np.nan                      # on the stride-2 and the stride-4 lattice
    moving[2, 2, 3] = np.nan
    moving[0, 0, 0] = np.inf
    for m in (np.hstack([np.eye(3), np.zeros((3, 1))]), tilted(moving.shape, fixed.shape)):
        # ranges inside the values' span: the clamp works at both ends
        want = loop_histogram(fixed, moving, m, bins, stride, (100.0, 700.0), (200.0, 300.0))
        got = G.joint_histogram_np(fixed, moving, m, bins, stride, (100.0, 700.0), (200.0, 300.0))
        assert got.dtype == np.int64 and got.shape == (bins, bins) and np.array_equal(got, want)
        if stride == 1:
            assert want[0].sum() > 0 and want[-1].sum() > 0 and want[:, 0].sum() > 0 and want[:, -1].sum() > 0
        # the total: the inside samples whose two values are no NaN
        ms = G.strided_matrix(m, stride)
        fs = fixed[::stride, ::stride, ::stride]
        mv = reslice_np(moving, ms, fs.shape, "linear")
        inside = source_coordinates_np(ms, fs.shape, moving.shape)[1]
        assert got.sum() == (inside & ~np.isnan(fs) & ~np.isnan(mv)).sum() < fs.size


def test_joint_histogram_refuses():
    v = np.zeros((4, 4, 4), dtype=np.float32)
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    ok = dict(fixed=v, moving=v, m=eye, bins=16, stride=1, fixed_range=(0.0, 1.0), moving_range=(0.0, 1.0))
    assert G.joint_histogram_np(**ok).sum() == 64
    for bad in (dict(bins=8), dict(bins=128), dict(stride=3), dict(stride=16), dict(fixed_range=(1.0, 1.0)), dict(moving_range=(2.0, 1.0)),
                dict(fixed_range=(0.0, float("inf"))), dict(moving_range=(float("nan"), 1.0)), dict(fixed_range=(0.0, 1e-45)),
                dict(m=np.full((3, 4), np.nan)), dict(m=np.eye(4)), dict(fixed=v.astype(np.float64)), dict(moving=v[0])):
        with pytest.raises(ValueError):
            G.joint_histogram_np(**{**ok, **bad})


def test_nmi():
    fixed, _ = U.synthetic_pair()
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    r = (float(fixed.min()), float(fixed.max()))
    for bins in (16, 64):
        H = G.joint_histogram_np(fixed, fixed, eye, bins, 2, r, r)
        assert (np.diag(H) > 0).sum() > 1 and H.sum() == np.diag(H).sum() == G.sample_count(fixed.shape, 2)
        value, count = G.nmi_np(H, 1)
        assert value == 2.0 and count == H.sum() and count.dtype == np.int64      # exactly: the three sums add the same terms
    # independent uniform marginals: H_fm = H_f + H_m
    assert G.nmi_np(np.full((16, 16), 3, dtype=np.int64))[0] == pytest.approx(1.0, rel=1e-14)
    # a hand-computed case
    H = np.zeros((16, 16), dtype=np.int64)
    H[0, 0], H[0, 1], H[3, 1] = 2, 1, 1
    ent = lambda ps: -sum(p * math.log(p) for p in ps)                          # noqa: E731
    assert G.nmi_np(H)[0] == pytest.approx((ent([0.75, 0.25]) + ent([0.5, 0.5])) / ent([0.5, 0.25, 0.25]), rel=1e-15)
    # too few samples: -inf, the count still reported; an empty histogram is -inf whatever min_count
    assert G.nmi_np(H, 5) == (float("-inf"), 4) and G.nmi_np(H, 4)[0] > 0
    assert G.nmi_np(np.zeros((16, 16), dtype=np.int64), 0) == (float("-inf"), 0)
    # one occupied cell: H_fm == 0 -> 0.0
    one = np.zeros((32, 32), dtype=np.int64)
    one[5, 7] = 1000
    assert G.nmi_np(one, 10) == (0.0, 1000)
    with pytest.raises(ValueError):
        G.nmi_np(np.zeros((16, 8), dtype=np.int64))
    with pytest.raises(ValueError):
        G.nmi_np(np.zeros((16, 16)))


def test_rigid_parametrisation():
    centre = G.volume_centre(U.FIXED_AFFINE, U.FIXED_SHAPE)
    assert np.array_equal(centre, U.FIXED_AFFINE[:3, :3] @ ((np.array(U.FIXED_SHAPE) - 1) / 2) + U.FIXED_AFFINE[:3, 3])
    # p = 0: the header matrix, to the last bit
    m0 = G.candidate_matrix(np.zeros(6), U.FIXED_AFFINE, U.MOVING_AFFINE, centre)
    assert m0.tobytes() == grid_matrix(U.MOVING_AFFINE, U.FIXED_AFFINE).tobytes()
    assert G.rigid_world(np.zeros(6), centre).tobytes() == np.eye(4).tobytes()
    # a pure translation; the centre is the fixed point of a pure rotation
    w = G.rigid_world([1.0, -2.0, 3.0, 0, 0, 0], centre)
    assert np.array_equal(w[:3, :3], np.eye(3)) and np.array_equal(w[:3, 3], [1.0, -2.0, 3.0])
    w = G.rigid_world([0, 0, 0, 10.0, -20.0, 30.0], centre)
    assert np.allclose(w[:3, :3] @ centre + w[:3, 3], centre, atol=1e-12)
    assert np.allclose(w[:3, :3] @ w[:3, :3].T, np.eye(3), atol=1e-15) and np.linalg.det(w[:3, :3]) == pytest.approx(1.0)
    # R = Rz Ry Rx: 90 degrees about x, then about z, takes e_y to e_z and e_x to e_y
    r = G.rotation_np(90, 0, 90)
    assert np.allclose(r @ [0, 1, 0], [0, 0, 1], atol=1e-15) and np.allclose(r @ [1, 0, 0], [0, 1, 0], atol=1e-15)
    # composition and inverse: rotations about one axis add; the inverse world matrix takes the image back
    a, b = G.rigid_world([0, 0, 0, 0, 0, 12.0], centre), G.rigid_world([0, 0, 0, 0, 0, 30.0], centre)
    assert np.allclose(a @ b, G.rigid_world([0, 0, 0, 0, 0, 42.0], centre), atol=1e-12)
    w = G.rigid_world(U.P_TRUE, centre)
    x = np.array([3.0, -7.0, 11.0, 1.0])
    assert np.allclose(np.linalg.inv(w) @ (w @ x), x, atol=1e-12)
    assert np.allclose((w @ x)[:3], G.rotation_np(*U.P_TRUE[3:]) @ (x[:3] - centre) + centre + U.P_TRUE[:3], atol=1e-12)
    # the candidate matrix is inv(A_mov) W A_fix
    m = G.candidate_matrix(U.P_TRUE, U.FIXED_AFFINE, U.MOVING_AFFINE, centre)
    assert np.allclose(m, (np.linalg.inv(U.MOVING_AFFINE) @ w @ U.FIXED_AFFINE)[:3], atol=1e-12)
    assert G.corner_displacement(w, w, U.FIXED_AFFINE, U.FIXED_SHAPE) == 0.0
    assert G.corner_displacement(G.rigid_world([3.0, 4.0, 0, 0, 0, 0], centre), np.eye(4), U.FIXED_AFFINE, U.FIXED_SHAPE) == pytest.approx(5.0)
    with pytest.raises(ValueError):
        G.rigid_world([0, 0, 0, 0, 0, float("nan")], centre)
    with pytest.raises(ValueError):
        G.rigid_world(np.zeros(5), centre)


def test_compass_search_order_and_tie_rule():
    """A concave quadratic with its maximum at a known point: the trace is replayed step by step."""
    target = np.array([3.0, -1.0, 0.5, 2.0, 0.0, -4.0])
    calls = []

    def cost(ps, stride):
        calls.append((np.array(ps), stride))
        return [-float(((p - target) ** 2).sum()) for p in ps]

    levels = [(4, (2.0,) * 3 + (2.0,) * 3, 0.5), (2, (0.5,) * 3 + (0.5,) * 3, 1 / 16)]
    p, value, n_eval, trace = G.compass_search(cost, np.zeros(6), levels)
    assert len(trace) == len(calls) and n_eval == sum(len(c[0]) for c in calls)
    assert np.array_equal(p, target) and value == 0.0           # the target is on the lattice of dyadic steps
    assert [t["kind"] for t in trace].count("start") == 2 and trace[0]["kind"] == "start" and trace[0]["p"] == (0.0,) * 6
    cur, best, level = np.zeros(6), None, -1
    for entry, (ps, stride) in zip(trace, calls):
        assert stride == levels[entry["level"]][0] == entry["stride"]
        if entry["kind"] == "start":
            level += 1
            step = np.array(levels[level][1])
            assert entry["level"] == level and len(ps) == 1 and np.array_equal(ps[0], cur)
            best = entry["values"][0]
            continue
        assert entry["p"] == tuple(cur) and entry["step"] == tuple(step) and step[0] >= levels[level][2]
        # the 12 candidates: axis ascending, + before -
        assert len(ps) == 12
        for a in range(6):
            e = np.zeros(6)
            e[a] = step[a]
            assert np.array_equal(ps[2 * a], cur + e) and np.array_equal(ps[2 * a + 1], cur - e)
        vals = np.array(entry["values"])
        j = int(np.argmax(vals))
        if vals[j] > best:
            assert entry["accepted"] == j
            cur, best = ps[j], vals[j]
        else:
            assert entry["accepted"] is None
            step = step / 2
        assert entry["best"] == best
    # every level ends below its stop
    assert trace[-1]["accepted"] is None and trace[-1]["step"][0] == 1 / 16

    # ties: two equal maxima -> the first in the documented order; an argmax equal to the best so far is not taken
    def flat(ps, stride):
        return [0.0 if abs(p[0]) + abs(p[1]) == 0 else (1.0 if abs(p[1]) == 1.0 and p[0] == 0 else -1.0) for p in ps]
    p, value, _, trace = G.compass_search(flat, np.zeros(6), [(1, (1.0,) * 6, 1.0)])
    assert trace[1]["accepted"] == 2 and trace[1]["values"][2] == trace[1]["values"][3] == 1.0      # +y before -y
    assert tuple(p) == (0, 1, 0, 0, 0, 0) and value == 1.0
    assert trace[2]["accepted"] is None and max(trace[2]["values"]) <= 1.0 and len(trace) == 3       # -y of (0, 1) is 0.0: no move
    p, value, n_eval, trace = G.compass_search(lambda ps, s: [float("-inf")] * len(ps), np.ones(6), [(1, (1.0,) * 6, 0.25)])
    assert np.array_equal(p, np.ones(6)) and value == float("-inf") and n_eval == 1 + 12 * 3 and len(trace) == 4
    with pytest.raises(ValueError):
        G.compass_search(cost, np.zeros(6), [(1, (1.0,) * 5, 1.0)])


def test_levels_and_strides(caplog):
    v = G.voxel_size(U.FIXED_AFFINE)
    assert v == pytest.approx((1.0 + 0.9 + 1.25) / 3)
    (s0, step0, stop0), (s1, step1, stop1) = G.default_levels(U.FIXED_AFFINE)
    assert (s0, s1) == (4, 2) and step0 == (2 * v,) * 3 + (2.0,) * 3 and stop0 == 0.5 * v
    assert step1 == (0.5 * v,) * 3 + (0.5,) * 3 and stop1 == v / 16
    assert G.effective_stride((40, 48, 36), 4) == 4 and G.effective_stride((32, 29, 64), 4) == 4
    with caplog.at_level("INFO"):
        assert G.effective_stride((40, 28, 36), 4) == 2 and G.effective_stride((9, 40, 40), 8) == 1
    assert "fewer than 8 samples" in caplog.text
    assert G.effective_stride((3, 3, 3), 2) == 1
    assert G.sample_count((40, 48, 36), 4) == 10 * 12 * 9 and G.sample_count((11, 7, 37), 2) == 6 * 4 * 19


def test_register_rigid_np_on_the_synthetic_pair():
    """The 40 x 48 x 36 pair of tests/registerutil.py, 32 bins: moved by 2.3 / -1.6 / 1.2 mm and 4 / -3 / 5 degrees (worst corner 6.6
    voxels off under the headers), contrast-inverted through a square root, noise.  The worst corner displacement between the found
    and the true transform must be at most ONE fixed voxel - the smallest voxel size, 0.9 mm, is taken.  The specification reaches
    0.25 voxels (parameters 2.3625, -1.575, 1.18125 mm; 3.875, -3.1875, 4.875 degrees) in 410 evaluations."""
    start = U.corner_error_voxels(np.eye(4))
    assert start > 5.0
    r = U.specification_result()
    err = U.corner_error_voxels(r.world)
    print(f"corner displacement {start:.3f} -> {err:.3f} voxels, p = {r.p.tolist()}, NMI {r.trace[0]['best']:.6f} -> {r.value:.6f}, "
          f"{r.n_evaluations} evaluations")
    assert err <= 1.0
    assert r.value > r.trace[0]["best"] and r.n_evaluations == sum(len(t["values"]) for t in r.trace)
    centre = G.volume_centre(U.FIXED_AFFINE, U.FIXED_SHAPE)
    assert np.array_equal(r.world, G.rigid_world(r.p, centre))
    assert np.array_equal(r.matrix, G.candidate_matrix(r.p, U.FIXED_AFFINE, U.MOVING_AFFINE, centre))
    assert [t["stride"] for t in r.trace if t["kind"] == "start"] == [4, 2]


def test_library_has_the_registration_entries():
    lib = _lib.load()
    for name in ("mrisr_f32_volume_joint_histogram", "mrisr_joint_histogram_nmi"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.mrisr_version() == _lib.ABI_VERSION >= 316


def test_cpu_tensors_raise():
    import torch
    v = torch.zeros((4, 4, 4), dtype=torch.float32)
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    with pytest.raises(ValueError):
        G.joint_histogram(v, v, eye, 16, 1, (0.0, 1.0), (0.0, 1.0))
    with pytest.raises(ValueError):
        G.nmi(torch.zeros((16, 16), dtype=torch.int64))
    with pytest.raises(ValueError):
        G.register_rigid(v, np.eye(4), v, np.eye(4))
