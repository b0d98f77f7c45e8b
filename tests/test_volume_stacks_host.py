"""Reconstruction from orthogonal stacks, the host side (no GPU): the numpy specification of
mri_superresolution_amd/volume_stacks.py on hand cases, its quality on the phantom of tests/stackutil.py, the grid helpers and the
argument checks of the C entry points."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import stackutil as U                                                        # noqa: E402
from mri_superresolution_amd import volume_stacks as S                       # noqa: E402
from mri_superresolution_amd.utils.nifti import grid_matrix                  # noqa: E402

# RMSE against the truth after 10 iterations over the initial estimate's, thickness factors 2, 3, 4, measured with this
# specification on the CPU (numpy 1.26); asserted with a margin of 5 % of the value: the specification is deterministic, the margin
# covers other numpy builds
MEASURED_RATIOS = {2: 0.0196, 3: 0.0707, 4: 0.1058}


def identity_geometry(samples=1):
    return S.stack_geometry(np.diag([1.0, 1.0, 2.0, 1.0]), np.diag([1.0, 1.0, 2.0, 1.0]), 2, samples=samples)


# ---------------------------------------------------------------- the profile and the grid helpers

def test_profile_weights_sum_to_one_are_symmetric_and_one_sample_is_a_delta():
    for profile in S.PROFILES:
        for T in range(1, 17):
            for rho in (1.0, 0.8, 1.3):
                o, w = S.slice_profile(profile, T, rho)
                assert o.dtype == np.float64 and w.dtype == np.float32 and o.shape == w.shape == (T,)
                assert abs(w.astype(np.float64).sum() - 1.0) <= T * 2.0 ** -25          # half a float32 spacing below 1 per weight
                assert np.array_equal(w, w[::-1]) and np.array_equal(o, -o[::-1]) and (np.diff(o) > 0).all()
                assert np.abs(o).max() <= (rho if profile == "gaussian" else rho / 2)
        o, w = S.slice_profile(profile, 1, 1.7)
        assert o.tolist() == [0.0] and w.tolist() == [1.0]
    o, w = S.slice_profile("box", 4, 2.0)
    assert np.allclose(o, [-0.75, -0.25, 0.25, 0.75]) and w.tolist() == [0.25] * 4
    o, w = S.slice_profile("gaussian", 3, 1.0)
    assert o.tolist() == [-1.0, 0.0, 1.0] and abs(w[0] / w[1] - 2.0 ** -4) < 1e-6       # the FWHM is the thickness: 1/2 at 0.5, 1/16 at 1
    for bad in (dict(profile="sinc"), dict(samples=0), dict(samples=17), dict(samples=2.0), dict(rho=0.0), dict(rho=np.inf)):
        with pytest.raises(ValueError):
            S.slice_profile(**bad)
    assert S.default_profile_samples("box", 5.0, 1.5) == 4 and S.default_profile_samples("gaussian", 5.0, 1.5) == 7
    assert S.default_profile_samples("box", 0.5, 1.5) == 1 and S.default_profile_samples("box", 50.0, 1.0) == 16


def test_default_slice_axis_and_its_tie():
    assert S.default_slice_axis(np.diag([1.5, 1.5, 5.0, 1.0])) == 2
    assert S.default_slice_axis(np.diag([1.5, 4.0, 1.5, 1.0])) == 1
    a = np.eye(4)
    a[:3, :3] = U.rotation(10, 20, 30) @ np.diag([5.0, 1.0, 1.2])
    assert S.default_slice_axis(a) == 0
    for tie in (np.eye(4), np.diag([1.0, 5.0, 5.0, 1.0])):
        with pytest.raises(ValueError, match="--slice_axis"):
            S.default_slice_axis(tie)


def test_default_output_grid_is_the_bounding_box_in_the_first_stacks_orientation():
    out = np.diag([1.5, 1.5, 1.5, 1.0])
    out[:3, 3] = [-20.0, 5.0, 7.0]
    grids = [U.thick_grid((32, 36, 40), axis, 3, out) for axis in (2, 1, 0)]
    affine, shape = S.default_output_grid([g[0] for g in grids], [g[1] for g in grids])
    # the stacks' last slices hang out of the 32 x 36 x 40 grid: 11 x 3 = 33, 12 x 3 = 36, 14 x 3 = 42 voxels of 1.5 mm
    assert shape == (33, 36, 42) and np.allclose(affine, out)
    affine, shape = S.default_output_grid([g[0] for g in grids], [g[1] for g in grids], spacing=3.0)
    assert shape == (17, 18, 21) and np.allclose(S.voxel_sizes(affine), 3.0)
    assert np.allclose(affine @ [-0.5, -0.5, -0.5, 1.0], out @ [-0.5, -0.5, -0.5, 1.0])        # the corner stays
    rot = np.eye(4)
    rot[:3, :3] = U.rotation(0, 0, 90) @ np.diag([1.0, 1.0, 4.0])
    affine, shape = S.default_output_grid([rot, np.eye(4)], [(8, 6, 2), (4, 4, 4)])
    assert np.allclose(affine[:3, :3], U.rotation(0, 0, 90)) and np.allclose(S.voxel_sizes(affine), 1.0)
    corners = np.array([affine @ [i, j, k, 1.0] for i in (-0.5, shape[0] - 0.5) for j in (-0.5, shape[1] - 0.5) for k in (-0.5, shape[2] - 0.5)])
    for a, n in ((rot, (8, 6, 2)), (np.eye(4), (4, 4, 4))):
        theirs = np.array([a @ [i, j, k, 1.0] for i in (-0.5, n[0] - 0.5) for j in (-0.5, n[1] - 0.5) for k in (-0.5, n[2] - 0.5)])
        assert (theirs.min(0) >= corners.min(0) - 1e-9).all() and (theirs.max(0) <= corners.max(0) + 1e-9).all()
    with pytest.raises(ValueError):
        S.default_output_grid([np.eye(4)], [(4, 4, 4)], spacing=-1.0)
    with pytest.raises(ValueError):
        S.default_output_grid([np.eye(4)], [])


def test_stack_geometry_folds_a_world_transform_into_both_matrices():
    out, a = np.eye(4), np.diag([1.0, 1.0, 4.0, 1.0])
    world = np.eye(4)
    world[:3, 3] = [0.0, 2.0, 0.0]
    g = S.stack_geometry(a, out, world=world)
    assert g.slice_axis == 2 and g.offsets.size == 4
    assert np.allclose(g.from_output, grid_matrix(a, world @ out)) and np.allclose(g.from_output[:, 3], [0.0, 2.0, 0.0])
    full = np.vstack([g.to_output, [0, 0, 0, 1]]) @ np.vstack([g.from_output, [0, 0, 0, 1]])
    assert np.allclose(full, np.eye(4))
    with pytest.raises(ValueError, match="--slice_axis"):
        S.stack_geometry(np.eye(4), out)
    for bad in (dict(slice_axis=3), dict(slice_axis=True), dict(thickness_mm=0.0), dict(samples=17)):
        with pytest.raises(ValueError):
            S.stack_geometry(a, out, **bad)


# ---------------------------------------------------------------- hand cases of the specification

def test_a_stack_on_the_output_grid_is_a_fixed_point():
    rng = np.random.default_rng(3)
    y = rng.uniform(0.0, 900.0, (5, 6, 7)).astype(np.float32)
    g = identity_geometry()
    got = S.combine_stacks_np([y], [g], y.shape, iterations=3)
    assert U.same_bits(got.initial, y) and U.same_bits(got.volume, y)
    r, (s, n) = S.stack_residual_np(got.initial, y, g)
    assert not r.any() and not np.signbit(r).any() and (s, n) == (0.0, y.size)
    assert not got.rms.any() and (got.counts == y.size).all() and got.coverage.tolist() == [0, y.size]


@pytest.mark.parametrize("oblique", [False, True], ids=["aligned", "oblique"])
def test_the_residual_at_the_truth_is_exactly_zero(oblique):
    x = U.phantom()
    if oblique:
        shape = (20, 24, 9)
        a = U.oblique_affine(x.shape, shape, (1.5, 1.5, 4.0))
    else:
        a, shape = U.thick_grid(x.shape, 1, 3)
    g = S.stack_geometry(a, np.eye(4), samples=4)
    y = S.simulate_stack_np(x, g, shape)
    r, (s, n) = S.stack_residual_np(x, y, g)
    assert not r.any() and s == 0.0 and 0 < n <= y.size and (y[r == 0].max() > 600)


def test_a_constant_volume_is_reproduced():
    truth = np.full((12, 15, 17), np.float32(417.3))          # 17 = 5 slices of 3 and one with two of its three samples inside
    stacks, geometries, _ = U.orthogonal_stacks(truth, 3)
    got = S.combine_stacks_np(stacks, geometries, truth.shape, iterations=4)
    assert np.abs(got.volume / np.float32(417.3) - 1.0).max() <= 1e-6 and np.abs(got.initial / np.float32(417.3) - 1.0).max() <= 1e-6


def test_uncovered_voxels_keep_the_fill_and_single_coverage_counts_once():
    out_shape = (8, 8, 8)
    y0, y1 = np.full((4, 8, 8), np.float32(100)), np.full((8, 4, 8), np.float32(300))
    g0 = S.stack_geometry(np.eye(4), np.eye(4), 0, samples=1)                           # covers x < 3.5
    a1 = np.eye(4)
    a1[1, 3] = 4.0                                                                      # covers y > 3.5
    g1 = S.stack_geometry(a1, np.eye(4), 1, samples=1)
    x, cnt = S.stack_update_np(np.full(out_shape, np.float32(-7)), [y0, y1], [g0, g1], 1.0, clamp=0.0)
    assert (cnt[:4, :4] == 1).all() and (cnt[:4, 4:] == 2).all() and (cnt[4:, :4] == 0).all() and (cnt[4:, 4:] == 1).all()
    assert (x[4:, :4] == -7).all()                                                      # not covered: neither stepped nor clamped
    assert (x[:4, :4] == 93).all() and (x[4:, 4:] == 293).all() and (x[:4, 4:] == 193).all()
    got = S.combine_stacks_np([y0, y1], [g0, g1], out_shape, iterations=3, fill=-7.0)
    assert (got.volume[4:, :4] == -7).all() and (got.initial[4:, :4] == -7).all() and got.coverage.tolist() == [128, 256, 128]
    assert (got.initial[:4, :4] == 93).all() and (got.initial[:4, 4:] == 193).all()
    assert (S.stack_update_np(np.full(out_shape, np.float32(-7)), [y0 - 200], [g0], 1.0, clamp=None)[0][:4] == -107).all()
    assert (S.stack_update_np(np.full(out_shape, np.float32(-7)), [y0 - 200], [g0], 1.0, clamp=0.0)[0][:4] == 0).all()


def test_the_weight_sum_rule_at_the_edge_of_the_field_of_view():
    x = np.arange(6, dtype=np.float32).reshape(1, 1, 6) * 10 + 10            # 10 .. 60 along z
    a = np.diag([1.0, 1.0, 4.0, 1.0])
    a[2, 3] = 1.5 + 1.0                                                      # slice 0 covers z -0.5 .. 3.5 moved by one: 0.5 .. 4.5
    g = S.stack_geometry(a, np.eye(4), 2, samples=4)
    assert np.allclose(g.offsets * 4, [-1.5, -0.5, 0.5, 1.5])
    # slice 0: samples at z = 1, 2, 3, 4 all inside; slice 1: z = 5 inside, 6, 7, 8 outside (wsum 0.25: no residual);
    # slice -1 does not exist.  A stack moved so that two samples of slice 1 are inside passes the test with wsum = 0.5
    y = np.array([35.0, 99.0], dtype=np.float32).reshape(1, 1, 2)
    sim = S.simulate_stack_np(x, g, (1, 1, 2), fill=-1.0)
    assert sim.reshape(-1).tolist() == [35.0, -1.0]
    r, (s, n) = S.stack_residual_np(x, y, g)
    assert r.reshape(-1).tolist() == [0.0, 0.0] and (s, n) == (0.0, 1)
    a[2, 3] = 1.5
    g = S.stack_geometry(a, np.eye(4), 2, samples=4)                         # slice 1: z = 4, 5 inside, 6, 7 outside: wsum = 0.5
    sim = S.simulate_stack_np(x, g, (1, 1, 2), fill=-1.0)
    assert sim.reshape(-1).tolist() == [25.0, 55.0]
    r, (s, n) = S.stack_residual_np(x, y, g)
    assert r.reshape(-1).tolist() == [10.0, 44.0] and (s, n) == (100.0 + 44.0 * 44.0, 2)


def test_arguments_are_checked():
    x = np.zeros((4, 4, 4), dtype=np.float32)
    g = identity_geometry()
    with pytest.raises(ValueError, match="float32"):
        S.stack_residual_np(x.astype(np.float64), x, g)
    with pytest.raises(ValueError, match="StackGeometry"):
        S.stack_residual_np(x, x, (g.to_output, g.from_output))
    with pytest.raises(ValueError, match="slice axis"):
        S.stack_residual_np(x, x, g._replace(slice_axis=3))
    with pytest.raises(ValueError, match="profile"):
        S.stack_residual_np(x, x, g._replace(weights=g.weights.astype(np.float64)))
    with pytest.raises(ValueError, match="not finite"):
        S.stack_residual_np(x, x, g._replace(offsets=np.array([np.nan])))
    with pytest.raises(ValueError, match="finite"):
        S.stack_residual_np(x, x, g._replace(to_output=np.full((3, 4), np.inf)))
    with pytest.raises(ValueError, match="1..8 stacks"):
        S.stack_update_np(x, [x] * 9, [g] * 9)
    with pytest.raises(ValueError, match="1..8 stacks"):
        S.combine_stacks_np([], [], x.shape)
    with pytest.raises(ValueError, match="geometries"):
        S.stack_update_np(x, [x, x], [g])
    for bad in (dict(step=np.nan), dict(clamp=np.inf)):
        with pytest.raises(ValueError, match="finite"):
            S.stack_update_np(x, [x], [g], **bad)
    with pytest.raises(ValueError, match="iterations"):
        S.combine_stacks_np([x], [g], x.shape, iterations=-1)
    with pytest.raises(ValueError, match="CUDA tensor"):
        import torch
        S.combine_stacks([torch.zeros(4, 4, 4)], [g], x.shape)


# ---------------------------------------------------------------- quality

@functools.lru_cache(maxsize=None)
def errors(factor, noise):
    truth = U.phantom()
    stacks, geometries, _ = U.orthogonal_stacks(truth, factor, noise=noise, seed=factor)
    out = []
    S.combine_stacks_np(stacks, geometries, truth.shape, iterations=10, on_iteration=lambda it, x: out.append(U.rmse(x, truth)))
    return out


@pytest.mark.parametrize("factor", [2, 3, 4])
def test_the_reconstruction_beats_the_initial_estimate_at_every_iteration(factor):
    e = errors(factor, 0.0)
    print(f"factor {factor}: RMSE {e[0]:.3f} -> {e[10]:.3f}, ratio {e[10] / e[0]:.4f}; per iteration {[round(v / e[0], 4) for v in e]}")
    assert len(e) == 11 and e[10] < e[0]
    assert all(b <= a for a, b in zip(e, e[1:]))
    assert abs(e[10] / e[0] - MEASURED_RATIOS[factor]) <= 0.05 * MEASURED_RATIOS[factor]


@pytest.mark.parametrize("factor", [2, 3, 4])
def test_with_noise_the_fifth_iterate_beats_the_initial_estimate(factor):
    """Noise of sigma 20: the error is lowest after two or three iterations and rises slowly afterwards (semi-convergence, there is
    no regulariser); only iteration 5 against the initial estimate is asserted."""
    e = errors(factor, 20.0)
    print(f"factor {factor}, sigma 20: ratio at iteration 5 {e[5] / e[0]:.4f}, lowest at {int(np.argmin(e))}; {[round(v / e[0], 4) for v in e]}")
    assert e[5] < e[0]


# ---------------------------------------------------------------- the library

def test_library_declares_the_entry_points_and_checks_their_arguments():
    from mri_superresolution_amd import _lib
    lib = _lib.load()
    names = ("mrisr_f32_volume_stack_workspace_bytes", "mrisr_f32_volume_stack_residual", "mrisr_f32_volume_stack_update")
    with open(os.path.join(REPO, "include", "mrisr.h")) as f:
        header = f.read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and f" {name}(" in header
    assert lib.mrisr_version() == _lib.ABI_VERSION >= 328
    assert ctypes.sizeof(_lib.StackView) == 120
    region = lib.mrisr_f32_volume_stack_workspace_bytes(1)
    assert region == lib.mrisr_f32_volume_deform_workspace_bytes() and lib.mrisr_f32_volume_stack_workspace_bytes(8) == 8 * region
    assert lib.mrisr_f32_volume_stack_workspace_bytes(0) == 0 and lib.mrisr_f32_volume_stack_workspace_bytes(9) == 0
    ARG, SHAPE = -1, -2
    buf = (ctypes.c_uint64 * 64)()                       # host memory: nothing is launched when a check fails
    p = ctypes.addressof(buf)
    q, r, w = p + 64, p + 128, p + 256
    eye = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    off, wt = (ctypes.c_double * 16)(), (ctypes.c_float * 16)(*([1.0] * 16))
    ok = [p, 1, 1, 1, q, 1, 1, 1, eye, 2, off, wt, 1, r, w, None, None]

    def residual(**changed):
        args = list(ok)
        for i, v in changed.items():
            args[int(i[1:])] = v
        return lib.mrisr_f32_volume_stack_residual(*args)

    for i in (0, 4, 8, 10, 11, 13, 14):
        assert residual(**{f"a{i}": None}) == ARG
    assert b"null pointer" in lib.mrisr_last_error()
    for bad in (dict(a12=0), dict(a12=17), dict(a9=-1), dict(a9=3), dict(a13=p), dict(a13=q), dict(a0=p + 2), dict(a14=w + 4), dict(a15=w + 4)):
        assert residual(**bad) == ARG
    for bad in (dict(a1=0), dict(a7=0), dict(a6=-1), dict(a1=65536, a2=32768), dict(a5=65536, a6=32768)):
        assert residual(**bad) == SHAPE
    nan_m = (ctypes.c_double * 12)(*([float("nan")] + [0.0] * 11))
    inf_o, nan_w = (ctypes.c_double * 16)(float("inf")), (ctypes.c_float * 16)(float("nan"))
    assert residual(a8=nan_m) == ARG and residual(a10=inf_o) == ARG and residual(a11=nan_w) == ARG
    assert b"not finite" in lib.mrisr_last_error()

    def view(data=q, n=(1, 1, 1), m=None):
        v = _lib.StackView()
        v.data, (v.nx, v.ny, v.nz) = data, n
        v.m[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] if m is None else m
        return v

    def update(views, x=p, shape=(1, 1, 1), K=None, step=1.0, use=1, lo=0.0, out=r, cover=None, ws=None, rows=None):
        arr = (_lib.StackView * max(len(views), 1))(*views)
        return lib.mrisr_f32_volume_stack_update(x, *shape, arr if views else None, len(views) if K is None else K, step, use, lo, out, cover,
                                                 ws, rows, None)

    assert update([view()], x=None) == ARG and update([view()], out=None) == ARG and update([]) == ARG
    assert update([view()], K=0) == ARG and update([view()] * 8, K=9) == ARG
    assert update([view(data=None)]) == ARG and update([view(data=q + 2)]) == ARG and update([view(data=r)]) == ARG
    assert update([view()], step=float("nan")) == ARG and update([view()], lo=float("inf")) == ARG and update([view()], use=2) == ARG
    assert update([view(m=[float("inf")] + [0.0] * 11)]) == ARG
    assert update([view()], ws=w) == ARG and update([view()], rows=w) == ARG
    assert b"go together" in lib.mrisr_last_error()
    assert update([view()], cover=p) == ARG and update([view()], cover=r) == ARG and update([view()], cover=q) == ARG
    assert update([view()], shape=(0, 1, 1)) == SHAPE and update([view(n=(1, 0, 1))]) == SHAPE
    assert update([view()], shape=(65536, 32768, 1)) == SHAPE and update([view(n=(65536, 32768, 1))]) == SHAPE
