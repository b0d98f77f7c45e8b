"""CPU-only tests of the diffeomorphic variant of the deformable registration (mri_superresolution_amd/volume_deform.py, numpy part):
the composition of fields, the update-only force, the exponential, one interpolation through matrix and field, the registration,
the C entries' argument checks and the command-line choices."""
import functools
import os
import sys

import numpy as np
import pytest

from deformutil import PHANTOM_SHAPE, messy_volume, phantom, quality, same_bits, smooth_field
from mri_superresolution_amd import volume_deform as D
from mri_superresolution_amd.volume_reslice import reslice_np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def values(shape, seed):
    return messy_volume(shape, seed, specials=False)


# ---------------------------------------------------------------- compose_np

def test_composition_with_a_zero_field_is_the_other_field():
    u = smooth_field((5, 7, 9), 1)
    zero = np.zeros_like(u)
    assert same_bits(D.compose_np(u, zero), u)
    assert same_bits(D.compose_np(zero, u), u)


def test_composition_of_integer_translations_adds_them_and_continues_the_field_past_the_faces():
    """u is a ramp along axis 0, v a shift of +2 along it: inside the grid the result is v + u[i + 2], past the last plane the ramp
    stays at its last value (a zero fill would give v + 0 there)."""
    shape = (6, 3, 4)
    i = np.arange(6, dtype=np.float32).reshape(-1, 1, 1) + np.zeros(shape, dtype=np.float32)
    u = np.stack([10 + i, np.zeros(shape, np.float32), -i]).astype(np.float32)
    v = np.zeros_like(u)
    v[0] = 2.0
    want = v.copy()
    at = np.minimum(np.arange(6) + 2, 5)
    want[0] += u[0][at]
    want[2] += u[2][at]
    assert same_bits(D.compose_np(u, v), want)
    v[0] = -7.5                                     # every voxel points below the first plane: u's first plane everywhere
    want = v.copy()
    want[0] += u[0][0]
    want[2] += u[2][0]
    assert same_bits(D.compose_np(u, v), want)


def test_composition_documents_what_nan_and_infinite_displacements_do():
    """An infinite displacement is clamped onto a face like any other and leaves v + U infinite in its own component only; a NaN one
    makes all three components of that voxel NaN."""
    u = smooth_field((4, 5, 6), 2)
    v = np.zeros_like(u)
    v[0, 1, 1, 1], v[1, 2, 2, 2], v[2, 3, 3, 3], v[2, 0, 4, 5] = np.inf, -np.inf, np.nan, 1e9
    out = D.compose_np(u, v)
    want = u.copy()                                  # v is zero elsewhere
    want[:, 1, 1, 1] = [np.inf, u[1, 3, 1, 1], u[2, 3, 1, 1]]                   # x clamped to the last plane
    want[:, 2, 2, 2] = [u[0, 2, 0, 2], -np.inf, u[2, 2, 0, 2]]                  # y clamped to the first row
    want[:, 3, 3, 3] = np.nan
    want[:, 0, 4, 5] = [u[0, 0, 4, 5], u[1, 0, 4, 5], np.float32(1e9) + u[2, 0, 4, 5]]
    assert same_bits(out, want)


def test_two_warps_are_the_warp_through_the_composition_for_integer_fields():
    """warp(warp(m, u), v) = warp(m, compose(u, v)) exactly where no interpolation happens: integer displacements that stay inside."""
    m = values((7, 6, 8), 3)
    rng = np.random.default_rng(4)
    u = rng.integers(-1, 2, (3,) + m.shape).astype(np.float32)
    v = rng.integers(-1, 2, (3,) + m.shape).astype(np.float32)
    both = D.warp_np(D.warp_np(m, u, fill=-1.0), v, fill=-1.0)
    once = D.warp_np(m, D.compose_np(u, v), fill=-1.0)
    inner = (slice(2, -2),) * 3                      # two steps of one voxel never leave the grid from here
    i, j, k = (g[inner] for g in np.meshgrid(*(np.arange(n) for n in m.shape), indexing="ij"))
    y = [g + v[a][inner].astype(int) for a, g in enumerate((i, j, k))]
    z = [g + u[a][tuple(y)].astype(int) for a, g in enumerate(y)]
    assert same_bits(once[inner], m[tuple(z)]) and same_bits(both[inner], once[inner])


# ---------------------------------------------------------------- demons_update_np, exp_field_np

def test_the_update_is_the_force_without_the_field_and_scales_exactly():
    fixed, moving = values((6, 5, 7), 5), values((6, 5, 7), 6)
    u = smooth_field(fixed.shape, 7)
    zero = np.zeros_like(u)
    w, stats = D.demons_update_np(fixed, moving, zero, max_step=0.4, fill=2.0)
    v, stats_force = D.demons_force_np(fixed, moving, zero, max_step=0.4, fill=2.0)
    assert same_bits(w + np.float32(0), v) and stats == stats_force        # 0 + upd = upd; w may carry -0.0 where v has +0.0
    w1 = D.demons_update_np(fixed, moving, u, max_step=0.4, fill=2.0)[0]
    w4, stats4 = D.demons_update_np(fixed, moving, u, max_step=0.4, fill=2.0, scale=0.25)
    assert same_bits(w4, w1 * np.float32(0.25)) and np.abs(w4).max() <= 0.1
    assert stats4 == D.demons_force_np(fixed, moving, u, max_step=0.4, fill=2.0)[1]
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="scale"):
            D.demons_update_np(fixed, moving, u, scale=bad)


def test_the_exponential_of_zero_steps_is_the_field_and_steps_are_checked():
    w = smooth_field((5, 4, 6), 8)
    assert same_bits(D.exp_field_np(w, 0), w)
    half = w * np.float32(0.5)
    assert same_bits(D.exp_field_np(w, 1), D.compose_np(half, half))
    for bad in (-1, 9, 1.5, True):
        with pytest.raises(ValueError, match="exp_steps"):
            D.exp_field_np(w, bad)


def test_the_exponential_of_a_folding_velocity_does_not_fold():
    """v_0 = 6 sin(2 pi i / 32), v_1 = 0.5 cos(2 pi i / 32) on (32, 6, 5): read as a displacement it folds (its slope along axis 0
    reaches -1.18); its exponential is a diffeomorphism."""
    shape = (32, 6, 5)
    i = np.arange(32, dtype=np.float64).reshape(-1, 1, 1) + np.zeros(shape)
    v = np.zeros((3,) + shape, dtype=np.float32)
    v[0], v[1] = 6 * np.sin(2 * np.pi * i / 32), 0.5 * np.cos(2 * np.pi * i / 32)
    min_v, count_v = D.jacobian_stats_np(v)
    min_e, count_e = D.jacobian_stats_np(D.exp_field_np(v, 4))
    print(f"displacement: minimum {min_v:.4f}, {count_v} folded; exponential: minimum {min_e:.4f}, {count_e} folded")
    assert count_v > 0
    assert count_e == 0 and min_e > 0


# ---------------------------------------------------------------- warp_matrix_np

ROTATED = np.array([[0.9 * 0.8, -0.6 * 1.3, 0.0, 1.7], [0.9 * 0.6, 0.8 * 1.3, 0.05, -2.2], [0.02, 0.0, 0.5, 0.3]])


@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_one_interpolation_with_a_zero_field_is_the_reslice(method):
    src = values((9, 7, 5), 9)
    shape = (6, 8, 7)
    got = D.warp_matrix_np(src, ROTATED, np.zeros((3,) + shape, dtype=np.float32), method, fill=-2.0)
    want = reslice_np(src, ROTATED, shape, method, fill=-2.0)
    assert same_bits(got, want) and (want != -2.0).sum() > 20 and (want == -2.0).sum() > 20


@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_one_interpolation_with_the_identity_matrix_is_the_warp(method):
    src = values((6, 5, 7), 10)
    u = smooth_field(src.shape, 11, amplitude=2.0)
    u[0, 0, 0, 0], u[1, 1, 1, 1], u[2, 2, 2, 2] = np.nan, np.inf, -1e9
    identity = np.hstack([np.eye(3), np.zeros((3, 1))])
    assert same_bits(D.warp_matrix_np(src, identity, u, method, fill=4.0), D.warp_np(src, u, method, fill=4.0))


def test_one_interpolation_of_a_translation_and_a_constant_field_adds_them():
    src = values((8, 6, 9), 12)
    m = np.hstack([np.eye(3), np.array([[0.5], [-1.0], [0.25]])])
    u = np.broadcast_to(np.array([0.25, 0.5, -1.25], dtype=np.float32).reshape(3, 1, 1, 1), (3,) + src.shape).copy()
    total = np.hstack([np.eye(3), np.array([[0.75], [-0.5], [-1.0]])])        # sums that are exact either way
    assert same_bits(D.warp_matrix_np(src, m, u, "cubic", fill=1.0), reslice_np(src, total, src.shape, "cubic", fill=1.0))


# ---------------------------------------------------------------- the registration

def test_identical_scans_leave_the_field_exactly_zero():
    fixed = phantom()[0]
    r = D.register_diffeomorphic_np(fixed, fixed.copy(), levels=2, iterations=(3, 2))
    assert r.field.shape == (3,) + PHANTOM_SHAPE and not r.field.any()
    assert same_bits(r.warped, fixed) and r.jacobian == (1.0, 0)
    assert r.stats == [(0.0, 12 * 14 * 16)] * 3 + [(0.0, 24 * 28 * 32)] * 2


@functools.lru_cache(maxsize=None)
def registered(kind, noise, sigma):
    fixed, moving = phantom(noise)[:2]
    fn = D.register_diffeomorphic_np if kind == "diffeomorphic" else D.register_deformable_np
    return fn(fixed, moving, levels=2, iterations=(15, 10), sigma_vox=sigma)


def test_diffeomorphic_registration_recovers_the_phantoms_field():
    """Two levels, 15 and 10 iterations, sigma 1.5, exp_steps 2.  Measured with the specification on the CPU, inside the object:

        additive        intensity ratio 0.0982   end-point ratio 0.5194   minimum determinant 0.7487
        diffeomorphic   intensity ratio 0.0994   end-point ratio 0.5219   minimum determinant 0.7452

    The diffeomorphic intensity ratio is asserted with a margin of a quarter (for later edits of the phantom: the specification is
    deterministic)."""
    fixed, moving, truth, mask = phantom()
    r = registered("diffeomorphic", 0.0, 1.5)
    intensity, endpoint, min_det = quality(fixed, moving, truth, mask, r)
    print(f"intensity ratio {intensity:.4f}, end-point ratio {endpoint:.4f}, minimum determinant {min_det:.4f}")
    assert intensity < 1.25 * 0.0994
    assert r.jacobian[1] == 0 and min_det > 0 and len(r.stats) == 25
    assert r.stats[14][0] < r.stats[0][0] and r.stats[24][0] < r.stats[15][0]


@pytest.mark.parametrize("noise, sigma", [(0.0, 0.0), (10.0, 0.5)])
def test_where_the_additive_field_folds_the_diffeomorphic_one_does_not(noise, sigma):
    """The phantom with the schedule above and too little regularisation.  Measured with the specification on the CPU:

        noise 0, sigma 0      additive 36 voxels folded (minimum -3.447)   diffeomorphic 0 (minimum 0.058)
        noise 10, sigma 0.5   additive 4 voxels folded (minimum -0.363)    diffeomorphic 0 (minimum 0.412)"""
    additive, diffeo = registered("additive", noise, sigma), registered("diffeomorphic", noise, sigma)
    print(f"additive {additive.jacobian}, diffeomorphic {diffeo.jacobian}")
    assert additive.jacobian[1] > 0 and additive.jacobian[0] <= 0
    assert diffeo.jacobian[1] == 0 and diffeo.jacobian[0] > 0


def test_arguments_are_checked():
    v = np.zeros((4, 4, 4), dtype=np.float32)
    u = np.zeros((3, 4, 4, 4), dtype=np.float32)
    with pytest.raises(ValueError):
        D.compose_np(u, u[:, :3])
    with pytest.raises(ValueError):
        D.compose_np(u.astype(np.float64), u)
    with pytest.raises(ValueError, match="Unknown interpolation method"):
        D.warp_matrix_np(v, np.eye(4)[:3], u, "nearest")
    with pytest.raises(ValueError):
        D.warp_matrix_np(v, np.eye(3), u)
    with pytest.raises(ValueError, match="exp_steps"):
        D.register_diffeomorphic_np(v, v, exp_steps=9)
    with pytest.raises(ValueError):
        D.register_diffeomorphic_np(v, v[:3])


def test_device_functions_refuse_cpu_tensors_and_bad_steps():
    import torch
    v, u = torch.ones((3, 3, 3)), torch.zeros((3, 3, 3, 3))
    m = np.eye(4)[:3]
    for call in (lambda: D.compose(u, u), lambda: D.demons_update(v, v, u), lambda: D.exp_field(u, 2), lambda: D.warp_matrix(v, m, u),
                 lambda: D.register_diffeomorphic(v, v)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    for bad in (-1, 9, 2.0):
        with pytest.raises(ValueError, match="exp_steps"):
            D.register_diffeomorphic(v, v, exp_steps=bad)
        with pytest.raises(ValueError, match="exp_steps"):
            D.DiffeoWorkspace((4, 4, 4), "cpu", levels=1, iterations=1, exp_steps=bad)


# ---------------------------------------------------------------- the C side, without a GPU

def test_library_declares_the_entry_points_and_checks_their_arguments():
    import ctypes
    from mri_superresolution_amd import _lib
    lib = _lib.load()
    for name in ("mrisr_f32_volume_field_compose", "mrisr_f32_volume_demons_update", "mrisr_f32_volume_warp_matrix"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.mrisr_version() == _lib.ABI_VERSION >= 322
    ARG, SHAPE = -1, -2
    buf = (ctypes.c_float * 64)()                        # host memory: nothing is launched when a check fails
    p = ctypes.addressof(buf)
    q, r, w = p + 64, p + 128, p + 192
    m = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    lin = _lib.RESAMPLE_LINEAR
    assert lib.mrisr_f32_volume_field_compose(None, p, 1, 1, 1, q, None) == ARG
    assert lib.mrisr_f32_volume_field_compose(p, None, 1, 1, 1, q, None) == ARG
    assert lib.mrisr_f32_volume_field_compose(p, p, 1, 1, 1, None, None) == ARG
    assert lib.mrisr_f32_volume_field_compose(p, q, 1, 1, 1, p, None) == ARG
    assert lib.mrisr_f32_volume_field_compose(p, q, 1, 1, 1, q, None) == ARG
    assert b"of its own" in lib.mrisr_last_error()
    assert lib.mrisr_f32_volume_field_compose(p, p, 1, 1, 1, p + 2, None) == ARG             # misaligned
    assert lib.mrisr_f32_volume_field_compose(p, p, 1, 0, 1, q, None) == SHAPE
    assert lib.mrisr_f32_volume_field_compose(p, p, 65536, 32768, 1, q, None) == SHAPE       # 2^31 voxels
    assert b"2^31" in lib.mrisr_last_error()
    assert lib.mrisr_f32_volume_demons_update(p, p, p, 1, 1, 1, 2.0, 0.0, 0.25, None, w, None, None) == ARG
    assert lib.mrisr_f32_volume_demons_update(p, p, p, 1, 1, 1, 2.0, 0.0, 0.25, q, None, None, None) == ARG
    assert lib.mrisr_f32_volume_demons_update(None, p, p, 1, 1, 1, 2.0, 0.0, 0.25, q, w, None, None) == ARG
    assert lib.mrisr_f32_volume_demons_update(p, p, p, 1, 1, 1, -1.0, 0.0, 0.25, q, w, None, None) == ARG
    assert lib.mrisr_f32_volume_demons_update(p, p, p, 1, 1, 1, 2.0, 0.0, 0.0, q, w, None, None) == ARG
    assert lib.mrisr_f32_volume_demons_update(p, p, p, 1, 1, 1, 2.0, 0.0, float("nan"), q, w, None, None) == ARG
    assert b"scale" in lib.mrisr_last_error()
    assert lib.mrisr_f32_volume_demons_update(p, p, p, 1, 1, 1, 2.0, 0.0, 0.25, p, w, None, None) == ARG
    assert lib.mrisr_f32_volume_demons_update(p, p, p, 0, 1, 1, 2.0, 0.0, 0.25, q, w, None, None) == SHAPE
    assert lib.mrisr_f32_volume_demons_update(p, p, p, 2048, 2048, 512, 2.0, 0.0, 0.25, q, w, None, None) == SHAPE
    assert lib.mrisr_f32_volume_demons_force(p, p, p, 1, 1, 1, 2.0, 0.0, p, w, None, None) == ARG      # the sibling, as before
    assert b"f32_volume_demons_force: v must be a buffer of its own" in lib.mrisr_last_error()
    assert lib.mrisr_f32_volume_warp_matrix(None, 1, 1, 1, q, 1, 1, 1, m, lin, 0.0, r, None) == ARG
    assert lib.mrisr_f32_volume_warp_matrix(p, 1, 1, 1, None, 1, 1, 1, m, lin, 0.0, r, None) == ARG
    assert lib.mrisr_f32_volume_warp_matrix(p, 1, 1, 1, q, 1, 1, 1, None, lin, 0.0, r, None) == ARG
    assert lib.mrisr_f32_volume_warp_matrix(p, 1, 1, 1, q, 1, 1, 1, m, lin, 0.0, None, None) == ARG
    assert lib.mrisr_f32_volume_warp_matrix(p, 1, 1, 1, q, 1, 1, 1, m, _lib.RESAMPLE_NEAREST, 0.0, r, None) == ARG
    assert lib.mrisr_f32_volume_warp_matrix(p, 1, 1, 1, q, 1, 1, 1, m, 77, 0.0, r, None) == ARG
    assert lib.mrisr_f32_volume_warp_matrix(p, 1, 1, 1, q, 1, 1, 1, m, lin, 0.0, p, None) == ARG
    assert lib.mrisr_f32_volume_warp_matrix(p, 1, 1, 1, q, 1, 1, 1, m, lin, 0.0, q, None) == ARG
    m[5] = float("inf")
    assert lib.mrisr_f32_volume_warp_matrix(p, 1, 1, 1, q, 1, 1, 1, m, lin, 0.0, r, None) == ARG
    assert b"not finite" in lib.mrisr_last_error()
    m[5] = 1.0
    assert lib.mrisr_f32_volume_warp_matrix(p, 1, 0, 1, q, 1, 1, 1, m, lin, 0.0, r, None) == SHAPE
    assert lib.mrisr_f32_volume_warp_matrix(p, 1, 1, 1, q, 1, 1, -3, m, lin, 0.0, r, None) == SHAPE
    assert lib.mrisr_f32_volume_warp_matrix(p, 65536, 32768, 1, q, 1, 1, 1, m, lin, 0.0, r, None) == SHAPE
    assert lib.mrisr_f32_volume_warp_matrix(p, 1, 1, 1, q, 2048, 2048, 512, m, lin, 0.0, r, None) == SHAPE


# ---------------------------------------------------------------- the command lines

def test_register_volume_parses_the_new_choices_and_keeps_its_defaults():
    from scripts import register_volume as cli
    base = ["--fixed", "f.nii", "--moving", "m.nii", "--output", "o.nii"]
    args = cli.parse_args(base)
    assert (args.nonrigid, args.nonrigid_exp_steps, args.nonrigid_resample) == ("none", 2, "twice")
    args = cli.parse_args(base + ["--nonrigid", "diffeomorphic", "--nonrigid_exp_steps", "3", "--nonrigid_resample", "once"])
    assert (args.nonrigid, args.nonrigid_exp_steps, args.nonrigid_resample) == ("diffeomorphic", 3, "once")
    assert cli.parse_args(base + ["--nonrigid", "demons", "--nonrigid_resample", "once"]).nonrigid_resample == "once"
    for bad in (["--nonrigid", "syn"], ["--nonrigid_resample", "thrice"], ["--nonrigid_exp_steps", "two"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    cli.check_options()
    cli.check_options("demons", 2, "once", "field.nii")
    cli.check_options("diffeomorphic", 0, "twice")
    with pytest.raises(ValueError, match="--nonrigid_resample once goes with --nonrigid"):
        cli.check_options("none", 2, "once")
    with pytest.raises(ValueError, match="--save_field goes with --nonrigid"):
        cli.check_options("none", 2, "twice", "field.nii")
    with pytest.raises(ValueError, match="--nonrigid_exp_steps"):
        cli.check_options("diffeomorphic", 9)
    with pytest.raises(ValueError, match="--nonrigid must be"):
        cli.check_options("syn")


def test_register_volume_refuses_one_resampling_without_a_field_before_it_reads_a_file(tmp_path):
    from scripts import register_volume as cli
    with pytest.raises(ValueError, match="--nonrigid_resample once goes with --nonrigid"):
        cli.register_file(str(tmp_path / "no_fixed.nii"), str(tmp_path / "no_moving.nii"), str(tmp_path / "out.nii"), nonrigid_resample="once")
    assert not os.path.exists(tmp_path / "out.nii")


def test_evaluate_volume_parses_the_new_choices_and_keeps_its_rules():
    from scripts import evaluate_volume as cli
    args = cli.parse_args(["--reference", "r.nii"])
    assert (args.deform_input, args.deform_exp_steps) == ("none", 2)
    args = cli.parse_args(["--reference", "r.nii", "--input", "i.nii", "--deform_input", "diffeomorphic", "--deform_exp_steps", "4"])
    assert (args.deform_input, args.deform_exp_steps) == ("diffeomorphic", 4)
    with pytest.raises(SystemExit):
        cli.parse_args(["--reference", "r.nii", "--deform_input", "syn"])
    cli.check_options("i.nii", None, "linear", "header", "none", "none", deform_input="diffeomorphic", deform_exp_steps=4)
    cli.check_options("i.nii", None, "linear", "header", "none", "none", "none", 25.0, "none", None, 1.0, 3, "demons")     # as before
    with pytest.raises(ValueError, match="goes with --input"):
        cli.check_options(None, None, "linear", "header", "none", "none", deform_input="diffeomorphic")
    with pytest.raises(ValueError, match="--deform_exp_steps"):
        cli.check_options("i.nii", None, "linear", "header", "none", "none", deform_input="diffeomorphic", deform_exp_steps=9)
    with pytest.raises(ValueError, match="--deform_input is"):
        cli.check_options("i.nii", None, "linear", "header", "none", "none", deform_input="syn")
