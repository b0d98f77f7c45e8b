"""Edge sharpness, the host side (no GPU): the numpy specification of mri_superresolution_amd/volume_sharpness.py on hand cases and
against a brute-force loop, ``edge_width`` on synthetic profiles, the phantom of tests/edgeutil.py, the argument checks of the C
entry points and the command lines."""
import math
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import edgeutil as E                                                         # noqa: E402
from mri_superresolution_amd import volume_sharpness as V                    # noqa: E402


# ---------------------------------------------------------------- sides and signed distance

def test_interface_sides_on_every_label():
    labels = np.arange(8, dtype=np.uint8).reshape(2, 2, 2)
    got = V.interface_sides_np(labels, 3)
    assert got.dtype == np.uint8 and got.reshape(-1).tolist() == [0, 1, 1, 1, 2, 2, 2, 2]
    assert V.interface_sides_np(labels, 1).reshape(-1).tolist() == [0, 1, 2, 2, 2, 2, 2, 2]
    for bad in (0, 255, True, 1.0):
        with pytest.raises(ValueError, match="k must be"):
            V.interface_sides_np(labels, bad)
    with pytest.raises(ValueError, match="uint8"):
        V.interface_sides_np(labels.astype(np.int32), 1)


def _plane():
    labels = np.zeros((8, 3, 2), dtype=np.uint8)
    labels[:4] = 1
    labels[4:] = 2
    return labels


def test_signed_distance_of_a_plane_interface():
    s = V.signed_distance_np(_plane(), 1)
    assert s.dtype == np.float32
    for x, want in enumerate((-4, -3, -2, -1, 1, 2, 3, 4)):            # between voxel centres: no voxel has |s| < 1
        assert (s[x] == want).all()
    s = V.signed_distance_np(_plane(), 1, (0.8, 1, 2.5))
    step = np.float32(0.8 * 0.8)                                       # the squared voxel size: a float64 product, rounded once
    for x, d in enumerate((4, 3, 2, 1, 1, 2, 3, 4)):
        want = np.sqrt(np.float32(step * np.float32(d * d)))
        assert (np.abs(s[x]) == want).all() and (np.sign(s[x]) == (-1 if x < 4 else 1)).all()
    across = np.transpose(_plane(), (2, 1, 0)).copy()                  # the interface across the axis of 2.5
    s = V.signed_distance_np(across, 1, (0.8, 1, 2.5))
    assert (s[:, :, 3] == -2.5).all() and (s[:, :, 4] == 2.5).all() and (s[:, :, 7] == 10.0).all()


def test_signed_distance_of_an_absent_side_and_of_label_zero():
    labels = _plane()
    labels[0, 0, 0] = 0
    labels[7, 2, 1] = 0
    s = V.signed_distance_np(labels, 1)
    assert np.isnan(s[0, 0, 0]) and np.isnan(s[7, 2, 1]) and np.isnan(s).sum() == 2
    assert s[1, 0, 0] == -3 and s[6, 2, 1] == 3                        # label 0 is no site of either side
    s = V.signed_distance_np(labels, 2)                                # nothing above 2: side 2 is absent
    assert np.isneginf(s[labels != 0]).all() and np.isnan(s[labels == 0]).all()
    only_bright = np.where(labels != 0, 2, 0).astype(np.uint8)
    s = V.signed_distance_np(only_bright, 1)
    assert np.isposinf(s[labels != 0]).all() and np.isnan(s[labels == 0]).all()
    with pytest.raises(ValueError, match="voxel sizes"):
        V.signed_distance_np(labels, 1, (1, 0, 1))
    with pytest.raises(ValueError, match="limit of 1024"):
        V.signed_distance_np(np.ones((1, 1, 1025), np.uint8), 1)


# ---------------------------------------------------------------- the profile

def test_edge_profile_equals_a_brute_force_loop():
    rng = np.random.default_rng(3)
    shape = (5, 4, 6)
    vol = rng.normal(100.0, 40.0, shape).astype(np.float32)
    sdist = rng.uniform(-3.0, 3.0, (2,) + shape).astype(np.float32)
    sdist[0].reshape(-1)[::7] = np.nan
    sdist[1].reshape(-1)[::5] = np.inf
    sdist[1].reshape(-1)[3::11] = -np.inf
    sdist[0, 0, 0, 1] = -2.0                                           # exactly the lower edge of bin 0
    sdist[0, 0, 0, 2] = 2.0                                            # exactly the upper edge of the range: outside
    vol[1, 1, 1] = np.nan
    vol[2, 2, 2] = np.inf
    for radius, width in ((2.0, 0.5), (2.0, 0.3), (1.0, 1.0)):
        got = V.edge_profile_np(vol, sdist, radius, width)
        want = E.brute_profile(vol, sdist, radius, width)
        nb = math.ceil(2 * radius / width)
        assert got.count.dtype == np.int64 and got.count.shape == (2, nb) and got.sum_v.dtype == np.float64
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        assert got.count.sum() > 40
    assert V.edge_profile_np(vol, sdist, 2.0, 0.5).count[0, 0] >= 1


def test_edge_profile_checks_its_arguments():
    vol, sdist = np.zeros((2, 3, 4), np.float32), np.zeros((1, 2, 3, 4), np.float32)
    V.edge_profile_np(vol, sdist, 4.0, 0.125)                          # 64 bins
    with pytest.raises(ValueError, match="65 bins"):
        V.edge_profile_np(vol, sdist, 4.0625, 0.125)
    with pytest.raises(ValueError, match="1 bins"):
        V.edge_profile_np(vol, sdist, 1.0, 2.0)
    for radius, width in ((0.0, 0.5), (4.0, -1.0), (float("nan"), 0.5), (4.0, float("inf")), ("x", 0.5)):
        with pytest.raises(ValueError, match="finite positive"):
            V.edge_profile_np(vol, sdist, radius, width)
    with pytest.raises(ValueError, match="signed distances"):
        V.edge_profile_np(vol, sdist[0])
    with pytest.raises(ValueError, match="signed distances"):
        V.edge_profile_np(vol, np.zeros((6, 2, 3, 4), np.float32))
    with pytest.raises(ValueError, match="signed distances"):
        V.edge_profile_np(vol, sdist.astype(np.float64))
    with pytest.raises(ValueError, match="float32 volume"):
        V.edge_profile_np(vol.astype(np.float64), sdist)


# ---------------------------------------------------------------- the width

def _profile(x, m, count=10):
    """One interface whose bins have the abscissae x and the means m."""
    c = np.full((1, len(x)), count, dtype=np.int64)
    x, m = np.asarray(x, dtype=np.float64)[None], np.asarray(m, dtype=np.float64)[None]
    return V.EdgeProfile(c, m * c, x * c, m * m * c)


def test_edge_width_of_a_linear_ramp():
    x = np.arange(16) * 0.5 - 3.75
    m = 100.0 + 800.0 * np.clip((x + 2.0) / 4.0, 0.0, 1.0)             # from 100 at -2 to 900 at +2: 10 % at -1.6, 90 % at +1.6
    width, contrast = V.edge_width(_profile(x, m))
    assert contrast[0] == 800.0 and abs(width[0] - 3.2) <= 1e-12
    over = m.copy()
    over[12] = 1000.0                                                  # overshoot: p = 1.125 at x = 2.25, past the crossing
    w_over, c_over = V.edge_width(_profile(x, over))
    assert c_over[0] == 800.0 and abs(w_over[0] - 3.2) <= 1e-12
    # a steeper ramp, from -1.5 to +1.5: both bins of either crossing lie on it, so the interpolation is exact again
    steep = V.edge_width(_profile(x, 100.0 + 800.0 * np.clip((x + 1.5) / 3.0, 0.0, 1.0)))[0]
    assert abs(steep[0] - 2.4) <= 1e-12
    two = V.EdgeProfile(*(np.concatenate([a, b]) for a, b in zip(_profile(x, m), _profile(x, over))))
    assert np.allclose(V.edge_width(two)[0], [3.2, 3.2], rtol=0, atol=1e-12)


def test_edge_width_is_nan_where_it_is_undefined():
    x = np.arange(16) * 0.5 - 3.75
    ramp = 100.0 + 800.0 * np.clip((x + 2.0) / 4.0, 0.0, 1.0)
    width, contrast = V.edge_width(_profile(x, ramp[::-1].copy()))     # falling: the contrast is negative
    assert np.isnan(width[0]) and contrast[0] == -800.0
    width, contrast = V.edge_width(_profile(x, np.full(16, 5.0)))
    assert np.isnan(width[0]) and contrast[0] == 0.0
    width, contrast = V.edge_width(_profile(x[:3], ramp[:3]))          # fewer than 4 bins
    assert np.isnan(width[0]) and np.isnan(contrast[0])
    width, contrast = V.edge_width(_profile(x, ramp, count=7))         # every bin below min_count
    assert np.isnan(width[0]) and np.isnan(contrast[0])
    assert abs(V.edge_width(_profile(x, ramp, count=7), min_count=7)[0][0] - 3.2) <= 1e-12
    # the dark plateau is two bins (n // 8) of which the first is bright: the walk starts at the first bin, and no crossing lies
    # to its left
    m = ramp.copy()
    m[0] = 900.0
    width, contrast = V.edge_width(_profile(x, m))
    assert np.isnan(width[0]) and contrast[0] == 400.0
    some = _profile(x, ramp)
    some.count[0, 5] = 3                                               # a thin bin is skipped, its neighbours interpolate across it
    width, _ = V.edge_width(some)
    assert abs(width[0] - 3.2) <= 1e-12
    with pytest.raises(ValueError, match="min_count"):
        V.edge_width(some, 0)
    with pytest.raises(ValueError, match="\\(J, nb\\)"):
        V.edge_width((np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4)))


# ---------------------------------------------------------------- the phantom

# measured with the specification (true labels, radius 4, bin width 0.5), interfaces 1 and 2, sigma = 0, 0.75, 1, 1.5, 2
CLEAN_WIDTHS = ((1.7101, 3.1670, 4.4219, 5.7708, 6.0222), (1.7068, 2.9149, 3.5301, 5.2762, 5.7299))
NOISY_WIDTHS = ((1.7310, 3.1796, 4.5712, 5.8234, 6.0423), (1.7282, 2.9250, 3.5809, 5.3148, 5.7258))
NOISE_MARGIN = 0.07                        # the largest relative change measured is 3.4 % (interface 1, sigma 1); a factor 2


def test_widths_on_the_phantom_grow_with_the_blur():
    """Three nested spheres (radii 18.3 / 13.6 / 8.4 voxels on (40, 44, 48), intensities 300 / 600 / 900) blurred by a Gaussian of
    sigma 0, 0.75, 1, 1.5, 2 voxels: the specification's widths across the interfaces 1|2 and 2|3 are
    1.7101 < 3.1670 < 4.4219 < 5.7708 < 6.0222 and 1.7068 < 2.9149 < 3.5301 < 5.2762 < 5.7299, with noise of sigma 30 added
    1.7310 < 3.1796 < 4.5712 < 5.8234 < 6.0423 and 1.7282 < 2.9250 < 3.5809 < 5.3148 < 5.7258.  They are not 2.563 sigma: the shells
    are thin and the plateaus sit inside the blur; at sigma 0 the width is that of a step sampled between voxel centres."""
    labels = E.truth()
    sdist = np.stack([V.signed_distance_np(labels, k) for k in (1, 2)])
    assert np.isnan(sdist[:, labels == 0]).all() and np.nanmin(np.abs(sdist)) == 1.0
    found = {}
    for noise, recorded in ((0.0, CLEAN_WIDTHS), (E.PHANTOM_NOISE, NOISY_WIDTHS)):
        widths, contrasts = [], []
        for sigma in E.PHANTOM_SIGMAS:
            width, contrast = V.edge_width(V.edge_profile_np(E.phantom(sigma, noise), sdist, 4.0, 0.5))
            widths.append(width)
            contrasts.append(contrast)
        widths = np.array(widths).T                                    # (2 interfaces, 5 sigmas)
        print(noise, widths.tolist())
        assert np.isfinite(widths).all() and (np.diff(widths, axis=1) > 0).all(), widths
        assert np.allclose(widths, recorded, rtol=0, atol=1e-4)
        assert (np.array(contrasts) > 290.0).all()
        found[noise] = widths
    assert (np.abs(found[E.PHANTOM_NOISE] / found[0.0] - 1.0) <= NOISE_MARGIN).all()
    clean = V.edge_sharpness_np(E.phantom(0.0), labels, 3)
    assert clean.contrast.tolist() == [300.0, 300.0] and clean.profile.count.shape == (2, 16)
    assert np.array_equal(clean.width, found[0.0][:, 0])


# ---------------------------------------------------------------- the device entries without a device

def test_device_entries_refuse_cpu_tensors_and_bad_arguments():
    import torch
    labels = torch.from_numpy(np.array(E.truth((4, 5, 6))))
    vol, sdist = torch.zeros(4, 5, 6), torch.zeros(2, 4, 5, 6)
    for call in (lambda: V.interface_sides(labels, 1), lambda: V.signed_distance(labels, 1), lambda: V.signed_distances(labels, 3),
                 lambda: V.edge_profile(vol, sdist), lambda: V.edge_sharpness(vol, labels), lambda: V.edge_sharpness(vol, sdist=sdist),
                 lambda: V.EdgeWorkspace(2, 16, "cpu")):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="65 bins"):
        V.edge_profile(vol, sdist, 4.0625, 0.125)
    with pytest.raises(ValueError, match="interfaces must be"):
        V.EdgeWorkspace(6, 16, "cuda")
    with pytest.raises(ValueError, match="bins must be"):
        V.EdgeWorkspace(2, 65, "cuda")
    with pytest.raises(ValueError, match="labels or sdist"):
        V.edge_sharpness(vol)


def test_library_declares_the_entry_points_and_checks_their_arguments():
    import ctypes
    from mri_superresolution_amd import _lib
    lib = _lib.load()
    names = ("mrisr_u8_volume_interface_sides", "mrisr_f32_volume_signed_distance", "mrisr_f32_volume_edge_workspace_bytes",
             "mrisr_f32_volume_edge_profile")
    with open(os.path.join(REPO, "include", "mrisr.h")) as f:
        header = f.read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and f" {name}(" in header
    assert lib.mrisr_version() == _lib.ABI_VERSION >= 327
    assert lib.mrisr_f32_volume_edge_workspace_bytes(2, 16) == 1024 * 2 * 16 * 32
    assert lib.mrisr_f32_volume_edge_workspace_bytes(5, 64) == 1024 * 320 * 32
    for bad in ((0, 16), (6, 16), (2, 1), (2, 65)):
        assert lib.mrisr_f32_volume_edge_workspace_bytes(*bad) == 0
    ARG, SHAPE = -1, -2
    buf = (ctypes.c_uint64 * 64)()                       # host memory: nothing is launched when a check fails
    p = ctypes.addressof(buf)
    q, r, w = p + 64, p + 128, p + 256
    assert lib.mrisr_u8_volume_interface_sides(None, 4, 1, q, None) == ARG
    assert lib.mrisr_u8_volume_interface_sides(p, 4, 1, None, None) == ARG
    assert lib.mrisr_u8_volume_interface_sides(p, 4, 0, q, None) == ARG
    assert lib.mrisr_u8_volume_interface_sides(p, 4, 255, q, None) == ARG
    assert b"1..254" in lib.mrisr_last_error()
    assert lib.mrisr_u8_volume_interface_sides(p, 0, 1, q, None) == SHAPE
    assert lib.mrisr_u8_volume_interface_sides(p, 1 << 32, 1, q, None) == SHAPE
    assert lib.mrisr_f32_volume_signed_distance(None, q, r, 4, w, None) == ARG
    assert lib.mrisr_f32_volume_signed_distance(p, None, r, 4, w, None) == ARG
    assert lib.mrisr_f32_volume_signed_distance(p, q, None, 4, w, None) == ARG
    assert lib.mrisr_f32_volume_signed_distance(p, q, r, 4, None, None) == ARG
    assert lib.mrisr_f32_volume_signed_distance(p, q + 2, r, 4, w, None) == ARG
    assert lib.mrisr_f32_volume_signed_distance(p, q, r, 4, w + 1, None) == ARG
    assert b"misaligned" in lib.mrisr_last_error()
    assert lib.mrisr_f32_volume_signed_distance(p, q, r, 0, w, None) == SHAPE
    ok = (p, q, 1, 4, 4.0, 0.5, 16, r, w, None)

    def profile(**changed):
        args = list(ok)
        for i, v in changed.items():
            args[int(i[1:])] = v
        return lib.mrisr_f32_volume_edge_profile(*args)

    for i in (0, 1, 7, 8):
        assert profile(**{f"a{i}": None}) == ARG
    assert profile(a0=p + 2) == ARG and profile(a7=r + 4) == ARG and profile(a8=w + 4) == ARG
    assert b"misaligned" in lib.mrisr_last_error()
    assert profile(a2=0) == ARG and profile(a2=6) == ARG and profile(a6=1) == ARG and profile(a6=65) == ARG
    assert b"bins" in lib.mrisr_last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert profile(a4=bad) == ARG and profile(a5=bad) == ARG
    assert b"finite, positive" in lib.mrisr_last_error()
    assert profile(a3=0) == SHAPE and profile(a3=1 << 32) == SHAPE


# ---------------------------------------------------------------- the command lines

def test_command_lines_parse_and_check_the_new_options():
    from scripts import evaluate_volume as eval_cli
    from scripts import segment_volume as segment_cli
    plain = eval_cli.parse_args(["--reference", "r.nii"])
    assert plain.tissue_edges is False and plain.edge_radius_mm == 4.0 and plain.edge_bin_mm == 0.5
    on = eval_cli.parse_args(["--reference", "r.nii", "--mask", "otsu", "--tissue_dice", "3", "--tissue_edges", "--edge_radius_mm", "3",
                              "--edge_bin_mm", "0.25"])
    assert on.tissue_edges is True and on.edge_radius_mm == 3.0 and on.edge_bin_mm == 0.25
    base = (None, None, "linear", "header", "none", "none")
    eval_cli.check_options(*base, tissue_dice=3, mask="otsu", tissue_edges=True)
    eval_cli.check_options(*base, tissue_dice=3, mask="otsu", tissue_edges=True, edge_radius_mm=4.0, edge_bin_mm=0.125)
    with pytest.raises(ValueError, match="--tissue_edges goes with --tissue_dice"):
        eval_cli.check_options(*base, mask="otsu", tissue_edges=True)
    with pytest.raises(ValueError, match="65 bins"):
        eval_cli.check_options(*base, tissue_dice=3, mask="otsu", tissue_edges=True, edge_radius_mm=4.0625, edge_bin_mm=0.125)
    with pytest.raises(ValueError, match="finite positive"):
        eval_cli.check_options(*base, tissue_dice=3, mask="otsu", tissue_edges=True, edge_bin_mm=0.0)
    eval_cli.check_options(*base, edge_radius_mm=100.0)                # without the switch the two numbers are not read
    assert eval_cli.edge_columns(3) == ["esw_1", "esw_2", "econ_1", "econ_2"] and eval_cli.edge_columns(0) == []
    assert segment_cli.parse_args(["--input", "a.nii", "--output", "b.nii"]).edges is None
    assert segment_cli.parse_args(["--input", "a.nii", "--output", "b.nii", "--edges", "s.nii"]).edges == "s.nii"


def test_evaluate_volume_option_rules_need_no_device():
    import torch
    from mri_superresolution_amd.volume_eval import evaluate_volume
    ref = torch.zeros(4, 4, 4)
    with pytest.raises(ValueError, match="tissue_edges needs tissue_dice"):
        evaluate_volume(None, ref, mask="otsu", tissue_edges=True)
    with pytest.raises(ValueError, match="65 bins"):
        evaluate_volume(None, ref, mask="otsu", tissue_dice=3, tissue_edges=True, edge_radius=4.0625, edge_bin=0.125)
    with pytest.raises(ValueError, match="spacing needs tissue_surface"):
        evaluate_volume(None, ref, mask="otsu", tissue_dice=3, spacing=(1, 1, 1))
    with pytest.raises(ValueError, match="voxel sizes"):
        evaluate_volume(None, ref, mask="otsu", tissue_dice=3, tissue_edges=True, spacing=(1, 0, 1))
