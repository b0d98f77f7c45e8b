"""Connected-component clean-up of foreground masks, the part that needs no GPU: the numpy specifications label_components_np,
largest_component_np and fill_holes_np (against scipy where it is installed, and against their own rules), foreground_mask_np with
the defaults, the refusals of the new C-ABI entry points (argument checks run before any launch) and the argument errors of the
Python surface and of the command line."""
import hashlib
import os
import sys
import time

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd import _lib                                   # noqa: E402
from mri_superresolution_amd import volume_eval as V                       # noqa: E402
from scripts import evaluate_volume as cli                                 # noqa: E402
from labelutil import bernoulli, check_canonical, fixed_volume, serpentine      # noqa: E402

E_ARG, E_SHAPE, E_UNSUPPORTED = -1, -2, -5      # include/mrisr.h
SHAPES = [(1, 1, 1), (3, 5, 7), (17, 9, 33), (70, 37, 45), (64, 64, 80)]
DENSITIES = [0.1, 0.3, 0.5, 0.9]


def test_specifications_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rounds = 0
    for shape in SHAPES:
        for p in DENSITIES:
            m = bernoulli(shape, p, seed=sum(shape) + int(10 * p))
            for conn in (6, 26):
                lab = V.label_components_np(m, conn)
                want, count = ndi.label(m, ndi.generate_binary_structure(3, 1 if conn == 6 else 3))
                # the same partition: the pairs (ours, scipy's) are a bijection between the two label sets
                pairs = np.unique(lab.reshape(-1).astype(np.int64) * (count + 1) + want.reshape(-1))
                assert pairs.size == count + (1 if (m == 0).any() else 0) == len(np.unique(lab)) == len(np.unique(want))
                check_canonical(lab, m != 0, V.backward_offsets(conn))
                rounds += 1
            for p_fill in (p, 0.6, 0.8) if shape == (70, 37, 45) else (p,):
                q = bernoulli(shape, p_fill, seed=int(100 * p_fill))
                got, filled = V.fill_holes_np(q)
                want = ndi.binary_fill_holes(q)
                assert np.array_equal(got, want.astype(np.uint8)) and filled == int(want.sum()) - int(q.sum())
                for axis in (0, 1, 2):
                    got, filled = V.fill_holes_np(q, axis)
                    want = np.stack([ndi.binary_fill_holes(np.take(q, i, axis)) for i in range(shape[axis])], axis)
                    assert np.array_equal(got, want.astype(np.uint8)) and filled == int(want.sum()) - int(q.sum())
    assert rounds == 40


def test_label_rule_plane_mode_and_invert_without_scipy():
    for shape in SHAPES[:4]:
        m = bernoulli(shape, 0.45, seed=sum(shape))
        for conn in (6, 26):
            for axis in (None, 0, 1, 2):
                lab = V.label_components_np(m, conn, axis)
                check_canonical(lab, m != 0, V.backward_offsets(conn, -1 if axis is None else axis))
                assert np.array_equal(V.label_components_np(m, conn, axis, invert=True), V.label_components_np(1 - m, conn, axis))
                if axis is None:
                    continue
                # plane mode against a loop over the planes: labels of a plane alone, moved to the volume's indices
                index = np.arange(m.size).reshape(shape)
                for i in range(shape[axis]):
                    plane = np.take(m, [i], axis)
                    alone = V.label_components_np(plane, conn).reshape(-1)
                    where = np.take(index, [i], axis).reshape(-1)
                    want = np.where(alone > 0, where[np.maximum(alone, 1) - 1] + 1, 0)
                    assert np.array_equal(np.take(lab, [i], axis).reshape(-1), want)
    assert len(V.backward_offsets(26)) == 13 and len(V.backward_offsets(6)) == 3
    assert len(V.backward_offsets(26, 1)) == 4 and len(V.backward_offsets(6, 2)) == 2
    # a 3-D checkerboard: one component under 26, singletons under 6
    x, y, z = np.meshgrid(*(np.arange(s) for s in (6, 5, 7)), indexing="ij")
    board = ((x + y + z) % 2 == 0).astype(np.uint8)
    assert len(np.unique(V.label_components_np(board, 26))) == 2
    lab6 = V.label_components_np(board, 6)
    assert np.array_equal(lab6.reshape(-1), np.where(board.reshape(-1) != 0, np.arange(1, board.size + 1), 0))


def test_serpentine_is_one_component_and_quick():
    m = serpentine()
    t0 = time.perf_counter()
    lab = V.label_components_np(m, 6)
    took = time.perf_counter() - t0
    print(f"serpentine: {int(m.sum())} voxels, {took:.3f} s")
    assert m.sum() > 64 * 64 * 80 // 4
    assert np.array_equal(np.unique(lab), [0, 1])               # one component, and it starts at voxel 0
    assert took < 1.0
    assert np.array_equal(V.largest_component_np(m, 6)[0], m)


def test_largest_component_ties_empty_and_full_masks():
    m = np.zeros((9, 10, 11), dtype=np.uint8)
    m[1:3, 1:4, 1:5] = 1                                        # 24 voxels
    m[5:7, 5:8, 5:9] = 1                                        # 24 voxels, later in C order
    m[8, 9, 10] = 1
    kept, st = V.largest_component_np(m, 26)
    first = np.ravel_multi_index((1, 1, 1), m.shape) + 1
    assert st.tolist() == [3.0, 24.0, float(first)] and kept.dtype == np.uint8
    assert kept[1:3, 1:4, 1:5].all() and kept.sum() == 24      # the tie goes to the smaller label
    m[5, 5, 4] = 1                                              # now the second box is larger
    kept, st = V.largest_component_np(m, 6)
    assert st[:2].tolist() == [3.0, 25.0] and kept[5:7, 5:8, 5:9].all() and kept.sum() == 25
    kept, st = V.largest_component_np(np.zeros((3, 4, 5), dtype=np.uint8))
    assert not kept.any() and st.tolist() == [0.0, 0.0, 0.0]
    kept, st = V.largest_component_np(np.full((3, 4, 5), 9, dtype=np.uint8))
    assert kept.all() and st.tolist() == [1.0, 60.0, 1.0]
    assert not V.label_components_np(np.zeros((3, 4, 5), dtype=np.uint8)).any()
    assert (V.label_components_np(np.ones((3, 4, 5), dtype=np.uint8), 6) == 1).all()


def test_fill_holes_shell_pin_hole_and_diagonal_gap():
    shell = np.zeros((9, 9, 9), dtype=np.uint8)
    shell[2:7, 2:7, 2:7] = 1
    shell[3:6, 3:6, 3:6] = 0                                    # a cavity of 27 voxels
    got, filled = V.fill_holes_np(shell)
    assert filled == 27 and got[2:7, 2:7, 2:7].all() and got.sum() == 125
    pin = shell.copy()
    pin[2, 4, 4] = 0                                            # a one-voxel channel through a face of the shell
    got, filled = V.fill_holes_np(pin)
    assert filled == 0 and np.array_equal(got, pin)
    gap = shell.copy()
    gap[2, 2, 2] = 0                                            # the corner of the shell: only diagonal to the cavity's corner
    got, filled = V.fill_holes_np(gap)
    assert filled == 27 and got[2, 2, 2] == 0                   # the background is 6-connected: still a hole
    # plane by plane: the pin-hole plane is open only in the planes that contain the channel
    got0, filled0 = V.fill_holes_np(pin, 0)
    assert filled0 == 28 and got0[2, 4, 4] == 1                 # across axis 0 every plane is closed, the channel's voxel as well
    got1, filled1 = V.fill_holes_np(pin, 1)
    assert filled1 == 18 and got1[3, 4, 4] == 0                 # the plane y = 4 holds the channel: its 9 voxels stay open
    assert V.fill_holes_np(np.zeros((1, 5, 5), dtype=np.uint8))[1] == 0
    assert V.fill_holes_np(np.ones((4, 5, 5), dtype=np.uint8) * 7)[0].max() == 1      # the result is 0 / 1


def test_foreground_mask_np_defaults_are_unchanged_and_the_clean_up_works():
    v = fixed_volume()
    for r in (0, 1):
        mask, st = V.foreground_mask_np(v, r, return_stats=True)
        # what the function was before it learnt to clean up: Otsu bins, threshold, closing
        lo, hi, bins = V.otsu_bins_np(v)
        t = V.otsu_threshold_np(np.bincount(bins.reshape(-1), minlength=256))
        want = (bins > t).astype(np.uint8)
        want = V.erode_np(V.dilate_np(want, r), r) if r else want
        assert np.array_equal(mask, want) and "cleanup" not in st and sorted(st) == ["count", "counts", "hi", "lo", "t"]
        assert np.array_equal(V.foreground_mask_np(v, r), mask)
        assert np.array_equal(V.foreground_mask_np(v, r, largest=False, fill_holes=None), mask)
    # what the commit before the clean-up returned for foreground_mask_np(v, 1) on this volume: t*, the counts, the mask's digest
    mask, st = V.foreground_mask_np(v, 1, return_stats=True)
    assert (st["t"], st["count"], int(mask.sum())) == (28, 1570, 1588)
    assert hashlib.sha256(mask.tobytes()).hexdigest() == PARENT_DIGEST
    plain = V.foreground_mask_np(v, 0)
    assert plain[1, 2, 3] == 1 and plain[18, 20, 5] == 1 and plain[10, 12, 14] == 0
    cleaned, st = V.foreground_mask_np(v, 0, return_stats=True, largest=True, fill_holes="3d")
    assert cleaned[1, 2, 3] == 0 and cleaned[18, 20, 5] == 0 and cleaned[10, 12, 14] == 1
    found, kept, filled = st["cleanup"]
    assert found == 3 and kept == plain.sum() - 2 and filled == cleaned.sum() - kept > 0
    only_fill, st = V.foreground_mask_np(v, 0, return_stats=True, fill_holes=2)
    assert only_fill[1, 2, 3] == 1 and np.isnan(st["cleanup"][:2]).all() and st["cleanup"][2] == only_fill.sum() - plain.sum()
    for bad in ("2d", 3, -1, True, 1.0):
        with pytest.raises(ValueError):
            V.foreground_mask_np(v, fill_holes=bad)


PARENT_DIGEST = "e5d1b5e4b5e3885109b3945e6d19e10f63a4d63be93c729ea3d580832a84b737"


def test_the_c_abi_declares_the_new_entries_and_refuses_bad_arguments():
    lib = _lib.load()
    for name in ("mrisr_u8_volume_label", "mrisr_u8_volume_label_workspace_bytes", "mrisr_u8_volume_keep_largest",
                 "mrisr_u8_volume_fill_holes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.mrisr_version() == _lib.ABI_VERSION >= 314
    assert lib.mrisr_u8_volume_label_workspace_bytes(3, 5, 7) == 64 + 8 * 105
    assert lib.mrisr_u8_volume_label_workspace_bytes(0, 5, 7) == 0 and lib.mrisr_u8_volume_label_workspace_bytes(2048, 2048, 2048) == 0
    # host buffers stand in for device memory: every call below is refused before anything is launched
    buf = np.zeros(8192, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    m, lab, dst, st, ws = p, p + 1024, p + 2048, p + 3072, p + 4096
    label, largest, fill = lib.mrisr_u8_volume_label, lib.mrisr_u8_volume_keep_largest, lib.mrisr_u8_volume_fill_holes
    assert label(None, 2, 2, 2, 26, -1, 0, lab, None) == E_ARG and b"null" in lib.mrisr_last_error()
    assert label(m, 2, 2, 2, 26, -1, 0, None, None) == E_ARG
    assert label(m, 2, 2, 2, 26, -1, 0, lab + 2, None) == E_ARG and b"misaligned" in lib.mrisr_last_error()
    for conn in (0, 4, 8, 18, 27):
        assert label(m, 2, 2, 2, conn, -1, 0, lab, None) == E_ARG
        assert largest(m, 2, 2, 2, conn, dst, st, ws, None) == E_ARG
    for axis in (-2, 3):
        assert label(m, 2, 2, 2, 6, axis, 0, lab, None) == E_ARG
        assert fill(m, 2, 2, 2, axis, dst, st, ws, None) == E_ARG
    assert label(m, 2, 2, 2, 6, 0, 2, lab, None) == E_ARG
    for shape in ((0, 2, 2), (2, 32768, 2), (2, 2, -1)):
        assert label(m, *shape, 26, -1, 0, lab, None) == E_SHAPE
        assert largest(m, *shape, 26, dst, st, ws, None) == E_SHAPE
        assert fill(m, *shape, -1, dst, st, ws, None) == E_SHAPE
    for shape in ((2048, 2048, 512), (32767, 32767, 3)):       # 2^31 voxels and more: one past the last int32 label
        assert label(m, *shape, 26, -1, 0, lab, None) == E_UNSUPPORTED and b"2^31 - 2" in lib.mrisr_last_error()
        assert largest(m, *shape, 26, dst, st, ws, None) == E_UNSUPPORTED
        assert fill(m, *shape, -1, dst, st, ws, None) == E_UNSUPPORTED
    for args in ((None, dst, st, ws), (m, None, st, ws), (m, dst, None, ws), (m, dst, st, None)):
        assert largest(args[0], 2, 2, 2, 26, *args[1:], None) == E_ARG and b"null" in lib.mrisr_last_error()
        assert fill(args[0], 2, 2, 2, -1, *args[1:], None) == E_ARG and b"null" in lib.mrisr_last_error()
    assert largest(m, 2, 2, 2, 26, m, st, ws, None) == E_ARG and b"must not be the mask" in lib.mrisr_last_error()
    assert fill(m, 2, 2, 2, -1, m, st, ws, None) == E_ARG and b"must not be the mask" in lib.mrisr_last_error()
    assert largest(m, 2, 2, 2, 26, dst, st + 4, ws, None) == E_ARG and fill(m, 2, 2, 2, -1, dst, st, ws + 8, None) == E_ARG
    assert not buf.any()                                        # nothing was written


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    vol = torch.zeros((4, 6, 8))
    mask = torch.ones((4, 6, 8), dtype=torch.uint8)
    for call in (lambda: V.label_components(mask), lambda: V.largest_component(mask), lambda: V.fill_holes(mask),
                 lambda: V.foreground_mask(vol, largest=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for conn in (4, 18, True, "26"):
        with pytest.raises(ValueError, match="connectivity"):
            V.label_components(mask, conn)
        with pytest.raises(ValueError, match="connectivity"):
            V.largest_component(mask, conn)
        with pytest.raises(ValueError, match="connectivity"):
            V.label_components_np(mask.numpy(), conn)
    for axis in (3, -1, "x", True):
        with pytest.raises(ValueError, match="plane_axis"):
            V.label_components(mask, 6, axis)
        with pytest.raises(ValueError, match="axis"):
            V.fill_holes(mask, axis)
    with pytest.raises(ValueError):
        V.label_components_np(np.zeros((2, 2)))
    with pytest.raises(ValueError, match="fill_holes"):
        V.foreground_mask(vol, fill_holes="2d")
    with pytest.raises(ValueError, match="need a mask"):
        V.evaluate_volume(None, vol, mask=None, mask_largest=True)
    with pytest.raises(ValueError, match="need a mask"):
        V.evaluate_volume(None, vol, mask_fill_holes="3d")
    with pytest.raises(ValueError, match="fill_holes"):
        V.evaluate_volume(None, vol, mask="otsu", mask_fill_holes=4)
    assert V.VolumeScores().mask_cleanup is None


def test_command_line_flags():
    args = cli.parse_args(["--reference", "a.nii"])
    assert args.mask_largest is False and args.mask_fill_holes is None and args.save_mask is None
    args = cli.parse_args(["--reference", "a.nii", "--mask", "otsu", "--mask_largest", "--mask_fill_holes", "3d", "--save_mask", "m.nii"])
    assert args.mask_largest is True and args.mask_fill_holes == "3d" and args.save_mask == "m.nii"
    assert cli.parse_args(["--reference", "a.nii", "--mask", "otsu", "--mask_fill_holes", "1"]).mask_fill_holes == "1"
    with pytest.raises(SystemExit):
        cli.parse_args(["--reference", "a.nii", "--mask", "otsu", "--mask_fill_holes", "4"])
    assert cli.CSV_COLUMNS_MASKED == ["scan", "region", "method", "ssim", "psnr", "mse", "rmse", "mae"]      # unchanged
    row = {"mask_voxels": 250, "voxels": 1000, "threshold": 123.5}
    nan = float("nan")
    assert cli.foreground_title([row]) == "foreground: 250 voxels, 25.0 % of the volume, Otsu threshold 123.5"
    assert cli.foreground_title([{**row, "cleanup": None}]) == "foreground: 250 voxels, 25.0 % of the volume, Otsu threshold 123.5"
    assert cli.foreground_title([{**row, "cleanup": (7.0, 240.0, 10.0)}]) == \
        "foreground: 250 voxels, 25.0 % of the volume, Otsu threshold 123.5, 7 components, kept 240 voxels, filled 10"
    assert cli.foreground_title([{**row, "threshold": None, "cleanup": (nan, nan, 10.0)}]) == \
        "foreground: 250 voxels, 25.0 % of the volume, filled 10"
    assert cli.foreground_title([{**row, "threshold": None, "cleanup": (7.0, 240.0, nan)}]) == \
        "foreground: 250 voxels, 25.0 % of the volume, 7 components, kept 240 voxels"
