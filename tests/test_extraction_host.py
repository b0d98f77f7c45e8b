"""Paired-slice extraction, host side (no GPU): the tap tables of csrc/resample.hip's host helper against their float64
restatement, the any-size Dirichlet rows, and utils/extraction.py's bookkeeping and NumPy chain against
tests/golden/extraction.npz - what the REFERENCE's own extract_slices_3d handed to cv2.resize and cv2.imwrite
(tools/gen_extraction_golden.py; a recording cv2 stub, so everything except cv2.resize itself is pinned).

Tie condition (what tests/test_gpu_extraction.py relies on): the uint8 image is a truncation, so a device pixel may differ
from the restatement only where value x 255 lies within the tie band of an integer.  The band is 255 x the float bar of the
resampler, 2 (K_y + K_x + 4) 2^-24 max sum|w_y| max sum|w_x| (every product and sum of the two fp32 passes rounds once, the
weights are rounded once, inputs in [0,1]).  At most 1 % of each fixture image may lie inside it."""
import ctypes as C
import os

import numpy as np
import pytest

from mri_superresolution_amd import _lib as L
from mri_superresolution_amd.utils import extraction as E
from mri_superresolution_amd.utils import lowfield as LF

METHODS = {"linear": E.LINEAR, "cubic": E.CUBIC, "area": E.AREA, "lanczos4": E.LANCZOS4}
PAIRS = [(37, 64), (29, 48), (70, 32), (50, 22), (70, 24), (64, 32), (48, 24), (5, 16), (7, 16), (31, 31), (193, 256), (229, 128),
         (45, 22), (31, 32), (2, 9), (1, 4), (160, 10)]


def float_bar(yw, xw):
    """The resampler's derived fp32 bar for inputs in [0,1] from its two tables."""
    return 2 * (yw.shape[1] + xw.shape[1] + 4) * 2.0 ** -24 * np.abs(yw).sum(1).max() * np.abs(xw).sum(1).max()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "extraction.npz"))


@pytest.fixture(scope="module")
def host_runs(golden):
    runs = {}
    for c in "ab":
        noise = [(n[0], n[1]) for n in golden[c + "_noise"]]
        runs[c] = E.extract_pairs_host(golden[c + "_volume"], int(golden["n_slices"]), float(golden["lower_percent"]),
                                       float(golden["upper_percent"]), tuple(int(v) for v in golden[c + "_target"]),
                                       float(golden["crop_factor"]), float(golden["noise_std"]), kspace_noise=noise)
    return runs


# ---------------------------------------------------------------- tap tables
@pytest.mark.parametrize("method", sorted(METHODS))
def test_tables_equal_the_restatement(method):
    for src, dst in PAIRS:
        index, weight = E.resample_taps(METHODS[method], src, dst)
        ref_i, ref_w = E.resample_taps_np(METHODS[method], src, dst)
        assert index.dtype == np.int16 and weight.dtype == np.float32 and index.shape == ref_i.shape == weight.shape
        assert np.array_equal(index, ref_i), (method, src, dst)
        assert np.array_equal(weight, ref_w.astype(np.float32)), (method, src, dst)
        assert index.min() >= 0 and index.max() <= src - 1
        assert np.abs(weight.astype(np.float64).sum(1) - 1).max() <= 4 * 2.0 ** -24, (method, src, dst)
        assert np.all(np.diff(index.astype(int), axis=0) >= 0)       # what the kernel's source window relies on


def test_tap_counts_and_unused_slots():
    for method, k in ((E.LINEAR, 2), (E.CUBIC, 4), (E.LANCZOS4, 8)):
        assert E.resample_taps(method, 37, 64)[0].shape == (64, k) and E.resample_taps(method, 70, 32)[0].shape == (32, k)
    assert E.resample_taps(E.AREA, 70, 32)[0].shape == (32, 4) and E.resample_taps(E.AREA, 64, 32)[0].shape == (32, 2)
    # AREA enlarging uses the LINEAR taps (stated deviation)
    for a, b in zip(E.resample_taps(E.AREA, 37, 64), E.resample_taps(E.LINEAR, 37, 64)):
        assert np.array_equal(a, b)
    # the raw call: slots past the tap count carry weight 0 and a valid index
    index, weight, k = np.full((32, 16), -7, dtype=np.int16), np.full((32, 16), 9, dtype=np.float32), C.c_int(0)
    assert L.load().mrisr_resample_taps(E.AREA, 70, 32, 16, C.addressof(k), index.ctypes.data, weight.ctypes.data) == 0
    assert k.value == 4 and np.all(weight[:, 4:] == 0) and index.min() >= 0 and index.max() <= 69


@pytest.mark.parametrize("method", sorted(METHODS))
def test_same_size_is_the_identity(method):
    index, weight = E.resample_taps(METHODS[method], 31, 31)
    assert np.all((weight == 1).sum(1) == 1) and np.all((weight != 0).sum(1) == 1)
    assert np.array_equal(index[weight == 1], np.arange(31))
    img = np.random.default_rng(0).random((9, 31))
    assert np.array_equal(E.resample_letterbox_host(img, (31, 9), METHODS[method]), img)


def test_area_integer_ratio_and_brute_force():
    for src, r in ((64, 2), (48, 3), (60, 5)):
        index, weight = E.resample_taps(E.AREA, src, src // r)
        assert weight.shape[1] == r and np.all(weight == np.float32(1.0 / r))
        assert np.array_equal(index, np.arange(src).reshape(-1, r))
    # 70 -> 32 against overlaps measured on a fine grid: 32 * 70 cells per unit make every boundary a grid line
    index, weight = E.resample_taps(E.AREA, 70, 32)
    fine = 32
    owner_src = np.arange(70 * fine) // fine                 # cell c of width 1 / 32 lies in source sample c // 32
    owner_dst = np.arange(70 * fine) // 70                   # and in output sample c // 70 (output samples are 70 / 32 wide)
    dense = np.zeros((32, 70))
    np.add.at(dense, (owner_dst, owner_src), 1.0 / 70)       # cell width / (70 / 32)
    got = np.zeros((32, 70))
    np.add.at(got, (np.arange(32)[:, None].repeat(weight.shape[1], 1), index.astype(int)), weight.astype(np.float64))
    assert np.abs(got - dense).max() <= 2.0 ** -24


def test_border_indices_are_clamped():
    index, weight = E.resample_taps(E.LANCZOS4, 5, 16)
    assert index.shape == (16, 8) and index.min() == 0 and index.max() == 4
    assert np.array_equal(index[0], np.clip(np.arange(-4, 4), 0, 4))      # s = -0.34: floor(s) - 3 = -4
    assert np.array_equal(index[-1], np.clip(np.arange(1, 9), 0, 4))      # s = 4.34: floor(s) - 3 = 1
    assert (index[0] == 0).sum() == 5 and (index[-1] == 4).sum() == 5
    # replicated border: a constant image stays constant
    assert np.abs(E.resample_letterbox_host(np.full((5, 5), 0.37), (16, 16), E.LANCZOS4) - 0.37).max() < 1e-15


def test_refusals():
    lib = L.load()
    index, weight, k = np.zeros((10, 32), dtype=np.int16), np.zeros((10, 32), dtype=np.float32), C.c_int(0)

    def call(method=E.AREA, src=170, dst=10, room=32, kp=C.addressof(k), ip=index.ctypes.data, wp=weight.ctypes.data):
        return lib.mrisr_resample_taps(method, src, dst, room, kp, ip, wp)

    assert call() == -5 and b"17 taps" in lib.mrisr_last_error()          # MRISR_E_UNSUPPORTED
    assert call(src=160) == 0 and k.value == 16
    assert call(src=160, room=8) == -2 and call(src=0) == -2 and call(dst=0) == -2 and call(src=40000) == -2
    assert call(method=0) == -1 and call(method=5) == -1 and call(kp=None) == -1 and call(ip=None) == -1 and call(wp=None) == -1
    with pytest.raises(RuntimeError, match="17 taps"):
        E.resample_taps(E.AREA, 170, 10)
    with pytest.raises(ValueError):
        E.resample_taps_np(E.AREA, 170, 10)


# ---------------------------------------------------------------- Dirichlet rows of any size
@pytest.mark.parametrize("n", [31, 45, 32, 2, 3])
def test_dirichlet_rows_of_any_size(n):
    f = 0.5 if n > 3 else 1.0
    re, im = LF.dirichlet_table_any(n, f)
    a = int(n * f) // 2
    d = np.arange(n)
    p = np.exp(2j * np.pi * np.outer(d, np.arange(-a, a)) / n).sum(1) / n
    assert np.abs(re - p.real).max() <= 1e-7 and np.abs(im - p.imag).max() <= 1e-7
    if n % 2 == 0 and n >= 4:
        even = LF.dirichlet_table(n, f)
        assert np.array_equal(even[0], re) and np.array_equal(even[1], im)


def test_dirichlet_any_is_the_reference_mask_for_odd_sizes():
    """The circulant with the rows of mrisr_lowfield_dirichlet_any equals the reference's fftshift / mask / ifftshift."""
    rng = np.random.default_rng(3)
    x = rng.random((31, 45))
    ref = LF.simulate_low_field_f32_host(x, 0.5, 0.0)

    def circ(n):
        re, im = LF.dirichlet_table_any(n, 0.5)
        d = np.arange(n)
        return (re.astype(np.float64) + 1j * im)[(d[:, None] - d[None, :]) % n]

    assert np.abs(np.abs(circ(31) @ x @ circ(45).T) - ref["magnitude"]).max() <= 5e-6
    lib = L.load()
    buf = np.zeros(8, dtype=np.float32)
    assert lib.mrisr_lowfield_dirichlet_any(1, 0.5, buf.ctypes.data, buf.ctypes.data) == -2
    assert lib.mrisr_lowfield_dirichlet_any(3, 0.5, buf.ctypes.data, buf.ctypes.data) == -1       # keeps nothing
    assert lib.mrisr_lowfield_dirichlet_any(5, 1.5, buf.ctypes.data, buf.ctypes.data) == -1
    assert lib.mrisr_lowfield_dirichlet_any(5, 0.5, None, buf.ctypes.data) == -1
    assert lib.mrisr_lowfield_dirichlet(31, 0.5, buf.ctypes.data, buf.ctypes.data) == -2          # the even-size entry keeps its rule


# ---------------------------------------------------------------- bookkeeping against the reference's run
def test_bookkeeping_equals_the_fixture(golden, host_runs):
    assert [E.bids_identifier(str(n)) for n in golden["bids_in"]] == [str(n) for n in golden["bids_out"]]
    for c in "ab":
        vol = golden[c + "_volume"]
        idx = E.slice_indices(vol.shape[2], int(golden["n_slices"]), float(golden["lower_percent"]), float(golden["upper_percent"]))
        assert np.array_equal(idx, golden[c + "_indices"]) and np.array_equal(host_runs[c]["indices"], idx)
        tp = int(golden[c + "_timepoint"])
        assert [E.pair_filename("sub-01_T1w", i, None if tp < 0 else tp) for i in idx] == [str(n) for n in golden[c + "_names"]]
        tw, th = (int(v) for v in golden[c + "_target"])
        new_w, new_h, x_off, y_off = E.letterbox_geometry(vol.shape[0], vol.shape[1], tw, th)
        assert all(tuple(d) == (new_w, new_h) for d in golden[c + "_hr_dsize"])
        assert x_off == (tw - new_w) // 2 and y_off == (th - new_h) // 2 and new_w <= tw and new_h <= th
        # what the reference asked cv2.resize for, call by call
        assert all(tuple(d) == tuple(host_runs[c]["hr_dsize"]) for d in golden[c + "_hr_dsize"])
        assert all(tuple(d) == tuple(host_runs[c]["lr_dsize"]) for d in golden[c + "_lr_dsize"])
        assert np.all(golden[c + "_hr_interpolation"] == host_runs[c]["hr_interpolation"]) and host_runs[c]["hr_interpolation"] == E.LANCZOS4
        assert np.all(golden[c + "_lr_interpolation"] == host_runs[c]["lr_interpolation"]) and host_runs[c]["lr_interpolation"] == E.AREA
        # and what it wrote: target and target // 2, uint8
        shapes = golden[c + "_image_shapes"]
        assert np.all(shapes[0::2] == (th, tw)) and np.all(shapes[1::2] == (th // 2, tw // 2))
        for k in range(len(idx)):
            assert host_runs[c]["hr_u8"][k].shape == (th, tw) and host_runs[c]["lr_u8"][k].shape == (th // 2, tw // 2)
            assert host_runs[c]["hr_u8"][k].dtype == np.uint8
    assert E.letterbox_geometry(31, 45, 64, 48) == (64, 44, 0, 2) and E.letterbox_geometry(70, 50, 32, 32) == (22, 32, 5, 0)


def test_slice_indices_rules():
    assert np.array_equal(E.slice_indices(160), np.linspace(32, 128, 10, dtype=int))
    assert np.array_equal(E.slice_indices(12, 4, 0.2, 0.8), [2, 4, 6, 9])
    with pytest.raises(ValueError):
        E.slice_indices(12, 4, 0.2, 1.0)          # int(1.0 * 12) = 12 is outside
    assert E.pair_filename("s", 7) == "s_s007.png" and E.pair_filename("s", 7, 0) == "s_T0_s007.png"


def test_recorded_planes_are_reproduced(golden, host_runs):
    for c in "ab":
        for k in range(int(golden["n_slices"])):
            hr_err = np.abs(host_runs[c]["hr_plane"][k].astype(np.float64) - golden[c + "_hr_plane"][k].astype(np.float64)).max()
            lr_err = np.abs(host_runs[c]["lr_plane"][k] - golden[c + "_lr_plane"][k]).max()
            print(f"volume {c} slice {k}: HR plane max abs err {hr_err:.3e}, simulated plane {lr_err:.3e}")
            assert golden[c + "_hr_plane"][k].dtype == np.float32 and hr_err <= 1e-6
            assert lr_err <= 1e-12
            # the plain float64 restatement (what the device path is compared against) differs from the reference's run only
            # by the precision numpy gives the forward transform of a float32 slice
            plain = LF.simulate_low_field_f32_host(host_runs[c]["hr_plane"][k].astype(np.float64), float(golden["crop_factor"]),
                                                   float(golden["noise_std"]), tuple(golden[c + "_noise"][k]))["clipped"]
            assert np.abs(plain - golden[c + "_lr_plane"][k]).max() <= 1e-6


def test_constant_slice_becomes_zeros(golden):
    vol = golden["a_volume"]
    assert np.all(vol[:, :, 0] == vol[0, 0, 0]) and 0 not in golden["a_indices"]
    assert np.all(E.normalise_slice_np(vol[:, :, 0]) == 0)
    r = E.extract_pairs_host(vol[:, :, :1].repeat(3, 2), 2, 0.0, 0.5, (64, 48), noise_std=0.0)
    assert all(np.all(a == 0) for a in r["hr_u8"]) and all(np.all(a == 0) for a in r["lr_u8"])


def test_tie_condition_on_the_fixture_volumes(golden, host_runs):
    for c in "ab":
        vol = golden[c + "_volume"]
        tw, th = (int(v) for v in golden[c + "_target"])
        for kind, method, size in (("hr", E.LANCZOS4, (tw, th)), ("lr", E.AREA, (tw // 2, th // 2))):
            new_w, new_h, x_off, y_off = E.letterbox_geometry(vol.shape[0], vol.shape[1], *size)
            yw, xw = E.resample_taps_np(method, vol.shape[0], new_h)[1], E.resample_taps_np(method, vol.shape[1], new_w)[1]
            band = 255 * float_bar(yw, xw)
            for k, img in enumerate(host_runs[c][kind]):
                v = img[y_off:y_off + new_h, x_off:x_off + new_w] * 255       # the pad is written exactly: it cannot move
                inside = np.abs(v - np.rint(v)) <= band
                print(f"volume {c} {kind} slice {k}: band {band:.3e}, {int(inside.sum())}/{v.size} block pixels inside")
                assert inside.sum() <= 0.01 * v.size
