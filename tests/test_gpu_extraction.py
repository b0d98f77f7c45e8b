"""Paired-slice extraction on the device (GPU): the float, any-size low-field simulation (mrisr_lowfield_simulate_f32) against
its float64 restatement, the seeded noise, utils/extraction.extract_pairs against extract_pairs_host on the two fixture
volumes of tests/golden/extraction.npz, and scripts/extract_paired_slices.py.

Bars: the simulated float plane within 5e-5 absolute of the float64 host plane (the bar tests/test_gpu_lowfield.py uses for the
same arithmetic).  uint8 images: at most 1 grey level away, on at most 1 % of the pixels of each image, and equal outside the
tie band of the truncation, 255 x 2 (K_y + K_x + 4) 2^-24 max sum|w_y| max sum|w_x| - the resampler's band for HR and LR alike,
the one tests/test_extraction_host.py counts the fixture's pixels with.  The float simulation runs with the fixture's replayed
noise at 31 x 45; the fixture holds no 32 x 48 plane, so that size draws its k-space noise from a seeded generator.
Measured on an MI355X: simulated plane 7.6e-7 (31 x 45) and 4.5e-7 (32 x 48) from the host plane, the two entries' magnitude
planes 2.4e-7 apart, no differing uint8 pixel on either fixture volume (profiles/NOTES.md, "Paired-slice extraction")."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mri_superresolution_amd import _lib as L                                            # noqa: E402
from mri_superresolution_amd.utils import extraction as E                                # noqa: E402
from mri_superresolution_amd.utils import lowfield as LF                                 # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, write_nifti                 # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_BAR, U8_SHARE = 5e-5, 0.01


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "extraction.npz"))


def _planes(knoise):
    n = np.stack([LF.image_noise_from_kspace(a, b) for a, b in knoise])
    return torch.from_numpy(n.real.astype(np.float32)).cuda(), torch.from_numpy(n.imag.astype(np.float32)).cuda()


@pytest.mark.parametrize("shape", [(31, 45), (32, 48)])
@pytest.mark.parametrize("noisy", [True, False])
def test_float_simulation_against_the_host(golden, shape, noisy):
    h, w = shape
    rng = np.random.default_rng(h * 100 + w)
    x = rng.random((4, h, w)).astype(np.float32)
    x[1] = np.float32(0.2) + np.float32(0.5) * x[1]            # extrema away from 0 and 1
    if noisy and shape == (31, 45):
        knoise = [(n[0], n[1]) for n in golden["a_noise"]]     # the fixture's replayed draw
    elif noisy:
        s = (5.0 / 255.0) * np.sqrt(h * w) / 10
        knoise = [(rng.normal(0, s, (h, w)), rng.normal(0, s, (h, w))) for _ in range(4)]
    else:
        knoise = [(np.zeros((h, w)), np.zeros((h, w)))] * 4
    got, mag = LF.simulate_low_field_f32(torch.from_numpy(x).cuda(), 0.5, noise=_planes(knoise), _return_magnitude=True)
    assert got.shape == (4, h, w) and got.dtype == torch.float32
    got, mag = got.cpu().numpy(), mag.cpu().numpy()
    for k in range(4):
        ref = LF.simulate_low_field_f32_host(x[k].astype(np.float64), 0.5, kspace_noise=knoise[k])
        err, merr = np.abs(got[k] - ref["clipped"]).max(), np.abs(mag[k] - ref["magnitude"]).max()
        print(f"{h} x {w} noise {noisy} image {k}: plane max abs err {err:.3e}, magnitude {merr:.3e}")
        assert err <= F32_BAR and merr <= F32_BAR
        assert got[k].min() >= 0 and got[k].max() <= 1
    if not noisy:       # noise_std = 0 is the same as zero planes, whatever the seeds
        assert np.array_equal(got, LF.simulate_low_field_f32(torch.from_numpy(x).cuda(), 0.5, 0.0, seeds=[1, 2, 3, 4]).cpu().numpy())


def test_seeded_noise_and_the_uint8_entry():
    rng = np.random.default_rng(8)
    u8 = torch.from_numpy(rng.integers(0, 256, (3, 32, 48)).astype(np.uint8)).cuda()
    x = u8.float() / 255
    seeds = [11, 12, 2 ** 63 + 5]
    a = LF.simulate_low_field_f32(x, 0.5, 5.0, seeds=seeds)
    assert torch.equal(a, LF.simulate_low_field_f32(x, 0.5, 5.0, seeds=seeds))
    c = LF.simulate_low_field_f32(x, 0.5, 5.0, seeds=[11, 13, 2 ** 63 + 5])
    assert torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1]) and torch.equal(a[2], c[2])
    assert torch.equal(LF.simulate_low_field_f32(x, 0.5, 5.0, seeds=3), LF.simulate_low_field_f32(x, 0.5, 5.0, seeds=LF.derive_seeds(3, None, range(3))))
    # the same seeds draw the same noise in both entries: the magnitude planes agree within the fp32 bar
    _, mag_f = LF.simulate_low_field_f32(x, 0.5, 5.0, seeds=seeds, _return_magnitude=True)
    mag_f = mag_f.clone()
    _, mag_u = LF.simulate_low_field_u8(u8, 0.5, 5.0, seeds=seeds, _return_magnitude=True)
    err = float((mag_f - mag_u).abs().max())
    print(f"magnitude plane, float entry on u8 / 255 against the uint8 entry: max abs diff {err:.3e}")
    assert err <= F32_BAR
    # odd sizes, seeded
    y = torch.rand((2, 31, 45), device="cuda")
    b = LF.simulate_low_field_f32(y, 0.5, 5.0, seeds=[5, 6])
    assert torch.equal(b, LF.simulate_low_field_f32(y, 0.5, 5.0, seeds=[5, 6])) and not torch.equal(b[0], LF.simulate_low_field_f32(y[:1], 0.5, 5.0, seeds=[7])[0])


def test_float_simulation_checks_and_constant_image():
    x = torch.full((2, 31, 45), 0.3, device="cuda")
    out = LF.simulate_low_field_f32(x, 0.5, 0.0)
    assert torch.all(out == np.float32(0.3))                   # constant magnitude: its own minimum (the existing deviation)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        LF.simulate_low_field_f32(x.cpu())
    with pytest.raises(ValueError):
        LF.simulate_low_field_f32(x.to(torch.uint8))
    with pytest.raises(RuntimeError, match="crop_factor"):
        LF.simulate_low_field_f32(x, 1.2)
    with pytest.raises(RuntimeError, match="keeps nothing"):
        LF.simulate_low_field_f32(torch.zeros((1, 3, 45), device="cuda"), 0.5)
    with pytest.raises(ValueError):
        LF.simulate_low_field_f32(x, 0.5, 5.0, seeds=[1])
    lib = L.load()
    t = torch.zeros(64, device="cuda")
    ws = torch.zeros(2 * 31 * 45 + 8, device="cuda")
    o = torch.zeros((2, 31, 45), device="cuda")

    def call(inp=x.data_ptr(), batch=2, h=31, sigma=0.0, nre=None, work=ws.data_ptr(), out=o.data_ptr()):
        return lib.mrisr_lowfield_simulate_f32(inp, batch, h, 45, 0.5, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), sigma,
                                               nre, None, None, work, out, None)

    assert call(inp=None) == -1 and call(work=None) == -1 and call(out=None) == -1 and call(nre=t.data_ptr()) == -1 and call(sigma=-1.0) == -1
    assert call(batch=0) == -2 and call(h=1) == -2
    assert call() == 0
    torch.cuda.synchronize()


def _check_u8(tag, got, ref_u8, ref, band, block):
    y0, y1, x0, x1 = block
    d = np.abs(got.astype(int) - ref_u8.astype(int))
    v = ref * 255
    tie = np.abs(v - np.rint(v)) <= band
    print(f"{tag}: {int((d > 0).sum())}/{d.size} pixels differ (max {d.max()}), {int(tie.sum())} inside the tie band {band:.3e}")
    assert d.max() <= 1 and (d > 0).mean() <= U8_SHARE and np.all(d[~tie] == 0)
    outside = np.ones(d.shape, dtype=bool)
    outside[y0:y1, x0:x1] = False
    assert np.all(got[outside] == 0)


@pytest.mark.parametrize("c", ["a", "b"])
def test_extract_pairs_on_the_fixture_volumes(golden, c):
    vol = golden[c + "_volume"]
    tw, th = (int(v) for v in golden[c + "_target"])
    knoise = [(n[0], n[1]) for n in golden[c + "_noise"]]
    args = (int(golden["n_slices"]), float(golden["lower_percent"]), float(golden["upper_percent"]), (tw, th),
            float(golden["crop_factor"]), float(golden["noise_std"]))
    ref = E.extract_pairs_host(vol, *args, kspace_noise=knoise)
    idx, hr, lr = E.extract_pairs(torch.from_numpy(vol).cuda(), *args, noise=_planes(knoise))
    assert np.array_equal(idx, ref["indices"]) and np.array_equal(idx, golden[c + "_indices"])
    assert hr.shape == (len(idx), th, tw) and lr.shape == (len(idx), th // 2, tw // 2) and hr.dtype == lr.dtype == torch.uint8
    assert hr.is_cuda and lr.is_cuda
    hr, lr = hr.cpu().numpy(), lr.cpu().numpy()
    h, w = vol.shape[:2]
    for kind, got, method, size in (("hr", hr, E.LANCZOS4, (tw, th)), ("lr", lr, E.AREA, (tw // 2, th // 2))):
        new_w, new_h, x_off, y_off = E.letterbox_geometry(h, w, *size)
        yw, xw = E.resample_taps_np(method, h, new_h)[1], E.resample_taps_np(method, w, new_w)[1]
        gain = np.abs(yw).sum(1).max() * np.abs(xw).sum(1).max()
        bar = 2 * (yw.shape[1] + xw.shape[1] + 4) * 2.0 ** -24 * gain
        for k in range(len(idx)):
            _check_u8(f"volume {c} {kind} slice {idx[k]}", got[k], ref[kind + "_u8"][k], ref[kind][k], 255 * bar,
                      (y_off, y_off + new_h, x_off, x_off + new_w))


def test_constant_slice_becomes_zeros(golden):
    vol = golden["a_volume"].copy()
    vol[:, :, 4] = 731.0
    idx, hr, lr = E.extract_pairs(torch.from_numpy(vol).cuda(), 4, 0.2, 0.8, (64, 48), seeds=1)
    k = list(idx).index(4)
    assert torch.all(hr[k] == 0) and torch.all(lr[k] == 0) and int(hr[k - 1].max()) > 100
    with pytest.raises(RuntimeError, match="CPU tensor"):
        E.extract_pairs(torch.from_numpy(vol))
    with pytest.raises(ValueError):
        E.extract_pairs(torch.from_numpy(vol).cuda(), 4, 0.2, 1.0)


def test_script_writes_the_pairs(tmp_path, golden):
    from PIL import Image
    vol3 = golden["a_volume"]
    vol4 = np.stack([golden["b_volume"], golden["b_volume"][::-1].copy()], axis=3)
    anat = tmp_path / "data" / "set1" / "sub-01" / "anat"
    anat.mkdir(parents=True)
    (tmp_path / "data" / "set1" / "sub-01" / "func").mkdir()

    header = NiftiHeader.new

    write_nifti(str(anat / "sub-01_T1w.nii.gz"), vol3, header(vol3.shape))
    write_nifti(str(anat / "sub-01_task-rest_BOLD.nii"), vol4, header(vol4.shape))
    write_nifti(str(tmp_path / "data" / "set1" / "sub-01" / "func" / "sub-01_T2w.nii.gz"), vol3, header(vol3.shape))      # not in anat/: ignored
    (anat / "sub-01_broken.nii").write_bytes(b"not a scan")                                                              # reported and skipped
    hr_dir, lr_dir = tmp_path / "hr", tmp_path / "lr"
    cmd = [sys.executable, os.path.join(REPO, "scripts", "extract_paired_slices.py"), "--datasets_dir", str(tmp_path / "data"),
           "--hr_output_dir", str(hr_dir), "--lr_output_dir", str(lr_dir), "--n_slices", "3", "--target_size", "64", "48",
           "--noise_std", "4", "--seed", "9"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert any(l.startswith("skipped") and "sub-01_broken" in l for l in r.stdout.splitlines())
    # sorted order: T1w (3-D) first, then the broken file, then the 4-D file's two timepoints
    want, written = {}, 0
    for subject, tp, vol in (("sub-01_T1w", None, vol3), ("sub-01_task-rest_BOLD", 0, vol4[..., 0]), ("sub-01_task-rest_BOLD", 1, vol4[..., 1])):
        idx, hr, lr = E.extract_pairs(torch.from_numpy(np.ascontiguousarray(vol)).cuda(), 3, 0.2, 0.8, (64, 48), 0.5, 4.0,
                                      seeds=LF.derive_seeds(9, None, range(written, written + 3)))
        written += 3
        for k, i in enumerate(idx):
            want[E.pair_filename(subject, int(i), tp)] = (hr[k].cpu().numpy(), lr[k].cpu().numpy())
    assert sorted(os.listdir(hr_dir)) == sorted(want) == sorted(os.listdir(lr_dir)) and len(want) == 9
    assert "sub-01_T1w_s002.png" in want and "sub-01_task-rest_BOLD_T1_s001.png" in want
    for name, (hr, lr) in want.items():
        got_hr, got_lr = np.asarray(Image.open(hr_dir / name)), np.asarray(Image.open(lr_dir / name))
        assert got_hr.shape == (48, 64) and got_lr.shape == (24, 32) and got_hr.dtype == np.uint8
        assert np.array_equal(got_hr, hr) and np.array_equal(got_lr, lr)
