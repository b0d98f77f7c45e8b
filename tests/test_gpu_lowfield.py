"""Low-field simulation on the device (GPU): csrc/lowfield.hip through utils/lowfield.simulate_low_field_u8 against the
float64 restatement of the reference (utils/lowfield.simulate_low_field_host, itself pinned to the reference's recorded
outputs in tests/test_lowfield_host.py), the seeded noise generator, the argument checks, DevicePairLoader(simulate_lr=...)
and the two command lines.

Bars (set before the kernel existed): the fp32 LR plane within 5e-5 absolute of the float64 host plane (the project's fp32
absolute bar; an fp32 CPU emulation of the same arithmetic stays below 5.1e-7 of the range up to 512^2); the uint8 image at
most 1 grey level away on at most 1 % of the pixels of each image (truncation makes exact ties discontinuous)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mri_superresolution_amd import _lib as L                                            # noqa: E402
from mri_superresolution_amd.utils import lowfield as LF                                 # noqa: E402
from mri_superresolution_amd.utils.dataset import MRISuperResDataset                     # noqa: E402
from mri_superresolution_amd.utils.gpu_augment import DevicePairLoader                   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, 32), (48, 40), (30, 44), (64, 96)]
KINDS = ["uniform", "constant", "binary", "ramp"]
F32_BAR, U8_SHARE = 5e-5, 0.01


def _image(rng, kind, h, w, k):
    if kind == "uniform":
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    if kind == "constant":
        return np.full((h, w), (37, 128, 255)[k % 3], dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy * (k + 1) + xx * 3) * 255.0 / ((h - 1) * (k + 1) + (w - 1) * 3)).astype(np.uint8)


def _kspace_noise(rng, h, w, noise_std):
    s = (noise_std / 255.0) * math.sqrt(h * w) / 10            # preprocessing.py:274
    return rng.normal(0, s, (h, w)), rng.normal(0, s, (h, w))


def _check_batch(images, knoise, crop, check_u8=True):
    """images: list of (H,W) uint8; knoise: list of (N_re, N_im) k-space arrays; one device call for the batch."""
    n_img = np.stack([LF.image_noise_from_kspace(a, b) for a, b in knoise])
    planes = (torch.from_numpy(n_img.real.astype(np.float32)).cuda(), torch.from_numpy(n_img.imag.astype(np.float32)).cuda())
    u8, f32 = LF.simulate_low_field_u8(torch.from_numpy(np.stack(images)).cuda(), crop, noise=planes, return_float=True)
    u8, f32 = u8.cpu().numpy(), f32.cpu().numpy()
    for k, (img, kn) in enumerate(zip(images, knoise)):
        ref = LF.simulate_low_field_host(img, crop, kspace_noise=kn)
        err = np.abs(f32[k].astype(np.float64) - ref["lr"]).max()
        d = np.abs(u8[k].astype(int) - ref["lr_u8"].astype(int))
        print(f"image {k} {img.shape}: fp32 plane max abs err {err:.3e}, uint8 differing {int((d > 0).sum())}/{d.size}, max {d.max()}")
        assert err <= F32_BAR
        assert d.max() <= 1 and (not check_u8 or (d > 0).mean() <= U8_SHARE)
        # the uint8 image is the truncation of the fp32 plane the kernel reports
        assert np.array_equal(u8[k], np.clip(f32[k] * np.float32(255), 0, 255).astype(np.uint8))


def test_fixture_cases_match_host_restatement(golden_dir):
    g = np.load(os.path.join(golden_dir, "lowfield.npz"))
    for shape in ("32x32", "48x40", "30x44"):
        keys = [f"{shape}_n0", f"{shape}_n5"]
        _check_batch([g[k + "_image"] for k in keys], [(g[k + "_noise_re"], g[k + "_noise_im"]) for k in keys],
                     float(g["crop_factor"]))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_explicit_noise(kind, shape):
    h, w = shape
    rng = np.random.default_rng(KINDS.index(kind) * 10000 + h * 100 + w)
    images = [_image(rng, kind, h, w, k) for k in range(3)]              # different images and different noise per batch entry
    knoise = [_kspace_noise(rng, h, w, (5.0, 2.0, 9.0)[k]) for k in range(3)]
    _check_batch(images, knoise, 0.5)


def test_other_crop_factors_and_no_noise():
    """crop_factor 1 keeps all of k-space: without noise Y = x, the renormalisation maps the 8-bit grid onto itself and
    every 2x2 mean times 255 is a multiple of 1/4 - a quarter of the pixels are EXACT truncation ties, which fp32 and
    float64 rounding land on either side of.  The share rule does not apply there: fp32 plane and <= 1 grey level only."""
    rng = np.random.default_rng(5)
    for f in (0.3, 0.77, 1.0):
        images = [_image(rng, "uniform", 48, 40, k) for k in range(2)]
        _check_batch(images, [(np.zeros((48, 40)), np.zeros((48, 40)))] * 2, f, check_u8=f < 1.0)
        got = LF.simulate_low_field_u8(torch.from_numpy(np.stack(images)).cuda(), f, noise_std=0.0)
        planes = (torch.zeros((2, 48, 40), device="cuda"), torch.zeros((2, 48, 40), device="cuda"))
        assert torch.equal(got, LF.simulate_low_field_u8(torch.from_numpy(np.stack(images)).cuda(), f, noise=planes))


def test_constant_image_takes_the_max_equals_min_rule():
    """A constant image has max x == min x, and without noise a constant magnitude: the reference divides 0 by 0, this
    build returns min x everywhere (with noise the renormalised span is 0 and the result is the same)."""
    x = torch.full((2, 32, 48), 77, dtype=torch.uint8, device="cuda")
    x[1] = 200
    for noise_std in (0.0, 5.0):
        u8, f32 = LF.simulate_low_field_u8(x, 0.5, noise_std=noise_std, seeds=[1, 2], return_float=True)
        for k, v in enumerate((77, 200)):
            assert torch.all(u8[k] == v) and torch.all(f32[k] == float(np.float32(v) / np.float32(255)))
    host = LF.simulate_low_field_host(np.full((32, 48), 77, dtype=np.uint8), 0.5, noise_std=0.0)
    assert np.array_equal(host["lr_u8"], np.full((16, 24), 77, dtype=np.uint8))


def test_seeded_noise_is_reproducible():
    rng = np.random.default_rng(2)
    x = torch.from_numpy(np.stack([_image(rng, "uniform", 64, 96, k) for k in range(3)])).cuda()
    a = LF.simulate_low_field_u8(x, 0.5, 5.0, seeds=[11, 12, 2 ** 63 + 5])
    b = LF.simulate_low_field_u8(x, 0.5, 5.0, seeds=[11, 12, 2 ** 63 + 5])
    c = LF.simulate_low_field_u8(x, 0.5, 5.0, seeds=[11, 13, 2 ** 63 + 5])
    assert torch.equal(a, b)
    assert torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1]) and torch.equal(a[2], c[2])
    # same image, same seed in different batch slots: the same output; a seed's high word matters
    y = x[:1].repeat(3, 1, 1)
    d = LF.simulate_low_field_u8(y, 0.5, 5.0, seeds=[7, 7, 7 + 2 ** 32])
    assert torch.equal(d[0], d[1]) and not torch.equal(d[0], d[2])
    # noise_std = 0 ignores the seed
    e = LF.simulate_low_field_u8(x, 0.5, 0.0, seeds=[1, 2, 3])
    assert torch.equal(e, LF.simulate_low_field_u8(x, 0.5, 0.0, seeds=[4, 5, 6])) and not torch.equal(e, a)
    assert torch.equal(e, LF.simulate_low_field_u8(x, 0.5, 0.0))
    # an int seed, and fresh seeds when none are given
    assert torch.equal(LF.simulate_low_field_u8(x, 0.5, 5.0, seeds=3), LF.simulate_low_field_u8(x, 0.5, 5.0, seeds=LF.derive_seeds(3, None, range(3))))
    assert not torch.equal(LF.simulate_low_field_u8(x, 0.5, 5.0), LF.simulate_low_field_u8(x, 0.5, 5.0))


def test_seeded_noise_has_rician_moments():
    """Constant 128 (0.502) inside a frame that holds 0 and 255, so that the extrema are fixed.  m = |Y + n|, n ~ CN(0, sigma^2)
    per component, sigma = noise_std / 2550, is Rician around nu = |Y| pixel by pixel (nu from the float64 host restatement
    without noise; the frame rings into the interior).  Over the 256 x 256 interior pixels (65536):
      mean of  m - E[m | nu]            is 0 within 5 standard errors, SE = sqrt(mean Var[m | nu] / N)
      mean of (m - E[m | nu])^2         is mean Var[m | nu] within 5 standard errors, SE = sample std of the squares / sqrt(N)
    Moments: E[m^2] = nu^2 + 2 sigma^2 exactly; E[m] = nu + sigma^2 / (2 nu) + sigma^4 / (8 nu^3), the large-nu series whose next
    term is O(sigma^6 / nu^5), below 1e-13 for nu >= 0.2.  fp32 rounding of Y (below 1e-6) is a tenth of the mean's SE."""
    noise_std, fr = 10.0, 8
    sigma = noise_std / 2550.0
    img = np.full((256 + 2 * fr, 256 + 2 * fr), 128, dtype=np.uint8)
    img[:fr], img[-fr:], img[:, :fr], img[:, -fr:] = 0, 255, 0, 255
    nu = LF.simulate_low_field_host(img, 0.5, noise_std=0.0)["magnitude"][fr:-fr, fr:-fr]
    assert nu.min() >= 0.2
    _, mag = LF.simulate_low_field_u8(torch.from_numpy(img).cuda(), 0.5, noise_std, seeds=[12345], _return_magnitude=True)
    m = mag[0].cpu().numpy().astype(np.float64)[fr:-fr, fr:-fr]
    mean = nu + sigma ** 2 / (2 * nu) + sigma ** 4 / (8 * nu ** 3)
    var = nu ** 2 + 2 * sigma ** 2 - mean ** 2
    d = m - mean
    n = d.size
    assert n >= 65536
    se_mean = math.sqrt(var.mean() / n)
    se_var = (d ** 2).std(ddof=1) / math.sqrt(n)
    print(f"mean residual {d.mean():.3e} (SE {se_mean:.3e}), variance {np.mean(d ** 2):.6e} vs {var.mean():.6e} (SE {se_var:.3e})")
    assert abs(d.mean()) <= 5 * se_mean
    assert abs(np.mean(d ** 2) - var.mean()) <= 5 * se_var


def test_argument_checks():
    lib = L.load()
    x = torch.zeros((1, 32, 32), dtype=torch.uint8, device="cuda")
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    ws = torch.zeros(32 * 32 + 4, dtype=torch.float32, device="cuda")
    out = torch.zeros((1, 16, 16), dtype=torch.uint8, device="cuda")
    E_ARG, E_SHAPE = -1, -2

    def call(high=x.data_ptr(), h=32, w=32, f=0.5, tab=t.data_ptr(), sigma=0.0, nre=None, nim=None, work=ws.data_ptr(),
             o=out.data_ptr(), batch=1):
        return lib.mrisr_lowfield_simulate(high, batch, h, w, f, tab, tab, tab, tab, sigma, nre, nim, None, work, o, None, None)

    assert call(h=31) == E_SHAPE and call(w=33) == E_SHAPE and call(h=2) == E_SHAPE and call(w=2) == E_SHAPE
    assert call(batch=0) == E_SHAPE
    for f in (0.0, -1.0, 1.5, float("nan")):
        assert call(f=f) == E_ARG
    assert call(f=0.05) == E_ARG and b"keeps nothing" in lib.mrisr_last_error()
    assert call(high=None) == E_ARG and b"null" in lib.mrisr_last_error()
    assert call(tab=None) == E_ARG and call(work=None) == E_ARG and call(o=None) == E_ARG
    assert call(nre=t.data_ptr()) == E_ARG and call(sigma=-1.0) == E_ARG
    assert call() == 0
    torch.cuda.synchronize()
    # Python layer
    with pytest.raises(RuntimeError, match="CPU tensor"):
        LF.simulate_low_field_u8(torch.zeros((32, 32), dtype=torch.uint8))
    with pytest.raises(ValueError):
        LF.simulate_low_field_u8(torch.zeros((32, 32), dtype=torch.float32, device="cuda"))
    with pytest.raises(RuntimeError, match="even"):
        LF.simulate_low_field_u8(torch.zeros((31, 32), dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="crop_factor"):
        LF.simulate_low_field_u8(x, 1.2)
    with pytest.raises(ValueError):
        LF.simulate_low_field_u8(x, 0.5, 5.0, seeds=[1, 2])
    with pytest.raises(RuntimeError, match="CPU tensor"):
        LF.simulate_low_field_u8(x, 0.5, noise=(torch.zeros((1, 32, 32)), torch.zeros((1, 32, 32))))


def _img(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(110 + 70 * np.sin(yy / 7.0) * np.cos(xx / 5.0) + rng.normal(0, 12, (h, w)), 0, 255).astype(np.uint8)


def _make_dirs(tmp_path, n, h, w):
    """n HR slices of (h, w); the stored LR files are a CONSTANT 200, so any use of them shows."""
    from PIL import Image
    rng = np.random.default_rng(1)
    hr, lr = tmp_path / "hr", tmp_path / "lr"
    hr.mkdir(), lr.mkdir()
    for i in range(n):
        Image.fromarray(_img(rng, h, w)).save(hr / f"sub-S{i % 3}_s{i:03d}.png")
        Image.fromarray(np.full((h // 2, w // 2), 200, dtype=np.uint8)).save(lr / f"sub-S{i % 3}_s{i:03d}.png")
    return hr, lr


def test_loader_draws_lr_from_hr(tmp_path):
    hr, lr = _make_dirs(tmp_path, 10, 48, 64)
    ds = MRISuperResDataset(str(hr), str(lr), augmentation=False)
    sim = {"kspace_crop_factor": 0.5, "noise_std": 5.0}
    ids = [7, 2, 5, 0, 9, 3, 1]
    val = DevicePairLoader(ds, 3, ids, shuffle=False, augmentation=False, seed=4, simulate_lr=sim)
    got = list(val)
    low, high = torch.cat([b[0] for b in got]), torch.cat([b[1] for b in got])
    assert low.shape == (7, 1, 24, 32) and high.shape == (7, 1, 48, 64) and low.dtype == torch.float32
    assert torch.equal(high.cpu(), torch.stack([ds[i][1] for i in ids]))        # ToTensor of the HR files, as without the flag
    high_u8 = torch.stack([(ds[i][1][0] * 255).round().to(torch.uint8) for i in ids]).cuda()
    # the loader's sample index is the position in its index set; no epoch for a loader that neither shuffles nor augments
    want = LF.simulate_low_field_u8(high_u8, seeds=LF.derive_seeds(4, None, range(7)), **sim)
    assert torch.equal(low[:, 0].cpu(), want.cpu().float() / 255)
    assert float((low.cpu() == torch.tensor(200.0) / 255).float().mean()) < 0.05      # nothing of the stored (constant 200) LR files
    again = torch.cat([b[0] for b in val])                      # second epoch of the validation loader: identical
    assert val.epoch == 2 and torch.equal(again, low)
    # streaming mode yields the same batches
    val2 = DevicePairLoader(ds, 3, ids, shuffle=False, augmentation=False, seed=4, simulate_lr=sim, max_resident_bytes=0)
    assert not val2.resident and torch.equal(torch.cat([b[0] for b in val2]), low)
    # shuffled training loader: the same sample gets another noise draw in the next epoch, reproducibly from (seed, epoch)
    tr = DevicePairLoader(ds, 4, None, shuffle=True, augmentation=False, seed=5, simulate_lr=sim)
    lows, highs = [], []
    for _ in range(2):
        batches = list(tr)
        lows.append(torch.cat([b[0] for b in batches]))
        highs.append(torch.cat([b[1] for b in batches]))
    key = [h.sum((1, 2, 3)) for h in highs]                     # identifies the sample (HR is untouched)
    for s in range(10):
        i0, i1 = int((key[0] == key[0][s]).nonzero()[0]), int((key[1] == key[0][s]).nonzero()[0])
        assert torch.equal(highs[0][i0], highs[1][i1]) and not torch.equal(lows[0][i0], lows[1][i1])
        assert (lows[0][i0] - lows[1][i1]).abs().max() <= 40 / 255          # the same image under another noise draw
    tr.set_epoch(0)
    assert torch.equal(torch.cat([b[0] for b in tr]), lows[0])
    # without simulate_lr the stored files are what comes out (unchanged behaviour)
    plain = next(iter(DevicePairLoader(ds, 3, ids, shuffle=False, augmentation=False)))
    assert torch.all(plain[0].cpu() == torch.tensor(200.0) / 255)


def test_simulate_lr_cli_and_training_flag(tmp_path):
    from PIL import Image
    hr, lr = _make_dirs(tmp_path, 4, 64, 64)
    out = tmp_path / "lr_sim"
    cmd = [sys.executable, os.path.join(REPO, "scripts", "simulate_lr.py"), "--full_res_dir", str(hr), "--low_res_dir", str(out),
           "--noise_std", "4", "--seed", "9", "--batch_size", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    names = sorted(os.listdir(hr))
    assert sorted(os.listdir(out)) == names and len(names) == 4
    high = torch.from_numpy(np.stack([np.asarray(Image.open(hr / n)) for n in names])).cuda()
    want = LF.simulate_low_field_u8(high, 0.5, 4.0, seeds=LF.derive_seeds(9, None, range(4))).cpu().numpy()
    for k, n in enumerate(names):
        got = np.asarray(Image.open(out / n))
        assert got.shape == (32, 32) and got.dtype == np.uint8 and np.array_equal(got, want[k])
    # train.py --gpu_data --simulate_lr: one tiny epoch, finite loss; the constant LR files only name the pairs
    train = [sys.executable, os.path.join(REPO, "scripts", "train.py"), "--full_res_dir", str(hr), "--low_res_dir", str(lr),
             "--base_filters", "16", "--batch_size", "2", "--epochs", "1", "--num_workers", "0", "--seed", "1",
             "--checkpoint_dir", str(tmp_path / "ck"), "--log_dir", str(tmp_path / "logs"), "--validation_split", "0.25"]
    r = subprocess.run(train + ["--gpu_data", "--simulate_lr", "--noise_std", "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    msgs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    ep = [m for m in msgs if m["type"] == "epoch_summary"]
    assert len(ep) == 1 and np.isfinite(ep[0]["train_loss"]) and np.isfinite(ep[0]["val_loss"])
    assert any("simulated on the device" in m.get("message", "") for m in msgs if m["type"] == "info")
    bad = subprocess.run(train + ["--simulate_lr"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "--gpu_data" in bad.stderr
