"""Device-resident data pipeline (GPU): utils/gpu_augment.py + the augmentation kernels of csrc/image.hip against PIL,
which is what the reference's dataset (utils/dataset.py:138-175, through torchvision's functional wrappers) runs on the
host, and utils/dataset.py (host path) for the un-augmented items.

PARITY UNPINNED against the reference module itself (it needs torchvision, absent).  Bars: flip / brightness / contrast /
ToTensor bit-exact vs PIL; rotation (NEAREST, mean fill): <= 0.5 % of the pixels may differ (float32 vs PIL's double
coordinate arithmetic on pixel-boundary ties); noise: distribution checks."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mri_superresolution_amd import _lib as L                                      # noqa: E402
from mri_superresolution_amd.utils.dataset import MRISuperResDataset               # noqa: E402
from mri_superresolution_amd.utils.gpu_augment import DevicePairLoader, _u8_means  # noqa: E402


def _img(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    a = 110 + 70 * np.sin(yy / 7.0) * np.cos(xx / 5.0) + rng.normal(0, 12, (h, w))
    return np.clip(a, 0, 255).astype(np.uint8)


def _run(img, flip=0, angle=None, brightness=1.0, contrast=1.0, sigma=0.0, seed=0, off=0):
    """``off``: the image and the stage start this many bytes past a 16-byte boundary."""
    buf = torch.zeros(img.size + off, dtype=torch.uint8, device="cuda")
    buf[off:] = torch.from_numpy(img).cuda().reshape(-1)
    x = buf[off:].view((1,) + img.shape)
    geo = (L.AugGeo * 1)()
    g = geo[0]
    g.cos_a, g.sin_a, g.rotate, g.flip, g.fill, g.brightness = 1.0, 0.0, 0, flip, 0, brightness
    if angle is not None:
        a = -math.radians(angle)
        g.rotate, g.cos_a, g.sin_a = 1, math.cos(a), math.sin(a)
    pho = (L.AugPhoto * 1)()
    pho[0].contrast, pho[0].mean, pho[0].noise_sigma, pho[0].seed = contrast, 0, sigma, seed
    gd = torch.frombuffer(bytearray(bytes(geo)), dtype=torch.uint8).cuda()
    pd = torch.frombuffer(bytearray(bytes(pho)), dtype=torch.uint8).cuda()
    st = L.stream_ptr()
    stage = torch.zeros(img.size + off, dtype=torch.uint8, device="cuda")[off:].view(x.shape)
    assert x.data_ptr() % 16 == off and stage.data_ptr() % 16 == off
    L.call("mrisr_augment_geo_u8", x.data_ptr(), stage.data_ptr(), 1, img.shape[0], img.shape[1], gd.data_ptr(),
           _u8_means(x).data_ptr(), st)
    out = torch.empty((1, 1) + img.shape, dtype=torch.float32, device="cuda")
    L.call("mrisr_augment_finish_u8", stage.data_ptr(), out.data_ptr(), 1, img.size, pd.data_ptr(),
           _u8_means(stage).data_ptr(), st)
    return stage[0].cpu().numpy(), out[0, 0].cpu().numpy()


def test_augmentation_stages_match_pil():
    from PIL import Image, ImageEnhance
    rng = np.random.default_rng(0)
    img = _img(rng, 48, 64)
    pil = Image.fromarray(img)
    # ToTensor alone
    stage, out = _run(img)
    assert np.array_equal(stage, img) and np.array_equal(out, img.astype(np.float32) / 255.0)
    # flip
    stage, _ = _run(img, flip=1)
    assert np.array_equal(stage, np.asarray(pil.transpose(Image.FLIP_LEFT_RIGHT)))
    # brightness / contrast, both sides of 1 (interpolating and extrapolating branches of Image.blend)
    for f in (0.9, 0.937, 1.0, 1.061, 1.1):
        stage, _ = _run(img, brightness=f)
        assert np.array_equal(stage, np.asarray(ImageEnhance.Brightness(pil).enhance(f))), f
        _, out = _run(img, contrast=f)
        ref = np.asarray(ImageEnhance.Contrast(pil).enhance(f)).astype(np.float32) / 255.0
        assert np.array_equal(out, ref), (f, np.abs(out - ref).max())
    # rotation: NEAREST, no expand, fill = int(mean) (TF.rotate(img, angle, fill=int(mean * 255)))
    fill = int(img.astype(np.float32).mean())
    for ang in (-5.0, -1.3, 0.7, 3.0, 5.0):
        stage, _ = _run(img, angle=ang)
        ref = np.asarray(pil.rotate(ang, resample=Image.NEAREST, fillcolor=fill))
        diff = (stage != ref).mean()
        assert diff <= 0.005, (ang, diff)
        if abs(ang) >= 3.0:
            assert fill in (stage[0, 0], stage[0, -1])             # a corner that comes from outside the image
    # flip + rotate + brightness in the reference's order
    stage, _ = _run(img, flip=1, angle=4.0, brightness=1.05)
    ref = ImageEnhance.Brightness(pil.transpose(Image.FLIP_LEFT_RIGHT).rotate(4.0, resample=Image.NEAREST, fillcolor=fill)).enhance(1.05)
    assert (stage != np.asarray(ref)).mean() <= 0.005


def test_augmentation_stages_off_a_16_byte_boundary():
    """37 x 53 = 1961 pixels (no multiple of 4), image and stage 1 byte past a 16-byte boundary: the exact stages against PIL."""
    from PIL import Image, ImageEnhance
    img = _img(np.random.default_rng(4), 37, 53)
    pil = Image.fromarray(img)
    stage, out = _run(img, off=1)
    assert np.array_equal(stage, img) and np.array_equal(out, img.astype(np.float32) / 255.0)
    stage, _ = _run(img, flip=1, brightness=1.061, off=1)
    assert np.array_equal(stage, np.asarray(ImageEnhance.Brightness(pil.transpose(Image.FLIP_LEFT_RIGHT)).enhance(1.061)))
    _, out = _run(img, contrast=0.937, off=1)
    assert np.array_equal(out, np.asarray(ImageEnhance.Contrast(pil).enhance(0.937)).astype(np.float32) / 255.0)


def test_noise_is_gaussian_in_uint8_units_and_seeded():
    img = np.full((128, 128), 100, dtype=np.uint8)
    _, a = _run(img, sigma=2.55, seed=1234)
    _, b = _run(img, sigma=2.55, seed=1234)
    _, c = _run(img, sigma=2.55, seed=99)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    d = a * 255.0 - 100.0                       # truncation shifts the mean by about -0.5
    assert abs(d.mean() + 0.5) < 0.1 and abs(d.std() - math.sqrt(2.55 ** 2 + 1 / 12.0)) < 0.1
    assert np.all(a * 255.0 == np.round(a * 255.0))                # still 8-bit levels


def _make_dataset(tmp_path, n=10, h=24, w=32):
    from PIL import Image
    rng = np.random.default_rng(1)
    hr, lr = tmp_path / "hr", tmp_path / "lr"
    hr.mkdir(), lr.mkdir()
    for i in range(n):
        Image.fromarray(_img(rng, 2 * h, 2 * w)).save(hr / f"sub-S{i % 3}_s{i:03d}.png")
        Image.fromarray(_img(rng, h, w)).save(lr / f"sub-S{i % 3}_s{i:03d}.png")
    Image.fromarray(_img(rng, 2 * h, 2 * w)).save(hr / "sub-S9_unpaired.png")     # HR file without an LR twin
    return MRISuperResDataset(str(hr), str(lr), augmentation=False)


def test_device_loader_equals_host_dataset_without_augmentation(tmp_path):
    ds = _make_dataset(tmp_path)
    assert len(ds) == 10 and ds.get_unique_subjects() and len(ds.get_subject_indices("S0")) == 4
    assert ds.metadata[0]["filename"] == ds.valid_pairs[0] and ds.metadata[0]["subject"] == "S0"
    ids = [7, 2, 5, 0, 9, 3, 1]
    ld = DevicePairLoader(ds, 3, ids, shuffle=False, augmentation=False)
    assert len(ld) == 3 and ld.resident
    got = list(ld)
    low = torch.cat([b[0] for b in got]).cpu()
    high = torch.cat([b[1] for b in got]).cpu()
    for k, i in enumerate(ids):
        l_ref, h_ref = ds[i]
        assert torch.equal(low[k], l_ref) and torch.equal(high[k], h_ref)
    # streaming mode (pinned host copy + side-stream prefetch) yields the same batches
    ld2 = DevicePairLoader(ds, 3, ids, shuffle=False, augmentation=False, max_resident_bytes=0)
    assert not ld2.resident
    for (a, b), (c, d) in zip(got, ld2):
        assert torch.equal(a, c) and torch.equal(b, d)
    # shuffling: a permutation per epoch, reproducible from (seed, epoch)
    ld3 = DevicePairLoader(ds, 4, None, shuffle=True, augmentation=False, seed=5)
    e0 = torch.cat([b[0] for b in ld3]).cpu()
    e1 = torch.cat([b[0] for b in ld3]).cpu()
    assert e0.shape[0] == 10 and not torch.equal(e0, e1)
    assert torch.equal(e0.sum((1, 2, 3)).sort().values, e1.sum((1, 2, 3)).sort().values)
    ld3.set_epoch(0)
    assert torch.equal(torch.cat([b[0] for b in ld3]).cpu(), e0)


def test_device_loader_paired_augmentation_properties(tmp_path):
    ds = _make_dataset(tmp_path, n=64)
    params = {"flip_prob": 1.0, "rotate_prob": 0.0, "brightness_prob": 0.0, "contrast_prob": 0.0, "noise_prob": 0.0}
    ds.params.update(params)
    ld = DevicePairLoader(ds, 16, None, shuffle=False, augmentation=True)
    low, high = next(iter(ld))
    l0, h0 = ds[0]
    assert torch.equal(low[0].cpu(), l0.flip(-1)) and torch.equal(high[0].cpu(), h0.flip(-1))     # both images of the pair
    # noise touches the low-resolution image only
    ds.params.update({"flip_prob": 0.0, "noise_prob": 1.0})
    low, high = next(iter(DevicePairLoader(ds, 16, None, shuffle=False, augmentation=True)))
    assert torch.equal(high[0].cpu(), h0) and not torch.equal(low[0].cpu(), l0)
    assert (low[0].cpu() - l0).abs().max() <= 16 / 255.0
    # default probabilities: roughly half of the pairs come out flipped / rotated, values stay in [0,1]
    ds.params.update({"flip_prob": 0.5, "rotate_prob": 0.5, "brightness_prob": 0.3, "contrast_prob": 0.3, "noise_prob": 0.2})
    changed = 0
    for low, high in DevicePairLoader(ds, 16, None, shuffle=False, augmentation=True, seed=3):
        assert low.min() >= 0 and low.max() <= 1 and high.dtype == torch.float32 and low.shape[1:] == (1, 24, 32)
        changed += sum(int(not torch.equal(low[k].cpu(), ds[0][0])) for k in range(low.shape[0]))
    assert changed == 64 or changed >= 48
