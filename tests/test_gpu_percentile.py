"""Float percentile window on the device (GPU): csrc/percentile.hip + utils/imageops.py against the numpy restatement
(imageops.percentile_bounds_np, itself pinned to np.percentile in tests/test_percentile_host.py).

Bars: the bounds are an exact selection followed by numpy's float32 interpolation, so they EQUAL the restatement by value
(-0.0 == +0.0); the window and its inverse restate numpy float32 arithmetic one operation at a time and are bit-equal.
Shapes are the smallest at which each mechanism can go wrong: n = 1, 2, 3; below one wavefront; a row that is no multiple of
four floats; a partial last workgroup; per-image offsets in a batch (odd image size: images that start unaligned); one 512^2
image whose 64 workgroups merge into one image's histogram."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd import _lib as L                        # noqa: E402
from mri_superresolution_amd.utils import imageops                    # noqa: E402
from test_percentile_host import CLASSES, input_class                # noqa: E402

SHAPES = [(1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 7, 9), (1, 1, 201), (1, 24, 40), (1, 50, 70), (5, 128, 128), (1, 512, 512)]
PAIRS = [(0.5, 99.5), (0.0, 100.0), (50.0, 50.0)]


def _batch(name, shape):
    return np.stack([input_class(name, shape[1:], seed=10 + b) for b in range(shape[0])])


def _check_bounds(imgs, got, q_lo, q_hi, what):
    for b in range(imgs.shape[0]):
        want = imageops.percentile_bounds_np(imgs[b], q_lo, q_hi)
        assert got[b, 0] == want[0] and got[b, 1] == want[1], (what, b, got[b], want)


@pytest.mark.parametrize("name", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bounds_equal_the_numpy_restatement(name, shape):
    imgs = _batch(name, shape)
    x = torch.from_numpy(imgs).cuda()
    for q_lo, q_hi in PAIRS:
        got = imageops.percentile_bounds_f32(x, q_lo, q_hi)
        assert got.shape == (shape[0], 2) and got.dtype == torch.float32
        _check_bounds(imgs, got.cpu().numpy(), q_lo, q_hi, (name, shape, q_lo, q_hi))


def test_images_of_different_classes_in_one_batch_get_their_own_bounds():
    for hw in ((50, 70), (37, 53)):       # 37 x 53 = 1961 floats: every second image starts off a 16-byte boundary
        imgs = np.stack([input_class(name, hw, seed=5) for name in CLASSES])
        got = imageops.percentile_bounds_f32(torch.from_numpy(imgs).cuda())
        _check_bounds(imgs, got.cpu().numpy(), 0.5, 99.5, hw)


def test_bounds_of_an_image_whose_base_is_off_a_16_byte_boundary():
    n = 4099                              # one more than a workgroup's 4096-element step, no multiple of 4
    img = input_class("normal", (1, n), seed=7)
    buf = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(img).cuda().reshape(-1)
    x = buf[1:].view(1, 1, n)
    assert x.data_ptr() % 16 == 4
    for q_lo, q_hi in PAIRS:
        _check_bounds(img[None], imageops.percentile_bounds_f32(x, q_lo, q_hi).cpu().numpy(), q_lo, q_hi, ("unaligned", q_lo, q_hi))


def test_one_workspace_serves_call_after_call_without_clearing():
    nbytes = int(L.load().mrisr_f32_percentile_workspace_bytes(3))
    assert nbytes > 0 and L.load().mrisr_f32_percentile_workspace_bytes(0) == 0
    ws = torch.full((nbytes // 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")      # never zeroed by the caller
    first, second = _batch("mri", (3, 50, 70)), _batch("normal", (3, 50, 70))
    got1 = imageops.percentile_bounds_f32(torch.from_numpy(first).cuda(), workspace=ws).cpu().numpy()
    got2 = imageops.percentile_bounds_f32(torch.from_numpy(second).cuda(), workspace=ws).cpu().numpy()
    _check_bounds(first, got1, 0.5, 99.5, "first call")
    _check_bounds(second, got2, 0.5, 99.5, "second call")


def test_bounds_and_normalise_replay_in_a_graph_on_new_data():
    first, second = _batch("mri", (2, 50, 70)), _batch("normal", (2, 50, 70))
    static_in = torch.from_numpy(first).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        imageops.normalise_percentile_f32(static_in)          # warm-up outside the capture: loads the library, the workspace
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lohi = imageops.normalise_percentile_f32(static_in, return_bounds=True)
    static_in.copy_(torch.from_numpy(second).cuda())           # overwritten in place, then replayed
    graph.replay()
    torch.cuda.synchronize()
    _check_bounds(second, lohi.cpu().numpy(), 0.5, 99.5, "replay")
    assert np.array_equal(out.cpu().numpy()[:, 0], np.stack([_window_np(second[b]) for b in range(2)]))


def _window_np(a, q_lo=0.5, q_hi=99.5):
    """numpy float32, one operation at a time; a constant image -> zeros (reference utils/preprocessing.py:143-153)."""
    lo, hi = imageops.percentile_bounds_np(a, q_lo, q_hi)
    if hi == lo:
        return np.zeros_like(a)
    return (np.clip(a, lo, hi) - lo) / np.float32(hi - lo)


@pytest.mark.parametrize("name", CLASSES)
def test_normalise_is_bit_equal_to_numpy_float32(name):
    for shape in ((1, 1, 3), (3, 50, 70), (1, 128, 128)):
        imgs = _batch(name, shape)
        out, lohi = imageops.normalise_percentile_f32(torch.from_numpy(imgs).cuda(), return_bounds=True)
        assert out.shape == (shape[0], 1, shape[1], shape[2]) and out.dtype == torch.float32
        got = out.cpu().numpy()
        for b in range(shape[0]):
            want = _window_np(imgs[b])
            assert want.dtype == np.float32
            assert np.array_equal(got[b, 0].view(np.uint32), want.view(np.uint32)), (name, shape, b)
        if name == "constant":
            assert not got.any()
    single = imageops.normalise_percentile_f32(torch.from_numpy(_batch("mri", (1, 24, 40))[0]).cuda())       # (H,W) input
    assert single.shape == (1, 1, 24, 40)


def test_restore_is_bit_equal_to_numpy_float32():
    rng = np.random.default_rng(7)
    y = rng.uniform(-0.2, 1.2, (4, 1, 50, 70)).astype(np.float32)
    y[0, 0, 0, :4] = [0.0, 1.0, -0.0, 0.5]
    lohi = np.array([[0.0, 3000.0], [-123.456, 789.012], [17.0, 17.0], [1e-3, 4095.7]], dtype=np.float32)
    got = imageops.restore_window(torch.from_numpy(y).cuda(), torch.from_numpy(lohi).cuda())
    assert got.shape == y.shape and got.dtype == torch.float32
    for b in range(4):
        lo, hi = lohi[b]
        want = np.clip(y[b], np.float32(0), np.float32(1)) * np.float32(hi - lo) + lo      # a rounded product, then a rounded sum
        assert want.dtype == np.float32 and np.array_equal(got[b].cpu().numpy(), want), b
    got3 = imageops.restore_window(torch.from_numpy(y[:, 0]).cuda(), torch.from_numpy(lohi).cuda())       # (B,H,W) input
    assert torch.equal(got3, got[:, 0])


def test_normalise_and_restore_off_a_16_byte_boundary():
    """One image of 4099 floats (one more than whole 4096-element steps, no multiple of 4), input and output of both calls at a
    base 4 bytes past a 16-byte boundary."""
    n = 4099
    img = input_class("normal", (1, n), seed=8)
    buf = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(img).cuda().reshape(-1)
    x = buf[1:].view(1, 1, n)
    assert x.data_ptr() % 16 == 4
    out, lohi = imageops.normalise_percentile_f32(x, return_bounds=True)
    want = _window_np(img)
    assert np.array_equal(out[0, 0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    buf[1:] = out.reshape(-1)                                  # the normalised image, off the boundary too
    lo, hi = lohi[0].cpu().numpy()
    for dtype in (torch.float32, torch.int16):
        obuf = torch.zeros(n + 8, dtype=dtype, device="cuda")
        k = 1 if dtype == torch.float32 else 2                 # 4 bytes past the boundary
        dst = obuf[k:k + n].view(1, 1, n)
        assert dst.data_ptr() % 16 == 4
        imageops.restore_window(x, lohi, dtype=dtype, out=dst)
        r = np.clip(want, np.float32(0), np.float32(1)) * np.float32(hi - lo) + lo
        r = r if dtype == torch.float32 else np.clip(np.rint(r), -32768, 32767).astype(np.int16)
        assert np.array_equal(dst.cpu().numpy().reshape(1, n), r), dtype


def test_restore_int16_rounds_half_to_even_and_saturates():
    # window (lo, hi) = (-40000, 40000): y in [0, 1] spans both ends of int16; window (0, 8): y = k / 16 lands on .5 ties exactly
    ties = (np.arange(0, 17, dtype=np.float32) / np.float32(16)).reshape(1, 1, 1, 17)
    wide = np.linspace(0, 1, 17, dtype=np.float32).reshape(1, 1, 1, 17)
    neg_ties = ties.copy()
    y = np.concatenate([ties, wide, neg_ties])
    lohi = np.array([[0.0, 8.0], [-40000.0, 40000.0], [-8.5, -0.5]], dtype=np.float32)
    got = imageops.restore_window(torch.from_numpy(y).cuda(), torch.from_numpy(lohi).cuda(), dtype=torch.int16)
    assert got.dtype == torch.int16 and got.shape == y.shape
    saw_tie = saw_low = saw_high = False
    for b in range(3):
        lo, hi = lohi[b]
        r = np.clip(y[b], np.float32(0), np.float32(1)) * np.float32(hi - lo) + lo
        want = np.clip(np.rint(r), -32768, 32767).astype(np.int16)
        assert np.array_equal(got[b].cpu().numpy(), want), (b, got[b].cpu().numpy(), want)
        saw_tie |= bool((np.abs(r - np.trunc(r)) == 0.5).any())
        saw_low |= bool((r < -32768).any())
        saw_high |= bool((r > 32767).any())
    assert saw_tie and saw_low and saw_high


def test_refusals():
    good = torch.zeros((2, 8, 8), dtype=torch.float32)
    for fn in (imageops.percentile_bounds_f32, imageops.normalise_percentile_f32):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(good)
        with pytest.raises(ValueError):
            fn(good.cuda().double())
        with pytest.raises(ValueError):
            fn(good.cuda().to(torch.uint8))
        with pytest.raises(ValueError):
            fn(good.cuda().reshape(2, 1, 8, 8))
        with pytest.raises(ValueError):
            fn(good.cuda().reshape(-1))
    with pytest.raises(RuntimeError, match="percentiles"):
        imageops.percentile_bounds_f32(good.cuda(), 60.0, 40.0)
    lohi = torch.zeros((2, 2), dtype=torch.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imageops.restore_window(good, lohi.cuda())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imageops.restore_window(good.cuda(), lohi)
    with pytest.raises(ValueError):
        imageops.restore_window(good.cuda().half(), lohi.cuda())
    with pytest.raises(ValueError):
        imageops.restore_window(good.cuda()[0], lohi.cuda())
    with pytest.raises(ValueError):
        imageops.restore_window(good.cuda(), lohi.cuda()[:1])
    with pytest.raises(ValueError):
        imageops.restore_window(good.cuda(), lohi.cuda(), dtype=torch.uint8)
