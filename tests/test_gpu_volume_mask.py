"""Foreground-masked volume evaluation (GPU): csrc/volume_mask.hip against foreground_mask_np / dilate_np / erode_np bit for bit,
the masked instantiation of csrc/volume_metrics.hip against the float64 specification volume_metrics_np(mask=...),
evaluate_volume(mask=...) and scripts/evaluate_volume.py --mask.

Bars, per region (the project's own rule, restated here).  mse, rmse and mae: 1e-6 relative, PSNR 1e-5 dB - the kernel forms a - b,
|a - b| and (a - b)^2 exactly in double; only the order of the double sums differs.  SSIM: max(5e-6, 4 dev), dev the distance of the
same masked mean of a float32 torch-CPU restatement of the map from the float64 specification - a bar measured against a reference
computation, never against the kernel.  The count of mask voxels is exact.  Everything else here is bit-equal."""
import csv
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd import _lib as L                                # noqa: E402
from mri_superresolution_amd import volume_eval as V                         # noqa: E402
from mri_superresolution_amd.models.unet_model import UNetSuperRes          # noqa: E402
from mri_superresolution_amd.utils.evalops import METRIC_COLUMNS             # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, write_nifti     # noqa: E402
from scripts import evaluate_volume as cli                                   # noqa: E402

# ---------------------------------------------------------------- Otsu mask

# (64, 64, 80): 327680 voxels = 20 workgroups of the counts pass merge into one histogram; (70, 37, 45): an odd count (scalar tail)
OTSU_SHAPES = [(1, 1, 1), (3, 5, 7), (12, 11, 10), (70, 37, 45), (64, 64, 80)]
KINDS = ["signed", "int12", "constant"]


def otsu_volume(shape, kind, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if kind == "constant":
        return np.full(shape, -12.25, dtype=np.float32)
    if kind == "signed":                                        # negative intensities, two modes
        v = rng.normal(-200.0, 25.0, n)
        bright = rng.uniform(size=n) < 0.3
        v[bright] = rng.normal(150.0, 40.0, int(bright.sum()))
        return v.astype(np.float32).reshape(shape)
    # 12-bit-like integers on [0, 4096]: scale = 1 / 16 exactly, so every multiple of 16 sits exactly on a bin edge
    v = np.rint(np.abs(rng.normal(0, 60, n)))
    bright = rng.uniform(size=n) < 0.35
    v[bright] = np.rint(rng.uniform(1200, 4096, int(bright.sum())) / 16) * 16
    v = np.clip(v, 0, 4096)
    if n >= 2:
        v[0], v[-1] = 4096, 0                                   # voxels exactly at hi and at lo
    return v.astype(np.float32).reshape(shape)


def check_otsu(x, v):
    want_mask, st = V.foreground_mask_np(v, return_stats=True)
    mask, stats, counts = V.otsu_mask(x)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == v.shape and stats.dtype == torch.float64 and counts.dtype == torch.int64
    stats, counts = stats.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(counts, st["counts"]), np.flatnonzero(counts != st["counts"])[:8]
    assert stats[0] == float(st["lo"]) and stats[1] == float(st["hi"]) and stats[2] == st["t"] and stats[3] == st["count"], (stats, st)
    got = mask.cpu().numpy()
    assert np.array_equal(got, want_mask), int((got != want_mask).sum())
    return st


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", OTSU_SHAPES, ids=str)
def test_otsu_mask_is_bit_equal_to_the_specification(shape, kind):
    v = otsu_volume(shape, kind, seed=sum(shape))
    st = check_otsu(torch.from_numpy(v).cuda(), v)
    if kind == "constant" or v.size == 1:
        assert st["t"] == -1 and st["count"] == v.size
    else:
        assert 0 <= st["t"] < 255 and 0 < st["count"] < v.size and st["counts"][0] > 0 and st["counts"][255] > 0


def test_otsu_mask_on_an_unaligned_volume_and_with_guard_cells():
    """The volume 4 bytes off a 16-byte boundary (the scalar form of every pass); the mask inside a larger buffer of 7s."""
    shape = (70, 37, 45)
    v = otsu_volume(shape, "int12", seed=5)
    n = v.size
    buf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    buf[1:1 + n] = torch.from_numpy(v).cuda().reshape(-1)
    x = buf[1:1 + n].view(shape)
    assert x.data_ptr() % 16 == 4
    check_otsu(x, v)
    lib, st = L.load(), L.stream_ptr()
    ws = torch.empty(int(lib.mrisr_f32_volume_otsu_workspace_bytes()) // 8, dtype=torch.int64, device="cuda")
    stats = torch.empty(4, dtype=torch.float64, device="cuda")
    y = torch.from_numpy(v).cuda()
    want = V.foreground_mask_np(v)
    for margin in (64, 61):                                     # the mask on and off a 4-byte boundary
        guard = torch.full((n + 2 * margin,), 7, dtype=torch.uint8, device="cuda")
        assert lib.mrisr_f32_volume_otsu_mask(y.data_ptr(), *shape, guard.data_ptr() + margin, stats.data_ptr(), ws.data_ptr(), st) == 0
        g = guard.cpu().numpy()
        assert (g[:margin] == 7).all() and (g[margin + n:] == 7).all()
        assert np.array_equal(g[margin:margin + n].reshape(shape), want)
    # an extent outside 1..32767 is refused before any launch: MRISR_E_SHAPE, the buffers untouched
    before = guard.clone()
    for bad in ((0, 37, 45), (70, 32768, 45), (70, 37, -1)):
        assert lib.mrisr_f32_volume_otsu_mask(y.data_ptr(), *bad, guard.data_ptr() + margin, stats.data_ptr(), ws.data_ptr(), st) == -2
        assert lib.mrisr_u8_volume_morph(guard.data_ptr(), *bad, 1, L.MORPH_DILATE, before.data_ptr(), ws.data_ptr(), st) == -2
    assert torch.equal(guard, before)


def test_foreground_mask_returns_the_closed_mask_and_refuses_bad_arguments():
    v = otsu_volume((12, 11, 10), "signed", seed=2)
    x = torch.from_numpy(v).cuda()
    for r in (0, 2):
        mask, stats = V.foreground_mask(x, close_radius=r)
        want, st = V.foreground_mask_np(v, r, return_stats=True)
        assert mask.is_cuda and mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), want)
        assert stats.is_cuda and stats.cpu().tolist() == [float(st["lo"]), float(st["hi"]), float(st["t"]), float(st["count"])]
    with pytest.raises(ValueError):
        V.foreground_mask(x, close_radius=5)
    with pytest.raises(ValueError):
        V.foreground_mask(x.double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.foreground_mask(x.cpu())


# ---------------------------------------------------------------- closing

# (1, 3, 40): extents below the radius; (70, 37, 45): more than one run of 16 along x and y, Z no multiple of 4 (the bytewise form);
# (5, 6, 300): two z tiles of 256 in the word form, the halo crosses the tile edge; (3, 5, 261): the same in the bytewise form
MORPH_SHAPES = [(1, 3, 40), (12, 11, 10), (70, 37, 45), (5, 6, 300), (3, 5, 261)]
RADII = [0, 1, 2, 4]


def morph_guarded(m, radius, op, margin=64):
    """The C entry point with dst and tmp inside larger buffers of 7s; -> dst as numpy, after checking dst's guard cells."""
    lib, st = L.load(), L.stream_ptr()
    n = m.size
    src = torch.from_numpy(m).cuda()
    dst = torch.full((n + 2 * margin,), 7, dtype=torch.uint8, device="cuda")
    tmp = torch.full((n + 2 * margin,), 7, dtype=torch.uint8, device="cuda")
    assert lib.mrisr_u8_volume_morph(src.data_ptr(), *m.shape, radius, op, dst.data_ptr() + margin, tmp.data_ptr() + margin, st) == 0
    d, t = dst.cpu().numpy(), tmp.cpu().numpy()
    assert (d[:margin] == 7).all() and (d[margin + n:] == 7).all() and (t[:margin] == 7).all() and (t[margin + n:] == 7).all()
    assert np.array_equal(src.cpu().numpy(), m)                 # the source is left alone
    return d[margin:margin + n].reshape(m.shape)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", MORPH_SHAPES, ids=str)
def test_dilation_erosion_and_closing_are_bit_equal_to_the_specification(shape, radius):
    rng = np.random.default_rng(sum(shape) + radius)
    m = (rng.uniform(size=shape) < 0.3).astype(np.uint8)
    grown = morph_guarded(m, radius, L.MORPH_DILATE)
    assert np.array_equal(grown, V.dilate_np(m, radius))
    assert np.array_equal(morph_guarded(m, radius, L.MORPH_ERODE), V.erode_np(m, radius))
    closed = morph_guarded(grown, radius, L.MORPH_ERODE)
    want = V.erode_np(V.dilate_np(m, radius), radius)
    assert np.array_equal(closed, want)
    assert np.array_equal(V.binary_close(torch.from_numpy(m).cuda(), radius).cpu().numpy(), want)
    if radius == 0:
        assert np.array_equal(closed, m)


def test_morphology_of_grey_bytes_off_a_word_boundary_and_of_an_otsu_mask():
    """Any uint8 value (bytewise max / min, not just 0 / 1); dst and tmp 1 byte off a 4-byte boundary with Z a multiple of 4."""
    rng = np.random.default_rng(11)
    g = rng.integers(0, 256, (9, 7, 40), dtype=np.uint8)
    for margin in (64, 61):
        assert np.array_equal(morph_guarded(g, 2, L.MORPH_DILATE, margin), V.dilate_np(g, 2))
        assert np.array_equal(morph_guarded(g, 3, L.MORPH_ERODE, margin), V.erode_np(g, 3))
    v = otsu_volume((70, 37, 45), "signed", seed=4)
    x = torch.from_numpy(v).cuda()
    mask, _, _ = V.otsu_mask(x)
    for r in (1, 4):
        want = V.foreground_mask_np(v, r)
        assert np.array_equal(V.binary_close(mask, r).cpu().numpy(), want)
        assert np.array_equal(V.binary_erode(V.binary_dilate(mask, r), r).cpu().numpy(), want)
    with pytest.raises(ValueError):
        V.binary_close(mask, 5)
    with pytest.raises(ValueError):
        V.binary_dilate(mask.float(), 1)


# ---------------------------------------------------------------- masked metrics

METRIC_SHAPES = [(1, 1, 1), (5, 3, 40), (12, 11, 10), (70, 37, 45)]      # those of tests/test_gpu_volume_eval.py
WINDOWS = [3, 11, 15]
MASK_KINDS = ["ones", "half", "otsu", "voxel", "empty"]


def make_pair(shape, seed):
    """Ground truth plus a smooth error plus noise, in [0, 1] (the kind of pair tests/test_gpu_volume_eval.py uses)."""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, s) if s > 1 else np.zeros(1) for s in shape), indexing="ij")
    truth = 0.5 + 0.35 * np.exp(-1.5 * (x * x + y * y)) * np.cos(4 * x + 2 * z) + rng.normal(0, 0.05, shape)
    pred = truth + 0.03 * np.sin(3 * y + 2 * z + x) + rng.normal(0, 0.02, shape)
    return np.clip(pred, 0, 1).astype(np.float32), np.clip(truth, 0, 1).astype(np.float32)


def make_mask(kind, shape, ref):
    if kind == "ones":
        return np.ones(shape, dtype=np.uint8)
    if kind == "empty":
        return np.zeros(shape, dtype=np.uint8)
    if kind == "voxel":
        m = np.zeros(shape, dtype=np.uint8)
        m[tuple(s // 2 for s in shape)] = 1
        return m
    if kind == "otsu":
        return V.foreground_mask_np(ref, 1)                     # the closed Otsu mask of the reference, from the specification
    x, y, z = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")      # an oblique half-space: cuts through every tile and chunk
    return (3 * x + 2 * y + z < (3 * shape[0] + 2 * shape[1] + shape[2]) // 2).astype(np.uint8) * 255


def ssim_map_float32_torch(a, b, val_range, window_size, sigma=1.5):
    """The SSIM map restated in float32 with torch's separable conv3d on the CPU."""
    g = torch.from_numpy(V.gaussian_window_np(window_size, sigma)).float()
    h = window_size // 2

    def blur(x):
        x = x[None, None]
        x = F.conv3d(x, g.view(1, 1, -1, 1, 1), padding=(h, 0, 0))
        x = F.conv3d(x, g.view(1, 1, 1, -1, 1), padding=(0, h, 0))
        return F.conv3d(x, g.view(1, 1, 1, 1, -1), padding=(0, 0, h))[0, 0]

    a, b = torch.from_numpy(a), torch.from_numpy(b)
    c1, c2 = np.float32((0.01 * val_range) ** 2), np.float32((0.03 * val_range) ** 2)
    mu1, mu2 = blur(a), blur(b)
    s11, s22, s12 = blur(a * a) - mu1 * mu1, blur(b * b) - mu2 * mu2, blur(a * b) - mu1 * mu2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))).double().numpy()


@pytest.fixture(scope="module")
def metric_cases():
    """{(shape, window): (pred, ref, whole-volume specification, {mask kind: (mask, specification, ssim bar, dev)})}: computed once."""
    cases = {}
    for shape in METRIC_SHAPES:
        a, b = make_pair(shape, seed=sum(shape))
        masks = {kind: make_mask(kind, shape, b) for kind in MASK_KINDS}
        for win in WINDOWS:
            map32 = ssim_map_float32_torch(a, b, 1.0, win)
            whole = V.volume_metrics_np(a, b, 1.0, win)
            per = {}
            for kind, m in masks.items():
                want = V.volume_metrics_np(a, b, 1.0, win, mask=m)
                sel = m != 0
                dev = abs(float(map32[sel].mean()) - want[0]) if sel.any() else 0.0
                per[kind] = (m, want, max(5e-6, 4 * dev), dev)
            dev0 = abs(float(map32.mean()) - whole[0])
            cases[shape, win] = (a, b, (whole, max(5e-6, 4 * dev0), dev0), per)
    return cases


def check_row(row, want, bar, what):
    ssim, mse, rmse, mae, psnr = row
    print(f"{what}: ssim off {abs(ssim - want[0]):.2e} (bar {bar:.1e}), mse rel {abs(mse - want[1]) / want[1]:.2e}, "
          f"rmse rel {abs(rmse - want[2]) / want[2]:.2e}, mae rel {abs(mae - want[3]) / want[3]:.2e}, psnr off {abs(psnr - want[4]):.2e} dB")
    assert abs(mse - want[1]) <= 1e-6 * want[1] and abs(rmse - want[2]) <= 1e-6 * want[2] and abs(mae - want[3]) <= 1e-6 * want[3], what
    assert abs(psnr - want[4]) <= 1e-5, what
    assert abs(ssim - want[0]) <= bar, what


@pytest.mark.parametrize("window_size", WINDOWS)
@pytest.mark.parametrize("shape", METRIC_SHAPES, ids=str)
def test_masked_metrics_against_the_float64_specification(metric_cases, shape, window_size):
    a, b, (whole, bar0, _), per = metric_cases[shape, window_size]
    x, y = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    plain = V.volume_metrics(x, y, 1.0, window_size)
    assert tuple(plain.shape) == (5,)                           # without a mask: what it always returned
    for kind in MASK_KINDS:
        m, want, bar, dev = per[kind]
        got = V.volume_metrics(x, y, 1.0, window_size, mask=torch.from_numpy(m).cuda())
        assert got.dtype == torch.float64 and tuple(got.shape) == (2, 5) and got.is_cuda and tuple(got.packed.shape) == (11,)
        assert float(got.mask_count) == float((m != 0).sum()) == float(got.packed[10])      # exact
        assert torch.allclose(got[0], plain, rtol=1e-12, atol=0), kind      # row 0 is the unmasked call (the order of the double atomics is free)
        rows = got.cpu().numpy()
        what = f"{shape} w{window_size} {kind} ({int((m != 0).sum())} voxels, float32 torch off {dev:.2e})"
        check_row(rows[0], whole, bar0, what + " whole")
        if kind == "empty":
            assert np.isnan(rows[1]).all() and np.isnan(want).all() and np.isfinite(rows[0]).all()
            continue
        check_row(rows[1], want, bar, what)
        if kind == "ones":
            assert np.allclose(rows[1], rows[0], rtol=1e-12, atol=0)
    bool_mask = torch.from_numpy(per["half"][0] != 0).cuda()    # a bool mask is the same mask
    again = V.volume_metrics(x, y, 1.0, window_size, mask=bool_mask)
    assert torch.allclose(again, V.volume_metrics(x, y, 1.0, window_size, mask=torch.from_numpy(per["half"][0]).cuda()), rtol=1e-12, atol=0)


def test_masked_metrics_read_nothing_outside_their_buffers_and_accumulate(metric_cases):
    """a, b in the middle of buffers of NaN and the mask in the middle of a buffer of 255s: a voxel read out of bounds would make a
    sum NaN, a mask byte read out of bounds would change the count."""
    shape = (70, 37, 45)
    a, b, _, per = metric_cases[shape, 15]
    m, want, bar, _ = per["otsu"]
    n, margin = a.size, 70 * 45 * 2 + 64
    bufs = []
    for v in (a, b):
        buf = torch.full((n + 2 * margin,), float("nan"), dtype=torch.float32, device="cuda")
        buf[margin:margin + n] = torch.from_numpy(v).cuda().reshape(-1)
        bufs.append(buf)
    mbuf = torch.full((n + 2 * margin,), 255, dtype=torch.uint8, device="cuda")
    mbuf[margin:margin + n] = torch.from_numpy(m).cuda().reshape(-1)
    x, y = (buf[margin:margin + n].view(shape) for buf in bufs)
    mm = mbuf[margin:margin + n].view(shape)
    got = V.volume_metrics(x, y, 1.0, 15, mask=mm)
    plain = V.volume_metrics(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 1.0, 15, mask=torch.from_numpy(m).cuda())
    assert float(got.mask_count) == float((m != 0).sum())
    assert torch.isfinite(got).all() and torch.allclose(got, plain, rtol=1e-12, atol=0)
    assert abs(float(got[1, 0]) - want[0]) <= bar
    # sums7 accumulate (the caller zeroes them), and the refusals launch nothing
    lib, st = L.load(), L.stream_ptr()
    sums = torch.zeros(7, dtype=torch.float64, device="cuda")
    args = (x.data_ptr(), y.data_ptr(), mm.data_ptr(), *shape, 1.0, 1.5, 11, sums.data_ptr(), st)
    assert lib.mrisr_f32_volume_metrics_masked(*args) == 0
    once = sums.cpu().numpy().copy()
    assert lib.mrisr_f32_volume_metrics_masked(*args) == 0
    assert np.allclose(sums.cpu().numpy(), 2 * once, rtol=1e-12, atol=0) and once[6] == (m != 0).sum()
    assert lib.mrisr_f32_volume_metrics_masked(x.data_ptr(), y.data_ptr(), mm.data_ptr(), *shape, 1.0, 1.5, 4, sums.data_ptr(), st) == -1
    assert lib.mrisr_f32_volume_metrics_masked(x.data_ptr(), y.data_ptr(), mm.data_ptr(), 0, 37, 45, 1.0, 1.5, 11, sums.data_ptr(), st) == -2
    with pytest.raises(ValueError):
        V.volume_metrics(x, y, 1.0, mask=mm[:10])
    with pytest.raises(ValueError):
        V.volume_metrics(x, y, 1.0, mask=mm.float())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.volume_metrics(x, y, 1.0, mask=mm.cpu())


# ---------------------------------------------------------------- wiring

def synthetic_volume(shape, seed=0):
    """Intensities 0..3000: a bright smooth structure in a dark noisy background (as tests/test_gpu_volume_eval.py)."""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, s) for s in shape), indexing="ij")
    v = 3000.0 * np.exp(-2.0 * (x * x + y * y)) * (0.6 + 0.4 * np.cos(3 * x + z)) + rng.normal(0, 40, shape)
    v = np.clip(np.rint(v), 0, 3000)
    v[:3] = 0
    return v.astype(np.float32)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(1234)
    return UNetSuperRes(1, 1, base_filters=16).cuda().eval()


def test_evaluate_volume_with_a_mask(model):
    full = synthetic_volume((33, 48, 16), seed=5)               # the odd extent is cropped: the mask follows the reference
    ref = torch.from_numpy(full).cuda()
    kw = dict(batch_size=2, use_graph=False)
    plain = V.evaluate_volume(model, ref, **kw)
    res = V.evaluate_volume(model, ref, mask="otsu", mask_close=1, **kw)
    assert list(res) == list(plain) == ["unet", "linear", "cubic"]
    cropped = np.ascontiguousarray(full[:32])
    want_mask, st = V.foreground_mask_np(cropped, 1, return_stats=True)
    assert np.array_equal(res.mask.cpu().numpy(), want_mask) and 0 < want_mask.sum() < want_mask.size
    assert res.mask_stats.cpu().tolist() == [float(st["lo"]), float(st["hi"]), float(st["t"]), float(st["count"])]
    for k, v in res.items():
        assert tuple(v.shape) == (2, 5) and v.dtype == torch.float64 and v.is_cuda
        assert torch.allclose(v[0], plain[k], rtol=1e-12, atol=0), k
        assert float(v.mask_count) == float(want_mask.sum())
        assert torch.isfinite(v).all() and not torch.allclose(v[1], v[0], rtol=1e-3, atol=0)
    # row 1 is volume_metrics of the same method inside that mask
    lr = V.downsample2(torch.from_numpy(cropped).cuda(), (0, 1))
    rng = float(cropped.max() - cropped.min())
    direct = V.volume_metrics(V.upscale2(lr, "linear", (0, 1)), torch.from_numpy(cropped).cuda(), rng, mask=torch.from_numpy(want_mask).cuda())
    assert torch.allclose(res["linear"], direct, rtol=1e-12, atol=0)
    # the same mask passed in (of the uncropped shape: it gets the reference's crop), uint8 and bool
    given = np.concatenate([want_mask, np.ones((1, 48, 16), dtype=np.uint8)], axis=0)
    for m in (torch.from_numpy(given).cuda(), torch.from_numpy(given != 0).cuda()):
        same = V.evaluate_volume(model, ref, mask=m, **kw)
        assert same.mask_stats is None and all(torch.allclose(same[k], res[k], rtol=1e-12, atol=0) for k in res)
    # closing a given mask: otsu + close 1 is close 1 of the plain otsu mask
    closed = V.evaluate_volume(model, ref, mask=torch.from_numpy(np.concatenate([V.foreground_mask_np(cropped), given[32:]])).cuda(),
                               mask_close=1, **kw)
    assert all(torch.allclose(closed[k], res[k], rtol=1e-12, atol=0) for k in res)
    with pytest.raises(ValueError, match="reference's shape"):
        V.evaluate_volume(model, ref, mask=torch.from_numpy(want_mask).cuda(), **kw)      # the cropped shape is not the reference's
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.evaluate_volume(model, ref, mask=torch.from_numpy(given), **kw)
    with pytest.raises(ValueError, match="mask_close"):
        V.evaluate_volume(model, ref, mask_close=1, **kw)


def test_command_line_with_a_mask(model, tmp_path, capsys):
    ckdir = tmp_path / "ck"
    ckdir.mkdir()
    torch.save({"model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, ckdir / "best_model_unet.pth")
    vol = synthetic_volume((32, 48, 16), seed=5)
    vol4 = np.stack([vol, vol[::-1].copy()], axis=3)
    one, two = tmp_path / "scan.nii.gz", tmp_path / "scan4d.nii"
    write_nifti(str(one), vol, NiftiHeader.new(vol.shape, (1.0, 1.0, 1.0)), ())
    write_nifti(str(two), vol4, NiftiHeader.new(vol4.shape, (1.0, 1.0, 1.0, 2.0)), ())
    common = ["--checkpoint_dir", str(ckdir), "--base_filters", "16", "--batch_size", "2", "--no_graph"]
    methods = ["unet", "linear", "cubic"]

    def rows_of(path):
        with open(path, newline="") as f:
            return list(csv.DictReader(f))

    out = tmp_path / "otsu.csv"
    capsys.readouterr()
    assert cli.main(cli.parse_args(["--reference", str(one), str(two), "--mask", "otsu", "--mask_close", "1", "--output_csv", str(out)] + common)) == 0
    text = capsys.readouterr().out
    want_mask, st = V.foreground_mask_np(vol, 1, return_stats=True)
    count = int(want_mask.sum())
    thr = V.otsu_threshold_value(st["lo"], st["hi"], st["t"])
    title = f"foreground: {count} voxels, {100.0 * count / vol.size:.1f} % of the volume, Otsu threshold {thr:.6g}"
    assert text.count("foreground: ") == 3 and text.count(title) == 3 and "foreground, mean over 3 scan(s)" in text      # t = 1 is the mirrored scan
    assert text.index("scan.nii.gz\n") < text.index(title) < text.index("scan4d.nii[t=0]\n") and text.count("mean over 3 scan(s)") == 2
    rows = rows_of(out)
    assert list(rows[0]) == ["scan", "region", "method", "ssim", "psnr", "mse", "rmse", "mae"]
    scans = ["scan.nii.gz", "scan4d.nii[t=0]", "scan4d.nii[t=1]"]
    order = [(s, r, m) for s in scans for r in ("whole", "foreground") for m in methods]
    order += [("mean", r, m) for r in ("whole", "foreground") for m in methods]
    assert [(r["scan"], r["region"], r["method"]) for r in rows] == order
    x = torch.from_numpy(vol).cuda()
    want = V.evaluate_volume(model, x, batch_size=2, use_graph=False, mask="otsu", mask_close=1)
    for r in rows[:6]:
        region = ("whole", "foreground").index(r["region"])
        assert [float(r[k]) for k in METRIC_COLUMNS] == pytest.approx(want[r["method"]][region].cpu().tolist(), rel=1e-12)
    assert float(rows[18 + 4]["ssim"]) == pytest.approx(np.mean([float(rows[i]["ssim"]) for i in (4, 10, 16)]), rel=1e-12)

    # without --mask: the old columns and half the rows, equal to the whole-volume rows above
    out0 = tmp_path / "plain.csv"
    assert cli.main(cli.parse_args(["--reference", str(one), str(two), "--output_csv", str(out0)] + common)) == 0
    text0 = capsys.readouterr().out
    rows0 = rows_of(out0)
    assert list(rows0[0]) == ["scan", "method", "ssim", "psnr", "mse", "rmse", "mae"] and "foreground" not in text0
    assert len(rows) == 2 * len(rows0)
    whole = [r for r in rows if r["region"] == "whole"]
    for r0, r1 in zip(rows0, whole):
        assert (r0["scan"], r0["method"]) == (r1["scan"], r1["method"])
        assert [float(r0[k]) for k in METRIC_COLUMNS] == pytest.approx([float(r1[k]) for k in METRIC_COLUMNS], rel=1e-12)

    # --mask PATH with the Otsu mask in the file: identical numbers (int16 voxels, a 3-D mask for the 3-D scan)
    mpath = tmp_path / "mask.nii.gz"
    write_nifti(str(mpath), (want_mask * 3).astype(np.int16), NiftiHeader.new(vol.shape, (1.0, 1.0, 1.0)), ())
    out1 = tmp_path / "file.csv"
    assert cli.main(cli.parse_args(["--reference", str(one), "--mask", str(mpath), "--output_csv", str(out1)] + common)) == 0
    text1 = capsys.readouterr().out
    assert f"foreground: {count} voxels, {100.0 * count / vol.size:.1f} % of the volume\n" in text1 and "Otsu" not in text1
    rows1 = rows_of(out1)
    assert [(r["scan"], r["region"], r["method"]) for r in rows1[:6]] == order[:6] and len(rows1) == 12
    for r1, r in zip(rows1[:6], rows[:6]):
        assert [float(r1[k]) for k in METRIC_COLUMNS] == pytest.approx([float(r[k]) for k in METRIC_COLUMNS], rel=1e-12)
    # a 3-D mask serves every timepoint of the 4-D scan; a 4-D mask needs the same number of timepoints
    assert cli.main(cli.parse_args(["--reference", str(two), "--mask", str(mpath)] + common)) == 0
    m4 = tmp_path / "mask4d.nii"
    m3t = np.stack([want_mask] * 3, axis=3).astype(np.int16)
    write_nifti(str(m4), m3t, NiftiHeader.new(m3t.shape, (1.0, 1.0, 1.0, 2.0)), ())
    assert cli.main(cli.parse_args(["--reference", str(two), "--mask", str(m4)] + common)) == 1
    # errors through the script's error path
    assert cli.main(cli.parse_args(["--reference", str(one), "--mask_close", "1"] + common)) == 1
    assert cli.main(cli.parse_args(["--reference", str(one), "--mask", "otsu", "--mask_close", "5"] + common)) == 1
    small = tmp_path / "small.nii"
    write_nifti(str(small), want_mask[:16].astype(np.int16), NiftiHeader.new((16, 48, 16), (1.0, 1.0, 1.0)), ())
    assert cli.main(cli.parse_args(["--reference", str(one), "--mask", str(small)] + common)) == 1
    assert cli.main(cli.parse_args(["--reference", str(one), "--mask", str(tmp_path / "missing.nii")] + common)) == 1
