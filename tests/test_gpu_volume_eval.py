"""Volume evaluation (GPU): csrc/volume_eval.hip against its numpy specifications bit for bit, csrc/volume_metrics.hip against
the float64 specification volume_metrics_np, evaluate_volume's wiring and scripts/evaluate_volume.py.

Bars.  down2 / up2 restate their specifications operation by operation: bit-equal.  mse and mae: 1e-6 relative, PSNR 1e-5 dB -
the bars of tests/test_gpu_eval.py by the same argument (the kernel forms a - b, |a - b| and (a - b)^2 exactly in double; only the
order of the double sums differs).  SSIM: the project's 5e-6, unless the same metric restated with float32 torch on the CPU is
itself further than 5e-6 / 4 from the float64 specification on the test's inputs - then four times that deviation.  Measured on
these inputs: the float32 restatement deviates by at most 1.4e-7 (the mean over the map averages the float32 cancellation noise
of sigma = E[x^2] - mu^2 out), so the bar is 5e-6; the kernel is at most 1.2e-7 off on an MI355X."""
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
from mri_superresolution_amd.volume import enhance_volume, enhance_volume_isotropic   # noqa: E402
from scripts import evaluate_volume as cli                                   # noqa: E402

E_ARG, E_SHAPE = -1, -2      # MRISR_E_ARG, MRISR_E_SHAPE (include/mrisr.h)
MASKS = range(1, 8)


def axes_of(mask):
    return tuple(a for a in (0, 1, 2) if mask >> a & 1)


def values(shape, seed):
    """+-3000; every other voxel along z at an integer step."""
    v = np.random.default_rng(seed).uniform(-3000.0, 3000.0, shape)
    v[..., ::2] = np.rint(v[..., ::2])
    return v.astype(np.float32)


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---------------------------------------------------------------- bit-exact kernels

# (34, 18, 130): more than one 64-wide block along z and more than one 4-row block along y, with remainders
@pytest.mark.parametrize("shape", [(2, 2, 2), (2, 6, 10), (4, 2, 66), (34, 18, 130)], ids=str)
def test_downsample2_is_bit_equal_to_the_specification(shape):
    v = values(shape, seed=sum(shape))
    x = torch.from_numpy(v).cuda()
    for mask in MASKS:
        got = V.downsample2(x, axes_of(mask)).cpu().numpy()
        assert same_bits(got, V.downsample2_np(v, axes_of(mask))), (shape, mask)


def test_downsample2_odd_unset_axis_and_refusals():
    v = values((4, 6, 5), seed=9)
    x = torch.from_numpy(v).cuda()
    assert same_bits(V.downsample2(x, (0, 1)).cpu().numpy(), V.downsample2_np(v, (0, 1)))
    lib, st = L.load(), L.stream_ptr()
    out = torch.full((4, 6, 5), 9.0, dtype=torch.float32, device="cuda")
    assert lib.mrisr_f32_volume_down2(x.data_ptr(), 4, 6, 5, 4, out.data_ptr(), st) == E_SHAPE      # odd set axis
    assert lib.mrisr_f32_volume_down2(x.data_ptr(), 4, 6, 5, 7, out.data_ptr(), st) == E_SHAPE
    assert lib.mrisr_f32_volume_down2(x.data_ptr(), 4, 6, 5, 0, out.data_ptr(), st) == E_ARG
    assert lib.mrisr_f32_volume_down2(x.data_ptr(), 4, 6, 5, 8, out.data_ptr(), st) == E_ARG
    assert lib.mrisr_f32_volume_down2(x.data_ptr(), 0, 6, 5, 2, out.data_ptr(), st) == E_SHAPE
    assert lib.mrisr_f32_volume_up2(x.data_ptr(), 4, 6, 5, 0, L.RESAMPLE_LINEAR, out.data_ptr(), st) == E_ARG
    assert lib.mrisr_f32_volume_up2(x.data_ptr(), 4, 6, 5, 8, L.RESAMPLE_CUBIC, out.data_ptr(), st) == E_ARG
    assert lib.mrisr_f32_volume_up2(x.data_ptr(), 4, 6, 5, 1, L.RESAMPLE_AREA, out.data_ptr(), st) == E_ARG
    assert lib.mrisr_f32_volume_up2(x.data_ptr(), 4, 6, 32768, 1, L.RESAMPLE_CUBIC, out.data_ptr(), st) == E_SHAPE
    torch.cuda.synchronize()
    assert (out == 9.0).all()                                    # nothing was launched
    with pytest.raises(ValueError):
        V.downsample2(x, (2,))


# extents 1, 2 and 3: every clamped cubic tap (i - 2, i + 2) fires on both ends; (33, 17, 65) crosses the 64 x 4 block in z and y
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 5), (2, 1, 7), (3, 4, 2), (33, 17, 65)], ids=str)
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_upscale2_is_bit_equal_to_the_specification(method, shape):
    v = values(shape, seed=sum(shape) + 1)
    x = torch.from_numpy(v).cuda()
    for mask in MASKS:
        got = V.upscale2(x, method, axes_of(mask)).cpu().numpy()
        want = V.upscale2_np(v, method, axes_of(mask))
        assert same_bits(got, want), (method, shape, mask, int((got != want).sum()))


def off_boundary(v, k):
    """The float32 volume v on the device, its base k floats past a 16-byte boundary."""
    buf = torch.zeros(v.size + k, dtype=torch.float32, device="cuda")
    buf[k:] = torch.from_numpy(v).cuda().reshape(-1)
    x = buf[k:].view(v.shape)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4 * k
    return x


def test_down2_up2_and_metrics_off_a_16_byte_boundary():
    """Volumes of at most 5 x 7 x 9 voxels (315: no multiple of 4; down2 needs even extents on its set axes) at a base 4 bytes past
    a 16-byte boundary, 8 bytes where pairs along z are read as one load."""
    v = values((5, 7, 9), seed=21)
    for method in ("linear", "cubic"):
        for mask in MASKS:
            got = V.upscale2(off_boundary(v, 1), method, axes_of(mask)).cpu().numpy()
            assert same_bits(got, V.upscale2_np(v, method, axes_of(mask))), (method, mask)
    for shape, mask in (((4, 6, 9), 3), ((4, 7, 9), 1), ((5, 6, 9), 2), ((5, 7, 6), 4), ((4, 6, 6), 7)):
        v = values(shape, seed=sum(shape))
        got = V.downsample2(off_boundary(v, 2 if mask & 4 else 1), axes_of(mask)).cpu().numpy()
        assert same_bits(got, V.downsample2_np(v, axes_of(mask))), (shape, mask)
    a, b = make_pair((5, 7, 9), seed=21)
    want = V.volume_metrics_np(a, b, 1.0, 3)
    dev = abs(ssim_float32_torch(a, b, 1.0, 3) - want[0])
    got = V.volume_metrics(off_boundary(a, 1), off_boundary(b, 1), 1.0, 3).cpu().numpy()
    plain = V.volume_metrics(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 1.0, 3).cpu().numpy()
    assert np.allclose(got, plain, rtol=1e-12, atol=0)          # the order of the double atomics is free
    assert abs(got[0] - want[0]) <= (4 * dev if dev > 5e-6 / 4 else 5e-6)        # the bar of metric_cases
    assert abs(got[1] - want[1]) <= 1e-6 * want[1] and abs(got[3] - want[3]) <= 1e-6 * want[3]


# ---------------------------------------------------------------- metrics kernel

# the kernel's tile is 16 (y) x 32 (z) with x chunks of at least 32 planes: (70, 37, 45) is 2 x-chunks of 35, 3 y-tiles (16, 16, 5)
# and 2 z-tiles (32, 13) - a remainder in every direction, and halo planes of a neighbouring chunk on both sides
METRIC_SHAPES = [(1, 1, 1), (5, 3, 40), (12, 11, 10), (70, 37, 45)]
WINDOWS = [3, 11, 15]


def make_pair(shape, seed):
    """Ground truth plus a smooth error plus noise, in [0, 1]."""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, s) if s > 1 else np.zeros(1) for s in shape), indexing="ij")
    truth = 0.5 + 0.35 * np.exp(-1.5 * (x * x + y * y)) * np.cos(4 * x + 2 * z) + rng.normal(0, 0.05, shape)
    pred = truth + 0.03 * np.sin(3 * y + 2 * z + x) + rng.normal(0, 0.02, shape)
    return np.clip(pred, 0, 1).astype(np.float32), np.clip(truth, 0, 1).astype(np.float32)


def ssim_float32_torch(a, b, val_range, window_size, sigma=1.5):
    """The metric restated in float32 with torch's separable conv3d on the CPU; the mean of the float32 map taken in float64."""
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
    m = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))
    return float(m.double().mean())


@pytest.fixture(scope="module")
def metric_cases():
    """{(shape, window): (pred, ref, specification, ssim bar)}: computed once, read by the tests below."""
    cases = {}
    for shape in METRIC_SHAPES:
        a, b = make_pair(shape, seed=sum(shape))
        for win in WINDOWS:
            want = V.volume_metrics_np(a, b, 1.0, win)
            dev = abs(ssim_float32_torch(a, b, 1.0, win) - want[0])
            cases[shape, win] = (a, b, want, 4 * dev if dev > 5e-6 / 4 else 5e-6, dev)
    return cases


@pytest.mark.parametrize("window_size", WINDOWS)
@pytest.mark.parametrize("shape", METRIC_SHAPES, ids=str)
def test_volume_metrics_against_the_float64_specification(metric_cases, shape, window_size):
    a, b, want, bar, dev = metric_cases[shape, window_size]
    got = V.volume_metrics(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 1.0, window_size)
    assert got.dtype == torch.float64 and tuple(got.shape) == (5,) and got.is_cuda
    got = got.cpu().numpy()
    ssim, mse, rmse, mae, psnr = got
    print(f"{shape} w{window_size}: ssim {ssim:.9f} (spec {want[0]:.9f}, off {abs(ssim - want[0]):.2e}, float32 torch off {dev:.2e}, "
          f"bar {bar:.1e}), mse rel {abs(mse - want[1]) / want[1]:.2e}, mae rel {abs(mae - want[3]) / want[3]:.2e}, "
          f"psnr off {abs(psnr - want[4]):.2e} dB")
    assert abs(mse - want[1]) <= 1e-6 * want[1] and abs(mae - want[3]) <= 1e-6 * want[3]
    assert abs(rmse - want[2]) <= 1e-6 * want[2]
    assert abs(psnr - want[4]) <= 1e-5
    assert abs(ssim - want[0]) <= bar


def test_volume_metrics_scale_accumulation_and_identity(metric_cases):
    a, b, want, bar, _ = metric_cases[(70, 37, 45), 11]
    x, y = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    base = V.volume_metrics(x, y, 1.0).cpu().numpy()
    scaled = V.volume_metrics(x * 4096.0, y * 4096.0, 4096.0).cpu().numpy()      # a power of two: exact in float32
    assert abs(scaled[0] - want[0]) <= bar and abs(scaled[0] - base[0]) <= bar
    assert abs(scaled[4] - want[4]) <= 1e-4 and abs(scaled[4] - base[4]) <= 1e-4
    assert abs(scaled[1] - 4096.0 ** 2 * want[1]) <= 1e-6 * 4096.0 ** 2 * want[1]
    # sums accumulate: the caller zeroes them
    lib, st = L.load(), L.stream_ptr()
    sums = torch.zeros(3, dtype=torch.float64, device="cuda")
    args = (x.data_ptr(), y.data_ptr(), *a.shape, 1.0, 1.5, 11, sums.data_ptr(), st)
    assert lib.mrisr_f32_volume_metrics(*args) == 0
    once = sums.cpu().numpy().copy()
    assert lib.mrisr_f32_volume_metrics(*args) == 0
    twice = sums.cpu().numpy()
    assert np.all(once > 0) and np.allclose(twice, 2 * once, rtol=1e-12, atol=0)
    assert abs(once[1] / a.size - want[0]) <= bar
    # identical volumes
    same = V.volume_metrics(x, x, 1.0).cpu().numpy()
    assert abs(same[0] - 1) <= 1e-6 and same[1] == 0 and same[3] == 0 and same[4] == 100.0
    # refusals
    assert lib.mrisr_f32_volume_metrics(x.data_ptr(), y.data_ptr(), *a.shape, 1.0, 1.5, 4, sums.data_ptr(), st) == E_ARG
    assert lib.mrisr_f32_volume_metrics(x.data_ptr(), y.data_ptr(), *a.shape, 1.0, 1.5, 17, sums.data_ptr(), st) == E_ARG
    assert lib.mrisr_f32_volume_metrics(x.data_ptr(), y.data_ptr(), 0, 37, 45, 1.0, 1.5, 11, sums.data_ptr(), st) == E_SHAPE
    with pytest.raises(NotImplementedError):
        V.volume_metrics(x, y, 1.0, window_size=4)
    with pytest.raises(ValueError):
        V.volume_metrics(x, y[:10], 1.0)
    with pytest.raises(ValueError):
        V.volume_metrics(x, y, 0.0)


@pytest.mark.parametrize("shape", [(12, 11, 10), (70, 37, 45)], ids=str)
def test_volume_metrics_reads_nothing_outside_the_volumes(metric_cases, shape):
    """a and b in the middle of larger buffers of NaN: one voxel read out of bounds would make a sum NaN."""
    a, b, want, bar, _ = metric_cases[shape, 15]
    n, margin = a.size, 70 * 45 * 2 + 64
    bufs = []
    for v in (a, b):
        buf = torch.full((n + 2 * margin,), float("nan"), dtype=torch.float32, device="cuda")
        buf[margin:margin + n] = torch.from_numpy(v).cuda().reshape(-1)
        bufs.append(buf)
    x, y = (buf[margin:margin + n].view(shape) for buf in bufs)
    assert x.is_contiguous() and x.data_ptr() == bufs[0].data_ptr() + 4 * margin
    got = V.volume_metrics(x, y, 1.0, 15).cpu().numpy()
    plain = V.volume_metrics(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 1.0, 15).cpu().numpy()
    assert np.isfinite(got).all() and np.allclose(got, plain, rtol=1e-12, atol=0)      # the order of the double atomics is free
    assert abs(got[0] - want[0]) <= bar


# ---------------------------------------------------------------- wiring

def synthetic_volume(shape, seed=0):
    """The generator of tests/test_gpu_isotropic.py without the constant slice: intensities 0..3000, smooth structure, noise."""
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


def rows_equal(a, b):
    """Equal up to the order in which the blocks' double partial sums reach the three accumulators (atomics): 1e-12 relative."""
    return torch.allclose(a, b, rtol=1e-12, atol=0)


def test_evaluate_volume_rows_are_the_metrics_of_their_methods(model):
    """Reference (48, 80, 64): its low-resolution volumes are the (24, 40, ..) shapes of tests/test_gpu_isotropic.py."""
    ref = torch.from_numpy(synthetic_volume((48, 80, 64))).cuda()
    rng = float((ref.max() - ref.min()).item())
    kw = dict(batch_size=8, use_graph=False)
    res = V.evaluate_volume(model, ref, **kw)
    assert list(res) == ["unet", "linear", "cubic"]
    lr = V.downsample2(ref, (0, 1))
    assert tuple(lr.shape) == (24, 40, 64)
    assert rows_equal(res["unet"], V.volume_metrics(enhance_volume(model, lr, axis=2, **kw), ref, rng))
    for method in ("linear", "cubic"):
        assert rows_equal(res[method], V.volume_metrics(V.upscale2(lr, method, (0, 1)), ref, rng))
    given = V.evaluate_volume(model, ref, lr=lr, val_range=rng, **kw)             # the same lr, passed in
    assert all(rows_equal(given[k], res[k]) for k in res)
    vals = {k: v.cpu().numpy() for k, v in res.items()}
    for k, v in vals.items():
        print(k, dict(zip(METRIC_COLUMNS, v.tolist())))
    # an SSIM term of two non-negative volumes lies in [-1, 1], and so does the mean; a random-weight network may land below 0,
    # the interpolation of a smooth volume may not
    assert all(np.isfinite(v).all() and -1 <= v[0] <= 1 and v[1] > 0 and abs(v[2] - np.sqrt(v[1])) <= 1e-9 * v[2] for v in vals.values())
    assert vals["linear"][0] > 0 and vals["cubic"][0] > 0

    iso = V.evaluate_volume(model, ref, isotropic=True, **kw)
    assert list(iso) == ["unet", "unet_axis2_linear", "linear", "cubic"]
    lr3 = V.downsample2(ref)
    assert tuple(lr3.shape) == (24, 40, 32)
    assert rows_equal(iso["unet"], V.volume_metrics(enhance_volume_isotropic(model, lr3, **kw), ref, rng))
    assert rows_equal(iso["unet_axis2_linear"], V.volume_metrics(enhance_volume_isotropic(model, lr3, planes=(2,), **kw), ref, rng))
    for method in ("linear", "cubic"):
        assert rows_equal(iso[method], V.volume_metrics(V.upscale2(lr3, method), ref, rng))
    assert not rows_equal(iso["unet"], iso["unet_axis2_linear"])
    other = V.evaluate_volume(model, ref, axis=0, **kw)
    assert rows_equal(other["linear"], V.volume_metrics(V.upscale2(V.downsample2(ref, (1, 2)), "linear", (1, 2)), ref, rng))


def test_evaluate_volume_crops_an_odd_reference_and_refuses_a_wrong_lr(model):
    full = synthetic_volume((17, 25, 6), seed=3)
    ref = torch.from_numpy(full).cuda()
    res = V.evaluate_volume(model, ref, batch_size=2, use_graph=False)
    cropped = torch.from_numpy(np.ascontiguousarray(full[:16, :24])).cuda()
    rng = float((cropped.max() - cropped.min()).item())
    lr = V.downsample2(cropped, (0, 1))
    for method in ("linear", "cubic"):
        assert rows_equal(res[method], V.volume_metrics(V.upscale2(lr, method, (0, 1)), cropped, rng))
    assert rows_equal(res["unet"], V.volume_metrics(enhance_volume(model, lr, batch_size=2, use_graph=False), cropped, rng))
    with pytest.raises(ValueError, match="exactly half"):
        V.evaluate_volume(model, cropped, lr=lr[:, :, :3])
    with pytest.raises(ValueError, match="exactly half"):
        V.evaluate_volume(model, ref, lr=lr)                                      # an odd reference has no half
    with pytest.raises(ValueError, match="exactly half"):
        V.evaluate_volume(model, cropped, lr=lr, isotropic=True)
    with pytest.raises(ValueError, match="range"):
        V.evaluate_volume(model, torch.full((4, 8, 8), 5.0, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.evaluate_volume(model, cropped, lr=lr.cpu())


def test_command_line(model, tmp_path):
    ckdir = tmp_path / "ck"
    ckdir.mkdir()
    torch.save({"model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, ckdir / "best_model_unet.pth")
    vol = synthetic_volume((32, 48, 16), seed=5)      # halved on every axis the slices are still 8 x 8 at least (three 2 x 2 pools)
    vol4 = np.stack([vol, vol[::-1].copy()], axis=3)
    one, two = tmp_path / "scan.nii.gz", tmp_path / "scan4d.nii"
    write_nifti(str(one), vol, NiftiHeader.new(vol.shape, (1.0, 1.0, 1.0)), ())
    write_nifti(str(two), vol4, NiftiHeader.new(vol4.shape, (1.0, 1.0, 1.0, 2.0)), ())
    common = ["--checkpoint_dir", str(ckdir), "--base_filters", "16", "--batch_size", "2", "--no_graph"]
    out = tmp_path / "out" / "scores.csv"
    assert cli.main(cli.parse_args(["--reference", str(one), str(two), "--isotropic", "--output_csv", str(out)] + common)) == 0
    with open(out, newline="") as f:
        rows = list(csv.DictReader(f))
    methods = ["unet", "unet_axis2_linear", "linear", "cubic"]
    assert list(rows[0]) == ["scan", "method", "ssim", "psnr", "mse", "rmse", "mae"] and set(METRIC_COLUMNS) <= set(rows[0])
    scans = ["scan.nii.gz", "scan4d.nii[t=0]", "scan4d.nii[t=1]", "mean"]
    assert [(r["scan"], r["method"]) for r in rows] == [(s, m) for s in scans for m in methods]
    x = torch.from_numpy(vol).cuda()
    want = V.evaluate_volume(model, x, isotropic=True, batch_size=2, use_graph=False)
    for r in rows[:4]:
        assert [float(r[k]) for k in METRIC_COLUMNS] == pytest.approx(want[r["method"]].cpu().tolist(), rel=1e-12)
    assert [float(r["ssim"]) for r in rows[:4]] == pytest.approx([float(r["ssim"]) for r in rows[4:8]], rel=1e-12)      # t=0 is the 3-D scan
    assert float(rows[12]["ssim"]) == pytest.approx(np.mean([float(rows[i]["ssim"]) for i in (0, 4, 8)]), rel=1e-12)

    # a supplied low-resolution scan, default axis
    low = tmp_path / "low.nii"
    lr = V.downsample2(x, (0, 1)).cpu().numpy()
    write_nifti(str(low), lr, NiftiHeader.new(lr.shape, (2.0, 2.0, 1.0)), ())
    out2 = tmp_path / "given.csv"
    assert cli.main(cli.parse_args(["--reference", str(one), "--input", str(low), "--data_range", "3000", "--output_csv", str(out2)] + common)) == 0
    with open(out2, newline="") as f:
        rows2 = list(csv.DictReader(f))
    assert [(r["scan"], r["method"]) for r in rows2] == [(s, m) for s in ("scan.nii.gz", "mean") for m in ("unet", "linear", "cubic")]
    want2 = V.evaluate_volume(model, x, val_range=3000.0, batch_size=2, use_graph=False)
    assert float(rows2[1]["psnr"]) == pytest.approx(float(want2["linear"][4]), rel=1e-12)

    assert cli.main(cli.parse_args(["--reference", str(one), "--cpu"] + common)) == 1
    assert cli.main(cli.parse_args(["--reference", str(one), str(two), "--input", str(low)] + common)) == 1      # --input with two scans
    assert cli.main(cli.parse_args(["--reference", str(tmp_path / "missing.nii")] + common)) == 1
