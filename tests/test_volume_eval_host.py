"""Volume evaluation, the part that needs no GPU: the numpy specifications of mri_superresolution_amd/volume_eval.py against
independent torch implementations on the CPU, the argument checks of evaluate_volume and the command line's parser.

Bars.  One interpolation pass along one axis is, per output, 2 (linear) or 4 (cubic) rounded products and 1 or 3 rounded sums of
magnitude at most W * A (A the amplitude of the data, W the sum of the absolute weights: 1 linear, 1.28125 cubic): at most 1.5 or
3.5 ulp(W^p * A) of error per pass p, and the same again for torch's own float32 arithmetic.  So the bar is
2 * 1.5 * passes ulp(A) for linear and 2 * 3.5 * passes ulp(1.28125^passes * A) for cubic - a few ulp of the amplitude.
Measured with A = 3000: linear over three axes 2 ulp (bar 9), cubic over one axis 2 ulp (bar 7), over two axes 2 ulp of
1.28125^2 A (bar 14)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd import _lib                                   # noqa: E402
from mri_superresolution_amd import volume_eval as V                       # noqa: E402
from scripts import evaluate_volume as cli                                 # noqa: E402

AMP = 3000.0


def volume(shape, seed=0):
    return np.random.default_rng(seed).uniform(-AMP, AMP, shape).astype(np.float32)


def test_the_c_abi_declares_the_new_entries():
    for name in ("mrisr_f32_volume_down2", "mrisr_f32_volume_up2", "mrisr_f32_volume_metrics", "mrisr_volume_metrics_finalize"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    lib = _lib.load()      # refusals need no GPU: nothing is launched
    assert lib.mrisr_f32_volume_down2(None, 2, 2, 2, 7, None, None) == -1 and b"null" in lib.mrisr_last_error()
    assert lib.mrisr_f32_volume_up2(None, 2, 2, 2, 7, _lib.RESAMPLE_LINEAR, None, None) == -1
    assert lib.mrisr_f32_volume_metrics(None, None, 2, 2, 2, 1.0, 1.5, 11, None, None) == -1
    assert lib.mrisr_volume_metrics_finalize(None, 2, 2, 2, 1.0, None, None) == -1


def test_linear_equals_torch_trilinear():
    v = volume((5, 6, 7))
    got = V.upscale2_np(v, "linear")
    want = F.interpolate(torch.from_numpy(v)[None, None], scale_factor=2, mode="trilinear", align_corners=False)[0, 0].numpy()
    err = np.abs(got - want).max() / np.spacing(np.float32(AMP))
    print(f"linear against trilinear: {err:.1f} ulp of the amplitude")
    assert got.shape == (10, 12, 14) and err <= 2 * 1.5 * 3


@pytest.mark.parametrize("axes", [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2)], ids=str)
def test_cubic_equals_torch_bicubic(axes):
    """torch's CPU bicubic: A = -0.75, half-pixel centres, clamped indices - written independently of this project."""
    v = volume((5, 6, 7), seed=1)
    # extents 1, 2, 3 on the interpolated axes as well: every clamped tap on both ends
    for shape in ((5, 6, 7), (1, 2, 3), (3, 1, 2), (2, 3, 1)):
        v = volume(shape, seed=sum(shape))
        got = V.upscale2_np(v, "cubic", axes)
        rest = [a for a in (0, 1, 2) if a not in axes]
        if len(axes) == 1:
            t = torch.from_numpy(np.ascontiguousarray(np.moveaxis(v, axes[0], 2))).reshape(1, -1, 1, shape[axes[0]])
            r = F.interpolate(t, scale_factor=(1, 2), mode="bicubic", align_corners=False)
            want = np.moveaxis(r.reshape(*[shape[a] for a in rest], 2 * shape[axes[0]]).numpy(), 2, axes[0])
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.moveaxis(v, rest[0], 0)))[None]
            want = np.moveaxis(F.interpolate(t, scale_factor=2, mode="bicubic", align_corners=False)[0].numpy(), 0, rest[0])
        passes = len(axes)
        ulp = np.spacing(np.float32(1.28125 ** passes * AMP))
        err = np.abs(got - want).max() / ulp
        print(f"cubic {axes} {shape}: {err:.1f} ulp")
        assert got.shape == want.shape and err <= 2 * 3.5 * passes


def test_cubic_weights_are_keys_minus_three_quarters_and_exact_in_float32():
    a = -0.75

    def keys(x):
        x = abs(x)
        return (a + 2) * x ** 3 - (a + 3) * x ** 2 + 1 if x <= 1 else a * x ** 3 - 5 * a * x ** 2 + 8 * a * x - 4 * a

    assert [keys(d) for d in (1.75, 0.75, 0.25, 1.25)] == list(V.CUBIC_WEIGHTS)
    assert all(float(np.float32(w)) == w for w in V.CUBIC_WEIGHTS) and sum(V.CUBIC_WEIGHTS) == 1.0


def test_down_of_up_of_a_constant_is_the_constant():
    c = np.full((4, 6, 2), 7.25, dtype=np.float32)
    for axes in ((0, 1, 2), (0, 1), (2,)):
        assert np.array_equal(V.downsample2_np(V.upscale2_np(c, "linear", axes), axes), c)
    v = volume((4, 6, 2), seed=3)
    d = V.downsample2_np(v, (0, 2))
    assert d.shape == (2, 6, 1) and d[1, 4, 0] == np.float32((v[2, 4, 0] + v[3, 4, 0]) + (v[2, 4, 1] + v[3, 4, 1])) * np.float32(0.25)
    with pytest.raises(ValueError):
        V.downsample2_np(volume((3, 4, 4)), (0,))
    with pytest.raises(ValueError):
        V.downsample2_np(v, ())
    with pytest.raises(ValueError):
        V.upscale2_np(v, "nearest")


@pytest.mark.parametrize("window_size", [3, 11, 15])
def test_metrics_specification_equals_a_full_window_conv3d(window_size):
    rng = np.random.default_rng(window_size)
    a = rng.uniform(0, 1, (9, 8, 7))
    b = np.clip(a + rng.normal(0, 0.05, a.shape), 0, 1)
    got = V.volume_metrics_np(a, b, 1.0, window_size)
    g = torch.from_numpy(V.gaussian_window_np(window_size, 1.5))
    w = (g[:, None, None] * g[None, :, None] * g[None, None, :])[None, None]

    def blur(x):
        return F.conv3d(torch.from_numpy(x)[None, None], w, padding=window_size // 2)[0, 0].numpy()

    mu1, mu2 = blur(a), blur(b)
    s11, s22, s12 = blur(a * a) - mu1 ** 2, blur(b * b) - mu2 ** 2, blur(a * b) - mu1 * mu2
    ssim = (((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 ** 2 + mu2 ** 2 + 1e-4) * (s11 + s22 + 9e-4))).mean()
    mse = ((a - b) ** 2).mean()
    want = [ssim, mse, np.sqrt(mse), np.abs(a - b).mean(), 10 * np.log10(1.0 / mse)]
    assert np.abs(got - np.array(want)).max() <= 1e-12
    assert abs(V.gaussian_window_np(window_size, 1.5).sum() - 1) < 1e-6


def test_identical_volumes_give_ssim_one_and_psnr_hundred():
    a = np.random.default_rng(0).uniform(0, 1, (6, 5, 4))
    m = V.volume_metrics_np(a, a, 1.0)
    assert abs(m[0] - 1) <= 1e-12 and m[1] == 0 and m[3] == 0 and m[4] == 100.0
    with pytest.raises(NotImplementedError):
        V.volume_metrics_np(a, a, 1.0, window_size=4)
    with pytest.raises(ValueError):
        V.volume_metrics_np(a, a, 0.0)


def test_evaluate_volume_argument_checks():
    ref = torch.zeros((4, 6, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.evaluate_volume(None, ref)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.volume_metrics(ref, ref, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.upscale2(ref, "cubic")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.downsample2(ref)
    for bad in (ref[0], ref.double(), torch.zeros((0, 2, 2))):
        with pytest.raises(ValueError):
            V.evaluate_volume(None, bad)
    with pytest.raises(ValueError):
        V.evaluate_volume(None, ref, axis=3)
    with pytest.raises(ValueError):
        V.evaluate_volume(None, ref, batch_size=0)
    with pytest.raises(ValueError):
        V.evaluate_volume(None, ref, val_range=0.0)
    with pytest.raises(ValueError, match="exactly half"):
        V.evaluate_volume(None, ref, lr=torch.zeros((2, 3, 4)))                       # axis 2 is not doubled without isotropic
    with pytest.raises(ValueError, match="exactly half"):
        V.evaluate_volume(None, ref, lr=torch.zeros((2, 3, 8)), isotropic=True)
    with pytest.raises(ValueError, match="exactly half"):
        V.evaluate_volume(None, torch.zeros((5, 6, 8)), lr=torch.zeros((2, 3, 8)))    # an odd extent has no half
    with pytest.raises(ValueError):
        V.evaluate_volume(None, torch.zeros((1, 6, 8)))                               # nothing left after the crop
    with pytest.raises(ValueError):
        V.upscale2(ref, "nearest")
    with pytest.raises(ValueError):
        V.downsample2(ref, axes=(0, 0))


def test_command_line_parser_and_cpu_refusal():
    args = cli.parse_args(["--reference", "a.nii.gz", "b.nii"])
    assert args.reference == ["a.nii.gz", "b.nii"] and args.axis == 2 and not args.isotropic and args.input is None
    assert args.batch_size == 16 and args.data_range is None and args.output_csv is None and not args.no_graph and not args.use_amp
    args = cli.parse_args(["--reference", "a.nii", "--input", "lr.nii", "--isotropic", "--data_range", "4095", "--output_csv", "o.csv",
                           "--no_graph", "--use_amp", "--batch_size", "4", "--base_filters", "16", "--checkpoint_path", "x.pth"])
    assert args.isotropic and args.data_range == 4095.0 and args.output_csv == "o.csv" and args.batch_size == 4 and args.input == "lr.nii"
    with pytest.raises(SystemExit):
        cli.parse_args(["--reference", "a.nii", "--isotropic", "--axis", "0"])
    with pytest.raises(SystemExit):
        cli.parse_args([])
    assert cli.main(cli.parse_args(["--reference", "a.nii", "--cpu"])) == 1
    assert cli.CSV_COLUMNS == ["scan", "method", "ssim", "psnr", "mse", "rmse", "mae"]
    rows = [{"scan": s, "method": m, "ssim": v, "mse": v, "rmse": v, "mae": v, "psnr": v} for s, v in (("a", 1.0), ("b", 3.0))
            for m in ("unet", "linear")]
    means = cli.mean_rows(rows)
    assert [r["method"] for r in means] == ["unet", "linear"] and all(r["ssim"] == 2.0 and r["scan"] == "mean" for r in means)
    assert "unet" in cli.format_table("a", rows[:2])
