"""Device-side evaluation (GPU): csrc/evalops.hip + the metrics pass of csrc/loss.hip + utils/evalops.py + the batched path
of scripts/evaluate.py.

Bars: the x2 baselines are EXACTLY the host restatement scripts/evaluate.py:upscale_array (integer weights in 1/256, two
exact int32 passes - no tolerance).  PARITY UNPINNED against cv2 itself, like the host function.  mse / mae against float64
numpy on the same fp32 arrays: 1e-6 relative (every term carries at most two fp32 roundings, <= 1.2e-7 relative, all terms
are non-negative; the block-level fp32 partial sums of 1024 terms add a few 1e-7 at worst).  PSNR: 1e-5 dB (4.34 dB per unit
relative error of the mse).  SSIM: 5e-6 against the existing kernel's per-sample value and against the CPU oracle, the bound
tests/test_gpu_model.py uses for per-sample SSIM.  Batched against per-image harness: see the test."""
import csv
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd.utils import evalops                    # noqa: E402
from mri_superresolution_amd.utils.losses import ssim                # noqa: E402
from oracle import losses_ref                                        # noqa: E402
from oracle.inputs import make_pair                                  # noqa: E402
from scripts import evaluate                                         # noqa: E402

UP_METHODS = ("bilinear", "bicubic", "sharp_bilinear")
SHAPES = [(1, 1, 1), (1, 1, 5), (2, 5, 1), (1, 2, 2), (3, 37, 53), (2, 64, 80), (2, 128, 128), (1, 50, 70)]


def _images(rng, b, h, w, kind):
    if kind == "uniform":
        return rng.integers(0, 256, (b, h, w), dtype=np.uint8)
    if kind == "binary":      # 0 / 255 noise: the largest cubic overshoots, saturation on both sides
        return (rng.integers(0, 2, (b, h, w)) * 255).astype(np.uint8)
    if kind == "constant":
        return np.full((b, h, w), 200, dtype=np.uint8)
    if kind == "ramp":        # horizontal ramp: exact .5 ties in the interpolated values
        return np.broadcast_to((np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8), (b, h, w)).copy()
    if kind == "mri":         # as tests/test_gpu_image.py: dark background + bright structure
        a = np.clip(rng.normal(60, 40, (b, h, w)), 0, 255)
        a[:, : h // 3] = 0
        a[:, -2:, -5:] = 255
        return a.astype(np.uint8)
    raise ValueError(kind)


def _check_upscale(imgs, dev, method):
    b, h, w = imgs.shape
    got_u8 = evalops.upscale2_u8(dev, method, as_float=False)
    got_f = evalops.upscale2_u8(dev, method)
    assert got_u8.shape == (b, 2 * h, 2 * w) and got_u8.dtype == torch.uint8
    assert got_f.shape == (b, 1, 2 * h, 2 * w) and got_f.dtype == torch.float32
    got_u8, got_f = got_u8.cpu().numpy(), got_f.cpu().numpy()
    for i in range(b):
        ref = evaluate.upscale_array(imgs[i], method)
        assert ref.dtype == np.float32
        ref_u8 = np.rint(ref * 255).astype(np.uint8)
        assert np.array_equal(got_u8[i], ref_u8), (method, i, np.abs(got_u8[i].astype(int) - ref_u8).max())
        assert np.array_equal(got_f[i, 0], ref), (method, i)


@pytest.mark.parametrize("kind", ["uniform", "binary", "constant", "ramp", "mri"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("method", UP_METHODS)
def test_upscale2_equals_host_restatement_exactly(method, shape, kind):
    rng = np.random.default_rng(sum(map(ord, kind + method)) * 1000 + shape[0] * 100 + shape[1] * 7 + shape[2])
    imgs = _images(rng, *shape, kind)
    _check_upscale(imgs, torch.from_numpy(imgs).cuda(), method)


@pytest.mark.parametrize("method", UP_METHODS)
def test_upscale2_misaligned_input_takes_the_tail_path(method):
    """A batch that starts at an odd byte address (contiguous there): no 16-byte loads, same result; a single (h,w) image
    takes the same path as a batch of one."""
    rng = np.random.default_rng(11)
    b, h, w = 2, 48, 64
    imgs = rng.integers(0, 256, (b, h, w), dtype=np.uint8)
    buf = torch.zeros(b * h * w + 1, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(b, h, w)
    view.copy_(torch.from_numpy(imgs))
    assert view.is_contiguous() and view.data_ptr() % 16 == 1
    _check_upscale(imgs, view, method)
    one = evalops.upscale2_u8(torch.from_numpy(imgs[0]).cuda(), method).cpu().numpy()
    assert np.array_equal(one[0, 0], evaluate.upscale_array(imgs[0], method))


def test_upscale2_and_unit_from_u8_argument_checks():
    x = torch.zeros((4, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match="Unknown interpolation method: lanczos"):
        evalops.upscale2_u8(x.cuda(), "lanczos")
    with pytest.raises(RuntimeError):
        evalops.upscale2_u8(x, "bilinear")                 # CPU tensor: no fallback
    with pytest.raises(ValueError):
        evalops.upscale2_u8(x.cuda().float(), "bilinear")
    with pytest.raises(RuntimeError):
        evalops.unit_from_u8(x)
    v = torch.arange(256, dtype=torch.uint8).repeat(40).cuda()
    for t in (v, v[:259], v[:3], v[1:]):                   # vector path, with a tail, tail only, misaligned start
        got = evalops.unit_from_u8(t).cpu().numpy()
        assert got.shape == tuple(t.shape)
        assert np.array_equal(got, (t.cpu().numpy() / 255.0).astype(np.float32))


def _metric_pairs():
    pairs = []
    for n, h, w, seed in ((3, 32, 40, 3), (2, 25, 35, 4)):
        low, high = make_pair(n, h, w, seed)
        pairs.append((torch.nn.functional.interpolate(low, scale_factor=2, mode="nearest"), high, "make_pair"))
    base = make_pair(1, 32, 40, 9)[1]                        # 64 x 80
    same = base.clone()
    eps4, eps255 = base.clone(), base.clone()
    base[0, 0, 30, 41] = 0.5
    same[0, 0, 30, 41] = 0.5
    eps4[0, 0, 30, 41] = 0.5 + 1e-4                          # mse = 1e-8 / 5120 ~ 2e-12: below the 1e-10 guard
    eps255[0, 0, 30, 41] = 0.5 + 1.0 / 255.0                 # mse ~ 3e-9: above the guard, ~ 85.2 dB
    pairs.append((same, base, "identical"))
    pairs.append((eps4, base, "guard"))
    pairs.append((eps255, base, "formula"))
    return pairs


@pytest.mark.parametrize("case", range(5))
def test_image_metrics_against_numpy_and_the_ssim_kernel(case):
    pred, ref, kind = _metric_pairs()[case]
    got = evalops.image_metrics(pred.cuda(), ref.cuda())
    assert got.shape == (pred.shape[0], 5) and got.dtype == torch.float64 and got.is_cuda
    got = got.cpu().numpy()
    ss_kernel = ssim(pred.cuda(), ref.cuda(), size_average=False).cpu().numpy()
    ss_oracle = losses_ref.ssim(pred, ref, size_average=False).numpy()
    for i in range(pred.shape[0]):
        d = pred[i, 0].numpy().astype(np.float64) - ref[i, 0].numpy().astype(np.float64)
        mse, mae = float((d * d).mean()), float(np.abs(d).mean())
        s, g_mse, g_rmse, g_mae, g_psnr = (float(v) for v in got[i])
        print(f"{kind}[{i}]: mse {g_mse:.9e} (numpy {mse:.9e}), mae {g_mae:.9e} (numpy {mae:.9e}), psnr {g_psnr:.7f}, "
              f"ssim {s:.8f} (kernel {ss_kernel[i]:.8f}, oracle {ss_oracle[i]:.8f})")
        assert abs(g_mse - mse) <= 1e-6 * mse and abs(g_mae - mae) <= 1e-6 * mae
        assert g_rmse == math.sqrt(g_mse)
        ref_psnr = 100.0 if mse < 1e-10 else 10.0 * math.log10(1.0 / mse)
        assert abs(g_psnr - ref_psnr) <= 1e-5
        if kind in ("identical", "guard"):
            assert g_psnr == 100.0
        if kind == "formula":
            assert 85.0 < g_psnr < 85.4
        assert abs(s - float(ss_kernel[i])) <= 5e-6 and abs(s - float(ss_oracle[i])) <= 5e-6


@pytest.mark.parametrize("window_size", [3, 15])
def test_image_metrics_window_sizes(window_size):
    low, high = make_pair(2, 25, 35, 6)
    pred = torch.nn.functional.interpolate(low, scale_factor=2, mode="nearest").cuda()
    got = evalops.image_metrics(pred, high.cuda(), window_size=window_size, sigma=1.2, val_range=1.0).cpu().numpy()
    ref = ssim(pred, high.cuda(), window_size=window_size, sigma=1.2, size_average=False).cpu().numpy()
    assert np.abs(got[:, 0] - ref).max() <= 5e-6


def test_image_metrics_argument_checks_and_val_range():
    low, high = make_pair(1, 16, 16, 2)
    a, b = high.cuda(), (high * 0.9).cuda()
    with pytest.raises(NotImplementedError):
        evalops.image_metrics(a, b, window_size=10)          # even window: refused like ssim()
    with pytest.raises(RuntimeError):
        evalops.image_metrics(high, high)                    # CPU tensors: no fallback
    with pytest.raises(ValueError):
        evalops.image_metrics(a, b[..., :-1])
    m1 = evalops.image_metrics(a, b).cpu().numpy()[0]
    m255 = evalops.image_metrics(a * 255.0, b * 255.0, val_range=255.0).cpu().numpy()[0]
    assert abs(m255[4] - m1[4]) <= 1e-4                      # PSNR is scale-free: R^2 / mse


def _write_pairs(tmp_path):
    from PIL import Image
    from mri_superresolution_amd.models.unet_model import UNetSuperRes
    from oracle.unet_ref import formula_state_dict
    lr, hr, ck = tmp_path / "lr", tmp_path / "hr", tmp_path / "ck"
    for d in (lr, hr, ck):
        d.mkdir()
    low, high = make_pair(5, 32, 40, 3)
    low2, high2 = make_pair(2, 24, 24, 4)
    files = [(f"a{i}.png", low[i, 0], high[i, 0]) for i in range(5)] + [(f"b{i}.png", low2[i, 0], high2[i, 0]) for i in range(2)]
    for name, l, h in files:
        Image.fromarray((l.numpy() * 255).astype(np.uint8)).save(lr / name)
        Image.fromarray((h.numpy() * 255).astype(np.uint8)).save(hr / name)
    m = UNetSuperRes(1, 1, 16)
    m.load_state_dict(formula_state_dict(16, 2))
    torch.save({"model_state_dict": m.state_dict()}, ck / "best_model_unet.pth")
    return lr, hr, ck, [n for n, _, _ in files]


def test_batched_harness_equals_per_image_harness(tmp_path):
    """7 pairs of two sizes in chunks of 3 (one full chunk -> graph replay, partial chunks -> eager).  Baselines: ssim 5e-6,
    mse / mae 1e-5 relative (the per-image path averages in float32 numpy, itself only good to a few 1e-7 - the exact check of
    the kernel is the metrics test above, this one checks the wiring).  U-Net, graph on and off: ssim, rmse, mae 1e-6
    absolute, the bound of tests/test_gpu_image.py for batched against single-image inference."""
    from scripts import infer
    lr, hr, ck, names = _write_pairs(tmp_path)
    model = infer.load_model("unet", str(ck / "best_model_unet.pth"), torch.device("cuda"), base_filters=16)
    pairs = evaluate.find_pairs(str(hr), str(lr))
    assert len(pairs) == 7
    ref = {(r["image"], r["method"]): r for r in evaluate.run_benchmarks(pairs, model, torch.device("cuda"))}
    for use_graph in (True, False):
        rows = evaluate.run_benchmarks_batched(pairs, model, torch.device("cuda"), batch_size=3, use_graph=use_graph)
        got = {(r["image"], r["method"]): r for r in rows}
        assert len(rows) == 28 and set(got) == set(ref) == {(n, m) for n in names for m in evaluate.METHODS}
        assert [(r["image"], r["method"]) for r in rows] == [(os.path.basename(p), m) for p, _ in pairs for m in evaluate.METHODS]
        for key, r in ref.items():
            g = got[key]
            assert set(g) == set(r) and g["time"] > 0.0
            print(key, use_graph, {k: (g[k], r[k]) for k in ("ssim", "mse", "rmse", "mae", "psnr")})
            if key[1] == "unet":
                assert all(abs(g[k] - r[k]) <= 1e-6 for k in ("ssim", "rmse", "mae")), (key, g, r)
            else:
                assert abs(g["ssim"] - r["ssim"]) <= 5e-6, (key, g, r)
                assert all(abs(g[k] - r[k]) <= 1e-5 * r[k] for k in ("mse", "mae")), (key, g, r)
                assert abs(g["psnr"] - r["psnr"]) <= 1e-5       # same images, float64 numpy mse: 4.34 dB x 1e-6, rounded up
            assert g["rmse"] == math.sqrt(g["mse"])
    # a pair whose HR image is not twice the LR size is refused as in the per-image path
    from PIL import Image
    Image.fromarray(np.zeros((50, 80), np.uint8)).save(hr / "a2.png")
    with pytest.raises(ValueError, match="a2.png: bicubic output"):
        evaluate.run_benchmarks_batched(pairs, model, torch.device("cuda"), batch_size=3)


def test_evaluate_cli_batched(tmp_path):
    lr, hr, ck, names = _write_pairs(tmp_path)
    out = tmp_path / "eval"
    cmd = [sys.executable, os.path.join(REPO, "scripts", "evaluate.py"), "--full_res_dir", str(hr), "--low_res_dir", str(lr),
           "--checkpoint_dir", str(ck), "--base_filters", "16", "--output_dir", str(out), "--batch_size", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = list(csv.DictReader(open(out / "benchmark_results.csv")))
    assert len(rows) == 4 * len(names) and {r["method"] for r in rows} == set(evaluate.METHODS)
    assert list(rows[0]) == ["image", "method", "ssim", "psnr", "mse", "rmse", "mae", "time"]
    for r in rows:
        assert 0.0 <= float(r["ssim"]) <= 1.0 and float(r["psnr"]) > 5.0 and abs(float(r["rmse"]) ** 2 - float(r["mse"])) < 1e-9
    assert os.path.exists(out / "summary.txt")
    bad = subprocess.run(cmd[:7] + [str(tmp_path / "nope")] + cmd[8:], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1
    cpu = subprocess.run(cmd + ["--cpu"], capture_output=True, text=True, timeout=300)
    assert cpu.returncode == 1                               # --cpu still fails loudly
