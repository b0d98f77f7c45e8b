"""Zero-filling and k-space truncation (GPU), the public surface: ``volume_eval.evaluate_volume(zerofill=, degrade=)`` and
``scripts/evaluate_volume.py --zerofill / --degrade`` on a tiny model and tiny NIfTI files written here.

The reference volumes are at most (32, 16, 32): ``volume_metrics`` then runs as ONE workgroup, its float64 sums have one addend
each, and two runs give identical floats - so rows can be compared exactly, as numbers and as text."""
import csv
import logging
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd import volume_eval as V                         # noqa: E402
from mri_superresolution_amd import volume_kspace as K                       # noqa: E402
from mri_superresolution_amd.models.unet_model import UNetSuperRes          # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, write_nifti    # noqa: E402
from scripts import evaluate_volume as eval_cli                              # noqa: E402

SHAPE = (16, 16, 24)
KW = dict(batch_size=4, use_graph=False)


def phantom(shape=SHAPE, seed=0):
    """Smooth, periodic and band-limited far below the low-resolution grid's Nyquist rate: a sum of products of cosines with at
    most ``extent / 8`` periods per axis.  K-space truncation loses nothing of it, and zero-filling gives all of it back."""
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in shape), indexing="ij")
    x = np.full(shape, 2.0)
    for _ in range(8):
        term = np.full(shape, rng.uniform(0.2, 1.0))
        for g, d in zip(grids, shape):
            term = term * np.cos(2 * np.pi * rng.integers(0, max(d // 8, 1) + 1) * (g + rng.uniform(0, d)) / d)
        x = x + term
    return (100.0 * x).astype(np.float32)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(1234)
    return UNetSuperRes(1, 1, base_filters=16).cuda().eval()


def test_zerofill_adds_one_row_and_changes_no_other(model):
    ref = torch.from_numpy(phantom()).cuda()
    rng = float((ref.max() - ref.min()).item())
    plain = V.evaluate_volume(model, ref, **KW)
    res = V.evaluate_volume(model, ref, zerofill="none", **KW)
    assert list(plain) == ["unet", "linear", "cubic"] and list(res) == ["unet", "linear", "cubic", "zerofill"]
    for method in plain:
        assert torch.equal(res[method], plain[method]), method      # identical floats
    lr = V.downsample2(ref, (0, 1))
    assert torch.equal(res["zerofill"], V.volume_metrics(K.zerofill2(lr, (0, 1)), ref, rng))
    ham = V.evaluate_volume(model, ref, zerofill="hamming", isotropic=True, **KW)
    assert list(ham) == ["unet", "unet_axis2_linear", "linear", "cubic", "zerofill_hamming"]
    assert torch.equal(ham["zerofill_hamming"], V.volume_metrics(K.zerofill2(V.downsample2(ref), (0, 1, 2), "hamming"), ref, rng))
    # the row gets what every row gets: masked metrics and Dice, in front of the closing row "reference"
    masked = V.evaluate_volume(model, ref, zerofill="none", mask="otsu", tissue_dice=2, **KW)
    assert list(masked) == ["unet", "linear", "cubic", "zerofill", "reference"] and tuple(masked["zerofill"].shape) == (2, 5)
    assert masked.tissue_dice["zerofill"].shape == (2,)
    for bad in (dict(zerofill="hann"), dict(zerofill=True), dict(degrade="fft"), dict(degrade=None)):
        with pytest.raises(ValueError, match="zerofill|degrade"):
            V.evaluate_volume(model, ref, **bad, **KW)


def test_degrade_kspace_makes_the_low_resolution_volume_by_truncation(model, caplog):
    vol = phantom()
    ref = torch.from_numpy(vol).cuda()
    rng = float((ref.max() - ref.min()).item())
    # the claim of this test, for the numpy specification on the CPU: on this phantom zero-filling beats linear and cubic
    lr_np = K.truncate2_np(vol, (0, 1))
    psnr_np = {name: 10 * np.log10(rng ** 2 / max(np.mean((up.astype(np.float64) - vol) ** 2), 1e-300))
               for name, up in (("zerofill", K.zerofill2_np(lr_np, (0, 1))), ("linear", V.upscale2_np(lr_np, "linear", (0, 1))),
                                ("cubic", V.upscale2_np(lr_np, "cubic", (0, 1))))}
    assert psnr_np["zerofill"] > psnr_np["cubic"] > psnr_np["linear"]
    res = V.evaluate_volume(model, ref, zerofill="none", degrade="kspace", **KW)
    lr = K.truncate2(ref, (0, 1))
    assert np.array_equal(lr.cpu().numpy().view(np.uint32), lr_np.view(np.uint32))
    for method in ("linear", "cubic"):
        assert torch.equal(res[method], V.volume_metrics(V.upscale2(lr, method, (0, 1)), ref, rng)), method
    assert torch.equal(res["zerofill"], V.volume_metrics(K.zerofill2(lr, (0, 1)), ref, rng))
    psnr = {k: float(v[4]) for k, v in res.items()}
    print(psnr, psnr_np)
    assert psnr["zerofill"] > psnr["linear"] and psnr["zerofill"] > psnr["cubic"]
    mean = V.evaluate_volume(model, ref, **KW)
    assert not torch.equal(mean["linear"], res["linear"])            # another low-resolution volume
    ham = V.evaluate_volume(model, ref, degrade="kspace_hamming", **KW)
    assert list(ham) == ["unet", "linear", "cubic"]
    assert torch.equal(ham["cubic"], V.volume_metrics(V.upscale2(K.truncate2(ref, (0, 1), "hamming"), "cubic", (0, 1)), ref, rng))
    # a given lr is taken as it is: the setting is ignored, and said so once
    V._DEGRADE_WARNED = False
    with caplog.at_level(logging.WARNING, logger=V.logger.name):
        given = V.evaluate_volume(model, ref, lr=V.downsample2(ref, (0, 1)), degrade="kspace", **KW)
        V.evaluate_volume(model, ref, lr=V.downsample2(ref, (0, 1)), degrade="kspace", **KW)
    assert sum("is ignored" in r.getMessage() for r in caplog.records) == 1
    assert torch.equal(given["linear"], mean["linear"])


def test_cli_flags_rows_titles_and_an_unchanged_default(model, tmp_path, capsys):
    ckdir = tmp_path / "ck"
    ckdir.mkdir()
    torch.save({"model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, ckdir / "best_model_unet.pth")
    common = ["--checkpoint_dir", str(ckdir), "--base_filters", "16", "--batch_size", "4", "--no_graph"]
    ref = str(tmp_path / "ref.nii.gz")
    write_nifti(ref, phantom(), NiftiHeader.new(SHAPE, (1.0, 1.0, 1.0)))

    def run(name, *flags):
        out = str(tmp_path / f"{name}.csv")
        capsys.readouterr()
        code = eval_cli.main(eval_cli.parse_args(["--reference", ref, "--output_csv", out, *flags] + common))
        with open(out, newline="") as f:
            text = f.read()
        return code, text, list(csv.DictReader(text.splitlines())), capsys.readouterr().out

    code, plain_csv, plain, plain_out = run("plain")
    assert code == 0 and [r["method"] for r in plain] == ["unet", "linear", "cubic"] * 2
    assert plain_csv.splitlines()[0] == ",".join(eval_cli.CSV_COLUMNS) and "degrade" not in plain_out and "zerofill" not in plain_out
    code, again_csv, _, again_out = run("again")
    assert code == 0 and again_csv == plain_csv and again_out == plain_out      # a run is reproducible to the byte at this size
    # --zerofill: the rows of the run without it, byte for byte, plus the new row after cubic (the scan and the mean)
    code, zf_csv, zf, zf_out = run("zf", "--zerofill", "none")
    assert code == 0 and [r["method"] for r in zf] == ["unet", "linear", "cubic", "zerofill"] * 2
    assert [ln for ln in zf_csv.splitlines() if ",zerofill," not in ln] == plain_csv.splitlines()
    assert [ln for ln in zf_out.splitlines() if not ln.startswith("zerofill")] == plain_out.splitlines()
    assert sum(ln.startswith("zerofill ") for ln in zf_out.splitlines()) == 2
    x = torch.from_numpy(phantom()).cuda()
    want = V.evaluate_volume(model, x, zerofill="none", **KW)["zerofill"].cpu().numpy()
    row = [r for r in zf if r["method"] == "zerofill" and r["scan"] != "mean"][0]
    assert [float(row[c]) for c in V.METRIC_COLUMNS] == want.tolist()
    # --degrade: in the titles, and another low-resolution volume behind the same methods
    code, _, deg, deg_out = run("deg", "--zerofill", "hamming", "--degrade", "kspace")
    assert code == 0 and [r["method"] for r in deg] == ["unet", "linear", "cubic", "zerofill_hamming"] * 2
    assert "ref.nii.gz (degrade kspace)" in deg_out and "scan(s) (degrade kspace)" in deg_out
    want = V.evaluate_volume(model, x, degrade="kspace", **KW)["cubic"].cpu().numpy()
    row = [r for r in deg if r["method"] == "cubic" and r["scan"] != "mean"][0]
    assert [float(row[c]) for c in V.METRIC_COLUMNS] == want.tolist() and row["psnr"] != plain[2]["psnr"]
    with pytest.raises(SystemExit):
        eval_cli.parse_args(["--reference", ref, "--zerofill", "hann"])
    with pytest.raises(SystemExit):
        eval_cli.parse_args(["--reference", ref, "--degrade", "box"])
