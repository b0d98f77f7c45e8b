"""Surface distances (GPU), the public surface: scripts/evaluate_volume.py --tissue_surface and scripts/segment_volume.py --compare on
tiny NIfTI files written here."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import tissueutil as U                                                       # noqa: E402
from mri_superresolution_amd import volume_surface as S                      # noqa: E402
from mri_superresolution_amd.models.unet_model import UNetSuperRes          # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, write_nifti     # noqa: E402
from scripts import evaluate_volume as eval_cli                              # noqa: E402
from scripts import segment_volume as segment_cli                            # noqa: E402

PIXDIM = (1.0, 1.25, 2.0)


@pytest.fixture(scope="module")
def checkpoint_args(tmp_path_factory):
    torch.manual_seed(1234)
    model = UNetSuperRes(1, 1, base_filters=16).cuda().eval()
    ckdir = tmp_path_factory.mktemp("ck")
    torch.save({"model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, ckdir / "best_model_unet.pth")
    return ["--checkpoint_dir", str(ckdir), "--base_filters", "16", "--batch_size", "4", "--no_graph"]


def test_evaluate_volume_tissue_surface(checkpoint_args, tmp_path, capsys, monkeypatch):
    vol = U.phantom()[0]
    ref = str(tmp_path / "ref.nii.gz")
    write_nifti(ref, np.array(vol), NiftiHeader.new(vol.shape, PIXDIM))
    seen = []
    real = S.surface_distances

    def recording(a, b, classes, spacing, background, workspace):
        seen.append((a.cpu().numpy(), b.cpu().numpy(), classes, tuple(spacing), background))
        return real(a, b, classes, spacing, background, workspace)

    monkeypatch.setattr(S, "surface_distances", recording)

    def run(name, *flags):
        out = str(tmp_path / f"{name}.csv")
        code = eval_cli.main(eval_cli.parse_args(["--reference", ref, "--output_csv", out, *flags] + checkpoint_args))
        with open(out, newline="") as f:
            reader = csv.DictReader(f)
            rows = list(reader)
        return code, reader.fieldnames, rows

    code, names, rows = run("surface", "--mask", "otsu", "--tissue_dice", "3", "--tissue_surface")
    assert code == 0
    table = capsys.readouterr().out
    columns = eval_cli.surface_columns(3)
    assert names == eval_cli.CSV_COLUMNS_MASKED + eval_cli.dice_columns(3) + columns
    assert "assd_1" in table and "hd95_3" in table
    methods = ["unet", "linear", "cubic", "reference"]
    assert [r["method"] for r in rows if r["region"] == "foreground" and r["scan"] != "mean"] == methods and len(seen) == 4
    for method, (a, b, classes, spacing, background) in zip(methods, seen):
        assert classes == 3 and background is False and spacing == pytest.approx(PIXDIM, rel=1e-6)
        want = S.surface_distances_np(a, b, 3, spacing, False)
        row = [r for r in rows if r["method"] == method and r["region"] == "foreground" and r["scan"] != "mean"][0]
        got = np.array([float(row[c]) for c in columns])
        assert np.array_equal(got[3:], want.hd95, equal_nan=True)
        assert got[:3] == pytest.approx(want.assd, rel=1e-12, abs=0, nan_ok=True)
        if method == "reference":
            assert got.tolist() == [0.0] * 6
        elif method in ("linear", "cubic"):                            # the random network's classes need not touch each other
            assert np.isfinite(got).all() and (got[:3] > 0).all()
    for r in rows:
        if r["region"] == "whole":
            assert [r[c] for c in columns] == [""] * 6
    # without the switch: the header and the rows of a --tissue_dice run, the Dice columns equal
    code, names, plain = run("plain", "--mask", "otsu", "--tissue_dice", "3")
    assert code == 0 and names == eval_cli.CSV_COLUMNS_MASKED + eval_cli.dice_columns(3) and len(seen) == 4
    assert "assd_" not in capsys.readouterr().out and len(plain) == len(rows)
    for ra, rb in zip(rows, plain):
        assert [ra[c] for c in ("scan", "region", "method", "dice_1", "dice_2", "dice_3")] == \
            [rb[c] for c in ("scan", "region", "method", "dice_1", "dice_2", "dice_3")]
    # option rules
    assert eval_cli.main(eval_cli.parse_args(["--reference", ref, "--mask", "otsu", "--tissue_surface"] + checkpoint_args)) == 1
    assert eval_cli.main(eval_cli.parse_args(["--reference", ref, "--tissue_surface"] + checkpoint_args)) == 1


def test_segment_volume_compare_prints_the_three_distances(tmp_path, capsys):
    vol, mask, _ = U.phantom()
    paths = {n: str(tmp_path / f"{n}.nii.gz") for n in ("scan", "mask", "labels", "smooth", "again")}
    write_nifti(paths["scan"], np.array(vol), NiftiHeader.new(vol.shape, PIXDIM))
    write_nifti(paths["mask"], np.array(mask), NiftiHeader.new(mask.shape, PIXDIM))
    base = ["--mask", paths["mask"], "--classes", "3", "--iterations", "20"]
    assert segment_cli.main(segment_cli.parse_args(["--input", paths["scan"], "--output", paths["labels"], "--beta", "0.0"] + base)) == 0
    capsys.readouterr()
    args = ["--input", paths["scan"], "--output", paths["smooth"], "--beta", "1.0", "--compare", paths["labels"]] + base
    assert segment_cli.main(segment_cli.parse_args(args)) == 0
    out = capsys.readouterr().out
    from mri_superresolution_amd.utils.nifti import read_nifti
    a, b = (read_nifti(paths[n])[0].astype(np.uint8) for n in ("smooth", "labels"))
    want = S.surface_distances_np(a, b, 3, PIXDIM, True)
    for name, values in (("ASSD", want.assd), ("HD95", want.hd95), ("HD", want.hd)):
        line = f"{name} against {paths['labels']}: " + "  ".join(f"class {k + 1} {d:.6f}" for k, d in enumerate(values))
        assert line in out, (line, out)
    assert "Dice against" in out and (want.hd > 0).all()
    # against its own output: every distance is 0
    args = ["--input", paths["scan"], "--output", paths["again"], "--beta", "1.0", "--compare", paths["smooth"]] + base
    assert segment_cli.main(segment_cli.parse_args(args)) == 0
    out = capsys.readouterr().out
    for name in ("ASSD", "HD95", "HD"):
        assert f"{name} against {paths['smooth']}: class 1 0.000000  class 2 0.000000  class 3 0.000000" in out
