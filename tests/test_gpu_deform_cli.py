"""Deformable registration (GPU), the public surface: scripts/register_volume.py --nonrigid and scripts/evaluate_volume.py
--deform_input on tiny NIfTI files written here."""
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
sys.path.insert(0, os.path.join(REPO, "tests"))

import deformutil as U                                                       # noqa: E402
from mri_superresolution_amd.models.unet_model import UNetSuperRes          # noqa: E402
from mri_superresolution_amd.utils.evalops import METRIC_COLUMNS             # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, read_nifti, write_nifti   # noqa: E402
from mri_superresolution_amd.volume_eval import upscale2_np                  # noqa: E402
from scripts import evaluate_volume as eval_cli                              # noqa: E402
from scripts import register_volume as register_cli                          # noqa: E402

PIXDIM = (1.0, 1.25, 2.0)
AFFINE = np.array([[1.0, 0.0, 0.0, -12.0], [0.0, 1.25, 0.0, -17.0], [0.0, 0.0, 2.0, -31.0], [0.0, 0.0, 0.0, 1.0]])


def rms(a, b, where):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b)[where] ** 2)))


def test_register_volume_nonrigid(tmp_path, caplog):
    fixed, moving, _, mask = U.phantom()
    paths = {n: str(tmp_path / f"{n}.nii") for n in ("fixed", "moving", "plain", "none", "demons")}
    field_path = str(tmp_path / "sub" / "field.nii.gz")
    write_nifti(paths["fixed"], fixed, NiftiHeader.new(fixed.shape, PIXDIM, affine=AFFINE))
    write_nifti(paths["moving"], moving, NiftiHeader.new(moving.shape, PIXDIM, affine=AFFINE))
    base = ["--fixed", paths["fixed"], "--moving", paths["moving"], "--bins", "32"]
    assert register_cli.main(register_cli.parse_args(base + ["--output", paths["plain"]])) == 0
    assert register_cli.main(register_cli.parse_args(base + ["--output", paths["none"], "--nonrigid", "none"])) == 0
    with caplog.at_level(logging.INFO):
        assert register_cli.main(register_cli.parse_args(base + ["--output", paths["demons"], "--nonrigid", "demons", "--nonrigid_levels", "2",
                                                                 "--nonrigid_iterations", "15", "10", "--save_field", field_path])) == 0
    assert "level 12x14x16: mean squared difference" in caplog.text and "level 24x28x32: mean squared difference" in caplog.text
    assert "minimum Jacobian determinant" in caplog.text and "--nonrigid_sigma" not in caplog.text
    # the default path is reached unchanged: the same bytes without the flag and with --nonrigid none
    with open(paths["plain"], "rb") as a, open(paths["none"], "rb") as b:
        assert a.read() == b.read()
    h_fixed = read_nifti(paths["fixed"])[1]
    rigid = np.ascontiguousarray(read_nifti(paths["none"])[0])
    data, hdr = read_nifti(paths["demons"])
    data = np.ascontiguousarray(data)
    assert hdr.shape == fixed.shape and np.array_equal(hdr.affine(), h_fixed.affine()) and hdr.get("datatype") == 16
    field, field_hdr = read_nifti(field_path)
    assert field.shape == fixed.shape + (3,) and field.dtype == np.float32 and field_hdr.get("datatype") == 16
    assert np.array_equal(field_hdr.affine(), h_fixed.affine()) and list(field_hdr.get("dim"))[:5] == [4, 24, 28, 32, 3]
    assert 0.5 < np.abs(field).max() < 3.0
    # closer to the fixed scan than the rigid stage alone: the specification reaches 0.10 of the starting difference here
    before, after = rms(rigid, fixed, mask), rms(data, fixed, mask)
    print(f"RMS difference inside the object: rigid {before:.3f}, demons {after:.3f}")
    assert after < 0.5 * before
    # a field that folds is warned about, and the warning names the remedy
    caplog.clear()
    with caplog.at_level(logging.INFO):
        assert register_cli.main(register_cli.parse_args(base + ["--output", paths["demons"], "--nonrigid", "demons", "--nonrigid_sigma", "0",
                                                                 "--nonrigid_iterations", "30"])) == 0
    if "0 voxel(s) with a determinant that is not positive" not in caplog.text:
        assert "--nonrigid_sigma" in caplog.text
    # option rules
    assert register_cli.main(register_cli.parse_args(base + ["--output", paths["demons"], "--save_field", field_path])) == 1
    assert register_cli.main(register_cli.parse_args(base + ["--output", paths["demons"], "--nonrigid", "demons", "--nonrigid_sigma", "9"])) == 1
    with pytest.raises(SystemExit):
        register_cli.parse_args(base + ["--output", paths["demons"], "--nonrigid", "syn"])


@pytest.fixture(scope="module")
def checkpoint_args(tmp_path_factory):
    torch.manual_seed(1234)
    model = UNetSuperRes(1, 1, base_filters=16).cuda().eval()
    ckdir = tmp_path_factory.mktemp("ck")
    torch.save({"model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, ckdir / "best_model_unet.pth")
    return ["--checkpoint_dir", str(ckdir), "--base_filters", "16", "--batch_size", "4", "--no_graph"]


def read_rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def test_evaluate_volume_deform_input(checkpoint_args, tmp_path, caplog):
    """The reference is the fixed phantom doubled in plane; the input is the moving phantom, the same head under a field of 1.5
    voxels.  --deform_input demons must run, keep the table's rows and raise the PSNR of the interpolation baselines, which see the
    input itself; --deform_input none must score what a run without the option scores."""
    fixed, moving = U.phantom(shape=(16, 24, 24))[:2]
    ref = upscale2_np(fixed, "linear", (0, 1))
    ref_affine = AFFINE.copy()
    ref_affine[:3, 0], ref_affine[:3, 1] = AFFINE[:3, 0] / 2, AFFINE[:3, 1] / 2
    paths = {n: str(tmp_path / f"{n}.nii.gz") for n in ("ref", "low")}
    write_nifti(paths["ref"], ref, NiftiHeader.new(ref.shape, (0.5, 0.625, 2.0), affine=ref_affine))
    write_nifti(paths["low"], moving, NiftiHeader.new(moving.shape, PIXDIM, affine=AFFINE))

    def run(name, *flags):
        out = str(tmp_path / f"{name}.csv")
        code = eval_cli.main(eval_cli.parse_args(["--reference", paths["ref"], "--input", paths["low"], "--output_csv", out, *flags] + checkpoint_args))
        assert code == 0, name
        return read_rows(out)

    plain = run("plain")
    none = run("none", "--deform_input", "none")
    with caplog.at_level(logging.INFO):
        demons = run("demons", "--deform_input", "demons", "--match_intensity", "range")
    assert "warped onto" in caplog.text and "minimum Jacobian determinant" in caplog.text and "without --match_intensity" not in caplog.text
    assert [r["method"] for r in plain] == [r["method"] for r in none] == [r["method"] for r in demons]
    assert [r["method"] for r in demons][:3] == ["unet", "linear", "cubic"] and set(METRIC_COLUMNS) <= set(demons[0])
    for ra, rb in zip(plain, none):      # the 1e-12 of tests/test_gpu_reslice_cli.py: the metrics' double atomics arrive in any order
        assert [ra[k] for k in ra if k not in METRIC_COLUMNS] == [rb[k] for k in rb if k not in METRIC_COLUMNS]
        assert [float(ra[k]) for k in METRIC_COLUMNS] == pytest.approx([float(rb[k]) for k in METRIC_COLUMNS], rel=1e-12, abs=0)
    matched = run("matched", "--match_intensity", "range")
    for rm, rd in zip(matched, demons):
        print(f"{rm['method']:8s} PSNR matched {float(rm['psnr']):.3f} demons {float(rd['psnr']):.3f}")
        if rm["method"] in ("linear", "cubic"):
            assert float(rd["psnr"]) > float(rm["psnr"])
    caplog.clear()
    with caplog.at_level(logging.INFO):
        run("unmatched", "--deform_input", "demons")
    assert "without --match_intensity" in caplog.text
    # option rules
    args = eval_cli.parse_args(["--reference", "r.nii"])
    assert args.deform_input == "none"
    with pytest.raises(SystemExit):
        eval_cli.parse_args(["--reference", "r.nii", "--deform_input", "syn"])
    with pytest.raises(ValueError, match="goes with --input"):
        eval_cli.check_options(None, None, "linear", "header", "none", "none", deform_input="demons")
