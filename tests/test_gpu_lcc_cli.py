"""The force across contrasts (GPU), the public surface: scripts/register_volume.py --nonrigid_force lcc and
scripts/evaluate_volume.py --deform_force lcc on tiny NIfTI files written here (the phantom seen in another contrast)."""
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
import lccutil                                                               # noqa: E402
from mri_superresolution_amd import volume_deform as D                       # noqa: E402
from mri_superresolution_amd.models.unet_model import UNetSuperRes          # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, read_nifti, write_nifti   # noqa: E402
from mri_superresolution_amd.volume_eval import upscale2_np                  # noqa: E402
from scripts import evaluate_volume as eval_cli                              # noqa: E402
from scripts import register_volume as register_cli                          # noqa: E402

PIXDIM = (1.0, 1.25, 2.0)
AFFINE = np.array([[1.0, 0.0, 0.0, -12.0], [0.0, 1.25, 0.0, -17.0], [0.0, 0.0, 2.0, -31.0], [0.0, 0.0, 0.0, 1.0]])
LEVELS = ["--nonrigid_levels", "2", "--nonrigid_iterations", "15", "10"]


def read_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_register_volume_with_the_correlation_force(tmp_path, caplog):
    fixed, moving = lccutil.contrast_phantom()[:2]
    paths = {n: str(tmp_path / f"{n}.nii") for n in ("fixed", "moving", "rigid", "plain", "ssd", "lcc", "field")}
    write_nifti(paths["fixed"], fixed, NiftiHeader.new(fixed.shape, PIXDIM, affine=AFFINE))
    write_nifti(paths["moving"], moving, NiftiHeader.new(moving.shape, PIXDIM, affine=AFFINE))
    base = ["--fixed", paths["fixed"], "--moving", paths["moving"], "--bins", "32"]
    demons = base + ["--nonrigid", "demons"] + LEVELS
    assert register_cli.main(register_cli.parse_args(base + ["--output", paths["rigid"]])) == 0
    with caplog.at_level(logging.INFO):
        assert register_cli.main(register_cli.parse_args(demons + ["--output", paths["plain"]])) == 0
    assert "mean squared difference" in caplog.text and "mean rho^2" not in caplog.text
    assert register_cli.main(register_cli.parse_args(demons + ["--output", paths["ssd"], "--nonrigid_force", "ssd"])) == 0
    assert read_bytes(paths["plain"]) == read_bytes(paths["ssd"])             # the default writes what it wrote
    caplog.clear()
    with caplog.at_level(logging.INFO):
        assert register_cli.main(register_cli.parse_args(demons + ["--output", paths["lcc"], "--nonrigid_force", "lcc", "--nonrigid_lcc_radius",
                                                                   "2", "--save_field", paths["field"]])) == 0
    assert "level 12x14x16: 1 - mean rho^2" in caplog.text and "level 24x28x32: 1 - mean rho^2" in caplog.text
    assert "mean squared difference" not in caplog.text and "minimum Jacobian determinant" in caplog.text
    # the output is the library's registration of the rigid stage's output
    rigid = torch.from_numpy(np.ascontiguousarray(read_nifti(paths["rigid"])[0], dtype=np.float32)).cuda()
    want = D.register_deformable(torch.from_numpy(fixed.copy()).cuda(), rigid, force="lcc", lcc_radius=2, **lccutil.SCHEDULE)
    data = np.ascontiguousarray(read_nifti(paths["lcc"])[0])
    assert U.same_bits(data, want.warped.cpu().numpy())
    assert U.same_bits(data, D.warp(rigid, want.field).cpu().numpy())
    field, field_hdr = read_nifti(paths["field"])
    assert field.shape == fixed.shape + (3,) and list(field_hdr.get("dim"))[:5] == [4, 24, 28, 32, 3]
    assert U.same_bits(np.ascontiguousarray(np.moveaxis(field, 3, 0)), want.field.cpu().numpy())
    assert read_bytes(paths["lcc"]) != read_bytes(paths["ssd"])
    # option rules
    assert register_cli.main(register_cli.parse_args(base + ["--output", paths["lcc"], "--nonrigid_force", "lcc"])) == 1
    assert register_cli.main(register_cli.parse_args(demons + ["--output", paths["lcc"], "--nonrigid_force", "lcc", "--nonrigid_lcc_radius",
                                                               "5"])) == 1
    with pytest.raises(SystemExit):
        register_cli.parse_args(base + ["--output", paths["lcc"], "--nonrigid_force", "mi"])


def test_evaluate_volume_with_the_correlation_force(tmp_path, caplog):
    torch.manual_seed(1234)
    model = UNetSuperRes(1, 1, base_filters=16).cuda().eval()
    torch.save({"model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, tmp_path / "best_model_unet.pth")
    fixed, moving = U.phantom(shape=(16, 24, 24))[:2]
    ref = upscale2_np(fixed, "linear", (0, 1))
    ref_affine = AFFINE.copy()
    ref_affine[:3, 0], ref_affine[:3, 1] = AFFINE[:3, 0] / 2, AFFINE[:3, 1] / 2
    paths = {n: str(tmp_path / f"{n}.nii.gz") for n in ("ref", "low")}
    write_nifti(paths["ref"], ref, NiftiHeader.new(ref.shape, (0.5, 0.625, 2.0), affine=ref_affine))
    write_nifti(paths["low"], lccutil.other_contrast(moving), NiftiHeader.new(moving.shape, PIXDIM, affine=AFFINE))
    args = ["--reference", paths["ref"], "--input", paths["low"], "--output_csv", str(tmp_path / "out.csv"), "--checkpoint_dir",
            str(tmp_path), "--base_filters", "16", "--batch_size", "4", "--no_graph", "--deform_input", "demons", "--deform_force", "lcc"]
    with caplog.at_level(logging.INFO):
        assert eval_cli.main(eval_cli.parse_args(args)) == 0
    assert "warped onto" in caplog.text and "1 - mean rho^2" in caplog.text
    assert "--match_intensity" not in caplog.text and "mean squared difference" not in caplog.text
    assert os.path.getsize(tmp_path / "out.csv") > 0
    # option rules
    assert eval_cli.parse_args(["--reference", "r.nii"]).deform_force == "ssd"
    with pytest.raises(SystemExit):
        eval_cli.parse_args(["--reference", "r.nii", "--deform_force", "mi"])
    with pytest.raises(ValueError, match="--deform_force lcc goes with"):
        eval_cli.check_options("i.nii", None, "linear", "header", "none", "none", deform_force="lcc")
    with pytest.raises(ValueError, match="--deform_lcc_radius"):
        eval_cli.check_options("i.nii", None, "linear", "header", "none", "none", deform_input="demons", deform_force="lcc", deform_lcc_radius=0)
