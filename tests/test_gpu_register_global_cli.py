"""Registration from far apart (GPU), the public surface: scripts/register_volume.py --init global --mask otsu on the far pair of
tests/farpairutil.py written as two NIfTI files, and the refusal of scripts/evaluate_volume.py --align_init without --align rigid."""
import logging
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import farpairutil as F                                                      # noqa: E402
from mri_superresolution_amd import volume_register as G                     # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, read_nifti, write_nifti      # noqa: E402
from scripts import evaluate_volume as eval_cli                              # noqa: E402
from scripts import register_volume as register_cli                          # noqa: E402


def spacing(affine):
    return tuple(float(s) for s in np.linalg.norm(affine[:3, :3], axis=0))


@pytest.fixture(scope="module")
def far_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("far")
    fixed, moving = F.far_pair()
    paths = {n: str(d / f"{n}.nii.gz") for n in ("fixed", "moving")}
    write_nifti(paths["fixed"], fixed, NiftiHeader.new(fixed.shape, spacing(F.FIXED_AFFINE), affine=F.FIXED_AFFINE))
    write_nifti(paths["moving"], moving, NiftiHeader.new(moving.shape, spacing(F.MOVING_AFFINE), affine=F.MOVING_AFFINE))
    return paths


def test_register_volume_from_far_apart(far_files, tmp_path, caplog):
    """The stored headers are float32 srow fields: the truth moves by less than a hundredth of a voxel."""
    def run(name, *flags):
        transform, out = str(tmp_path / f"{name}.txt"), str(tmp_path / f"{name}.nii.gz")
        code = register_cli.main(register_cli.parse_args(["--fixed", far_files["fixed"], "--moving", far_files["moving"], "--output", out,
                                                          "--bins", str(F.BINS), "--save_transform", transform, *flags]))
        assert code == 0, name
        world = np.loadtxt(transform)
        assert world.shape == (4, 4) and np.array_equal(world[3], [0, 0, 0, 1])
        assert read_nifti(out)[1].shape == F.FIXED_SHAPE
        return world

    with caplog.at_level(logging.INFO):
        found = run("global", "--init", "global", "--mask", "otsu")
    assert "coarse stage: candidate" in caplog.text and "of 125 at stride 4" in caplog.text
    err = F.corner_error_voxels(found)
    print(f"--init global --mask otsu: {err:.3f} voxels off at the worst corner")
    assert err <= 1.0
    caplog.clear()
    with caplog.at_level(logging.INFO):
        default = run("default")
    assert "coarse stage" not in caplog.text
    smallest = float(np.linalg.norm(F.FIXED_AFFINE[:3, :3], axis=0).min())
    apart = G.corner_displacement(found, default, F.FIXED_AFFINE, F.FIXED_SHAPE) / smallest
    print(f"the default flags end {apart:.3f} voxels from it")
    assert apart > 20.0
    for flags in (["--init", "local"], ["--mask", "file.nii"], ["--init_step", "x"]):
        with pytest.raises(SystemExit):
            register_cli.parse_args(["--fixed", far_files["fixed"], "--moving", far_files["moving"], "--output", "o.nii"] + flags)
    # a grid the library refuses: exit code 1, the error logged
    assert register_cli.main(register_cli.parse_args(["--fixed", far_files["fixed"], "--moving", far_files["moving"], "--output",
                                                      str(tmp_path / "o.nii"), "--init", "global", "--init_step", "2"])) == 1


def test_evaluate_volume_refuses_the_new_flags_without_align_rigid(far_files, tmp_path, caplog):
    for flags in (["--align_init", "global"], ["--align_mask", "otsu"], ["--align", "header", "--align_init", "global"],
                  ["--align", "header", "--align_mask", "otsu"]):
        caplog.clear()
        with caplog.at_level(logging.ERROR):
            code = eval_cli.main(eval_cli.parse_args(["--reference", far_files["fixed"], "--input", far_files["moving"],
                                                      "--checkpoint_dir", str(tmp_path / "none"), *flags]))
        assert code == 1 and "go with --align rigid" in caplog.text, flags
    args = eval_cli.parse_args(["--reference", far_files["fixed"]])
    assert args.align_init == "header" and args.align_mask == "none"
    with pytest.raises(SystemExit):
        eval_cli.parse_args(["--reference", far_files["fixed"], "--align_init", "far"])
