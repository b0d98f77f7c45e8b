"""GPU tests of scripts/combine_stacks.py: three small NIfTI stacks of the phantom of tests/stackutil.py in, one isotropic volume out."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import stackutil as U                                                                        # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, grid_matrix, read_nifti, write_nifti   # noqa: E402
from mri_superresolution_amd.volume_reslice import reslice                                   # noqa: E402
from mri_superresolution_amd.volume_stacks import voxel_sizes                                # noqa: E402
from scripts import combine_stacks as cli                                                    # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 3


def truth_affine():
    a = np.diag([1.5, 1.5, 1.5, 1.0])
    a[:3, 3] = [-24.0, -27.0, -30.0]
    return a


@functools.lru_cache(maxsize=None)
def stacks():
    return U.orthogonal_stacks(U.phantom(), FACTOR, affine_out=truth_affine())


def write_stacks(tmp_path, volumes, affines, tag=""):
    paths = []
    for k, (y, a) in enumerate(zip(volumes, affines)):
        paths.append(str(tmp_path / f"stack{tag}{k}.nii.gz"))
        write_nifti(paths[-1], y, NiftiHeader.new(y.shape, voxel_sizes(a), a))
    return paths


def run(args):
    assert cli.main(cli.parse_args(args)) == 0
    return args[args.index("--output") + 1]


def error(path):
    t = U.phantom()
    return U.rmse(read_nifti(path)[0][:t.shape[0], :t.shape[1], :t.shape[2]], t)


def test_the_output_lies_on_the_bounding_grid_and_beats_the_reslice_mean(tmp_path):
    ys, _, affines = stacks()
    paths = write_stacks(tmp_path, ys, affines)
    out, initial = str(tmp_path / "iso.nii.gz"), str(tmp_path / "initial.nii.gz")
    run(["--inputs", *paths, "--output", out, "--save_initial", initial, "--profile_samples", str(FACTOR)])
    data, header = read_nifti(out)
    # the last slices hang out of the 32 x 36 x 40 phantom: 11, 12 and 14 slices of three 1.5 mm voxels
    assert data.dtype == np.float32 and data.shape == (33, 36, 42) and tuple(header.shape) == (33, 36, 42)
    assert np.allclose(header.affine(), truth_affine()) and np.allclose(header.get("pixdim")[1:4], 1.5)
    total, count = torch.zeros(data.shape, device="cuda"), torch.zeros(data.shape, device="cuda")
    for y, a in zip(ys, affines):
        g = reslice(torch.from_numpy(y).cuda(), grid_matrix(a, truth_affine()), data.shape, "linear", fill=float("nan"))
        total = total + torch.nan_to_num(g, nan=0.0)
        count = count + (~torch.isnan(g)).float()
    baseline = torch.where(count > 0, total / count.clamp(min=1), torch.zeros_like(total)).clamp(min=0).cpu().numpy()
    assert np.array_equal(read_nifti(initial)[0], baseline)
    assert error(out) < 0.5 * error(initial)                  # the specification reaches 0.07 of it (tests/test_volume_stacks_host.py)


def test_rigid_registration_repairs_a_header_that_is_two_voxels_off(tmp_path):
    ys, _, affines = stacks()
    moved = [a.copy() for a in affines]
    moved[1][:3, 3] += [0.0, 0.0, 3.0]                        # stack 1 claims to lie two 1.5 mm voxels further along z, in its plane
    paths = write_stacks(tmp_path, ys, moved)
    common = ["--inputs", *paths, "--profile_samples", str(FACTOR), "--like", write_stacks(tmp_path, [U.phantom()], [truth_affine()], "truth")[0]]
    plain = run(common + ["--output", str(tmp_path / "plain.nii.gz")])
    registered = run(common + ["--output", str(tmp_path / "registered.nii.gz"), "--register", "rigid"])
    assert read_nifti(registered)[0].shape == U.phantom().shape
    assert error(registered) < error(plain)


def test_a_4d_input_is_combined_frame_by_frame(tmp_path):
    ys, _, affines = stacks()
    second = [(np.float32(0.5) * y[::-1]).copy() for y in ys]
    both = [np.stack([y, z], axis=3) for y, z in zip(ys, second)]
    paths4 = []
    for k, (y, a) in enumerate(zip(both, affines)):
        paths4.append(str(tmp_path / f"frames{k}.nii.gz"))
        write_nifti(paths4[-1], y, NiftiHeader.new(y.shape, voxel_sizes(a), a))
    args = ["--iterations", "3", "--profile", "gaussian", "--no_clamp"]
    out4 = read_nifti(run(["--inputs", *paths4, "--output", str(tmp_path / "iso4.nii.gz"), *args]))[0]
    assert out4.shape == (33, 36, 42, 2)
    for t, volumes in enumerate((ys, second)):
        out3 = read_nifti(run(["--inputs", *write_stacks(tmp_path, volumes, affines, f"f{t}_"), "--output", str(tmp_path / f"iso3_{t}.nii.gz"), *args]))[0]
        assert np.array_equal(out4[..., t], out3)
    assert cli.main(cli.parse_args(["--inputs", paths4[0], write_stacks(tmp_path, ys[1:2], affines[1:2], "lone")[0], "--output",
                                    str(tmp_path / "bad.nii.gz")])) == 1


def test_options_are_refused_before_anything_is_read(tmp_path):
    missing = [str(tmp_path / "a.nii"), str(tmp_path / "b.nii")]
    for bad in (dict(iterations=-1), dict(step=float("nan")), dict(slice_axis=["0", "1", "2"]), dict(thickness_mm=[-1.0]),
                dict(profile_samples=17), dict(spacing=0.0)):
        with pytest.raises(ValueError):
            cli.check_options(missing, **bad)
    with pytest.raises(ValueError, match="1..8"):
        cli.check_options(missing * 5)
    assert cli.check_options(missing, slice_axis=["auto", "2"], thickness_mm=[5.0]) == ([None, 2], [5.0, 5.0])
    assert cli.main(cli.parse_args(["--inputs", *missing, "--output", str(tmp_path / "o.nii"), "--cpu"])) == 1
