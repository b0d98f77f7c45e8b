"""Gibbs-ringing removal (GPU), the public surface: ``scripts/unring_volume.py``, ``scripts/infer_volume.py --unring`` and
``scripts/evaluate_volume.py --unring_input`` on a tiny model and tiny NIfTI files written here.

The reference volumes are (16, 16, 24): ``volume_metrics`` then runs as ONE workgroup and two runs give identical floats, so rows
are compared exactly, as numbers and as text (tests/test_gpu_kspace_cli.py)."""
import csv
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
from mri_superresolution_amd import volume_unring as U                       # noqa: E402
from mri_superresolution_amd.models.unet_model import UNetSuperRes          # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, read_nifti, write_nifti    # noqa: E402
from scripts import evaluate_volume as eval_cli                              # noqa: E402
from scripts import infer_volume as infer_cli                                # noqa: E402
from scripts import unring_volume as unring_cli                              # noqa: E402

SHAPE = (16, 16, 24)


def boxes(shape=SHAPE, seed=0):
    """Piecewise constant: its truncated k-space rings."""
    rng = np.random.default_rng(seed)
    x = np.full(shape, 50.0, dtype=np.float32)
    x[3:11, 5:13, 5:19] = 400.0
    x[5:9, 7:11, 9:15] = 1000.0
    return x + rng.uniform(0.0, 1.0, shape).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(1234)
    return UNetSuperRes(1, 1, base_filters=16).cuda().eval()


@pytest.fixture(scope="module")
def files(tmp_path_factory, model):
    d = tmp_path_factory.mktemp("unring")
    ref = boxes()
    low = K.truncate2_np(ref, (0, 1))                               # (8, 8, 24): the input of a run across axis 2
    paths = {"ref": str(d / "ref.nii.gz"), "low": str(d / "low.nii.gz"), "low4": str(d / "low4.nii.gz"), "dir": d}
    write_nifti(paths["ref"], ref, NiftiHeader.new(SHAPE, (1.0, 1.0, 1.0)))
    write_nifti(paths["low"], low, NiftiHeader.new(low.shape, (2.0, 2.0, 1.0)))
    four = np.stack([low, low[::-1].copy() * np.float32(0.5)], axis=3)
    write_nifti(paths["low4"], four, NiftiHeader.new(four.shape, (2.0, 2.0, 1.0)))
    ck = d / "ck"
    ck.mkdir()
    torch.save({"model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, ck / "best_model_unet.pth")
    paths["ck"] = str(ck)
    paths["arrays"] = (ref, low, four)
    return paths


def test_unring_volume_script_3d_and_4d(files, caplog):
    ref, low, four = files["arrays"]
    out3, out4 = str(files["dir"] / "u3.nii.gz"), str(files["dir"] / "u4.nii")
    with caplog.at_level("INFO"):
        assert unring_cli.main(unring_cli.parse_args(["--input", files["low"], "--output", out3])) == 0
    got, header = read_nifti(out3)
    want = U.unring(torch.from_numpy(low).cuda()).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)) and not np.array_equal(got, low)
    assert tuple(header.shape) == low.shape and np.allclose(header.affine(), read_nifti(files["low"])[1].affine())
    text = caplog.text
    assert "unring before: min" in text and "unring after: min" in text and "total variation per axis" in text
    assert unring_cli.main(unring_cli.parse_args(["--input", files["low4"], "--output", out4, "--axes", "0", "2", "--shifts", "3",
                                                  "--window", "1", "2"])) == 0
    got4, header4 = read_nifti(out4)
    assert got4.shape == four.shape and got4.dtype == np.float32
    for t in range(2):
        frame = torch.from_numpy(np.ascontiguousarray(four[..., t])).cuda()
        assert np.array_equal(bits(got4[..., t]), bits(U.unring(frame, (0, 2), 3, (1, 2)).cpu().numpy())), t
    # errors are logged, the exit code is 1: a line below 8, a bad K, the CPU
    assert unring_cli.main(unring_cli.parse_args(["--input", files["low"], "--output", out3, "--shifts", "40"])) == 1
    assert unring_cli.main(unring_cli.parse_args(["--input", files["low"], "--output", out3, "--cpu"])) == 1
    with pytest.raises(SystemExit):
        unring_cli.parse_args(["--input", files["low"], "--output", out3, "--axes", "3"])


def infer_args(files, inp, out, *flags):
    return infer_cli.parse_args(["--input", inp, "--output", out, "--checkpoint_dir", files["ck"], "--base_filters", "16", "--batch_size", "4",
                                 "--no_graph", *flags])


def test_infer_volume_sees_the_unringed_input_and_is_unchanged_without_the_flag(files):
    d = files["dir"]
    plain, again, flagged, by_hand = (str(d / f"{n}.nii") for n in ("plain", "again", "flagged", "by_hand"))
    assert infer_cli.main(infer_args(files, files["low"], plain)) == 0
    assert infer_cli.main(infer_args(files, files["low"], again)) == 0
    assert open(plain, "rb").read() == open(again, "rb").read()     # a run is reproducible to the byte
    assert not hasattr(infer_args(files, files["low"], plain), "unring")      # the parsed defaults are those of a build without it
    # with the flag: the bytes of a run on the file unring_volume.py writes
    unringed = str(d / "low_unringed.nii.gz")
    assert unring_cli.main(unring_cli.parse_args(["--input", files["low"], "--output", unringed, "--shifts", "5"])) == 0
    assert infer_cli.main(infer_args(files, files["low"], flagged, "--unring", "--unring_shifts", "5")) == 0
    assert infer_cli.main(infer_args(files, unringed, by_hand)) == 0
    assert open(flagged, "rb").read() == open(by_hand, "rb").read() != open(plain, "rb").read()
    assert infer_cli.main(infer_args(files, files["low"], flagged, "--unring_shifts", "5")) == 1      # a sub-option alone


def test_evaluate_volume_unrings_the_input_and_says_so(files, model, capsys):
    d = files["dir"]
    common = ["--checkpoint_dir", files["ck"], "--base_filters", "16", "--batch_size", "4", "--no_graph"]

    def run(name, *flags):
        out = str(d / f"{name}.csv")
        capsys.readouterr()
        code = eval_cli.main(eval_cli.parse_args(["--reference", files["ref"], "--output_csv", out, *flags] + common))
        text = open(out, newline="").read() if code == 0 else ""
        return code, text, list(csv.DictReader(text.splitlines())), capsys.readouterr().out

    code, plain_csv, plain, plain_out = run("plain", "--input", files["low"])
    assert code == 0 and [r["method"] for r in plain] == ["unet", "linear", "cubic"] * 2 and "unring" not in plain_out
    code, again_csv, _, again_out = run("again", "--input", files["low"])
    assert code == 0 and again_csv == plain_csv and again_out == plain_out
    # with the flag: the rows of a run on the unringed file, and a title that names the step
    unringed = str(d / "low_unringed_eval.nii.gz")
    assert unring_cli.main(unring_cli.parse_args(["--input", files["low"], "--output", unringed])) == 0
    code, flag_csv, flagged, flag_out = run("flagged", "--input", files["low"], "--unring_input")
    code2, hand_csv, _, hand_out = run("by_hand", "--input", unringed)
    assert code == 0 and code2 == 0 and flag_csv == hand_csv != plain_csv
    assert "ref.nii.gz (input unringed along 0 1 2, K = 20)" in flag_out and "scan(s) (input unringed along 0 1 2, K = 20)" in flag_out
    assert flag_out.replace(" (input unringed along 0 1 2, K = 20)", "") == hand_out
    # without --input: the low-resolution volume --degrade kspace makes is unringed
    code, _, deg, deg_out = run("deg", "--degrade", "kspace", "--unring_input", "--unring_axes", "0", "1", "--unring_shifts", "3")
    assert code == 0 and "ref.nii.gz (degrade kspace) (input unringed along 0 1, K = 3)" in deg_out
    ref = torch.from_numpy(files["arrays"][0]).cuda()
    lr = U.unring(K.truncate2(ref, (0, 1)), (0, 1), 3)
    want = V.volume_metrics(V.upscale2(lr, "cubic", (0, 1)), ref, float((ref.max() - ref.min()).item())).cpu().numpy()
    row = [r for r in deg if r["method"] == "cubic" and r["scan"] != "mean"][0]
    assert [float(row[c]) for c in V.METRIC_COLUMNS] == want.tolist()
    code, _, raw, _ = run("deg_plain", "--degrade", "kspace")
    assert code == 0 and [r for r in raw if r["method"] == "cubic"][0]["psnr"] != row["psnr"]
    # the flag needs something to unring; a sub-option needs the flag
    assert run("alone", "--unring_input")[0] == 1
    assert run("sub", "--input", files["low"], "--unring_shifts", "3")[0] == 1
