"""Bias-field matching (GPU), the public surface: scripts/match_bias.py on phantom NIfTIs and scripts/evaluate_volume.py's
--match_bias (its option rules and the function that prepares an input frame)."""
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

import biasutil as B                                                         # noqa: E402
from mri_superresolution_amd import volume_bias as V                         # noqa: E402
from mri_superresolution_amd import volume_intensity as I                    # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, read_nifti, write_nifti   # noqa: E402
from mri_superresolution_amd.volume_eval import downsample2_np, foreground_mask_np     # noqa: E402
from scripts import evaluate_volume as eval_cli                              # noqa: E402
from scripts import match_bias as bias_cli                                   # noqa: E402

PIXDIM = (1.0, 1.25, 2.0)
AFFINE = np.array([[1.0, 0.0, 0.0, -20.0], [0.0, 1.25, 0.0, -30.0], [0.0, 0.0, 2.0, -36.0], [0.0, 0.0, 0.0, 1.0]])


def read(path):
    data, hdr = read_nifti(path)
    return np.ascontiguousarray(data), hdr


def test_match_bias_cli(tmp_path, caplog):
    src, ref, _, sm, rm = B.phantom()
    src4 = np.stack([src, (src * np.float32(0.5)).astype(np.float32)], axis=3)
    paths = {n: str(tmp_path / f"{n}.nii.gz") for n in ("in", "like", "in4", "out", "out4", "mask", "like_mask", "shifted", "small")}
    field_path = str(tmp_path / "sub" / "field.nii.gz")
    write_nifti(paths["in"], src, NiftiHeader.new(src.shape, PIXDIM, affine=AFFINE))
    write_nifti(paths["like"], ref, NiftiHeader.new(ref.shape, PIXDIM, affine=AFFINE))
    write_nifti(paths["in4"], src4, NiftiHeader.new(src4.shape, PIXDIM + (2.0,), affine=AFFINE))
    write_nifti(paths["mask"], sm, NiftiHeader.new(sm.shape, PIXDIM, affine=AFFINE))
    write_nifti(paths["like_mask"], rm, NiftiHeader.new(rm.shape, PIXDIM, affine=AFFINE))
    sigmas = V.sigmas_for(AFFINE, 8.0)
    assert sigmas == (8.0, 6.4, 4.0)
    # the pair form, masks from files, the field saved
    base = ["--input", paths["in"], "--output", paths["out"], "--sigma_mm", "8"]
    with caplog.at_level(logging.INFO):
        assert bias_cli.main(bias_cli.parse_args(base + ["--like", paths["like"], "--mask", paths["mask"], "--like_mask", paths["like_mask"],
                                                         "--save_field", field_path])) == 0
    assert "field in" in caplog.text
    want_out, want_field = V.match_bias_np(src, ref, sm, rm, sigmas)
    out, hdr = read(paths["out"])
    h_in = read_nifti(paths["in"])[1]
    assert B.same_bits(out, want_out) and B.same_bits(read(field_path)[0], want_field)
    assert hdr.shape == src.shape and np.array_equal(hdr.affine(), h_in.affine()) and hdr.get("datatype") == 16
    assert list(hdr.get("pixdim")) == list(h_in.get("pixdim"))
    # Otsu masks (the default) and another limit
    assert bias_cli.main(bias_cli.parse_args(base + ["--like", paths["like"], "--limit", "1.1"])) == 0
    want_out = V.match_bias_np(src, ref, foreground_mask_np(src), foreground_mask_np(ref), sigmas, 1.1)[0]
    assert B.same_bits(read(paths["out"])[0], want_out)
    # the single-scan form
    assert bias_cli.main(bias_cli.parse_args(base + ["--mask", paths["mask"], "--save_field", field_path])) == 0
    want_out, want_field = V.correct_bias_np(src, sm, sigmas)
    assert B.same_bits(read(paths["out"])[0], want_out) and B.same_bits(read(field_path)[0], want_field)
    # 4-D, frame by frame, a 3-D --like and 3-D masks serving both frames
    for like in ([], ["--like", paths["like"], "--like_mask", paths["like_mask"]]):
        assert bias_cli.main(bias_cli.parse_args(["--input", paths["in4"], "--output", paths["out4"], "--sigma_mm", "8", "--mask", paths["mask"],
                                                  "--save_field", field_path] + like)) == 0
        data4, hdr4 = read_nifti(paths["out4"])
        field4 = read_nifti(field_path)[0]
        assert hdr4.shape == src.shape + (2,) and field4.shape == src.shape + (2,)
        for t in range(2):
            frame = np.ascontiguousarray(src4[..., t])
            want_out, want_field = V.match_bias_np(frame, ref, sm, rm, sigmas) if like else V.correct_bias_np(frame, sm, sigmas)
            assert B.same_bits(np.ascontiguousarray(data4[..., t]), want_out) and B.same_bits(np.ascontiguousarray(field4[..., t]), want_field)
    # a --like on another grid: the error points to the tools that bring it onto this one
    shifted = AFFINE.copy()
    shifted[:3, 3] += 2.0
    write_nifti(paths["shifted"], ref, NiftiHeader.new(ref.shape, PIXDIM, affine=shifted))
    write_nifti(paths["small"], np.ascontiguousarray(ref[:-2]), NiftiHeader.new((ref.shape[0] - 2,) + ref.shape[1:], PIXDIM, affine=AFFINE))
    for other in ("shifted", "small"):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            assert bias_cli.main(bias_cli.parse_args(base + ["--like", paths[other]])) == 1
        assert "reslice_volume.py" in caplog.text and "register_volume.py" in caplog.text
    # bad combinations
    assert bias_cli.main(bias_cli.parse_args(base + ["--like_mask", paths["like_mask"]])) == 1      # goes with --like
    assert bias_cli.main(bias_cli.parse_args(base + ["--sigma_mm", "60"])) == 1                      # 180 taps either side
    assert bias_cli.main(bias_cli.parse_args(base + ["--limit", "0.5"])) == 1
    assert bias_cli.main(bias_cli.parse_args(base + ["--cpu"])) == 1
    assert bias_cli.main(bias_cli.parse_args(["--input", str(tmp_path / "none.nii"), "--output", paths["out"]])) == 1


def test_evaluate_volume_check_options():
    ok = ("in.nii", None, "linear", "header", "none", "none")
    eval_cli.check_options(*ok)
    eval_cli.check_options(*ok, "none", 25.0)
    eval_cli.check_options(*ok, "pair", 10.0)
    eval_cli.check_options(*ok, match_bias="pair")
    eval_cli.check_options("in.nii", "rigid", "cubic", "global", "otsu", "landmarks", "pair", 0.0)
    eval_cli.check_options(None, None, "linear", "header", "none", "none", "none")
    with pytest.raises(ValueError, match="--match_bias goes with --input"):
        eval_cli.check_options(None, None, "linear", "header", "none", "none", "pair")
    with pytest.raises(ValueError, match="none or pair"):
        eval_cli.check_options(*ok, "hum")
    with pytest.raises(ValueError, match="sigma"):
        eval_cli.check_options(*ok, "pair", -1.0)
    with pytest.raises(ValueError, match="sigma"):
        eval_cli.check_options(*ok, "pair", float("nan"))
    args = eval_cli.parse_args(["--reference", "r.nii"])
    assert args.match_bias == "none" and args.match_bias_sigma_mm == 25.0
    args = eval_cli.parse_args(["--reference", "r.nii", "--input", "i.nii", "--match_bias", "pair", "--match_bias_sigma_mm", "12"])
    assert args.match_bias == "pair" and args.match_bias_sigma_mm == 12.0
    with pytest.raises(SystemExit):
        eval_cli.parse_args(["--reference", "r.nii", "--match_bias", "n4"])


def test_evaluate_volume_prepares_the_input():
    """--match_bias none: the frame the methods see is what it was before the flag existed - the input itself, or what
    match_intensity returns; pair: match_bias against downsample2 of the reference, after the intensity map."""
    src, ref, _, _, _ = B.phantom()                  # (40, 48, 36): the reference; the input is its mean over pairs times a field
    low_ref = downsample2_np(ref, (0, 1))
    low = (low_ref * downsample2_np(B.phantom()[2], (0, 1))).astype(np.float32)
    lr, vol = torch.from_numpy(low).cuda(), torch.from_numpy(ref).cuda()
    assert eval_cli.prepare_input(lr, vol) is lr
    assert eval_cli.prepare_input(lr, vol, "none", "none", (0, 1), None) is lr
    mapped = I.match_intensity(lr, vol, torch.from_numpy(foreground_mask_np(low)).cuda(), torch.from_numpy(foreground_mask_np(ref)).cuda())[0]
    got = eval_cli.prepare_input(lr, vol, "landmarks", "none", (0, 1), None)
    assert torch.equal(got.view(torch.int32), mapped.view(torch.int32))
    sigmas = (3.0, 3.0, 6.0)
    want = V.match_bias_np(low, low_ref, foreground_mask_np(low), foreground_mask_np(low_ref), sigmas)[0]
    got = eval_cli.prepare_input(lr, vol, "none", "pair", (0, 1), sigmas)
    assert B.same_bits(got.cpu().numpy(), want)
    assert B.relative_rms(want, low_ref, foreground_mask_np(low_ref) != 0) < 0.5 * B.relative_rms(low, low_ref, foreground_mask_np(low_ref) != 0)
    want_both = V.match_bias_np(mapped.cpu().numpy(), low_ref, foreground_mask_np(mapped.cpu().numpy()), foreground_mask_np(low_ref), sigmas)[0]
    got = eval_cli.prepare_input(lr, vol, "landmarks", "pair", (0, 1), sigmas)
    assert B.same_bits(got.cpu().numpy(), want_both)
    with pytest.raises(ValueError, match="not half"):
        eval_cli.prepare_input(lr, vol[:30].contiguous(), "none", "pair", (0, 1), sigmas)
