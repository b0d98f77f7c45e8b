"""The low-field degradation (GPU), the public surface: ``scripts/simulate_lowfield_volume.py`` on small 3-D and 4-D NIfTI files written
here, and ``scripts/evaluate_volume.py --degrade_noise / --degrade_snr / --degrade_seed`` on the tiny model and files of
tests/test_gpu_unring_cli.py (reference volumes of (16, 16, 24): ``volume_metrics`` runs as one workgroup, rows compare exactly)."""
import csv
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mri_superresolution_amd import volume_eval as V                         # noqa: E402
from mri_superresolution_amd import volume_kspace as K                       # noqa: E402
from mri_superresolution_amd import volume_lowfield as LF                    # noqa: E402
from mri_superresolution_amd.volume_intensity import masked_landmarks_np      # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, downscaled_affine, read_nifti, write_nifti    # noqa: E402
from scripts import evaluate_volume as eval_cli                              # noqa: E402
from scripts import simulate_lowfield_volume as sim_cli                      # noqa: E402
from test_gpu_unring_cli import SHAPE, bits, boxes, files, model             # noqa: E402, F401  (the fixtures)


def test_simulate_script_3d(files, caplog):
    ref = files["arrays"][0]
    out = str(files["dir"] / "sim3.nii.gz")
    with caplog.at_level("INFO"):
        assert sim_cli.main(sim_cli.parse_args(["--input", files["ref"], "--output", out, "--noise_sigma", "20", "--seed", "5"])) == 0
    got, header = read_nifti(out)
    seed = LF.frame_seeds(5, 0, 1)[0]
    want = LF.simulate_lowfield_np(ref, sigma=20.0, seed=seed)
    assert got.dtype == np.float32 and got.shape == (8, 8, 12) and np.array_equal(bits(got), bits(want))
    assert tuple(header.shape) == (8, 8, 12)
    assert np.allclose(header.affine(), downscaled_affine(read_nifti(files["ref"])[1].affine(), (0, 1, 2)))
    assert [float(p) for p in header.get("pixdim")[1:4]] == [2.0, 2.0, 2.0]
    assert "sigma 20" in caplog.text and f"seed {seed}" in caplog.text and "% of the foreground median" in caplog.text
    # two runs write the same bytes; another seed does not; gaussian, two axes and a window follow the specification
    again = str(files["dir"] / "sim3_again.nii.gz")
    assert sim_cli.main(sim_cli.parse_args(["--input", files["ref"], "--output", again, "--noise_sigma", "20", "--seed", "5"])) == 0
    assert np.array_equal(bits(read_nifti(again)[0]), bits(got))
    assert sim_cli.main(sim_cli.parse_args(["--input", files["ref"], "--output", again, "--noise_sigma", "20", "--seed", "6", "--axes", "0", "1",
                                            "--window", "hamming", "--noise", "gaussian"])) == 0
    other, header = read_nifti(again)
    want = LF.simulate_lowfield_np(ref, (0, 1), "hamming", 20.0, LF.frame_seeds(6, 0, 1)[0], rician=False)
    assert other.shape == (8, 8, 24) and np.array_equal(bits(other), bits(want)) and tuple(header.shape) == (8, 8, 24)
    # the grid kept; no noise flag: the truncation alone
    assert sim_cli.main(sim_cli.parse_args(["--input", files["ref"], "--output", again, "--no_truncate", "--noise_sigma", "3"])) == 0
    kept, header = read_nifti(again)
    assert np.array_equal(bits(kept), bits(LF.add_noise_np(ref, 3.0, LF.frame_seeds(0, 0, 1)[0]))) and tuple(header.shape) == SHAPE
    assert sim_cli.main(sim_cli.parse_args(["--input", files["ref"], "--output", again])) == 0
    assert np.array_equal(bits(read_nifti(again)[0]), bits(K.truncate2_np(ref)))
    # errors are logged, the exit code is 1
    assert sim_cli.main(sim_cli.parse_args(["--input", files["ref"], "--output", again, "--noise_sigma", "-1"])) == 1
    assert sim_cli.main(sim_cli.parse_args(["--input", files["ref"], "--output", again, "--snr", "0"])) == 1
    assert sim_cli.main(sim_cli.parse_args(["--input", files["ref"], "--output", again, "--cpu"])) == 1
    with pytest.raises(SystemExit):
        sim_cli.parse_args(["--input", files["ref"], "--output", again, "--snr", "3", "--noise_sigma", "2"])


def test_simulate_script_4d_and_snr(files, caplog):
    ref = files["arrays"][0]
    four = np.stack([ref, ref[::-1].copy() * np.float32(0.5)], axis=3)
    src, out = str(files["dir"] / "hr4.nii.gz"), str(files["dir"] / "sim4.nii")
    write_nifti(src, four, NiftiHeader.new(four.shape, (1.0, 1.0, 1.0)))
    with caplog.at_level("INFO"):
        assert sim_cli.main(sim_cli.parse_args(["--input", src, "--output", out, "--snr", "12.5", "--seed", "9", "--axes", "0", "1"])) == 0
    got, header = read_nifti(out)
    assert got.shape == (8, 8, 24, 2) and got.dtype == np.float32 and tuple(header.shape) == (8, 8, 24, 2)
    seeds = LF.frame_seeds(9, 0, 2)
    assert seeds[0] != seeds[1]
    logged = [float(x) for x in re.findall(r"sigma ([0-9.eE+-]+) = the foreground median", caplog.text)]
    assert len(logged) == 2
    for t in range(2):
        low = K.truncate2_np(np.ascontiguousarray(four[..., t]), (0, 1))
        median = float(masked_landmarks_np(low, V.foreground_mask_np(low), (50.0,))[0][0])
        sigma = median / 12.5
        assert abs(logged[t] / sigma - 1) < 1e-5                             # six digits are logged
        assert np.array_equal(bits(got[..., t]), bits(LF.add_noise_np(low, sigma, seeds[t]))), t


def test_evaluate_volume_adds_noise_to_the_volume_it_makes(files, model, capsys):
    d = files["dir"]
    common = ["--checkpoint_dir", files["ck"], "--base_filters", "16", "--batch_size", "4", "--no_graph"]

    def run(name, *flags):
        out = str(d / f"{name}.csv")
        capsys.readouterr()
        code = eval_cli.main(eval_cli.parse_args(["--reference", files["ref"], "--output_csv", out, *flags] + common))
        text = open(out, newline="").read() if code == 0 else ""
        return code, text, list(csv.DictReader(text.splitlines())), capsys.readouterr().out

    ref = torch.from_numpy(files["arrays"][0]).cuda()
    data_range = float((ref.max() - ref.min()).item())

    def linear_of(low):
        return V.volume_metrics(V.upscale2(torch.from_numpy(low).cuda(), "linear", (0, 1)), ref, data_range).cpu().numpy().tolist()

    # without any new flag: the table of before, twice the same, and no word of noise
    code, plain_csv, plain, plain_out = run("plain", "--degrade", "kspace")
    code2, again_csv, _, again_out = run("again", "--degrade", "kspace")
    assert code == 0 and code2 == 0 and plain_csv == again_csv and plain_out == again_out and "noise" not in plain_out
    assert "ref.nii.gz (degrade kspace)\n" in plain_out
    assert not any(hasattr(eval_cli.parse_args(["--reference", "x"]), n) for n in ("degrade_noise", "degrade_snr", "degrade_seed"))
    row = [r for r in plain if r["method"] == "linear" and r["scan"] != "mean"][0]
    assert [float(row[c]) for c in V.METRIC_COLUMNS] == linear_of(K.truncate2_np(files["arrays"][0], (0, 1)))
    # --degrade kspace --degrade_noise 20: the title says so, the linear row is that of the specification's volume
    code, _, noisy, noisy_out = run("noisy", "--degrade", "kspace", "--degrade_noise", "20")
    assert code == 0 and "ref.nii.gz (degrade kspace, noise σ = 20, seed 0)\n" in noisy_out
    assert "scan(s) (degrade kspace, noise σ = 20, seed 0)\n" in noisy_out
    want = LF.add_noise_np(K.truncate2_np(files["arrays"][0], (0, 1)), 20.0, LF.frame_seeds(0, 0, 1)[0])
    row = [r for r in noisy if r["method"] == "linear" and r["scan"] != "mean"][0]
    assert [float(row[c]) for c in V.METRIC_COLUMNS] == linear_of(want) and [r["method"] for r in noisy] == [r["method"] for r in plain]
    # the default degradation, the mean over pairs, another seed; an SNR
    code, _, mean_rows, mean_out = run("mean", "--degrade_noise", "20", "--degrade_seed", "4")
    assert code == 0 and "ref.nii.gz (degrade mean, noise σ = 20, seed 4)\n" in mean_out
    want = LF.add_noise_np(V.downsample2_np(files["arrays"][0], (0, 1)), 20.0, LF.frame_seeds(4, 0, 1)[0])
    row = [r for r in mean_rows if r["method"] == "linear" and r["scan"] != "mean"][0]
    assert [float(row[c]) for c in V.METRIC_COLUMNS] == linear_of(want)
    code, _, _, snr_out = run("snr", "--degrade", "kspace", "--degrade_snr", "10")
    assert code == 0 and "(degrade kspace, noise SNR = 10, seed 0)" in snr_out
    # --denoise_input nlm is accepted next to it and changes the rows; alone it raises the message of before
    code, _, denoised, den_out = run("denoised", "--degrade", "kspace", "--degrade_noise", "20", "--denoise_input", "nlm", "--denoise_sigma", "20")
    assert code == 0 and "noise σ = 20, seed 0" in den_out
    assert [r for r in denoised if r["method"] == "linear"][0]["psnr"] != [r for r in noisy if r["method"] == "linear"][0]["psnr"]
    with pytest.raises(ValueError, match="^--denoise_input goes with --input$"):
        eval_cli.check_options(None, None, "linear", "header", "none", "none", denoise_input="nlm")
    assert run("alone", "--denoise_input", "nlm")[0] == 1
    eval_cli.check_options(None, None, "linear", "header", "none", "none", denoise_input="nlm", degrade_noise={"sigma": 20.0, "seed": 0})
    # with --input there is nothing to add the noise to; the seed alone; a negative sigma; both levels
    assert run("input", "--input", files["low"], "--degrade_noise", "20")[0] == 1
    with pytest.raises(ValueError, match="go without --input"):
        eval_cli.check_options(files["low"], None, "linear", "header", "none", "none", degrade_noise={"sigma": 20.0, "seed": 0})
    assert run("seed", "--degrade_seed", "3")[0] == 1 and run("negative", "--degrade_noise", "-2")[0] == 1
    with pytest.raises(SystemExit):
        eval_cli.parse_args(["--reference", "x", "--degrade_noise", "2", "--degrade_snr", "3"])
