#!/usr/bin/env python3
"""Simulate a low-field acquisition of a high-resolution NIfTI scan on the device (extension).

    python scripts/simulate_lowfield_volume.py --input hr.nii.gz --output lr.nii.gz --snr 15
    python scripts/simulate_lowfield_volume.py --input hr.nii.gz --output lr.nii.gz --axes 0 1 --window hamming --noise_sigma 20 --seed 3

The volume twin of ``scripts/simulate_lr.py``: k-space is truncated to its centre along ``--axes`` (default all three, even extents;
``volume_kspace.truncate2``, ``--window hamming`` with that window; ``--no_truncate`` leaves the grid as it is), complex Gaussian noise
of standard deviation sigma is added and the magnitude taken - Rician noise (``volume_lowfield.add_noise``, ``csrc/volume_noise.hip``);
``--noise gaussian`` adds the real part alone.  Sigma is ``--noise_sigma``, in intensity units, or with ``--snr R`` the median of the
truncated volume's Otsu foreground over ``R``; with neither no noise is added.  The noise is seeded and reproducible to the bit:
frame ``t`` draws with ``volume_lowfield.frame_seeds(--seed, 0, frames)[t]``, so no frame of a 4-D file shares a draw with another.
A 4-D input goes frame by frame.  The output is float32 under the header of the halved grid (``utils.nifti.downscaled_affine``,
``header_for_grid``): the scan stays where it was in world space, and ``scripts/evaluate_volume.py --input`` takes it next to the
original.  Sigma, its share of the foreground median and the seed are logged.  Exit code 0 / 1 (error logged).
"""
import argparse
import logging
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from mri_superresolution_amd.utils.nifti import downscaled_affine, frames as frames_of, header_for_grid, read_nifti      # noqa: E402
from mri_superresolution_amd.volume_kspace import truncate2                                                             # noqa: E402
from mri_superresolution_amd.volume_lowfield import add_noise, foreground_median, frame_seeds, sigma_for_snr            # noqa: E402
from scripts._cli import add_cpu_flag, frame_tag, join_frames, run, save_nifti, to_device                                # noqa: E402

logger = logging.getLogger("simulate_lowfield_volume")


def simulate_file(input_path, output_path, axes=(0, 1, 2), window="none", truncate=True, noise_sigma=None, snr=None, rician=True,
                  seed=0, device="cuda"):
    """NIfTI file -> simulated low-field NIfTI file; returns the output array as written."""
    if noise_sigma is not None and snr is not None:
        raise ValueError("--noise_sigma and --snr exclude each other")
    data, header = read_nifti(input_path)
    frames = frames_of(data)
    axes = tuple(sorted(axes))
    seeds = frame_seeds(seed, 0, len(frames))
    outs = []
    for t, frame in enumerate(frames):
        tag = frame_tag(t, len(frames))
        lr = to_device(frame, device)
        if truncate:
            lr = truncate2(lr, axes, window)
        if noise_sigma is None and snr is None:
            logger.info(f"{tag}no noise added (neither --noise_sigma nor --snr)")
        else:
            sigma = float(noise_sigma) if snr is None else sigma_for_snr(lr, snr)
            median, count = foreground_median(lr)
            out = add_noise(lr, sigma, seeds[t], rician=rician, out=lr if truncate else None)
            share = f"{100.0 * sigma / median:.3g} % of the foreground median {median:.6g}" if median > 0 else f"foreground median {median:.6g}"
            logger.info(f"{tag}{'Rician' if rician else 'Gaussian'} noise sigma {sigma:.6g} ({share}, {count} voxels), seed {seeds[t]} "
                        f"(from --seed {seed})")
            lr = out
        outs.append(lr.cpu().numpy())
    result = join_frames(outs, data.ndim)
    if truncate:
        header = header_for_grid(header, result.shape[:3], downscaled_affine(header.affine(), axes))
    save_nifti(output_path, result, header)
    logger.info(f"Simulated low-field volume {tuple(result.shape)} (from {tuple(data.shape)}) saved to {output_path}")
    return result


def _body(args, device):
    simulate_file(args.input, args.output, args.axes, args.window, not args.no_truncate, args.noise_sigma, args.snr, args.noise == "rician",
                  args.seed, device)


def main(args):
    return run(_body, args, logger, "low-field simulation")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Simulate a low-field acquisition of a NIfTI volume: k-space truncation and Rician noise (extension)")
    p.add_argument("--input", type=str, required=True, help="high-resolution scan: single-file NIfTI-1, .nii or .nii.gz, 3-D or 4-D")
    p.add_argument("--output", type=str, required=True, help="output scan, .nii or .nii.gz, float32, the header of the halved grid")
    p.add_argument("--axes", type=int, nargs="+", choices=[0, 1, 2], default=[0, 1, 2], help="the axes to halve (even extents, at most 1024 voxels)")
    p.add_argument("--window", type=str, choices=["none", "hamming"], default="none", help="the k-space window of the truncation")
    p.add_argument("--no_truncate", action="store_true", help="keep the grid: the noise alone")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--noise_sigma", type=float, default=None, metavar="S", help="standard deviation of the noise in intensity units")
    g.add_argument("--snr", type=float, default=None, metavar="R", help="sigma = the median of the truncated volume's Otsu foreground / R")
    p.add_argument("--noise", type=str, choices=["rician", "gaussian"], default="rician", help="magnitude of complex noise, or its real part alone")
    p.add_argument("--seed", type=int, default=0, help="the seed every frame's draw derives from")
    add_cpu_flag(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
