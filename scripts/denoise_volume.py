#!/usr/bin/env python3
"""Take the noise out of a NIfTI scan on the device (extension).

    python scripts/denoise_volume.py --input lowfield.nii.gz --output denoised.nii.gz
    python scripts/denoise_volume.py --input scan.nii.gz --output denoised.nii.gz --sigma 12.5 --beta 0.8 --radius 2

Noise is the defining property of low-field MR, and in a magnitude image it is Rician: it lifts the dark regions.  This is the 3-D
non-local-means filter with 3 x 3 x 3 patches, a search window of ``--radius`` voxels either side (1..5, default 3) and the Rician
correction on the squared signal (``--noise rician``, the default; ``gaussian`` is the plain weighted mean).  ``--sigma`` is the
noise level in intensity units; without it, it is estimated per frame from the air around the head, whose magnitude follows a
Rayleigh distribution: the background is the complement of the Otsu foreground (``volume_eval.foreground_mask``) grown by
``--noise_margin`` voxels (0..4, default 3), written with ``--save_background``.  A skull-stripped or zero-padded scan has no air to
measure: the run stops and asks for ``--sigma``.  ``--beta`` (default 1) scales the filter's strength, ``h^2 = 2 beta sigma^2`` per
patch voxel.  A 4-D input is processed frame by frame, sigma per frame.  The output keeps the input's header, as float32.  Sigma
(9 digits: the float32 value exactly), the background count and sigma as a share of the foreground median are logged.  Equal to ``volume_denoise.denoise_np`` bit for bit
(``csrc/volume_denoise.hip``).  Exit code 0 / 1 (error logged), as ``scripts/match_bias.py``.
"""
import argparse
import logging
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from mri_superresolution_amd.utils.nifti import frames as frames_of, read_nifti      # noqa: E402
from mri_superresolution_amd.volume_denoise import denoise_volume                                  # noqa: E402
from mri_superresolution_amd.volume_eval import foreground_mask                                    # noqa: E402
from scripts._cli import add_cpu_flag, frame_tag, join_frames, run, save_nifti, to_device        # noqa: E402

logger = logging.getLogger("denoise_volume")


def denoise_file(input_path, output_path, sigma=None, beta=1.0, radius=3, noise="rician", noise_margin=3, save_background=None,
                 device="cuda"):
    """NIfTI file -> denoised NIfTI file; returns (the output array as written, the sigma of every frame)."""
    if noise not in ("gaussian", "rician"):
        raise ValueError(f"--noise is gaussian or rician, got {noise!r}")
    if save_background and sigma is not None:
        raise ValueError("--save_background goes with an estimated sigma: with --sigma there is no background mask")
    data, header = read_nifti(input_path)
    frames = frames_of(data)
    outs, backgrounds, sigmas = [], [], []
    for t, frame in enumerate(frames):
        vol = to_device(frame, device)
        out, found = denoise_volume(vol, sigma=sigma, beta=beta, radius=radius, rician=noise == "rician", margin=noise_margin,
                                    return_noise=True)
        fg = vol[(foreground_mask(vol)[0] != 0) & torch.isfinite(vol)]
        median = float(fg.median()) if fg.numel() else float("nan")
        share = f"{100.0 * found['sigma'] / median:.2f} % of the foreground median {median:.6g}" if median > 0 else "no foreground median"
        origin = f"estimated from {found['count']} background voxels" if sigma is None else "given"
        logger.info(f"{frame_tag(t, len(frames))}sigma {found['sigma']:.9g} ({origin}), {share}")
        sigmas.append(found["sigma"])
        outs.append(out.cpu().numpy())
        if save_background:
            backgrounds.append(found["background"].to(torch.uint8).cpu().numpy())
    result = join_frames(outs, data.ndim)
    save_nifti(output_path, result, header)
    if save_background:
        save_nifti(save_background, join_frames(backgrounds, data.ndim), header)
        logger.info(f"Saved the background mask to {save_background}")
    logger.info(f"Denoised volume {tuple(data.shape)} ({noise}, radius {radius}, beta {beta:g}) saved to {output_path}")
    return result, sigmas


def _body(args, device):
    denoise_file(args.input, args.output, args.sigma, args.beta, args.radius, args.noise, args.noise_margin, args.save_background,
                 device)


def main(args):
    return run(_body, args, logger, "denoising")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Rician non-local-means denoising of a NIfTI volume (extension)")
    p.add_argument("--input", type=str, required=True, help="input scan: single-file NIfTI-1, .nii or .nii.gz, 3-D or 4-D")
    p.add_argument("--output", type=str, required=True, help="output scan, .nii or .nii.gz, float32, the input's header")
    p.add_argument("--sigma", type=float, default=None, help="the noise level in intensity units; default: estimated from the background of every frame")
    p.add_argument("--beta", type=float, default=1.0, help="strength of the filter: h^2 = 2 beta sigma^2 per patch voxel")
    p.add_argument("--radius", type=int, default=3, help="search radius in voxels, 1..5")
    p.add_argument("--noise", type=str, choices=["gaussian", "rician"], default="rician",
                   help="rician (default): the weighted mean of the squared signal minus 2 sigma^2, then the root; gaussian: the plain weighted mean")
    p.add_argument("--noise_margin", type=int, default=3, help="the background is this many voxels (0..4) away from the Otsu foreground")
    p.add_argument("--save_background", type=str, default=None, help="write the background mask sigma was estimated from as a NIfTI with the input's header")
    add_cpu_flag(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
