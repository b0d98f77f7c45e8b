#!/usr/bin/env python3
"""Take the Gibbs ringing out of a NIfTI scan on the device (extension).

    python scripts/unring_volume.py --input lowfield.nii.gz --output unringed.nii.gz
    python scripts/unring_volume.py --input scan.nii.gz --output unringed.nii.gz --axes 0 1 --shifts 20 --window 1 3

A low-matrix acquisition truncates k-space, and every sharp interface (skull / CSF / cortex) rings with a period of one voxel pair.
This is Kellner's method of local subvoxel shifts (Kellner et al., MRM 2016): every line along ``--axes`` (default all three) is
re-sampled at ``2 x --shifts`` sub-voxel offsets by periodic sinc interpolation, every voxel takes the offset whose neighbourhood -
the differences ``--window`` a..b to one side - oscillates least, and is interpolated back to its own position; the axes are
combined with Kellner's k-space weighting (``volume_unring.unring``, one fused kernel per axis: ``csrc/volume_unring.hip``).  Every
extent along ``--axes`` is 8..512 voxels.  The scan must be on its acquired grid: zero-filled ("interpolated matrix") or
partial-Fourier data rings with another period and is not served.  A 4-D input is processed frame by frame.  The output keeps the
input's header, as float32.  Minimum, maximum and the total variation along each axis are logged before and after.  Exit code 0 / 1
(error logged), as ``scripts/denoise_volume.py``.
"""
import argparse
import logging
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from mri_superresolution_amd.utils.nifti import frames as frames_of, read_nifti                     # noqa: E402
from scripts._cli import add_cpu_flag, frame_tag, join_frames, run, save_nifti, to_device, unring_frame      # noqa: E402

logger = logging.getLogger("unring_volume")


def unring_file(input_path, output_path, axes=(0, 1, 2), shifts=20, window=(1, 3), device="cuda"):
    """NIfTI file -> unringed NIfTI file; returns the output array as written."""
    data, header = read_nifti(input_path)
    frames = frames_of(data)
    options = dict(axes=tuple(axes), K=shifts, window=tuple(window))
    outs = [unring_frame(to_device(frame, device), options, logger, frame_tag(t, len(frames))).cpu().numpy()
            for t, frame in enumerate(frames)]
    result = join_frames(outs, data.ndim)
    save_nifti(output_path, result, header)
    logger.info(f"Unringed volume {tuple(data.shape)} saved to {output_path}")
    return result


def _body(args, device):
    unring_file(args.input, args.output, args.axes, args.shifts, args.window, device)


def main(args):
    return run(_body, args, logger, "unringing")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Gibbs-ringing removal of a NIfTI volume by local subvoxel shifts (extension)")
    p.add_argument("--input", type=str, required=True, help="input scan: single-file NIfTI-1, .nii or .nii.gz, 3-D or 4-D")
    p.add_argument("--output", type=str, required=True, help="output scan, .nii or .nii.gz, float32, the input's header")
    p.add_argument("--axes", type=int, nargs="+", choices=[0, 1, 2], default=[0, 1, 2], help="the axes to unring along (8..512 voxels each)")
    p.add_argument("--shifts", type=int, default=20, help="K: 2K sub-voxel shifts are tried, 1..32")
    p.add_argument("--window", type=int, nargs=2, default=[1, 3], metavar=("A", "B"),
                   help="the differences a..b either side of a voxel judge a shift, 1 <= a <= b <= 4")
    add_cpu_flag(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
