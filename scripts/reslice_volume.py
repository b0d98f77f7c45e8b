#!/usr/bin/env python3
"""Reslice a NIfTI scan onto another voxel grid on the device (extension).

    python scripts/reslice_volume.py --input lowfield.nii.gz --output on_ref_grid.nii.gz --like reference.nii.gz --interp cubic
    python scripts/reslice_volume.py --input thick.nii.gz --output iso.nii.gz --spacing 0 0 1.5

``--like`` takes the grid - extents and affine - of another scan: the input is resampled through the two headers' affines
(``utils.nifti.grid_matrix``), whatever the spacing, field of view, axis order or rotation between them.  ``--spacing SX SY SZ``
changes the voxel size in mm per axis on the input's own grid (0 keeps an axis; ``utils.nifti.respaced_grid``: the corner of the
first voxel stays where it is).  ``--interp nearest|linear|cubic`` (``csrc/volume_reslice.hip``, bit-equal to
``volume_reslice.reslice_np``); voxels whose centre falls outside the input are ``--fill``, and their share is logged.  A 4-D
file goes timepoint by timepoint.  The output is float32 under ``utils.nifti.header_for_grid`` of the input's header.  The
transform itself is never estimated: the headers are taken as they are.  Exit code 0 / 1 (error logged), as
``scripts/infer_volume.py``.
"""
import argparse
import logging
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from mri_superresolution_amd.utils.nifti import frames, grid_matrix, header_for_grid, read_nifti, respaced_grid   # noqa: E402
from mri_superresolution_amd.volume_reslice import covered_share, reslice                                              # noqa: E402
from scripts._cli import add_cpu_flag, join_frames, run, save_nifti                                                   # noqa: E402

logger = logging.getLogger("reslice_volume")


def reslice_file(input_path, output_path, like=None, spacing=None, interp="linear", fill=0.0, device="cuda"):
    """NIfTI file -> NIfTI file on the grid of ``like`` or at ``spacing``; returns the output array (as written)."""
    data, header = read_nifti(input_path)
    src_affine = header.affine()
    if like is not None:
        like_header = read_nifti(like)[1]
        dst_affine, dst_shape = like_header.affine(), tuple(like_header.shape[:3])
    else:
        dst_affine, dst_shape = respaced_grid(src_affine, data.shape[:3], spacing)
    m = grid_matrix(src_affine, dst_affine)
    outs = [reslice(torch.from_numpy(np.ascontiguousarray(f)).to(device), m, dst_shape, interp, fill) for f in frames(data)]
    share = covered_share(data.shape[:3], m, dst_shape, device)
    result = join_frames([o.cpu().numpy() for o in outs], data.ndim)
    logger.info(f"{100.0 * (1.0 - float(share)):.2f} % of the output voxels fell outside the input (set to {fill:g}).")
    save_nifti(output_path, result, header_for_grid(header, dst_shape, dst_affine))
    logger.info(f"Resliced volume {tuple(data.shape)} -> {tuple(result.shape)} ({interp}) saved to {output_path}")
    return result


def _body(args, device):
    reslice_file(args.input, args.output, args.like, args.spacing, args.interp, args.fill, device)


def main(args):
    return run(_body, args, logger, "reslicing")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Reslice a NIfTI volume onto another voxel grid (extension)")
    p.add_argument("--input", type=str, required=True, help="input scan: single-file NIfTI-1, .nii or .nii.gz, 3-D or 4-D")
    p.add_argument("--output", type=str, required=True, help="output scan, .nii or .nii.gz, float32")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--like", type=str, default=None, help="take the grid (extents and affine) of this scan")
    g.add_argument("--spacing", type=float, nargs=3, default=None, metavar=("SX", "SY", "SZ"),
                   help="voxel size in mm per axis on the input's own grid; 0 keeps an axis")
    p.add_argument("--interp", type=str, choices=["nearest", "linear", "cubic"], default="linear")
    p.add_argument("--fill", type=float, default=0.0, help="value of the output voxels whose centre lies outside the input")
    add_cpu_flag(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
