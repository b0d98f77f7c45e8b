#!/usr/bin/env python3
"""Segment a NIfTI scan into tissue classes on the device (extension).

    python scripts/segment_volume.py --input scan.nii.gz --output labels.nii.gz --classes 3 --mask otsu --mask_largest --mask_fill_holes 3d
    python scripts/segment_volume.py --input sr.nii.gz --output sr_labels.nii.gz --mask brain.nii.gz --compare reference_labels.nii.gz

Inside a foreground mask the voxels are classified into ``--classes`` K tissue classes, class 1 the darkest: a Gaussian mixture on a
256-bin quantisation of the masked 1st..99th percentile range with a Potts prior of strength ``--beta`` over the 6 face neighbours,
minimised by at most ``--iterations`` sweeps of iterated conditional modes (``volume_tissue.segment_tissue``;
``csrc/volume_tissue.hip``, bit-equal to ``volume_tissue.segment_tissue_np``).  ``--mask otsu`` (the default) takes the mask of
``scripts/evaluate_volume.py``: the exact Otsu threshold of each frame, ``--mask_close``, ``--mask_largest`` and ``--mask_fill_holes``
wired as there; ``--mask PATH`` reads it from a NIfTI-1 file of the input's spatial shape (non-zero = inside; a 3-D mask serves every
timepoint).  The labels are written as uint8 under the input's header, 0 outside the mask, a 4-D file timepoint by timepoint; the
class means, the voxel counts and the sweeps are logged per frame.  ``--compare`` prints the Dice overlap per class with another
label file of the same shape, inside the mask, and the surface distances per class between the two label volumes in the world units
of the input's header: ASSD, HD95 and HD (``volume_surface.surface_distances``).  ``--edges SCAN`` prints, per interface between the classes just written,
the 10 % - 90 % width in those units and the contrast of ``SCAN``'s edge across it (``volume_sharpness.edge_sharpness``; ``SCAN`` has the
input's shape).  Exit code 0 / 1 (error logged), as ``scripts/reslice_volume.py``.
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

from mri_superresolution_amd.utils.nifti import frames, read_nifti      # noqa: E402
from mri_superresolution_amd.volume_eval import foreground_mask                      # noqa: E402
from mri_superresolution_amd.volume_tissue import TissueWorkspace, dice, label_confusion, segment_tissue      # noqa: E402
from mri_superresolution_amd.volume_surface import SurfaceWorkspace, surface_distances                      # noqa: E402
from mri_superresolution_amd.volume_sharpness import edge_sharpness                                         # noqa: E402
from scripts._cli import add_cpu_flag, join_frames, load_mask, run, save_nifti, to_device, voxel_sizes      # noqa: E402

logger = logging.getLogger("segment_volume")


def segment_file(input_path, output_path, classes=3, beta=1.0, iterations=20, mask="otsu", mask_close=0, mask_largest=False,
                 mask_fill_holes=None, compare=None, device="cuda", edges=None):
    """NIfTI file -> uint8 NIfTI label file; returns (the label array as written, the Dice per frame against ``compare`` or None)."""
    data, header = read_nifti(input_path)
    if mask != "otsu" and (mask_close != 0 or mask_largest or mask_fill_holes is not None):
        raise ValueError("--mask_close, --mask_largest and --mask_fill_holes go with --mask otsu")
    if not 0 <= mask_close <= 4:
        raise ValueError(f"--mask_close must be in 0..4, got {mask_close}")
    masks = load_mask(mask, data) if mask != "otsu" else None
    other = None
    if compare is not None:
        other = read_nifti(compare)[0]
        if other.shape != data.shape:
            raise ValueError(f"{compare} has the shape {tuple(other.shape)}, {input_path} {tuple(data.shape)}")
        if not np.array_equal(other, np.clip(np.rint(other), 0, 255)):
            raise ValueError(f"{compare} does not hold labels 0..255")
    scan = None
    if edges is not None:
        scan = read_nifti(edges)[0]
        if scan.shape != data.shape:
            raise ValueError(f"{edges} has the shape {tuple(scan.shape)}, {input_path} {tuple(data.shape)}")
    ws = TissueWorkspace(data.shape[:3], classes, device)
    surface_ws = SurfaceWorkspace(data.shape[:3], classes, device) if compare is not None else None
    outs, overlaps = [], []
    for t, frame in enumerate(frames(data)):
        vol = to_device(frame, device)
        m = foreground_mask(vol, mask_close, bool(mask_largest), mask_fill_holes)[0] if masks is None else torch.from_numpy(masks[t]).to(device)
        found = segment_tissue(vol, m, classes, beta, iterations, workspace=ws)
        what = f"{input_path}{f'[t={t}]' if data.ndim == 4 else ''}"
        logger.info(f"{what}: {int(found.counts.sum())} voxels in {classes} classes after {found.sweeps} sweep(s), {found.changed} label(s) "
                    f"changed in the last; means " + ", ".join(f"{x:.6g}" for x in found.means) + "; counts "
                    + ", ".join(str(int(c)) for c in found.counts) + (" (degenerate range: one bin)" if found.degenerate else ""))
        if other is not None:
            theirs = torch.from_numpy(np.ascontiguousarray(frames(other)[t]).astype(np.uint8)).to(device)
            overlaps.append(dice(label_confusion(found.labels, theirs, m, classes)))
            print(f"{what} Dice against {compare}: " + "  ".join(f"class {k + 1} {d:.6f}" for k, d in enumerate(overlaps[-1])))
            far = surface_distances(found.labels, theirs, classes, voxel_sizes(header.affine()), workspace=surface_ws)
            for name, values in (("ASSD", far.assd), ("HD95", far.hd95), ("HD", far.hd)):
                print(f"{what} {name} against {compare}: " + "  ".join(f"class {k + 1} {d:.6f}" for k, d in enumerate(values)))
        if scan is not None:
            theirs = to_device(frames(scan)[t], device)
            sharp = edge_sharpness(theirs, found.labels, classes, voxel_sizes(header.affine()))
            for name, values in (("edge width", sharp.width), ("edge contrast", sharp.contrast)):
                print(f"{what} {name} of {edges}: " + "  ".join(f"interface {k + 1} {d:.6f}" for k, d in enumerate(values)))
        outs.append(found.labels.cpu().numpy())
    result = join_frames(outs, data.ndim)
    save_nifti(output_path, result, header.copy())
    logger.info(f"Labels {tuple(result.shape)} saved to {output_path}")
    return result, (overlaps if other is not None else None)


def _body(args, device):
    fill = args.mask_fill_holes if args.mask_fill_holes in (None, "3d") else int(args.mask_fill_holes)
    segment_file(args.input, args.output, args.classes, args.beta, args.iterations, args.mask, args.mask_close, args.mask_largest, fill,
                 args.compare, device, args.edges)


def main(args):
    return run(_body, args, logger, "segmentation")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Segment a NIfTI volume into tissue classes (extension)")
    p.add_argument("--input", type=str, required=True, help="input scan: single-file NIfTI-1, .nii or .nii.gz, 3-D or 4-D")
    p.add_argument("--output", type=str, required=True, help="output labels, .nii or .nii.gz, uint8: 0 outside the mask, 1..K inside")
    p.add_argument("--classes", type=int, default=3, help="tissue classes K, 2..6; class 1 is the darkest")
    p.add_argument("--beta", type=float, default=1.0, help="strength of the Potts prior, 0..16 (0: every voxel on its own)")
    p.add_argument("--iterations", type=int, default=20, help="at most this many sweeps, 0..100 (0: the maximum-likelihood labels)")
    p.add_argument("--mask", type=str, default="otsu",
                   help="'otsu' (exact Otsu threshold of each frame, on the device) or a NIfTI-1 mask of the input's spatial shape "
                        "(non-zero = inside)")
    p.add_argument("--mask_close", type=int, default=0, help="close the Otsu mask with a box of this radius in voxels (0..4)")
    p.add_argument("--mask_largest", action="store_true", help="keep the largest 26-connected component of the Otsu mask")
    p.add_argument("--mask_fill_holes", type=str, choices=["3d", "0", "1", "2"], default=None,
                   help="fill the holes of the Otsu mask: those of the volume (3d) or of every plane across this axis")
    p.add_argument("--compare", type=str, default=None, help="print the Dice overlap per class with this label file (same shape)")
    p.add_argument("--edges", type=str, default=None,
                   help="print the 10 %% - 90 %% edge width and the contrast of this scan (same shape) across every interface of the labels")
    add_cpu_flag(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
