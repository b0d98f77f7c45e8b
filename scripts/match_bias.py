#!/usr/bin/env python3
"""Take the slowly varying gain (bias field) out of a NIfTI scan on the device (extension).

    python scripts/match_bias.py --input lowfield.nii.gz --like reference.nii.gz --output matched.nii.gz
    python scripts/match_bias.py --input scan.nii.gz --output corrected.nii.gz --sigma_mm 30 --save_field field.nii.gz

B1 / coil sensitivity multiplies a scan by a smooth field that differs between scanners and sessions and that no global intensity
map can remove.  With ``--like`` the input is multiplied by the ratio of the two scans' masked Gaussian low-passes (differential
bias correction): the input then carries the field of ``--like``.  The two scans must share a grid - bring them onto one with
``scripts/reslice_volume.py`` or ``scripts/register_volume.py`` first.  Without ``--like`` the input is divided by its own low-pass
over the median of that low-pass inside the mask (homomorphic unsharp masking).  ``--sigma_mm`` is the Gaussian's sigma in
millimetres, turned into voxels per axis through the input header's voxel sizes (at most 128 taps either side); the field is clamped
to ``[1 / limit, limit]``.  ``--mask`` (the input's) and ``--like_mask``: ``otsu`` (default; ``volume_eval.foreground_mask`` of each
scan on its own, no closing) or a NIfTI-1 file of the scan's spatial shape (non-zero = foreground); the pair form smooths inside
the intersection of the two.  A 4-D input is processed frame by frame; a 3-D ``--like`` (or mask) serves every frame.  The output
keeps the input's header, as float32; ``--save_field`` writes the field the same way.  Equal to ``volume_bias.match_bias_np`` /
``correct_bias_np`` bit for bit (``csrc/volume_bias.hip``).  Exit code 0 / 1 (error logged), as ``scripts/reslice_volume.py``.
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

from mri_superresolution_amd.utils.nifti import frames as frames_of, mask_frames, read_nifti      # noqa: E402
from mri_superresolution_amd.volume_bias import BiasWorkspace, correct_bias, match_bias, sigmas_for           # noqa: E402
from mri_superresolution_amd.volume_eval import foreground_mask                                                # noqa: E402
from scripts._cli import add_cpu_flag, frame_tag, join_frames, run, save_nifti, to_device      # noqa: E402

logger = logging.getLogger("match_bias")


def _mask_frames(spec, data, count, what):
    """-> ``count`` entries: ``"otsu"`` or a uint8 array of the scan's spatial shape."""
    if spec == "otsu":
        return ["otsu"] * count
    return mask_frames(spec, data.shape[:3], count, what)[0]


def _on_device(frame, mask, device):
    vol = to_device(frame, device)
    return vol, (foreground_mask(vol)[0] if isinstance(mask, str) else torch.from_numpy(mask).to(device))


def match_file(input_path, output_path, like_path=None, sigma_mm=25.0, limit=4.0, mask="otsu", like_mask="otsu", save_field=None,
               device="cuda"):
    """NIfTI file -> NIfTI file without the input's bias field (``like_path`` None) or with that of ``like_path``; returns (the
    output array as written, the field as an array of the same shape)."""
    data, header = read_nifti(input_path)
    frames = frames_of(data)
    sigmas = sigmas_for(header.affine(), sigma_mm)
    like_frames = like_masks = None
    if like_path is not None:
        like, like_header = read_nifti(like_path)
        if tuple(like.shape[:3]) != tuple(data.shape[:3]) or not np.allclose(like_header.affine(), header.affine(), rtol=0, atol=1e-3):
            raise ValueError(f"{like_path} {tuple(like.shape[:3])} and {input_path} {tuple(data.shape[:3])} do not share a grid (shape and "
                             "affine): bring one onto the other's with scripts/reslice_volume.py or scripts/register_volume.py first")
        like_frames = frames_of(like)
        if len(like_frames) not in (1, len(frames)):
            raise ValueError(f"{like_path} has {len(like_frames)} timepoints, {input_path} has {len(frames)}")
        like_masks = _mask_frames(like_mask, like, len(like_frames), "--like_mask")
    masks = _mask_frames(mask, data, len(frames), "--mask")
    ws = BiasWorkspace(data.shape[:3], sigmas, device)
    logger.info(f"sigma {sigma_mm:g} mm = ({sigmas[0]:.3f}, {sigmas[1]:.3f}, {sigmas[2]:.3f}) voxels, radii {ws.radii}, limit {limit:g}")
    outs, fields = [], []
    target = None
    for t, frame in enumerate(frames):
        src, smask = _on_device(frame, masks[t], device)
        if like_frames is None:
            out, field = correct_bias(src, smask, sigmas, limit, ws)
        else:
            if t == 0 or len(like_frames) > 1:                       # a 3-D --like is uploaded (and masked) once
                target = _on_device(like_frames[t], like_masks[t], device)
            out, field = match_bias(src, target[0], smask, target[1], sigmas, limit, ws)
        lo, hi = torch.aminmax(field)
        logger.info(f"{frame_tag(t, len(frames))}field in [{float(lo):.4f}, {float(hi):.4f}]")
        outs.append(out.cpu().numpy())
        fields.append(field.cpu().numpy())
    result, field = join_frames(outs, data.ndim), join_frames(fields, data.ndim)
    save_nifti(output_path, result, header)
    if save_field:
        save_nifti(save_field, field, header)
        logger.info(f"Saved the field to {save_field}")
    logger.info(f"Corrected volume {tuple(data.shape)} saved to {output_path}")
    return result, field


def _body(args, device):
    if args.like is None and args.like_mask != "otsu":
        raise ValueError("--like_mask goes with --like")
    match_file(args.input, args.output, args.like, args.sigma_mm, args.limit, args.mask, args.like_mask, args.save_field, device)


def main(args):
    return run(_body, args, logger, "bias-field matching")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Remove or match the bias field of a NIfTI volume (extension)")
    p.add_argument("--input", type=str, required=True, help="input scan: single-file NIfTI-1, .nii or .nii.gz, 3-D or 4-D")
    p.add_argument("--output", type=str, required=True, help="output scan, .nii or .nii.gz, float32, the input's header")
    p.add_argument("--like", type=str, default=None, help="the scan whose field is taken (same grid); default: the input's own field is removed")
    p.add_argument("--sigma_mm", type=float, default=25.0, help="sigma of the Gaussian low-pass in millimetres")
    p.add_argument("--limit", type=float, default=4.0, help="the field is clamped to [1 / limit, limit]")
    p.add_argument("--mask", type=str, default="otsu", help="foreground of the input: otsu (default) or a NIfTI-1 mask")
    p.add_argument("--like_mask", type=str, default="otsu", help="foreground of --like: otsu (default) or a NIfTI-1 mask")
    p.add_argument("--save_field", type=str, default=None, help="write the field as a float32 NIfTI with the input's header")
    add_cpu_flag(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
