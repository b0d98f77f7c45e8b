#!/usr/bin/env python3
"""Bring a NIfTI scan onto another scan's intensity scale on the device (extension).

    python scripts/match_intensity.py --input lowfield.nii.gz --like reference.nii.gz --output matched.nii.gz
    python scripts/match_intensity.py --input a.nii.gz --like b.nii.gz --output c.nii.gz --mode range --mask none --like_mask brain.nii.gz

MR intensities are in arbitrary units: two scanners or two sessions differ by a scale, an offset and usually a monotone contrast
curve.  ``--mode landmarks`` (Nyul-Udupa) takes the percentiles 1, 10, 20, ..., 90, 99 of each scan's foreground and maps the
input through the piecewise-linear function that sends its landmarks onto those of ``--like``; ``--mode range`` uses the
percentiles 1 and 99 alone (one linear map); ``--percentiles P ...`` gives 2..16 of them.  Below the first and above the last
landmark the first and the last segment extend linearly.  The two scans need not share a grid: only their histograms meet.
``--mask`` (the input's) and ``--like_mask``: ``otsu`` (default; ``volume_eval.foreground_mask`` of each scan on its own, no
closing), ``none`` (every voxel) or a NIfTI-1 file of that scan's spatial shape (non-zero = foreground).  A 4-D input is matched
frame by frame; a 3-D ``--like`` (or mask) serves every frame, a 4-D one must have as many frames.  The output keeps the input's
header, as float32.  ``--save_landmarks F.txt``: three text columns - percentile, source landmark, target landmark - one block per
frame.  The percentiles are selected exactly on the device (``csrc/volume_intensity.hip``, equal to
``volume_intensity.match_intensity_np``).  Exit code 0 / 1 (error logged), as ``scripts/reslice_volume.py``.
"""
import argparse
import logging
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from mri_superresolution_amd.utils.nifti import frames as frames_of, mask_frames, read_nifti      # noqa: E402
from mri_superresolution_amd.volume_eval import foreground_mask                                  # noqa: E402
from mri_superresolution_amd.volume_intensity import LANDMARKS, RANGE, match_intensity          # noqa: E402
from scripts._cli import add_cpu_flag, frame_tag, join_frames, make_parent, run, save_nifti, to_device    # noqa: E402

logger = logging.getLogger("match_intensity")
MODES = {"landmarks": LANDMARKS, "range": RANGE}


def _mask_frames(spec, data, count, what):
    """-> ``count`` entries: ``"otsu"``, None, or a uint8 array of the scan's spatial shape."""
    if spec == "otsu":
        return ["otsu"] * count
    if spec == "none":
        return [None] * count
    return mask_frames(spec, data.shape[:3], count, what)[0]


def _on_device(frame, mask, device):
    vol = to_device(frame, device)
    if isinstance(mask, str):
        return vol, foreground_mask(vol)[0]
    return vol, (None if mask is None else torch.from_numpy(mask).to(device))


def format_landmarks(found):
    return "  ".join(f"{q:g}%: {s:.6g} -> {t:.6g}" for q, s, t in zip(found.percentiles, found.source_landmarks, found.target_landmarks))


def match_file(input_path, like_path, output_path, percentiles=LANDMARKS, mask="otsu", like_mask="otsu", save_landmarks=None, device="cuda"):
    """NIfTI file -> NIfTI file on the intensity scale of ``like_path``; returns (the output array as written, one
    ``IntensityMatch`` per frame)."""
    data, header = read_nifti(input_path)
    like = read_nifti(like_path)[0]
    frames, like_frames = frames_of(data), frames_of(like)
    if len(like_frames) not in (1, len(frames)):
        raise ValueError(f"{like_path} has {len(like_frames)} timepoints, {input_path} has {len(frames)}")
    masks = _mask_frames(mask, data, len(frames), "--mask")
    like_masks = _mask_frames(like_mask, like, len(like_frames), "--like_mask")
    outs, founds = [], []
    target = None
    for t, frame in enumerate(frames):
        src, smask = _on_device(frame, masks[t], device)
        if t == 0 or len(like_frames) > 1:                       # a 3-D --like is uploaded (and masked) once
            target = _on_device(like_frames[t], like_masks[t], device)
        out, found = match_intensity(src, target[0], smask, target[1], percentiles)
        logger.info(f"{frame_tag(t, len(frames))}{found.source_count} source and {found.target_count} target "
                    f"voxels; landmarks {format_landmarks(found)}")
        outs.append(out.cpu().numpy())
        founds.append(found)
    result = join_frames(outs, data.ndim)
    save_nifti(output_path, result, header)
    if save_landmarks:
        make_parent(save_landmarks)
        with open(save_landmarks, "w") as f:
            for t, found in enumerate(founds):
                f.write(f"# frame {t}: percentile, source landmark, target landmark ({found.source_count} / {found.target_count} voxels)\n")
                for q, s, d in zip(found.percentiles, found.source_landmarks, found.target_landmarks):
                    f.write(f"{q:.17g} {float(s):.9g} {float(d):.9g}\n")
        logger.info(f"Saved the landmarks to {save_landmarks}")
    logger.info(f"Matched volume {tuple(data.shape)} saved to {output_path}")
    return result, founds


def _body(args, device):
    if args.percentiles is not None and args.mode is not None:
        raise ValueError("--percentiles goes without --mode")
    percentiles = tuple(args.percentiles) if args.percentiles is not None else MODES[args.mode or "landmarks"]
    match_file(args.input, args.like, args.output, percentiles, args.mask, args.like_mask, args.save_landmarks, device)


def main(args):
    return run(_body, args, logger, "intensity matching")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Map a NIfTI volume onto another volume's intensity scale (extension)")
    p.add_argument("--input", type=str, required=True, help="input scan: single-file NIfTI-1, .nii or .nii.gz, 3-D or 4-D")
    p.add_argument("--like", type=str, required=True, help="the scan whose intensity scale is taken (any grid)")
    p.add_argument("--output", type=str, required=True, help="output scan, .nii or .nii.gz, float32, the input's header")
    p.add_argument("--mode", type=str, choices=sorted(MODES), default=None,
                   help="landmarks (default): percentiles 1, 10, ..., 90, 99 (Nyul-Udupa); range: percentiles 1 and 99")
    p.add_argument("--percentiles", type=float, nargs="+", default=None, help="2..16 non-decreasing percentiles instead of a --mode")
    p.add_argument("--mask", type=str, default="otsu", help="foreground of the input: otsu (default), none, or a NIfTI-1 mask")
    p.add_argument("--like_mask", type=str, default="otsu", help="foreground of --like: otsu (default), none, or a NIfTI-1 mask")
    p.add_argument("--save_landmarks", type=str, default=None, help="write percentile, source landmark, target landmark as text")
    add_cpu_flag(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
