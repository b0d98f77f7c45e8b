#!/usr/bin/env python3
"""Extracts paired high-resolution / simulated low-resolution PNG slices from NIfTI scans on the device (extension; the
reference's ``scripts/extract_paired_slices.py``, same flags and defaults plus ``--seed``).

    python scripts/extract_paired_slices.py --datasets_dir ./datasets --hr_output_dir ./training_data
                                            --lr_output_dir ./training_data_1.5T [--n_slices 10] [--target_size 256 256] ...

Every ``*.nii`` / ``*.nii.gz`` file in a directory named ``anat`` below ``datasets_dir/<set>/`` (sorted order) is read with
``utils/nifti.read_nifti``; a 3-D scan, or every timepoint of a 4-D scan, goes through
``mri_superresolution_amd/utils/extraction.py:extract_pairs`` and its slices are written as same-named 8-bit grayscale PNGs
into the two output directories: valid ``--full_res_dir`` / ``--low_res_dir`` input of ``scripts/train.py``.  The noise of the
k-th pair written comes from ``derive_seeds(seed, None, [k])``.  A scan that fails is reported and skipped.  There is no CPU path.
"""
import argparse
import os
import pathlib
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="NIfTI scans -> paired HR / simulated-LR 8-bit PNG slices, computed on the device")
    p.add_argument("--datasets_dir", type=str, default="./datasets", help="root that holds one folder per dataset; scans are looked for in its anat/ folders")
    p.add_argument("--hr_output_dir", type=str, default="./training_data", help="where the HR PNGs go (train.py --full_res_dir)")
    p.add_argument("--lr_output_dir", type=str, default="./training_data_1.5T", help="where the same-named LR PNGs go (train.py --low_res_dir)")
    p.add_argument("--n_slices", type=int, default=10, help="slices taken from every volume, equally spaced")
    p.add_argument("--lower_percent", type=float, default=0.2, help="first slice, as a fraction of the slice count")
    p.add_argument("--upper_percent", type=float, default=0.8, help="last slice, as a fraction of the slice count")
    p.add_argument("--target_size", type=int, nargs=2, default=[256, 256], metavar=("W", "H"), help="HR canvas; LR is half of it")
    p.add_argument("--noise_std", type=float, default=5, help="noise level of the simulation on the 0..255 scale")
    p.add_argument("--kspace_crop_factor", type=float, default=0.5, help="share of k-space kept along each axis")
    p.add_argument("--seed", type=int, default=0, help="(extension) seed of the simulated noise")
    return p.parse_args(argv)


def find_scans(datasets_dir):
    """Sorted paths of the ``.nii`` / ``.nii.gz`` files whose folder is called ``anat`` (any letter case), anywhere below a
    dataset folder of ``datasets_dir``; files lying directly in ``datasets_dir`` are not looked at."""
    root = pathlib.Path(datasets_dir)
    scans = []
    for dataset in sorted(d for d in root.iterdir() if d.is_dir()):
        scans += sorted(str(f) for f in dataset.rglob("*")
                        if f.is_file() and f.parent.name.lower() == "anat" and f.name.endswith((".nii", ".nii.gz")))
    return scans


def main(argv=None):
    args = parse_args(argv)
    from PIL import Image
    from mri_superresolution_amd.utils.extraction import bids_identifier, extract_pairs, pair_filename
    from mri_superresolution_amd.utils.lowfield import derive_seeds
    from mri_superresolution_amd.utils.nifti import read_nifti
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only (hand-written HIP kernels, no CPU fallback)")
    os.makedirs(args.hr_output_dir, exist_ok=True)
    os.makedirs(args.lr_output_dir, exist_ok=True)
    written = 0
    for path in find_scans(args.datasets_dir):
        print(f"reading {path}")
        try:
            data, _ = read_nifti(path)
            subject = bids_identifier(path)
            frames = [(None, data)] if data.ndim == 3 else [(t, data[..., t]) for t in range(data.shape[3])]
            for timepoint, frame in frames:
                vol = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float32)).cuda()
                seeds = derive_seeds(args.seed, None, range(written, written + args.n_slices))
                idx, hr, lr = extract_pairs(vol, args.n_slices, args.lower_percent, args.upper_percent, tuple(args.target_size),
                                            args.kspace_crop_factor, args.noise_std, seeds=seeds)
                hr, lr = hr.cpu().numpy(), lr.cpu().numpy()
                for k, i in enumerate(idx):
                    name = pair_filename(subject, int(i), timepoint)
                    Image.fromarray(hr[k]).save(os.path.join(args.hr_output_dir, name))
                    Image.fromarray(lr[k]).save(os.path.join(args.lr_output_dir, name))
                written += len(idx)
        except Exception as e:
            print(f"skipped {path}: {type(e).__name__}: {e}")
    print(f"wrote {written} slice pairs to {args.hr_output_dir} and {args.lr_output_dir}")


if __name__ == "__main__":
    main()
