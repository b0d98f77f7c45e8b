#!/usr/bin/env python3
"""Writes the low-resolution directory of a high-resolution one through the device-side low-field simulation (extension).

    python scripts/simulate_lr.py --full_res_dir HR --low_res_dir LR [--kspace_crop_factor 0.5] [--noise_std 5]
                                  [--seed 0] [--batch_size 16]

Every 8-bit grayscale PNG of ``--full_res_dir`` (even height and width) gets a same-named PNG of half the size in
``--low_res_dir``: k-space crop, complex Gaussian noise, magnitude, renormalisation, 2x2 mean, uint8
(``mri_superresolution_amd/utils/lowfield.py``; the reference's ``simulate_low_field_mri`` + ``extract_slices`` steps).  The
noise of file number i (sorted names) comes from ``derive_seeds(seed, None, [i])``, whatever the batch size.  The two
directories are valid ``--full_res_dir`` / ``--low_res_dir`` input of ``scripts/train.py`` here and in the reference.
There is no CPU path.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Simulate low-field low-resolution slices from high-resolution ones on the device")
    p.add_argument("--full_res_dir", type=str, required=True, help="Directory of high-resolution PNG slices (input)")
    p.add_argument("--low_res_dir", type=str, required=True, help="Directory the low-resolution PNG slices are written to")
    p.add_argument("--kspace_crop_factor", type=float, default=0.5)
    p.add_argument("--noise_std", type=float, default=5.0)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--batch_size", type=int, default=16)
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    from PIL import Image
    from mri_superresolution_amd.utils.lowfield import derive_seeds, simulate_low_field_u8
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only (hand-written HIP kernels, no CPU fallback)")
    names = sorted(f for f in os.listdir(args.full_res_dir) if f.lower().endswith(".png"))
    if not names:
        raise SystemExit(f"no PNG files in {args.full_res_dir}")
    os.makedirs(args.low_res_dir, exist_ok=True)
    images = [np.asarray(Image.open(os.path.join(args.full_res_dir, n)).convert("L"), dtype=np.uint8) for n in names]
    # batches of equally sized images, in file order
    start = 0
    while start < len(names):
        stop = start + 1
        while stop < len(names) and stop - start < args.batch_size and images[stop].shape == images[start].shape:
            stop += 1
        high = torch.from_numpy(np.stack(images[start:stop])).cuda()
        low = simulate_low_field_u8(high, args.kspace_crop_factor, args.noise_std,
                                    seeds=derive_seeds(args.seed, None, range(start, stop))).cpu().numpy()
        for k in range(start, stop):
            Image.fromarray(low[k - start]).save(os.path.join(args.low_res_dir, names[k]))
        start = stop
    print(f"wrote {len(names)} low-resolution slices to {args.low_res_dir}")


if __name__ == "__main__":
    main()
