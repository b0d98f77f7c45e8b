#!/usr/bin/env python3
"""Writes tests/golden/extraction.npz by calling the REFERENCE's own ``utils/extraction_utils.py:extract_slices_3d``.

    python tools/gen_extraction_golden.py --reference /path/to/reference/checkout

The reference modules are imported at generation time only, with a RECORDING ``cv2`` stub: the ``INTER_*`` constants are
0..4, ``resize`` stores its input array, ``dsize`` and interpolation and returns zeros of ``dsize``, ``imwrite`` stores the path.
The reference script ``scripts/extract_paired_slices.py`` is imported the same way with an empty ``nibabel`` stub (it only loads
files with it), and ITS ``preprocess_high_res_slice`` is the function handed to ``extract_slices_3d``, as in the reference's run.
``np.random.seed(s)`` followed by two ``np.random.normal`` draws per slice replays the k-space noise the run draws after the
same seed.  The fixture therefore pins everything in the chain except ``cv2.resize`` itself: per slice the two arrays the
reference handed to ``cv2.resize``, their ``dsize`` and interpolation, the file names and the replayed noise; plus a few
``generate_bids_identifier`` input / output strings.

Volumes (values like a 12-bit scan): A 31 x 45 x 12 to target (64, 48) - an enlarging letter-box, slice 0 constant and outside
the selected range; B 70 x 50 x 6 to target (32, 32) - a reducing one.  ``n_slices`` = 4, noise_std 5, crop factor 0.5.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"a": ((31, 45, 12), (64, 48), 4100), "b": ((70, 50, 6), (32, 32), 4200)}
N_SLICES, LOWER, UPPER, CROP, NOISE_STD = 4, 0.2, 0.8, 0.5, 5.0
BIDS_NAMES = ["/data/set1/sub-01/anat/sub-01_T1w.nii.gz", "sub-02_ses-1_acq-MPRAGE_T1w.nii.gz", "sub-03_ses-2_run-1_bold.nii",
              "sub-A7_task-rest_BOLD.nii.gz", "scan_0007.nii.gz", "plainname.nii", "sub-11_FLAIR.nii", "sub-12_acq-hi_res.nii.gz",
              "dir.with-dash/volume.nii.gz"]


def volume(rng, shape):
    x, y, z = shape
    xx, yy, zz = np.mgrid[0:x, 0:y, 0:z]
    r = np.sqrt(((xx - x / 2) / (0.45 * x)) ** 2 + ((yy - y / 2) / (0.45 * y)) ** 2)
    v = 1800 * np.clip(1.2 - r, 0, 1) * (1 + 0.3 * np.sin(xx / 3.1 + zz) * np.cos(yy / 4.3)) + rng.normal(60, 25, shape)
    v = np.clip(v, 0, 4095)
    v[:, :, 0] = 517.0           # a constant slice, outside the selected range
    return v.astype(np.float64)  # nibabel's get_fdata() returns float64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "extraction.npz"))
    args = ap.parse_args()

    calls = {"resize": [], "imwrite": []}
    stub = types.ModuleType("cv2")
    stub.INTER_NEAREST, stub.INTER_LINEAR, stub.INTER_CUBIC, stub.INTER_AREA, stub.INTER_LANCZOS4 = 0, 1, 2, 3, 4

    def resize(src, dsize, interpolation=1):
        calls["resize"].append((np.array(src, copy=True), tuple(int(v) for v in dsize), int(interpolation)))
        return np.zeros((dsize[1], dsize[0]), dtype=src.dtype)

    def imwrite(path, img):
        calls["imwrite"].append((str(path), tuple(img.shape), str(img.dtype)))
        return True

    stub.resize, stub.imwrite = resize, imwrite
    sys.modules["cv2"] = stub
    sys.path.insert(0, os.path.abspath(args.reference))
    sys.modules["nibabel"] = types.ModuleType("nibabel")       # the script imports it at the top and uses it only to load files
    from utils import extraction_utils as ref_ex
    spec = importlib.util.spec_from_file_location("ref_extract_script", os.path.join(args.reference, "scripts", "extract_paired_slices.py"))
    ref_script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_script)
    preprocess = ref_script.preprocess_high_res_slice            # the reference script's own per-slice function

    out = {"crop_factor": np.float64(CROP), "noise_std": np.float64(NOISE_STD), "n_slices": np.int64(N_SLICES),
           "lower_percent": np.float64(LOWER), "upper_percent": np.float64(UPPER),
           "bids_in": np.array(BIDS_NAMES), "bids_out": np.array([ref_ex.generate_bids_identifier(n) for n in BIDS_NAMES])}
    rng = np.random.default_rng(20308)
    for name, (shape, target, seed) in CASES.items():
        vol = volume(rng, shape)
        timepoint = None if name == "a" else 1
        calls["resize"].clear(), calls["imwrite"].clear()
        np.random.seed(seed)
        ref_ex.extract_slices_3d(vol, "sub-01_T1w", "HR", "LR", timepoint=timepoint, n_slices=N_SLICES, lower_percent=LOWER,
                                 upper_percent=UPPER, target_size=target, preprocess_function=preprocess,
                                 apply_simulation=True, noise_std=NOISE_STD, kspace_crop_factor=CROP)
        assert len(calls["resize"]) == 2 * N_SLICES and len(calls["imwrite"]) == 2 * N_SLICES
        # the replay: the run draws noise_real, then noise_imag, once per slice, and nothing else
        np.random.seed(seed)
        scaled = (NOISE_STD / 255.0) * np.sqrt(shape[0] * shape[1]) / 10
        noise = np.stack([np.stack([np.random.normal(0, scaled, shape[:2]), np.random.normal(0, scaled, shape[:2])])
                          for _ in range(N_SLICES)])
        hr, lr = calls["resize"][0::2], calls["resize"][1::2]
        names = [os.path.basename(p) for p, _, _ in calls["imwrite"][0::2]]
        assert names == [os.path.basename(p) for p, _, _ in calls["imwrite"][1::2]]
        out[name + "_volume"] = vol.astype(np.float32)       # exact: the values are float32 after the slice's astype
        assert np.array_equal(out[name + "_volume"].astype(np.float32), vol.astype(np.float32))
        out[name + "_target"] = np.array(target, dtype=np.int64)
        out[name + "_timepoint"] = np.int64(-1 if timepoint is None else timepoint)
        out[name + "_indices"] = np.array([int(n.rsplit("_s", 1)[1][:3]) for n in names], dtype=np.int64)
        out[name + "_names"] = np.array(names)
        out[name + "_noise"] = noise
        out[name + "_hr_plane"] = np.stack([a for a, _, _ in hr])
        out[name + "_lr_plane"] = np.stack([a for a, _, _ in lr])
        out[name + "_hr_dsize"] = np.array([d for _, d, _ in hr], dtype=np.int64)
        out[name + "_lr_dsize"] = np.array([d for _, d, _ in lr], dtype=np.int64)
        out[name + "_hr_interpolation"] = np.array([i for _, _, i in hr], dtype=np.int64)
        out[name + "_lr_interpolation"] = np.array([i for _, _, i in lr], dtype=np.int64)
        out[name + "_image_shapes"] = np.array([s for _, s, _ in calls["imwrite"]], dtype=np.int64)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
