#!/usr/bin/env python3
"""Writes tests/golden/lowfield.npz by calling the REFERENCE's own ``utils/preprocessing.py:simulate_low_field_mri``.

    python tools/gen_lowfield_golden.py --reference /path/to/reference/checkout

The reference module is imported at generation time only (its ``import cv2`` is satisfied by a stub module without functions: the
simulation itself is NumPy).  ``np.random.seed(s)`` followed by two ``np.random.normal(0, scaled_std, shape)`` draws
replays the noise the function draws after the same seed; the fixture stores those two k-space arrays, the uint8 input and
the function's float64 output (before the clip).  Cases: 32x32, 48x40, 30x44, each with noise_std 0 and 5.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, 32), (48, 40), (30, 44)]
CROP = 0.5


def image(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    a = 120 + 80 * np.sin(yy / 4.0) * np.cos(xx / 3.0) + rng.normal(0, 15, (h, w))
    return np.clip(a, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "lowfield.npz"))
    args = ap.parse_args()
    if "cv2" not in sys.modules:
        stub = types.ModuleType("cv2")


        def constant(name):       # the module reads cv2.INTER_* constants into enums at import; nothing is called
            if name.startswith("__"):
                raise AttributeError(name)
            return 0

        stub.__getattr__ = constant
        sys.modules["cv2"] = stub
    spec = importlib.util.spec_from_file_location("ref_preprocessing", os.path.join(args.reference, "utils", "preprocessing.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    rng = np.random.default_rng(20240)
    out = {"crop_factor": np.float64(CROP)}
    for ci, (h, w) in enumerate(SHAPES):
        u8 = image(rng, h, w)
        data = u8.astype(np.float64) / 255.0
        for noise_std in (0.0, 5.0):
            seed = 1000 + ci
            scaled = (noise_std / 255.0) * np.sqrt(h * w) / 10
            np.random.seed(seed)
            n_re = np.random.normal(0, scaled, (h, w))
            n_im = np.random.normal(0, scaled, (h, w))
            np.random.seed(seed)
            sim = ref.simulate_low_field_mri(data, kspace_crop_factor=CROP, noise_std=noise_std)
            key = f"{h}x{w}_n{int(noise_std)}"
            out[key + "_image"] = u8
            out[key + "_noise_re"] = n_re
            out[key + "_noise_im"] = n_im
            out[key + "_simulated"] = np.asarray(sim, dtype=np.float64)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {sorted(k for k in out if k.endswith('_simulated'))}")


if __name__ == "__main__":
    main()
