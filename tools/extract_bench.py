#!/usr/bin/env python3
"""Time of the device-side paired-slice extraction (utils/extraction.py:extract_pairs) per stage, against the NumPy chain.

    python tools/extract_bench.py [--reps 20] [--host_slices 4]

A synthetic 256 x 256 x 160 float volume (values like a 12-bit scan) with EVERY slice selected, target 256 x 256: HIP events
around each stage after warm-up - window (exact percentiles + normalise), resample HR (LANCZOS4 letter-box, uint8), simulate
(float low-field simulation, seeded noise), resample LR (AREA letter-box to half, uint8) - and around the whole
``extract_pairs`` call; medians in microseconds.  The host figure is ``extract_pairs_host`` on --host_slices slices, scaled
to 160.  Prints one JSON line (profiles/NOTES.md, "Paired-slice extraction")."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(times), 1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--host_slices", type=int, default=4)
    args = p.parse_args()
    from mri_superresolution_amd.utils import extraction as E
    from mri_superresolution_amd.utils import imageops, lowfield
    x, y, z = 256, 256, 160
    rng = np.random.default_rng(0)
    xx, yy, zz = np.mgrid[0:x, 0:y, 0:z]
    vol = (1800 * np.clip(1.2 - np.hypot((xx - x / 2) / (0.45 * x), (yy - y / 2) / (0.45 * y)), 0, 1)
           * (1 + 0.3 * np.sin(xx / 9.0 + zz / 5.0) * np.cos(yy / 11.0)) + rng.normal(60, 25, (x, y, z))).clip(0, 4095).astype(np.float32)
    dev = torch.from_numpy(vol).cuda()
    sel = dict(n_slices=z, lower_percent=0.0, upper_percent=(z - 1) / z + 1e-9, target_size=(256, 256))
    slices = dev.permute(2, 0, 1).contiguous()
    seeds = torch.arange(1, z + 1, dtype=torch.int64, device="cuda")
    norm = imageops.normalise_percentile_f32(slices)[:, 0]
    sim = lowfield.simulate_low_field_f32(norm, 0.5, 5.0, seeds=seeds)
    res = {"gpu": torch.cuda.get_device_name(0), "volume": [x, y, z], "slices": z, "target": [256, 256],
           "window_us": timed(lambda: imageops.normalise_percentile_f32(slices), args.reps, args.warmup),
           "resample_hr_us": timed(lambda: E.resample_letterbox_f32(norm, (256, 256), E.LANCZOS4, as_uint8=True), args.reps, args.warmup),
           "simulate_us": timed(lambda: lowfield.simulate_low_field_f32(norm, 0.5, 5.0, seeds=seeds), args.reps, args.warmup),
           "resample_lr_us": timed(lambda: E.resample_letterbox_f32(sim, (128, 128), E.AREA, as_uint8=True), args.reps, args.warmup),
           "extract_pairs_us": timed(lambda: E.extract_pairs(dev, seeds=seeds, **sel), args.reps, args.warmup)}
    t0 = time.perf_counter()
    E.extract_pairs_host(vol[:, :, :args.host_slices], args.host_slices, 0.0, (args.host_slices - 1) / args.host_slices + 1e-9,
                         (256, 256), rng=np.random.default_rng(1))
    res["host_us_scaled_to_all_slices"] = round((time.perf_counter() - t0) * 1e6 * z / args.host_slices, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
