#!/usr/bin/env python3
"""Time of the device-side low-field simulation (csrc/lowfield.hip) for a batch of 16 slices at 256^2 and 512^2 HR.

    python tools/lowfield_bench.py [--batch 16] [--reps 50]

HIP events around every call (all three launches: extrema reset, pass 1, pass 2) after warm-up, seeded noise, inputs resident
in HBM; the median and the minimum over --reps calls in microseconds, and the median's share of the C2 train step
(profiles/r03_bench_c2.log: batch 16, 256^2 -> 512^2, ms_per_step).  Prints one JSON line (profiles/NOTES.md, "Low-field
simulation")."""
import argparse
import json
import os
import re
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    args = p.parse_args()
    from mri_superresolution_amd.utils.lowfield import simulate_low_field_u8
    step_ms = float(re.search(r'"ms_per_step": ([0-9.]+)', open(os.path.join(REPO, "profiles", "r03_bench_c2.log")).read()).group(1))
    res = {"gpu": torch.cuda.get_device_name(0), "batch": args.batch, "c2_step_ms": step_ms}
    for size in (256, 512):
        x = torch.randint(0, 256, (args.batch, size, size), dtype=torch.uint8, device="cuda")
        seeds = torch.arange(1, args.batch + 1, dtype=torch.int64, device="cuda")
        for _ in range(args.warmup):
            simulate_low_field_u8(x, 0.5, 5.0, seeds=seeds)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            simulate_low_field_u8(x, 0.5, 5.0, seeds=seeds)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        med = statistics.median(times)
        flop = args.batch * size * size * (4 * size + 8 * size)          # circulant form: 2 real FMAs per term, then 4
        res[f"hr{size}"] = {"us_median": round(med, 1), "us_min": round(min(times), 1), "tflops_fp32": round(flop / med * 1e-6, 2),
                            "share_of_c2_step": round(med * 1e-3 / step_ms, 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
