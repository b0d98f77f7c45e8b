#!/usr/bin/env python3
"""Cost of the volume noise kernel (csrc/volume_noise.hip) next to a copy of the same bytes and next to torch's own generator.

    python tools/lowfield_volume_bench.py [--sizes 256 512] [--reps 5] [--warmup 2] [--inner 3]

Per size n, on an n^3 float32 volume, HIP events, the median of ``--reps`` alternating rounds (smallest and largest next to it):
(a) ``volume_lowfield.add_noise`` (Rician, seeded) into a second volume, and the Gaussian mode, which draws one normal per voxel
    instead of two;
(b) a device copy of the same bytes - the volume read once and written once;
(c) ``torch.randn`` twice plus ``torch.hypot``: the same noise model from torch's generator, three kernels and two temporaries.
At 256^3 the 134 MB of source and result fit the last-level cache: only the 512^3 figure is an HBM rate.  Prints one JSON line
(README.md, "Simulated low-field volumes")."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.benchutil import alternating_times      # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--inner", type=int, default=3)
    p.add_argument("--sigma", type=float, default=20.0)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lowfield_volume_bench needs the MI355X: there is nothing to time on a CPU")
    from mri_superresolution_amd.volume_lowfield import add_noise

    dev = torch.device("cuda")
    res = {"gpu": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, "sigma": args.sigma, "sizes": {}}
    for n in args.sizes:
        g = torch.Generator(device="cuda").manual_seed(0)
        vol = torch.rand((n, n, n), device=dev, generator=g) * 4095.0
        out = torch.empty_like(vol)
        sigma = args.sigma

        def by_torch():
            re = torch.randn(vol.shape, device=dev, generator=g).mul_(sigma).add_(vol)
            return torch.hypot(re, torch.randn(vol.shape, device=dev, generator=g).mul_(sigma), out=out)

        fns = {"add_noise": lambda: add_noise(vol, sigma, 1, out=out), "add_noise_gaussian": lambda: add_noise(vol, sigma, 1, rician=False, out=out),
               "copy": lambda: out.copy_(vol), "torch_randn_hypot": by_torch}
        times = alternating_times(fns, args.reps, args.warmup, args.inner)
        t = {k: v["us_median"] for k, v in times.items()}
        nbytes = 8 * vol.numel()
        res["sizes"][str(n)] = {"MB": round(nbytes / 1e6, 1), "times": times,
                                "add_noise_TBps": round(nbytes / (t["add_noise"] * 1e-6) / 1e12, 3),
                                "copy_TBps": round(nbytes / (t["copy"] * 1e-6) / 1e12, 3),
                                "share_of_copy_rate": round(t["copy"] / t["add_noise"], 3),
                                "gaussian_share_of_copy_rate": round(t["copy"] / t["add_noise_gaussian"], 3),
                                "torch_over_add_noise": round(t["torch_randn_hypot"] / t["add_noise"], 2)}
        del vol, out
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
