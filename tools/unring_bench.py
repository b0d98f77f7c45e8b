#!/usr/bin/env python3
"""Cost of the unring kernel (csrc/volume_unring.hip) next to the same operator written with torch, a zero-filling pass of the same
extent, and a copy.

    python tools/unring_bench.py [--size 256] [--shifts 20] [--reps 5] [--warmup 2] [--inner 2]

(a) ``unring_axis`` of a size^3 float32 volume along each axis (one launch each) and ``unring`` over all three (the k-space split by
    ``torch.fft`` plus three launches), HIP events, the median of ``--reps`` alternating rounds;
(b) the one-axis operator written with torch on the device: per shift an ``rfft`` phase ramp and ``irfft`` along the axis (the
    spectrum is taken once), the differences, the windowed sums by ``roll`` and the two selects by ``where`` - 2K passes over the
    volume; the largest absolute difference to the kernel's result is printed next to the data range (the two differ in rounding,
    and where two variations are closer than that, in the shift taken);
(c) one ``zerofill2`` pass along axis 0 of the same volume: the kernel is expected at roughly K times this (2K circulant sums of n
    terms per sample against 2);
(d) a device copy of the ALGORITHMIC bytes of one axis - the volume read once, written once.
Prints one JSON line (README.md, "Gibbs-ringing removal")."""
import argparse
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.benchutil import alternating_times      # noqa: E402


def make_torch_unring(n, axis, K, window, device):
    """The rule of ``volume_unring.unring_axis_np`` with FFT shifts, in float32 torch."""
    from mri_superresolution_amd.volume_unring import shift_order
    a, b = window
    k = torch.arange(n // 2 + 1, dtype=torch.float64, device=device)
    ramps = []
    for m in shift_order(K):
        s = m / (2.0 * K)
        ramp = torch.exp(2j * math.pi * k * s / n)
        if n % 2 == 0:
            ramp[-1] = math.cos(math.pi * s)
        form = [1, 1, 1]
        form[axis] = n // 2 + 1
        ramps.append((s, ramp.to(torch.complex64).reshape(form)))

    def variations(f):
        d = (f - f.roll(-1, axis)).abs()
        tvl = sum(d.roll(j + 1, axis) for j in range(a, b + 1))
        tvr = sum(d.roll(-j, axis) for j in range(a, b + 1))
        return tvl, tvr

    def run(v):
        spec = torch.fft.rfft(v, dim=axis)
        best, tvr = variations(v)
        value = v.clone()
        best = torch.minimum(best, tvr)
        for s, ramp in ramps:
            f = torch.fft.irfft(spec * ramp, n=n, dim=axis)
            cand = f - (f - f.roll(1, axis)) * s if s > 0 else f + (f - f.roll(-1, axis)) * s
            for tv in variations(f):
                win = tv < best
                best = torch.where(win, tv, best)
                value = torch.where(win, cand, value)
        return value
    return run


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=256, help="the extent n of the n^3 volume (8..512)")
    p.add_argument("--shifts", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--inner", type=int, default=2)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unring_bench needs the MI355X: there is nothing to time on a CPU")
    from mri_superresolution_amd.volume_kspace import zerofill2
    from mri_superresolution_amd.volume_unring import unring, unring_axis

    n, K, dev, window = args.size, args.shifts, torch.device("cuda"), (1, 3)
    g = torch.Generator(device="cuda").manual_seed(0)
    vol = torch.zeros((n, n, n), device=dev)
    vol[n // 4:3 * n // 4, n // 3:2 * n // 3, n // 5:4 * n // 5] = 1000.0      # a box, so that there is something to select
    vol += torch.rand((n, n, n), device=dev, generator=g) * 40.0
    out = torch.empty_like(vol)
    up_out = torch.empty((2 * n, n, n), device=dev)
    by_torch = make_torch_unring(n, 2, K, window, dev)
    copy_src, copy_dst = torch.empty_like(vol), torch.empty_like(vol)
    res = {"gpu": torch.cuda.get_device_name(0), "size": n, "shifts": K, "window": list(window), "reps": args.reps, "inner": args.inner}
    diff = (unring_axis(vol, 2, K, window) - by_torch(vol)).abs()
    res["torch_vs_kernel_axis2"] = {"max_abs_diff": float(diff.max()), "share_above_0.01": float((diff > 0.01).float().mean()),
                                    "data_range": 1040.0}
    fns = {"unring_axis0": lambda: unring_axis(vol, 0, K, window, out=out), "unring_axis1": lambda: unring_axis(vol, 1, K, window, out=out),
           "unring_axis2": lambda: unring_axis(vol, 2, K, window, out=out), "unring_3axes": lambda: unring(vol, (0, 1, 2), K, window),
           "torch_axis2": lambda: by_torch(vol), "zerofill_axis0": lambda: zerofill2(vol, (0,), out=up_out),
           "copy": lambda: copy_dst.copy_(copy_src)}
    res["times"] = alternating_times(fns, args.reps, args.warmup, args.inner)
    t = {k: v["us_median"] for k, v in res["times"].items()}
    pairs = 2 * K * n ** 4                                           # multiply-add pairs of one axis: 2K candidates, n terms per sample
    for name in ("unring_axis0", "unring_axis1", "unring_axis2"):
        res[name] = {"ms": round(t[name] / 1e3, 3), "over_zerofill_pass": round(t[name] / t["zerofill_axis0"], 2),
                     "over_copy": round(t[name] / t["copy"], 1), "T_pairs_per_s": round(pairs / (t[name] * 1e-6) / 1e12, 3)}
    res["unring_axis2"]["over_torch"] = round(t["unring_axis2"] / t["torch_axis2"], 3)
    res["unring_3axes"] = {"ms": round(t["unring_3axes"] / 1e3, 3),
                           "split_ms": round((t["unring_3axes"] - t["unring_axis0"] - t["unring_axis1"] - t["unring_axis2"]) / 1e3, 3)}
    res["G_pairs_per_axis"] = round(pairs / 1e9, 2)
    res["copy_TBps"] = round(8 * vol.numel() / (t["copy"] * 1e-6) / 1e12, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
