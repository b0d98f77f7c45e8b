#!/usr/bin/env python3
"""Cost of the intensity standardisation (csrc/volume_intensity.hip) next to the same work written with torch.

    python tools/intensity_bench.py [--reps 20] [--warmup 3] [--inner 5] [--size 256] [--skip_torch]

On a ``--size``^3 float32 phantom with a mask that is about half full: ``masked_percentiles`` with the 11 landmarks plus
``piecewise_map`` onto fixed target landmarks (the unit of ``volume_intensity.match_intensity`` per scan, without its one read).
HIP events around ``--inner`` back-to-back runs after warm-up, the median over ``--reps`` such windows, per run; no read-back inside
the window.  The torch path does the same work - ``torch.sort(vol[mask])``, the two order statistics of every landmark by indexing
with numpy's interpolation, then ``torch.searchsorted`` and the map's arithmetic (``torch.quantile`` refuses inputs this large) -
and alternates with the kernel in one loop, so that the ratio is taken on one box in one run.  Its count needs a host read
(``vol[mask]`` synchronises), the kernel's does not.  The two results are compared: landmarks by value, mapped voxels by their
largest difference.  ``bytes``: what the passes read and write - four histogram passes over the volume (4 bytes a voxel) and the
mask (1), the map 8 bytes a voxel.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.benchutil import alternating_times_fine as alternating_times      # noqa: E402


def phantom(n, device):
    """Smooth blobs in 0..1000 on an n^3 grid plus noise."""
    g = torch.Generator(device=device).manual_seed(0)
    ax = torch.linspace(-1, 1, n, device=device)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    v = 0.55 * torch.exp(-((x / 0.75) ** 4 + (y / 0.85) ** 4 + (z / 0.8) ** 4))
    for cx, cy, cz, s, a in ((0.3, 0.2, -0.15, 0.25, 0.45), (-0.35, -0.3, 0.25, 0.2, 0.35), (0.1, -0.45, -0.4, 0.15, -0.3),
                             (-0.2, 0.4, 0.1, 0.3, 0.25)):
        v = v + a * torch.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (2 * s * s))
    mask = ((x * x + y * y + z * z) <= 0.985 ** 2).to(torch.uint8).contiguous()      # a ball: 4 pi / 3 * 0.985^3 / 8 = 50 % of the box
    return (1000.0 * (v.clamp_min(0) + 0.01 * torch.randn(v.shape, device=device, generator=g))).contiguous(), mask


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--inner", type=int, default=5)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--skip_torch", action="store_true")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("intensity_bench needs the MI355X: there is nothing to time on a CPU")
    from mri_superresolution_amd import volume_intensity as I

    n = args.size
    vol, mask = phantom(n, "cuda")
    q = I.LANDMARKS
    target = torch.linspace(50.0, 900.0, len(q), device="cuda")
    ws = I.percentiles_workspace(len(q), "cuda")
    out = torch.empty_like(vol)
    res = {"gpu": torch.cuda.get_device_name(0), "size": n, "landmarks": len(q), "inner": args.inner, "reps": args.reps,
           "mask_share": round(float(mask.float().mean()), 4),
           "bytes": {"masked_percentiles": 4 * 5 * vol.numel(), "piecewise_map": 8 * vol.numel()}}

    def landmarks_only():
        return I.masked_percentiles(vol, mask, q, ws)

    def ours():
        sl, count = I.masked_percentiles(vol, mask, q, ws)
        return sl, count, I.piecewise_map(vol, sl, target, out=out)
    fns = {"kernel": ours, "kernel_landmarks_only": landmarks_only}
    if not args.skip_torch:
        q32 = torch.tensor([np.float32(x) / np.float32(100) for x in q], dtype=torch.float32, device="cuda")
        bmask = mask.bool()
        tout = torch.empty_like(vol)

        def torch_path():
            s = torch.sort(vol[bmask]).values                    # the boolean index reads the count back: a synchronisation
            cnt = s.numel()
            virt = torch.tensor(float(cnt - 1), dtype=torch.float32, device="cuda") * q32
            prev = virt.floor()
            k = prev.long().clamp_(max=cnt - 1)
            lo, hi, t = s[k], s[(k + 1).clamp_(max=cnt - 1)], virt - prev
            d = hi - lo
            sl = torch.where(t >= 0.5, hi - d * (1 - t), lo + d * t)
            i = (torch.searchsorted(sl, vol.reshape(-1), right=True) - 1).clamp_(0, len(q) - 2)
            w = sl[1:] - sl[:-1]
            slope = torch.where(w == 0, torch.zeros_like(w), (target[1:] - target[:-1]) / w)
            torch.add(target[i], (vol.reshape(-1) - sl[i]) * slope[i], out=tout.reshape(-1))
            return sl, cnt, tout
        fns["torch"] = torch_path
    res["times"] = alternating_times(fns, args.reps, args.warmup, args.inner)
    sl, count, mapped = ours()
    res["count"] = int(count.cpu()[0])
    res["source_landmarks"] = [round(float(x), 4) for x in sl.cpu()]
    if not args.skip_torch:
        tsl, tcnt, tmapped = torch_path()
        res["torch_equal"] = {"count": tcnt == res["count"], "landmarks": bool(torch.equal(tsl, sl)),
                              "mapped_max_abs_diff": float((tmapped - mapped).abs().max())}
        res["kernel_over_torch"] = round(res["times"]["kernel"]["us_median"] / res["times"]["torch"]["us_median"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
