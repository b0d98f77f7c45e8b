#!/usr/bin/env python3
"""Cost of the multi-planar blend of isotropic whole-volume inference (csrc/volume_blend.hip) next to the passes it combines.

    python tools/isotropic_bench.py [--size 256] [--batch 16] [--reps 20] [--base_filters 64]

On a size^3 float32 volume (V voxels) with synthetic weights:
(a) the three enhance_volume passes (axis 0, 1, 2; fp32 forward, full batches replayed as HIP graphs captured before the clock
    starts; wall clock around synchronised calls, best of 3);
(b) the three blend launches SET -> ADD -> FINISH on resident slice-major planes, HIP events around the three after warm-up;
    its achieved bytes/s against the traffic model: per plane read 4V floats, read 8V except for the first plane, write 8V;
(c) the same blend written with torch: per plane movedim().contiguous(), F.interpolate along the slice axis, add; one division.
Prints one JSON line (profiles/NOTES.md, "Isotropic volumes")."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.benchutil import event_times      # noqa: E402


def synthetic_volume(size, seed=0):
    """MRI-like: a dark background of exact zeros, integer intensities 0..4095 elsewhere."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(0, 4096, (size, size, size), device="cuda", generator=g).float()
    return x * (torch.rand((size, size, size), device="cuda", generator=g) > 0.6)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--base_filters", type=int, default=64)
    args = p.parse_args()
    from mri_superresolution_amd import _lib as L
    from mri_superresolution_amd.models.unet_model import UNetSuperRes
    from mri_superresolution_amd.volume import enhance_volume, up2_blend

    torch.manual_seed(0)
    model = UNetSuperRes(1, 1, base_filters=args.base_filters).cuda().eval().set_compute_dtype(torch.float32)
    n = args.size
    voxels = n ** 3
    vol = synthetic_volume(n)
    res = {"gpu": torch.cuda.get_device_name(0), "size": n, "batch": args.batch, "base_filters": args.base_filters}

    cache = {}
    for axis in (0, 1, 2):                                        # warm-up, capture
        enhance_volume(model, vol, axis=axis, batch_size=args.batch, graph_cache=cache)
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        for axis in (0, 1, 2):
            enhance_volume(model, vol, axis=axis, batch_size=args.batch, graph_cache=cache)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res["passes"] = {"ms_best_of_3": round(min(times) * 1e3, 2), "slices_per_s": round(3 * n / min(times), 1)}
    del cache

    g = torch.Generator(device="cuda").manual_seed(1)
    planes = [torch.rand((n, 2 * n, 2 * n), device="cuda", generator=g) * 4095 for _ in range(3)]      # slice-major [S][R][C]
    acc = torch.empty((2 * n, 2 * n, 2 * n), dtype=torch.float32, device="cuda")

    def blend():
        up2_blend(planes[0], 0, acc, L.VOLBLEND_SET)
        up2_blend(planes[1], 1, acc, L.VOLBLEND_ADD)
        up2_blend(planes[2], 2, acc, L.VOLBLEND_FINISH, 3, acc)

    def blend_torch():
        total = None
        for axis in (0, 1, 2):
            e = planes[axis].movedim(0, axis).contiguous()         # C order, as enhance_volume's caller sees it after a copy
            lead = e.movedim(axis, 2).reshape(1, -1, n)            # F.interpolate's linear mode works on the last axis of (N, C, L)
            u = F.interpolate(lead, scale_factor=2, mode="linear", align_corners=False)
            shape = list(e.shape)
            del shape[axis]
            u = u.reshape(shape + [2 * n]).movedim(2, axis)
            total = u.contiguous() if total is None else total.add_(u)
        return total.div_(3.0)

    res["blend"] = event_times(blend, args.reps, args.warmup)
    for axis, mode, extra in ((0, L.VOLBLEND_SET, ()), (1, L.VOLBLEND_ADD, ()), (2, L.VOLBLEND_FINISH, (3, acc))):
        res[f"blend_axis{axis}"] = event_times(lambda: up2_blend(planes[axis], axis, acc, mode, *extra), args.reps, args.warmup)
    res["blend_torch"] = event_times(blend_torch, max(3, args.reps // 4), 1)
    model_bytes = 4 * voxels * (3 * 4 + 2 * 8 + 3 * 8)            # reads of the planes, of acc (not by the first), writes
    res["blend_model_bytes"] = model_bytes
    res["blend_TBps"] = round(model_bytes / (res["blend"]["us_median"] * 1e-6) / 1e12, 3)
    res["blend_over_torch"] = round(res["blend"]["us_median"] / res["blend_torch"]["us_median"], 4)
    res["blend_share_of_passes"] = round(res["blend"]["us_median"] * 1e-3 / res["passes"]["ms_best_of_3"], 5)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
