#!/usr/bin/env python3
"""Cost of the volume evaluation kernels (csrc/volume_metrics.hip, csrc/volume_eval.hip) next to the same work written with torch.

    python tools/volume_eval_bench.py [--shapes 256x256x256 512x512x256] [--reps 10] [--warmup 2] [--skip_torch]

Per shape, on a pair of float32 volumes in [0, 1] ("truth plus error"):
(a) ``volume_metrics`` (window 11, the fused pass plus the finalising launch), HIP events around the call after warm-up; the
    achieved bytes/s against the ALGORITHMIC traffic - the two volumes read once, 8 bytes per voxel - and its share of the
    8.0 TB/s HBM3E specification rate (6.3 TB/s is what a copy achieves on this part);
(b) the same metric written with torch: five moment volumes, three separable ``conv3d`` passes each, then the element-wise map
    and three reductions, all float32 on the device; the two SSIM values are printed side by side;
(c) ``upscale2`` linear and cubic of the volume HALVED on every axis (so that the output has the shape above), against
    ``F.interpolate(mode="trilinear")`` for the linear one; traffic model: input once, output once.
Prints one JSON line (profiles/NOTES.md, "Volume evaluation")."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_SPEC_BPS = 8.0e12


def event_times(fn, reps, warmup):
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
    return {"us_median": round(statistics.median(times), 1), "us_min": round(min(times), 1)}


def rate(nbytes, t):
    bps = nbytes / (t["us_median"] * 1e-6)
    return {"TBps": round(bps / 1e12, 3), "share_of_hbm_spec": round(bps / HBM_SPEC_BPS, 4)}


def metrics_torch(a, b, val_range, window_size=11, sigma=1.5):
    """(ssim, mse, mae) as 0-d device tensors: float32, separable conv3d, zero padding."""
    from mri_superresolution_amd.utils.losses import gaussian_window
    g = gaussian_window(window_size, sigma).to(a.device)
    h = window_size // 2

    def blur(x):
        x = F.conv3d(x, g.view(1, 1, -1, 1, 1), padding=(h, 0, 0))
        x = F.conv3d(x, g.view(1, 1, 1, -1, 1), padding=(0, h, 0))
        return F.conv3d(x, g.view(1, 1, 1, 1, -1), padding=(0, 0, h))

    a, b = a[None, None], b[None, None]
    c1, c2 = (0.01 * val_range) ** 2, (0.03 * val_range) ** 2
    mu1, mu2 = blur(a), blur(b)
    s11, s22, s12 = blur(a * a) - mu1 * mu1, blur(b * b) - mu2 * mu2, blur(a * b) - mu1 * mu2
    ssim = (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))).mean()
    d = a - b
    return ssim, (d * d).mean(), d.abs().mean()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", type=str, nargs="+", default=["256x256x256", "512x512x256"])
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--skip_torch", action="store_true")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("volume_eval_bench needs the MI355X: there is nothing to time on a CPU")
    from mri_superresolution_amd.volume_eval import upscale2, volume_metrics

    res = {"gpu": torch.cuda.get_device_name(0), "window": 11, "shapes": {}}
    for text in args.shapes:
        shape = tuple(int(s) for s in text.split("x"))
        voxels = shape[0] * shape[1] * shape[2]
        g = torch.Generator(device="cuda").manual_seed(0)
        ref = torch.rand(shape, device="cuda", generator=g)
        pred = (ref + 0.05 * torch.randn(shape, device="cuda", generator=g)).clamp_(0, 1)
        r = {"voxels": voxels}
        r["volume_metrics"] = event_times(lambda: volume_metrics(pred, ref, 1.0), args.reps, args.warmup)
        r["volume_metrics"].update(rate(8 * voxels, r["volume_metrics"]))
        vals = volume_metrics(pred, ref, 1.0).cpu().tolist()
        r["ssim_hip"], r["mse_hip"] = vals[0], vals[1]
        if not args.skip_torch:
            r["metrics_torch"] = event_times(lambda: metrics_torch(pred, ref, 1.0), max(3, args.reps // 2), 1)
            ssim_t, mse_t, _ = metrics_torch(pred, ref, 1.0)
            r["ssim_torch"], r["mse_torch"] = float(ssim_t), float(mse_t)
            r["hip_over_torch"] = round(r["volume_metrics"]["us_median"] / r["metrics_torch"]["us_median"], 4)
        low = torch.rand(tuple(s // 2 for s in shape), device="cuda", generator=g) * 4095
        for method in ("linear", "cubic"):
            r[f"upscale2_{method}"] = event_times(lambda: upscale2(low, method), args.reps, args.warmup)
            r[f"upscale2_{method}"].update(rate(4 * (low.numel() + voxels), r[f"upscale2_{method}"]))
        if not args.skip_torch:
            r["trilinear_torch"] = event_times(
                lambda: F.interpolate(low[None, None], scale_factor=2, mode="trilinear", align_corners=False), max(3, args.reps // 2), 1)
        res["shapes"][text] = r
        del ref, pred, low
    print(json.dumps(res))


if __name__ == "__main__":
    main()
