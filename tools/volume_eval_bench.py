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
(d) the foreground mask (csrc/volume_mask.hip): ``otsu_mask`` (five launches; the volume read three times, the mask written once:
    13 bytes per voxel), ``binary_close`` at radius 2 (six passes, each reads and writes one byte per voxel), and
    ``foreground_mask(close_radius=2)`` as a whole, next to one metrics launch;
(e) ``volume_metrics(mask=...)`` - the masked instantiation, 9 bytes per voxel - alternating with the unmasked call in one loop,
    so that the ratio of the two is taken on one box in one run.  ``--parent_lib PATH`` adds the unmasked kernel of another
    build of the library (called through ctypes, nothing else of it is used) to the same alternation.
(f) connected components of that mask (csrc/volume_label.hip): ``label_components`` (26-connected; 3 launches), ``largest_component``
    (5 launches) and ``fill_holes`` of the volume (4 launches), each with its time and voxels per second, and their sum next to one
    masked metrics pass.  Algorithmic traffic, bytes per voxel: the local pass reads the mask and writes the labels (5; 9 with the
    cleared side array), the merge pass reads the labels of the voxels on tile surfaces and their neighbours across (about 4 x 0.47
    plus atomics), the flatten pass reads and writes the labels (8, plus one atomic per run of a wave), then 8 (largest: labels and
    sizes) + 5 (select) or 9 (fill: mask, labels, marks gathered by root; mask written).
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

from tools.benchutil import event_times      # noqa: E402

HBM_SPEC_BPS = 8.0e12


def alternating_times(fns, reps, warmup):
    """{name: times} of several callables timed in turn, round after round: what they share of the box's state they share alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: {"us_median": round(statistics.median(v), 1), "us_min": round(min(v), 1)} for k, v in times.items()}


def parent_metrics_call(path, pred, ref):
    """The unmasked fused pass of another build of libmrisr.so on the same pair (window 11, sigma 1.5, range 1)."""
    import ctypes as C
    lib = C.CDLL(path)
    fn = lib.mrisr_f32_volume_metrics
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    sums = torch.zeros(3, dtype=torch.float64, device=pred.device)

    def call():
        sums.zero_()
        rc = fn(pred.data_ptr(), ref.data_ptr(), *pred.shape, 1.0, 1.5, 11, sums.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return call, sums


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
    p.add_argument("--parent_lib", type=str, default=None, help="another build of libmrisr.so: its unmasked metrics kernel joins (e)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("volume_eval_bench needs the MI355X: there is nothing to time on a CPU")
    from mri_superresolution_amd.volume_eval import (binary_close, fill_holes, foreground_mask, label_components, largest_component,
                                                     otsu_mask, upscale2, volume_metrics)

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
        # (d) the mask of a head-like volume: a bright ball in a dark noisy background, about half of the voxels
        x, y, z = torch.meshgrid(*(torch.linspace(-1, 1, n, device="cuda") for n in shape), indexing="ij")
        head = torch.where(x * x + y * y + z * z < 0.95, 600.0 + 200.0 * torch.rand(shape, device="cuda", generator=g),
                           40.0 * torch.rand(shape, device="cuda", generator=g)).contiguous()
        del x, y, z
        mask0 = otsu_mask(head)[0]
        r["otsu_mask"] = event_times(lambda: otsu_mask(head), args.reps, args.warmup)
        r["otsu_mask"].update(rate(13 * voxels, r["otsu_mask"]))
        r["binary_close_r2"] = event_times(lambda: binary_close(mask0, 2), args.reps, args.warmup)
        r["binary_close_r2"].update(rate(12 * voxels, r["binary_close_r2"]))
        r["foreground_mask_r2"] = event_times(lambda: foreground_mask(head, 2), args.reps, args.warmup)
        mask = foreground_mask(head, 2)[0]
        r["mask_share"] = round(float(mask.count_nonzero()) / voxels, 4)
        # (e) masked against unmasked, alternating
        fns = {"unmasked": lambda: volume_metrics(pred, ref, 1.0), "masked": lambda: volume_metrics(pred, ref, 1.0, mask=mask)}
        if args.parent_lib:
            fns["parent_unmasked_kernel"], psums = parent_metrics_call(args.parent_lib, pred, ref)
        r["alternating"] = alternating_times(fns, args.reps, args.warmup)
        r["masked_over_unmasked"] = round(r["alternating"]["masked"]["us_median"] / r["alternating"]["unmasked"]["us_median"], 4)
        r["mask_build_over_metrics"] = round(r["foreground_mask_r2"]["us_median"] / r["alternating"]["unmasked"]["us_median"], 4)
        both = volume_metrics(pred, ref, 1.0, mask=mask).cpu()
        r["ssim_whole_masked_call"], r["ssim_foreground"] = float(both[0, 0]), float(both[1, 0])
        if args.parent_lib:
            r["ssim_parent_kernel"] = float(psums[1]) / voxels
        # (f) connected components of the head phantom's mask
        for name, fn in (("label_components", lambda: label_components(mask, 26)), ("largest_component", lambda: largest_component(mask, 26)),
                         ("fill_holes_3d", lambda: fill_holes(mask))):
            r[name] = event_times(fn, args.reps, args.warmup)
            r[name]["Gvoxels_per_s"] = round(voxels / (r[name]["us_median"] * 1e-6) / 1e9, 3)
        kept, st3 = largest_component(mask, 26)
        r["components"], r["kept_share"] = int(st3[0]), round(float(st3[1]) / voxels, 4)
        r["filled"] = int(fill_holes(mask)[1])
        r["cleanup_over_masked_metrics"] = round((r["largest_component"]["us_median"] + r["fill_holes_3d"]["us_median"])
                                                 / r["alternating"]["masked"]["us_median"], 4)
        del kept
        res["shapes"][text] = r
        del ref, pred, low, head, mask, mask0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
