#!/usr/bin/env python3
"""Cost of the float windowing of whole-volume inference (csrc/percentile.hip) and throughput of enhance_volume.

    python tools/volume_bench.py [--batch 16] [--reps 30] [--base_filters 64]

(a) bounds + normalise + restore for a batch of 16 slices at 256^2 and 512^2 (the restore on the 512^2 / 1024^2 outputs), HIP
    events around the whole sequence after warm-up, inputs resident in HBM; next to it a torch.quantile-per-slice version of the
    same window (the plumbing one would write without the kernels) and the fp32 eval forward of the same batch, replayed as a
    HIP graph; the windowing's share of that forward.
(b) slices/s of enhance_volume on a synthetic 256 x 256 x 160 volume, graph on and off (wall clock around synchronised calls,
    the graph captured before the clock starts).
Prints one JSON line (profiles/NOTES.md, "Whole-volume inference")."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.benchutil import event_times      # noqa: E402

WINDOW_LAUNCHES = 9 + 1 + 1      # mrisr_f32_percentile_bounds (init + 4 x (histogram, pick)), normalise, restore


def synthetic_slices(b, size, seed=0):
    """MRI-like: a dark background of exact zeros, integer intensities 0..4095 elsewhere."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(0, 4096, (b, size, size), device="cuda", generator=g).float()
    return x * (torch.rand((b, size, size), device="cuda", generator=g) > 0.6)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--base_filters", type=int, default=64)
    p.add_argument("--depth", type=int, default=160, help="slices of the synthetic volume of part (b)")
    args = p.parse_args()
    from mri_superresolution_amd.models.unet_model import UNetSuperRes
    from mri_superresolution_amd.utils import imageops
    from mri_superresolution_amd.volume import enhance_volume

    torch.manual_seed(0)
    model = UNetSuperRes(1, 1, base_filters=args.base_filters).cuda().eval().set_compute_dtype(torch.float32)
    res = {"gpu": torch.cuda.get_device_name(0), "batch": args.batch, "base_filters": args.base_filters,
           "window_launches_per_chunk": WINDOW_LAUNCHES}
    for size in (256, 512):
        x = synthetic_slices(args.batch, size)
        y = torch.rand((args.batch, 1, 2 * size, 2 * size), device="cuda")
        out = torch.empty_like(y)

        def window():
            _, lohi = imageops.normalise_percentile_f32(x, return_bounds=True)
            imageops.restore_window(y, lohi, out=out)

        def window_torch():
            flat = x.reshape(args.batch, -1)
            lohi = torch.stack([torch.quantile(flat[b], torch.tensor([0.005, 0.995], device="cuda")) for b in range(args.batch)])
            lo, hi = lohi[:, 0, None], lohi[:, 1, None]
            xn = ((torch.minimum(torch.maximum(flat, lo), hi) - lo) / (hi - lo)).reshape(args.batch, 1, size, size)
            torch.add(y.clamp(0, 1).reshape(args.batch, -1) * (hi - lo), lo, out=out.view(args.batch, -1))
            return xn

        xn = imageops.normalise_percentile_f32(x)
        run = model.graphed_forward(xn)
        entry = {"window": event_times(window, args.reps, args.warmup),
                 "window_torch_quantile": event_times(window_torch, args.reps, args.warmup),
                 "forward_graph": event_times(lambda: run(xn), args.reps, args.warmup)}
        entry["window_share_of_forward"] = round(entry["window"]["us_median"] / entry["forward_graph"]["us_median"], 4)
        res[f"in{size}"] = entry
        del run
    vol = synthetic_slices(args.depth, 256, seed=1).permute(1, 2, 0).contiguous()      # (256, 256, depth), slices across axis 2
    for use_graph in (True, False):
        cache = {}
        enhance_volume(model, vol, batch_size=args.batch, use_graph=use_graph, graph_cache=cache)      # warm-up, capture
        torch.cuda.synchronize()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            enhance_volume(model, vol, batch_size=args.batch, use_graph=use_graph, graph_cache=cache)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        res["volume_256x256x%d_%s" % (args.depth, "graph" if use_graph else "eager")] = {
            "slices_per_s": round(args.depth / min(times), 1), "ms_best_of_3": round(min(times) * 1e3, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
