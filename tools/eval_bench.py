#!/usr/bin/env python3
"""Wall time of scripts/evaluate.py's per-image path against its batched device-side path, and the achieved bandwidth of the
kernels the batched path adds (profiles/NOTES.md, "Batched evaluation").

    python tools/eval_bench.py [--pairs 256] [--size 256] [--base_filters 64] [--batch_size 16]

One process, synthetic pairs written as PNGs into a temporary directory.  PNG decode is excluded from both sides: the
batched path reports it separately, the per-image path's share (LR decoded four times, HR once per pair) is measured on its
own and subtracted.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pairs", type=int, default=256)
    p.add_argument("--size", type=int, default=256, help="LR edge; HR is twice that")
    p.add_argument("--base_filters", type=int, default=64)
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--reps", type=int, default=20, help="launches per kernel in the bandwidth pass")
    args = p.parse_args()
    from PIL import Image
    from mri_superresolution_amd.engine import KernelTimer
    from mri_superresolution_amd.models.unet_model import UNetSuperRes
    from mri_superresolution_amd.utils import evalops
    from oracle.inputs import make_pair
    from scripts import evaluate

    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = UNetSuperRes(1, 1, args.base_filters).to(dev).eval()
    res = {"gpu": torch.cuda.get_device_name(0), "pairs": args.pairs, "lr_size": args.size, "base_filters": args.base_filters,
           "batch_size": args.batch_size}
    with tempfile.TemporaryDirectory() as tmp:
        lr_dir, hr_dir = os.path.join(tmp, "lr"), os.path.join(tmp, "hr")
        os.makedirs(lr_dir), os.makedirs(hr_dir)
        for i0 in range(0, args.pairs, 16):
            low, high = make_pair(min(16, args.pairs - i0), args.size, args.size, 100 + i0)
            for j in range(low.shape[0]):
                Image.fromarray((low[j, 0].numpy() * 255).astype(np.uint8)).save(os.path.join(lr_dir, f"p{i0 + j:04d}.png"))
                Image.fromarray((high[j, 0].numpy() * 255).astype(np.uint8)).save(os.path.join(hr_dir, f"p{i0 + j:04d}.png"))
        pairs = evaluate.find_pairs(hr_dir, lr_dir)
        # warm both paths on one chunk (kernel attributes, weight packing, allocator)
        evaluate.run_benchmarks(pairs[:2], model, dev)
        evaluate.run_benchmarks_batched(pairs[:args.batch_size], model, dev, batch_size=args.batch_size)
        torch.cuda.synchronize()

        t0 = time.time()
        for lr_path, hr_path in pairs:
            for _ in range(4):
                np.asarray(Image.open(lr_path).convert("L"))
            np.asarray(Image.open(hr_path).convert("L"))
        res["per_image_decode_s"] = time.time() - t0
        t0 = time.time()
        rows = evaluate.run_benchmarks(pairs, model, dev)
        torch.cuda.synchronize()
        res["per_image_total_s"] = time.time() - t0
        res["per_image_s"] = res["per_image_total_s"] - res["per_image_decode_s"]
        for name, graph in (("batched", True), ("batched_no_graph", False)):
            tm = {}
            t0 = time.time()
            rows_b = evaluate.run_benchmarks_batched(pairs, model, dev, batch_size=args.batch_size, use_graph=graph, timings=tm)
            torch.cuda.synchronize()
            res[name + "_total_s"] = time.time() - t0
            res[name + "_decode_s"] = tm["decode"]
            res[name + "_s"] = tm["device"]
        res["speedup_excl_decode"] = res["per_image_s"] / res["batched_s"]
        res["summary_per_image"] = {m: round(s["ssim"], 6) for m, s in evaluate.summarise(rows).items()}
        res["summary_batched"] = {m: round(s["ssim"], 6) for m, s in evaluate.summarise(rows_b).items()}

    # achieved bandwidth of the new launches on one chunk, from the nbytes timer (algorithmic bytes / event time)
    g = torch.Generator().manual_seed(1)
    lr = torch.randint(0, 256, (args.batch_size, args.size, args.size), dtype=torch.uint8, generator=g).to(dev)
    a = torch.rand((args.batch_size, 1, 2 * args.size, 2 * args.size), generator=g).to(dev)
    b = torch.rand((args.batch_size, 1, 2 * args.size, 2 * args.size), generator=g).to(dev)
    kernels = {}
    jobs = [(f"u8_upscale2[{m}]", "mrisr_u8_upscale2", lambda m=m: evalops.upscale2_u8(lr, m)) for m in evalops.METHODS]
    jobs.append(("image_metrics", "mrisr_image_metrics", lambda: evalops.image_metrics(a, b)))
    for label, entry, fn in jobs:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        with KernelTimer() as kt:
            for _ in range(args.reps):
                fn()
        torch.cuda.synchronize()
        s = kt.summary()[entry]
        kernels[label] = {"us": round(s["ms_per_launch"] * 1e3, 2), "MB": round(s["bytes_per_launch"] / 1e6, 2),
                          "GBps": round(s["tbps"] * 1e3, 1)}
    res["kernels"] = kernels
    print(json.dumps(res))


if __name__ == "__main__":
    main()
