#!/usr/bin/env python3
"""Cost of the non-local-means kernel (csrc/volume_denoise.hip) next to the same filter written with torch.

    python tools/denoise_bench.py [--reps 10] [--warmup 2] [--inner 1] [--size 256] [--radius 3] [--torch_size 256] [--skip_torch]

On a ``--size``^3 float32 phantom with Rician noise: ``denoise`` (one launch of ``mrisr_f32_volume_nlm``), ``estimate_noise`` and
``background_mask`` apart, and ``denoise_volume(check=False)`` (all of them).  HIP events around ``--inner`` back-to-back runs after
warm-up, the median over ``--reps`` such windows, per run; no read-back inside the window.  The torch path is the same filter on the
same device in the textbook formulation - for every candidate a shifted view of the edge-padded volume, the squared difference,
``avg_pool3d`` (3 x 3 x 3, times 27) for the patch distance, ``exp`` for the weight - on the central ``--torch_size``^3 voxels of the
phantom (all of it by default); ``kernel_over_torch`` compares the two at THAT size, in one loop, alternating.  The torch weights are ``exp(-x)``, not the table's midpoints, and its sums are in another order: the two results are
compared by their largest absolute difference over the intensity scale.  ``ops``: 3 operations per squared difference of a plane (9
of them, 10 planes per 8 voxels) and candidate; ``lds_reads``: 18 reads per plane.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.benchutil import alternating_times      # noqa: E402


def phantom(n, sigma, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    ax = torch.linspace(-1, 1, n, device=device)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    clean = 600.0 * (r < 0.8) + 300.0 * (r < 0.5) - 200.0 * ((x.abs() < 0.12) & (r < 0.8))
    re = clean + sigma * torch.randn(clean.shape, device=device, generator=g)
    im = sigma * torch.randn(clean.shape, device=device, generator=g)
    return torch.sqrt(re * re + im * im).contiguous()


def torch_nlm(v, inv_h2, two_sigma2, radius):
    import torch.nn.functional as F
    n0, n1, n2 = v.shape
    h = radius + 1
    pad = F.pad(v[None, None], (h,) * 6, mode="replicate")[0, 0]
    val = v * v
    valp = F.pad(val[None, None], (h,) * 6)[0, 0]
    inside = F.pad(torch.ones_like(v)[None, None], (h,) * 6)[0, 0]
    a = pad[h - 1:h + n0 + 1, h - 1:h + n1 + 1, h - 1:h + n2 + 1]
    num, den, wmax = torch.zeros_like(v), torch.zeros_like(v), torch.zeros_like(v)
    for t0 in range(-radius, radius + 1):
        for t1 in range(-radius, radius + 1):
            for t2 in range(-radius, radius + 1):
                if t0 == t1 == t2 == 0:
                    continue
                b = pad[h - 1 + t0:h + n0 + 1 + t0, h - 1 + t1:h + n1 + 1 + t1, h - 1 + t2:h + n2 + 1 + t2]
                d = F.avg_pool3d(((a - b) ** 2)[None, None], 3, stride=1)[0, 0] * 27.0
                x = d * inv_h2
                sl = (slice(h + t0, h + t0 + n0), slice(h + t1, h + t1 + n1), slice(h + t2, h + t2 + n2))
                w = torch.exp(-x) * (x < 16) * inside[sl]
                num += w * valp[sl]
                den += w
                wmax = torch.maximum(wmax, w)
    wc = torch.where(wmax > 0, wmax, torch.ones_like(wmax))
    m = (num + wc * val) / (den + wc)
    return torch.sqrt((m - two_sigma2).clamp_min(0))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--inner", type=int, default=1)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--torch_size", type=int, default=256)
    p.add_argument("--radius", type=int, default=3)
    p.add_argument("--sigma", type=float, default=40.0)
    p.add_argument("--skip_torch", action="store_true")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_bench needs the MI355X: there is nothing to time on a CPU")
    from mri_superresolution_amd import volume_denoise as D

    n, R = args.size, args.radius
    vol = phantom(n, args.sigma, "cuda", 1)
    bg = D.background_mask(vol)
    params, count = D.estimate_noise(vol, bg)
    out = torch.empty_like(vol)
    candidates = (2 * R + 1) ** 3 - 1
    planes = vol.numel() / 8 * 10 * candidates
    res = {"gpu": torch.cuda.get_device_name(0), "size": n, "radius": R, "candidates": candidates, "inner": args.inner, "reps": args.reps,
           "sigma": float(params[2]), "background": int(count), "squared_differences": 9 * planes, "ops": 27 * planes, "lds_reads": 18 * planes}
    fns = {"denoise": lambda: D.denoise(vol, params, R, True, out=out),
           "estimate_noise": lambda: D.estimate_noise(vol, bg),
           "background_mask": lambda: D.background_mask(vol),
           "denoise_volume": lambda: D.denoise_volume(vol, radius=R, check=False)}
    res["times"] = alternating_times(fns, args.reps, args.warmup, args.inner)
    us = res["times"]["denoise"]["us_median"]
    res["tops_per_s"] = round(res["ops"] / (us * 1e-6) / 1e12, 2)
    res["lds_tb_per_s"] = round(4 * res["lds_reads"] / (us * 1e-6) / 1e12, 2)
    if not args.skip_torch:
        m = min(args.torch_size, n)
        lo = (n - m) // 2
        small = vol[lo:lo + m, lo:lo + m, lo:lo + m].contiguous()
        small_out = torch.empty_like(small)
        inv_h2, two_sigma2 = float(params[0]), float(params[1])
        pair = alternating_times({"kernel": lambda: D.denoise(small, params, R, True, out=small_out),
                                  "torch": lambda: torch_nlm(small, inv_h2, two_sigma2, R)}, max(3, args.reps // 2), 1, 1)
        res["torch_size"] = m
        res["times_at_torch_size"] = pair
        res["kernel_over_torch"] = round(pair["kernel"]["us_median"] / pair["torch"]["us_median"], 5)
        res["torch_max_abs_diff_over_scale"] = float((torch_nlm(small, inv_h2, two_sigma2, R) - D.denoise(small, params, R, True)).abs().max() / 900.0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
