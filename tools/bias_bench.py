#!/usr/bin/env python3
"""Cost of the bias-field matching (csrc/volume_bias.hip) next to the same smoothing written with torch.

    python tools/bias_bench.py [--reps 20] [--warmup 3] [--inner 3] [--size 256] [--sigma 25] [--skip_torch]

On a ``--size``^3 float32 phantom pair with masks that are about half full and a sigma of ``--sigma`` voxels on every axis (25:
R = 75, 151 taps): ``match_bias`` (two masked smooths of three passes and two channels each, one launch that forms and applies the
field), one ``smooth_masked`` alone, and ``smooth_masked`` with the sigma on one axis only and on none - the passes cannot be timed
apart through one entry point, so ``pass_us`` is derived: the time with the sigma on that axis alone, minus the time with it on none,
plus a third of the latter.  HIP events around ``--inner`` back-to-back runs after warm-up, the median over ``--reps`` such windows,
per run; no read-back inside the window.  The torch path is the same three-pass, two-channel smoothing with
``torch.nn.functional.conv1d`` (zero padding, the same float32 taps; its sums are in the library's order, not ascending) and
alternates with the kernels in one loop, so that the ratio is taken on one box in one run.  The two results are compared by their
largest relative difference.  ``min_bytes``: the least HBM traffic of a smooth - read the volume (4 bytes a voxel) and the mask
(1; 2 with two masks), write two volumes, then twice read two and write two - and of ``match_bias`` - two smooths and 28 bytes a
voxel for the field (five volumes read, two written); ``tb_per_s`` = min_bytes over the median time, ``hbm_share`` that over
``--hbm_tb_per_s`` (6.29: the measured float4-copy rate of an MI355X).  The taps are rounded products and sums, never an fma:
``ops`` counts 4 operations per tap, channel-pair and voxel, ``tops_per_s`` their rate.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.benchutil import alternating_times      # noqa: E402


def phantom(n, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    ax = torch.linspace(-1, 1, n, device=device)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    v = 0.55 * torch.exp(-((x / 0.75) ** 4 + (y / 0.85) ** 4 + (z / 0.8) ** 4))
    v = v * torch.exp(0.25 * x - 0.2 * y * y + 0.15 * z * x * seed)
    mask = ((x * x + y * y + z * z) <= 0.985 ** 2).to(torch.uint8).contiguous()      # a ball: about 50 % of the box
    return (1000.0 * (v + 0.01 * torch.randn(v.shape, device=device, generator=g)).clamp_min(0)).contiguous(), mask


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--inner", type=int, default=3)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--sigma", type=float, default=25.0)
    p.add_argument("--hbm_tb_per_s", type=float, default=6.29)
    p.add_argument("--skip_torch", action="store_true")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bias_bench needs the MI355X: there is nothing to time on a CPU")
    from mri_superresolution_amd import volume_bias as V

    n, s = args.size, args.sigma
    src, sm = phantom(n, "cuda", 1)
    ref, rm = phantom(n, "cuda", 0)
    voxels = src.numel()
    taps = V.gaussian_taps(s)
    sig = {"all": (s, s, s), "axis0": (s, 0, 0), "axis1": (0, s, 0), "axis2": (0, 0, s), "none": (0, 0, 0)}
    ws = {k: V.BiasWorkspace(src.shape, v, "cuda") for k, v in sig.items()}
    res = {"gpu": torch.cuda.get_device_name(0), "size": n, "sigma_vox": s, "radius": (taps.size - 1) // 2, "inner": args.inner,
           "reps": args.reps, "mask_share": round(float(sm.float().mean()), 4),
           "min_bytes": {"smooth_masked": 45 * voxels, "match_bias": (2 * 46 + 28) * voxels},
           "ops": {"pass": 4 * taps.size * voxels}}
    fns = {"match_bias": lambda: V.match_bias(src, ref, sm, rm, sig["all"], workspace=ws["all"]),
           **{f"smooth_{k}": (lambda k=k: V.smooth_masked(src, sm, sig[k], ws[k])) for k in sig}}
    if not args.skip_torch:
        import torch.nn.functional as F
        w = torch.from_numpy(taps).cuda().view(1, 1, -1)
        r = (taps.size - 1) // 2

        def torch_smooth():
            keep = (sm != 0) & ~torch.isnan(src)
            x = torch.stack([torch.where(keep, src, torch.zeros_like(src)), keep.float()])      # (2, X, Y, Z)
            for axis in (3, 2, 1):
                x = x.movedim(axis, -1)
                shape = x.shape
                x = F.conv1d(x.reshape(-1, 1, shape[-1]), w, padding=r).reshape(shape).movedim(-1, axis)
            return x[0], x[1]
        fns["torch_smooth"] = torch_smooth
    t = alternating_times(fns, args.reps, args.warmup, args.inner)
    res["times"] = t
    none = t["smooth_none"]["us_median"]
    res["pass_us"] = {a: round(t[f"smooth_{a}"]["us_median"] - none + none / 3, 1) for a in ("axis2", "axis1", "axis0")}
    res["tops_per_s"] = {a: round(res["ops"]["pass"] / (us * 1e-6) / 1e12, 2) for a, us in res["pass_us"].items()}
    for k, name in (("smooth_masked", "smooth_all"), ("match_bias", "match_bias")):
        rate = res["min_bytes"][k] / (t[name]["us_median"] * 1e-6) / 1e12
        res[k] = {"tb_per_s": round(rate, 3), "hbm_share": round(rate / args.hbm_tb_per_s, 3)}
    if not args.skip_torch:
        num, den = V.smooth_masked(src, sm, sig["all"], ws["all"])
        tnum, tden = torch_smooth()
        res["torch_max_rel_diff"] = {"num": float(((tnum - num).abs() / num.abs().clamp_min(1e-3)).max()),
                                     "den": float(((tden - den).abs() / den.abs().clamp_min(1e-3)).max())}
        res["kernel_over_torch"] = round(t["smooth_all"]["us_median"] / t["torch_smooth"]["us_median"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
