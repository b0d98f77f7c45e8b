#!/usr/bin/env python3
"""Times the profile pass of csrc/volume_edge.hip on a --size^3 volume against the same binning written with torch operators on the
device and against a device copy of its algorithmic bytes.  Not run by bench.py.

    python tools/edge_bench.py --size 256 --iters 20 --rounds 5

The volume holds three nested spheres (labels 1..3, intensities 300 / 600 / 900 plus noise); the signed distances to its K - 1 = 2
interfaces are taken once with ``volume_sharpness.signed_distances`` (timed with a host clock, for the record).  ``edge_profile``
with an ``EdgeWorkspace`` - both launches - is timed with device events around a loop, next to

  torch    per interface: the bin of every voxel with the same float32 arithmetic, ``bucketize`` of it against the bin edges, then
           ``bincount`` four times, three of them with float64 weights (v, s, v * v);
  copy     a device-to-device copy that moves the pass's algorithmic bytes, 4 (J + 1) per voxel, half read and half written,

in alternating order, --rounds times each; the median is reported with the smallest and the largest.  The pass reads the volume only
where a wave has a voxel in range, so it can move fewer bytes than the copy.  Whether torch gives the same counts, and the largest
relative difference of the sums, are reported.  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.benchutil import timed      # noqa: E402

from mri_superresolution_amd import volume_sharpness as V                    # noqa: E402


def stats(t):
    return [round(float(f(t)), 4) for f in (np.median, min, max)]


def torch_profile(vol, sdist, radius, bin_width, nb):
    """The same binning with torch operators: the baseline.  -> (J, nb, 4) float64: count, sum v, sum s, sum v * v."""
    r32 = torch.tensor(float(np.float32(radius)), dtype=torch.float32, device=vol.device)
    w32 = torch.tensor(float(np.float32(bin_width)), dtype=torch.float32, device=vol.device)
    edges = torch.arange(1, nb + 1, dtype=torch.float32, device=vol.device)      # bin b: b <= q < b + 1
    v = vol.reshape(-1)
    out = torch.zeros((sdist.shape[0], nb, 4), dtype=torch.float64, device=vol.device)
    for j in range(sdist.shape[0]):
        s = sdist[j].reshape(-1)
        q = (s + r32) / w32
        ok = torch.isfinite(s) & (q >= 0) & (q < nb) & torch.isfinite(v)
        b = torch.bucketize(q[ok], edges, right=True)
        v64, s64 = v[ok].double(), s[ok].double()
        out[j, :, 0] = torch.bincount(b, minlength=nb)[:nb]
        out[j, :, 1] = torch.bincount(b, weights=v64, minlength=nb)[:nb]
        out[j, :, 2] = torch.bincount(b, weights=s64, minlength=nb)[:nb]
        out[j, :, 3] = torch.bincount(b, weights=v64 * v64, minlength=nb)[:nb]
    return out


def main(args):
    if not torch.cuda.is_available():
        raise SystemExit("this tool measures on an MI355X: no GPU found")
    n, K = args.size, args.classes
    x = np.linspace(-1, 1, n, dtype=np.float32)
    r = np.sqrt(x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2)
    radii = np.linspace(0.92, 0.38, K)
    labels_np = np.zeros(r.shape, dtype=np.uint8)
    for k, radius in enumerate(radii, start=1):
        labels_np[r <= radius] = k
    vol_np = (300.0 * labels_np + np.random.default_rng(0).normal(0.0, 30.0, r.shape)).astype(np.float32)
    labels, vol = torch.from_numpy(labels_np).cuda(), torch.from_numpy(vol_np).cuda()
    voxels, J = vol.numel(), K - 1
    nb = V.check_bins(args.radius, args.bin)[2]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sdist = V.signed_distances(labels, K, args.spacing)
    torch.cuda.synchronize()
    sdist_ms = (time.perf_counter() - t0) * 1e3
    ws = V.EdgeWorkspace(J, nb, "cuda")
    nbytes = 4 * (J + 1) * voxels
    src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    t_k, t_t, t_c = [], [], []
    for _ in range(args.rounds):
        t_k.append(timed(lambda: V.edge_profile(vol, sdist, args.radius, args.bin, ws), args.iters, args.warmup))
        t_t.append(timed(lambda: torch_profile(vol, sdist, args.radius, args.bin, nb), args.torch_iters, 1))
        t_c.append(timed(lambda: dst.copy_(src), args.iters, args.warmup))
    ours = V.profile_of(V.edge_profile(vol, sdist, args.radius, args.bin, ws).cpu().numpy())
    theirs = torch_profile(vol, sdist, args.radius, args.bin, nb).cpu().numpy()
    sums = np.stack([ours.sum_v, ours.sum_s, ours.sum_vv], axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.nanmax(np.where(theirs[..., 1:] != 0, np.abs(sums - theirs[..., 1:]) / np.abs(theirs[..., 1:]), 0.0))
    in_range = float(ours.count.sum()) / (J * voxels)
    found = V.edge_width(ours)
    result = {"size": n, "classes": K, "spacing": list(args.spacing), "radius": args.radius, "bin": args.bin, "bins": nb, "rounds": args.rounds,
              "signed_distances_ms": round(sdist_ms, 3), "share_of_voxels_in_range": round(in_range, 4),
              "edge_profile_ms": stats(t_k), "torch_profile_ms": stats(t_t), "copy_same_bytes_ms": stats(t_c),
              "algorithmic_GBps": round(nbytes / np.median(t_k) / 1e6, 1),
              "share_of_copy_rate": round(float(np.median(t_c) / np.median(t_k)), 3),
              "speedup_over_torch": round(float(np.median(t_t) / np.median(t_k)), 1),
              "torch_gives_the_same_counts": bool(np.array_equal(ours.count, theirs[..., 0].astype(np.int64))),
              "largest_relative_difference_of_the_sums": float(rel),
              "width": [round(float(v), 4) for v in found[0]], "contrast": [round(float(v), 3) for v in found[1]]}
    print(json.dumps(result))
    return 0


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Time the edge-profile pass against torch and a device copy")
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--classes", type=int, default=3)
    p.add_argument("--spacing", type=float, nargs=3, default=[1.0, 1.0, 1.0])
    p.add_argument("--radius", type=float, default=4.0)
    p.add_argument("--bin", type=float, default=0.5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--torch_iters", type=int, default=3)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=5, help="alternating repetitions of every timing")
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
