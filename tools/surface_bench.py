#!/usr/bin/env python3
"""Times the distance transform of csrc/volume_surface.hip on label boundaries of a --size^3 volume against the same three passes
written with torch operators on the device, and a whole surface_distances.  Not run by bench.py.

    python tools/surface_bench.py --size 256 --iters 20 --rounds 5

The volume holds three nested ellipsoidal shells (labels 1..3); the second label volume is the first moved by two voxels.  The sites
of the transform are the boundary voxels of one class, as in surface_distances.  Every pass of the transform is timed alone with
device events around the launch, its input restored before each launch (a pass works in place), next to a device-to-device copy of
its algorithmic bytes, in alternating order, --rounds times each; the median is reported with the smallest and the largest.
Algorithmic bytes per voxel: the pass along axis 2 reads the bytes and writes floats (5), the two others read and write floats (8).
A pass is bound by the candidates it visits, not by HBM: its share of the copy rate is reported, not tuned to.  Each pass is also
timed in the form that visits every candidate of a line (full_scan): the walk that stops early is kept only while it is faster.

The whole transform is timed back to back against the torch formulation: per axis a chunked broadcast (g[:, None, :] + T).amin(-1)
over the lines; whether both give the same bits is reported.  surface_distances (K = --classes, both directions, all classes, one
download) is timed with a host clock around the call.  One JSON line at the end.
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

from mri_superresolution_amd import volume_surface as S                      # noqa: E402
from mri_superresolution_amd._volume_args import check_spacing               # noqa: E402


def timed(fn, iters, warmup, prepare=None):
    """ms per call: device events around every call on its own when ``prepare`` runs before each, around the whole loop otherwise."""
    for _ in range(warmup):
        if prepare:
            prepare()
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    if prepare is None:
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / iters
    total = 0.0
    for _ in range(iters):
        prepare()
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        total += start.elapsed_time(stop)
    return total / iters


def stats(t):
    return [round(float(f(t)), 4) for f in (np.median, min, max)]


def torch_edt_sq(sites, value, weights, chunk_bytes=1 << 30):
    """The three passes with torch operators: the baseline."""
    g = torch.where(sites == value, 0.0, float("inf")).to(torch.float32)
    for axis in (2, 1, 0):
        n = g.shape[axis]
        d = torch.arange(n, device=g.device)
        table = (torch.tensor(float(weights[axis]), dtype=torch.float32, device=g.device) * ((d * d).to(torch.float32)))
        T = table[(d[:, None] - d[None, :]).abs()]                     # (i, j)
        lines = g.movedim(axis, -1).reshape(-1, n)
        out = torch.empty_like(lines)
        step = max(1, chunk_bytes // (4 * n * n))
        for lo in range(0, lines.shape[0], step):
            out[lo:lo + step] = (lines[lo:lo + step, None, :] + T[None]).amin(dim=-1)
        g = out.reshape(g.movedim(axis, -1).shape).movedim(-1, axis).contiguous()
    return g


def main(args):
    if not torch.cuda.is_available():
        raise SystemExit("this tool measures on an MI355X: no GPU found")
    n, K = args.size, args.classes
    x = np.linspace(-1, 1, n, dtype=np.float32)
    r = np.sqrt(x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2)
    a_np = np.select([r <= 0.38, r <= 0.66, r <= 0.92], [3, 2, 1], 0).astype(np.uint8)
    a = torch.from_numpy(a_np).cuda()
    b = torch.from_numpy(np.roll(a_np, 2, axis=0)).cuda()
    voxels = a.numel()
    w = check_spacing(args.spacing)
    sites = S.label_boundary(b)
    value = 2
    out = torch.empty(a.shape, dtype=torch.float32, device="cuda")
    states = {}                                                        # the volume after the pass along an axis
    S._edt_launch(sites, a.shape, value, w, out, passes=4)
    states[2] = out.clone()
    S._edt_launch(sites, a.shape, value, w, out, passes=2)
    states[1] = out.clone()
    S._edt_launch(sites, a.shape, value, w, out, passes=1)
    whole = S.distance_transform_sq(sites, value, w)
    result = {"size": n, "classes": K, "spacing": list(args.spacing), "rounds": args.rounds,
              "site_share": round(float((sites == value).sum()) / voxels, 5),
              "passes_alone_give_the_transform": bool(torch.equal(out.view(torch.int32), whole.view(torch.int32)))}
    for axis, mask, per_voxel in ((2, 4, 5), (1, 2, 8), (0, 1, 8)):
        nbytes = per_voxel * voxels
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        prepare = None if axis == 2 else (lambda axis=axis: out.copy_(states[axis + 1]))      # what the pass before left
        t_k, t_f, t_c = [], [], []
        for _ in range(args.rounds):
            t_k.append(timed(lambda: S._edt_launch(sites, a.shape, value, w, out, passes=mask), args.iters, args.warmup, prepare))
            t_f.append(timed(lambda: S._edt_launch(sites, a.shape, value, w, out, passes=mask, full_scan=True), args.iters, args.warmup, prepare))
            t_c.append(timed(lambda: dst.copy_(src), args.iters, args.warmup))      # nbytes / 2 read and nbytes / 2 written
        result.update({f"axis{axis}_ms": stats(t_k), f"axis{axis}_full_scan_ms": stats(t_f), f"axis{axis}_copy_same_bytes_ms": stats(t_c),
                       f"axis{axis}_share_of_copy_rate": round(float(np.median(t_c) / np.median(t_k)), 3)})
    t_dev, t_full, t_torch = [], [], []
    for _ in range(args.rounds):
        t_dev.append(timed(lambda: S._edt_launch(sites, a.shape, value, w, out), args.iters, args.warmup))
        t_full.append(timed(lambda: S._edt_launch(sites, a.shape, value, w, out, full_scan=True), args.iters, args.warmup))
        t_torch.append(timed(lambda: torch_edt_sq(sites, value, w), args.torch_iters, 1))
    same = torch.equal(torch_edt_sq(sites, value, w).view(torch.int32), whole.view(torch.int32))
    result.update({"edt_ms": stats(t_dev), "edt_full_scan_ms": stats(t_full), "torch_edt_ms": stats(t_torch),
                   "torch_gives_the_same_bits": bool(same), "edt_speedup_over_torch": round(float(np.median(t_torch) / np.median(t_dev)), 1)})
    ws = S.SurfaceWorkspace(a.shape, K, "cuda")
    t_all = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found = S.surface_distances(a, b, K, args.spacing, True, ws)
        t_all.append((time.perf_counter() - t0) * 1e3)
    result.update({"surface_distances_ms": stats(t_all), "assd": [round(float(v), 6) for v in found.assd],
                   "hd95": [round(float(v), 6) for v in found.hd95], "hd": [round(float(v), 6) for v in found.hd]})
    print(json.dumps(result))
    return 0


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Time the distance transform against torch and a whole surface_distances")
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--classes", type=int, default=3)
    p.add_argument("--spacing", type=float, nargs=3, default=[1.0, 1.0, 1.0])
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--torch_iters", type=int, default=2)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=5, help="alternating repetitions of every timing")
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
