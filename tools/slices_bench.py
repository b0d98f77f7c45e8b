#!/usr/bin/env python3
"""Times the kernels of the slice-to-volume motion correction (csrc/volume_slices.hip).  Not run by bench.py.

    python tools/slices_bench.py --size 256 --slices 64 --samples 4 --iters 20 --rounds 5

The output is --size^3; the three stacks are size x size x slices voxels, thick along a different axis each, box profile with
--samples samples; every slice has a small pose of its own.  Timed with device events around a loop, in alternating order, --rounds
times each; the median is reported with the smallest and the largest:

  cost           the slice-cost launches of one stack at C = 13, stride 1 (``mrisr_f32_volume_slice_cost``, the candidates on the device);
  residual_x13   13 launches of the existing stack-wide residual kernel on that stack: the same forward-model work without the sums;
  torch_x13      13 times ``affine_grid`` + ``grid_sample`` of that stack's T samples with torch;
  update_slices  the per-slice update launch for the three stacks;
  update         the plain update launch on stack-wide matrices;
  search_iter    one whole search iteration of one stack at stride 1: 12 x S ``slice_geometries`` on the host, the upload, the launches
                 and the device-to-host read of the sums.

One JSON line at the end.
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
from tools.stacks_bench import stats, torch_iteration      # noqa: E402

from mri_superresolution_amd import volume_slices as V                       # noqa: E402
from mri_superresolution_amd import volume_stacks as S                       # noqa: E402


def main(args):
    if not torch.cuda.is_available():
        raise SystemExit("this tool measures on an MI355X: no GPU found")
    n, ns, T, C = args.size, args.slices, args.samples, V.MAX_CANDIDATES
    rng = np.random.default_rng(0)
    stacks, geometries, affines, poses = [], [], [], []
    for axis in range(3):
        shape = tuple(ns if a == axis else n for a in range(3))
        affine = np.eye(4)
        affine[axis, axis] = n / ns
        affine[axis, 3] = 0.5 * (n / ns - 1.0)
        affines.append(affine)
        geometries.append(S.stack_geometry(affine, np.eye(4), axis, "box", samples=T))
        stacks.append(torch.from_numpy(rng.uniform(0, 900, shape).astype(np.float32)).cuda())
        poses.append(rng.uniform(-1.0, 1.0, (ns, 6)))
    ws = S.StackWorkspace((n, n, n), [y.shape for y in stacks], "cuda", 2, motion=True)
    ws.x.copy_(torch.from_numpy(rng.uniform(0, 900, (n, n, n)).astype(np.float32)))
    for k in range(3):
        M, N = V.slice_geometries(affines[k], np.eye(4), stacks[k].shape, k, poses[k])
        ws.to_tables[k][:ns].copy_(torch.from_numpy(M.reshape(ns, 12)))
        ws.from_tables[k][:ns].copy_(torch.from_numpy(N.reshape(ns, 12)))
        S._residual(ws.x, stacks[k], geometries[k], ws.residuals[k], ws.region(k), None)
    from_tables = [t[:ns] for t in ws.from_tables]
    y, g = stacks[2], geometries[2]
    cands = np.repeat(poses[2][:, None, :], C, axis=1) + rng.uniform(-0.5, 0.5, (ns, C, 6))
    cand = np.stack([V.slice_geometries(affines[2], np.eye(4), y.shape, 2, cands[:, c])[0] for c in range(C)], axis=1)
    V.slice_cost(ws.x, y, g, cand, 1, ws.cost)                             # the candidates lie in the workspace from here on
    table, out = ws.cost.cand[:ns * C * 12], ws.cost.out[:ns * C * 6]

    def cost():
        S.L.call("mrisr_f32_volume_slice_cost", ws.x.data_ptr(), *ws.x.shape, y.data_ptr(), *y.shape, table.data_ptr(), ns, C, 2,
                 *S._profile_args(g), 1, ws.cost.slots.data_ptr(), out.data_ptr(), S.L.stream_ptr())

    def residual_x13():
        for _ in range(C):
            S._residual(ws.x, y, g, ws.residuals[2], ws.region(2), None)

    def torch_x13():
        for _ in range(C):
            torch_iteration(ws.x, [y], [g], 1.0)

    def search_iter():
        tabs = np.stack([V.slice_geometries(affines[2], np.eye(4), y.shape, 2, cands[:, c])[0] for c in range(12)], axis=1)
        return V.slice_cost(ws.x, y, g, tabs, 1, ws.cost).cpu().numpy()

    lo = np.float32(0)
    scratch = torch.empty_like(ws.x)
    t = {k: [] for k in ("cost", "residual_x13", "torch_x13", "update_slices", "update", "search_iter")}
    for _ in range(args.rounds):
        t["cost"].append(timed(cost, args.iters, args.warmup))
        t["residual_x13"].append(timed(residual_x13, args.iters, args.warmup))
        t["update_slices"].append(timed(lambda: V._update_slices(ws.x, ws.residuals, geometries, from_tables, 1.0, lo, scratch, None, None, None),
                                        args.iters, args.warmup))
        t["update"].append(timed(lambda: S._update(ws.x, ws.residuals, geometries, 1.0, lo, scratch, None, None, None), args.iters, args.warmup))
        t["torch_x13"].append(timed(torch_x13, args.torch_iters, 1))
        torch.cuda.synchronize()
        begin = time.perf_counter()
        for _ in range(args.search_iters):
            search_iter()
        t["search_iter"].append((time.perf_counter() - begin) * 1e3 / args.search_iters)      # host wall time: it ends with a read
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps({"size": n, "slices": ns, "samples": T, "candidates": C, "rounds": args.rounds, "cost_ms": stats(t["cost"]),
                      "residual_x13_ms": stats(t["residual_x13"]), "torch_x13_ms": stats(t["torch_x13"]),
                      "update_slices_ms": stats(t["update_slices"]), "update_ms": stats(t["update"]), "search_iteration_ms": stats(t["search_iter"]),
                      "cost_over_residual_x13": round(med["cost"] / med["residual_x13"], 3),
                      "cost_speedup_over_torch": round(med["torch_x13"] / med["cost"], 2),
                      "update_slices_over_update": round(med["update_slices"] / med["update"], 3)}))
    return 0


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Time the kernels of the slice-to-volume motion correction")
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--slices", type=int, default=64)
    p.add_argument("--samples", type=int, default=4)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--torch_iters", type=int, default=2)
    p.add_argument("--search_iters", type=int, default=3)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=5, help="alternating repetitions of every timing")
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
