#!/usr/bin/env python3
"""Times the kernels of the tissue classification (csrc/volume_tissue.hip) on a volume of --size^3 and a whole segment_tissue against
the same loop written with torch operators on the device.  Not run by bench.py.

    python tools/tissue_bench.py --size 256 --iters 50 --rounds 5

The quantise pass, the joint histogram and one half-sweep are timed with device events around --iters back-to-back launches after
--warmup, each next to a device-to-device copy of its algorithmic bytes, in alternating order, --rounds times each; the median is
reported with the smallest and the largest.  Algorithmic bytes per voxel: quantise 7 (the float32 volume and the mask read, the bins and
the seed written), joint histogram 2 (bins and labels read), half-sweep 1.5 (the labels and the bins of the colour's half read; the
neighbouring rows come from cache, the labels that change are written on top).  The half-sweep is bound by byte-granular work per
voxel, not by HBM: its share of the copy rate is reported, not tuned to.

segment_tissue (K = --classes, --iterations, beta 1) is timed with a host clock around the call, which ends in a synchronisation,
against the same driver with the voxel work in torch: a gather of the cost table and six shifted comparisons per class for a
half-sweep, bincount for the histograms.  Whether both produce the same labels is reported.  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.benchutil import timed      # noqa: E402

from mri_superresolution_amd import volume_tissue as T                       # noqa: E402
from mri_superresolution_amd.volume_intensity import RANGE, masked_percentiles     # noqa: E402


def stats(t):
    return [round(float(f(t)), 4) for f in (np.median, min, max)]


class TorchBackend:
    """The steps of volume_tissue._drive with torch operators (the baseline): the same integers, other launches."""

    def __init__(self, vol, mask, K):
        self.vol, self.mask, self.K = vol, mask != 0, K
        i, j, k = torch.meshgrid(*(torch.arange(n, device=vol.device) for n in vol.shape), indexing="ij")
        self.parity = (i + j + k) & 1

    def quantise(self):
        marks, _ = masked_percentiles(self.vol, self.mask, RANGE)
        lo, hi = (float(x) for x in marks.cpu().numpy())
        scale, degenerate = T._range_scale(lo, hi)
        pos = (self.vol - marks[0]) * float(scale) if not degenerate else torch.zeros_like(self.vol)
        self.q = pos.clamp(0, 255).long()
        self.labels = self.mask.to(torch.uint8)
        return lo, hi, torch.bincount(self.q[self.mask], minlength=256).cpu().numpy()

    def half(self, cost, beta_q, colour):
        p = F.pad(self.labels, (1, 1, 1, 1, 1, 1))
        nb = [p[:-2, 1:-1, 1:-1], p[2:, 1:-1, 1:-1], p[1:-1, :-2, 1:-1], p[1:-1, 2:, 1:-1], p[1:-1, 1:-1, :-2], p[1:-1, 1:-1, 2:]]
        nonzero = sum((n != 0).long() for n in nb)
        best = None
        for k in range(self.K):
            e = (cost[k][self.q] + beta_q * (nonzero - sum((n == k + 1).long() for n in nb))) * 8 + (k + 1)      # ties: the smaller class
            best = e if best is None else torch.minimum(best, e)
        update = self.mask & (self.parity == colour)
        self.labels = torch.where(update, (best & 7).to(torch.uint8), self.labels)

    def sweep(self, cost, beta_q):
        before = self.labels
        table = torch.from_numpy(cost).to(self.vol.device).long()
        for colour in (0, 1):
            self.half(table, beta_q, colour)
        changed = int((self.labels != before).sum())
        cell = (self.labels[self.mask].long() - 1) * 256 + self.q[self.mask]
        return changed, torch.bincount(cell, minlength=self.K * 256).cpu().numpy().reshape(self.K, 256)


def main(args):
    if not torch.cuda.is_available():
        raise SystemExit("this tool measures on an MI355X: no GPU found")
    n, K = args.size, args.classes
    rng = np.random.default_rng(0)
    x = np.linspace(-1, 1, n, dtype=np.float32)
    r = np.sqrt(x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2)
    clean = np.select([r <= 0.38, r <= 0.66, r <= 0.92], [740.0, 520.0, 300.0], 0.0).astype(np.float32)
    vol = torch.from_numpy(np.where(clean > 0, clean + rng.normal(0, 60, clean.shape), 0).astype(np.float32)).cuda()
    mask = torch.from_numpy((clean > 0).astype(np.uint8)).cuda()
    voxels = vol.numel()
    ws = T.TissueWorkspace(vol.shape, K, vol.device)
    found = T.segment_tissue(vol, mask, K, 1.0, args.iterations, workspace=ws)      # leaves bins, labels and a table in the workspace
    marks, _ = masked_percentiles(vol, mask, RANGE)
    labels0 = ws.labels.clone()
    found = found._replace(labels=labels0)                                          # the workspace's labels are overwritten below

    def half():
        T._icm_half_launch(ws.q, ws.labels, ws.shape, K, ws.cost, 65536, 0, ws.counters[0:1])

    kernels = {"quantise": (lambda: T._quantise(vol, mask, marks, ws.q, ws.labels, ws.counters[2:258], ws.counters[1:2]), 7.0),
               "joint_hist": (lambda: T._joint_hist(ws.q, ws.labels, K, ws.counters[258:]), 2.0),
               "icm_half": (half, 1.5)}
    result = {"size": n, "classes": K, "iterations": args.iterations, "rounds": args.rounds, "masked_share": round(float(mask.sum()) / voxels, 4)}
    for name in ("joint_hist", "icm_half", "quantise"):      # quantise last: it overwrites the labels with the seed
        fn, per_voxel = kernels[name]
        nbytes = int(per_voxel * voxels)
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        t_k, t_c = [], []
        for _ in range(args.rounds):
            if name == "icm_half":
                ws.labels.copy_(labels0)
            t_k.append(timed(fn, args.iters, args.warmup))
            t_c.append(timed(lambda: dst.copy_(src), args.iters, args.warmup))      # nbytes / 2 read and nbytes / 2 written
        result.update({f"{name}_ms": stats(t_k), f"{name}_GBps": round(nbytes / np.median(t_k) / 1e6, 1),
                       f"{name}_copy_same_bytes_ms": stats(t_c), f"{name}_share_of_copy_rate": round(float(np.median(t_c) / np.median(t_k)), 3)})
    t_dev, t_torch, same = [], [], True
    for _ in range(args.segment_rounds):
        for times, run in ((t_dev, lambda: T.segment_tissue(vol, mask, K, 1.0, args.iterations, workspace=ws)),
                           (t_torch, lambda: T._drive(TorchBackend(vol, mask, K), K, 65536, args.iterations))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            same = same and torch.equal(out.labels, found.labels) and out.sweeps == found.sweeps
    result.update({"sweeps": found.sweeps, "torch_loop_gives_the_same_labels": bool(same), "segment_ms": stats(t_dev), "torch_segment_ms": stats(t_torch),
                   "speedup_over_torch": round(float(np.median(t_torch) / np.median(t_dev)), 2)})
    print(json.dumps(result))
    return 0


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Time the tissue-classification kernels against device copies and segment_tissue against torch")
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--classes", type=int, default=3)
    p.add_argument("--iterations", type=int, default=20)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rounds", type=int, default=5, help="alternating repetitions of every kernel timing")
    p.add_argument("--segment_rounds", type=int, default=3, help="alternating repetitions of the two whole segmentations")
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
