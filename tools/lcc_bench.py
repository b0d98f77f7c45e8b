#!/usr/bin/env python3
"""Times one demons iteration with the force across contrasts (the warp, the fused force of csrc/volume_lcc.hip and the three
smoothing passes) on a volume of --size^3 at --radius and --sigma.  Not run by bench.py.

    python tools/lcc_bench.py --size 256 --radius 2 --sigma 1.5 --iters 20 --rounds 5

Three comparisons, each timed in alternating order --rounds times, the median reported with the smallest and largest:
  the lcc iteration against the ssd iteration (the parent's four launches) on the same pair;
  the lcc iteration against the same iteration written with torch on the device (grid_sample for the warp, avg_pool3d times the
      count in float64 for the six window sums, conv1d per axis for the smoothing: its own roundings);
  the force kernel alone against a device-to-device copy of its algorithmic bytes: fixed, warped and the three components read,
      three components written, 8 floats per voxel.
Times are device events around --iters back-to-back calls after --warmup.  One JSON line at the end.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from mri_superresolution_amd import _lib as L                                # noqa: E402
from mri_superresolution_amd import volume_deform as D                       # noqa: E402
from mri_superresolution_amd.volume_bias import gaussian_taps                # noqa: E402
from tools.deform_bench import timed                                         # noqa: E402


def torch_lcc_iteration(fixed, moving, u, taps, radius, max_step):
    """The lcc iteration with torch operators (its own roundings and orders)."""
    X, Y, Z = fixed.shape
    idx = torch.stack(torch.meshgrid(*(torch.arange(n, device=u.device, dtype=torch.float32) for n in (X, Y, Z)), indexing="ij"))
    p = idx + u
    grid = torch.stack([2 * (p[2] + 0.5) / Z - 1, 2 * (p[1] + 0.5) / Y - 1, 2 * (p[0] + 0.5) / X - 1], dim=-1)[None]
    warped = F.grid_sample(moving[None, None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0, 0]
    Fd, Md = fixed.double(), warped.double()
    k = 2 * radius + 1
    chans = torch.stack([torch.ones_like(Fd), Fd, Md, Fd * Fd, Md * Md, Fd * Md])[None]
    n, sF, sM, sFF, sMM, sFM = (F.avg_pool3d(chans, k, stride=1, padding=radius, count_include_pad=True) * float(k ** 3))[0]
    mF, mM = sF / n, sM / n
    A, B, C = sFM - mM * sF, sFF - mF * sF, sMM - mM * sM
    ok = (B > 0) & (C > 0) & (A != 0)
    d = torch.where(ok, (Md - mM) * (B / A) - (Fd - mF), torch.zeros_like(A)).float()
    w = torch.where(ok, (A * A / (B * C)).clamp(max=1.0), torch.zeros_like(A)).float()
    g = torch.stack(torch.gradient(fixed))
    den = (g * g).sum(0) + d * d
    s = torch.where(den > 1e-9, d / den, torch.zeros_like(d)) * w
    v = u + (-(s * g)).clamp(-max_step, max_step)
    r = (taps.numel() - 1) // 2
    for axis in (3, 2, 1):
        x = v.movedim(axis, -1).reshape(-1, 1, v.shape[axis])
        x = F.conv1d(F.pad(x, (r, r), mode="replicate"), taps.view(1, 1, -1))
        v = x.reshape(*v.movedim(axis, -1).shape).movedim(-1, axis)
    return v


def main(args):
    if not torch.cuda.is_available():
        raise SystemExit("this tool measures on an MI355X: no GPU found")
    n = args.size
    rng = np.random.default_rng(0)
    x = np.linspace(-1, 1, n, dtype=np.float32)
    base = 600 * np.exp(-2 * (x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2)).astype(np.float32)
    fixed = torch.from_numpy(base + rng.normal(0, 5, base.shape).astype(np.float32)).cuda()
    moving = (900.0 - 0.7 * torch.roll(fixed, (1, -1, 1), (0, 1, 2))).contiguous()             # the other contrast
    u = torch.from_numpy(rng.uniform(-1.5, 1.5, (3, n, n, n)).astype(np.float32)).cuda()
    ws_lcc = D.DeformWorkspace(fixed.shape, fixed.device, levels=1, iterations=1, sigma_vox=args.sigma, force="lcc", lcc_radius=args.radius)
    ws_ssd = D.DeformWorkspace(fixed.shape, fixed.device, levels=1, iterations=1, sigma_vox=args.sigma)
    for ws in (ws_lcc, ws_ssd):
        ws.field(0, 0).copy_(u)
    taps = torch.from_numpy(gaussian_taps(args.sigma)).cuda()
    a, b, warped = ws_lcc.field(0, 0), ws_lcc.field(1, 0), ws_lcc.scratch(0)
    D.warp(moving, a, "linear", float("nan"), out=warped)
    nbytes = 32 * fixed.numel()
    src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")

    def force_only():
        L.call("mrisr_f32_volume_lcc_force", fixed.data_ptr(), warped.data_ptr(), a.data_ptr(), n, n, n, args.radius, 2.0, 1.0, 0,
               b.data_ptr(), ws_lcc.slots.data_ptr(), L.ptr(None), L.stream_ptr(), nbytes=nbytes)

    cases = {"lcc_iteration_ms": lambda: D._iterate(ws_lcc, 0, fixed, moving, 1, 0, 2.0, 0.0),
             "ssd_iteration_ms": lambda: D._iterate(ws_ssd, 0, fixed, moving, 1, 0, 2.0, 0.0),
             "torch_lcc_iteration_ms": lambda: torch_lcc_iteration(fixed, moving, u, taps, args.radius, 2.0),
             "lcc_force_ms": force_only, "copy_same_bytes_ms": lambda: dst.copy_(src)}
    times = {name: [] for name in cases}
    with torch.no_grad():
        for _ in range(args.rounds):
            for name, fn in cases.items():
                slow = name.startswith("torch")
                times[name].append(timed(fn, max(args.iters // 5, 2) if slow else args.iters, 2 if slow else args.warmup))
    med = {name: float(np.median(t)) for name, t in times.items()}
    result = {"size": n, "radius": args.radius, "sigma": args.sigma, "rounds": args.rounds,
              **{name: [round(f(t), 4) for f in (np.median, min, max)] for name, t in times.items()},
              "lcc_over_ssd": round(med["lcc_iteration_ms"] / med["ssd_iteration_ms"], 3),
              "speedup_over_torch": round(med["torch_lcc_iteration_ms"] / med["lcc_iteration_ms"], 2),
              "lcc_force_GBps": round(nbytes / med["lcc_force_ms"] / 1e6, 1),
              "lcc_force_share_of_copy_rate": round(med["copy_same_bytes_ms"] / med["lcc_force_ms"], 3)}
    print(json.dumps(result))
    return 0


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Time the demons iteration with the correlation force against the ssd iteration, torch and a copy")
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--radius", type=int, default=2)
    p.add_argument("--sigma", type=float, default=1.5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=5)
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
