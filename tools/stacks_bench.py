#!/usr/bin/env python3
"""Times one iteration of the reconstruction from orthogonal stacks (csrc/volume_stacks.hip) and each of its two kernels alone against
the same iteration written with torch operators and against device copies of the kernels' algorithmic bytes.  Not run by bench.py.

    python tools/stacks_bench.py --size 256 --slices 64 --samples 4 --iters 20 --rounds 5

The output is --size^3; the three stacks are size x size x slices voxels, thick along a different axis each, box profile with
--samples samples.  Timed with device events around a loop, in alternating order, --rounds times each; the median is reported with
the smallest and the largest:

  iteration   K residual launches and the update (``volume_stacks._iterate`` with ``_launchers`` on a ``StackWorkspace``);
  residual    the residual launch of one stack (the median over the three stacks is reported per stack);
  update      the update launch alone;
  torch       the same iteration with ``affine_grid`` + ``grid_sample`` (trilinear, border padding): per stack T sampled volumes,
              their mean, the difference; then K sampled residuals, their mean, the step and the clamp;
  copy        device-to-device copies that move each kernel's algorithmic bytes (every tensor read or written once).

With --regularise the same run also times, alternating with the plain ones in every round:

  update_reg     the regularised update launch alone (``mrisr_f32_volume_stack_update_reg``: lambda 0.03, delta 60, unit coefficients,
                 the coverage counts of the stacks), from one estimate into the other;
  iteration_reg  the regularised iteration (``volume_stacks._iterate`` on a ``StackWorkspace(..., regularised=True)``), an even and
                 an odd one in turn: half the time of the pair is reported;
  torch_reg      the torch iteration with the same prior written with shifted slices (replicated faces: a difference of 0), ``clamp``
                 for the clip.

One JSON line at the end.
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

from tools.benchutil import timed      # noqa: E402

from mri_superresolution_amd import volume_stacks as S                       # noqa: E402


def stats(t):
    return [round(float(f(t)), 4) for f in (np.median, min, max)]


def theta(m, src_shape, dst_shape):
    """The (1, 3, 4) matrix of ``affine_grid`` (align_corners=False, coordinates x = z index, y, z = x index, normalised) for the
    index matrix ``m``: destination index -> source index."""
    def norm(n):                                              # index -> normalised: (2 i + 1) / n - 1
        a = np.eye(4)
        for d in range(3):
            a[d, d], a[d, 3] = 2.0 / n[d], 1.0 / n[d] - 1.0
        return a
    full = norm(src_shape) @ np.vstack([m, [0, 0, 0, 1]]) @ np.linalg.inv(norm(dst_shape))
    flip = np.eye(4)[[2, 1, 0, 3]]
    return torch.from_numpy((flip @ full @ flip)[:3]).float().unsqueeze(0).cuda()


def torch_prior(x, delta):
    """The sum over the six face neighbours of the clipped differences (unit coefficients, every voxel covered)."""
    reg = torch.zeros_like(x)
    for a in range(3):
        lo, hi = x.narrow(a, 0, x.shape[a] - 1), x.narrow(a, 1, x.shape[a] - 1)
        d = (hi - lo).clamp_(-delta, delta)
        reg.narrow(a, 0, x.shape[a] - 1).add_(d)
        reg.narrow(a, 1, x.shape[a] - 1).sub_(d)
    return reg


def torch_iteration(x, stacks, geometries, step, lam=0.0, delta=float("inf")):
    res = []
    for y, g in zip(stacks, geometries):
        acc = torch.zeros_like(y)
        for o, w in zip(g.offsets, g.weights):
            m = g.to_output.copy()
            m[:, 3] += m[:, g.slice_axis] * o
            grid = F.affine_grid(theta(m, x.shape, y.shape), (1, 1) + tuple(y.shape), align_corners=False)
            acc = acc + float(w) * F.grid_sample(x[None, None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0, 0]
        res.append(y - acc)
    total = torch.zeros_like(x)
    for r, g in zip(res, geometries):
        grid = F.affine_grid(theta(g.from_output, r.shape, x.shape), (1, 1) + tuple(x.shape), align_corners=False)
        total = total + F.grid_sample(r[None, None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0, 0]
    if lam > 0:
        return (x + step * (total / len(res) + lam * torch_prior(x, delta))).clamp_(min=0)
    return (x + step * (total / len(res))).clamp_(min=0)


def main(args):
    if not torch.cuda.is_available():
        raise SystemExit("this tool measures on an MI355X: no GPU found")
    n, ns, T = args.size, args.slices, args.samples
    out_shape = (n, n, n)
    rng = np.random.default_rng(0)
    stacks, geometries = [], []
    for axis in range(3):
        shape = tuple(ns if a == axis else n for a in range(3))
        affine = np.eye(4)
        affine[axis, axis] = n / ns
        affine[axis, 3] = 0.5 * (n / ns - 1.0)
        geometries.append(S.stack_geometry(affine, np.eye(4), axis, "box", samples=T))
        stacks.append(torch.from_numpy(rng.uniform(0, 900, shape).astype(np.float32)).cuda())
    ws = S.StackWorkspace(out_shape, [y.shape for y in stacks], "cuda", 2, regularised=args.regularise)
    ws.x.copy_(torch.from_numpy(rng.uniform(0, 900, out_shape).astype(np.float32)))
    x0 = ws.x.clone()
    voxels, sv = n ** 3, n * n * ns
    res_bytes, upd_bytes = 4 * (voxels + 2 * sv), 4 * (2 * voxels + 3 * sv)
    buf = torch.empty(max(res_bytes, upd_bytes) // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(buf)
    t = {k: [] for k in ("iteration", "residual", "update", "torch", "copy_residual", "copy_update")}
    lo = np.float32(0)
    plain = S._launchers(ws, stacks, geometries, 1.0, lo)
    if args.regularise:
        t.update({k: [] for k in ("iteration_reg", "update_reg", "torch_reg")})
        lam, delta = 0.03, 60.0
        reg = S._check_regulariser(1.0, lam, delta, None)
        regularised = S._launchers(ws, stacks, geometries, 1.0, lo, reg)
        S._update(ws.x, stacks, geometries, 1.0, lo, ws.x2, ws.cover, None, None)      # the coverage counts: geometry only
        ws.x.copy_(x0)
    for _ in range(args.rounds):
        if args.regularise:
            t["iteration_reg"].append(0.5 * timed(lambda: S._iterate(ws, 0, 2, *regularised), args.iters, args.warmup))
            ws.x.copy_(x0)
        t["iteration"].append(timed(lambda: S._iterate(ws, 0, 1, *plain), args.iters, args.warmup))
        per = [timed(lambda k=k: S._residual(ws.x, stacks[k], geometries[k], ws.residuals[k], ws.region(k), None), args.iters, args.warmup)
               for k in range(3)]
        t["residual"].append(float(np.median(per)))
        t["update"].append(timed(lambda: S._update(ws.x, ws.residuals, geometries, 1.0, np.float32(0), ws.x, None, None, None), args.iters,
                                 args.warmup))
        if args.regularise:
            t["update_reg"].append(timed(lambda: S._update_reg(ws.x, ws.residuals, geometries, 1.0, lo, reg, ws.cover, ws.x2, None, None, None),
                                         args.iters, args.warmup))
            t["torch_reg"].append(timed(lambda: torch_iteration(x0, stacks, geometries, 1.0, lam, delta), args.torch_iters, 1))
        t["torch"].append(timed(lambda: torch_iteration(x0, stacks, geometries, 1.0), args.torch_iters, 1))
        t["copy_residual"].append(timed(lambda: dst[:res_bytes // 2].copy_(buf[:res_bytes // 2]), args.iters, args.warmup))
        t["copy_update"].append(timed(lambda: dst[:upd_bytes // 2].copy_(buf[:upd_bytes // 2]), args.iters, args.warmup))
    ws.x.copy_(x0)
    S._iterate(ws, 0, 1, *plain)
    theirs = torch_iteration(x0, stacks, geometries, 1.0)
    diff = float((ws.x - theirs).abs().max())
    med = {k: float(np.median(v)) for k, v in t.items()}
    result = {"size": n, "slices": ns, "samples": T, "rounds": args.rounds, "iteration_ms": stats(t["iteration"]),
              "residual_ms_per_stack": stats(t["residual"]), "update_ms": stats(t["update"]), "torch_iteration_ms": stats(t["torch"]),
              "copy_residual_bytes_ms": stats(t["copy_residual"]), "copy_update_bytes_ms": stats(t["copy_update"]),
              "speedup_over_torch": round(med["torch"] / med["iteration"], 2),
              "residual_share_of_copy_rate": round(med["copy_residual"] / med["residual"], 3),
              "update_share_of_copy_rate": round(med["copy_update"] / med["update"], 3),
              "iteration_share_of_copy_rate": round((3 * med["copy_residual"] + med["copy_update"]) / med["iteration"], 3),
              "largest_difference_from_torch": diff}
    if args.regularise:
        ws.x.copy_(x0)
        S._iterate(ws, 0, 1, *regularised)
        result.update({"reg_lambda": lam, "reg_delta": delta, "iteration_reg_ms": stats(t["iteration_reg"]),
                       "update_reg_ms": stats(t["update_reg"]), "torch_reg_iteration_ms": stats(t["torch_reg"]),
                       "update_reg_over_update": round(med["update_reg"] / med["update"], 3),
                       "iteration_reg_over_iteration": round(med["iteration_reg"] / med["iteration"], 3),
                       "reg_speedup_over_torch": round(med["torch_reg"] / med["iteration_reg"], 2),
                       "largest_reg_difference_from_torch": float((ws.x2 - torch_iteration(x0, stacks, geometries, 1.0, lam, delta)).abs().max())})
    print(json.dumps(result))
    return 0


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Time an iteration of the stack reconstruction against torch and device copies")
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--slices", type=int, default=64)
    p.add_argument("--samples", type=int, default=4)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--torch_iters", type=int, default=3)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=5, help="alternating repetitions of every timing")
    p.add_argument("--regularise", action="store_true", help="also time the regularised update launch and iteration, alternating with the plain ones")
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
