#!/usr/bin/env python3
"""Cost of the registration cost function (csrc/volume_register.hip) next to the same work written with torch.

    python tools/register_bench.py [--reps 20] [--warmup 3] [--inner 5] [--size 256] [--skip_torch] [--variant_libs name=path ...]
    python tools/register_bench.py --global_init [--reps 20] [--warmup 3] [--inner 5] [--size 256]

A 12-candidate evaluation - the unit of ``volume_register.compass_search`` - on a ``--size``^3 float32 phantom against a rotated,
shifted, contrast-inverted copy: ``joint_histogram`` of the 12 probe matrices around a point plus ``nmi``, at strides 4 and 2 with
64 bins.  HIP events around ``--inner`` back-to-back evaluations after warm-up, the median over ``--reps`` such windows, per
evaluation (no read-back inside the window); ``search_step_us`` adds the one read of the 12 values a search iteration makes
(wall clock).  The torch path does the same work per candidate - ``F.affine_grid`` + ``F.grid_sample`` (trilinear) on the strided
sample grid, the two bins, ``torch.bincount`` - and alternates with the kernel in one loop, so that the ratio is taken on one
box in one run; its histograms are compared with the kernel's by total count only (torch pads with zeros, rounds the
coordinates in float32 and has no inside test).  ``--variant_libs``: other builds of libmrisr.so (``-DMRISR_REGISTER_KLOOP=1``: a
workgroup loops over all candidates instead of serving one) join the alternation through ctypes; ``raw`` is this build's entry
called the same way.  ``registration``: the wall time of one whole ``register_rigid`` of the pair and what it found.
``--global_init`` times what ``register_rigid(init="global", mask_cost=True)`` adds instead: the 125-candidate coarse stage
(8 chunks of 16 ``joint_histogram`` + ``nmi`` launches at stride 4, no read-back inside the window) and one 12-candidate
evaluation at strides 4 and 2, each with the fixed-side mask in the cost and without, alternating in one loop.  The mask is an
ellipsoid that fills about 25 % of the box; ``mask_moments`` of it is timed as well.
Prints one JSON line (profiles/NOTES.md, "Register")."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.benchutil import alternating_times_fine as alternating_times      # noqa: E402

BINS = 64


def phantom(n, device):
    """Smooth blobs in [0, 1] on an n^3 grid plus noise: anatomy-like runs of equal histogram cells."""
    g = torch.Generator(device=device).manual_seed(0)
    ax = torch.linspace(-1, 1, n, device=device)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    v = 0.55 * torch.exp(-((x / 0.75) ** 4 + (y / 0.85) ** 4 + (z / 0.8) ** 4))
    for cx, cy, cz, s, a in ((0.3, 0.2, -0.15, 0.25, 0.45), (-0.35, -0.3, 0.25, 0.2, 0.35), (0.1, -0.45, -0.4, 0.15, -0.3),
                             (-0.2, 0.4, 0.1, 0.3, 0.25)):
        v = v + a * torch.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (2 * s * s))
    return (v.clamp_min(0) + 0.01 * torch.randn(v.shape, device=device, generator=g)).contiguous()


def torch_theta(m, src, dst, device):
    """tools/reslice_bench.py's theta of ``F.affine_grid(align_corners=False)`` for the index matrix ``m``."""
    S, D = np.array(src, dtype=np.float64), np.array(dst, dtype=np.float64)
    lin = m[:, :3] * D[None, :] / S[:, None]
    off = (m[:, :3] @ (D - 1) + 2 * m[:, 3] + 1) / S - 1
    theta = np.hstack([lin[::-1, ::-1], off[::-1, None]])
    return torch.tensor(theta[None], dtype=torch.float32, device=device)


def ellipsoid_mask(n, device, semi=0.78):
    """uint8 n^3: an ellipsoid with semi-axes ``semi`` of the half extent (pi / 6 * 0.78^3 = 24.8 % of the box)."""
    ax = torch.linspace(-1, 1, n, device=device)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return ((x * x + y * y + z * z) <= semi * semi).to(torch.uint8).contiguous()


def global_init_case(args, G, fixed, moving, affine, centre):
    """The coarse stage and a 12-candidate evaluation, masked against unmasked."""
    n, shape = args.size, tuple(fixed.shape)
    mask = ellipsoid_mask(n, "cuda")
    franges, mranges = G.volume_range(fixed), G.volume_range(moving)
    res = {"gpu": torch.cuda.get_device_name(0), "size": n, "bins": BINS, "inner": args.inner, "reps": args.reps,
           "mask_share": round(float(mask.float().mean()), 4)}
    grid = G.rotation_grid(40.0, 20.0)
    coarse_ps = np.hstack([np.zeros((len(grid), 3)), grid])
    step = np.array([2.0] * 6)
    probe_ps = np.zeros((12, 6))
    for a in range(6):
        probe_ps[2 * a, a], probe_ps[2 * a + 1, a] = step[a], -step[a]
    hist = torch.empty((G.MAX_CANDIDATES, BINS, BINS), dtype=torch.int64, device="cuda")

    def evaluation(ps, stride, fixed_mask, min_count):
        ms = np.stack([G.candidate_matrix(q, affine, affine, centre) for q in ps])
        values = torch.empty(len(ps), dtype=torch.float64, device="cuda")
        chunks = [(at, ms[at:at + G.MAX_CANDIDATES]) for at in range(0, len(ms), G.MAX_CANDIDATES)]

        def run():
            for at, m in chunks:
                h = G.joint_histogram(fixed, moving, m, BINS, stride, franges, mranges, fixed_mask=fixed_mask, out=hist[:len(m)])
                values[at:at + len(m)] = G.nmi(h, min_count)[0]
            return values
        return run

    for name, ps, strides in (("coarse_125", coarse_ps, (4,)), ("probe_12", probe_ps, (4, 2))):
        for stride in strides:
            samples = G.sample_count(shape, stride)
            inside = int(torch.count_nonzero(mask[::stride, ::stride, ::stride]))
            fns = {"unmasked": evaluation(ps, stride, None, samples // 4), "masked": evaluation(ps, stride, mask, inside // 4)}
            r = {"samples": samples, "masked_samples": inside, "times": alternating_times(fns, args.reps, args.warmup, args.inner)}
            r["masked_over_unmasked"] = round(r["times"]["masked"]["us_median"] / r["times"]["unmasked"]["us_median"], 4)
            r["finite_values"] = {k: int(torch.isfinite(fn()).sum()) for k, fn in fns.items()}
            res[f"{name}_stride{stride}"] = r
    res["mask_moments"] = alternating_times({"kernel": lambda: G.mask_moments(mask)}, args.reps, args.warmup, args.inner)["kernel"]
    res["mask_moments"]["moments"] = G.mask_moments(mask).cpu().tolist()
    return res


def raw_call(path, fixed, moving, ms, stride, franges, mranges, hist, values, counts, min_count):
    """Both entries of a build of libmrisr.so, into preallocated buffers."""
    lib = C.CDLL(path)
    jh, nm = lib.mrisr_f32_volume_joint_histogram, lib.mrisr_joint_histogram_nmi
    jh.restype = nm.restype = C.c_int
    jh.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int,
                   C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    nm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    k = len(ms)
    arg = (C.c_double * (12 * k))(*ms.reshape(-1).tolist())

    def call():
        st = torch.cuda.current_stream().cuda_stream
        rc = jh(fixed.data_ptr(), *fixed.shape, moving.data_ptr(), *moving.shape, arg, k, stride, BINS, *franges, *mranges, hist.data_ptr(), st)
        assert rc == 0, rc
        rc = nm(hist.data_ptr(), k, BINS, min_count, values.data_ptr(), counts.data_ptr(), st)
        assert rc == 0, rc
    return call


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--inner", type=int, default=5)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--skip_torch", action="store_true")
    p.add_argument("--skip_registration", action="store_true")
    p.add_argument("--variant_libs", type=str, nargs="*", default=[], help="name=path of other builds of libmrisr.so")
    p.add_argument("--global_init", action="store_true", help="time the coarse stage and the masked cost instead (module docstring)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("register_bench needs the MI355X: there is nothing to time on a CPU")
    from mri_superresolution_amd import volume_register as G
    from mri_superresolution_amd._lib import LIB_PATH
    from mri_superresolution_amd.volume_reslice import reslice

    n = args.size
    shape = (n, n, n)
    affine = np.eye(4)
    centre = G.volume_centre(affine, shape)
    p_true = np.array([3.2, -2.4, 1.7, 4.0, -3.0, 5.0]) * np.array([n / 64] * 3 + [1] * 3)
    fixed = phantom(n, "cuda")
    moving = (1.0 - reslice(fixed, np.linalg.inv(G.rigid_world(p_true, centre))[:3], shape, "linear").clamp_min(0).sqrt()).contiguous()
    if args.global_init:
        print(json.dumps(global_init_case(args, G, fixed, moving, affine, centre)))
        return
    franges, mranges = G.volume_range(fixed), G.volume_range(moving)
    # the 12 probes of a first search iteration around p = 0
    step = np.array([2.0] * 6)
    ps = np.zeros((12, 6))
    for a in range(6):
        ps[2 * a, a], ps[2 * a + 1, a] = step[a], -step[a]
    ms = np.stack([G.candidate_matrix(q, affine, affine, centre) for q in ps])
    res = {"gpu": torch.cuda.get_device_name(0), "size": n, "bins": BINS, "inner": args.inner, "strides": {}}
    for stride in (4, 2):
        samples = G.sample_count(shape, stride)
        min_count = samples // 4
        r = {"samples": samples}
        hist = torch.empty((12, BINS, BINS), dtype=torch.int64, device="cuda")

        def ours():
            return G.nmi(G.joint_histogram(fixed, moving, ms, BINS, stride, franges, mranges, out=hist), min_count)[0]
        fns, bufs = {"kernel": ours}, {}
        for spec in [f"raw={LIB_PATH}"] + args.variant_libs:
            vname, path = spec.split("=", 1)
            bufs[vname] = (torch.empty((12, BINS, BINS), dtype=torch.int64, device="cuda"),
                           torch.empty(12, dtype=torch.float64, device="cuda"), torch.empty(12, dtype=torch.int64, device="cuda"))
            fns[vname] = raw_call(path, fixed, moving, ms, stride, franges, mranges, *bufs[vname], min_count)
        if not args.skip_torch:
            fs = fixed[::stride, ::stride, ::stride].contiguous()      # taken once, outside the timed path, in torch's favour
            fscale, mscale = BINS / (franges[1] - franges[0]), BINS / (mranges[1] - mranges[0])
            fbin = ((fs - franges[0]) * fscale).long().clamp_(0, BINS - 1).reshape(-1) * BINS
            thetas = [torch_theta(G.strided_matrix(m, stride), shape, fs.shape, "cuda") for m in ms]
            torch_hist = torch.empty((12, BINS * BINS), dtype=torch.int64, device="cuda")

            def torch_path():
                for c, theta in enumerate(thetas):
                    grid = F.affine_grid(theta, (1, 1) + tuple(fs.shape), align_corners=False)
                    mv = F.grid_sample(moving[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)
                    cell = fbin + ((mv.reshape(-1) - mranges[0]) * mscale).long().clamp_(0, BINS - 1)
                    torch_hist[c] = torch.bincount(cell, minlength=BINS * BINS)
                pj = torch_hist.double() / torch_hist.sum(dim=1, keepdim=True)
                pj3 = pj.reshape(12, BINS, BINS)
                ent = lambda q: -(torch.where(q > 0, q * torch.log(q.clamp_min(1e-300)), torch.zeros_like(q))).sum(dim=-1)      # noqa: E731
                return (ent(pj3.sum(dim=2)) + ent(pj3.sum(dim=1))) / ent(pj)
            fns["torch"] = torch_path
        r["times"] = alternating_times(fns, args.reps, args.warmup, args.inner)
        # one search iteration as the search makes it: the launches and the read of the 12 values
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            ours().cpu()
        r["search_step_us"] = round((time.perf_counter() - t0) / 20 * 1e6, 1)
        values = ours().cpu().numpy()
        r["nmi_first_probe"] = float(values[0])
        r["counts_share"] = round(float(hist[0].sum()) / samples, 4)
        for vname, (h, v, _) in bufs.items():
            r[f"{vname}_equal"] = bool(torch.equal(h, hist)) and bool(np.array_equal(v.cpu().numpy(), values))
        if not args.skip_torch:
            r["kernel_over_torch"] = round(r["times"]["kernel"]["us_median"] / r["times"]["torch"]["us_median"], 4)
            r["torch_nmi_first_probe"] = float(torch_path()[0])
        res["strides"][str(stride)] = r
    if not args.skip_registration:
        G.register_rigid(fixed, affine, moving, affine, bins=BINS)      # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found = G.register_rigid(fixed, affine, moving, affine, bins=BINS)
        torch.cuda.synchronize()
        res["registration"] = {"wall_s": round(time.perf_counter() - t0, 4), "n_evaluations": found.n_evaluations,
                               "iterations": len(found.trace), "p": [round(float(x), 5) for x in found.p],
                               "p_true": p_true.tolist(), "nmi": [found.trace[0]["best"], found.value],
                               "corner_displacement_voxels": round(G.corner_displacement(found.world, G.rigid_world(p_true, centre), affine, shape), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
