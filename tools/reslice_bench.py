#!/usr/bin/env python3
"""Cost of the reslicing kernel (csrc/volume_reslice.hip) next to the same work written with torch.

    python tools/reslice_bench.py [--reps 20] [--warmup 3] [--inner 10] [--skip_torch] [--variant_libs name=path ...]

Cases, on a float32 volume in [0, 4095]:
(a) 256^3 -> 256^3 under a rotation of 10 / 20 / 30 degrees about the x / y / z axis through the centre;
(b) 256 x 256 x 52 -> 256^3: a thick-slice scan respaced along z (the first corner kept).
Per case ``reslice`` with ``nearest``, ``linear`` and ``cubic``, and ``reslice_mask``: HIP events around ``--inner`` back-to-back
calls after warm-up, the median over ``--reps`` such windows, per call; the achieved GB/s count the destination bytes once plus
the source bytes once (the algorithmic traffic: every tap beyond the first use of a voxel is cache traffic).  The torch path is
``F.affine_grid`` + ``F.grid_sample(mode="bilinear")`` on the 5-D input - trilinear, the counterpart of ``linear`` only; torch has no
cubic mode for volumes and ``nearest`` is reported alone as well.  The torch path alternates with the ``linear`` kernel in one loop, so
that the ratio is taken on one box in one run; its result is compared with the kernel's where no tap leaves the volume (torch pads
with zeros, the kernel replicates the border and cuts at the volume's faces).  ``--variant_libs``: other builds of libmrisr.so (another
brick shape, ``-DMRISR_RESLICE_BX=.. -DMRISR_RESLICE_BY=.. -DMRISR_RESLICE_BZ=..``) join the same alternation through ctypes; ``raw:*`` is
this build's own entry called the same way (preallocated output, no wrapper).
Prints one JSON line (profiles/NOTES.md, "Reslice")."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def rotation_matrix(shape, degrees=(10.0, 20.0, 30.0)):
    ax, ay, az = np.deg2rad(degrees)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    rot = rz @ ry @ rx
    c = (np.array(shape, dtype=np.float64) - 1) / 2
    return np.hstack([rot, (c - rot @ c)[:, None]])


def respacing_matrix(src, dst):
    s = np.array(src, dtype=np.float64) / np.array(dst, dtype=np.float64)
    return np.hstack([np.diag(s), (0.5 * s - 0.5)[:, None]])


def torch_theta(m, src, dst, device):
    """The (1, 3, 4) theta of ``F.affine_grid(align_corners=False)`` for the index matrix ``m``: voxel index i of an axis of extent n
    sits at the normalised coordinate (2 i + 1) / n - 1; torch orders the coordinates (z, y, x) of an (X, Y, Z) volume."""
    S, D = np.array(src, dtype=np.float64), np.array(dst, dtype=np.float64)
    lin = m[:, :3] * D[None, :] / S[:, None]
    off = (m[:, :3] @ (D - 1) + 2 * m[:, 3] + 1) / S - 1
    theta = np.hstack([lin[::-1, ::-1], off[::-1, None]])
    return torch.tensor(theta[None], dtype=torch.float32, device=device)


def alternating_times(fns, reps, warmup, inner):
    """{name: us per call} of several callables timed in turn, round after round: what they share of the box's state they share alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {k: {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2)} for k, v in times.items()}


def variant_call(path, vol, m, out, method):
    """The float entry of another build of libmrisr.so (nothing else of it is used)."""
    lib = C.CDLL(path)
    fn = lib.mrisr_f32_volume_reslice
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_float,
                   C.c_void_p]
    m12 = (C.c_double * 12)(*m.reshape(-1).tolist())

    def call():
        rc = fn(vol.data_ptr(), *vol.shape, out.data_ptr(), *out.shape, m12, method, 0.0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return call


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--skip_torch", action="store_true")
    p.add_argument("--variant_libs", type=str, nargs="*", default=[], help="name=path of other builds of libmrisr.so (brick shapes)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reslice_bench needs the MI355X: there is nothing to time on a CPU")
    from mri_superresolution_amd._lib import LIB_PATH
    from mri_superresolution_amd.volume_reslice import METHODS, reslice, reslice_mask

    cases = {"rotate_256": ((256, 256, 256), (256, 256, 256), rotation_matrix((256, 256, 256))),
             "respace_256x256x52": ((256, 256, 52), (256, 256, 256), respacing_matrix((256, 256, 52), (256, 256, 256)))}
    res = {"gpu": torch.cuda.get_device_name(0), "inner": args.inner, "cases": {}}
    for name, (src, dst, m) in cases.items():
        g = torch.Generator(device="cuda").manual_seed(0)
        vol = torch.rand(src, device="cuda", generator=g) * 4095
        mask = (vol > 2000).to(torch.uint8)
        nsrc, ndst = vol.numel(), dst[0] * dst[1] * dst[2]
        r = {"src": list(src), "dst": list(dst), "bytes_f32": 4 * (nsrc + ndst)}
        fns = {method: (lambda method=method: reslice(vol, m, dst, method)) for method in ("nearest", "linear", "cubic")}
        fns["mask_u8"] = lambda: reslice_mask(mask, m, dst)
        outs = {}
        # "raw": this build's entry called the way the variants are - into a preallocated output, without the wrapper's checks and
        # allocation - so that brick shapes compare like for like and the wrapper's host cost shows
        for spec in [f"raw={LIB_PATH}"] + args.variant_libs:
            vname, path = spec.split("=", 1)
            for method in ("nearest", "linear", "cubic") if vname == "raw" else ("linear", "cubic"):
                outs[vname, method] = torch.empty(dst, dtype=torch.float32, device="cuda")
                fns[f"{vname}:{method}"] = variant_call(path, vol, m, outs[vname, method], METHODS[method])
        if not args.skip_torch:
            theta = torch_theta(m, src, dst, "cuda")

            def torch_path():
                grid = F.affine_grid(theta, (1, 1) + tuple(dst), align_corners=False)
                return F.grid_sample(vol[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)
            fns["torch_trilinear"] = torch_path
        r["times"] = alternating_times(fns, args.reps, args.warmup, args.inner)
        for k, t in r["times"].items():
            nbytes = nsrc + ndst if k == "mask_u8" else 4 * (nsrc + ndst)
            t["GBps"] = round(nbytes / (t["us_median"] * 1e-6) / 1e9, 1)
        if not args.skip_torch:
            r["linear_over_torch"] = round(r["times"]["linear"]["us_median"] / r["times"]["torch_trilinear"]["us_median"], 4)
            # where all eight taps are inside, the two paths interpolate the same values: the coordinates differ by float32 rounding
            ours, theirs = reslice(vol, m, dst, "linear"), torch_path()[0, 0]
            i, j, k = torch.meshgrid(*(torch.arange(n, device="cuda", dtype=torch.float64) for n in dst), indexing="ij")
            mt = torch.tensor(m, device="cuda")
            free = torch.ones(dst, dtype=torch.bool, device="cuda")
            for a in range(3):
                pa = mt[a, 0] * i + mt[a, 1] * j + mt[a, 2] * k + mt[a, 3]
                free &= (pa >= 0) & (pa <= src[a] - 1)
            r["interior_share"] = round(float(free.double().mean()), 4)
            r["max_abs_diff_to_torch_interior"] = float((ours - theirs)[free].abs().max())
            del i, j, k, free, ours, theirs
        for (vname, method), out in outs.items():
            r[f"{vname}:{method}_equal"] = bool(torch.equal(out, reslice(vol, m, dst, method)))
        r["covered_share"] = round(float(reslice_mask(torch.ones_like(mask), m, dst).double().mean()), 4)
        res["cases"][name] = r
        del vol, mask, outs
    print(json.dumps(res))


if __name__ == "__main__":
    main()
