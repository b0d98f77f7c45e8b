#!/usr/bin/env python3
"""Combine orthogonal thick-slice stacks of one head into one isotropic volume on the device (extension).

    python scripts/combine_stacks.py --inputs ax.nii.gz cor.nii.gz sag.nii.gz --output iso.nii.gz
    python scripts/combine_stacks.py --inputs ax.nii.gz cor.nii.gz --output iso.nii.gz --spacing 1.5 --register rigid --profile gaussian

Iterative back-projection (``volume_stacks.combine_stacks``: ``csrc/volume_stacks.hip``, bit-equal to
``volume_stacks.combine_stacks_np``).  The output grid is ``volume_stacks.default_output_grid`` of the stacks - the first stack's
orientation, isotropic at the smallest voxel size of any stack or at ``--spacing`` mm, the bounding box of all the stacks - or the
grid of ``--like``.  ``--slice_axis`` (one value for all stacks or one per stack; ``auto``: the axis with the largest voxel size),
``--thickness_mm`` (likewise; default: the spacing along the slice axis), ``--profile box|gaussian`` and ``--profile_samples`` (default:
a sample per output voxel over the profile) describe the slices.  ``--register rigid`` registers every stack after the first to the
first (``volume_register.register_rigid``) and folds the transform into that stack's matrices: the patient moves between
acquisitions.  Per iteration and stack the RMS of the residual is logged, and the share of the output voxels covered by 0, 1, ...,
K stacks.  ``--no_clamp`` lets the estimate go below 0; ``--fill`` is the value of the voxels no stack covers; ``--save_initial``
writes the initial estimate (the mean of the stacks' linear reslices).  ``--regularise LAMBDA`` (default 0: none) adds the Huber
prior of ``volume_stacks.stack_update_np`` on the six face neighbours to every update - on noisy stacks the plain iteration is past
its best after two or three updates, with the prior it settles and can be run to convergence; ``--regularise_delta D`` (default inf:
the quadratic prior) clips the neighbour differences at ``D`` intensity units, which keeps tissue steps and fine detail; the
coefficients are ``volume_stacks.regulariser_coeffs`` of the output grid.  ``--motion slices`` (default ``none``) corrects motion
between the slices of a stack: after the reconstruction with stack-wide matrices, ``--motion_rounds`` (2) times, every slice of every
stack is registered rigidly to the current estimate (``volume_slices.register_slices``: normalised cross-correlation, a compass search
for all slices at once, poses within ``--motion_limit_mm`` / ``--motion_limit_deg`` (10 / 10); slices whose contrast is below
``--motion_min_contrast`` (0.1) of the stack's keep their pose) and the estimate is rebuilt with a matrix per slice.  Per round and
stack the active slices, the mean cost before and after and the largest displacement of a slice corner are logged; ``--save_motion
F.csv`` writes a row per slice (of the last frame): stack, slice, the six parameters, the active flag, the cost at the start and the
end of the last round.  ``--motion slices`` with ``--regularise`` is not built and is refused.  4-D inputs must agree in their frame count and are combined
frame by frame.  The output is float32 under ``utils.nifti.header_for_grid`` of the first input's header.  Exit code 0 / 1 (error
logged), as ``scripts/infer_volume.py``.
"""
import argparse
import logging
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from mri_superresolution_amd import volume_slices as V                                                     # noqa: E402
from mri_superresolution_amd import volume_stacks as S                                                     # noqa: E402
from mri_superresolution_amd.utils.nifti import frames, header_for_grid, read_nifti           # noqa: E402
from scripts._cli import add_cpu_flag, join_frames, run, save_nifti                                          # noqa: E402

logger = logging.getLogger("combine_stacks")


MOTIONS = ("none", "slices")
MOTION_WITH_REGULARISER = "--motion slices with --regularise is not built: the regularised update takes one matrix per stack"


def per_stack(values, count, name, default):
    """One value for all the stacks, or one per stack."""
    if values is None:
        return [default] * count
    if len(values) not in (1, count):
        raise ValueError(f"--{name} takes one value or one per input ({count}), got {len(values)}")
    return list(values) * (count if len(values) == 1 else 1)


def check_options(inputs, iterations=S.DEFAULT_ITERATIONS, step=1.0, slice_axis=None, thickness_mm=None, profile_samples=None, spacing=None,
                  regularise=0.0, regularise_delta=float("inf"), motion="none", motion_rounds=2, motion_limit_mm=10.0, motion_limit_deg=10.0,
                  motion_min_contrast=0.1):
    """The checks that need no file: raises ``ValueError`` before anything is read."""
    if motion not in MOTIONS:
        raise ValueError(f"--motion is one of {MOTIONS}, got {motion!r}")
    if motion != "none":
        if regularise > 0:
            raise ValueError(MOTION_WITH_REGULARISER)
        if motion_rounds < 0 or not (motion_limit_mm > 0 and motion_limit_deg > 0 and motion_min_contrast >= 0):
            raise ValueError("--motion_rounds must not be negative, --motion_limit_mm and --motion_limit_deg positive, "
                             "--motion_min_contrast not negative")
    if not 1 <= len(inputs) <= S.MAX_STACKS:
        raise ValueError(f"1..{S.MAX_STACKS} stacks are combined, got {len(inputs)}")
    S._check_iterations(iterations), S._check_step(step)
    S._check_regulariser(0.0, regularise, regularise_delta, None)      # the stability bound needs the grid's coefficients: combine_stacks checks it
    axes = [None if a == "auto" else int(a) for a in per_stack(slice_axis, len(inputs), "slice_axis", "auto")]
    if any(a is not None and a not in (0, 1, 2) for a in axes):
        raise ValueError(f"--slice_axis is auto, 0, 1 or 2, got {slice_axis}")
    thickness = per_stack(thickness_mm, len(inputs), "thickness_mm", None)
    if any(t is not None and not (np.isfinite(t) and t > 0) for t in thickness):
        raise ValueError(f"--thickness_mm must be positive, got {thickness_mm}")
    if profile_samples is not None and not 1 <= profile_samples <= S.MAX_SAMPLES:
        raise ValueError(f"--profile_samples is 1..{S.MAX_SAMPLES}, got {profile_samples}")
    if spacing is not None and not (np.isfinite(spacing) and spacing > 0):
        raise ValueError(f"--spacing must be positive, got {spacing}")
    return axes, thickness


def combine_files(inputs, output_path, spacing=None, like=None, iterations=S.DEFAULT_ITERATIONS, step=1.0, profile="box", thickness_mm=None,
                  slice_axis=None, profile_samples=None, register="none", clamp=0.0, fill=0.0, save_initial=None, device="cuda",
                  regularise=0.0, regularise_delta=float("inf"), motion="none", motion_rounds=2, motion_limit_mm=10.0, motion_limit_deg=10.0,
                  motion_min_contrast=0.1, save_motion=None):
    """NIfTI stacks -> one NIfTI volume; returns the output array (as written)."""
    axes, thickness = check_options(inputs, iterations, step, slice_axis, thickness_mm, profile_samples, spacing, regularise, regularise_delta,
                                    motion, motion_rounds, motion_limit_mm, motion_limit_deg, motion_min_contrast)
    scans = [read_nifti(p) for p in inputs]
    per_scan = [[np.ascontiguousarray(f, dtype=np.float32) for f in frames(d)] for d, _ in scans]
    if len({len(f) for f in per_scan}) != 1 or len({d.ndim for d, _ in scans}) != 1:
        raise ValueError(f"the inputs must agree in their frame count, got shapes {[tuple(d.shape) for d, _ in scans]}")
    affines, shapes = [h.affine() for _, h in scans], [tuple(d.shape[:3]) for d, _ in scans]
    if like is not None:
        like_header = read_nifti(like)[1]
        affine_out, shape_out = like_header.affine(), tuple(like_header.shape[:3])
    else:
        affine_out, shape_out = S.default_output_grid(affines, shapes, spacing)
    worlds = [None] * len(inputs)
    if register == "rigid":
        from mri_superresolution_amd.volume_register import register_rigid
        fixed = torch.from_numpy(per_scan[0][0]).to(device)
        for k in range(1, len(inputs)):
            r = register_rigid(fixed, affines[0], torch.from_numpy(per_scan[k][0]).to(device), affines[k])
            worlds[k] = r.world
            logger.info(f"stack {k} registered to stack 0: tx, ty, tz (mm), rx, ry, rz (deg) = {np.round(r.p, 3).tolist()}, NMI {r.value:.4f}")
    geometries = [S.stack_geometry(a, affine_out, axes[k], profile, thickness[k], profile_samples, worlds[k]) for k, a in enumerate(affines)]
    for k, g in enumerate(geometries):
        logger.info(f"stack {k}: {shapes[k]} voxels of {np.round(S.voxel_sizes(affines[k]), 3).tolist()} mm, slice axis {g.slice_axis}, "
                    f"{g.offsets.size} {profile} profile samples over {g.offsets[-1] - g.offsets[0]:.3f} slices")
    coeffs = S.regulariser_coeffs(affine_out) if regularise > 0 else None
    if regularise > 0:
        logger.info(f"regulariser: lambda {regularise:g}, delta {regularise_delta:g}, coefficients {[round(float(c), 6) for c in coeffs]} "
                    f"(output voxels of {np.round(S.voxel_sizes(affine_out), 3).tolist()} mm)")
    options = {}
    if motion == "slices":                                           # without the flag the call is the one it always was
        options["motion"] = V.MotionOptions(tuple(affines), affine_out, tuple(worlds), motion_rounds, motion_limit_mm, motion_limit_deg,
                                            motion_min_contrast)
    ws = S.StackWorkspace(shape_out, shapes, device, iterations, regularised=regularise > 0, **({"motion": True} if options else {}))
    outs, initials = [], []
    for t in range(len(per_scan[0])):
        r = S.combine_stacks([torch.from_numpy(f[t]).to(device) for f in per_scan], geometries, shape_out, iterations, step, clamp, fill,
                             workspace=ws, check=True, reg_lambda=regularise, reg_delta=regularise_delta, reg_coeffs=coeffs, **options)
        if options:
            log_motion(t, r, affines, shapes, geometries)
            if save_motion is not None:
                write_motion_csv(save_motion, r)
        for it in range(iterations):
            logger.info(f"frame {t} iteration {it + 1}: residual RMS per stack {[round(float(v), 4) for v in r.rms[it]]}")
        shares = r.coverage / float(r.coverage.sum())
        logger.info(f"frame {t}: share of the output voxels covered by 0..{len(inputs)} stacks: {[round(float(s), 4) for s in shares]}")
        outs.append(r.volume.cpu().numpy())
        initials.append(r.initial.cpu().numpy())
    header = header_for_grid(scans[0][1], shape_out, affine_out)
    result = None
    for path, vols in ((output_path, outs), (save_initial, initials)):
        if path is None:
            continue
        data = join_frames(vols, scans[0][0].ndim)
        save_nifti(path, data, header)
        result = data if result is None else result
    logger.info(f"Combined {len(inputs)} stacks into {tuple(result.shape)} ({iterations} iterations) saved to {output_path}")
    return result


def log_motion(t, r, affines, shapes, geometries):
    """Per round and stack: the mean cost before and after; per stack: the active slices and the largest corner displacement."""
    for rnd, row in enumerate(r.motion_cost):
        for k, (before, after) in enumerate(row):
            logger.info(f"frame {t} motion round {rnd + 1} stack {k}: mean NCC of the active slices {before:.5f} -> {after:.5f}")
    for k, (p, m) in enumerate(zip(r.motion, r.motion_detail)):
        d = V.slice_corner_displacement(p, np.zeros_like(p), affines[k], shapes[k], geometries[k].slice_axis)
        logger.info(f"frame {t} stack {k}: {int(m.active.sum())} of {m.active.size} slices active, largest displacement of a slice corner "
                    f"{float(d.max()):.3f} mm")


def write_motion_csv(path, r):
    """A row per slice: stack, slice, tx, ty, tz (mm), rx, ry, rz (degrees), active, the cost at the start and the end of the last round."""
    with open(path, "w") as f:
        f.write("stack,slice,tx,ty,tz,rx,ry,rz,active,cost_start,cost_end\n")
        for k, (p, m) in enumerate(zip(r.motion, r.motion_detail)):
            for s in range(p.shape[0]):
                f.write(f"{k},{s}," + ",".join(repr(float(v)) for v in p[s]) + f",{int(m.active[s])},{float(m.start[s])!r},{float(m.end[s])!r}\n")


def _body(args, device):
    combine_files(args.inputs, args.output, args.spacing, args.like, args.iterations, args.step, args.profile, args.thickness_mm,
                  args.slice_axis, args.profile_samples, args.register, None if args.no_clamp else 0.0, args.fill, args.save_initial, device,
                  args.regularise, args.regularise_delta, args.motion, args.motion_rounds, args.motion_limit_mm, args.motion_limit_deg,
                  args.motion_min_contrast, args.save_motion)


def main(args):
    return run(_body, args, logger, "the reconstruction")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Combine orthogonal thick-slice stacks into one isotropic volume (extension)")
    p.add_argument("--inputs", type=str, nargs="+", required=True, help="the stacks: single-file NIfTI-1, 3-D or 4-D; the first gives the orientation")
    p.add_argument("--output", type=str, required=True, help="output volume, .nii or .nii.gz, float32")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--spacing", type=float, default=None, help="isotropic output voxel size in mm (default: the smallest of any stack)")
    g.add_argument("--like", type=str, default=None, help="take the output grid (extents and affine) of this scan")
    p.add_argument("--iterations", type=int, default=S.DEFAULT_ITERATIONS)
    p.add_argument("--step", type=float, default=1.0)
    p.add_argument("--profile", type=str, choices=list(S.PROFILES), default="box")
    p.add_argument("--thickness_mm", type=float, nargs="+", default=None, help="slice thickness, one value or one per input (default: the slice spacing)")
    p.add_argument("--slice_axis", type=str, nargs="+", default=None, choices=["auto", "0", "1", "2"], help="one value or one per input")
    p.add_argument("--profile_samples", type=int, default=None, help="samples of the slice profile, 1..16")
    p.add_argument("--register", type=str, choices=["none", "rigid"], default="none", help="register every stack after the first to the first")
    p.add_argument("--no_clamp", action="store_true", help="do not clamp the estimate at 0")
    p.add_argument("--fill", type=float, default=0.0, help="value of the output voxels no stack covers")
    p.add_argument("--save_initial", type=str, default=None, help="write the initial estimate (the mean of the linear reslices)")
    p.add_argument("--regularise", type=float, default=0.0, metavar="LAMBDA", help="weight of the Huber prior on the six face neighbours (default 0: none); "
                   "step * LAMBDA * (sum of the coefficients) <= 0.5")
    p.add_argument("--regularise_delta", type=float, default=float("inf"), metavar="D", help="clip the neighbour differences at D (default inf: quadratic prior)")
    p.add_argument("--motion", type=str, choices=list(MOTIONS), default="none", help="slices: register every slice to the estimate and rebuild it")
    p.add_argument("--motion_rounds", type=int, default=2, help="rounds of slice registration and rebuild")
    p.add_argument("--motion_limit_mm", type=float, default=10.0, help="largest translation of a slice, per component")
    p.add_argument("--motion_limit_deg", type=float, default=10.0, help="largest rotation of a slice, per component")
    p.add_argument("--motion_min_contrast", type=float, default=0.1, help="slices with less contrast than this share of the stack's keep their pose")
    p.add_argument("--save_motion", type=str, default=None, metavar="F.csv", help="write the slices' poses, active flags and costs")
    add_cpu_flag(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
