#!/usr/bin/env python3
"""Rigid registration of a NIfTI scan to another on the device (extension).

    python scripts/register_volume.py --fixed highfield.nii.gz --moving lowfield.nii.gz --output lowfield_on_fixed.nii.gz \
        --interp cubic --save_transform fixed_to_moving.txt

The six parameters of a rigid transform between the two scans' world frames are estimated by maximising the normalised mutual
information of their joint histogram (``volume_register.register_rigid``: ``csrc/volume_register.hip``, ``--bins`` 16, 32 or
64), starting from the two headers as they are - or, with ``--init global``, from the best of a coarse grid of rotations
(``--init_limit``, ``--init_step`` degrees) about the two foreground masks' centres of mass, for scans whose world frames are
centimetres and tens of degrees apart; ``--mask otsu`` counts only the samples inside the fixed scan's Otsu foreground.  The output is the moving scan resliced ONCE onto the fixed scan's grid through the
estimated transform (``--interp linear|cubic``, voxels outside the moving scan are ``--fill``), float32 under
``utils.nifti.header_for_grid`` of the moving scan's header.  ``--save_transform`` writes the 4 x 4 fixed world -> moving world
matrix as text (``numpy.loadtxt`` reads it back).  A 4-D file is registered on its frame 0 and the transform is applied to every
frame.  Exit code 0 / 1 (error logged), as ``scripts/infer_volume.py``.

``--nonrigid demons`` adds a deformable stage for what a rigid transform leaves between two scanners (gradient non-linearity,
susceptibility distortion): after the rigid stage and its one reslice, a displacement field on the fixed grid is estimated against
the fixed scan (``volume_deform.register_deformable``: ``csrc/volume_deform.hip``, Thirion's demons, ``--nonrigid_levels``,
``--nonrigid_iterations`` coarse to fine, ``--nonrigid_sigma`` and ``--nonrigid_max_step`` in voxels) and the resliced scan is
warped through it (``--interp``): the output is then interpolated twice.  The force is an intensity difference, so both scans should
be on one intensity scale (``scripts/evaluate_volume.py --match_intensity`` / ``--match_bias`` do that for an evaluation).
``--save_field`` writes the field as a 4-D float32 NIfTI of three frames (voxels of the fixed grid) under the fixed grid's header.
The default, ``none``, leaves the script as it was.

``--nonrigid diffeomorphic`` estimates the field by diffeomorphic demons instead (``volume_deform.register_diffeomorphic``): the
update of an iteration is turned into a small diffeomorphism by ``--nonrigid_exp_steps`` squarings and composed with the field, not
added to it, so the field does not fold where the additive one does.  ``--nonrigid_force lcc`` (with either method) replaces the
intensity difference by a locally normalised correlation force (``volume_deform.lcc_force``: ``csrc/volume_lcc.hip``,
``--nonrigid_lcc_radius`` voxels either side) for scans of different contrast, where an intensity difference moves the field away
from the truth; the log then reports ``1 - mean rho^2`` per level.  ``--nonrigid_resample once`` (with either method) writes every
frame as ONE interpolation of the original moving frame through the rigid matrix and the field
(``volume_deform.warp_matrix``: the frame at ``M (x + u(x))``), not as a warp of the resliced frame; the field itself is still
estimated on the resliced frame 0.  The default, ``twice``, writes the bytes it wrote before.
"""
import argparse
import logging
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from mri_superresolution_amd.utils.nifti import frames as frames_of, header_for_grid, read_nifti      # noqa: E402
from mri_superresolution_amd.volume_deform import DEFAULT_ITERATIONS, MAX_EXP_STEPS, register_deformable, warp      # noqa: E402
from mri_superresolution_amd.volume_deform import MAX_LCC_RADIUS, register_diffeomorphic, warp_matrix      # noqa: E402
from mri_superresolution_amd.volume_register import register_rigid                             # noqa: E402
from mri_superresolution_amd.volume_reslice import covered_share, reslice                      # noqa: E402
from scripts._cli import add_cpu_flag, join_frames, make_parent, run, save_nifti, to_device                 # noqa: E402

logger = logging.getLogger("register_volume")


def describe(result):
    p = result.p
    return (f"t = ({p[0]:.4f}, {p[1]:.4f}, {p[2]:.4f}) mm, r = ({p[3]:.4f}, {p[4]:.4f}, {p[5]:.4f}) degrees, NMI "
            f"{result.trace[0]['best']:.6f} -> {result.value:.6f} in {result.n_evaluations} evaluations")


def describe_coarse(result):
    """The coarse stage of ``--init global``: the candidate taken (the start of the search) and its value."""
    entry = result.trace[0]
    p = result.trace[1]["p"]
    return (f"coarse stage: candidate {entry['accepted']} of {entry['n_candidates']} at stride {entry['stride']}, t = ({p[0]:.4f}, "
            f"{p[1]:.4f}, {p[2]:.4f}) mm, r = ({p[3]:.4f}, {p[4]:.4f}, {p[5]:.4f}) degrees, NMI {entry['best']:.6f}")


def describe_nonrigid(result, force="ssd"):
    """One line per level: the mean squared difference at its first and last iteration - under ``force="lcc"`` one minus the mean
    squared local correlation, the rows being (sum of the confidences, count)."""
    lines, row = [], 0
    for shape, its in result.schedule:
        if its:
            (s0, n0), (s1, n1) = result.stats[row], result.stats[row + its - 1]
            if force == "lcc":
                lines.append(f"level {'x'.join(map(str, shape))}: 1 - mean rho^2 {1.0 - s0 / max(n0, 1):.6g} -> "
                             f"{1.0 - s1 / max(n1, 1):.6g} in {its} iterations")
            else:
                lines.append(f"level {'x'.join(map(str, shape))}: mean squared difference {s0 / max(n0, 1):.6g} -> {s1 / max(n1, 1):.6g} "
                             f"in {its} iterations")
        row += its
    return lines


def check_options(nonrigid="none", nonrigid_exp_steps=2, nonrigid_resample="twice", save_field=None, nonrigid_force="ssd",
                  nonrigid_lcc_radius=2):
    """The rules of the non-rigid options, stated once; ``register_file`` applies them before it reads a file."""
    if nonrigid not in ("none", "demons", "diffeomorphic"):
        raise ValueError(f"--nonrigid must be none, demons or diffeomorphic, got {nonrigid}")
    if save_field and nonrigid == "none":
        raise ValueError("--save_field goes with --nonrigid demons or diffeomorphic")
    if nonrigid_resample not in ("twice", "once"):
        raise ValueError(f"--nonrigid_resample must be twice or once, got {nonrigid_resample}")
    if nonrigid_resample == "once" and nonrigid == "none":
        raise ValueError("--nonrigid_resample once goes with --nonrigid demons or diffeomorphic: without a field the rigid stage "
                         "already interpolates once")
    if isinstance(nonrigid_exp_steps, bool) or not isinstance(nonrigid_exp_steps, int) or not 0 <= nonrigid_exp_steps <= MAX_EXP_STEPS:
        raise ValueError(f"--nonrigid_exp_steps must be an integer in 0..{MAX_EXP_STEPS}, got {nonrigid_exp_steps}")
    if nonrigid_force not in ("ssd", "lcc"):
        raise ValueError(f"--nonrigid_force must be ssd or lcc, got {nonrigid_force}")
    if nonrigid_force == "lcc" and nonrigid == "none":
        raise ValueError("--nonrigid_force lcc goes with --nonrigid demons or diffeomorphic")
    if isinstance(nonrigid_lcc_radius, bool) or not isinstance(nonrigid_lcc_radius, int) or not 1 <= nonrigid_lcc_radius <= MAX_LCC_RADIUS:
        raise ValueError(f"--nonrigid_lcc_radius must be an integer in 1..{MAX_LCC_RADIUS}, got {nonrigid_lcc_radius}")


def nonrigid_stage(fixed0, outs, interp, fill, levels, iterations, sigma, max_step, nonrigid="demons", exp_steps=2, once=None,
                   force="ssd", lcc_radius=2):
    """The field of frame 0 against the fixed scan, applied to every resliced frame -> (warped frames, DeformResult).  ``once =
    (original frames, matrix)``: every output frame is instead one interpolation of its original frame through matrix and field.
    ``force="lcc"``: the force across contrasts with windows of ``lcc_radius`` voxels either side (``volume_deform.lcc_force_np``)."""
    chosen = dict(force=force, lcc_radius=lcc_radius) if force != "ssd" else {}
    if isinstance(iterations, (list, tuple)) and len(iterations) == 1:
        iterations = int(iterations[0])
    if nonrigid == "diffeomorphic":
        result = register_diffeomorphic(fixed0, outs[0], levels=levels, iterations=iterations, sigma_vox=sigma, max_step=max_step,
                                        fill=fill, method=interp, exp_steps=exp_steps, **chosen)
    else:
        result = register_deformable(fixed0, outs[0], levels=levels, iterations=iterations, sigma_vox=sigma, max_step=max_step, fill=fill,
                                     method=interp, **chosen)
    for line in describe_nonrigid(result, force):
        logger.info(f"Non-rigid stage, {line}")
    min_det, folded = result.jacobian
    logger.info(f"Non-rigid stage: minimum Jacobian determinant {min_det:.4f}, {folded} voxel(s) with a determinant that is not positive")
    if folded:
        logger.warning(f"The field folds at {folded} voxel(s): raise --nonrigid_sigma (now {sigma:g}) for a smoother field.")
    if once is not None:
        frames, matrix = once
        logger.info(f"Non-rigid stage: every frame is interpolated once, through the rigid matrix and the field ({interp}).")
        return [warp_matrix(f, matrix, result.field, interp, fill) for f in frames], result
    return [result.warped] + [warp(o, result.field, interp, fill) for o in outs[1:]], result


def register_file(fixed_path, moving_path, output_path, interp="linear", bins=64, save_transform=None, fill=0.0, device="cuda",
                  init="header", init_limit=40.0, init_step=20.0, mask="none", nonrigid="none", nonrigid_levels=3,
                  nonrigid_iterations=DEFAULT_ITERATIONS, nonrigid_sigma=1.5, nonrigid_max_step=2.0, save_field=None, nonrigid_exp_steps=2,
                  nonrigid_resample="twice", nonrigid_force="ssd", nonrigid_lcc_radius=2):
    """NIfTI files -> the moving scan on the fixed scan's grid (written and returned), and the ``RigidResult``."""
    if mask not in ("none", "otsu"):
        raise ValueError(f"--mask must be none or otsu, got {mask}")
    check_options(nonrigid, nonrigid_exp_steps, nonrigid_resample, save_field, nonrigid_force, nonrigid_lcc_radius)
    fixed, fixed_header = read_nifti(fixed_path)
    moving, moving_header = read_nifti(moving_path)
    frames = [to_device(f, device) for f in frames_of(moving)]
    fixed0 = fixed if fixed.ndim == 3 else fixed[..., 0]
    fixed0 = to_device(fixed0, device)
    fixed_affine, shape = fixed_header.affine(), tuple(fixed.shape[:3])
    result = register_rigid(fixed0, fixed_affine, frames[0], moving_header.affine(), bins=bins, mask_cost=mask == "otsu", init=init,
                            init_limit=init_limit, init_step=init_step)
    if init == "global":
        logger.info(f"Registering {moving_path} to {fixed_path}, {describe_coarse(result)}")
    logger.info(f"Registered {moving_path} to {fixed_path}: {describe(result)}")
    outs = [reslice(f, result.matrix, shape, interp, fill) for f in frames]
    share = covered_share(moving.shape[:3], result.matrix, shape, device)
    if nonrigid != "none":
        outs, deformed = nonrigid_stage(fixed0, outs, interp, fill, nonrigid_levels, nonrigid_iterations, nonrigid_sigma, nonrigid_max_step,
                                        nonrigid, nonrigid_exp_steps, (frames, result.matrix) if nonrigid_resample == "once" else None,
                                        nonrigid_force, nonrigid_lcc_radius)
        if save_field:
            field = np.ascontiguousarray(np.moveaxis(deformed.field.cpu().numpy(), 0, 3))
            field_header = header_for_grid(fixed_header, shape, fixed_affine)
            dim = list(field_header.get("dim"))
            dim[0], dim[4] = 4, 3                                       # three frames: the components along the grid's axes
            field_header.set("dim", dim)
            save_nifti(save_field, field, field_header)
            logger.info(f"Field {tuple(field.shape)} (voxels of the fixed grid) saved to {save_field}")
    data = join_frames([o.cpu().numpy() for o in outs], moving.ndim)
    logger.info(f"{100.0 * (1.0 - float(share)):.2f} % of the output voxels fell outside the moving scan (set to {fill:g}).")
    save_nifti(output_path, data, header_for_grid(moving_header, shape, fixed_affine))
    logger.info(f"Moving scan {tuple(moving.shape)} -> {tuple(data.shape)} ({interp}) saved to {output_path}")
    if save_transform:
        make_parent(save_transform)
        np.savetxt(save_transform, result.world, fmt="%.17g", header="fixed world -> moving world (mm), 4 x 4")
        logger.info(f"Transform saved to {save_transform}")
    return data, result


def _body(args, device):
    register_file(args.fixed, args.moving, args.output, args.interp, args.bins, args.save_transform, args.fill, device, args.init,
                  args.init_limit, args.init_step, args.mask, args.nonrigid, args.nonrigid_levels, args.nonrigid_iterations,
                  args.nonrigid_sigma, args.nonrigid_max_step, args.save_field, args.nonrigid_exp_steps, args.nonrigid_resample,
                  args.nonrigid_force, args.nonrigid_lcc_radius)


def main(args):
    return run(_body, args, logger, "registration")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Rigid registration of a NIfTI volume to another (extension)")
    p.add_argument("--fixed", type=str, required=True, help="the scan whose grid the output lands on: single-file NIfTI-1, 3-D or 4-D")
    p.add_argument("--moving", type=str, required=True, help="the scan to bring onto it: single-file NIfTI-1, 3-D or 4-D")
    p.add_argument("--output", type=str, required=True, help="the moving scan on the fixed grid, .nii or .nii.gz, float32")
    p.add_argument("--interp", type=str, choices=["linear", "cubic"], default="linear", help="interpolation of the final reslice")
    p.add_argument("--bins", type=int, choices=[16, 32, 64], default=64, help="bins per axis of the joint histogram")
    p.add_argument("--init", type=str, choices=["header", "global"], default="header",
                   help="header: start from the two headers as they are; global: start from the best of a coarse grid of rotations "
                        "about the two Otsu masks' centres of mass (scans centimetres and tens of degrees apart)")
    p.add_argument("--init_limit", type=float, default=40.0, help="--init global: the grid spans +- this many degrees per axis")
    p.add_argument("--init_step", type=float, default=20.0, help="--init global: the grid's step in degrees")
    p.add_argument("--mask", type=str, choices=["none", "otsu"], default="none",
                   help="otsu: only the samples inside the fixed scan's Otsu foreground mask enter the cost")
    p.add_argument("--save_transform", type=str, default=None, help="write the 4 x 4 fixed world -> moving world matrix as text")
    p.add_argument("--fill", type=float, default=0.0, help="value of the output voxels whose centre lies outside the moving scan")
    p.add_argument("--nonrigid", type=str, choices=["none", "demons", "diffeomorphic"], default="none",
                   help="demons: after the rigid stage and its reslice, estimate a displacement field against the fixed scan (Thirion's "
                        "demons, an intensity-difference force: bring both scans onto one intensity scale first) and write the warped "
                        "scan instead; the output is then interpolated twice unless --nonrigid_resample once; diffeomorphic: the same "
                        "with the update composed with the field through its exponential, not added: a field that does not fold")
    p.add_argument("--nonrigid_force", type=str, choices=["ssd", "lcc"], default="ssd",
                   help="the force of --nonrigid demons / diffeomorphic.  ssd: the intensity difference (scans of one contrast on one "
                        "intensity scale); lcc: a locally normalised correlation force for scans of DIFFERENT contrast (64 mT against "
                        "3 T): every window gets its own affine intensity relation and only its residual drives the field")
    p.add_argument("--nonrigid_lcc_radius", type=int, default=2, help="--nonrigid_force lcc: the window is this many voxels either side (1..4)")
    p.add_argument("--nonrigid_exp_steps", type=int, default=2,
                   help="--nonrigid diffeomorphic: squarings of the exponential of one update (0..8; the update is scaled by 2^-N first)")
    p.add_argument("--nonrigid_resample", type=str, choices=["twice", "once"], default="twice",
                   help="twice: warp the resliced scan (as before); once: write every frame as ONE interpolation of the original moving "
                        "frame through the rigid matrix and the field (needs --nonrigid demons or diffeomorphic)")
    p.add_argument("--nonrigid_levels", type=int, default=3, help="--nonrigid demons: levels of the pyramid (halved while every extent is even and at least 16)")
    p.add_argument("--nonrigid_iterations", type=int, nargs="+", default=list(DEFAULT_ITERATIONS),
                   help="--nonrigid demons: iterations per level, coarse to fine (one count per level, or one for all)")
    p.add_argument("--nonrigid_sigma", type=float, default=1.5, help="--nonrigid demons: sigma of the field's Gaussian in voxels of a level (at most 5.33)")
    p.add_argument("--nonrigid_max_step", type=float, default=2.0, help="--nonrigid demons: bound of one iteration's update in voxels")
    p.add_argument("--save_field", type=str, default=None,
                   help="--nonrigid demons: write the field as a 4-D float32 NIfTI of three frames (voxels of the fixed grid)")
    add_cpu_flag(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
