#!/usr/bin/env python3
"""Whole-volume inference (extension): a NIfTI-1 scan in, the x2-enhanced scan out.

    python scripts/infer_volume.py --input scan.nii.gz --output out.nii.gz --checkpoint_dir ./checkpoints

The reference has no such driver: it reaches the network only through 8-bit PNG slices that its extraction script cuts out of
the volumes.  Here the volume is uploaded once; every slice across ``--axis`` is windowed at its own 0.5 / 99.5 percentiles
(exact selection on the float data, ``csrc/percentile.hip``), enhanced, restored to its intensity window and written into the
output volume on the device (``mri_superresolution_amd/volume.py``); one download, then the NIfTI file with ``dim`` doubled,
``pixdim`` halved and the sform / qform moved so that the volume stays where it was in world space
(``mri_superresolution_amd/utils/nifti.py``).  A 4-D file is processed timepoint by timepoint.  Checkpoint flags, checkpoint
search order and the exit code (0 / 1, error logged) are those of ``scripts/infer.py``.

``--isotropic`` doubles all three axes: the slices across axis 0, 1 and 2 are enhanced in turn, each result is interpolated
along its own slice axis and the three are averaged on the device (``volume.enhance_volume_isotropic``,
``csrc/volume_blend.hip``); a 1 mm scan comes out at 0.5 mm in every direction.

``--spacing SX SY SZ`` (mm, 0 keeps an axis) reslices the uploaded volume to that voxel size on the device before windowing and
enhancement (``volume_reslice.reslice``, ``--spacing_interp linear|cubic``): a 1.5 x 1.5 x 5 mm scan with
``--spacing 0 0 1.5 --isotropic`` comes out at 0.75 mm in every direction.  The output header is that of the respaced grid
(``utils.nifti.respaced_grid`` / ``header_for_grid``) after the x2 write.

``--denoise nlm`` takes the noise out of the uploaded volume first of all, before the ``--spacing`` reslice and the windowing: the
Rician non-local-means filter of ``volume_denoise.denoise_volume`` (``csrc/volume_denoise.hip``), sigma estimated per volume from
the air around the head or given with ``--denoise_sigma``; ``--denoise_beta`` (default 1) scales the filter's strength,
``--denoise_radius`` (default 3) is its search radius.  The default, ``none``, leaves a run as it was.

``--unring`` takes the Gibbs ringing of a truncated k-space out after ``--denoise`` and before the ``--spacing`` reslice and the
windowing (interpolation destroys the ringing's period): Kellner's local subvoxel shifts along ``--unring_axes`` (default all
three, 8..512 voxels each) with ``--unring_shifts`` K (default 20) and ``--unring_window`` a b (default 1 3), ``volume_unring.unring``
(``csrc/volume_unring.hip``).  Minimum, maximum and total variation are logged before and after.  Without the flag a run is as it was.
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

from mri_superresolution_amd.utils.nifti import frames, grid_matrix, header_for_grid, read_nifti, respaced_grid, write_nifti   # noqa: E402
from mri_superresolution_amd.volume import enhance_volume, enhance_volume_isotropic   # noqa: E402
from mri_superresolution_amd.volume_denoise import denoise_volume        # noqa: E402
from mri_superresolution_amd.volume_reslice import reslice               # noqa: E402
from scripts._cli import add_unring_flags, unring_frame, unring_options   # noqa: E402
from scripts.infer import find_best_checkpoint, load_model               # noqa: E402

logger = logging.getLogger("infer_volume")


def process_volume(model, input_path, output_path, axis=2, batch_size=16, use_amp=False, use_graph=True, output_dtype="float32",
                   device="cuda", isotropic=False, spacing=None, spacing_interp="linear", denoise="none", denoise_sigma=None,
                   denoise_beta=1.0, denoise_radius=3, unring=None):
    """NIfTI file -> NIfTI file; returns the output array (as written).  ``spacing`` (three voxel sizes in mm, 0 or ``None`` keeps
    an axis): every volume is resliced to that spacing on the device before it is windowed and enhanced.  ``denoise="nlm"``: every
    volume is denoised before that (``volume_denoise.denoise_volume``; ``denoise_sigma`` None: estimated from its background).  ``unring`` (the keywords of
    ``volume_unring.unring``: axes, K, window): every volume is unringed after the denoising and before the reslice, which would
    destroy the ringing's period."""
    if denoise not in ("none", "nlm"):
        raise ValueError(f"--denoise is none or nlm, got {denoise!r}")
    data, header = read_nifti(input_path)
    dtype = {"float32": torch.float32, "int16": torch.int16}[output_dtype]
    in_plane = (0, 1, 2) if isotropic else tuple(a for a in (0, 1, 2) if a != axis)
    if isotropic:
        logger.info("Isotropic mode: slices across all three axes, every axis doubled; --axis is not used.")
    shape, regrid = tuple(data.shape[:3]), None
    if spacing is not None and any(spacing):
        if spacing_interp not in ("linear", "cubic"):
            raise ValueError(f"--spacing_interp must be linear or cubic, got {spacing_interp}")
        affine = header.affine()
        new_affine, shape = respaced_grid(affine, shape, spacing)
        regrid = grid_matrix(affine, new_affine)
        header = header_for_grid(header, shape, new_affine)
        logger.info(f"Reslicing {tuple(data.shape[:3])} to {shape} voxels ({spacing_interp}) before enhancement.")
    if any(shape[a] % 8 for a in in_plane):
        logger.warning(f"In-plane dimensions {tuple(shape[a] for a in in_plane)} are not divisible by 8. This might affect "
                       "performance or spatial accuracy due to model pooling layers.")
    outs, graphs = [], {}
    for frame in frames(data):
        vol = torch.from_numpy(np.ascontiguousarray(frame)).to(device)
        if denoise != "none":
            vol, noise = denoise_volume(vol, sigma=denoise_sigma, beta=denoise_beta, radius=denoise_radius, return_noise=True)
            logger.info(f"Denoised (nlm, radius {denoise_radius}, beta {denoise_beta:g}): sigma {noise['sigma']:.6g}"
                        + (f" from {noise['count']} background voxels" if denoise_sigma is None else " (given)"))
        if unring is not None:
            vol = unring_frame(vol, unring, logger)
        if regrid is not None:
            vol = reslice(vol, regrid, shape, spacing_interp)
        if isotropic:
            out = enhance_volume_isotropic(model, vol, batch_size=batch_size, use_amp=use_amp, use_graph=use_graph, out_dtype=dtype,
                                           graph_cache=graphs)
        else:
            out = enhance_volume(model, vol, axis=axis, batch_size=batch_size, use_amp=use_amp, use_graph=use_graph, out_dtype=dtype,
                                 graph_cache=graphs)
        outs.append(out.cpu().numpy())
    result = outs[0] if data.ndim == 3 else np.stack(outs, axis=3)
    os.makedirs(os.path.dirname(os.path.abspath(output_path)), exist_ok=True)
    write_nifti(output_path, result, header, in_plane)
    logger.info(f"Enhanced volume {tuple(data.shape)} -> {tuple(result.shape)} saved to {output_path}")
    return result


def main(args):
    try:
        if args.cpu or not torch.cuda.is_available():
            raise RuntimeError("this build runs on MI355X only (hand-written HIP kernels, no CPU fallback)")
        device = torch.device("cuda")
        logger.info(f"Using device: {device} ({torch.cuda.get_device_name(0)})")
        if args.use_amp:
            logger.info("Using Automatic Mixed Precision (AMP) for inference.")
        if args.batch_size < 1:
            raise ValueError(f"--batch_size must be positive, got {args.batch_size}")
        if args.checkpoint_path and os.path.exists(args.checkpoint_path):
            ckpt = args.checkpoint_path
            logger.info(f"Using specified checkpoint: {ckpt}")
        else:
            ckpt = find_best_checkpoint(args.checkpoint_dir, args.model_type)
            logger.info(f"Automatically selected checkpoint: {ckpt}")
        model = load_model(args.model_type, ckpt, device, base_filters=args.base_filters)
        process_volume(model, args.input, args.output, args.axis, args.batch_size, args.use_amp, not args.no_graph,
                       args.output_dtype, device, isotropic=args.isotropic, spacing=getattr(args, "spacing", None),
                       spacing_interp=getattr(args, "spacing_interp", "linear"), denoise=getattr(args, "denoise", "none"),
                       denoise_sigma=getattr(args, "denoise_sigma", None), denoise_beta=getattr(args, "denoise_beta", 1.0),
                       denoise_radius=getattr(args, "denoise_radius", 3), unring=unring_options(args, "unring"))
        logger.info("Inference completed successfully!")
        return 0
    except Exception as e:
        logger.error(f"Error during inference: {e}")
        return 1


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="MRI quality enhancement inference on whole NIfTI volumes (extension)")
    p.add_argument("--input", type=str, required=True, help="(extension) input scan: single-file NIfTI-1, .nii or .nii.gz, 3-D or 4-D")
    p.add_argument("--output", type=str, required=True, help="(extension) output scan, .nii or .nii.gz: in-plane size doubled (every axis with --isotropic)")
    p.add_argument("--checkpoint_dir", type=str, default="./checkpoints")
    p.add_argument("--checkpoint_path", type=str, default=None)
    p.add_argument("--model_type", type=str, choices=["unet"], default="unet")
    p.add_argument("--base_filters", type=int, default=64)
    p.add_argument("--cpu", action="store_true", help="REFUSED: accepted only so that the reference's command lines parse; this build runs on an MI355X through "
                        "libmrisr.so only and exits with an error when --cpu is given (there is no CPU fallback)")
    p.add_argument("--use_amp", action="store_true", help="fp16 MFMA compute (the reference's autocast)")
    p.add_argument("--axis", type=int, choices=[0, 1, 2], default=2,
                   help="(extension) slices are taken across this axis; 2 is the reference's data[:, :, idx], the orientation of training")
    p.add_argument("--isotropic", action="store_true",
                   help="(extension) double all three axes: the passes across axis 0, 1 and 2, each interpolated along its slice axis, "
                        "averaged on the device; --axis is not used")
    p.add_argument("--batch_size", type=int, default=16, help="(extension) slices per forward")
    p.add_argument("--no_graph", action="store_true", help="(extension) do not replay the forward of full batches as a HIP graph")
    p.add_argument("--output_dtype", type=str, choices=["float32", "int16"], default="float32",
                   help="(extension) stored type of the output: float32, or int16 rounded half to even and saturated")
    # absent from the namespace unless given: the parsed defaults are those of a build without the two flags
    p.add_argument("--spacing", type=float, nargs=3, default=argparse.SUPPRESS, metavar=("SX", "SY", "SZ"),
                   help="(extension) reslice the volume to this voxel size in mm on the device before enhancement; 0 keeps an axis")
    p.add_argument("--spacing_interp", type=str, choices=["linear", "cubic"], default=argparse.SUPPRESS,
                   help="(extension) interpolation of the --spacing reslice (default: linear)")
    p.add_argument("--denoise", type=str, choices=["none", "nlm"], default=argparse.SUPPRESS,
                   help="(extension) denoise the uploaded volume before --spacing and the windowing: nlm, the Rician non-local-means "
                        "filter with sigma from the background (default: none)")
    p.add_argument("--denoise_sigma", type=float, default=argparse.SUPPRESS,
                   help="(extension) the noise level of --denoise in intensity units (default: estimated from the air around the head)")
    p.add_argument("--denoise_beta", type=float, default=argparse.SUPPRESS, help="(extension) strength of --denoise (default: 1)")
    p.add_argument("--denoise_radius", type=int, default=argparse.SUPPRESS, help="(extension) search radius of --denoise, 1..5 (default: 3)")
    add_unring_flags(p, "unring", "of the uploaded volume after --denoise and before --spacing and the windowing")
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
