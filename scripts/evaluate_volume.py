#!/usr/bin/env python3
"""Volume evaluation (extension): ground-truth NIfTI scans in, SSIM / PSNR tables of the x2 U-Net and the
x2 interpolation baselines out.

    python scripts/evaluate_volume.py --reference hr.nii.gz [more.nii.gz ...] --checkpoint_dir ./checkpoints --isotropic

Every reference scan is uploaded once.  Its low-resolution volume is the mean over pairs along the doubled axes
(``volume_eval.downsample2``) or, with ``--input``, the given scan (one reference only; half of the reference's extents on the
doubled axes) - the way to score a simulated low-field acquisition.  The doubled axes are all three with ``--isotropic``, else
the two in-plane axes of the slices across ``--axis``.  Methods: ``unet`` (``scripts/infer_volume.py``'s path), with
``--isotropic`` also ``unet_axis2_linear`` (one slice pass across axis 2 plus linear through-plane interpolation: the
alternative to the three-plane blend), ``linear`` and ``cubic``.  The metrics are 3-D: Gaussian-window SSIM over the volume,
MSE, RMSE, MAE, PSNR with ``--data_range`` (default: max - min of the reference), all computed on the device
(``csrc/volume_metrics.hip``).  A 4-D file is scored timepoint by timepoint.  One table per scan, the mean over scans, and the
same rows in ``--output_csv``.  Checkpoint flags and the exit code (0 / 1, error logged) are those of ``scripts/infer_volume.py``.

``--mask otsu`` scores every method inside a foreground mask as well: an exact Otsu threshold on the reference volume's 256-bin
histogram, closed with a box of ``--mask_close`` voxels (``csrc/volume_mask.hip``); ``--mask PATH`` takes the mask from a NIfTI-1
file of the reference's spatial shape instead (any voxel type, non-zero = foreground; a 3-D mask serves every timepoint).  Each
scan then prints a second table headed "foreground" (voxel count, share of the volume, Otsu threshold), the means come for both
regions, and the CSV gains a ``region`` column (``whole`` / ``foreground``).  Still one pass over the volumes per method and one
download per volume.

``--mask_largest`` keeps the largest 26-connected component of the (closed) mask - specks of background above the threshold go -
and ``--mask_fill_holes 3d|0|1|2`` then fills its holes, those of the volume or of every plane across an axis - CSF, sinuses and
ventricles come back (``csrc/volume_label.hip``: connected components on the device).  The "foreground" title then also says
"N components, kept K voxels, filled F".  ``--save_mask PATH`` writes the mask that was actually scored, after crop and clean-up,
as a uint8 NIfTI under the reference's header (one reference only; a 4-D reference gives a 4-D mask).  All three need ``--mask``.

``--align header`` (with ``--input``) lifts the demand of exactly half the extents: the input scan is resliced on the device through
the two headers' affines (``volume_reslice.reslice``, ``--align_interp linear|cubic``) onto the grid a x2 pass expects -
``utils.nifti.downscaled_affine`` of the reference's affine over the doubled axes, the reference's extents (after its crop to even
ones) halved on them - whatever its spacing, field of view, axis order or rotation; the share of that grid the input covers is
logged.  A ``--mask PATH`` on another grid is then resliced onto the reference's grid with ``nearest``.  The transform is not
estimated: the headers are taken as they are.

``--align rigid`` estimates it: the input is first registered to the reference - six rigid parameters, normalised mutual
information, starting from the two headers (``volume_register.register_rigid``, ``--align_bins``; frame 0 of a 4-D pair) - and
then resliced ONCE onto the same low-resolution grid through ``inv(A_input) W A_low``, ``W`` the estimated reference world ->
input world matrix: never two interpolations.  The parameters found and the NMI before and after are logged.  Two scans of one
head from two scanners or two sessions never share a world frame to sub-voxel accuracy; with ``--align header`` their table
measures patient positioning, with ``--align rigid`` the methods.  ``--align_init global`` starts the registration from the best of a
coarse grid of rotations about the two Otsu masks' centres of mass (world frames centimetres and tens of degrees apart, where the
start from the headers ends in a wrong local optimum); ``--align_mask otsu`` counts only the samples inside the reference's Otsu
foreground in its cost.  Both go with ``--align rigid`` only.

``--match_intensity landmarks|range`` (with ``--input``) handles what geometry does not: MR intensities are in arbitrary units, and
on a real pair the input differs from the reference by a scale, an offset and usually a monotone contrast curve - MSE, RMSE, MAE and
PSNR then measure the gain setting of two scanners, and so do SSIM's luminance and contrast terms.  After the ``--align`` reslice,
if there is one, and once, before any method sees it, every input frame is mapped onto its reference frame's intensity scale: the
piecewise-linear function that sends the percentiles 1, 10, ..., 90, 99 (``range``: 1 and 99) of the input's foreground onto those
of the reference's (``volume_intensity.match_intensity``, Nyul-Udupa; ``csrc/volume_intensity.hip``).  Each side's foreground is
its own Otsu mask (``volume_eval.foreground_mask``, no closing), whatever ``--mask`` says; the voxels a reslice left at the fill
value 0 fall below Otsu's threshold and do not move the landmarks.  The landmarks and the voxel counts are logged.  The default,
``none``, leaves a run as it was.

``--match_bias pair`` (with ``--input``) handles what a global map cannot: the slowly varying gain across the head (B1 / coil
sensitivity), strong at 3 T, weak at low field and different in every session.  After the ``--align`` reslice and after
``--match_intensity``, before any method sees it, every input frame is multiplied by the ratio of two masked Gaussian low-passes
(``volume_bias.match_bias``, ``--match_bias_sigma_mm``, default 25 mm; ``csrc/volume_bias.hip``): that of the reference frame's mean
over pairs (``volume_eval.downsample2``, on the input's grid) over its own, inside the intersection of the two Otsu foregrounds
``--match_intensity`` uses.  The default, ``none``, leaves a run as it was.

``--denoise_input nlm`` (with ``--input``) takes the noise out of every input frame first of all, on the frame's own grid and BEFORE
the ``--align`` reslice - interpolation correlates the noise of neighbouring voxels, and the Rayleigh estimate of sigma needs raw
air: the Rician non-local-means filter of ``volume_denoise.denoise_volume`` (``csrc/volume_denoise.hip``), sigma estimated per frame
from the background or given with ``--denoise_sigma``, ``--denoise_beta`` (default 1) scaling the filter's strength,
``--denoise_radius`` (default 3) its search window.  Sigma and the background count are logged.  The default, ``none``, leaves a
run as it was.

``--unring_input`` takes the Gibbs ringing of a truncated k-space out of every input frame on its own grid, after
``--denoise_input`` and BEFORE the ``--align`` reslice (interpolation destroys the ringing's period): Kellner's local subvoxel shifts
(``volume_unring.unring``, ``csrc/volume_unring.hip``) along ``--unring_axes`` (default all three, 8..512 voxels each) with
``--unring_shifts`` K (default 20) and ``--unring_window`` a b (default 1 3).  Without ``--input`` it goes with ``--degrade kspace`` /
``kspace_hamming`` and unrings the low-resolution volume that degradation makes (even extents on the doubled axes).  Minimum,
maximum and total variation are logged before and after, and the tables' titles name the step.  Without the flag a run is as it was.

``--deform_input demons`` (with ``--input``) handles what a rigid transform cannot: the non-rigid geometry between two scanners
(gradient non-linearity, susceptibility distortion).  After the ``--align`` reslice, ``--match_intensity`` and ``--match_bias``,
every input frame is warped onto ``downsample2`` of its reference frame (the input's grid, or the grid ``--align`` implies) through a
displacement field estimated by Thirion's demons (``volume_deform.register_deformable``; ``csrc/volume_deform.hip``) with
``--align_interp``: the frame is then interpolated twice.  The force is an intensity difference, so a run without
``--match_intensity`` is warned about.  ``--deform_force lcc`` (``--deform_lcc_radius``) takes the force across contrasts instead
(``volume_deform.lcc_force``; ``csrc/volume_lcc.hip``): every window of the scans gets its own affine intensity relation, so neither a
common intensity scale nor that warning is needed, and the log reports ``1 - mean rho^2``.  ``--deform_input diffeomorphic`` estimates the field by diffeomorphic demons instead
(``volume_deform.register_diffeomorphic``, ``--deform_exp_steps`` squarings of an update's exponential): the update is composed with
the field, not added, so the warped frame is not that of a folded field.  The default, ``none``, leaves a run as it was.

``--tissue_dice K`` (2..6, with ``--mask``) asks what SSIM and PSNR answer only indirectly - whether a method keeps the anatomy: the
reference and every method's output are segmented into K tissue classes inside the mask (``volume_tissue.segment_tissue``: a Gaussian
mixture on 256 bins with a Potts prior, iterated conditional modes; ``csrc/volume_tissue.hip``), the reference once, and the Dice
overlap per class, class 1 the darkest, is appended to the foreground tables and as the columns ``dice_1 ... dice_K`` to the CSV
(empty in the rows of the whole volume).  A last row ``reference`` - the reference against itself, Dice 1 - checks the path.  The
default, 0, leaves a run as it was.

``--tissue_surface`` (with ``--tissue_dice K``) adds how far the boundaries between the tissue classes have moved, in millimetres: the
average symmetric surface distance and the 95th-percentile Hausdorff distance per class between the method's and the reference's
tissue interfaces (``volume_surface.surface_distances`` with ``background=False``: an exact Euclidean distance transform with the
voxel sizes of the reference's header; ``csrc/volume_surface.hip``), as the columns ``assd_1 ... assd_K, hd95_1 ... hd95_K`` after the
Dice columns (empty in the rows of the whole volume, 0 in the row ``reference``, NaN for a class without an interface).  Without the
switch a run is as it was.

``--tissue_edges`` (with ``--tissue_dice K``) asks what none of the above can: whether a method's edges are sharper than interpolation's.
SSIM and PSNR reward smoothness, Dice and the surface distances are blind to the slope of an edge.  The signed distance of every voxel
to each of the K - 1 interfaces between the REFERENCE's tissue classes is taken once, with the voxel sizes of the reference's header;
one pass per method then gives the mean intensity of its output as a function of that distance, in bins of ``--edge_bin_mm`` (default
0.5) out to ``--edge_radius_mm`` (default 4) on either side (``volume_sharpness.edge_sharpness``; ``csrc/volume_edge.hip``).  Appended
after the Dice and surface columns: ``esw_1 ... esw_{K-1}``, the 10 % - 90 % width of that edge-spread function in millimetres (smaller
is sharper), and ``econ_1 ... econ_{K-1}``, the contrast of its two plateaus as a ratio to the reference row's (1 in the row
``reference``); empty in the rows of the whole volume, NaN where a crossing is not reached.  Without the switch a run is as it was.

``--zerofill none|hamming`` adds the baseline an MR reader expects first: what the scanner itself shows as its "interpolated matrix",
k-space padded with zeros and transformed back - periodic sinc interpolation of the same low-resolution volume over the same axes
(``volume_kspace.zerofill2``; ``csrc/volume_kspace.hip``), ``hamming`` with that window on k-space.  The row ``zerofill``
(``zerofill_hamming``) follows ``cubic`` and is scored like every other.  ``--degrade kspace|kspace_hamming`` makes the low-resolution
volume of a run without ``--input`` by truncating the reference's k-space to its centre (``volume_kspace.truncate2``), the resolution
loss of the 2-D training path (``csrc/lowfield.hip``), instead of the mean over pairs; the tables' titles then say so.  With ``--input``
it is ignored, with a warning.  Without the two flags a run writes the bytes it wrote before.

``--degrade_noise SIGMA`` or ``--degrade_snr R`` (without ``--input``, with any ``--degrade``, the default ``mean`` included; even extents
on the doubled axes) makes the low-resolution volume a simulated low-field acquisition: it is made first, then Rician noise of
standard deviation SIGMA - or the median of its Otsu foreground over R - is added (``volume_lowfield.add_noise``;
``csrc/volume_noise.hip``), seeded by ``--degrade_seed`` (default 0; every scan and frame draws its own noise) and reproducible to the
bit.  The U-Net is trained on noisy low-resolution slices; this scores it on such input.  The tables' titles say so: ``(degrade
kspace, noise σ = 20, seed 0)``.  With one of the two, ``--denoise_input nlm`` is accepted without ``--input`` and denoises the volume
just made, before ``--unring_input``: truncate, noise, denoise, x2, against a real truth.  Without the flags a run writes the bytes it
wrote before.
"""
import argparse
import csv
import logging
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from mri_superresolution_amd.utils.evalops import METRIC_COLUMNS          # noqa: E402
from mri_superresolution_amd.utils.nifti import downscaled_affine, frames, grid_matrix, read_nifti, write_nifti   # noqa: E402
from mri_superresolution_amd.volume_bias import match_bias as match_bias_field, sigmas_for                  # noqa: E402
from mri_superresolution_amd.volume_deform import MAX_EXP_STEPS, MAX_LCC_RADIUS, register_deformable, register_diffeomorphic      # noqa: E402
from mri_superresolution_amd.volume_denoise import denoise_volume                                             # noqa: E402
from mri_superresolution_amd.volume_eval import downsample2, evaluate_volume, foreground_mask, otsu_threshold_value      # noqa: E402
from mri_superresolution_amd.volume_intensity import LANDMARKS, RANGE, match_intensity    # noqa: E402
from mri_superresolution_amd.volume_register import register_rigid                         # noqa: E402
from mri_superresolution_amd.volume_reslice import covered_share, reslice    # noqa: E402
from mri_superresolution_amd.volume_sharpness import check_bins as check_edge_bins        # noqa: E402
from mri_superresolution_amd.volume_kspace import truncate2                  # noqa: E402
from mri_superresolution_amd.volume_lowfield import add_noise, frame_seeds, sigma_for_snr      # noqa: E402
from scripts._cli import (add_cpu_flag, add_degrade_noise_flags, add_kspace_flags, add_unring_flags, degrade_noise_options, join_frames,   # noqa: E402
                          kspace_options, load_mask, log_device, make_parent, require_gpu, start_logging, to_device, unring_frame,
                          unring_options, voxel_sizes)

logger = logging.getLogger("evaluate_volume")
CSV_COLUMNS = ["scan", "method", "ssim", "psnr", "mse", "rmse", "mae"]      # the column style of scripts/evaluate.py
CSV_COLUMNS_MASKED = ["scan", "region", "method", "ssim", "psnr", "mse", "rmse", "mae"]      # with --mask
REGIONS = ("whole", "foreground")


def dice_columns(classes):
    """The columns ``--tissue_dice K`` appends."""
    return [f"dice_{k}" for k in range(1, classes + 1)]


def surface_columns(classes):
    """The columns ``--tissue_surface`` appends after those of ``--tissue_dice K``."""
    return [f"{name}_{k}" for name in ("assd", "hd95") for k in range(1, classes + 1)]


def edge_columns(classes):
    """The columns ``--tissue_edges`` appends after those of ``--tissue_dice K`` and ``--tissue_surface``: one per interface."""
    return [f"{name}_{k}" for name in ("esw", "econ") for k in range(1, classes)]


def check_options(input_path, align, align_interp, align_init, align_mask, match, match_bias="none", match_bias_sigma_mm=25.0,
                  denoise_input="none", denoise_sigma=None, denoise_beta=1.0, denoise_radius=3, deform_input="none", deform_exp_steps=2,
                  tissue_dice=0, mask=None, tissue_surface=False, deform_force="ssd", deform_lcc_radius=2, tissue_edges=False,
                  edge_radius_mm=4.0, edge_bin_mm=0.5, degrade_noise=None):
    """The option rules of one scan, stated once: ``score_scan`` applies them, ``main`` before it loads a model."""
    if degrade_noise is not None:
        if input_path:
            raise ValueError("--degrade_noise and --degrade_snr go without --input: they add noise to the low-resolution volume made here")
        level = degrade_noise.get("sigma", degrade_noise.get("snr"))
        if len([k for k in ("sigma", "snr") if k in degrade_noise]) != 1 or not np.isfinite(level) or level < 0 or (level == 0 and "snr" in degrade_noise):
            raise ValueError(f"--degrade_noise takes a finite sigma that is not negative, --degrade_snr a finite positive ratio, one of the two; got {degrade_noise}")
    if isinstance(tissue_dice, bool) or not isinstance(tissue_dice, int) or not (tissue_dice == 0 or 2 <= tissue_dice <= 6):
        raise ValueError(f"--tissue_dice is 0 (off) or a number of classes in 2..6, got {tissue_dice}")
    if tissue_dice and mask is None:
        raise ValueError("--tissue_dice goes with --mask")
    if tissue_surface and not tissue_dice:
        raise ValueError("--tissue_surface goes with --tissue_dice")
    if tissue_edges:
        if not tissue_dice:
            raise ValueError("--tissue_edges goes with --tissue_dice")
        check_edge_bins(edge_radius_mm, edge_bin_mm)                 # --edge_radius_mm and --edge_bin_mm: at most 64 bins
    if deform_input not in ("none", "demons", "diffeomorphic"):
        raise ValueError(f"--deform_input is none, demons or diffeomorphic, got {deform_input!r}")
    if isinstance(deform_exp_steps, bool) or not isinstance(deform_exp_steps, int) or not 0 <= deform_exp_steps <= MAX_EXP_STEPS:
        raise ValueError(f"--deform_exp_steps must be an integer in 0..{MAX_EXP_STEPS}, got {deform_exp_steps}")
    if deform_input != "none" and not input_path:
        raise ValueError("--deform_input goes with --input")
    if deform_force not in ("ssd", "lcc"):
        raise ValueError(f"--deform_force is ssd or lcc, got {deform_force!r}")
    if deform_force == "lcc" and deform_input == "none":
        raise ValueError("--deform_force lcc goes with --deform_input demons or diffeomorphic")
    if isinstance(deform_lcc_radius, bool) or not isinstance(deform_lcc_radius, int) or not 1 <= deform_lcc_radius <= MAX_LCC_RADIUS:
        raise ValueError(f"--deform_lcc_radius must be an integer in 1..{MAX_LCC_RADIUS}, got {deform_lcc_radius}")
    if denoise_input not in ("none", "nlm"):
        raise ValueError(f"--denoise_input is none or nlm, got {denoise_input!r}")
    if denoise_input != "none" and not input_path and degrade_noise is None:
        raise ValueError("--denoise_input goes with --input")
    if denoise_sigma is not None and not (np.isfinite(denoise_sigma) and denoise_sigma > 0):
        raise ValueError(f"--denoise_sigma must be finite and positive, got {denoise_sigma}")
    if not (np.isfinite(denoise_beta) and denoise_beta > 0) or denoise_radius not in (1, 2, 3, 4, 5):
        raise ValueError(f"--denoise_beta must be finite and positive and --denoise_radius in 1..5, got {denoise_beta} and {denoise_radius}")
    if match_bias not in ("none", "pair"):
        raise ValueError(f"--match_bias is none or pair, got {match_bias!r}")
    if match_bias != "none" and not input_path:
        raise ValueError("--match_bias goes with --input")
    if not (np.isfinite(match_bias_sigma_mm) and match_bias_sigma_mm >= 0):
        raise ValueError(f"--match_bias_sigma_mm must be finite and not negative, got {match_bias_sigma_mm}")
    if match not in ("none", "landmarks", "range"):
        raise ValueError(f"--match_intensity is none, range or landmarks, got {match!r}")
    if match != "none" and not input_path:
        raise ValueError("--match_intensity goes with --input")
    if align not in (None, "header", "rigid"):
        raise ValueError(f"align must be None, 'header' or 'rigid', got {align!r}")
    if align and not input_path:
        raise ValueError("--align goes with --input")
    if align and align_interp not in ("linear", "cubic"):
        raise ValueError(f"--align_interp must be linear or cubic, got {align_interp}")
    if align_init not in ("header", "global") or align_mask not in ("none", "otsu"):
        raise ValueError(f"--align_init is header or global and --align_mask none or otsu, got {align_init} and {align_mask}")
    if align != "rigid" and (align_init != "header" or align_mask != "none"):
        raise ValueError("--align_init and --align_mask go with --align rigid")


def upload_input(frame, device="cuda", denoise_input="none", denoise_sigma=None, denoise_beta=1.0, denoise_radius=3, onto=None,
                 what="input", unring=None):
    """One input frame (a numpy array) -> the CUDA tensor the rest of the run works on: uploaded, with ``denoise_input="nlm"``
    denoised on its own grid (``volume_denoise.denoise_volume``, sigma estimated from the frame's background unless given), and only
    then, with ``onto = (matrix, shape, interpolation)``, resliced (``--align``).  ``unring`` (the keywords of ``volume_unring.unring``):
    unringed on its own grid after the denoising and before the reslice.  ``"none"``, no ``unring`` and no ``onto``: the upload alone."""
    lr = clean_input(torch.from_numpy(np.ascontiguousarray(frame)).to(device), denoise_input, denoise_sigma, denoise_beta, denoise_radius,
                     what, unring)
    if onto is not None:
        lr = reslice(lr, *onto)
    return lr


def clean_input(lr, denoise_input="none", denoise_sigma=None, denoise_beta=1.0, denoise_radius=3, what="input", unring=None):
    """The first two steps of ``upload_input`` on a CUDA volume, in its order: the denoising, then the unringing."""
    if denoise_input != "none":
        lr, noise = denoise_volume(lr, sigma=denoise_sigma, beta=denoise_beta, radius=denoise_radius, return_noise=True)
        logger.info(f"{what} denoised (nlm, radius {denoise_radius}, beta {denoise_beta:g}): sigma {noise['sigma']:.6g}"
                    + (f" from {noise['count']} background voxels" if denoise_sigma is None else " (given)"))
    if unring is not None:
        lr = unring_frame(lr, unring, logger, f"{what}: ")
    return lr


def low_reference(lr, vol, axes, option):
    """``downsample2(vol, axes)``, the reference on the input's grid (cropped to twice the input where it is larger)."""
    want = tuple(2 * d if a in axes else d for a, d in enumerate(lr.shape))
    if any(w > d for w, d in zip(want, vol.shape)):
        raise ValueError(f"{option}: the input {tuple(lr.shape)} is not half of the reference {tuple(vol.shape)} on the axes {axes}")
    return downsample2(vol[:want[0], :want[1], :want[2]].contiguous(), axes)


def prepare_input(lr, vol, match="none", match_bias="none", axes=(0, 1, 2), sigmas_vox=None, what="input", reference="its reference",
                  deform="none", deform_interp="linear", deform_exp_steps=2, deform_force="ssd", deform_lcc_radius=2):
    """What ``--match_intensity``, ``--match_bias`` and ``--deform_input`` do to one input frame ``lr`` next to its reference frame
    ``vol`` (CUDA tensors) -> the frame every method sees.  ``match`` first, then ``match_bias="pair"`` against
    ``downsample2(vol, axes)`` - the reference on the input's grid - with ``sigmas_vox`` on that grid, then ``deform="demons"``: a
    displacement field against that same low reference (``volume_deform.register_deformable``), the frame warped through it with
    ``deform_interp``; ``deform="diffeomorphic"``: the field of ``volume_deform.register_diffeomorphic`` with ``deform_exp_steps``.
    ``deform_force="lcc"``: either registration with the force across contrasts (``volume_deform.lcc_force_np``, windows of
    ``deform_lcc_radius`` voxels either side), which needs no common intensity scale.  All ``"none"``: ``lr`` itself."""
    if match != "none":
        lr, found = match_intensity(lr, vol, foreground_mask(lr)[0], foreground_mask(vol)[0], LANDMARKS if match == "landmarks" else RANGE)
        marks = "  ".join(f"{q:g}%: {a:.6g} -> {b:.6g}" for q, a, b in zip(found.percentiles, found.source_landmarks, found.target_landmarks))
        logger.info(f"{what} mapped onto the intensity scale of {reference} ({match}): {found.source_count} input and "
                    f"{found.target_count} reference foreground voxels; landmarks {marks}")
    if match_bias != "none":
        low_ref = low_reference(lr, vol, axes, "--match_bias")
        lr = match_bias_field(lr, low_ref, foreground_mask(lr)[0], foreground_mask(low_ref)[0], sigmas_vox, want_field=False)[0]
        logger.info(f"{what}: bias field matched to that of {reference} (sigmas {tuple(round(float(x), 3) for x in sigmas_vox)} voxels)")
    if deform != "none":
        chosen = dict(force=deform_force, lcc_radius=deform_lcc_radius) if deform_force != "ssd" else {}
        if match == "none" and deform_force != "lcc":
            logger.warning("--deform_input without --match_intensity: the demons force is an intensity difference, and the two scans "
                           "are not on one intensity scale.")
        if deform == "diffeomorphic":
            found = register_diffeomorphic(low_reference(lr, vol, axes, "--deform_input"), lr, method=deform_interp, exp_steps=deform_exp_steps,
                                           **chosen)
        else:
            found = register_deformable(low_reference(lr, vol, axes, "--deform_input"), lr, method=deform_interp, **chosen)
        first, last = found.stats[0], found.stats[-1]
        if deform_force == "lcc":
            cost = f"1 - mean rho^2 {1.0 - first[0] / max(first[1], 1):.6g} -> {1.0 - last[0] / max(last[1], 1):.6g}"
        else:
            cost = f"mean squared difference {first[0] / max(first[1], 1):.6g} -> {last[0] / max(last[1], 1):.6g}"
        logger.info(f"{what} warped onto {reference} ({deform}, {deform_interp}): {cost} over {len(found.stats)} iterations on {len(found.schedule)} level(s); minimum Jacobian "
                    f"determinant {found.jacobian[0]:.4f}, {found.jacobian[1]} voxel(s) not positive")
        lr = found.warped
    return lr


def score_scan(model, reference_path, input_path=None, isotropic=False, axis=2, data_range=None, batch_size=16, use_amp=False,
               use_graph=True, device="cuda", graph_cache=None, mask=None, mask_close=0, mask_largest=False, mask_fill_holes=None,
               save_mask=None, align=None, align_interp="linear", align_bins=64, align_init="header", align_mask="none",
               match="none", match_bias="none", match_bias_sigma_mm=25.0, denoise_input="none", denoise_sigma=None, denoise_beta=1.0,
               denoise_radius=3, deform_input="none", deform_exp_steps=2, tissue_dice=0, tissue_surface=False, deform_force="ssd",
               deform_lcc_radius=2, tissue_edges=False, edge_radius_mm=4.0, edge_bin_mm=0.5, zerofill=None, degrade="mean", unring_input=None,
               degrade_noise=None, scan_index=0):
    """-> rows ``{"scan", "method", *METRIC_COLUMNS}``, one per timepoint and method.  ``mask`` (``"otsu"`` or a NIfTI path): two
    rows per timepoint and method, with ``"region"`` (``whole`` / ``foreground``), ``"mask_voxels"``, ``"voxels"`` and, for Otsu,
    ``"threshold"``; with ``mask_largest`` / ``mask_fill_holes`` also ``"cleanup"`` (components, kept size, voxels filled; NaN for a
    step that is off).  ``save_mask``: the masks scored go to this NIfTI file.  ``align="header"``: ``input_path`` (and a mask file)
    may lie on any grid and are resliced through the headers' affines (module docstring); ``align="rigid"``: the input is registered
    to the reference first and resliced once through the estimated transform; ``align_init="global"`` starts that registration
    from a coarse grid of rotations about the masks' centres of mass, ``align_mask="otsu"`` puts the reference's Otsu mask in its
    cost (``volume_register.register_rigid``).  ``match`` (``"landmarks"`` / ``"range"``): every input frame is mapped onto its
    reference frame's intensity scale before any method sees it (module docstring); ``match_bias="pair"``: then its bias field is
    matched to the reference's (``prepare_input``).  ``denoise_input="nlm"``: every input frame is denoised on its own grid before
    anything else happens to it (``upload_input``).  ``deform_input="demons"``: after all of that every input frame is warped onto its
    reference frame on the input's grid (``prepare_input``); ``"diffeomorphic"`` with ``deform_exp_steps`` likewise;
    ``deform_force="lcc"`` with ``deform_lcc_radius``: the force across contrasts in either.
    ``tissue_dice`` K (needs ``mask``): the rows of the foreground carry ``dice_1 ... dice_K``, the Dice overlap of the method's tissue
    classes with the reference's (``""`` in the rows of the whole volume), and a last method ``reference`` is scored.
    ``tissue_surface`` (needs ``tissue_dice``): those rows also carry ``surface_columns(K)``, in the world units of the reference's header.
    ``tissue_edges`` (needs ``tissue_dice``): those rows also carry ``edge_columns(K)``, the widths in those units and the contrasts as
    ratios to the row ``reference``'s; ``edge_radius_mm`` and ``edge_bin_mm`` set the profile's range and bins.
    ``zerofill`` (``"none"`` / ``"hamming"``): a method ``zerofill`` (``zerofill_hamming``) follows ``cubic``; ``degrade`` (``"kspace"`` /
    ``"kspace_hamming"``): the low-resolution volume is the reference's truncated k-space (``volume_eval.evaluate_volume``).
    ``unring_input`` (the keywords of ``volume_unring.unring``: axes, K, window): every input frame is unringed on its own grid after
    ``denoise_input`` and before ``align`` (``upload_input``); without ``input_path`` the low-resolution volume a k-space ``degrade`` makes
    is unringed instead (even extents on the doubled axes).
    ``degrade_noise`` (``{"sigma": s}`` or ``{"snr": r}``, with ``"seed"``; without ``input_path``): the low-resolution volume is made
    here from the reference by ``degrade``, the mean over pairs included, and Rician noise is added to it (``volume_lowfield.add_noise``;
    ``snr``: sigma is the median of the volume's Otsu foreground over ``r``); frame ``t`` of scan number ``scan_index`` draws with
    ``volume_lowfield.frame_seeds(seed, scan_index, frames)[t]``.  ``denoise_input="nlm"`` then denoises that volume, before
    ``unring_input`` (even extents on the doubled axes)."""
    check_options(input_path, align, align_interp, align_init, align_mask, match, match_bias, match_bias_sigma_mm, denoise_input,
                  denoise_sigma, denoise_beta, denoise_radius, deform_input, deform_exp_steps, tissue_dice, mask, tissue_surface,
                  deform_force, deform_lcc_radius, tissue_edges, edge_radius_mm, edge_bin_mm, degrade_noise)
    noise_options = (denoise_input, denoise_sigma, denoise_beta, denoise_radius)
    if unring_input is not None and not input_path and degrade == "mean":
        raise ValueError("--unring_input goes with --input or with --degrade kspace / kspace_hamming")
    ref, ref_header = read_nifti(reference_path)
    low, low_header = read_nifti(input_path) if input_path else (None, None)
    if low is not None and low.ndim != ref.ndim:
        raise ValueError(f"{input_path} has {low.ndim} axes, {reference_path} has {ref.ndim}")
    if low is not None and low.ndim == 4 and low.shape[3] != ref.shape[3]:
        raise ValueError(f"{input_path} has {low.shape[3]} timepoints, {reference_path} has {ref.shape[3]}")
    ref_frames, low_frames = frames(ref), (frames(low) if low is not None else None)
    masks = load_mask(mask, ref, ref_header.affine() if align else None) if mask not in (None, "otsu") else None
    axes = (0, 1, 2) if isotropic else tuple(a for a in (0, 1, 2) if a != axis)
    bias_sigmas = sigmas_for(downscaled_affine(ref_header.affine(), axes), match_bias_sigma_mm) if match_bias != "none" else None
    if align:
        # the grid a x2 pass over the doubled axes expects its input on; the crop takes trailing voxels, so the affine stays
        crop = tuple(d - d % 2 if a in axes else d for a, d in enumerate(ref.shape[:3]))
        if 0 in crop:
            raise ValueError(f"nothing is left of the reference volume {tuple(ref.shape[:3])} after cropping to even extents")
        if crop != tuple(ref.shape[:3]):
            logger.warning(f"Reference volume {tuple(ref.shape[:3])} has an odd extent on a doubled axis: cropped to {crop}.")
            ref_frames = [f[:crop[0], :crop[1], :crop[2]] for f in ref_frames]
            if masks is not None:
                masks = [f[:crop[0], :crop[1], :crop[2]].contiguous() for f in masks]
        low_shape = tuple(d // 2 if a in axes else d for a, d in enumerate(crop))
        low_grid = downscaled_affine(ref_header.affine(), axes)
        if align == "rigid":
            # fixed = the reference, moving = the input, from the headers as they are (p0 = 0); W: reference world -> input world
            fixed, moving = to_device(frames(ref)[0], device), to_device(low_frames[0], device)
            found = register_rigid(fixed, ref_header.affine(), moving, low_header.affine(), bins=align_bins, init=align_init,
                                   mask_cost=align_mask == "otsu")
            p = found.p
            logger.info(f"{input_path} registered to {reference_path}: t = ({p[0]:.4f}, {p[1]:.4f}, {p[2]:.4f}) mm, r = ({p[3]:.4f}, "
                        f"{p[4]:.4f}, {p[5]:.4f}) degrees, NMI {found.trace[0]['best']:.6f} -> {found.value:.6f} in "
                        f"{found.n_evaluations} evaluations.")
            low_grid = found.world @ low_grid
            del fixed, moving
        m = grid_matrix(low_header.affine(), low_grid)
        low_frames = [upload_input(f, device, *noise_options, onto=(m, low_shape, align_interp),
                                   what=f"{input_path}{f'[t={t}]' if len(low_frames) > 1 else ''}", unring=unring_input)
                      for t, f in enumerate(low_frames)]
        share = float(covered_share(low.shape[:3], m, low_shape, device))
        logger.info(f"{input_path} {tuple(low.shape[:3])} resliced onto the low-resolution grid {low_shape} of {reference_path} "
                    f"({align_interp}); it covers {100.0 * share:.2f} % of that grid.")
    graphs = graph_cache if graph_cache is not None else {}
    name = os.path.basename(reference_path)
    rows, saved = [], []
    for t, frame in enumerate(ref_frames):
        vol = torch.from_numpy(np.ascontiguousarray(frame)).to(device)
        lr, m = None, mask
        if low_frames is not None:      # with --align the frames are on the device already
            lr = low_frames[t] if align else upload_input(low_frames[t], device, *noise_options,
                                                          what=f"{input_path}{f'[t={t}]' if len(ref_frames) > 1 else ''}",
                                                          unring=unring_input)
        made = (unring_input is not None or degrade_noise is not None) and lr is None       # the low-resolution volume is made here
        if made and degrade_noise is None:                   # the truncated k-space of the reference, unringed
            if any(vol.shape[a] % 2 for a in axes):
                raise ValueError(f"--unring_input with --degrade {degrade}: the reference {tuple(vol.shape)} has an odd extent on a doubled axis")
            vol = vol.float().contiguous()
            lr = unring_frame(truncate2(vol, axes, "hamming" if degrade == "kspace_hamming" else "none"), unring_input, logger,
                              f"{name}{f'[t={t}]' if len(ref_frames) > 1 else ''} (degrade {degrade}): ")
        elif made:                                           # degraded, then noise; denoised and unringed on request, in upload_input's order
            if any(vol.shape[a] % 2 for a in axes):
                raise ValueError(f"--degrade_noise / --degrade_snr: the reference {tuple(vol.shape)} has an odd extent on a doubled axis")
            what = f"{name}{f'[t={t}]' if len(ref_frames) > 1 else ''} (degrade {degrade})"
            vol = vol.float().contiguous()
            lr = downsample2(vol, axes) if degrade == "mean" else truncate2(vol, axes, "hamming" if degrade == "kspace_hamming" else "none")
            sigma = degrade_noise["sigma"] if "sigma" in degrade_noise else sigma_for_snr(lr, degrade_noise["snr"])
            seed = frame_seeds(degrade_noise.get("seed", 0), scan_index, len(ref_frames))[t]
            lr = add_noise(lr, sigma, seed, out=lr)
            logger.info(f"{what}: Rician noise added, sigma {sigma:.6g}, seed {seed}")
            lr = clean_input(lr, *noise_options, what=what, unring=unring_input)
        if masks is not None:
            m = masks[t] if align else torch.from_numpy(masks[t]).to(device)
        if lr is not None and not made:
            lr = prepare_input(lr, vol, match, match_bias, axes, bias_sigmas, f"{input_path}{f'[t={t}]' if len(ref_frames) > 1 else ''}",
                               reference_path, deform_input, align_interp, deform_exp_steps, deform_force, deform_lcc_radius)
        res = evaluate_volume(model, vol, lr=lr, isotropic=isotropic, axis=axis, val_range=data_range, batch_size=batch_size,
                              use_amp=use_amp, use_graph=use_graph, graph_cache=graphs, mask=m, mask_close=mask_close, mask_largest=mask_largest,
                              mask_fill_holes=mask_fill_holes, tissue_dice=tissue_dice, tissue_surface=tissue_surface,
                              spacing=voxel_sizes(ref_header.affine()) if tissue_surface or tissue_edges else None,
                              **(dict(tissue_edges=True, edge_radius=edge_radius_mm, edge_bin=edge_bin_mm) if tissue_edges else {}),
                              **(dict(zerofill=zerofill) if zerofill is not None else {}), **(dict(degrade=degrade) if degrade != "mean" and not made else {}))
        scan = name if len(ref_frames) == 1 else f"{name}[t={t}]"
        if mask is None:
            values = torch.stack(list(res.values())).cpu().numpy()            # one download per volume
            for method, vals in zip(res, values):
                rows.append({"scan": scan, "method": method, **dict(zip(METRIC_COLUMNS, (float(v) for v in vals)))})
            continue
        # the (2, 5) results of every method, the clean-up's three numbers, the mask's voxel count and the four mask statistics:
        # still one download per volume
        stats = res.mask_stats if res.mask_stats is not None else torch.full((4,), float("nan"), dtype=torch.float64, device=device)
        cleanup = res.mask_cleanup if res.mask_cleanup is not None else torch.full((3,), float("nan"), dtype=torch.float64, device=device)
        down = torch.cat([v.reshape(10) for v in res.values()] + [cleanup, res.mask_count.reshape(1), stats]).cpu().numpy()
        lo, hi, tstar, _ = down[-4:]
        extra = {"voxels": int(res.mask.numel()), "mask_voxels": int(down[-5]),
                 "threshold": otsu_threshold_value(lo, hi, int(tstar)) if res.mask_stats is not None else None,
                 "cleanup": tuple(float(c) for c in down[-8:-5]) if res.mask_cleanup is not None else None}
        if save_mask:
            saved.append(res.mask.cpu().numpy())
        for r, region in enumerate(REGIONS):
            for i, method in enumerate(res):
                vals = down[10 * i + 5 * r:10 * i + 5 * r + 5]
                rows.append({"scan": scan, "region": region, "method": method, **extra,
                             **dict(zip(METRIC_COLUMNS, (float(v) for v in vals)))})
                if tissue_dice:
                    overlap = res.tissue_dice[method]
                    rows[-1].update({c: float(overlap[k]) if region == "foreground" else "" for k, c in enumerate(dice_columns(tissue_dice))})
                if tissue_surface:
                    found = res.tissue_surface[method]
                    values = [float(x) for x in found.assd] + [float(x) for x in found.hd95]
                    rows[-1].update({c: v if region == "foreground" else "" for c, v in zip(surface_columns(tissue_dice), values)})
                if tissue_edges:
                    found, own = res.tissue_edges[method], res.tissue_edges["reference"]
                    with np.errstate(divide="ignore", invalid="ignore"):
                        values = [float(x) for x in found.width] + [float(x) for x in found.contrast / own.contrast]
                    rows[-1].update({c: v if region == "foreground" else "" for c, v in zip(edge_columns(tissue_dice), values)})
    if save_mask:
        data = join_frames(saved, ref.ndim)
        header = ref_header.copy()                              # the reference's, with the extents left after the crop
        dim = list(header.get("dim"))
        dim[1:4] = data.shape[:3]
        header.set("dim", dim)
        write_nifti(save_mask, data, header)
        logger.info(f"Saved the mask {tuple(data.shape)} to {save_mask}")
    return rows


def format_table(title, rows, dice=()):
    """``dice``: the columns of ``--tissue_dice`` and ``--tissue_surface`` to append (the foreground tables)."""
    lines = [title, f"{'method':18s} {'SSIM':>8s} {'PSNR':>8s} {'MSE':>12s} {'RMSE':>10s} {'MAE':>10s}" + "".join(f" {c:>8s}" for c in dice)]
    for r in rows:
        lines.append(f"{r['method']:18s} {r['ssim']:8.4f} {r['psnr']:8.3f} {r['mse']:12.6g} {r['rmse']:10.6g} {r['mae']:10.6g}"
                     + "".join(f" {r[c]:8.4f}" for c in dice))
    return "\n".join(lines)


def mean_rows(rows, dice=()):
    """``dice``: the columns of ``--tissue_dice`` and ``--tissue_surface``, averaged like the metrics where the rows carry numbers (the foreground)."""
    methods = list(dict.fromkeys(r["method"] for r in rows))
    columns = list(METRIC_COLUMNS) + [c for c in dice if rows and rows[0][c] != ""]
    return [{"scan": "mean", "method": m, **{c: "" for c in dice}, **{k: float(np.mean([r[k] for r in rows if r["method"] == m])) for k in columns}}
            for m in methods]


def foreground_title(rows):
    r = rows[0]
    title = f"foreground: {r['mask_voxels']} voxels, {100.0 * r['mask_voxels'] / r['voxels']:.1f} % of the volume"
    title += f", Otsu threshold {r['threshold']:.6g}" if r["threshold"] is not None else ""
    if r.get("cleanup") is not None:
        found, kept, filled = r["cleanup"]
        parts = [f"{int(found)} components, kept {int(kept)} voxels"] if found == found else []      # NaN: that step is off
        parts += [f"filled {int(filled)}"] if filled == filled else []
        title += ", " + ", ".join(parts)
    return title


def main(args):
    start_logging()
    try:
        device = require_gpu(args)
        if args.batch_size < 1:
            raise ValueError(f"--batch_size must be positive, got {args.batch_size}")
        if args.input and len(args.reference) != 1:
            raise ValueError("--input goes with exactly one --reference scan")
        if args.data_range is not None and not args.data_range > 0:
            raise ValueError(f"--data_range must be positive, got {args.data_range}")
        if args.mask is None and args.mask_close != 0:
            raise ValueError("--mask_close goes with --mask")
        if args.mask is None and (args.mask_largest or args.mask_fill_holes is not None or args.save_mask):
            raise ValueError("--mask_largest, --mask_fill_holes and --save_mask go with --mask")
        check_options(args.input, args.align, args.align_interp, args.align_init, args.align_mask, args.match_intensity, args.match_bias,
                      args.match_bias_sigma_mm, args.denoise_input, args.denoise_sigma, args.denoise_beta, args.denoise_radius,
                      args.deform_input, args.deform_exp_steps, args.tissue_dice, args.mask, args.tissue_surface, args.deform_force,
                      args.deform_lcc_radius, args.tissue_edges, args.edge_radius_mm, args.edge_bin_mm, degrade_noise_options(args))
        if args.save_mask and len(args.reference) != 1:
            raise ValueError("--save_mask goes with exactly one --reference scan")
        if not 0 <= args.mask_close <= 4:
            raise ValueError(f"--mask_close must be in 0..4, got {args.mask_close}")
        from scripts.infer import find_best_checkpoint, load_model
        log_device(device, logger)
        if args.checkpoint_path and os.path.exists(args.checkpoint_path):
            ckpt = args.checkpoint_path
        else:
            ckpt = find_best_checkpoint(args.checkpoint_dir, args.model_type)
        logger.info(f"Checkpoint: {ckpt}")
        model = load_model(args.model_type, ckpt, device, base_filters=args.base_filters)
        fill = args.mask_fill_holes if args.mask_fill_holes in (None, "3d") else int(args.mask_fill_holes)
        rows, graphs = [], {}
        regions = REGIONS if args.mask else (None,)
        dice = dice_columns(args.tissue_dice) + (surface_columns(args.tissue_dice) if args.tissue_surface else [])
        dice += edge_columns(args.tissue_dice) if args.tissue_edges else []
        shown = {"foreground": dice}                     # the tables of the whole volume stay as they are
        degraded = f" (degrade {args.degrade})" if args.degrade != "mean" else ""
        degrade_noise = degrade_noise_options(args)
        if degrade_noise is not None:
            level = f"σ = {degrade_noise['sigma']:g}" if "sigma" in degrade_noise else f"SNR = {degrade_noise['snr']:g}"
            degraded = f" (degrade {args.degrade}, noise {level}, seed {degrade_noise['seed']})"
            if args.denoise_input != "none":
                degraded += " (denoised)"
        unring_input = unring_options(args, "unring_input")
        if unring_input is not None:                     # what it goes with: score_scan's rule
            degraded += f" (input unringed along {' '.join(str(a) for a in sorted(unring_input['axes']))}, K = {unring_input['K']})"
        for index, path in enumerate(args.reference):
            scan_rows = score_scan(model, path, input_path=args.input, isotropic=args.isotropic, axis=args.axis, data_range=args.data_range,
                                   batch_size=args.batch_size, use_amp=args.use_amp, use_graph=not args.no_graph, device=device,
                                   graph_cache=graphs, mask=args.mask, mask_close=args.mask_close, mask_largest=args.mask_largest,
                                   mask_fill_holes=fill, save_mask=args.save_mask, align=args.align, align_interp=args.align_interp,
                                   align_bins=args.align_bins, align_init=args.align_init, align_mask=args.align_mask,
                                   match=args.match_intensity, match_bias=args.match_bias, match_bias_sigma_mm=args.match_bias_sigma_mm,
                                   denoise_input=args.denoise_input, denoise_sigma=args.denoise_sigma, denoise_beta=args.denoise_beta,
                                   denoise_radius=args.denoise_radius, deform_input=args.deform_input,
                                   deform_exp_steps=args.deform_exp_steps, deform_force=args.deform_force,
                                   deform_lcc_radius=args.deform_lcc_radius, tissue_dice=args.tissue_dice,
                                   tissue_surface=args.tissue_surface, tissue_edges=args.tissue_edges,
                                   edge_radius_mm=args.edge_radius_mm, edge_bin_mm=args.edge_bin_mm, **kspace_options(args),
                                   **(dict(unring_input=unring_input) if unring_input is not None else {}),
                                   **(dict(degrade_noise=degrade_noise, scan_index=index) if degrade_noise is not None else {}))
            for scan in dict.fromkeys(r["scan"] for r in scan_rows):
                for region in regions:
                    part = [r for r in scan_rows if r["scan"] == scan and r.get("region") == region]
                    print(format_table(foreground_title(part) if region == "foreground" else scan + degraded, part, shown.get(region, ())))
            rows += scan_rows
        means = []
        for region in regions:
            part = [r for r in rows if r.get("region") == region]
            title = f"mean over {len(set(r['scan'] for r in part))} scan(s)"
            mean = mean_rows(part, dice)
            if region is not None:
                mean = [{**r, "region": region} for r in mean]
            print(format_table(f"foreground, {title}" if region == "foreground" else title + degraded, mean, shown.get(region, ())))
            means += mean
        if args.output_csv:
            make_parent(args.output_csv)
            columns = (CSV_COLUMNS_MASKED if args.mask else CSV_COLUMNS) + dice
            with open(args.output_csv, "w", newline="") as f:
                wr = csv.DictWriter(f, fieldnames=columns)
                wr.writeheader()
                for r in rows + means:
                    wr.writerow({k: r[k] for k in columns})
            logger.info(f"Saved {len(rows) + len(means)} rows to {args.output_csv}")
        return 0
    except Exception as e:
        logger.error(f"Error during volume evaluation: {e}")
        return 1


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Evaluate x2 volume enhancement against interpolation baselines (extension)")
    p.add_argument("--reference", type=str, nargs="+", required=True, help="ground-truth scan(s): single-file NIfTI-1, 3-D or 4-D")
    p.add_argument("--input", type=str, default=None,
                   help="low-resolution scan of the one --reference (half its extents on the doubled axes); default: the mean over pairs")
    p.add_argument("--checkpoint_dir", type=str, default="./checkpoints")
    p.add_argument("--checkpoint_path", type=str, default=None)
    p.add_argument("--model_type", type=str, choices=["unet"], default="unet")
    p.add_argument("--base_filters", type=int, default=64)
    add_cpu_flag(p)
    add_unring_flags(p, "unring_input", "of every --input frame on its own grid, after --denoise_input and before --align (without --input: "
                                        "of the low-resolution volume --degrade kspace makes)")
    p.add_argument("--use_amp", action="store_true", help="fp16 MFMA compute (the reference's autocast)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--isotropic", action="store_true", help="double all three axes (the three-plane blend of infer_volume.py --isotropic)")
    g.add_argument("--axis", type=int, choices=[0, 1, 2], default=2, help="slices are taken across this axis; the two others are doubled")
    p.add_argument("--data_range", type=float, default=None, help="R of SSIM's constants and of PSNR; default: max - min of each reference volume")
    p.add_argument("--batch_size", type=int, default=16, help="slices per forward")
    p.add_argument("--no_graph", action="store_true", help="do not replay the forward of full batches as a HIP graph")
    p.add_argument("--mask", type=str, default=None,
                   help="score inside a foreground mask as well: 'otsu' (exact Otsu threshold of each reference volume, on the device) or "
                        "a NIfTI-1 mask of the reference's spatial shape (non-zero = foreground)")
    p.add_argument("--mask_close", type=int, default=0, help="close the mask with a box of this radius in voxels (0..4; needs --mask)")
    p.add_argument("--mask_largest", action="store_true", help="keep the largest 26-connected component of the mask (needs --mask)")
    p.add_argument("--mask_fill_holes", type=str, choices=["3d", "0", "1", "2"], default=None,
                   help="fill the holes of the mask: those of the volume (3d) or of every plane across this axis (needs --mask)")
    p.add_argument("--save_mask", type=str, default=None,
                   help="write the mask that was scored, after crop and clean-up, as a uint8 NIfTI with the reference's header (one "
                        "--reference; needs --mask)")
    p.add_argument("--align", type=str, choices=["header", "rigid"], default=None,
                   help="reslice --input (and a --mask file) through the NIfTI headers' affines onto the grid the reference implies, "
                        "instead of demanding exactly half its extents (needs --input); rigid: register the input to the reference "
                        "first (six parameters, mutual information) and reslice it once through the estimated transform")
    p.add_argument("--align_interp", type=str, choices=["linear", "cubic"], default="linear", help="interpolation of the --align reslice")
    p.add_argument("--align_bins", type=int, choices=[16, 32, 64], default=64, help="bins per axis of --align rigid's joint histogram")
    p.add_argument("--align_init", type=str, choices=["header", "global"], default="header",
                   help="--align rigid: start from the headers, or (global) from the best of a coarse grid of rotations about the two "
                        "Otsu masks' centres of mass, for scans centimetres and tens of degrees apart")
    p.add_argument("--align_mask", type=str, choices=["none", "otsu"], default="none",
                   help="--align rigid: otsu counts only the samples inside the reference's Otsu foreground in the registration's cost")
    p.add_argument("--match_intensity", type=str, choices=["none", "range", "landmarks"], default="none",
                   help="map every --input frame onto its reference frame's intensity scale before any method sees it: the percentiles "
                        "1, 10, ..., 90, 99 (landmarks) or 1 and 99 (range) of the two Otsu foregrounds (needs --input)")
    p.add_argument("--match_bias", type=str, choices=["none", "pair"], default="none",
                   help="match every --input frame's bias field to its reference frame's (the ratio of two masked Gaussian low-passes, "
                        "inside the two Otsu foregrounds), after --align and --match_intensity (needs --input)")
    p.add_argument("--match_bias_sigma_mm", type=float, default=25.0, help="sigma of --match_bias's low-pass in millimetres")
    p.add_argument("--denoise_input", type=str, choices=["none", "nlm"], default="none",
                   help="denoise every --input frame on its own grid, before the --align reslice: the Rician non-local-means filter, "
                        "sigma estimated from the frame's background (needs --input)")
    p.add_argument("--denoise_sigma", type=float, default=None, help="the noise level of --denoise_input, in intensity units (default: estimated)")
    p.add_argument("--denoise_beta", type=float, default=1.0, help="strength of --denoise_input: h^2 = 2 beta sigma^2 per patch voxel")
    p.add_argument("--denoise_radius", type=int, default=3, help="search radius of --denoise_input in voxels, 1..5")
    p.add_argument("--deform_input", type=str, choices=["none", "demons", "diffeomorphic"], default="none",
                   help="demons: warp every input frame onto its reference frame on the input's grid (downsample2 of the reference, or "
                        "the grid --align implies) by a demons displacement field, after the --align reslice, --match_intensity and "
                        "--match_bias; warped with --align_interp, so the frame is then interpolated twice (needs --input; an "
                        "intensity-difference force: use --match_intensity); diffeomorphic: the same with the update composed with the "
                        "field through its exponential, not added - a field that does not fold")
    p.add_argument("--deform_exp_steps", type=int, default=2, help="--deform_input diffeomorphic: squarings of an update's exponential, 0..8")
    p.add_argument("--deform_force", type=str, choices=["ssd", "lcc"], default="ssd",
                   help="the force of --deform_input.  ssd: the intensity difference (use --match_intensity); lcc: a locally normalised "
                        "correlation force for an input of another contrast than its reference - no common intensity scale is needed")
    p.add_argument("--deform_lcc_radius", type=int, default=2, help="--deform_force lcc: the window is this many voxels either side (1..4)")
    p.add_argument("--tissue_dice", type=int, default=0,
                   help="segment the reference and every method's output into this many tissue classes (2..6) inside the mask and append "
                        "the Dice overlap per class, dice_1 ... dice_K (needs --mask; 0: off)")
    p.add_argument("--tissue_surface", action="store_true",
                   help="append the surface distances per class between every method's and the reference's tissue interfaces in mm: "
                        "assd_1 ... assd_K, hd95_1 ... hd95_K (needs --tissue_dice)")
    p.add_argument("--tissue_edges", action="store_true",
                   help="append the 10 %% - 90 %% width in mm of every method's edge across each interface between the reference's tissue "
                        "classes, esw_1 ... esw_{K-1}, and the contrast across it as a ratio to the reference's, econ_1 ... econ_{K-1} "
                        "(needs --tissue_dice)")
    p.add_argument("--edge_radius_mm", type=float, default=4.0, help="--tissue_edges: the profile runs this far either side of an interface")
    p.add_argument("--edge_bin_mm", type=float, default=0.5, help="--tissue_edges: the width of a bin of the profile (at most 64 bins)")
    add_kspace_flags(p)
    add_degrade_noise_flags(p)
    p.add_argument("--output_csv", type=str, default=None, help="write every row and the means to this CSV file")
    return p.parse_args(argv)


if __name__ == "__main__":
    sys.exit(main(parse_args()))
