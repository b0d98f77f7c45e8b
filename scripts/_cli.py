"""What the volume scripts share: the ``--cpu`` flag, the k-space flags, the degradation's noise flags, the unring flags, the guarded ``main``, the upload of a frame, the joining
and saving of frames, and the mask loading of ``evaluate_volume.py`` and ``segment_volume.py``.  A script imports it after the
``REPO`` path insert.
"""
import logging
import os

import numpy as np
import torch

from mri_superresolution_amd.utils.nifti import grid_matrix, mask_frames, write_nifti
from mri_superresolution_amd.volume_reslice import reslice_mask
from mri_superresolution_amd.volume_stacks import voxel_sizes      # noqa: F401  (the scripts take it from here)

logger = logging.getLogger("volume_cli")


def add_cpu_flag(parser):
    parser.add_argument("--cpu", action="store_true", help="REFUSED: this build runs on an MI355X through libmrisr.so only (there is no CPU fallback)")


def add_kspace_flags(parser):
    """``--zerofill`` and ``--degrade`` of ``evaluate_volume.py`` (``volume_kspace``); ``kspace_options`` reads them back."""
    parser.add_argument("--zerofill", type=str, choices=["none", "hamming"], default=None,
                        help="add the baseline an MR scanner gives: k-space zero-filling (periodic sinc interpolation) of the same "
                             "low-resolution volume, as the row zerofill - with the k-space window hamming as zerofill_hamming "
                             "(no row unless the flag is present)")
    parser.add_argument("--degrade", type=str, choices=["mean", "kspace", "kspace_hamming"], default="mean",
                        help="how the low-resolution volume is made from the reference: the mean over pairs, or k-space truncation "
                             "(kspace_hamming: with a Hamming window), the degradation of the 2-D training path; ignored with --input")


def kspace_options(args) -> dict:
    """-> the keywords of ``score_scan`` / ``volume_eval.evaluate_volume`` for the two flags; empty when neither is used."""
    chosen = {}
    if args.zerofill is not None:
        chosen["zerofill"] = args.zerofill
    if args.degrade != "mean":
        chosen["degrade"] = args.degrade
    return chosen


def add_degrade_noise_flags(parser):
    """``--degrade_noise`` / ``--degrade_snr`` / ``--degrade_seed`` of ``evaluate_volume.py`` (``volume_lowfield``); absent from the
    namespace unless given, so the parsed defaults are those of a build without them.  ``degrade_noise_options`` reads them back."""
    import argparse
    g = parser.add_mutually_exclusive_group()
    g.add_argument("--degrade_noise", type=float, default=argparse.SUPPRESS, metavar="SIGMA",
                   help="(extension) without --input: add Rician noise of this sigma, in intensity units, to the low-resolution volume "
                        "made from the reference (any --degrade, the default mean included) - a simulated low-field acquisition")
    g.add_argument("--degrade_snr", type=float, default=argparse.SUPPRESS, metavar="R",
                   help="(extension) the same with sigma = the median of that volume's Otsu foreground / R")
    parser.add_argument("--degrade_seed", type=int, default=argparse.SUPPRESS, metavar="N",
                        help="(extension) the seed of --degrade_noise / --degrade_snr; every scan and frame draws its own noise from it (default: 0)")


def degrade_noise_options(args):
    """-> None without the flags (``--degrade_seed`` alone is an error), else ``{"sigma": s}`` or ``{"snr": r}`` with ``"seed"``."""
    chosen = {k: getattr(args, flag) for k, flag in (("sigma", "degrade_noise"), ("snr", "degrade_snr")) if hasattr(args, flag)}
    if not chosen:
        if hasattr(args, "degrade_seed"):
            raise ValueError("--degrade_seed goes with --degrade_noise or --degrade_snr")
        return None
    return {**chosen, "seed": getattr(args, "degrade_seed", 0)}


def add_unring_flags(parser, flag, when):
    """``--unring`` of ``infer_volume.py`` / ``--unring_input`` of ``evaluate_volume.py`` with the sub-options (``volume_unring``); absent
    from the namespace unless given, so the parsed defaults are those of a build without them.  ``unring_options`` reads them back."""
    import argparse
    parser.add_argument(f"--{flag}", action="store_true", default=argparse.SUPPRESS,
                        help=f"(extension) take the Gibbs ringing of a truncated k-space out {when}: local subvoxel shifts along "
                             "--unring_axes, fused in one kernel per axis (default: off)")
    parser.add_argument("--unring_axes", type=int, nargs="+", choices=[0, 1, 2], default=argparse.SUPPRESS,
                        help=f"(extension) the axes of --{flag} (default: 0 1 2)")
    parser.add_argument("--unring_shifts", type=int, default=argparse.SUPPRESS,
                        help=f"(extension) K of --{flag}: 2K sub-voxel shifts are tried, 1..32 (default: 20)")
    parser.add_argument("--unring_window", type=int, nargs=2, default=argparse.SUPPRESS, metavar=("A", "B"),
                        help=f"(extension) the differences a..b either side of a voxel judge a shift of --{flag}, 1 <= a <= b <= 4 (default: 1 3)")


def unring_options(args, flag):
    """-> None without the flag (a sub-option alone is an error), else the keywords of ``unring_frame``."""
    given = [o for o in ("unring_axes", "unring_shifts", "unring_window") if hasattr(args, o)]
    if not getattr(args, flag, False):
        if given:
            raise ValueError(f"--{given[0]} goes with --{flag}")
        return None
    return dict(axes=tuple(getattr(args, "unring_axes", (0, 1, 2))), K=getattr(args, "unring_shifts", 20),
                window=tuple(getattr(args, "unring_window", (1, 3))))


def unring_frame(vol, options, log, what="") -> torch.Tensor:
    """One CUDA volume -> unringed float32 (``volume_unring.unring``); minimum, maximum and the total variation along each axis are
    logged before and after."""
    from mri_superresolution_amd.volume_unring import total_variation, unring
    vol = vol.float().contiguous()
    out = unring(vol, **options)
    for name, v in (("before", vol), ("after", out)):
        tv = ", ".join(f"{t:.6g}" for t in total_variation(v))
        log.info(f"{what}unring {name}: min {float(v.min()):.6g}, max {float(v.max()):.6g}, total variation per axis {tv}")
    log.info(f"{what}unringed along the axes {' '.join(str(a) for a in sorted(options['axes']))} (K = {options['K']}, window "
             f"{options['window'][0]}..{options['window'][1]})")
    return out


def start_logging():
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")


def require_gpu(args) -> torch.device:
    if args.cpu or not torch.cuda.is_available():
        raise RuntimeError("this build runs on MI355X only (hand-written HIP kernels, no CPU fallback)")
    return torch.device("cuda")


def log_device(device, log):
    log.info(f"Using device: {device} ({torch.cuda.get_device_name(0)})")


def run(body, args, log, doing) -> int:
    """The ``main`` of a volume script: ``body(args, device)`` on the GPU -> 0; any exception is logged as ``Error during {doing}`` -> 1."""
    start_logging()
    try:
        device = require_gpu(args)
        log_device(device, log)
        body(args, device)
        return 0
    except Exception as e:
        log.error(f"Error during {doing}: {e}")
        return 1


def to_device(frame, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float32)).to(device)


def join_frames(outs, ndim):
    """The per-frame arrays of a scan of ``ndim`` axes: the one volume, or the frames along axis 3."""
    return outs[0] if ndim == 3 else np.stack(outs, axis=3)


def make_parent(path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)


def save_nifti(path, array, header):
    make_parent(path)
    write_nifti(path, array, header)


def frame_tag(t, count) -> str:
    return "frame " + str(t) + ": " if count > 1 else ""


def load_mask(mask_path, ref, ref_affine=None):
    """-> one uint8 frame per timepoint of the reference (``utils.nifti.mask_frames``).  ``ref_affine`` (``--align``): the mask may
    lie on any grid and is resliced onto the reference's through the two affines with ``nearest``, on the device; the frames are
    then CUDA tensors."""
    count = 1 if ref.ndim == 3 else ref.shape[3]
    masks, header = mask_frames(mask_path, None if ref_affine is not None else ref.shape[:3], count, "--mask")
    if ref_affine is None:
        return masks
    m = grid_matrix(header.affine(), ref_affine)
    distinct = masks if len(header.shape) == 4 else masks[:1]      # a 3-D mask is resliced once
    out = [reslice_mask(torch.from_numpy(f).cuda(), m, ref.shape[:3]) for f in distinct]
    logger.info(f"Mask {mask_path} {tuple(masks[0].shape)} resliced onto the reference grid {tuple(ref.shape[:3])} (nearest).")
    return out if len(header.shape) == 4 else out * count
