"""The argument checks of the volume tools after they moved into ``_volume_args``: every public entry point whose checks moved
still refuses a bad argument with ``ValueError`` and the message recorded here.  The messages were recorded by running the same
calls before the move; a row whose wording was unified carries the new wording and, in a comment, the old one.  Device wrappers
are called with CPU tensors and non-tensors: they refuse these before the library is loaded.  Their dtype and shape errors need
CUDA tensors and are in ``test_gpu_volume_args.py``.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import mri_superresolution_amd.volume_bias as B            # noqa: E402
import mri_superresolution_amd.volume_deform as D          # noqa: E402
import mri_superresolution_amd.volume_denoise as N         # noqa: E402
import mri_superresolution_amd.volume_eval as V            # noqa: E402
import mri_superresolution_amd.volume_intensity as I       # noqa: E402
import mri_superresolution_amd.volume_register as G        # noqa: E402
import mri_superresolution_amd.volume_reslice as R         # noqa: E402
import mri_superresolution_amd.volume_sharpness as E       # noqa: E402
import mri_superresolution_amd.volume_stacks as K          # noqa: E402
import mri_superresolution_amd.volume_surface as S         # noqa: E402
import mri_superresolution_amd.volume_tissue as T          # noqa: E402

F32 = np.zeros((5, 6, 7), dtype=np.float32)
F64 = np.zeros((5, 6, 7), dtype=np.float64)
EMPTY = np.zeros((0, 6, 7), dtype=np.float32)
FLAT = np.zeros((5, 6), dtype=np.float32)
HUGE = np.broadcast_to(np.float32(0), (2048, 2048, 1024))          # zero strides: 2^32 voxels, four bytes of memory
M8 = np.ones((5, 6, 7), dtype=np.uint8)
M8_WRONG = np.ones((5, 6, 8), dtype=np.uint8)
M32 = np.ones((5, 6, 7), dtype=np.int32)
U4 = np.zeros((3, 5, 6, 7), dtype=np.float32)
EYE = np.eye(4)[:3]
GEO = K.StackGeometry(EYE, EYE, 2, np.zeros(1), np.ones(1, dtype=np.float32))
T32 = torch.zeros((5, 6, 7), dtype=torch.float32)
T8 = torch.ones((5, 6, 7), dtype=torch.uint8)
T4 = torch.zeros((3, 5, 6, 7), dtype=torch.float32)

# (the call, the exact message).  A call is a string so that a failing row names itself; it is evaluated in this module.
CASES = [
    # numpy specifications: float64 instead of float32
    # was: reslice_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('R.reslice_np(F64, EYE, (5, 6, 7))',
     'reslice_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    ('I.landmarks_np(F64)',
     'landmarks_np: expected a non-empty float32 array, got float64 (5, 6, 7)'),
    ('I.piecewise_map_np(F64, F32[0, 0, :3], F32[0, 0, :3])',
     'piecewise_map_np: expected a non-empty float32 array, got float64 (5, 6, 7)'),
    ('I.match_intensity_np(F64, F32)',
     'match_intensity_np: expected a non-empty float32 array, got float64 (5, 6, 7)'),
    # was: smooth_masked_np: expected a non-empty float32 array, got float64 (5, 6, 7)
    ('B.smooth_masked_np(F64, M8, (1, 1, 1))',
     'smooth_masked_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: match_bias_np: the mask must be a uint8 or bool array of shape (5, 6, 7), got float64 (5, 6, 7)
    ('B.match_bias_np(F32, M8, F64, M8, (1, 1, 1))',
     'match_bias_np: the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got float64 (5, 6, 7)'),
    # was: correct_bias_np: expected a non-empty float32 array, got float64 (5, 6, 7)
    ('B.correct_bias_np(F64, M8, (1, 1, 1))',
     'correct_bias_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: denoise_np: expected a non-empty float32 array, got float64 (5, 6, 7)
    ('N.denoise_np(F64, 1.0, 1.0)',
     'denoise_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: estimate_sigma_np: expected a non-empty float32 array, got float64 (5, 6, 7)
    ('N.estimate_sigma_np(F64, M8)',
     'estimate_sigma_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: background_mask_np: expected a non-empty float32 array, got float64 (5, 6, 7)
    ('N.background_mask_np(F64)',
     'background_mask_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: warp_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('D.warp_np(F64, U4)',
     'warp_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: gradient_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('D.gradient_np(F64)',
     'gradient_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: demons_force_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('D.demons_force_np(F64, F32, U4)',
     'demons_force_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: warp_matrix_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('D.warp_matrix_np(F64, EYE, U4)',
     'warp_matrix_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: register_deformable_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('D.register_deformable_np(F32, F64)',
     'register_deformable_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: simulate_stack_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('K.simulate_stack_np(F64, GEO, (5, 6, 7))',
     'simulate_stack_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: stack_residual_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('K.stack_residual_np(F32, F64, GEO)',
     'stack_residual_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: stack_update_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('K.stack_update_np(F64, [F32], [GEO])',
     'stack_update_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: combine_stacks_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('K.combine_stacks_np([F64], [GEO], (5, 6, 7))',
     'combine_stacks_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    ('T.segment_tissue_np(F64, M8)',
     'segment_tissue_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    ('E.edge_profile_np(F64, U4[:2])',
     'edge_profile_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: downsample2_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('V.downsample2_np(F64)',
     'downsample2_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: upscale2_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('V.upscale2_np(F64, "linear")',
     'upscale2_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # empty
    # was: reslice_np: expected a non-empty float32 volume (X,Y,Z), got float32 (0, 6, 7)
    ('R.reslice_np(EMPTY, EYE, (5, 6, 7))',
     'reslice_np: expected a non-empty float32 volume (X, Y, Z), got float32 (0, 6, 7)'),
    ('I.landmarks_np(EMPTY)',
     'landmarks_np: expected a non-empty float32 array, got float32 (0, 6, 7)'),
    # was: smooth_masked_np: expected a non-empty float32 array, got float32 (0, 6, 7)
    ('B.smooth_masked_np(EMPTY, M8, (1, 1, 1))',
     'smooth_masked_np: expected a non-empty float32 volume (X, Y, Z), got float32 (0, 6, 7)'),
    # was: denoise_np: expected a non-empty float32 array, got float32 (0, 6, 7)
    ('N.denoise_np(EMPTY, 1.0, 1.0)',
     'denoise_np: expected a non-empty float32 volume (X, Y, Z), got float32 (0, 6, 7)'),
    # was: gradient_np: expected a non-empty float32 volume (X,Y,Z), got float32 (0, 6, 7)
    ('D.gradient_np(EMPTY)',
     'gradient_np: expected a non-empty float32 volume (X, Y, Z), got float32 (0, 6, 7)'),
    # was: stack_residual_np: expected a non-empty float32 volume (X,Y,Z), got float32 (0, 6, 7)
    ('K.stack_residual_np(EMPTY, F32, GEO)',
     'stack_residual_np: expected a non-empty float32 volume (X, Y, Z), got float32 (0, 6, 7)'),
    ('T.segment_tissue_np(EMPTY, M8)',
     'segment_tissue_np: expected a non-empty float32 volume (X, Y, Z), got float32 (0, 6, 7)'),
    # was: downsample2_np: expected a non-empty float32 volume (X,Y,Z), got float32 (0, 6, 7)
    ('V.downsample2_np(EMPTY)',
     'downsample2_np: expected a non-empty float32 volume (X, Y, Z), got float32 (0, 6, 7)'),
    # was: the labels must be a non-empty uint8 array, got uint8 (0, 6, 7)
    ('S.boundary_np(M8[:0])',
     'the labels must be a non-empty uint8 or bool volume (X, Y, Z), got uint8 (0, 6, 7)'),
    # was: a must be a non-empty uint8 array, got uint8 (0, 6, 7)
    ('T.confusion_np(M8[:0], M8[:0])',
     'a must be a non-empty uint8 or bool array, got uint8 (0, 6, 7)'),
    # 2-D where 3-D is required
    # was: reslice_np: expected a non-empty float32 volume (X,Y,Z), got float32 (5, 6)
    ('R.reslice_np(FLAT, EYE, (5, 6, 7))',
     'reslice_np: expected a non-empty float32 volume (X, Y, Z), got float32 (5, 6)'),
    # was: smooth_masked_np: a volume has three axes, got shape (5, 6)
    ('B.smooth_masked_np(FLAT, M8[0], (1, 1, 1))',
     'smooth_masked_np: expected a non-empty float32 volume (X, Y, Z), got float32 (5, 6)'),
    # was: denoise_np: a volume has three axes, got shape (5, 6)
    ('N.denoise_np(FLAT, 1.0, 1.0)',
     'denoise_np: expected a non-empty float32 volume (X, Y, Z), got float32 (5, 6)'),
    # was: patch_distance_np: a volume has three axes, got shape (5, 6)
    ('N.patch_distance_np(FLAT, (1, 0, 0))',
     'patch_distance_np: expected a non-empty float32 volume (X, Y, Z), got float32 (5, 6)'),
    # was: gradient_np: expected a non-empty float32 volume (X,Y,Z), got float32 (5, 6)
    ('D.gradient_np(FLAT)',
     'gradient_np: expected a non-empty float32 volume (X, Y, Z), got float32 (5, 6)'),
    # was: stack_residual_np: expected a non-empty float32 volume (X,Y,Z), got float32 (5, 6)
    ('K.stack_residual_np(FLAT, F32, GEO)',
     'stack_residual_np: expected a non-empty float32 volume (X, Y, Z), got float32 (5, 6)'),
    ('T.segment_tissue_np(FLAT, M8[0])',
     'segment_tissue_np: expected a non-empty float32 volume (X, Y, Z), got float32 (5, 6)'),
    ('E.edge_profile_np(FLAT, U4[:2])',
     'edge_profile_np: expected a non-empty float32 volume (X, Y, Z), got float32 (5, 6)'),
    # was: upscale2_np: expected a non-empty float32 volume (X,Y,Z), got float32 (5, 6)
    ('V.upscale2_np(FLAT, "linear")',
     'upscale2_np: expected a non-empty float32 volume (X, Y, Z), got float32 (5, 6)'),
    # was: the labels must be a volume (X, Y, Z), got (6, 7)
    ('S.boundary_np(M8[0])',
     'the labels must be a non-empty uint8 or bool volume (X, Y, Z), got uint8 (6, 7)'),
    # was: the sites must be a volume (X, Y, Z), got (6, 7)
    ('S.edt_sq_np(M8[0], 1)',
     'the sites must be a non-empty uint8 or bool volume (X, Y, Z), got uint8 (6, 7)'),
    # was: a must be a volume (X, Y, Z), got (6, 7)
    ('S.surface_distances_np(M8[0], M8[0])',
     'a must be a non-empty uint8 or bool volume (X, Y, Z), got uint8 (6, 7)'),
    # was: the labels must be a volume (X, Y, Z), got (6, 7)
    ('E.interface_sides_np(M8[0], 1)',
     'the labels must be a non-empty uint8 or bool volume (X, Y, Z), got uint8 (6, 7)'),
    # an axis above the extent limit, where it applies
    ('D.gradient_np(HUGE)',
     "gradient_np: the volume's shape (2048, 2048, 1024) has more than 2^31 - 1 voxels"),
    ('D.warp_matrix_np(HUGE, EYE, U4)',
     "warp_matrix_np: the volume's shape (2048, 2048, 1024) has more than 2^31 - 1 voxels"),
    ('K.stack_residual_np(F32, HUGE, GEO)',
     "stack_residual_np: the volume's shape (2048, 2048, 1024) has more than 2^31 - 1 voxels"),
    ('K.simulate_stack_np(HUGE, GEO, (5, 6, 7))',
     "simulate_stack_np: the volume's shape (2048, 2048, 1024) has more than 2^31 - 1 voxels"),
    # a mask of the wrong shape
    # was: landmarks_np: the mask must be a uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)
    ('I.landmarks_np(F32, M8_WRONG)',
     'landmarks_np: the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)'),
    # was: landmarks_np: the mask must be a uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)
    ('I.match_intensity_np(F32, F32, M8_WRONG)',
     'landmarks_np: the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)'),
    # was: smooth_masked_np: the mask must be a uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)
    ('B.smooth_masked_np(F32, M8_WRONG, (1, 1, 1))',
     'smooth_masked_np: the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)'),
    # was: correct_bias_np: the mask must be a uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)
    ('B.correct_bias_np(F32, M8_WRONG, (1, 1, 1))',
     'correct_bias_np: the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)'),
    # was: estimate_sigma_np: the mask must be a uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)
    ('N.estimate_sigma_np(F32, M8_WRONG)',
     'estimate_sigma_np: the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)'),
    # was: fixed_mask must be a uint8 or bool volume of shape (5, 6, 7), got uint8 (5, 6, 8)
    ('G.joint_histogram_np(F32, F32, EYE, 32, 1, (0.0, 1.0), (0.0, 1.0), M8_WRONG)',
     'fixed_mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)'),
    # was: the mask must be a non-empty uint8 array of shape (5, 6, 7), got uint8 (5, 6, 8)
    ('T.segment_tissue_np(F32, M8_WRONG)',
     'the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)'),
    # was: b must be a non-empty uint8 array of shape (5, 6, 7), got uint8 (5, 6, 8)
    ('T.confusion_np(M8, M8_WRONG)',
     'b must be a non-empty uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)'),
    # was: the mask must be a non-empty uint8 array of shape (5, 6, 7), got uint8 (5, 6, 8)
    ('T.confusion_np(M8, M8, M8_WRONG)',
     'the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)'),
    # was: b must be a non-empty uint8 array of shape (5, 6, 7), got uint8 (5, 6, 8)
    ('S.surface_distances_np(M8, M8_WRONG)',
     'b must be a non-empty uint8 or bool volume (X, Y, Z) of shape (5, 6, 7), got uint8 (5, 6, 8)'),
    # a mask of dtype int32
    # was: landmarks_np: the mask must be a uint8 or bool array of shape (5, 6, 7), got int32 (5, 6, 7)
    ('I.landmarks_np(F32, M32)',
     'landmarks_np: the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got int32 (5, 6, 7)'),
    # was: smooth_masked_np: the mask must be a uint8 or bool array of shape (5, 6, 7), got int32 (5, 6, 7)
    ('B.smooth_masked_np(F32, M32, (1, 1, 1))',
     'smooth_masked_np: the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got int32 (5, 6, 7)'),
    # was: estimate_sigma_np: the mask must be a uint8 or bool array of shape (5, 6, 7), got int32 (5, 6, 7)
    ('N.estimate_sigma_np(F32, M32)',
     'estimate_sigma_np: the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got int32 (5, 6, 7)'),
    # was: fixed_mask must be a uint8 or bool volume of shape (5, 6, 7), got int32 (5, 6, 7)
    ('G.joint_histogram_np(F32, F32, EYE, 32, 1, (0.0, 1.0), (0.0, 1.0), M32)',
     'fixed_mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got int32 (5, 6, 7)'),
    # was: the mask must be a non-empty uint8 array of shape (5, 6, 7), got int32 (5, 6, 7)
    ('T.segment_tissue_np(F32, M32)',
     'the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got int32 (5, 6, 7)'),
    # was: a must be a non-empty uint8 array, got int32 (5, 6, 7)
    ('T.confusion_np(M32, M32)',
     'a must be a non-empty uint8 or bool array, got int32 (5, 6, 7)'),
    # was: the labels must be a non-empty uint8 array, got int32 (5, 6, 7)
    ('S.boundary_np(M32)',
     'the labels must be a non-empty uint8 or bool volume (X, Y, Z), got int32 (5, 6, 7)'),
    # was: the labels must be a non-empty uint8 array, got int32 (5, 6, 7)
    ('E.interface_sides_np(M32, 1)',
     'the labels must be a non-empty uint8 or bool volume (X, Y, Z), got int32 (5, 6, 7)'),
    # two sigmas instead of three
    ('B.smooth_masked_np(F32, M8, (1, 1))',
     'three sigmas in voxels are expected, got (1, 1)'),
    ('B.correct_bias_np(F32, M8, (1, 1))',
     'three sigmas in voxels are expected, got (1, 1)'),
    ('D.smooth_field_np(U4, (1, 1))',
     'three sigmas in voxels are expected, got (1, 1)'),
    ('B.smooth_masked_np(F32, M8, None)',
     'three sigmas in voxels are expected, got None'),
    ('D.smooth_field_np(U4, (1, 1, 40))',
     'sigma 40 voxels needs a radius of 120 taps, at most 16 are built for a field'),
    # device wrappers: a CPU tensor
    ('R.reslice(T32, EYE, (5, 6, 7))',
     'reslice runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    ('R.reslice_mask(T8, EYE, (5, 6, 7))',
     'reslice_mask runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: masked_percentiles runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('I.masked_percentiles(T32)',
     'masked_percentiles runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: piecewise_map runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('I.piecewise_map(T32, T32[0, 0, :3], T32[0, 0, :3])',
     'piecewise_map runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: match_intensity runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('I.match_intensity(T32, T32)',
     'match_intensity runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: smooth_masked runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('B.smooth_masked(T32, T8, (1, 1, 1))',
     'smooth_masked runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: match_bias runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('B.match_bias(T32, T8, T32, T8, (1, 1, 1))',
     'match_bias runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: correct_bias runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('B.correct_bias(T32, T8, (1, 1, 1))',
     'correct_bias runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: denoise runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('N.denoise(T32, T32[0, 0, :4])',
     'denoise runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: estimate_noise runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('N.estimate_noise(T32, T8)',
     'estimate_noise runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: background_mask runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('N.background_mask(T32)',
     'background_mask runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: denoise_volume runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('N.denoise_volume(T32)',
     'denoise_volume runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: warp runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.warp(T32, T4)',
     'warp runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: demons_force runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.demons_force(T32, T32, T4)',
     'demons_force runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: smooth_field runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.smooth_field(T4, (1, 1, 1))',
     'smooth_field runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: jacobian_stats runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.jacobian_stats(T4)',
     'jacobian_stats runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: compose runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.compose(T4, T4)',
     'compose runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: demons_update runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.demons_update(T32, T32, T4)',
     'demons_update runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: lcc_force runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.lcc_force(T32, T32, T4)',
     'lcc_force runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: exp_field runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.exp_field(T4, 2)',
     'exp_field runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: warp_matrix runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.warp_matrix(T32, EYE, T4)',
     'warp_matrix runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: register_deformable runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.register_deformable(T32, T32)',
     'register_deformable runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: register_diffeomorphic runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.register_diffeomorphic(T32, T32)',
     'register_diffeomorphic runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    ('K.stack_residual(T32, T32, GEO)',
     'stack_residual runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    ('K.stack_update(T32, [T32], [GEO])',
     'stack_update runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    ('K.combine_stacks([T32], [GEO], (5, 6, 7))',
     'combine_stacks: stack 0 runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    ('G.joint_histogram(T32, T32, EYE, 32, 1, (0.0, 1.0), (0.0, 1.0))',
     'joint_histogram runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: mask_moments runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor
    ('G.mask_moments(T8)',
     'mask_moments runs on an MI355X through libmrisr.so only (no CPU fallback): the mask must be a CUDA tensor, got a CPU tensor'),
    ('G.nmi(torch.zeros((32, 32), dtype=torch.int64))',
     'nmi runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor'),
    ('G.register_rigid(T32, np.eye(4), T32, np.eye(4))',
     'register_rigid runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: segment_tissue runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('T.segment_tissue(T32, T8)',
     'segment_tissue runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: label_confusion runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('T.label_confusion(T8, T8)',
     'label_confusion runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    ('T.TissueWorkspace((5, 6, 7), 3, "cpu")',
     'TissueWorkspace runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA device'),
    # was: label_boundary runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('S.label_boundary(T8)',
     'label_boundary runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: distance_transform_sq runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('S.distance_transform_sq(T8, 1)',
     'distance_transform_sq runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: surface_distances runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('S.surface_distances(T8, T8)',
     'surface_distances runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    ('S.SurfaceWorkspace((5, 6, 7), 3, "cpu")',
     'SurfaceWorkspace runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA device'),
    # was: interface_sides runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('E.interface_sides(T8, 1)',
     'interface_sides runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: signed_distance runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('E.signed_distance(T8, 1)',
     'signed_distance runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: signed_distances runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('E.signed_distances(T8)',
     'signed_distances runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    ('E.edge_profile(T32, T4[:2])',
     'edge_profile runs on an MI355X through libmrisr.so only (no CPU fallback): expected CUDA tensors'),
    ('E.EdgeWorkspace(2, 16, "cpu")',
     'EdgeWorkspace runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA device'),
    # device wrappers: a non-tensor
    ('R.reslice(F32, EYE, (5, 6, 7))',
     'reslice runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got ndarray'),
    # was: masked_percentiles runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('I.masked_percentiles(F32)',
     'masked_percentiles runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got ndarray'),
    # was: smooth_masked runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('B.smooth_masked(F32, M8, (1, 1, 1))',
     'smooth_masked runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got ndarray'),
    # was: denoise runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('N.denoise(F32, None)',
     'denoise runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got ndarray'),
    # was: warp runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.warp(F32, U4)',
     'warp runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got ndarray'),
    ('K.stack_residual(F32, F32, GEO)',
     'stack_residual runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got ndarray'),
    ('K.combine_stacks([F32], [GEO], (5, 6, 7))',
     'combine_stacks: stack 0 runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got ndarray'),
    ('G.joint_histogram(F32, F32, EYE, 32, 1, (0.0, 1.0), (0.0, 1.0))',
     'joint_histogram runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got ndarray'),
    # was: segment_tissue runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('T.segment_tissue(F32, M8)',
     'segment_tissue runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got ndarray'),
    # was: label_confusion runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('T.label_confusion(M8, M8)',
     'label_confusion runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got ndarray'),
    # was: label_boundary runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('S.label_boundary(M8)',
     'label_boundary runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got ndarray'),
    # was: interface_sides runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('E.interface_sides(M8, 1)',
     'interface_sides runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got ndarray'),
    # precedence: one argument that trips two conditions raises what the parent raised first
    # was: reslice_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6)
    ('R.reslice_np(np.zeros((5, 6), dtype=np.float64), EYE, (0, 6, 7))',
     'reslice_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6)'),
    ('R.reslice(torch.zeros((5, 6), dtype=torch.float64), EYE, (5, 6, 7))',
     'reslice runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    ('I.landmarks_np(F64, M8_WRONG)',
     'landmarks_np: expected a non-empty float32 array, got float64 (5, 6, 7)'),
    # was: landmarks_np: the mask must be a uint8 or bool array of shape (5, 6, 7), got int32 (5, 6, 3)
    ('I.landmarks_np(F32, M32[:, :, :3])',
     'landmarks_np: the mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got int32 (5, 6, 3)'),
    # was: smooth_masked_np: expected a non-empty float32 array, got float64 (5, 6)
    ('B.smooth_masked_np(np.zeros((5, 6), dtype=np.float64), M8, (1, 1))',
     'smooth_masked_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6)'),
    # was: denoise_np: expected a non-empty float32 array, got float64 (5, 6)
    ('N.denoise_np(np.zeros((5, 6), dtype=np.float64), 1.0, 1.0, radius=99)',
     'denoise_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6)'),
    # was: gradient_np: expected a non-empty float32 volume (X,Y,Z), got float64 (2048, 2048, 1024)
    ('D.gradient_np(np.broadcast_to(np.float64(0), (2048, 2048, 1024)))',
     'gradient_np: expected a non-empty float32 volume (X, Y, Z), got float64 (2048, 2048, 1024)'),
    # was: stack_residual_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('K.stack_residual_np(F64, HUGE, GEO)',
     'stack_residual_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: a must be a non-empty uint8 array, got int32 (5, 6, 7)
    ('T.confusion_np(M32, M8_WRONG)',
     'a must be a non-empty uint8 or bool array, got int32 (5, 6, 7)'),
    ('S.surface_distances_np(M32[0], M8, classes=99)',
     'classes must be an integer in 2..6, got 99'),
    ('D.smooth_field_np(U4, (1, "x"))',
     "three sigmas in voxels are expected, got (1, 'x')"),
    # was: warp runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('D.warp(torch.zeros((5, 6), dtype=torch.float64), T4)',
     'warp runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # was: label_confusion runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor
    ('T.label_confusion(torch.ones((5, 6, 7), dtype=torch.int32), T8)',
     'label_confusion runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    ('K.stack_update(torch.zeros((5, 6), dtype=torch.float64), [T32], [GEO])',
     'stack_update runs on an MI355X through libmrisr.so only (no CPU fallback): expected a CUDA tensor, got a CPU tensor'),
    # entry points that reach a moved check through another entry
    # was: otsu_bins_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('V.otsu_bins_np(F64)',
     'otsu_bins_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    ('D.compose_np(np.broadcast_to(np.float32(0), (3, 2048, 2048, 1024)), U4)',
     "compose_np: the volume's shape (2048, 2048, 1024) has more than 2^31 - 1 voxels"),
    # was: demons_update_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('D.demons_update_np(F64, F32, U4)',
     'demons_update_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: lcc_force_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('D.lcc_force_np(F64, F32, U4)',
     'lcc_force_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: lcc_update_np: expected a non-empty float32 volume (X,Y,Z), got float32 (5, 6)
    ('D.lcc_update_np(F32, FLAT, U4)',
     'lcc_update_np: expected a non-empty float32 volume (X, Y, Z), got float32 (5, 6)'),
    # was: register_diffeomorphic_np: expected a non-empty float32 volume (X,Y,Z), got float64 (5, 6, 7)
    ('D.register_diffeomorphic_np(F64, F32)',
     'register_diffeomorphic_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    ('D.pyramid_shapes((0, 6, 7), 2)',
     'shape must be three positive extents, got (0, 6, 7)'),
    # was: the labels must be a volume (X, Y, Z), got (6, 7)
    ('E.signed_distance_np(M8[0], 1)',
     'the labels must be a non-empty uint8 or bool volume (X, Y, Z), got uint8 (6, 7)'),
    ('E.signed_distance_np(M8, 1, (1, 1))',
     'spacing is three finite positive voxel sizes, got (1, 1)'),
    ('E.edge_sharpness_np(F64, M8)',
     'edge_profile_np: expected a non-empty float32 volume (X, Y, Z), got float64 (5, 6, 7)'),
    # was: the labels must be a non-empty uint8 array, got int32 (5, 6, 7)
    ('E.edge_sharpness_np(F32, M32)',
     'the labels must be a non-empty uint8 or bool volume (X, Y, Z), got int32 (5, 6, 7)'),
    # was: fixed_mask must be a uint8 or bool volume of shape (5, 6, 7), got uint8 (5, 6, 8)
    ('G.register_rigid_np(F32, np.eye(4), F32, np.eye(4), fixed_mask=M8_WRONG)',
     'fixed_mask must be a non-empty uint8 or bool array of shape (5, 6, 7), got uint8 (5, 6, 8)'),
    ('G.register_rigid_np(F32, np.eye(4), F32, np.eye(4), mask_cost=True, moving_mask=M32)',
     'fixed_range must be finite in float32 with hi > lo (and a finite bins / (hi - lo)), got (0.0, 0.0)'),
    ('G.register_rigid_np(F32, np.eye(3), F32, np.eye(4))',
     'fixed_affine must be a 4 x 4 index -> world affine, got shape (3, 3)'),
    ('T.kmeans_hist_np(np.ones(256, dtype=np.int64), 99)',
     'classes must be an integer in 2..6, got 99'),
    ('K.default_output_grid([np.eye(3)], [(5, 6, 7)])',
     'affine must be a 4 x 4 index -> world affine, got shape (3, 3)'),
    ('K.StackWorkspace((0, 6, 7), [(5, 6, 7)], "cuda")',
     'shape_out must be three positive extents, got (0, 6, 7)'),
    ('K.stack_geometry(np.eye(4), np.eye(3))',
     'affine_out must be a 4 x 4 index -> world affine, got shape (3, 3)'),
]


@pytest.mark.parametrize("call,message", CASES, ids=[c for c, _ in CASES])
def test_refusal_message(call, message):
    with pytest.raises(ValueError) as info:
        eval(call)
    assert str(info.value) == message


def test_denoise_np_takes_a_view():
    """``denoise_np`` accepts a float32 view that is not contiguous and returns what it returned before the checks moved."""
    rng = np.random.default_rng(5)
    big = (rng.random((9, 12, 14)) * 100).astype(np.float32)
    view = big[:, ::2, ::2].transpose(2, 0, 1)
    assert not view.flags.c_contiguous
    inv_h2, two_sigma2 = N.noise_params_np(5.0)[:2]
    out = N.denoise_np(view, inv_h2, two_sigma2, radius=1)
    assert out.shape == (7, 9, 6) and out.dtype == np.float32
    assert np.array_equal(out, N.denoise_np(np.ascontiguousarray(view), inv_h2, two_sigma2, radius=1), equal_nan=True)
    assert hashlib.sha256(out.tobytes()).hexdigest() == "92c29e039e618f2a80808f8c1db9802b2401d3e113dc75d9c43924625202444d"


def test_masks_come_back_as_uint8_views():
    from mri_superresolution_amd import _volume_args as A
    m = np.ones((5, 6, 7), dtype=bool)
    got = A.mask_np(m, m.shape, "here")
    assert got.dtype == np.uint8 and np.shares_memory(got, m)


def test_volume_args_imports_no_volume_tool():
    code = ("import sys, mri_superresolution_amd._volume_args; "
            "print([m for m in sys.modules if m.startswith('mri_superresolution_amd.volume')])")
    done = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert done.stdout.strip() == "[]"
