"""Builds libmrisr.so (hand-written HIP kernels, gfx950 only) in-tree with hipcc.

    python -m mri_superresolution_amd.build            # incremental
    python -m mri_superresolution_amd.build --force

hipcc cross-compiles for gfx950 without a GPU.  The .so lands next to this file so that it
travels with the repo snapshot to the GPU box; objects go to build/ (git-ignored).
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(os.path.dirname(HERE), "build", "mrisr")
LIB = os.path.join(HERE, "libmrisr.so")
SOURCES = ["api.cpp", "conv_fwd.hip", "conv_igemm_bf16.hip", "conv_igemm_f16.hip", "conv_igemm_f32.hip", "conv_pack.hip", "conv_ring.hip", "conv_pc.hip", "conv1x1.hip", "conv_wgrad.hip", "conv_wgrad_rows.hip", "conv_upadj.hip", "norm.hip", "norm_bwd.hip", "norm_bwd_onepass.hip", "norm_bwd_shuffle.hip", "head_stem.hip", "loss.hip", "optim.hip", "vgg.hip", "image.hip", "evalops.hip", "lowfield.hip", "percentile.hip", "resample.hip", "volume_blend.hip", "volume_eval.hip", "volume_label.hip", "volume_mask.hip", "volume_metrics.hip", "volume_reslice.hip", "volume_register.hip", "volume_intensity.hip", "volume_bias.hip", "volume_denoise.hip", "volume_deform.hip", "volume_lcc.hip", "volume_tissue.hip", "volume_surface.hip", "volume_edge.hip", "volume_stacks.hip", "volume_slices.hip", "volume_kspace.hip", "volume_unring.hip", "volume_noise.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]
# conv_igemm_*.hip (the classic forward kernel) and conv_pack.hip (the packers, once in one file with it): no SLP
# vectorisation - it turns the epilogue's statistics into v_pk_*_f32 ops plus register shuffles, and
# packed fp32 ops issue at half speed next to the other wave's MFMA block (measured with the phase profile)
# image.hip: no fma contraction - it restates numpy / PIL float32 arithmetic operation by operation (HIP's __fmul_rn /
# __fadd_rn are plain operators, and under the default -ffp-contract=fast  a + alpha * (b - a)  becomes one fma: PIL's
# (UINT8) truncation then lands one grey level lower whenever the product is an integer minus 2^-22)
# evalops.hip: likewise a step-by-step restatement of host arithmetic (integer passes, one float32 division)
# lowfield.hip: likewise (the renormalisation pass; the FMAs of its convolution pass are written as fmaf())
# percentile.hip: likewise (numpy's float32 interpolation, window and restore: a rounded product, then a rounded sum)
# resample.hip: likewise (the uint8 epilogue; the tap sums are written as fmaf())
# volume_blend.hip: likewise (the through-plane interpolation and the mean of the planes: product, product, sum, division)
# volume_eval.hip: likewise (pair sums and interpolation taps of the volume baselines: every product and sum rounded on its own)
# volume_mask.hip: likewise (the histogram bin of a voxel in float32, Otsu's between-class variance in double)
# volume_reslice.hip: likewise (the source coordinate in double, the weights and the tap sums in float32)
# volume_register.hip: likewise (the same coordinate and taps through volume_taps.h, the bin of a value in float32)
# volume_intensity.hip: likewise (the virtual index and numpy's interpolation of a landmark; the map's difference, product, sum)
# volume_bias.hip: likewise (every tap of the masked Gaussian is a rounded product, then a rounded sum, in ascending order; the field's divisions)
# volume_denoise.hip: likewise (the squared differences of a patch and their nested sums, the weighted mean of the candidates in order)
# volume_deform.hip: likewise (the coordinate under the field in double, the taps through volume_taps.h, the force's products, sums and division, the taps of the field's Gaussian in ascending order; the float64 sum and its rounding error)
# volume_lcc.hip: likewise (the float64 channels, their nested window sums in ascending order, the regression's products, differences and divisions, then the force's float32 rule)
# volume_tissue.hip: likewise (the quantiser's difference and product: the bin of a voxel in float32; everything else there is integer)
# volume_surface.hip: likewise (a candidate of the distance transform: the weight times d * d, a rounded product, then a rounded sum with the line's value)
# volume_edge.hip: likewise (the bin of a voxel: a rounded float32 sum of the signed distance and the radius, then a rounded quotient by the bin width)
# volume_slices.hip: likewise (the same forward model and taps per slice, the through-plane distance and weight in double, the quotient by the slices' weight sum)
# volume_kspace.hip: likewise (a line's circulant sum: every product of a table entry and a sample rounded, then every sum, over the source index ascending)
# volume_unring.hip: likewise (the same circulant sum per sub-voxel shift, the differences and their windowed sums, the interpolation back: a difference, a product, a sum)
# volume_noise.hip: likewise (the table's interpolation - a rounded product, then a rounded sum - sigma times the normal, the sum with the voxel, the two squares, their sum and the square root)
# volume_stacks.hip: likewise (the sample's coordinate in double, the taps through volume_taps.h, the profile's products and sums, the quotient by the weight sum, the mean of the stacks and the step)
FILE_FLAGS = {**{f: ["-fno-slp-vectorize"] for f in ("conv_igemm_bf16.hip", "conv_igemm_f16.hip", "conv_igemm_f32.hip", "conv_pack.hip")},
              "image.hip": ["-ffp-contract=off"], "evalops.hip": ["-ffp-contract=off"],
              "lowfield.hip": ["-ffp-contract=off"], "percentile.hip": ["-ffp-contract=off"], "resample.hip": ["-ffp-contract=off"],
              "volume_blend.hip": ["-ffp-contract=off"], "volume_eval.hip": ["-ffp-contract=off"],
              "volume_mask.hip": ["-ffp-contract=off"], "volume_reslice.hip": ["-ffp-contract=off"],
              "volume_register.hip": ["-ffp-contract=off"], "volume_intensity.hip": ["-ffp-contract=off"],
              "volume_bias.hip": ["-ffp-contract=off"], "volume_denoise.hip": ["-ffp-contract=off"],
              "volume_deform.hip": ["-ffp-contract=off"], "volume_lcc.hip": ["-ffp-contract=off"],
              "volume_tissue.hip": ["-ffp-contract=off"],
              "volume_surface.hip": ["-ffp-contract=off"], "volume_edge.hip": ["-ffp-contract=off"],
              "volume_stacks.hip": ["-ffp-contract=off"], "volume_slices.hip": ["-ffp-contract=off"],
              "volume_kspace.hip": ["-ffp-contract=off"], "volume_unring.hip": ["-ffp-contract=off"],
              "volume_noise.hip": ["-ffp-contract=off"]}


def _deps_mtime():
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    hdrs.append(os.path.join(os.path.dirname(HERE), "include", "mrisr.h"))
    return max(os.path.getmtime(h) for h in hdrs)


def _compile(src, force):
    obj = os.path.join(OBJ, os.path.splitext(src)[0] + ".o")
    path = os.path.join(CSRC, src)
    if not force and os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(path), _deps_mtime()):
        return obj, False
    cmd = [HIPCC, *FLAGS, *FILE_FLAGS.get(src, []), "-c", path, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
    return obj, True


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJ, exist_ok=True)
    with ThreadPoolExecutor(max_workers=8) as ex:
        results = list(ex.map(lambda s: _compile(s, force), SOURCES))
    objs = [o for o, _ in results]
    if force or any(c for _, c in results) or not os.path.exists(LIB):
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
        if verbose:
            print(f"[mrisr] built {LIB}")
    elif verbose:
        print(f"[mrisr] {LIB} up to date")
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
