// What the kernels of the deformable registration (csrc/volume_deform.hip, csrc/volume_lcc.hip) share beyond the bricks and the
// slots of volume_bricks.h, one definition each: the gradient rule of the force, the floor of its denominator and the tiles of the
// field's smoothing passes.
#pragma once
#include "volume_bricks.h"

constexpr int kMaxRadius = 16;
constexpr int kZRows = 4, kZTile = 256;                // z pass: a wave per row, 4 outputs per thread
constexpr int kSCols = 64, kSGroups = 4, kSPer = 8;    // y / x pass: 64 columns, 4 x 8 outputs along the filtered axis
#define MRISR_DEFORM_DEN_MIN 1e-9f

// gradient_np along one axis: i the index on it, n its extent, stride its distance in elements
__device__ __forceinline__ float axis_gradient(const float* __restrict__ f, size_t idx, int i, int n, size_t stride) {
    if (n == 1) return 0.f;
    if (i == 0) return __fsub_rn(f[idx + stride], f[idx]);
    if (i == n - 1) return __fsub_rn(f[idx], f[idx - stride]);
    return __fmul_rn(0.5f, __fsub_rn(f[idx + stride], f[idx - stride]));
}
