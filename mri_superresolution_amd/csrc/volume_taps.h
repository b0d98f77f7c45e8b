// The interpolation taps of a resliced volume, shared by csrc/volume_reslice.hip (which documents the rules) and
// csrc/volume_register.hip: one definition of the clamp, the Keys weights, the taps and weights of an axis and the rounded tap sum,
// so that both files restate reslice_np with the same operations.  Include from files compiled with -ffp-contract=off.
#pragma once
#include "common.h"

#include <math.h>

constexpr int kNearest = MRISR_RESAMPLE_NEAREST, kLinear = MRISR_RESAMPLE_LINEAR, kCubic = MRISR_RESAMPLE_CUBIC;

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// Keys, A = -0.75, at distance x >= 0
__device__ __forceinline__ float keys_weight(float x) {
    const float wn = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(1.25f, x), 2.25f), x), x), 1.0f);
    const float wf = __fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(-0.75f, x), 3.75f), x), 6.0f), x), 3.0f);
    return x <= 1.0f ? wn : wf;
}

// taps and weights of one axis; p is inside [-0.5, n - 0.5]
template <int METHOD>
__device__ __forceinline__ void axis_taps(double p, int n, int* idx, float* w) {
    const double f = floor(p);
    const float t = (float)(p - f);      // the difference is exact in double
    const int fi = (int)f;               // -1 .. n - 1
    if constexpr (METHOD == kLinear) {
        idx[0] = clampi(fi, n);
        idx[1] = clampi(fi + 1, n);
        w[0] = __fsub_rn(1.0f, t);
        w[1] = t;
    } else {
#pragma unroll
        for (int d = 0; d < 4; ++d) idx[d] = clampi(fi - 1 + d, n);
        w[0] = keys_weight(__fadd_rn(1.0f, t));
        w[1] = keys_weight(t);
        w[2] = keys_weight(__fsub_rn(1.0f, t));
        w[3] = keys_weight(__fsub_rn(2.0f, t));
    }
}

template <int N>
__device__ __forceinline__ float weighted_sum(const float* w, const float* v) {
    float acc = __fmul_rn(w[0], v[0]);
#pragma unroll
    for (int d = 1; d < N; ++d) acc = __fadd_rn(acc, __fmul_rn(w[d], v[d]));
    return acc;
}

// the source coordinate of the voxel (di, dj, dk) along axis a of the row-major 3 x 4 matrix m: one rounded operation at a time
__device__ __forceinline__ double grid_coordinate(const double* m4, double di, double dj, double dk) {
    return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m4[0], di), __dmul_rn(m4[1], dj)), __dmul_rn(m4[2], dk)), m4[3]);
}
