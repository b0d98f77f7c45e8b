// The sampler of a float32 volume at a float64 coordinate (csrc/volume_reslice.hip documents the rules), one definition each: the
// clamp, the Keys weights, the taps and weights of an axis, the rounded tap sum, the coordinate through a 3 x 4 matrix with its
// inside test (volume_register.hip, volume_stacks.h), the gather that reduces the taps along z, then y, then x (volume_deform.hip),
// and the host check that copies the 12 doubles of an entry into a kernel argument (every entry that takes a matrix).
// Include from files compiled with -ffp-contract=off.
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

// p = m q and the inside test of a volume of extents n
__device__ __forceinline__ bool matrix_coordinate(const double (*m)[4], double q0, double q1, double q2, int n0, int n1, int n2, double* p) {
    const int n[3] = {n0, n1, n2};
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = grid_coordinate(m[a], q0, q1, q2);
        inside = inside && p[a] >= -0.5 && p[a] <= (double)n[a] - 0.5;      // NaN compares false
    }
    return inside;
}

// the taps of the three axes reduced along z, then y, then x
template <int N>
__device__ __forceinline__ float gather_at(const float* __restrict__ src, int Y, int Z, const int* ix, const int* iy, const int* iz,
                                           const float* wx, const float* wy, const float* wz) {
    float rx[N];
#pragma unroll
    for (int a = 0; a < N; ++a) {
        float ry[N];
#pragma unroll
        for (int b = 0; b < N; ++b) {
            const float* row = src + ((size_t)ix[a] * Y + iy[b]) * Z;
            float v[N];
#pragma unroll
            for (int c = 0; c < N; ++c) v[c] = row[iz[c]];
            ry[b] = weighted_sum<N>(wz, v);
        }
        rx[a] = weighted_sum<N>(wy, ry);
    }
    return weighted_sum<N>(wx, rx);
}

template <int METHOD>
__device__ __forceinline__ float gather(const float* __restrict__ src, int X, int Y, int Z, const double* p) {
    constexpr int N = METHOD == kLinear ? 2 : 4;
    int ix[N], iy[N], iz[N];
    float wx[N], wy[N], wz[N];
    axis_taps<METHOD>(p[0], X, ix, wx);
    axis_taps<METHOD>(p[1], Y, iy, wy);
    axis_taps<METHOD>(p[2], Z, iz, wz);
    return gather_at<N>(src, Y, Z, ix, iy, iz, wx, wy, wz);
}

// a row-major 3 x 4 matrix by value in the kernel arguments
struct Matrix34 {
    double m[3][4];
};

// the 12 doubles of an entry into a kernel argument's m[3][4]; MRISR_E_ARG for an entry that is not finite
static inline int check_matrix34(const char* name, const double* m12, double (*m)[4]) {
    for (int e = 0; e < 12; ++e) {
        if (!isfinite(m12[e])) MRISR_FAIL(MRISR_E_ARG, "%s: matrix entry [%d][%d] is not finite", name, e / 4, e % 4);
        m[e / 4][e % 4] = m12[e];
    }
    return MRISR_OK;
}
