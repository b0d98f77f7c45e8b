// What the kernels of the stack reconstruction (csrc/volume_stacks.hip, csrc/volume_slices.hip) share, one definition each: the
// slice profile as it travels in the kernel arguments, the voxel of a thread in a brick, the coordinate with its inside test, the
// linear gather and the host check of a matrix.  Include from files compiled with -ffp-contract=off.
#pragma once
#include "volume_deform.h"
#include "volume_taps.h"

constexpr int kMaxStacks = MRISR_STACKS_MAX, kMaxSamples = MRISR_STACK_SAMPLES_MAX;

struct StackProfile {
    double offset[kMaxSamples];
    float weight[kMaxSamples];
};

// voxel of thread tid in brick b (bricks numbered along z, then y, then x)
__device__ __forceinline__ bool stack_brick_voxel(unsigned b, unsigned nby, unsigned nbz, int X, int Y, int Z, int& i, int& j, int& k) {
    const unsigned bz = b % nbz, rest = b / nbz, by = rest % nby, bx = rest / nby;
    const int tid = threadIdx.x;
    k = (int)bz * kBZ + tid % kBZ, j = (int)by * kBY + tid / kBZ % kBY, i = (int)bx * kBX + tid / (kBZ * kBY);
    return i < X && j < Y && k < Z;
}

// the linear gather of src (X, Y, Z) at p, inside [-0.5, n - 0.5] on every axis: the taps reduced along z, then y, then x
__device__ __forceinline__ float linear_gather(const float* __restrict__ src, int X, int Y, int Z, const double* p) {
    int ix[2], iy[2], iz[2];
    float wx[2], wy[2], wz[2];
    axis_taps<kLinear>(p[0], X, ix, wx);
    axis_taps<kLinear>(p[1], Y, iy, wy);
    axis_taps<kLinear>(p[2], Z, iz, wz);
    float rx[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        float ry[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const float* row = src + ((size_t)ix[a] * Y + iy[b]) * Z;
            const float v[2] = {row[iz[0]], row[iz[1]]};
            ry[b] = weighted_sum<2>(wz, v);
        }
        rx[a] = weighted_sum<2>(wy, ry);
    }
    return weighted_sum<2>(wx, rx);
}

// p = m q and the inside test of a volume of extents n
__device__ __forceinline__ bool stack_coordinate(const double (*m)[4], double q0, double q1, double q2, int n0, int n1, int n2, double* p) {
    const int n[3] = {n0, n1, n2};
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = grid_coordinate(m[a], q0, q1, q2);
        inside = inside && p[a] >= -0.5 && p[a] <= (double)n[a] - 0.5;      // NaN compares false
    }
    return inside;
}

// the simulated value of the stack voxel (di, dj, dk) through g: the T samples of the profile along the slice axis, t ascending;
// false (and nothing in sim) where the weight sum stays below 0.5
__device__ __forceinline__ bool stack_simulate(const float* __restrict__ x, int X, int Y, int Z, const double (*g)[4], int axis,
                                               const StackProfile& pr, int T, double di, double dj, double dk, float& sim) {
    const double along = axis == 0 ? di : (axis == 1 ? dj : dk);
    float acc = 0.f, wsum = 0.f;
    for (int t = 0; t < T; ++t) {
        const double s = __dadd_rn(along, pr.offset[t]);
        double p[3];
        if (!stack_coordinate(g, axis == 0 ? s : di, axis == 1 ? s : dj, axis == 2 ? s : dk, X, Y, Z, p)) continue;
        const float w = pr.weight[t];
        acc = __fadd_rn(acc, __fmul_rn(w, linear_gather(x, X, Y, Z, p)));
        wsum = __fadd_rn(wsum, w);
    }
    if (!(wsum >= 0.5f)) return false;
    sim = __fdiv_rn(acc, wsum);
    return true;
}

static inline int check_matrix(const char* name, const double* m12, double (*m)[4]) {
    for (int e = 0; e < 12; ++e) {
        if (!isfinite(m12[e])) MRISR_FAIL(MRISR_E_ARG, "%s: matrix entry [%d][%d] is not finite", name, e / 4, e % 4);
        m[e / 4][e % 4] = m12[e];
    }
    return MRISR_OK;
}

// the profile of an entry into the kernel argument; MRISR_E_ARG for a count outside 1..16 or a sample that is not finite
static inline int check_profile(const char* name, const double* offsets, const float* weights, int T, StackProfile* pr) {
    if (T < 1 || T > kMaxSamples) MRISR_FAIL(MRISR_E_ARG, "%s: %d profile samples (1..%d)", name, T, kMaxSamples);
    *pr = StackProfile{};
    for (int t = 0; t < T; ++t) {
        if (!isfinite(offsets[t]) || !isfinite(weights[t])) MRISR_FAIL(MRISR_E_ARG, "%s: profile sample %d is not finite", name, t);
        pr->offset[t] = offsets[t];
        pr->weight[t] = weights[t];
    }
    return MRISR_OK;
}
