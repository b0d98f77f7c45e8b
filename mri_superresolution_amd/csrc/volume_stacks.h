// What the kernels of the stack reconstruction (csrc/volume_stacks.hip, csrc/volume_slices.hip) share, one definition each: the
// slice profile and the stack-wide views as they travel in the kernel arguments, the linear gather, the forward model and the residual of a stack voxel, the three parts of an update kernel
// (stats prologue, gather over the views, step-clamp-store epilogue) and the host checks the entry points share.  Include from files
// compiled with -ffp-contract=off.
#pragma once
#include "volume_bricks.h"
#include "volume_taps.h"

constexpr int kMaxStacks = MRISR_STACKS_MAX, kMaxSamples = MRISR_STACK_SAMPLES_MAX;

struct StackProfile {
    double offset[kMaxSamples];
    float weight[kMaxSamples];
};
struct StackViews {
    const float* data[kMaxStacks];
    int n[kMaxStacks][3];
    int nslots[kMaxStacks];
    double m[kMaxStacks][3][4];
};

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

// the simulated value of the stack voxel (di, dj, dk) through g: the T samples of the profile along the slice axis, t ascending;
// false (and nothing in sim) where the weight sum stays below 0.5
__device__ __forceinline__ bool stack_simulate(const float* __restrict__ x, int X, int Y, int Z, const double (*g)[4], int axis,
                                               const StackProfile& pr, int T, double di, double dj, double dk, float& sim) {
    const double along = axis == 0 ? di : (axis == 1 ? dj : dk);
    float acc = 0.f, wsum = 0.f;
    for (int t = 0; t < T; ++t) {
        const double s = __dadd_rn(along, pr.offset[t]);
        double p[3];
        if (!matrix_coordinate(g, axis == 0 ? s : di, axis == 1 ? s : dj, axis == 2 ? s : dk, X, Y, Z, p)) continue;
        const float w = pr.weight[t];
        acc = __fadd_rn(acc, __fmul_rn(w, linear_gather(x, X, Y, Z, p)));
        wsum = __fadd_rn(wsum, w);
    }
    if (!(wsum >= 0.5f)) return false;
    sim = __fdiv_rn(acc, wsum);
    return true;
}

// the residual of the stack voxel idx = (i, j, k) through g: y - the simulated value, its square into sq, where the weight sum
// reaches 0.5; +0 elsewhere
__device__ __forceinline__ void stack_residual_voxel(const float* __restrict__ x, int X, int Y, int Z, const float* __restrict__ y,
                                                     const double (*g)[4], int axis, const StackProfile& pr, int T, int i, int j, int k,
                                                     size_t idx, float* __restrict__ r, PairSum& sq) {
    float sim, res = 0.f;
    if (stack_simulate(x, X, Y, Z, g, axis, pr, T, (double)i, (double)j, (double)k, sim)) {
        res = __fsub_rn(y[idx], sim);
        sq.add((double)res * (double)res, 0.0, 1);          // the square of a float is exact in double
    }
    r[idx] = res;
}

// the first wave of an update launch adds the slots the K residual launches left into the iteration's stats rows
__device__ __forceinline__ void stack_update_stats(const DeformSlot* __restrict__ slots, const int* nslots, int K, StatsRow* __restrict__ rows) {
    if (rows && blockIdx.x == 0 && threadIdx.x < 64)
        for (int s = 0; s < K; ++s) finalize_force(slots + (size_t)s * kSlots, nslots[s], rows + s);
}

// sum: for s ascending, the linear gather of stack s at the output voxel (di, dj, dk) where that lies inside it; -> their count
__device__ __forceinline__ int stack_gather_views(const StackViews& v, int K, double di, double dj, double dk, float& sum) {
    int cnt = 0;
    sum = 0.f;
#pragma unroll 1
    for (int s = 0; s < K; ++s) {
        double p[3];
        if (!matrix_coordinate(v.m[s], di, dj, dk, v.n[s][0], v.n[s][1], v.n[s][2], p)) continue;
        sum = __fadd_rn(sum, linear_gather(v.data[s], v.n[s][0], v.n[s][1], v.n[s][2], p));
        ++cnt;
    }
    return cnt;
}

// out[idx] = xv + step * term(), clamped from below, where cnt > 0 and xv elsewhere; cover[idx] = cnt.  term: what the step
// multiplies - the mean of the stacks, sum / float(cnt), to which the regulariser adds its part; evaluated where cnt > 0 alone
template <class Term>
__device__ __forceinline__ void stack_update_store(float xv, int cnt, float step, int use_clamp, float lo, float* out,
                                                   unsigned char* __restrict__ cover, size_t idx, Term term) {
    if (cnt > 0) {
        xv = __fadd_rn(xv, __fmul_rn(step, term()));
        if (use_clamp && xv < lo) xv = lo;                  // a NaN stays
    }
    out[idx] = xv;
    if (cover) cover[idx] = (unsigned char)cnt;
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

// the step of every update entry: the stack count, the step and the clamp
static inline int check_update_step(const char* name, int K, float step, int use_clamp, float lo) {
    if (K < 1 || K > kMaxStacks) MRISR_FAIL(MRISR_E_ARG, "%s: %d stacks (1..%d)", name, K, kMaxStacks);
    if (!isfinite(step)) MRISR_FAIL(MRISR_E_ARG, "%s: step %g is not finite", name, (double)step);
    if (use_clamp != 0 && use_clamp != 1) MRISR_FAIL(MRISR_E_ARG, "%s: use_clamp %d (0 or 1)", name, use_clamp);
    if (use_clamp && !isfinite(lo)) MRISR_FAIL(MRISR_E_ARG, "%s: the lower clamp %g is not finite", name, (double)lo);
    return MRISR_OK;
}

// the estimate of every update entry: workspace and stats rows together or neither, the output grid, the alignment
static inline int check_update_volume(const char* name, const float* x, int X, int Y, int Z, const float* out, const void* workspace,
                                      const void* stats_rows, BrickGrid* grid) {
    if ((workspace == nullptr) != (stats_rows == nullptr)) MRISR_FAIL(MRISR_E_ARG, "%s: workspace and stats_rows go together", name);
    if (const int rc = check_field_volume(name, X, Y, Z, grid)) return rc;
    if (!aligned_to(x, 4) || !aligned_to(out, 4) || !aligned_to(workspace, 8) || !aligned_to(stats_rows, 8))
        MRISR_FAIL(MRISR_E_ARG, "%s: misaligned pointer", name);
    return MRISR_OK;
}
