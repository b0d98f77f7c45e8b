// What the volume kernels (csrc/volume_*.hip), percentile.hip and image.hip share, one definition each: the order-preserving key
// of a float, the register run in front of an LDS histogram, np.percentile's float32 rule and the host helpers of the launch
// wrappers.  The arithmetic restates numpy operation by operation; the specification of the percentile rule is
// utils/imageops.np_percentile_f32.
#pragma once
#include "common.h"

#include <math.h>

// ---------------------------------------------------------------- order-preserving key of a float
// Unsigned comparison of the keys is the comparison of the floats (negatives: all bits flipped, others: sign bit flipped).
// -0.0 sorts below +0.0; a caller that must not tell them apart passes v + 0.f.
__device__ __forceinline__ unsigned f32_order_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_from_order_key(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---------------------------------------------------------------- a run of equal cells in a register
// Flushed to the (LDS) histogram with one atomic when the cell changes: neighbouring voxels mostly fall into one cell, and
// same-address LDS atomics serialise.  Start with len = 0; flush after the last add.
struct RunCounter {
    int cell;
    unsigned len;
    __device__ __forceinline__ void add(int c, unsigned* hist) {
        if (c == cell) {
            ++len;
        } else {
            if (len) atomicAdd(&hist[cell], len);
            cell = c;
            len = 1u;
        }
    }
    __device__ __forceinline__ void flush(unsigned* hist) {
        if (len) atomicAdd(&hist[cell], len);
        len = 0u;
    }
};

// ---------------------------------------------------------------- np.percentile of float32[n], n >= 1
// numpy carries the quantile and the virtual index in float32: q32 = float32(q) / 100 (the caller's), v = float32(n - 1) * q32.
// k0 = floor(v) is the rank of the lower order statistic, k1 its upper neighbour, gamma = v - floor(v) the weight of np_lerp_f32.
__host__ __device__ inline void np_virtual_index(unsigned n, float q32, unsigned* k0, unsigned* k1, float* gamma) {
#pragma clang fp contract(off)
    const float virt = (float)(n - 1u) * q32;
    const float prev = floorf(virt);
    unsigned long long k = (unsigned long long)prev;
    if (k > n - 1u) k = n - 1u;             // float32(n - 1) may round up past the last index when n > 2^24
    *k0 = (unsigned)k;
    *k1 = k + 1 < n ? (unsigned)(k + 1) : n - 1u;
    *gamma = virt - prev;
}
// numpy's _lerp in float32: a + (c - a) * gamma, and c - (c - a) * (1 - gamma) where gamma >= 0.5
__device__ __forceinline__ float np_lerp_f32(float a, float c, float gamma) {
    const float diff = __fsub_rn(c, a);
    float r = __fadd_rn(a, __fmul_rn(diff, gamma));
    if (gamma >= 0.5f) r = __fsub_rn(c, __fmul_rn(diff, __fsub_rn(1.f, gamma)));
    return r;
}

// ---------------------------------------------------------------- host helpers of the launch wrappers
// workgroups for n elements at per_block each: at least one, at most cap
static inline int capped_grid(size_t n, size_t per_block, int cap) {
    const size_t b = (n + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > (size_t)cap ? (size_t)cap : b));
}
static inline bool aligned_to(const void* p, size_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }      // bytes: a power of two

// extent of a volume per axis: doubled extents, products of two extents and block counts stay inside int and the grid limits
constexpr int kMaxDim = 32767;
static inline bool volume_extents_ok(int X, int Y, int Z) {
    return X >= 1 && Y >= 1 && Z >= 1 && X <= kMaxDim && Y <= kMaxDim && Z <= kMaxDim;
}
static inline int check_volume_extents(const char* name, int X, int Y, int Z) {
    if (!volume_extents_ok(X, Y, Z))
        MRISR_FAIL(MRISR_E_SHAPE, "%s: volume %d x %d x %d (every axis 1..%d)", name, X, Y, Z, kMaxDim);
    return MRISR_OK;
}
