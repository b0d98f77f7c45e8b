// Float windowing of whole-volume inference on the device (gfx950; extension).
//
// MRI arrives as 12- to 16-bit or float volumes, and the reference windows each float32 slice at its 0.5 / 99.5 percentiles
// before anything else sees it (utils/extraction_utils.py:118-131 -> utils/preprocessing.py:126-158 robust_normalize).  The
// 256-bin histogram of image.hip cannot express the percentile of a float image, so this file selects it exactly:
//
//   f32_percentile_bounds   np.percentile(img_b, q) of every image of a batch for two q: an MSD radix select over the
//                           order-preserving 32-bit key of the float (negatives: all bits flipped, others: sign bit flipped),
//                           four passes of 8 bits.  Each quantile needs two order statistics, so four targets are tracked
//                           per image, each with its own (prefix, remaining rank).  Per pass: one histogram kernel (several
//                           workgroups per image, 256-bin histograms in LDS merged into the workspace with atomicAdd) and
//                           one tiny kernel that picks every target's bin.  Targets whose prefixes are still equal share
//                           one histogram (the first of them counts, the others read its bins), which is the common case:
//                           ranks k and k + 1 part ways in the last pass or never.  Workgroups hand over to each other by
//                           launch order only; nothing waits inside a kernel, nothing is read back by the host.
//   f32_window_normalise    (clip(x, lo, hi) - lo) / (hi - lo), zeros where hi == lo (robust_normalize's constant slices)
//   f32_window_restore      clamp(y, 0, 1) * (hi - lo) + lo -> float32 or int16 (np.rint, saturated)
//
// The arithmetic restates numpy's float32 path operation by operation (compiled with -ffp-contract=off): for a float32
// array np.percentile carries the quantile and the virtual index in float32 (the same rule as np_percentile_u8 of image.hip) and
// ends in _lerp's two branches: np_virtual_index and np_lerp_f32 of volume_common.h, where the key lives too.  The specification
// is utils/imageops.percentile_bounds_np, itself tested against np.percentile (tests/test_percentile_host.py).
#include "volume_common.h"

constexpr int kTargets = 4;                  // order statistics per image: (k, k + 1) of q_lo, (k, k + 1) of q_hi
constexpr int kBins = 256;                   // 8-bit digits
constexpr int kPasses = 4;
constexpr int kImageWords = kTargets * kBins + 2 * kTargets;    // workspace words per image: histograms, prefixes, ranks

struct RankSet { unsigned k[kTargets]; };

// first target whose prefix equals target t's: the one that owns their common histogram
__device__ __forceinline__ int owner_of(const unsigned* prefix, int t) {
    int o = t;
#pragma unroll
    for (int u = kTargets - 1; u >= 0; --u)
        if (u < t && prefix[u] == prefix[t]) o = u;
    return o;
}

__global__ __launch_bounds__(256) void f32_select_init_kernel(unsigned* __restrict__ ws, RankSet ranks) {
    unsigned* w = ws + (size_t)blockIdx.x * kImageWords;
    for (int i = threadIdx.x; i < kTargets * kBins; i += 256) w[i] = 0u;
    if (threadIdx.x < kTargets) {
        w[kTargets * kBins + threadIdx.x] = 0u;
        w[kTargets * kBins + kTargets + threadIdx.x] = ranks.k[threadIdx.x];
    }
}

// pass p counts digit p (most significant first) of every key whose higher digits equal a target's prefix
__global__ __launch_bounds__(256) void f32_select_hist_kernel(const float* __restrict__ x, size_t n, unsigned* __restrict__ ws, int pass) {
    __shared__ unsigned h[kTargets][kBins];
    const int t = threadIdx.x, b = blockIdx.y;
    unsigned* w = ws + (size_t)b * kImageWords;
    unsigned prefix[kTargets];
    bool own[kTargets];
#pragma unroll
    for (int k = 0; k < kTargets; ++k) prefix[k] = w[kTargets * kBins + k];
#pragma unroll
    for (int k = 0; k < kTargets; ++k) own[k] = owner_of(prefix, k) == k;
#pragma unroll
    for (int k = 0; k < kTargets; ++k) h[k][t] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    auto count = [&](float v) {
        const unsigned key = f32_order_key(v);
        const unsigned high = pass == 0 ? 0u : key >> (shift + 8);
        const unsigned digit = (key >> shift) & 255u;
#pragma unroll
        for (int k = 0; k < kTargets; ++k)
            if (own[k] && high == prefix[k]) atomicAdd(&h[k][digit], 1u);
    };
    const float* p = x + (size_t)b * n;
    // 16 bytes per thread and iteration where the image starts aligned; the tail (or everything) by single floats
    const size_t nv = ((uintptr_t)p & 15) == 0 ? n / 4 : 0;
    for (size_t i = (size_t)blockIdx.x * 256 + t; i < nv; i += (size_t)gridDim.x * 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + i * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) count(v[k]);
    }
    for (size_t i = nv * 4 + (size_t)blockIdx.x * 256 + t; i < n; i += (size_t)gridDim.x * 256) count(p[i]);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTargets; ++k)
        if (own[k] && h[k][t]) atomicAdd(&w[k * kBins + t], h[k][t]);
}

// one workgroup per image: every target's bin of this pass, its rank inside the bin; clears the histograms for the next
// pass (or the next call); after the last pass the four keys are values and the two interpolations give lohi
__global__ __launch_bounds__(256) void f32_select_pick_kernel(unsigned* __restrict__ ws, int pass, float t_lo, float t_hi,
                                                              float* __restrict__ lohi) {
    __shared__ unsigned cum[kBins];
    __shared__ unsigned s_prefix[kTargets], s_rank[kTargets], s_new_prefix[kTargets], s_new_rank[kTargets];
    const int t = threadIdx.x, b = blockIdx.x;
    unsigned* w = ws + (size_t)b * kImageWords;
    if (t < kTargets) {
        s_prefix[t] = w[kTargets * kBins + t];
        s_rank[t] = w[kTargets * kBins + kTargets + t];
    }
    __syncthreads();
    for (int k = 0; k < kTargets; ++k) {
        const unsigned mine = w[owner_of(s_prefix, k) * kBins + t];
        cum[t] = mine;
        __syncthreads();
        for (int o = 1; o < kBins; o <<= 1) {       // inclusive scan (256 entries: Hillis-Steele is fine)
            const unsigned v = t >= o ? cum[t - o] : 0u;
            __syncthreads();
            cum[t] += v;
            __syncthreads();
        }
        // the bin with  (count below it) <= rank < (count up to and including it): exactly one, as rank < total
        const unsigned incl = cum[t], excl = incl - mine, r = s_rank[k];
        if (excl <= r && r < incl) {
            s_new_prefix[k] = (s_prefix[k] << 8) | (unsigned)t;
            s_new_rank[k] = r - excl;
        }
        __syncthreads();
    }
    for (int i = t; i < kTargets * kBins; i += 256) w[i] = 0u;       // all reads of the histograms are behind the barrier above
    if (t < kTargets) {
        w[kTargets * kBins + t] = s_new_prefix[t];
        w[kTargets * kBins + kTargets + t] = s_new_rank[t];
    }
    if (pass == kPasses - 1 && t < 2) {
        const float a = f32_from_order_key(s_new_prefix[2 * t]), c = f32_from_order_key(s_new_prefix[2 * t + 1]);
        lohi[2 * (size_t)b + t] = np_lerp_f32(a, c, t == 0 ? t_lo : t_hi);
    }
}

__global__ __launch_bounds__(256) void f32_window_normalise_kernel(const float* __restrict__ x, const float* __restrict__ lohi, size_t n,
                                                                   float* __restrict__ out) {
    const int b = blockIdx.y;
    const float lo = lohi[2 * b], hi = lohi[2 * b + 1];
    const float range = __fsub_rn(hi, lo);
    const bool flat = hi == lo;            // robust_normalize: a constant slice (upper == lower) becomes zeros
    const float* p = x + (size_t)b * n;
    float* o = out + (size_t)b * n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float c = fminf(fmaxf(p[i], lo), hi);            // np.clip
        o[i] = flat ? 0.f : __fdiv_rn(__fsub_rn(c, lo), range);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void f32_window_restore_kernel(const float* __restrict__ y, const float* __restrict__ lohi, size_t n,
                                                                 T* __restrict__ out) {
    const int b = blockIdx.y;
    const float lo = lohi[2 * b], hi = lohi[2 * b + 1];
    const float range = __fsub_rn(hi, lo);
    const float* p = y + (size_t)b * n;
    T* o = out + (size_t)b * n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float c = fminf(fmaxf(p[i], 0.f), 1.f);           // NaN -> 0 like fmaxf
        const float r = __fadd_rn(__fmul_rn(c, range), lo);     // two roundings, as numpy's c * (hi - lo) + lo
        if constexpr (sizeof(T) == 2) o[i] = (T)(int)fminf(fmaxf(rintf(r), -32768.f), 32767.f);    // np.rint: half to even
        else o[i] = r;
    }
}

extern "C" size_t mrisr_f32_percentile_workspace_bytes(int batch) {
    if (batch < 1 || batch > 65535) return 0;
    return (size_t)batch * kImageWords * sizeof(unsigned);
}

extern "C" int mrisr_f32_percentile_bounds(const float* x, size_t pixels_per_image, int batch, double q_lo, double q_hi, float* lohi,
                                           void* workspace, void* stream) {
    if (!x || !lohi || !workspace) MRISR_FAIL(MRISR_E_ARG, "f32_percentile_bounds: null pointer");
    if (batch < 1 || batch > 65535 || pixels_per_image == 0 || pixels_per_image > 0xffffffffull)
        MRISR_FAIL(MRISR_E_SHAPE, "f32_percentile_bounds: batch %d, %zu pixels", batch, pixels_per_image);
    if (!(q_lo >= 0.0 && q_lo <= q_hi && q_hi <= 100.0)) MRISR_FAIL(MRISR_E_ARG, "f32_percentile_bounds: percentiles %g, %g", q_lo, q_hi);
    RankSet ranks;
    float t_lo, t_hi;
    const unsigned n = (unsigned)pixels_per_image;      // checked above: 1 .. 2^32 - 1
    np_virtual_index(n, (float)q_lo / 100.f, &ranks.k[0], &ranks.k[1], &t_lo);
    np_virtual_index(n, (float)q_hi / 100.f, &ranks.k[2], &ranks.k[3], &t_hi);
    unsigned* ws = (unsigned*)workspace;
    hipStream_t st = (hipStream_t)stream;
    f32_select_init_kernel<<<batch, 256, 0, st>>>(ws, ranks);
    MRISR_CHECK_LAUNCH("f32_percentile_bounds (init)");
    const dim3 grid(capped_grid(pixels_per_image, 256 * 16, 64), batch);
    for (int pass = 0; pass < kPasses; ++pass) {
        f32_select_hist_kernel<<<grid, 256, 0, st>>>(x, pixels_per_image, ws, pass);
        MRISR_CHECK_LAUNCH("f32_percentile_bounds (histogram)");
        f32_select_pick_kernel<<<batch, 256, 0, st>>>(ws, pass, t_lo, t_hi, lohi);
        MRISR_CHECK_LAUNCH("f32_percentile_bounds (pick)");
    }
    return MRISR_OK;
}

extern "C" int mrisr_f32_window_normalise(const float* x, const float* lohi, size_t pixels_per_image, int batch, float* out, void* stream) {
    if (!x || !lohi || !out) MRISR_FAIL(MRISR_E_ARG, "f32_window_normalise: null pointer");
    if (batch < 1 || batch > 65535 || pixels_per_image == 0) MRISR_FAIL(MRISR_E_SHAPE, "f32_window_normalise: batch %d, %zu pixels", batch, pixels_per_image);
    const dim3 grid(capped_grid(pixels_per_image, 256 * 8, 256), batch);
    f32_window_normalise_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, lohi, pixels_per_image, out);
    MRISR_CHECK_LAUNCH("f32_window_normalise");
    return MRISR_OK;
}

extern "C" int mrisr_f32_window_restore(const float* y, const float* lohi, size_t pixels_per_image, int batch, int out_dtype, void* out,
                                        void* stream) {
    if (!y || !lohi || !out) MRISR_FAIL(MRISR_E_ARG, "f32_window_restore: null pointer");
    if (batch < 1 || batch > 65535 || pixels_per_image == 0) MRISR_FAIL(MRISR_E_SHAPE, "f32_window_restore: batch %d, %zu pixels", batch, pixels_per_image);
    const dim3 grid(capped_grid(pixels_per_image, 256 * 8, 256), batch);
    if (out_dtype == MRISR_WINDOW_F32)
        f32_window_restore_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(y, lohi, pixels_per_image, (float*)out);
    else if (out_dtype == MRISR_WINDOW_I16)
        f32_window_restore_kernel<int16_t><<<grid, 256, 0, (hipStream_t)stream>>>(y, lohi, pixels_per_image, (int16_t*)out);
    else
        MRISR_FAIL(MRISR_E_ARG, "f32_window_restore: out_dtype %d", out_dtype);
    MRISR_CHECK_LAUNCH("f32_window_restore");
    return MRISR_OK;
}
