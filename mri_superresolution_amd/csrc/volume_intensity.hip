// Intensity standardisation between scans on the device (gfx950; extension): Nyul-Udupa landmarks.
//
//   f32_volume_masked_percentiles   np.percentile(vol[(mask != 0) & ~isnan(vol)], q) for up to 16 quantiles q at once.  The
//                                   MSD radix select of percentile.hip (four passes of 8 bits over the order-preserving key; the
//                                   key, the rank rule and the interpolation are volume_common.h's) with
//                                   two changes.  The number of counted voxels is known only on the device: pass 0's histogram is
//                                   common to all targets and its total IS the count, so the first pick kernel derives the
//                                   2 nq ranks and the nq weights from it before it picks.  And there are up to 32 targets (two
//                                   order statistics per quantile): after each pick the targets are grouped by their distinct
//                                   prefixes, ascending; a voxel finds its group by a binary search over those (at most 32)
//                                   prefixes and counts into that group's 256-bin histogram in LDS (32 groups: 32 KB).
//                                   Nothing is read back by the host and nothing waits inside a kernel: 9 launches in stream order.
//   f32_volume_piecewise_map        out = d[i] + (v - s[i]) * slope_i on the segment i of the source landmarks s that holds v; the
//                                   first and the last segment extend linearly (no clamp).
//
// The arithmetic restates numpy's float32 path operation by operation (compiled with -ffp-contract=off); the specification is
// volume_intensity.landmarks_np / piecewise_map_np, itself tested against np.percentile (tests/test_volume_intensity_host.py).
#include "volume_common.h"

constexpr int kMaxQ = 16;                    // quantiles per call
constexpr int kMaxT = 2 * kMaxQ;             // targets: the order statistics (k, k + 1) of every quantile
constexpr int kBins = 256;                   // 8-bit digits
constexpr int kPasses = 4;
constexpr int kMaxL = 16;                    // landmarks of the piecewise map
// workspace words: the histograms of the groups, then the state the kernels hand to each other
constexpr int kHistWords = kMaxT * kBins;
constexpr int kOffGroups = kHistWords;                 // number of distinct prefixes
constexpr int kOffCount = kOffGroups + 1;              // counted voxels (n <= 2^32 - 1)
constexpr int kOffGroupPrefix = kOffCount + 1;         // [kMaxT] the distinct prefixes, ascending
constexpr int kOffPrefix = kOffGroupPrefix + kMaxT;    // [kMaxT] per target
constexpr int kOffRank = kOffPrefix + kMaxT;           // [kMaxT] per target: rank left inside its prefix
constexpr int kOffGroup = kOffRank + kMaxT;            // [kMaxT] per target: index of its prefix among the distinct ones
constexpr int kOffGamma = kOffGroup + kMaxT;           // [kMaxQ] float bits: the interpolation weight of every quantile
constexpr int kWsWords = kOffGamma + kMaxQ;

struct QuantileSet {
    int nq;
    float q32[kMaxQ];        // float32(q) / 100, as numpy carries the quantile of a float32 array
};

__global__ __launch_bounds__(256) void masked_select_init_kernel(unsigned* __restrict__ ws) {
    for (int i = threadIdx.x; i < kHistWords; i += 256) ws[i] = 0u;
}

// pass p counts digit p (most significant first) of every counted voxel whose higher digits equal one of the distinct prefixes
__global__ __launch_bounds__(256) void masked_select_hist_kernel(const float* __restrict__ x, const unsigned char* __restrict__ mask, size_t n,
                                                                 unsigned* __restrict__ ws, int pass) {
    __shared__ unsigned h[kMaxT * kBins];
    __shared__ unsigned s_gp[kMaxT];
    const int t = threadIdx.x;
    const int ng = pass == 0 ? 1 : max(1, min((int)ws[kOffGroups], kMaxT));
    if (t < kMaxT) s_gp[t] = t < ng ? (pass == 0 ? 0u : ws[kOffGroupPrefix + t]) : 0xffffffffu;      // a prefix has at most 24 bits
    for (int i = t; i < ng * kBins; i += 256) h[i] = 0u;
    __syncthreads();
    const unsigned gmin = s_gp[0], gmax = s_gp[ng - 1];
    const int shift = 24 - 8 * pass;
    // runs of equal cells (pass 0 of a scan: nearly every voxel of a lane) cost one LDS atomic
    int cur = -1;
    unsigned run = 0u;
    auto count = [&](float v, unsigned m) {
        if (!m || v != v) return;
        const unsigned key = f32_order_key(v);
        const unsigned digit = (key >> shift) & 255u;
        int g = 0;
        if (pass != 0) {
            const unsigned high = key >> (shift + 8);
            if (high < gmin || high > gmax) return;
#pragma unroll
            for (int step = kMaxT / 2; step > 0; step >>= 1)      // first of the 32 padded entries that is >= high
                if (s_gp[g + step - 1] < high) g += step;
            if (s_gp[g] != high) return;
        }
        const int cell = g * kBins + (int)digit;
        if (cell == cur) {
            ++run;
        } else {
            if (run) atomicAdd(&h[cur], run);
            cur = cell;
            run = 1u;
        }
    };
    // 16 bytes of the volume and 4 of the mask per thread and iteration where both start aligned; the tail (or everything) singly
    const bool aligned = ((uintptr_t)x & 15) == 0 && (!mask || ((uintptr_t)mask & 3) == 0);
    const size_t nv = aligned ? n / 4 : 0;
    for (size_t i = (size_t)blockIdx.x * 256 + t; i < nv; i += (size_t)gridDim.x * 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
        const unsigned m4 = mask ? *reinterpret_cast<const unsigned*>(mask + i * 4) : 0x01010101u;
#pragma unroll
        for (int k = 0; k < 4; ++k) count(v[k], (m4 >> (8 * k)) & 255u);
    }
    for (size_t i = nv * 4 + (size_t)blockIdx.x * 256 + t; i < n; i += (size_t)gridDim.x * 256) count(x[i], mask ? mask[i] : 1u);
    if (run) atomicAdd(&h[cur], run);
    __syncthreads();
    for (int i = t; i < ng * kBins; i += 256)
        if (h[i]) atomicAdd(&ws[i], h[i]);
}

// one workgroup: in pass 0 the count, the ranks and the weights; every target's bin of this pass and its rank inside the bin; the
// targets regrouped by their new prefixes; the histograms cleared for the next pass.  After the last pass the prefixes are the
// keys of the order statistics and numpy's two-branch interpolation gives out.
__global__ __launch_bounds__(256) void masked_select_pick_kernel(unsigned* __restrict__ ws, int pass, QuantileSet qs, float* __restrict__ out,
                                                                 long long* __restrict__ count_out) {
    __shared__ unsigned s_prefix[kMaxT], s_rank[kMaxT], s_group[kMaxT], s_new_prefix[kMaxT], s_new_rank[kMaxT], s_first[kMaxT];
    __shared__ unsigned s_total;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int T = 2 * qs.nq;
    const int ng = pass == 0 ? 1 : max(1, min((int)ws[kOffGroups], kMaxT));
    if (t < kMaxT) {
        s_prefix[t] = pass == 0 ? 0u : ws[kOffPrefix + t];
        s_rank[t] = pass == 0 ? 0u : ws[kOffRank + t];
        s_group[t] = pass == 0 ? 0u : ws[kOffGroup + t];
        s_new_prefix[t] = 0u;          // count == 0: no bin holds a rank, the prefixes stay defined
        s_new_rank[t] = 0u;
    }
    if (pass == 0) {
        if (wave == 0) {
            const u32x4 c = *reinterpret_cast<const u32x4*>(ws + lane * 4);
            unsigned sum = c[0] + c[1] + c[2] + c[3];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            if (lane == 0) s_total = sum;
        }
        __syncthreads();
        const unsigned total = s_total;
        if (t < qs.nq) {
            unsigned k0 = 0u, k1 = 0u;
            float gamma = 0.f;
            if (total) np_virtual_index(total, qs.q32[t], &k0, &k1, &gamma);
            s_rank[2 * t] = k0;
            s_rank[2 * t + 1] = k1;
            ws[kOffGamma + t] = __float_as_uint(gamma);
        }
        if (t == 0) {
            ws[kOffCount] = total;
            *count_out = (long long)total;
        }
    }
    __syncthreads();
    // a wave per group: four bins per lane, an inclusive scan across the lanes, then every target of the group looks for the bin
    // with  (count below it) <= rank < (count up to and including it): exactly one, as rank < the group's total
    for (int g = wave; g < ng; g += 4) {
        const u32x4 c = *reinterpret_cast<const u32x4*>(ws + g * kBins + lane * 4);
        const unsigned mine = c[0] + c[1] + c[2] + c[3];
        unsigned incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        for (int k = 0; k < T; ++k) {
            if ((int)s_group[k] != g) continue;
            const unsigned r = s_rank[k];
            unsigned below = incl - mine;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (below <= r && r < below + c[j]) {
                    s_new_prefix[k] = (s_prefix[k] << 8) | (unsigned)(lane * 4 + j);
                    s_new_rank[k] = r - below;
                }
                below += c[j];
            }
        }
    }
    __syncthreads();
    for (int i = t; i < ng * kBins; i += 256) ws[i] = 0u;       // all reads of the histograms are behind the barrier above
    if (pass < kPasses - 1) {
        // the distinct new prefixes in ascending order: a target's group is the number of distinct prefixes below its own
        if (t < T) {
            bool first = true;
            for (int u = 0; u < t; ++u) first = first && s_new_prefix[u] != s_new_prefix[t];
            s_first[t] = first ? 1u : 0u;
        }
        __syncthreads();
        if (t < T) {
            unsigned g = 0u;
            for (int u = 0; u < T; ++u) g += (s_first[u] && s_new_prefix[u] < s_new_prefix[t]) ? 1u : 0u;
            ws[kOffPrefix + t] = s_new_prefix[t];
            ws[kOffRank + t] = s_new_rank[t];
            ws[kOffGroup + t] = g;
            if (s_first[t]) ws[kOffGroupPrefix + g] = s_new_prefix[t];
        }
        if (t == 0) {
            unsigned groups = 0u;
            for (int u = 0; u < T; ++u) groups += s_first[u];
            ws[kOffGroups] = groups;
        }
    } else if (t < qs.nq) {
        const float a = f32_from_order_key(s_new_prefix[2 * t]), c = f32_from_order_key(s_new_prefix[2 * t + 1]);
        const float r = np_lerp_f32(a, c, __uint_as_float(ws[kOffGamma + t]));
        out[t] = ws[kOffCount] ? r : __uint_as_float(0x7fc00000u);      // nothing counted: NaN
    }
}

__global__ __launch_bounds__(256) void piecewise_map_kernel(const float* src, size_t n, const float* __restrict__ sl,
                                                            const float* __restrict__ dl, int L, float* dst) {
    __shared__ float s[kMaxL], d[kMaxL], slope[kMaxL];
    const int t = threadIdx.x;
    if (t < L) {
        s[t] = sl[t];
        d[t] = dl[t];
    }
    if (t < L - 1) {
        const float w = __fsub_rn(sl[t + 1], sl[t]);
        slope[t] = w == 0.f ? 0.f : __fdiv_rn(__fsub_rn(dl[t + 1], dl[t]), w);
    }
    __syncthreads();
    auto map = [&](float v) {
        int c = 0;
        for (int j = 0; j < L; ++j) c += s[j] <= v ? 1 : 0;      // np.searchsorted(s, v, side="right")
        const int i = min(max(c - 1, 0), L - 2);
        return __fadd_rn(d[i], __fmul_rn(__fsub_rn(v, s[i]), slope[i]));
    };
    // src and dst may be one buffer: every element is read and written by the same thread, in the same iteration
    const bool aligned = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const size_t nv = aligned ? n / 4 : 0;
    for (size_t i = (size_t)blockIdx.x * 256 + t; i < nv; i += (size_t)gridDim.x * 256) {
        f32x4 v = *reinterpret_cast<const f32x4*>(src + i * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = map(v[k]);
        *reinterpret_cast<f32x4*>(dst + i * 4) = v;
    }
    for (size_t i = nv * 4 + (size_t)blockIdx.x * 256 + t; i < n; i += (size_t)gridDim.x * 256) dst[i] = map(src[i]);
}

extern "C" size_t mrisr_f32_masked_percentiles_workspace_bytes(int nq) {
    if (nq < 1 || nq > kMaxQ) return 0;
    return (size_t)kWsWords * sizeof(unsigned);
}

extern "C" int mrisr_f32_volume_masked_percentiles(const float* vol, const unsigned char* mask, size_t n, const double* q, int nq, float* out,
                                                   long long* count, void* workspace, void* stream) {
    if (!vol || !q || !out || !count || !workspace) MRISR_FAIL(MRISR_E_ARG, "f32_volume_masked_percentiles: null pointer");
    if (nq < 1 || nq > kMaxQ) MRISR_FAIL(MRISR_E_ARG, "f32_volume_masked_percentiles: %d percentiles (1..%d)", nq, kMaxQ);
    if (n == 0 || n > 0xffffffffull) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_masked_percentiles: %zu voxels", n);
    if (!aligned_to(workspace, 16)) MRISR_FAIL(MRISR_E_ARG, "f32_volume_masked_percentiles: the workspace must be 16-byte aligned");
    QuantileSet qs;
    memset(&qs, 0, sizeof(qs));
    qs.nq = nq;
    for (int i = 0; i < nq; ++i) {
        if (!(q[i] >= 0.0 && q[i] <= 100.0) || (i > 0 && q[i] < q[i - 1]))
            MRISR_FAIL(MRISR_E_ARG, "f32_volume_masked_percentiles: percentile %d is %g (non-decreasing values in [0, 100])", i, q[i]);
        qs.q32[i] = (float)q[i] / 100.f;
    }
    unsigned* ws = (unsigned*)workspace;
    hipStream_t st = (hipStream_t)stream;
    masked_select_init_kernel<<<1, 256, 0, st>>>(ws);
    MRISR_CHECK_LAUNCH("f32_volume_masked_percentiles (init)");
    const int grid = capped_grid(n, 256 * 16, 1024);
    for (int pass = 0; pass < kPasses; ++pass) {
        masked_select_hist_kernel<<<grid, 256, 0, st>>>(vol, mask, n, ws, pass);
        MRISR_CHECK_LAUNCH("f32_volume_masked_percentiles (histogram)");
        masked_select_pick_kernel<<<1, 256, 0, st>>>(ws, pass, qs, out, count);
        MRISR_CHECK_LAUNCH("f32_volume_masked_percentiles (pick)");
    }
    return MRISR_OK;
}

extern "C" int mrisr_f32_volume_piecewise_map(const float* src, size_t n, const float* src_landmarks, const float* dst_landmarks, int L,
                                              float* dst, void* stream) {
    if (!src || !src_landmarks || !dst_landmarks || !dst) MRISR_FAIL(MRISR_E_ARG, "f32_volume_piecewise_map: null pointer");
    if (L < 2 || L > kMaxL) MRISR_FAIL(MRISR_E_ARG, "f32_volume_piecewise_map: %d landmarks (2..%d)", L, kMaxL);
    if (n == 0) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_piecewise_map: no voxels");
    piecewise_map_kernel<<<capped_grid(n, 256 * 8, 2048), 256, 0, (hipStream_t)stream>>>(src, n, src_landmarks, dst_landmarks, L, dst);
    MRISR_CHECK_LAUNCH("f32_volume_piecewise_map");
    return MRISR_OK;
}
