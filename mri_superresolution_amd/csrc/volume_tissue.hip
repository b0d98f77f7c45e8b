// Tissue classification of a float32 volume on the device and the overlap of two label volumes (gfx950; extension, DESIGN.md
// section 7).  The specification is mri_superresolution_amd/volume_tissue.py; every kernel here is bit-equal to it.  Compiled with
// -ffp-contract=off (build.py): the bin of a voxel is a rounded float32 difference and a rounded float32 product, never an fma.
// Everything else is integer arithmetic, so no result depends on the order in which voxels are visited.
//
// A volume is (X, Y, Z) in C order, Z fastest.  A label volume is uint8: 0 outside the mask, 1..K inside.
//
//   quantise     q = the bin 0..255 of every voxel between range2 = (lo, hi), the 64-bit histogram of the bins inside the mask and,
//                when asked for, the seed of the labels (1 inside the mask, 0 outside), in one pass: 16-byte reads of the volume
//                and word accesses of the byte volumes where the pointers allow, the scalar form otherwise.  RunCounter (volume_common.h)
//                in front of a 32-bit LDS histogram, then one 64-bit atomic per non-zero bin and workgroup.
//   joint_hist   the same pattern over the cell (label - 1) * 256 + q, K * 256 LDS counters; label 0 and labels above K are skipped.
//   icm_half     one half-sweep of iterated conditional modes in place: the voxels inside the mask (label != 0) with
//                (x + y + z) & 1 == colour take the class of the smallest cost[k][q] + beta_q * d_k.  The cost table goes to LDS once
//                per workgroup (at most 6 KB, read with ds_read_b32).  A thread owns 16 consecutive z of one (x, y) row: it loads the
//                run's labels, its bins and the four neighbouring rows' labels (four words each where Z % 4 == 0 and the pointers
//                are on 4 bytes, bytes otherwise) and the two bytes in front of and behind the run; the in-row neighbours come
//                from registers.  Only voxels of `colour` change, and all six neighbours of such a voxel have the other colour, so
//                the update in place reads nothing that this launch changes.
//                Stores, the form built: in the word form a thread writes back the words of its run in which a label changed,
//                the other colour's bytes unchanged.  That is allowed because no other thread writes those bytes in this launch
//                (a run belongs to one thread), and a thread that reads them at the same time reads the value they had before
//                and have after.  It was chosen because a byte store costs a memory instruction like a word store: one to four
//                stores per run where the byte form issues up to eight.  The byte form (unaligned pointers, Z % 4 != 0) stores
//                the changed bytes alone.
//   confusion    an LDS histogram over a * (K + 1) + b inside the mask; a voxel with a label above K goes to one extra cell and is
//                not tallied, so no access leaves the table.
// The counters are accumulated: the caller clears them.  No kernel reads past n or outside a row: extents of 1, odd extents,
// n % 4 != 0, unaligned sub-tensor pointers and an empty mask take the same code with shorter loops.
#include "volume_common.h"

constexpr int kBins = 256;
constexpr int kMaxClasses = 6;
constexpr int kHistPerBlock = 16384;       // voxels a workgroup of the histogram passes takes per grid-stride step
constexpr int kMaxHistBlocks = 4096;
constexpr int kIcmRun = 16;                // consecutive z a thread of the half-sweep owns
constexpr int kMaxIcmBlocks = 1 << 16;
constexpr int kMaxBetaQ = 16 << 16;

struct QuantRange { float lo, scale; bool degenerate; };
__device__ __forceinline__ QuantRange quant_range(const float* __restrict__ range2) {
    QuantRange r;
    const float lo = range2[0], hi = range2[1];
    const float width = __fsub_rn(hi, lo);
    r.lo = lo;
    r.scale = __fdiv_rn(256.f, width);
    r.degenerate = hi == lo || !isfinite(width) || !isfinite(r.scale);
    return r;
}
// otsu_bin of volume_mask.hip clamped on both sides; the clamp is made in float so that the conversion stays in range
__device__ __forceinline__ unsigned quant_bin(float v, const QuantRange& r) {
    if (r.degenerate) return 0u;
    const float p = __fmul_rn(__fsub_rn(v, r.lo), r.scale);
    return (unsigned)(int)fminf(fmaxf(p, 0.f), (float)(kBins - 1));      // truncation
}

// vec: vol on 16 bytes, mask, q and labels on 4; the n / 4 whole vectors grid-stride, the tail of n % 4 goes to block 0
__global__ __launch_bounds__(256) void tissue_quantise_kernel(const float* __restrict__ v, const uint8_t* __restrict__ mask, size_t n, int vec,
                                                              const float* __restrict__ range2, uint8_t* __restrict__ q,
                                                              uint8_t* __restrict__ labels, unsigned long long* __restrict__ hist,
                                                              unsigned long long* __restrict__ flags) {
    __shared__ unsigned lh[kBins];
    const QuantRange r = quant_range(range2);
    lh[threadIdx.x] = 0u;
    __syncthreads();
    RunCounter run{0, 0u};
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    auto one = [&](size_t i) {
        const unsigned b = quant_bin(v[i], r), inside = mask[i] ? 1u : 0u;
        q[i] = (uint8_t)b;
        if (labels) labels[i] = (uint8_t)inside;
        if (inside) run.add((int)b, lh);
    };
    if (vec) {
        const size_t n4 = n / 4;
        for (size_t i = tid; i < n4; i += stride) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(v + 4 * i);
            const unsigned m = *reinterpret_cast<const unsigned*>(mask + 4 * i);
            unsigned qw = 0u, lw = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned b = quant_bin(x[k], r), inside = ((m >> 8 * k) & 255u) ? 1u : 0u;
                qw |= b << 8 * k;
                lw |= inside << 8 * k;
                if (inside) run.add((int)b, lh);
            }
            *reinterpret_cast<unsigned*>(q + 4 * i) = qw;
            if (labels) *reinterpret_cast<unsigned*>(labels + 4 * i) = lw;
        }
        if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) one(4 * n4 + threadIdx.x);
    } else {
        for (size_t i = tid; i < n; i += stride) one(i);
    }
    run.flush(lh);
    __syncthreads();
    const unsigned c = lh[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], (unsigned long long)c);
    if (blockIdx.x == 0 && threadIdx.x == 0 && r.degenerate) atomicOr(flags, 1ull);
}

// vec: both pointers on 16 bytes; the n / 16 whole vectors grid-stride, the tail goes to block 0
__global__ __launch_bounds__(256) void tissue_joint_hist_kernel(const uint8_t* __restrict__ q, const uint8_t* __restrict__ labels, size_t n,
                                                                int vec, int K, unsigned long long* __restrict__ joint) {
    __shared__ unsigned lh[kMaxClasses * kBins];
    for (int i = threadIdx.x; i < K * kBins; i += 256) lh[i] = 0u;
    __syncthreads();
    RunCounter run{0, 0u};
    auto add = [&](unsigned bin, unsigned label) {
        if (label - 1u < (unsigned)K) run.add((int)((label - 1u) * kBins + bin), lh);      // 0 and labels above K: skipped
    };
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    if (vec) {
        const size_t n16 = n / 16;
        for (size_t i = tid; i < n16; i += stride) {
            const u32x4 qw = *reinterpret_cast<const u32x4*>(q + 16 * i), lw = *reinterpret_cast<const u32x4*>(labels + 16 * i);
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int k = 0; k < 4; ++k) add((qw[w] >> 8 * k) & 255u, (lw[w] >> 8 * k) & 255u);
        }
        if (blockIdx.x == 0 && threadIdx.x < (int)(n - 16 * n16)) add(q[16 * n16 + threadIdx.x], labels[16 * n16 + threadIdx.x]);
    } else {
        for (size_t i = tid; i < n; i += stride) add(q[i], labels[i]);
    }
    run.flush(lh);
    __syncthreads();
    for (int i = threadIdx.x; i < K * kBins; i += 256) {
        const unsigned c = lh[i];
        if (c) atomicAdd(&joint[i], (unsigned long long)c);
    }
}

// conf: (K + 1)^2 cells and one more for the voxels with a label above K
__global__ __launch_bounds__(256) void tissue_confusion_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                               const uint8_t* __restrict__ mask, size_t n, int vec, int K,
                                                               unsigned long long* __restrict__ conf) {
    __shared__ unsigned lh[64];
    const int cells = (K + 1) * (K + 1);
    if (threadIdx.x < 64) lh[threadIdx.x] = 0u;
    __syncthreads();
    RunCounter run{0, 0u};
    auto add = [&](unsigned la, unsigned lb, unsigned m) {
        if (!m) return;
        run.add(la > (unsigned)K || lb > (unsigned)K ? cells : (int)(la * (unsigned)(K + 1) + lb), lh);
    };
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    if (vec) {
        const size_t n16 = n / 16;
        for (size_t i = tid; i < n16; i += stride) {
            const u32x4 aw = *reinterpret_cast<const u32x4*>(a + 16 * i), bw = *reinterpret_cast<const u32x4*>(b + 16 * i);
            u32x4 mw = {~0u, ~0u, ~0u, ~0u};
            if (mask) mw = *reinterpret_cast<const u32x4*>(mask + 16 * i);
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int k = 0; k < 4; ++k) add((aw[w] >> 8 * k) & 255u, (bw[w] >> 8 * k) & 255u, (mw[w] >> 8 * k) & 255u);
        }
        if (blockIdx.x == 0 && threadIdx.x < (int)(n - 16 * n16)) {
            const size_t i = 16 * n16 + threadIdx.x;
            add(a[i], b[i], mask ? mask[i] : 1u);
        }
    } else {
        for (size_t i = tid; i < n; i += stride) add(a[i], b[i], mask ? mask[i] : 1u);
    }
    run.flush(lh);
    __syncthreads();
    if (threadIdx.x <= cells) {
        const unsigned c = lh[threadIdx.x];
        if (c) atomicAdd(&conf[threadIdx.x], (unsigned long long)c);
    }
}

// ---------------------------------------------------------------- the half-sweep

// the len (<= 16) bytes at p as four words, zero behind them.  VEC: p on 4 bytes and len a multiple of 4
template <bool VEC> __device__ __forceinline__ void load_run(const uint8_t* p, int len, unsigned (&w)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (VEC) {
            w[j] = 4 * j < len ? *reinterpret_cast<const unsigned*>(p + 4 * j) : 0u;
        } else {
            unsigned word = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * j + k < len) word |= (unsigned)p[4 * j + k] << 8 * k;
            w[j] = word;
        }
    }
}
__device__ __forceinline__ unsigned run_byte(const unsigned (&w)[4], int i) { return (w[i >> 2] >> 8 * (i & 3)) & 255u; }

template <bool VEC>
__global__ __launch_bounds__(256) void tissue_icm_half_kernel(const uint8_t* __restrict__ q, uint8_t* labels, int X, int Y, int Z, int K,
                                                              const int* __restrict__ cost, int beta_q, int colour,
                                                              unsigned long long* __restrict__ changed) {
    __shared__ int tab[kMaxClasses * kBins];
    for (int i = threadIdx.x; i < K * kBins; i += 256) tab[i] = cost[i];
    __syncthreads();
    const int runs = (Z + kIcmRun - 1) / kIcmRun;
    const long long total = (long long)X * Y * runs;
    const size_t plane = (size_t)Y * Z;
    unsigned nchanged = 0u;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long row = t / runs;
        const int z0 = (int)(t - row * runs) * kIcmRun;
        const int x = (int)(row / Y), y = (int)(row - (long long)x * Y);
        const int len = Z - z0 < kIcmRun ? Z - z0 : kIcmRun;
        const size_t base = (size_t)row * Z + z0;
        unsigned own[4], bins[4], xm[4] = {0u, 0u, 0u, 0u}, xp[4] = {0u, 0u, 0u, 0u}, ym[4] = {0u, 0u, 0u, 0u}, yp[4] = {0u, 0u, 0u, 0u};
        load_run<VEC>(labels + base, len, own);
        if ((own[0] | own[1] | own[2] | own[3]) == 0u) continue;          // the run lies outside the mask
        load_run<VEC>(q + base, len, bins);
        if (x > 0) load_run<VEC>(labels + base - plane, len, xm);
        if (x < X - 1) load_run<VEC>(labels + base + plane, len, xp);
        if (y > 0) load_run<VEC>(labels + base - Z, len, ym);
        if (y < Y - 1) load_run<VEC>(labels + base + Z, len, yp);
        const unsigned before = z0 > 0 ? labels[base - 1] : 0u;
        const unsigned after = z0 + kIcmRun < Z ? labels[base + kIcmRun] : 0u;
        unsigned out[4] = {own[0], own[1], own[2], own[3]};
        const int parity = (x + y + z0) & 1;                              // kIcmRun is even: voxel i of the run has parity ^ (i & 1)
#pragma unroll
        for (int i = 0; i < kIcmRun; ++i) {
            const unsigned label = run_byte(own, i);                       // 0 behind the end of the row as well
            if ((parity ^ (i & 1)) != colour || label == 0u) continue;
            const unsigned nb[6] = {run_byte(xm, i), run_byte(xp, i), run_byte(ym, i), run_byte(yp, i),
                                    i > 0 ? run_byte(own, i - 1) : before, i < kIcmRun - 1 ? run_byte(own, i + 1) : after};
            int nonzero = 0;
#pragma unroll
            for (int j = 0; j < 6; ++j) nonzero += nb[j] != 0u;
            const unsigned bin = run_byte(bins, i);
            unsigned best = 0u;
            int best_e = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < kMaxClasses; ++k) {
                if (k >= K) break;
                int same = 0;
#pragma unroll
                for (int j = 0; j < 6; ++j) same += nb[j] == (unsigned)(k + 1);
                const int e = tab[k * kBins + bin] + beta_q * (nonzero - same);      // at most 2^30 + 6 * 2^20
                if (e < best_e) {                                            // a tie stays with the smaller class
                    best_e = e;
                    best = (unsigned)(k + 1);
                }
            }
            if (best != label) {
                out[i >> 2] = (out[i >> 2] & ~(255u << 8 * (i & 3))) | best << 8 * (i & 3);
                ++nchanged;
            }
        }
        if (VEC) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (out[j] != own[j]) *reinterpret_cast<unsigned*>(labels + base + 4 * j) = out[j];      // only words inside the row differ
        } else {
#pragma unroll
            for (int i = 0; i < kIcmRun; ++i)
                if (run_byte(out, i) != run_byte(own, i)) labels[base + i] = (uint8_t)run_byte(out, i);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nchanged += (unsigned)__shfl_xor((int)nchanged, o, 64);
    if ((threadIdx.x & 63) == 0 && nchanged) atomicAdd(changed, (unsigned long long)nchanged);
}

// ---------------------------------------------------------------- entries

static inline bool classes_ok(int K) { return K >= 2 && K <= kMaxClasses; }

extern "C" int mrisr_f32_volume_quantise(const float* vol, const uint8_t* mask, size_t n, const float* range2, uint8_t* q_out,
                                         uint8_t* labels_out, unsigned long long* hist256, unsigned long long* flags, void* stream) {
    if (!vol || !mask || !range2 || !q_out || !hist256 || !flags) MRISR_FAIL(MRISR_E_ARG, "f32_volume_quantise: null pointer");
    if (!aligned_to(vol, 4) || !aligned_to(range2, 4) || !aligned_to(hist256, 8) || !aligned_to(flags, 8))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_quantise: misaligned pointer");
    if (q_out == mask || labels_out == mask || (labels_out && labels_out == q_out))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_quantise: mask, q_out and labels_out must be buffers of their own");
    if (n == 0 || n > 0xffffffffull) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_quantise: %zu voxels (1..2^32 - 1)", n);
    const int vec = aligned_to(vol, 16) && aligned_to(mask, 4) && aligned_to(q_out, 4) && (!labels_out || aligned_to(labels_out, 4));
    tissue_quantise_kernel<<<capped_grid(n, kHistPerBlock, kMaxHistBlocks), 256, 0, (hipStream_t)stream>>>(vol, mask, n, vec, range2, q_out,
                                                                                                          labels_out, hist256, flags);
    MRISR_CHECK_LAUNCH("f32_volume_quantise");
    return MRISR_OK;
}

extern "C" int mrisr_u8_volume_joint_hist(const uint8_t* q, const uint8_t* labels, size_t n, int K, unsigned long long* joint, void* stream) {
    if (!q || !labels || !joint) MRISR_FAIL(MRISR_E_ARG, "u8_volume_joint_hist: null pointer");
    if (!aligned_to(joint, 8)) MRISR_FAIL(MRISR_E_ARG, "u8_volume_joint_hist: misaligned pointer");
    if (!classes_ok(K)) MRISR_FAIL(MRISR_E_ARG, "u8_volume_joint_hist: %d classes (2..%d)", K, kMaxClasses);
    if (n == 0 || n > 0xffffffffull) MRISR_FAIL(MRISR_E_SHAPE, "u8_volume_joint_hist: %zu voxels (1..2^32 - 1)", n);
    const int vec = aligned_to(q, 16) && aligned_to(labels, 16);
    tissue_joint_hist_kernel<<<capped_grid(n, kHistPerBlock, kMaxHistBlocks), 256, 0, (hipStream_t)stream>>>(q, labels, n, vec, K, joint);
    MRISR_CHECK_LAUNCH("u8_volume_joint_hist");
    return MRISR_OK;
}

extern "C" int mrisr_u8_volume_icm_half(const uint8_t* q, uint8_t* labels, int X, int Y, int Z, int K, const int* cost, int beta_q,
                                        int colour, unsigned long long* changed, void* stream) {
    if (!q || !labels || !cost || !changed) MRISR_FAIL(MRISR_E_ARG, "u8_volume_icm_half: null pointer");
    if (!aligned_to(cost, 4) || !aligned_to(changed, 8)) MRISR_FAIL(MRISR_E_ARG, "u8_volume_icm_half: misaligned pointer");
    if (q == labels) MRISR_FAIL(MRISR_E_ARG, "u8_volume_icm_half: q and labels must be two buffers");
    if (!classes_ok(K)) MRISR_FAIL(MRISR_E_ARG, "u8_volume_icm_half: %d classes (2..%d)", K, kMaxClasses);
    if (beta_q < 0 || beta_q > kMaxBetaQ) MRISR_FAIL(MRISR_E_ARG, "u8_volume_icm_half: beta_q %d (0..%d)", beta_q, kMaxBetaQ);
    if (colour != 0 && colour != 1) MRISR_FAIL(MRISR_E_ARG, "u8_volume_icm_half: colour %d (0 or 1)", colour);
    if (const int rc = check_volume_extents("u8_volume_icm_half", X, Y, Z)) return rc;
    const long long threads = (long long)X * Y * ceil_div(Z, kIcmRun);
    const long long blocks = (threads + 255) / 256;
    const int grid = (int)(blocks < kMaxIcmBlocks ? blocks : kMaxIcmBlocks);
    hipStream_t s = (hipStream_t)stream;
    if (Z % 4 == 0 && aligned_to(q, 4) && aligned_to(labels, 4))
        tissue_icm_half_kernel<true><<<grid, 256, 0, s>>>(q, labels, X, Y, Z, K, cost, beta_q, colour, changed);
    else
        tissue_icm_half_kernel<false><<<grid, 256, 0, s>>>(q, labels, X, Y, Z, K, cost, beta_q, colour, changed);
    MRISR_CHECK_LAUNCH("u8_volume_icm_half");
    return MRISR_OK;
}

extern "C" int mrisr_u8_volume_confusion(const uint8_t* a, const uint8_t* b, const uint8_t* mask, size_t n, int K, unsigned long long* conf,
                                         void* stream) {
    if (!a || !b || !conf) MRISR_FAIL(MRISR_E_ARG, "u8_volume_confusion: null pointer");
    if (!aligned_to(conf, 8)) MRISR_FAIL(MRISR_E_ARG, "u8_volume_confusion: misaligned pointer");
    if (!classes_ok(K)) MRISR_FAIL(MRISR_E_ARG, "u8_volume_confusion: %d classes (2..%d)", K, kMaxClasses);
    if (n == 0 || n > 0xffffffffull) MRISR_FAIL(MRISR_E_SHAPE, "u8_volume_confusion: %zu voxels (1..2^32 - 1)", n);
    const int vec = aligned_to(a, 16) && aligned_to(b, 16) && (!mask || aligned_to(mask, 16));
    tissue_confusion_kernel<<<capped_grid(n, kHistPerBlock, kMaxHistBlocks), 256, 0, (hipStream_t)stream>>>(a, b, mask, n, vec, K, conf);
    MRISR_CHECK_LAUNCH("u8_volume_confusion");
    return MRISR_OK;
}
