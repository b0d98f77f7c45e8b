// Gibbs-ringing removal of volumes by local subvoxel shifts (extension; Kellner et al., MRM 2016) along one
// axis, fused: no shifted line ever reaches memory.  The specification is mri_superresolution_amd/volume_unring.py (unring_axis_np);
// the tables come from the host (shift_table, shift_fractions: float64, rounded once) and no cosine is evaluated here.
//
//   candidate 0     f = v
//   candidate m     f[i] = sum_j S_m[(i - j) mod n] v[j]                 the line re-sampled at i + s_m; 2K of them, in table order
//   TVL[i], TVR[i]  0 + sum_{k = a..b} |f[i - k] - f[i - k - 1]|,  0 + sum_{k = a..b} |f[i + k] - f[i + k + 1]|     indices modulo n
//   value at i      v[i];  s > 0: f[i] - (f[i] - f[i - 1]) s;  s < 0: f[i] + (f[i] - f[i + 1]) s
//   selection       best = TVL of candidate 0, then TVR of candidate 0, then TVL, TVR of every m: a visit wins only if tv < best
//
// Every sum is  0 + t_0 + t_1 + ...  in the stated order, each product, difference and sum rounded to float32 (this file is compiled
// with -ffp-contract=off and the operations are written as __fmul_rn / __fadd_rn / __fsub_rn).  The blocking is over outputs, never
// over j or k, so no sum's order depends on the launch shape.
//
// A workgroup takes a bundle of W lines in the three addressing forms of csrc/volume_kspace.hip (axes 0 and 1: neighbours along axis
// 2; axis 2: W consecutive rows through LDS transposed).  LDS holds the W source lines and the W lines of the current candidate
// (sample j of line c at tile[j (W + 1) + c]) and two unrolled table rows E[x] = row[(x + 1) mod n]: the row of candidate m + 1 is
// fetched while candidate m is judged.  Thread (c, q) owns the outputs  i = chunk CH + q R + r  of line c (R = 8, at most 4 chunks) and
// keeps their (best, value) in registers.  Per candidate: the register-blocked circulant sum of volume_kspace.hip into the second
// tile, a barrier, then |diff|, the two windowed sums and the candidate value of the thread's own outputs from that tile, a barrier.
// No atomics; apart from the two selects nothing in the control flow depends on the data.
#include "volume_common.h"

namespace {

constexpr int kUnringMinLine = 8, kUnringMaxLine = 512;
constexpr int kUnringMaxShifts = 32;       // K: 2K candidates besides the line itself
constexpr int kUnringMaxWindow = 4;        // 1 <= a <= b <= 4
constexpr int kUnringR = 8;                // outputs per thread and chunk
constexpr int kUnringChunks = 4;           // chunks per line at the longest line of every bundle width
constexpr long long kUnringMaxVoxels = 2147483647LL;

template <int W> struct UnringLayout {
    static constexpr int P = W + 1, Q = 256 / W, CH = Q * kUnringR;     // tile pitch; threads per line; outputs per chunk
    static constexpr int MAX_N = CH * kUnringChunks;                     // the longest line of this bundle width
    static constexpr int WIN = 2 * kUnringR - 1;                         // table entries a block of R source samples needs
    __host__ __device__ static constexpr int ext(int n) { return 2 * n + 2 * kUnringR; }          // floats of one unrolled row
    __host__ __device__ static constexpr size_t floats(int n) { return 2 * (size_t)ext(n) + 2 * (size_t)n * P; }
};

// |f[t] - f[t + 1]| of the window around the outputs i0 .. i0 + R - 1 of one line, then both sums and the select.  f: the line
// in LDS at pitch P; D[u] belongs to t = i0 - (B + 1) + u with B = kUnringMaxWindow.
template <int P>
__device__ __forceinline__ void unring_judge(const float* __restrict__ f, int n, int i0, int a, int b, float s, bool first,
                                             const float* __restrict__ v, float* best, float* value) {
    constexpr int R = kUnringR, B = kUnringMaxWindow, NF = R + 2 * B + 2, ND = NF - 1;
    float g[NF], D[ND];
    int t = i0 - (B + 1);                                    // >= -5 > -n
    t = t < 0 ? t + n : t;
#pragma unroll
    for (int u = 0; u < NF; ++u) {
        g[u] = f[t * P];
        t = t + 1 == n ? 0 : t + 1;
    }
#pragma unroll
    for (int u = 0; u < ND; ++u) D[u] = fabsf(__fsub_rn(g[u], g[u + 1]));
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int at = r + B + 1;                            // g[at] = f[i], D[at] = |f[i] - f[i + 1]|
        float tvl = 0.f, tvr = 0.f;
#pragma unroll
        for (int k = 1; k <= B; ++k) {
            if (k >= a && k <= b) {
                tvl = __fadd_rn(tvl, D[at - k - 1]);
                tvr = __fadd_rn(tvr, D[at + k]);
            }
        }
        float val;
        if (first) val = v[r];
        else if (s > 0.f) val = __fsub_rn(g[at], __fmul_rn(__fsub_rn(g[at], g[at - 1]), s));
        else val = __fadd_rn(g[at], __fmul_rn(__fsub_rn(g[at], g[at + 1]), s));
        if (first) {
            best[r] = tvl;
            value[r] = val;
        } else if (tvl < best[r]) {
            best[r] = tvl;
            value[r] = val;
        }
        if (tvr < best[r]) {
            best[r] = tvr;
            value[r] = val;
        }
    }
}

// axes 0, 1: line position j of column m (< M) of outer index o lies at src[o * outer_stride + j * line_stride + m]; workgroup
// blockIdx.x = o * ceil(M / W) + m / W.  axis 2: line_stride = 1, M = the number of rows, workgroup b takes the rows b W ... b W + W - 1.
template <int W, bool AXIS2>
__global__ __launch_bounds__(256) void unring_kernel(const float* __restrict__ src, const float* __restrict__ table,
                                                     const float* __restrict__ fractions, float* __restrict__ dst, int n, int shifts,
                                                     int win_lo, int win_hi, size_t line_stride, long long M, size_t outer_stride) {
    using Lay = UnringLayout<W>;
    constexpr int P = Lay::P, Q = Lay::Q, R = kUnringR, CH = Lay::CH, WIN = Lay::WIN, NC = kUnringChunks;
    extern __shared__ float lds[];
    const int ext = Lay::ext(n);
    float* E = lds;                                          // two unrolled rows
    float* tile = lds + 2 * ext;                             // the source lines
    float* cand = tile + (size_t)n * P;                      // the lines of the current candidate; at the end the result
    const int tid = threadIdx.x, c = tid % W, q = tid / W;

    // E[x] = row[(x + 1) mod n]: every index the loops below form lies in [0, ext)
    for (int x = tid; x < ext; x += 256) E[x] = table[(x + 1) % n];

    bool in = false;
    float* out_base = dst;
    long long row0 = 0;
    if (AXIS2) {
        row0 = (long long)blockIdx.x * W;
        const long long left = M - row0;                     // rows of this bundle that exist (>= 1)
        const size_t total = (size_t)W * n, have = (size_t)(left < W ? left : W) * n;
        const float* base = src + (size_t)row0 * n;
        for (size_t e = tid; e < total; e += 256) {
            const int row = (int)(e / n), j = (int)(e - (size_t)row * n);
            tile[j * P + row] = e < have ? base[e] : 0.f;
        }
    } else {
        const long long chunks = (M + W - 1) / W;
        const long long o = blockIdx.x / chunks, m = (blockIdx.x - o * chunks) * W + c;
        in = m < M;
        const float* base = src + (size_t)o * outer_stride + (size_t)(in ? m : 0);
        for (int j = q; j < n; j += Q) tile[j * P + c] = in ? base[(size_t)j * line_stride] : 0.f;
        out_base = dst + (size_t)o * outer_stride + (size_t)(in ? m : 0);
    }
    __syncthreads();

    // candidate 0: the line itself
    float best[NC][R], value[NC][R];
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
        const int i0 = ch * CH + q * R;
        const int ic = i0 < n ? i0 : 0;                      // a thread past the end works on output 0 and keeps nothing
        float v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = ic + r;
            v[r] = tile[(i < n ? i : i - n) * P + c];
        }
        if (ch * CH < n) unring_judge<P>(tile + c, n, ic, win_lo, win_hi, 0.f, true, v, best[ch], value[ch]);
    }

    const float* col = tile + c;
    const int full = n - n % R;                              // source samples taken in blocks of R
    for (int mi = 0; mi < 2 * shifts; ++mi) {
        const float* E0 = E + (mi & 1) * ext;
        // f_m of the thread's own outputs into cand (the judging of candidate mi - 1 ended at the barrier below); a loop, not
        // unrolled: only the judging needs its chunk as a constant, for the registers of (best, value)
#pragma unroll 1
        for (int cb = 0; cb < n; cb += CH) {
            {
                const int i0 = cb + q * R;
                const int ic = i0 < n ? i0 : 0;
                const int x0 = ic + n - 1;                   // the table index of output ic at j = 0
                float acc[R];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = 0.f;
                for (int j0 = 0; j0 < full; j0 += R) {
                    // output ic + r at source sample j0 + u reads E[xb + r - u + R - 1]
                    const int xb = x0 - j0 - (R - 1);
                    float w[WIN];
#pragma unroll
                    for (int k = 0; k < WIN; ++k) w[k] = E0[xb + k];
#pragma unroll
                    for (int u = 0; u < R; ++u) {
                        const float v = col[(j0 + u) * P];
#pragma unroll
                        for (int r = 0; r < R; ++r) acc[r] = __fadd_rn(acc[r], __fmul_rn(w[r - u + R - 1], v));
                    }
                }
                for (int j = full; j < n; ++j) {             // the last n mod R source samples, one at a time
                    const float v = col[j * P];
                    const int x = x0 - j;
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r] = __fadd_rn(acc[r], __fmul_rn(E0[x + r], v));
                }
                if (i0 < n) {
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (i0 + r < n) cand[(i0 + r) * P + c] = acc[r];
                }
            }
        }
        __syncthreads();
        // the next row, while this candidate is judged: its buffer was last read before the barrier above
        if (mi + 1 < 2 * shifts) {
            float* E1 = E + ((mi + 1) & 1) * ext;
            const float* row = table + (size_t)(mi + 1) * n;
            for (int x = tid; x < ext; x += 256) E1[x] = row[(x + 1) % n];
        }
        const float s = fractions[mi];
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            const int i0 = ch * CH + q * R;
            if (ch * CH < n) unring_judge<P>(cand + c, n, i0 < n ? i0 : 0, win_lo, win_hi, s, false, nullptr, best[ch], value[ch]);
        }
        __syncthreads();
    }

    if (AXIS2) {
        // through LDS, so that a row's outputs leave in order
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            const int i0 = ch * CH + q * R;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (i0 + r < n) cand[(i0 + r) * P + c] = value[ch][r];
        }
        __syncthreads();
        const long long left = M - row0;
        const size_t have = (size_t)(left < W ? left : W) * n;
        float* base = dst + (size_t)row0 * n;
        for (size_t e = tid; e < have; e += 256) {
            const int row = (int)(e / n), j = (int)(e - (size_t)row * n);
            base[e] = cand[j * P + row];
        }
    } else if (in) {
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            const int i0 = ch * CH + q * R;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (i0 + r < n) out_base[(size_t)(i0 + r) * line_stride] = value[ch][r];
        }
    }
}

template <int W, bool AXIS2>
static int launch_unring(const float* src, const float* table, const float* fractions, float* dst, int n, int shifts, int win_lo,
                         int win_hi, size_t line_stride, long long M, long long outer, size_t outer_stride, hipStream_t s) {
    static_assert(UnringLayout<W>::MAX_N * W == 8192 && UnringLayout<W>::floats(UnringLayout<W>::MAX_N) * sizeof(float) <= 80 * 1024,
                  "unring_kernel: two workgroups per CU inside 160 KB of LDS");
    const long long bundles = outer * ((M + W - 1) / W);     // at most the voxel count: inside int
    const size_t lds = UnringLayout<W>::floats(n) * sizeof(float);
    // a tile past the default 64 KB needs the limit raised on the CURRENT device: asked for at every such launch (a host-side
    // attribute, not a stream operation)
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(unring_kernel<W, AXIS2>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024) != hipSuccess)
        MRISR_FAIL(MRISR_E_HIP, "f32_volume_unring_axis: cannot raise the LDS limit");
    unring_kernel<W, AXIS2><<<(unsigned)bundles, 256, lds, s>>>(src, table, fractions, dst, n, shifts, win_lo, win_hi, line_stride, M,
                                                               outer_stride);
    return MRISR_OK;
}

// the bundle width by the line's length: W n <= 8192, so both tiles stay below 70 KB and two workgroups share a CU
template <bool AXIS2>
static int pick_unring(const float* src, const float* table, const float* fractions, float* dst, int n, int shifts, int win_lo, int win_hi,
                       size_t line_stride, long long M, long long outer, size_t outer_stride, hipStream_t s) {
    if (n <= 128) return launch_unring<64, AXIS2>(src, table, fractions, dst, n, shifts, win_lo, win_hi, line_stride, M, outer, outer_stride, s);
    if (n <= 256) return launch_unring<32, AXIS2>(src, table, fractions, dst, n, shifts, win_lo, win_hi, line_stride, M, outer, outer_stride, s);
    return launch_unring<16, AXIS2>(src, table, fractions, dst, n, shifts, win_lo, win_hi, line_stride, M, outer, outer_stride, s);
}

}  // namespace

extern "C" int mrisr_f32_volume_unring_axis(const float* src, int X, int Y, int Z, int axis, int K, int win_lo, int win_hi,
                                            const float* table, const float* fractions, float* dst, void* stream) {
    if (!src || !table || !fractions || !dst) MRISR_FAIL(MRISR_E_ARG, "f32_volume_unring_axis: null pointer");
    if (!aligned_to(src, 4) || !aligned_to(table, 4) || !aligned_to(fractions, 4) || !aligned_to(dst, 4))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_unring_axis: misaligned pointer");
    if (axis < 0 || axis > 2) MRISR_FAIL(MRISR_E_ARG, "f32_volume_unring_axis: axis %d (0..2)", axis);
    if (K < 1 || K > kUnringMaxShifts) MRISR_FAIL(MRISR_E_ARG, "f32_volume_unring_axis: K = %d shifts (1..%d)", K, kUnringMaxShifts);
    if (win_lo < 1 || win_lo > win_hi || win_hi > kUnringMaxWindow)
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_unring_axis: window %d..%d (1 <= lo <= hi <= %d)", win_lo, win_hi, kUnringMaxWindow);
    if (const int rc = check_volume_extents("f32_volume_unring_axis", X, Y, Z)) return rc;
    const int n = axis == 0 ? X : (axis == 1 ? Y : Z);
    if (n < kUnringMinLine || n > kUnringMaxLine)
        MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_unring_axis: a line of %d samples (%d..%d)", n, kUnringMinLine, kUnringMaxLine);
    const long long voxels = (long long)X * Y * Z;
    if (voxels > kUnringMaxVoxels) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_unring_axis: more than 2^31 - 1 voxels");
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst, bytes = (uintptr_t)voxels * sizeof(float);
    if ((a <= b ? b - a : a - b) < bytes) MRISR_FAIL(MRISR_E_ARG, "f32_volume_unring_axis: src and dst overlap");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (axis == 2) rc = pick_unring<true>(src, table, fractions, dst, n, K, win_lo, win_hi, 1, (long long)X * Y, 1, 0, s);
    else if (axis == 1) rc = pick_unring<false>(src, table, fractions, dst, n, K, win_lo, win_hi, (size_t)Z, Z, X, (size_t)Y * Z, s);
    else rc = pick_unring<false>(src, table, fractions, dst, n, K, win_lo, win_hi, (size_t)Y * Z, (long long)Y * Z, 1, 0, s);
    if (rc != MRISR_OK) return rc;
    MRISR_CHECK_LAUNCH("f32_volume_unring_axis");
    return MRISR_OK;
}
