// Foreground mask of a float32 volume on the device (gfx950; extension): an exact Otsu threshold on a
// 256-bin histogram, the mask that is consistent with that histogram, and 3-D binary dilation / erosion of uint8 volumes
// (closing = erosion of the dilation).  The specification is volume_eval.foreground_mask_np; every kernel here is bit-equal
// to it.  Compiled with -ffp-contract=off (build.py): the bin of a voxel and the between-class variance restate host
// arithmetic one rounded operation at a time.
//
// A volume is (X, Y, Z) in C order, Z fastest; a mask is uint8, non-zero = foreground.
//
// Otsu mask, five launches, no host synchronisation:
//   init      clears the workspace: 256 64-bit counts, the two extrema keys.
//   extrema   lo, hi by integer atomic min / max on the order-preserving 32-bit key of the float (the map of f32_order_key in
//             volume_common.h: the trick of lowfield.hip, extended to negative values); order-independent, hence exact.
//   counts    bin(v) = min(255, int((v - lo) * scale)), scale = 256.f / (hi - lo), all float32.  A thread merges runs of
//             equal bins in a register before it touches the workgroup's 32-bit LDS histogram (RunCounter of volume_common.h:
//             background voxels come in long runs of one bin); the workgroup's non-zero bins go to the 64-bit
//             global counts with one atomic each.  A workgroup sees at most 2^45 / 2^20 + 2^14 voxels: 32 bits suffice.
//   otsu      ONE thread: exact int64 prefix sums, the between-class variance s_t in double in the order of the specification,
//             t* = the smallest t with the largest s_t; writes stats (lo, hi, t*, foreground count = N - w_t*).
//   mask      mask = bin(v) > t*: an integer comparison against the histogram's own binning, no float threshold.
// A degenerate range (hi == lo, hi - lo or scale not finite in float32) gives t* = -1 and a mask of ones.
// The input must be finite (not checked: that would cost a synchronisation); a NaN or infinity cannot make any access leave
// the histogram (the bin is clamped to 0..255 on both sides) but the result is then unspecified.
//
// Morphology (mrisr_u8_volume_morph), one pass per axis, box |d| <= r clipped to the volume (taps outside are ignored:
// the border neither grows nor erodes the mask):
//   axis 2 (z)       one workgroup stages 16 rows x (256 + halo) bytes in LDS - the body as 32-bit words where Z and the
//                    pointers allow it, the halo of r bytes either side bytewise - and every thread forms 4 consecutive outputs
//                    of a row from three LDS words and stores them as one word (bytewise in the unaligned form).
//                    LDS: ds_read_b32 / ds_write_b32 on consecutive dwords per lane, 66-dword row pitch: no bank conflicts.
//   axes 0 and 1     src and dst share the fastest axis, as the stream form of volume_blend.hip: a thread owns one 4-byte (or
//                    1-byte) column, walks kMorphRun outputs along the filtered axis with the 2r + 1 taps in a register ring
//                    (static indices) and loads kMorphRun + 2r words per kMorphRun stores.  Axis 1: [X][Y][Z]; axis 0 is the same
//                    map with one slab and columns of Y * Z.
#include "volume_common.h"

constexpr int kBins = 256;
constexpr int kHistPerBlock = 16384;       // voxels a workgroup of the counts pass takes per grid-stride step
constexpr int kMaxHistBlocks = 1 << 20;

struct OtsuWs {                            // the workspace; counts first (documented in include/mrisr.h)
    unsigned long long counts[kBins];
    unsigned key_min, key_max;
    int tstar, pad_;
};

// f32_order_key(v + 0.f) and f32_from_order_key of volume_common.h, in the XOR wording: the compiler selects other instructions
// for the two wordings, and the kernels below are kept as they were built.  v + 0.f folds -0.0 into +0.0: the two are equal to
// the specification's min / max, their keys are not.
__device__ __forceinline__ unsigned otsu_key(float v) {
    const unsigned b = __float_as_uint(v + 0.f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float otsu_unkey(unsigned k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

struct OtsuRange { float lo, scale; bool degenerate; };
__device__ __forceinline__ OtsuRange otsu_range(const OtsuWs* ws) {
    OtsuRange r;
    const float lo = otsu_unkey(ws->key_min), hi = otsu_unkey(ws->key_max);
    const float width = __fsub_rn(hi, lo);
    r.lo = lo;
    r.scale = __fdiv_rn(256.f, width);
    r.degenerate = hi == lo || !isfinite(width) || !isfinite(r.scale);
    return r;
}
__device__ __forceinline__ int otsu_bin(float v, const OtsuRange& r) {
    const int b = (int)__fmul_rn(__fsub_rn(v, r.lo), r.scale);       // truncation
    return min(kBins - 1, max(0, b));
}

__global__ void otsu_init_kernel(OtsuWs* __restrict__ ws) {
    const int t = threadIdx.x;
    if (t < kBins) ws->counts[t] = 0ull;
    if (t == 0) {
        ws->key_min = 0xffffffffu;
        ws->key_max = 0u;
        ws->tstar = -1;
        ws->pad_ = 0;
    }
}

// vec: the volume starts on 16 bytes; the n4 = n / 4 whole vectors grid-stride, the tail of n % 4 goes to block 0
__global__ __launch_bounds__(256) void otsu_extrema_kernel(const float* __restrict__ v, size_t n, int vec, OtsuWs* __restrict__ ws) {
    __shared__ unsigned smin[4], smax[4];
    unsigned kmin = 0xffffffffu, kmax = 0u;
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    if (vec) {
        const size_t n4 = n / 4;
        for (size_t i = tid; i < n4; i += stride) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(v + 4 * i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned key = otsu_key(q[k]);
                kmin = min(kmin, key);
                kmax = max(kmax, key);
            }
        }
        if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {
            const unsigned key = otsu_key(v[4 * n4 + threadIdx.x]);
            kmin = min(kmin, key);
            kmax = max(kmax, key);
        }
    } else {
        for (size_t i = tid; i < n; i += stride) {
            const unsigned key = otsu_key(v[i]);
            kmin = min(kmin, key);
            kmax = max(kmax, key);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o, 64));
        kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        smin[threadIdx.x >> 6] = kmin;
        smax[threadIdx.x >> 6] = kmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(&ws->key_min, min(min(smin[0], smin[1]), min(smin[2], smin[3])));
        atomicMax(&ws->key_max, max(max(smax[0], smax[1]), max(smax[2], smax[3])));
    }
}

__global__ __launch_bounds__(256) void otsu_counts_kernel(const float* __restrict__ v, size_t n, int vec, OtsuWs* __restrict__ ws) {
    __shared__ unsigned hist[kBins];
    const OtsuRange r = otsu_range(ws);
    if (r.degenerate) return;                                            // uniform over the grid
    hist[threadIdx.x] = 0u;
    __syncthreads();
    RunCounter run{0, 0u};
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    if (vec) {
        const size_t n4 = n / 4;
        for (size_t i = tid; i < n4; i += stride) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(v + 4 * i);
#pragma unroll
            for (int k = 0; k < 4; ++k) run.add(otsu_bin(q[k], r), hist);
        }
        if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) run.add(otsu_bin(v[4 * n4 + threadIdx.x], r), hist);
    } else {
        for (size_t i = tid; i < n; i += stride) run.add(otsu_bin(v[i], r), hist);
    }
    run.flush(hist);
    __syncthreads();
    const unsigned c = hist[threadIdx.x];
    if (c) atomicAdd(&ws->counts[threadIdx.x], (unsigned long long)c);
}

// stats: lo, hi, t*, foreground count (doubles).  One thread; nothing here is contracted (-ffp-contract=off) or reordered.
__global__ void otsu_threshold_kernel(OtsuWs* __restrict__ ws, double voxels, double* __restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const OtsuRange r = otsu_range(ws);
    int best = -1;
    double fg = voxels;
    if (!r.degenerate) {
        long long N = 0, M = 0;
        for (int k = 0; k < kBins; ++k) {
            N += (long long)ws->counts[k];
            M += (long long)k * (long long)ws->counts[k];
        }
        long long w = 0, m = 0, wbest = 0;
        double sbest = -1.0;                                             // every s_t is >= 0
        for (int t = 0; t < kBins - 1; ++t) {
            w += (long long)ws->counts[t];
            m += (long long)t * (long long)ws->counts[t];
            if (w <= 0 || w >= N) continue;
            const double mu0 = __ddiv_rn((double)m, (double)w);
            const double mu1 = __ddiv_rn((double)(M - m), (double)(N - w));
            const double d = __dsub_rn(mu1, mu0);
            const double s = __dmul_rn(__dmul_rn((double)w, (double)(N - w)), __dmul_rn(d, d));
            if (s > sbest) {
                sbest = s;
                best = t;
                wbest = w;
            }
        }
        // hi != lo puts voxels in bin 0 and in bin 255, so at least t = 0 qualified
        fg = (double)(N - wbest);
    }
    ws->tstar = best;
    stats[0] = (double)otsu_unkey(ws->key_min);
    stats[1] = (double)otsu_unkey(ws->key_max);
    stats[2] = (double)best;
    stats[3] = fg;
}

__global__ __launch_bounds__(256) void otsu_mask_kernel(const float* __restrict__ v, size_t n, int vec, const OtsuWs* __restrict__ ws,
                                                        uint8_t* __restrict__ mask) {
    const OtsuRange r = otsu_range(ws);
    const int tstar = ws->tstar;
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    auto bit = [&](float x) -> unsigned { return r.degenerate ? 1u : (otsu_bin(x, r) > tstar ? 1u : 0u); };
    if (vec) {                                                            // v on 16 bytes and mask on 4
        const size_t n4 = n / 4;
        for (size_t i = tid; i < n4; i += stride) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(v + 4 * i);
            *reinterpret_cast<unsigned*>(mask + 4 * i) = bit(q[0]) | bit(q[1]) << 8 | bit(q[2]) << 16 | bit(q[3]) << 24;
        }
        if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) mask[4 * n4 + threadIdx.x] = (uint8_t)bit(v[4 * n4 + threadIdx.x]);
    } else {
        for (size_t i = tid; i < n; i += stride) mask[i] = (uint8_t)bit(v[i]);
    }
}

extern "C" size_t mrisr_f32_volume_otsu_workspace_bytes(void) { return sizeof(OtsuWs); }

extern "C" int mrisr_f32_volume_otsu_mask(const float* vol, int X, int Y, int Z, uint8_t* mask_out, double* stats, void* workspace,
                                          void* stream) {
    if (!vol || !mask_out || !stats || !workspace) MRISR_FAIL(MRISR_E_ARG, "f32_volume_otsu_mask: null pointer");
    if (!aligned_to(vol, 4) || !aligned_to(stats, 8) || !aligned_to(workspace, 8))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_otsu_mask: misaligned pointer");
    if (const int rc = check_volume_extents("f32_volume_otsu_mask", X, Y, Z)) return rc;
    const size_t n = (size_t)X * Y * Z;
    OtsuWs* ws = (OtsuWs*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const int grid = capped_grid(n, kHistPerBlock, kMaxHistBlocks);
    const int vec_in = aligned_to(vol, 16) ? 1 : 0, vec_out = vec_in && aligned_to(mask_out, 4) ? 1 : 0;
    otsu_init_kernel<<<1, 256, 0, s>>>(ws);
    MRISR_CHECK_LAUNCH("f32_volume_otsu_mask (init)");
    otsu_extrema_kernel<<<grid, 256, 0, s>>>(vol, n, vec_in, ws);
    MRISR_CHECK_LAUNCH("f32_volume_otsu_mask (extrema)");
    otsu_counts_kernel<<<grid, 256, 0, s>>>(vol, n, vec_in, ws);
    MRISR_CHECK_LAUNCH("f32_volume_otsu_mask (counts)");
    otsu_threshold_kernel<<<1, 64, 0, s>>>(ws, (double)X * (double)Y * (double)Z, stats);
    MRISR_CHECK_LAUNCH("f32_volume_otsu_mask (threshold)");
    otsu_mask_kernel<<<grid, 256, 0, s>>>(vol, n, vec_out, ws, mask_out);
    MRISR_CHECK_LAUNCH("f32_volume_otsu_mask (mask)");
    return MRISR_OK;
}

// ---------------------------------------------------------------- morphology

constexpr int kMorphRun = 16;              // outputs a thread of the stream form walks
constexpr int kMorphRows = 16;             // z form: rows per workgroup
constexpr int kMorphTZ = 256;              // z form: body bytes per row and workgroup
constexpr int kMorphPitch = kMorphTZ / 4 + 2;      // dwords: 4 halo bytes, the body, 4 halo bytes

template <bool MIN> __device__ __forceinline__ unsigned morph_op(unsigned a, unsigned b) { return MIN ? min(a, b) : max(a, b); }
template <bool MIN> __device__ __forceinline__ unsigned morph_op4(unsigned a, unsigned b) {      // bytewise
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) r |= morph_op<MIN>((a >> 8 * k) & 255u, (b >> 8 * k) & 255u) << 8 * k;
    return r;
}
template <bool MIN, typename V> __device__ __forceinline__ V morph_combine(V a, V b) {
    if constexpr (sizeof(V) == 4) return morph_op4<MIN>(a, b);
    else return (V)morph_op<MIN>(a, b);
}

// [A][S][CV] in units of V (4 bytes or 1); thread = one column of one slab, grid z (strided) over runs of kMorphRun outputs
template <int R, bool MIN, typename V>
__global__ __launch_bounds__(256) void morph_stream_kernel(const V* __restrict__ src, V* __restrict__ dst, int A, int S, int CV) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)A * CV) return;
    const int a = (int)(idx / CV), cv = (int)(idx - (long long)a * CV);
    const V ident = MIN ? (V)~(V)0 : (V)0;                               // a tap outside the volume is ignored
    const size_t base = (size_t)a * S * CV + cv;
    auto tap = [&](int s) -> V { return s >= 0 && s < S ? src[base + (size_t)s * CV] : ident; };
    for (int s0 = blockIdx.z * kMorphRun; s0 < S; s0 += gridDim.z * kMorphRun) {
        const int s1 = s0 + kMorphRun < S ? s0 + kMorphRun : S;
        V win[2 * R + 1];
#pragma unroll
        for (int j = 0; j < 2 * R; ++j) win[j + 1] = tap(s0 - R + j);
        for (int s = s0; s < s1; ++s) {
#pragma unroll
            for (int j = 0; j < 2 * R; ++j) win[j] = win[j + 1];
            win[2 * R] = tap(s + R);
            V m = win[0];
#pragma unroll
            for (int j = 1; j <= 2 * R; ++j) m = morph_combine<MIN, V>(m, win[j]);
            dst[base + (size_t)s * CV] = m;
        }
    }
}

// rows of Z bytes; grid (row blocks, z tiles); vec: Z % 4 == 0 and both pointers on 4 bytes
template <int R, bool MIN>
__global__ __launch_bounds__(256) void morph_z_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long rows, int Z,
                                                      int vec) {
    __shared__ unsigned tile[kMorphRows * kMorphPitch];
    uint8_t* tb = reinterpret_cast<uint8_t*>(tile);
    const int t = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * kMorphRows;
    const int z0 = blockIdx.y * kMorphTZ;
    const unsigned ident = MIN ? 255u : 0u;
    // body: 16 rows x 64 words
    for (int e = t; e < kMorphRows * (kMorphTZ / 4); e += 256) {
        const int r = e >> 6, w = e & 63;
        const long long row = row0 + r;
        const int z = z0 + 4 * w;
        unsigned word = ident * 0x01010101u;
        if (row < rows && z < Z) {
            const uint8_t* p = src + (size_t)row * Z + z;
            if (vec) {
                word = *reinterpret_cast<const unsigned*>(p);            // Z % 4 == 0: the whole word is inside the row
            } else {
                word = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) word |= (z + k < Z ? (unsigned)p[k] : ident) << 8 * k;
            }
        }
        tile[r * kMorphPitch + 1 + w] = word;
    }
    // halo: R bytes either side of the body
    for (int e = t; e < kMorphRows * 2 * R; e += 256) {
        const int r = e / (2 * R), k = e - r * 2 * R;
        const long long row = row0 + r;
        const int c = k < R ? 4 - R + k : 4 + kMorphTZ + (k - R);           // byte column of the LDS row
        const int z = z0 + c - 4;
        tb[r * kMorphPitch * 4 + c] = (uint8_t)(row < rows && z >= 0 && z < Z ? (unsigned)src[(size_t)row * Z + z] : ident);
    }
    __syncthreads();
    for (int e = t; e < kMorphRows * (kMorphTZ / 4); e += 256) {
        const int r = e >> 6, w = e & 63;
        const long long row = row0 + r;
        const int z = z0 + 4 * w;
        if (row >= rows || z >= Z) continue;
        const unsigned q0 = tile[r * kMorphPitch + w], q1 = tile[r * kMorphPitch + w + 1], q2 = tile[r * kMorphPitch + w + 2];
        unsigned b[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b[k] = (q0 >> 8 * k) & 255u;
            b[4 + k] = (q1 >> 8 * k) & 255u;
            b[8 + k] = (q2 >> 8 * k) & 255u;
        }
        unsigned out = 0;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            unsigned m = b[4 + o - R];
#pragma unroll
            for (int j = 1; j <= 2 * R; ++j) m = morph_op<MIN>(m, b[4 + o - R + j]);
            out |= m << 8 * o;
        }
        uint8_t* p = dst + (size_t)row * Z + z;
        if (vec) {
            *reinterpret_cast<unsigned*>(p) = out;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (z + k < Z) p[k] = (uint8_t)(out >> 8 * k);
        }
    }
}

template <int R, bool MIN>
static int morph_passes(const uint8_t* src, int X, int Y, int Z, uint8_t* dst, uint8_t* tmp, hipStream_t s) {
    // z: src -> dst
    {
        const long long rows = (long long)X * Y;
        const int vec = Z % 4 == 0 && aligned_to(src, 4) && aligned_to(dst, 4);
        const dim3 grid((unsigned)((rows + kMorphRows - 1) / kMorphRows), ceil_div(Z, kMorphTZ));
        morph_z_kernel<R, MIN><<<grid, 256, 0, s>>>(src, dst, rows, Z, vec);
        MRISR_CHECK_LAUNCH("u8_volume_morph (z pass)");
    }
    // y: dst -> tmp ([X][Y][Z]), x: tmp -> dst (one slab, columns of Y * Z)
    auto stream_pass = [&](const char* name, const uint8_t* in, uint8_t* out, int A, int S, long long C) -> int {
        const bool vec = C % 4 == 0 && aligned_to(in, 4) && aligned_to(out, 4);
        const int CV = (int)(vec ? C / 4 : C);                           // Y * Z < 2^30
        const long long threads = (long long)A * CV;                    // X * Z < 2^30
        const int runs = ceil_div(S, kMorphRun);
        const dim3 grid((unsigned)((threads + 255) / 256), 1, runs < 65535 ? runs : 65535);
        if (vec) morph_stream_kernel<R, MIN, unsigned><<<grid, 256, 0, s>>>((const unsigned*)in, (unsigned*)out, A, S, CV);
        else morph_stream_kernel<R, MIN, uint8_t><<<grid, 256, 0, s>>>(in, out, A, S, CV);
        MRISR_CHECK_LAUNCH(name);
        return MRISR_OK;
    };
    const int rc = stream_pass("u8_volume_morph (y pass)", dst, tmp, X, Y, Z);
    return rc != MRISR_OK ? rc : stream_pass("u8_volume_morph (x pass)", tmp, dst, 1, X, (long long)Y * Z);
}

extern "C" int mrisr_u8_volume_morph(const uint8_t* src, int X, int Y, int Z, int radius, int op, uint8_t* dst, uint8_t* tmp,
                                     void* stream) {
    if (!src || !dst || (radius != 0 && !tmp)) MRISR_FAIL(MRISR_E_ARG, "u8_volume_morph: null pointer");
    if (src == dst || src == tmp || dst == tmp) MRISR_FAIL(MRISR_E_ARG, "u8_volume_morph: src, dst and tmp must be three buffers");
    if (op != MRISR_MORPH_DILATE && op != MRISR_MORPH_ERODE) MRISR_FAIL(MRISR_E_ARG, "u8_volume_morph: op %d", op);
    if (const int rc = check_volume_extents("u8_volume_morph", X, Y, Z)) return rc;
    if (radius < 0 || radius > 4) MRISR_FAIL(MRISR_E_SHAPE, "u8_volume_morph: radius %d (0..4)", radius);
    hipStream_t s = (hipStream_t)stream;
    const bool mn = op == MRISR_MORPH_ERODE;
    if (radius == 0) {
        if (hipMemcpyAsync(dst, src, (size_t)X * Y * Z, hipMemcpyDeviceToDevice, s) != hipSuccess)
            MRISR_FAIL(MRISR_E_HIP, "u8_volume_morph: copy failed");
        return MRISR_OK;
    }
#define MRISR_CALL(R) (mn ? morph_passes<R, true>(src, X, Y, Z, dst, tmp, s) : morph_passes<R, false>(src, X, Y, Z, dst, tmp, s))
    switch (radius) {                                                    // every launch is checked where it is made
        case 1: return MRISR_CALL(1);
        case 2: return MRISR_CALL(2);
        case 3: return MRISR_CALL(3);
        default: return MRISR_CALL(4);
    }
#undef MRISR_CALL
}
