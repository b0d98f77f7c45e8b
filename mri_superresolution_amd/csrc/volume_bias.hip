// Bias-field matching between scans on the device (gfx950; extension): the masked Gaussian low-pass of a
// volume and the field formed from one or two of them.  The specification is volume_bias.smooth_masked_np / match_bias_np /
// correct_bias_np; every kernel here is bit-equal to it.  Compiled with -ffp-contract=off (build.py): a tap is a rounded product,
// then a rounded sum, and the taps of a voxel are added in ascending order - never an fma, never partial sums.
//
// A volume is (X, Y, Z) in C order, Z fastest.  Two channels go through every pass together: a = the voxels that count (inside
// the mask, or both masks, and not NaN; else 0) and b = that predicate as 0 / 1.  Neither exists in memory before the first pass.
//
//   f32_volume_smooth_masked   three launches, axis 2, then 1, then 0.
//     z pass       rows of Z floats.  A workgroup stages kZRows row segments of kZTile outputs plus the halo (the radius rounded
//                  up to whole 16-byte quads) of both channels in LDS, forming a and b from the volume and the mask bytes as it
//                  loads; a thread then owns 4 consecutive outputs of a row and walks the quads of its window: two ds_read_b128
//                  (consecutive lanes, consecutive 16 bytes: conflict-free) and one broadcast ds_read_b128 of taps per quad,
//                  for 16 products and 16 sums per channel.
//     y, x passes  the stream form of volume_blend.hip / volume_mask.hip: src and dst share the fastest axis; a thread owns one
//                  16-byte column and P consecutive outputs along the filtered axis, a workgroup stages a
//                  (32 P + 2 R) x 8 column tile of both channels in LDS.  P in {4, 2, 1} is chosen at launch from R so that the
//                  tile and the taps stay inside 80 KB: two workgroups per CU up to R = 128.  Axis 1: [X][Y][Z]; axis 0 is the
//                  same map with one slab and columns of Y * Z.
//     In every pass the taps are loaded into LDS once per workgroup, an element outside the volume is staged as 0 (adding the
//     +0 of its product never changes a sum that starts at +0), and only the first and last taps of a window - where the
//     thread's outputs see different tap ranges - are guarded one by one.
//   f32_volume_bias_apply      one elementwise launch: the low-pass L = num / den where den >= 1e-3f, the field of the pair
//                              (L_ref / L_src) or of one scan (L / p50, p50 a device scalar), clamped, and the corrected volume.
#include "volume_common.h"

constexpr int kMaxRadius = 128;
constexpr int kZRows = 4;                  // z pass: rows per workgroup
constexpr int kZTile = 256;                // z pass: outputs per row and workgroup (4 per thread of a wave)
constexpr int kColQuads = 8;               // stream pass: 16-byte columns per workgroup (128 B of a tile row per channel)
constexpr int kSGroups = 256 / kColQuads;  // stream pass: threads along the filtered axis
constexpr size_t kStreamLdsMax = 80 * 1024;
#define MRISR_DEN_MIN 1e-3f

static inline int round_up4(int r) { return (r + 3) & ~3; }
static inline size_t z_pass_lds(int R) { return ((size_t)2 * kZRows * (kZTile + 2 * round_up4(R)) + 2 * round_up4(R) + 8) * sizeof(float); }
static inline size_t stream_pass_lds(int R, int P) {
    return (size_t)2 * (kSGroups * P + 2 * R) * kColQuads * sizeof(f32x4) + (size_t)(2 * R + P) * sizeof(float);
}

// rows of Z floats; grid (row blocks, z tiles).  vec_in: Z % 4 == 0, vol on 16 bytes, the masks on 4; vec_out: Z % 4 == 0, both
// outputs on 16 bytes.
__global__ __launch_bounds__(256) void smooth_z_kernel(const float* __restrict__ vol, const uint8_t* __restrict__ mask,
                                                       const uint8_t* __restrict__ mask2, float* __restrict__ outa,
                                                       float* __restrict__ outb, long long rows, int Z, const float* __restrict__ taps,
                                                       int R, int vec_in, int vec_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Rp = (R + 3) & ~3, d = Rp - R;
    const int Lt = kZTile + 2 * Rp;                    // floats of a staged row, a multiple of 4; position q is z0 - Rp + q
    float* ta = lds;
    float* tb = ta + kZRows * Lt;
    float* wl = tb + kZRows * Lt;                      // [2 Rp + 8]: wl[e] = w[e - 4 - d], 0 outside the taps
    const int t = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * kZRows;
    const int z0 = blockIdx.y * kZTile;
    for (int e = t; e < 2 * Rp + 8; e += 256) {
        const int idx = e - 4 - d;
        wl[e] = idx >= 0 && idx <= 2 * R ? taps[idx] : 0.f;
    }
    const int quads = Lt / 4;
    for (int e = t; e < kZRows * quads; e += 256) {
        const int r = e / quads, qq = e - r * quads;
        const long long row = row0 + r;
        const int z = z0 - Rp + 4 * qq;
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (row < rows && z + 3 >= 0 && z < Z) {
            const size_t off = (size_t)row * Z + z;        // of element z; only the elements inside the row are touched
            if (vec_in) {                                  // z % 4 == 0 and Z % 4 == 0: the quad is inside the row
                const f32x4 v = *reinterpret_cast<const f32x4*>(vol + off);
                unsigned m4 = *reinterpret_cast<const unsigned*>(mask + off);
                const unsigned n4 = mask2 ? *reinterpret_cast<const unsigned*>(mask2 + off) : 0x01010101u;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool keep = ((m4 >> 8 * k) & 255u) && ((n4 >> 8 * k) & 255u) && v[k] == v[k];
                    a[k] = keep ? v[k] : 0.f;
                    b[k] = keep ? 1.f : 0.f;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (z + k < 0 || z + k >= Z) continue;
                    const float v = vol[off + k];
                    const bool keep = mask[off + k] && (!mask2 || mask2[off + k]) && v == v;
                    a[k] = keep ? v : 0.f;
                    b[k] = keep ? 1.f : 0.f;
                }
            }
        }
        *reinterpret_cast<f32x4*>(ta + r * Lt + 4 * qq) = a;
        *reinterpret_cast<f32x4*>(tb + r * Lt + 4 * qq) = b;
    }
    __syncthreads();
    const int u = t & 63, r = t >> 6;
    const long long row = row0 + r;
    const int zo = z0 + 4 * u;
    if (row >= rows || zo >= Z) return;
    const float* pa = ta + r * Lt + 4 * u;
    const float* pb = tb + r * Lt + 4 * u;
    f32x4 acca = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};      // element j: the output zo + j
    float wv[8];                                                           // wv[4 + i - j]: the tap of position i for output j
    {
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(wl);
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[4 + k] = w0[k];
    }
    const int M = Rp / 2 + 1;                                              // quads of the window: positions 4 u .. 4 u + 2 Rp + 3
    for (int m = 0; m < M; ++m) {
        const f32x4 xa = *reinterpret_cast<const f32x4*>(pa + 4 * m);
        const f32x4 xb = *reinterpret_cast<const f32x4*>(pb + 4 * m);
        const f32x4 wn = *reinterpret_cast<const f32x4*>(wl + 4 * m + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            wv[k] = wv[4 + k];
            wv[4 + k] = wn[k];
        }
        const int first = 4 * m - d;                                       // tap index of (i, j) is first + i - j
        if (first - 3 >= 0 && first + 3 <= 2 * R) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acca[j] = acca[j] + wv[4 + i - j] * xa[i];
                    accb[j] = accb[j] + wv[4 + i - j] * xb[i];
                }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int idx = first + i - j;
                    if (idx < 0 || idx > 2 * R) continue;
                    acca[j] = acca[j] + wv[4 + i - j] * xa[i];
                    accb[j] = accb[j] + wv[4 + i - j] * xb[i];
                }
        }
    }
    const size_t off = (size_t)row * Z + zo;
    if (vec_out) {
        *reinterpret_cast<f32x4*>(outa + off) = acca;
        *reinterpret_cast<f32x4*>(outb + off) = accb;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (zo + k < Z) {
                outa[off + k] = acca[k];
                outb[off + k] = accb[k];
            }
    }
}

// [A][S][C] floats, the filter along S; grid (column groups of 32 floats, tiles of 32 P outputs, A).  vec: C % 4 == 0 and all four
// pointers on 16 bytes.
template <int P>
__global__ __launch_bounds__(256) void smooth_stream_kernel(const float* __restrict__ ina, const float* __restrict__ inb,
                                                            float* __restrict__ outa, float* __restrict__ outb, int S, long long C,
                                                            const float* __restrict__ taps, int R, int vec) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int T = kSGroups * P;
    const int tile_rows = T + 2 * R;                   // tile row q is s0 - R + q
    f32x4* ta = reinterpret_cast<f32x4*>(lds);
    f32x4* tb = ta + tile_rows * kColQuads;
    float* wl = reinterpret_cast<float*>(tb + tile_rows * kColQuads);     // [2 R + P]
    const int t = threadIdx.x;
    const long long c0 = (long long)blockIdx.x * (4 * kColQuads);
    const int s0 = blockIdx.y * T;
    const size_t slab = (size_t)blockIdx.z * (size_t)S * (size_t)C;
    for (int e = t; e < 2 * R + P; e += 256) wl[e] = e <= 2 * R ? taps[e] : 0.f;
    for (int e = t; e < tile_rows * kColQuads; e += 256) {
        const int q = e / kColQuads, cq = e - q * kColQuads;
        const int s = s0 - R + q;
        const long long c = c0 + 4 * cq;
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (s >= 0 && s < S && c < C) {
            const size_t off = slab + (size_t)s * (size_t)C + (size_t)c;
            if (vec) {
                a = *reinterpret_cast<const f32x4*>(ina + off);
                b = *reinterpret_cast<const f32x4*>(inb + off);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < C) {
                        a[k] = ina[off + k];
                        b[k] = inb[off + k];
                    }
            }
        }
        ta[e] = a;
        tb[e] = b;
    }
    __syncthreads();
    const int cq = t % kColQuads, sg = t / kColQuads;
    const long long c = c0 + 4 * cq;
    const int so = s0 + sg * P;                        // output j is so + j; its tap k' - j sits in tile row sg P + k'
    if (c >= C || so >= S) return;
    const f32x4* pa = ta + (sg * P) * kColQuads + cq;
    const f32x4* pb = tb + (sg * P) * kColQuads + cq;
    f32x4 acca[P], accb[P];
    float wv[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        acca[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        accb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        wv[j] = 0.f;
    }
    for (int kp = 0; kp < 2 * R + P; ++kp) {
#pragma unroll
        for (int j = P - 1; j > 0; --j) wv[j] = wv[j - 1];
        wv[0] = wl[kp];
        const f32x4 xa = pa[kp * kColQuads], xb = pb[kp * kColQuads];
        if (kp >= P - 1 && kp <= 2 * R) {
#pragma unroll
            for (int j = 0; j < P; ++j) {
                acca[j] = acca[j] + wv[j] * xa;
                accb[j] = accb[j] + wv[j] * xb;
            }
        } else {
#pragma unroll
            for (int j = 0; j < P; ++j) {
                if (kp - j < 0 || kp - j > 2 * R) continue;
                acca[j] = acca[j] + wv[j] * xa;
                accb[j] = accb[j] + wv[j] * xb;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
        if (so + j >= S) continue;
        const size_t off = slab + (size_t)(so + j) * (size_t)C + (size_t)c;
        if (vec) {
            *reinterpret_cast<f32x4*>(outa + off) = acca[j];
            *reinterpret_cast<f32x4*>(outb + off) = accb[j];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c + k < C) {
                    outa[off + k] = acca[j][k];
                    outb[off + k] = accb[j][k];
                }
        }
    }
}

template <int P>
static int launch_stream(const char* name, const float* ina, const float* inb, float* outa, float* outb, int A, int S, long long C,
                         const float* taps, int R, hipStream_t s) {
    const size_t lds = stream_pass_lds(R, P);
    // a tile past the default 64 KB needs the limit raised on the CURRENT device: asked for at every such launch (a host-side
    // attribute, not a stream operation), so that a process that changes devices never launches with the limit of another one
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(smooth_stream_kernel<P>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kStreamLdsMax) != hipSuccess)
        MRISR_FAIL(MRISR_E_HIP, "%s: cannot raise the LDS limit", name);
    const int vec = C % 4 == 0 && aligned_to(ina, 16) && aligned_to(inb, 16) && aligned_to(outa, 16) && aligned_to(outb, 16);
    const dim3 grid((unsigned)((C + 4 * kColQuads - 1) / (4 * kColQuads)), (unsigned)ceil_div(S, kSGroups * P), (unsigned)A);
    smooth_stream_kernel<P><<<grid, 256, lds, s>>>(ina, inb, outa, outb, S, C, taps, R, vec);
    MRISR_CHECK_LAUNCH(name);
    return MRISR_OK;
}

static int stream_pass(const char* name, const float* ina, const float* inb, float* outa, float* outb, int A, int S, long long C,
                       const float* taps, int R, hipStream_t s) {
    // the most outputs per thread whose tile leaves room for two workgroups on a CU (R <= 128: P = 1 always fits)
    if (stream_pass_lds(R, 4) <= kStreamLdsMax) return launch_stream<4>(name, ina, inb, outa, outb, A, S, C, taps, R, s);
    if (stream_pass_lds(R, 2) <= kStreamLdsMax) return launch_stream<2>(name, ina, inb, outa, outb, A, S, C, taps, R, s);
    return launch_stream<1>(name, ina, inb, outa, outb, A, S, C, taps, R, s);
}

extern "C" int mrisr_f32_volume_smooth_masked(const float* vol, const unsigned char* mask, const unsigned char* mask2, int X, int Y, int Z,
                                              const float* taps0, int r0, const float* taps1, int r1, const float* taps2, int r2,
                                              float* num, float* den, float* tmp, void* stream) {
    if (!vol || !mask || !num || !den || !tmp) MRISR_FAIL(MRISR_E_ARG, "f32_volume_smooth_masked: null pointer");
    if (!taps0 || !taps1 || !taps2) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_smooth_masked: null taps");
    if (r0 < 0 || r1 < 0 || r2 < 0 || r0 > kMaxRadius || r1 > kMaxRadius || r2 > kMaxRadius)
        MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_smooth_masked: radii %d, %d, %d (0..%d)", r0, r1, r2, kMaxRadius);
    if (const int rc = check_volume_extents("f32_volume_smooth_masked", X, Y, Z)) return rc;
    if (!aligned_to(vol, 4) || !aligned_to(num, 4) || !aligned_to(den, 4) || !aligned_to(tmp, 4) || !aligned_to(taps0, 4) ||
        !aligned_to(taps1, 4) || !aligned_to(taps2, 4))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_smooth_masked: misaligned pointer");
    if (num == den || num == tmp || den == tmp || vol == num || vol == den || vol == tmp)
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_smooth_masked: vol, num, den and tmp must be four buffers");
    static_assert(kZRows * 64 == 256 && kZTile == 4 * 64, "smooth_z_kernel: a wave per row, 4 outputs per thread");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)X * Y * Z;
    float* tmpb = tmp + n;
    {
        const long long rows = (long long)X * Y;
        const int vec_in = Z % 4 == 0 && aligned_to(vol, 16) && aligned_to(mask, 4) && (!mask2 || aligned_to(mask2, 4));
        const int vec_out = Z % 4 == 0 && aligned_to(num, 16) && aligned_to(den, 16);
        const dim3 grid((unsigned)((rows + kZRows - 1) / kZRows), (unsigned)ceil_div(Z, kZTile));
        smooth_z_kernel<<<grid, 256, z_pass_lds(r2), s>>>(vol, mask, mask2, num, den, rows, Z, taps2, r2, vec_in, vec_out);
        MRISR_CHECK_LAUNCH("f32_volume_smooth_masked (z pass)");
    }
    if (const int rc = stream_pass("f32_volume_smooth_masked (y pass)", num, den, tmp, tmpb, X, Y, Z, taps1, r1, s)) return rc;
    return stream_pass("f32_volume_smooth_masked (x pass)", tmp, tmpb, num, den, 1, X, (long long)Y * Z, taps0, r0, s);
}

struct BiasApply {
    const float *src, *num, *den, *num_ref, *den_ref, *p50;
    const long long* count;
    float *field, *out;
    float lo, hi;
    int mode;
};

__global__ __launch_bounds__(256) void bias_apply_kernel(const BiasApply p, size_t n, int vec) {
    const float nan = __uint_as_float(0x7fc00000u);
    float p50 = 1.f;
    bool counted = true;
    if (p.mode == MRISR_BIAS_HUM) {
        p50 = __fadd_rn(*p.p50, 0.f);                  // -0.0 and +0.0 are one median
        counted = *p.count > 0;
    }
    auto lowpass = [&](float num, float den) { return den >= MRISR_DEN_MIN ? __fdiv_rn(num, den) : nan; };
    auto clamp = [&](float f) { return f > p.hi ? p.hi : (f >= p.lo ? f : p.lo); };
    auto one = [&](size_t i, float num, float den, float numr, float denr, float v, float* field) -> float {
        const float l = lowpass(num, den);
        if (p.mode == MRISR_BIAS_LOWPASS) return l;
        float f = 1.f;
        if (p.mode == MRISR_BIAS_PAIR) {
            const float lr = lowpass(numr, denr);
            if (l > 0.f && lr > 0.f) f = __fdiv_rn(lr, l);
            f = clamp(f);
            *field = f;
            return __fmul_rn(v, f);
        }
        if (l > 0.f && counted) f = __fdiv_rn(l, p50);
        f = clamp(f);
        *field = f;
        return __fdiv_rn(v, f);
    };
    const bool pair = p.mode == MRISR_BIAS_PAIR, low = p.mode == MRISR_BIAS_LOWPASS;
    const size_t nv = vec ? n / 4 : 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const f32x4 num = *reinterpret_cast<const f32x4*>(p.num + 4 * i), den = *reinterpret_cast<const f32x4*>(p.den + 4 * i);
        const f32x4 numr = pair ? *reinterpret_cast<const f32x4*>(p.num_ref + 4 * i) : zero;
        const f32x4 denr = pair ? *reinterpret_cast<const f32x4*>(p.den_ref + 4 * i) : zero;
        const f32x4 v = low ? zero : *reinterpret_cast<const f32x4*>(p.src + 4 * i);
        f32x4 f = zero, o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float fk = 0.f;
            o[k] = one(i, num[k], den[k], numr[k], denr[k], v[k], &fk);
            f[k] = fk;
        }
        if (p.field) *reinterpret_cast<f32x4*>(p.field + 4 * i) = f;
        *reinterpret_cast<f32x4*>(p.out + 4 * i) = o;
    }
    for (size_t i = nv * 4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float f = 0.f;
        const float o = one(i, p.num[i], p.den[i], pair ? p.num_ref[i] : 0.f, pair ? p.den_ref[i] : 0.f, low ? 0.f : p.src[i], &f);
        if (p.field) p.field[i] = f;
        p.out[i] = o;
    }
}

extern "C" int mrisr_f32_volume_bias_apply(const float* src, size_t n, const float* num, const float* den, const float* num_ref,
                                           const float* den_ref, const float* p50, const long long* count, float limit, int mode,
                                           float* field, float* out, void* stream) {
    if (mode != MRISR_BIAS_PAIR && mode != MRISR_BIAS_HUM && mode != MRISR_BIAS_LOWPASS)
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_bias_apply: mode %d", mode);
    if (!num || !den || !out || (mode != MRISR_BIAS_LOWPASS && !src) || (mode == MRISR_BIAS_PAIR && (!num_ref || !den_ref)) ||
        (mode == MRISR_BIAS_HUM && (!p50 || !count)))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_bias_apply: null pointer");
    if (n == 0) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_bias_apply: no voxels");
    if (!(limit >= 1.f) || !isfinite(limit)) MRISR_FAIL(MRISR_E_ARG, "f32_volume_bias_apply: limit %g (finite, at least 1)", (double)limit);
    BiasApply p;
    p.src = src, p.num = num, p.den = den, p.num_ref = num_ref, p.den_ref = den_ref, p.p50 = p50, p.count = count;
    p.field = mode == MRISR_BIAS_LOWPASS ? nullptr : field;
    p.out = out;
    p.lo = 1.f / limit, p.hi = limit, p.mode = mode;
    const void* all[] = {src, num, den, num_ref, den_ref, p.field, out};
    int vec = 1;
    for (const void* q : all) vec = vec && (!q || aligned_to(q, 16));
    bias_apply_kernel<<<capped_grid(n, 256 * 8, 2048), 256, 0, (hipStream_t)stream>>>(p, n, vec);
    MRISR_CHECK_LAUNCH("f32_volume_bias_apply");
    return MRISR_OK;
}
