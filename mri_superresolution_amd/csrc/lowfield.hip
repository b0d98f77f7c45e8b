// Low-field MRI simulation on the device (gfx950): the degradation model that turns a high-resolution slice into its
// low-field counterpart - reference utils/preprocessing.py:225-293 (simulate_low_field_mri: FFT -> keep the centre of
// k-space -> complex Gaussian noise -> IFFT -> magnitude -> min/max renormalisation) and utils/extraction_utils.py:136-163
// (clip, 2x INTER_AREA downsampling, truncation to uint8).  utils/lowfield.py:simulate_low_field_host is the float64
// restatement the tests compare against.
//
// The masked FFT / IFFT pair keeps the shifted indices [n/2 - a, n/2 + a), a = int(n f) / 2, i.e. the ASYMMETRIC frequency
// set k in [-a, a).  It is therefore a separable circular convolution with complex Dirichlet rows,
//   Y = P_r x P_c^T,   P[m][n] = p[(m - n) mod N],   p[d] = (1/N) sum_{k=-a}^{a-1} exp(2 pi i k d / N),
// for any size (no FFT library, no power-of-two rule).  P is circulant: the operands are the two rows p_r, p_c
// (mrisr_lowfield_dirichlet fills them in double, stored as float), which live in LDS; P itself is never formed.  The
// reference's k-space noise is white, so in image space it is white complex Gaussian noise of per-component standard
// deviation sigma = noise_std / 2550: either explicit planes (a replayed draw) or Box-Muller on the hashed (seed, pixel)
// draws of common.h.
//
// Pass 1, one workgroup (128 or 256 threads) = kTR output rows of one image, fp32 FMAs throughout:
//   A  U[i][n] = sum_m p_r[(r0 + i - m) mod H] x[m][n]      (complex x real; x as the raw 8-bit value, / 255 at the end)
//      thread = kK columns x kTR rows; the kTR + 7 table entries of eight consecutive m sit in registers (Toeplitz
//      fragment as a sliding window over the LDS row), U goes to LDS and never to HBM
//   B  Y[i][c] = sum_n U[i][n] p_c[(c - n) mod W]            (complex x complex), thread = kK columns x kTR rows,
//      U read as LDS broadcasts, p_c per lane (consecutive lanes, consecutive entries)
//   then m = |Y + noise| -> fp32 plane, and the per-image extrema of m and of x by integer atomic min / max on the bit
//   patterns of the non-negative floats: order-independent, hence bitwise reproducible.
// Pass 2: s = (m - min m) / (max m - min m) * (max x - min x) + min x, clip to [0,1], 2x2 mean (INTER_AREA at exactly
// half scale), truncation to uint8.  DEVIATION: when max m == min m the reference divides 0 by 0; here s = min x.
//
// Float pipeline (mrisr_lowfield_simulate_f32: the slice extraction simulates the percentile-normalised float slice at the
// scan's own size, often odd): pass 1 templated on the input type, the input's extrema by the same integer atomics on the
// bit patterns of the non-negative floats, and a pass 2 that stops after the clip - float32 at full size.
//
// Compiled with -ffp-contract=off (build.py): pass 2 restates host arithmetic operation by operation; the FMAs of pass 1
// are written as fmaf().
#include <math.h>

#include "common.h"

constexpr int kTR = 8;        // output rows per workgroup
constexpr int kWin = kTR + 7; // table entries that eight consecutive source rows touch

// float2 entries of the two tables in LDS, rounded up to an even count so that U behind them starts on 16 bytes (odd H + W)
__host__ __device__ constexpr int lf_table_entries(int H, int W) { return (H + 16 + W + 1) & ~1; }

struct LfExt {                // per-image extrema, filled by pass 1
    unsigned m_min, m_max;    // bit patterns of non-negative floats
    unsigned x_min, x_max;    // 8-bit values; float input: bit patterns of non-negative floats
};

// input sample as the float the column pass multiplies, and as the unsigned key its extrema are taken on
__device__ __forceinline__ float lf_value(uint8_t v) { return (float)v; }
__device__ __forceinline__ float lf_value(float v) { return v; }
__device__ __forceinline__ unsigned lf_key(uint8_t v) { return v; }
__device__ __forceinline__ unsigned lf_key(float v) { return __float_as_uint(v + 0.f); }     // -0.0 -> +0.0

__global__ void lowfield_init_kernel(LfExt* __restrict__ ext, int batch, unsigned x_top) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch) ext[b] = LfExt{0x7f800000u, 0u, x_top, 0u};
}

template <int kK, int kLT, typename TIn>      // columns per thread, threads per workgroup, input type (uint8_t: x = img / 255)
__global__ __launch_bounds__(kLT) void lowfield_pass1_kernel(const TIn* __restrict__ img, const float* __restrict__ pr_re,
                                                             const float* __restrict__ pr_im, const float* __restrict__ pc_re,
                                                             const float* __restrict__ pc_im, const float* __restrict__ n_re,
                                                             const float* __restrict__ n_im, const unsigned long long* __restrict__ seeds,
                                                             float sigma, float* __restrict__ mag, LfExt* __restrict__ ext, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* tr = reinterpret_cast<float2*>(smem);               // [H + 16]: p_r, periodically extended
    float2* tc = tr + H + 16;                                   // [W]: p_c
    float* U = reinterpret_cast<float*>(tr + lf_table_entries(H, W));   // [W][2 kTR]: re of the kTR rows, then im (16-byte aligned)
    const int t = threadIdx.x, b = blockIdx.y, r0 = blockIdx.x * kTR;
    const TIn* x = img + (size_t)b * H * W;
    constexpr bool kU8 = sizeof(TIn) == 1;
    constexpr float kInScale = kU8 ? 1.f / 255.f : 1.f;
    constexpr unsigned kTop = kU8 ? 255u : 0x7f800000u;

    for (int i = t; i < H + 16; i += kLT) { const int d = i % H; tr[i] = make_float2(pr_re[d], pr_im[d]); }
    for (int i = t; i < W; i += kLT) tc[i] = make_float2(pc_re[i], pc_im[i]);
    __syncthreads();

    // ---- A: column pass over all source rows, eight at a time
    unsigned xmn = kTop, xmx = 0u;
    for (int c0 = 0; c0 < W; c0 += kLT * kK) {
        float are[kK][kTR], aim[kK][kTR];
#pragma unroll
        for (int j = 0; j < kK; ++j)
#pragma unroll
            for (int i = 0; i < kTR; ++i) are[j][i] = aim[j][i] = 0.f;
        for (int m0 = 0; m0 < H; m0 += 8) {
            // entry (i, u) of this fragment is p_r[(r0 + i - m0 - u) mod H] = win[i - u + 7]
            int base = (r0 - m0 - 7) % H;
            if (base < 0) base += H;
            float2 win[kWin];
#pragma unroll
            for (int w = 0; w < kWin; ++w) win[w] = tr[base + w];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int m = m0 + u;
                float xv[kK];
#pragma unroll
                for (int j = 0; j < kK; ++j) {
                    const int n = c0 + t + j * kLT;
                    float v = 0.f;
                    if (m < H && n < W) {
                        const TIn s = x[(size_t)m * W + n];
                        v = lf_value(s);
                        if (m >= r0 && m < r0 + kTR) { xmn = min(xmn, lf_key(s)); xmx = max(xmx, lf_key(s)); }
                    }
                    xv[j] = v;
                }
#pragma unroll
                for (int i = 0; i < kTR; ++i) {
                    const float2 p = win[i - u + 7];
#pragma unroll
                    for (int j = 0; j < kK; ++j) {
                        are[j][i] = fmaf(p.x, xv[j], are[j][i]);
                        aim[j][i] = fmaf(p.y, xv[j], aim[j][i]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kK; ++j) {
            const int n = c0 + t + j * kLT;
            if (n < W) {
#pragma unroll
                for (int i = 0; i < kTR; ++i) {
                    U[n * (2 * kTR) + i] = are[j][i] * kInScale;
                    U[n * (2 * kTR) + kTR + i] = aim[j][i] * kInScale;
                }
            }
        }
    }
    __syncthreads();

    // ---- B: row pass, then noise, magnitude and the extrema
    float mmn = __int_as_float(0x7f800000), mmx = 0.f;
    const unsigned long long seed = seeds ? seeds[b] : 0ull;
    const unsigned key = noise_key(seed);
    for (int c0 = 0; c0 < W; c0 += kLT * kK) {
        float yre[kK][kTR], yim[kK][kTR];
        int idx[kK];
#pragma unroll
        for (int j = 0; j < kK; ++j) {
            idx[j] = min(c0 + t + j * kLT, W - 1);      // (c - n) mod W at n = 0; columns past the edge are computed and dropped
#pragma unroll
            for (int i = 0; i < kTR; ++i) yre[j][i] = yim[j][i] = 0.f;
        }
        for (int n = 0; n < W; ++n) {
            const f32x4* up = reinterpret_cast<const f32x4*>(U + n * (2 * kTR));
            const f32x4 r0v = up[0], r1v = up[1], i0v = up[2], i1v = up[3];
            float ure[kTR], uim[kTR];
#pragma unroll
            for (int i = 0; i < 4; ++i) { ure[i] = r0v[i]; ure[4 + i] = r1v[i]; uim[i] = i0v[i]; uim[4 + i] = i1v[i]; }
#pragma unroll
            for (int j = 0; j < kK; ++j) {
                const float2 q = tc[idx[j]];
                idx[j] = idx[j] == 0 ? W - 1 : idx[j] - 1;
#pragma unroll
                for (int i = 0; i < kTR; ++i) {
                    yre[j][i] = fmaf(ure[i], q.x, fmaf(-uim[i], q.y, yre[j][i]));
                    yim[j][i] = fmaf(ure[i], q.y, fmaf(uim[i], q.x, yim[j][i]));
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kK; ++j) {
            const int c = c0 + t + j * kLT;
            if (c >= W) continue;
#pragma unroll
            for (int i = 0; i < kTR; ++i) {
                const int r = r0 + i;
                if (r >= H) continue;
                const size_t pix = (size_t)r * W + c, o = (size_t)b * H * W + pix;
                float re = yre[j][i], im = yim[j][i];
                if (n_re) {
                    re += n_re[o];
                    im += n_im[o];
                } else if (seeds && sigma > 0.f) {
                    float u1, u2;
                    hashed_uniform_pair(key, (unsigned)pix, u1, u2);
                    const float rad = sigma * sqrtf(-2.f * __logf(u1));
                    re = fmaf(rad, __cosf(6.28318530718f * u2), re);
                    im = fmaf(rad, __sinf(6.28318530718f * u2), im);
                }
                const float mg = sqrtf(fmaf(re, re, im * im));
                mag[o] = mg;
                mmn = fminf(mmn, mg);
                mmx = fmaxf(mmx, mg);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mmn = fminf(mmn, __shfl_xor(mmn, o, 64));
        mmx = fmaxf(mmx, __shfl_xor(mmx, o, 64));
        xmn = min(xmn, (unsigned)__shfl_xor((int)xmn, o, 64));
        xmx = max(xmx, (unsigned)__shfl_xor((int)xmx, o, 64));
    }
    if ((t & 63) == 0) {
        atomicMin(&ext[b].m_min, __float_as_uint(mmn));
        atomicMax(&ext[b].m_max, __float_as_uint(mmx));
        atomicMin(&ext[b].x_min, xmn);
        atomicMax(&ext[b].x_max, xmx);
    }
}

__global__ __launch_bounds__(256) void lowfield_pass2_kernel(const float* __restrict__ mag, const LfExt* __restrict__ ext,
                                                             uint8_t* __restrict__ out_u8, float* __restrict__ out_f32, int h, int w) {
    const int b = blockIdx.y;
    const LfExt e = ext[b];
    const float mn = __uint_as_float(e.m_min), mx = __uint_as_float(e.m_max);
    const float omin = __fdiv_rn((float)e.x_min, 255.f), omax = __fdiv_rn((float)e.x_max, 255.f);
    const float den = __fsub_rn(mx, mn), span = __fsub_rn(omax, omin);
    const size_t n = (size_t)h * w;
    const float* src = mag + (size_t)b * n * 4;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        const int y = (int)(p / w), xq = (int)(p - (size_t)y * w);
        float acc = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const float2 v = *reinterpret_cast<const float2*>(src + ((size_t)(2 * y + dy) * (2 * w) + 2 * xq));
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const float mv = dx ? v.y : v.x;
                float s = omin;                                      // max m == min m: the documented deviation
                if (den > 0.f) s = __fadd_rn(__fmul_rn(__fdiv_rn(__fsub_rn(mv, mn), den), span), omin);
                acc = __fadd_rn(acc, fminf(fmaxf(s, 0.f), 1.f));     // np.clip(simulated, 0, 1)
            }
        }
        const float lr = __fmul_rn(acc, 0.25f);                      // the 2x2 mean
        if (out_f32) out_f32[(size_t)b * n + p] = lr;
        if (out_u8) out_u8[(size_t)b * n + p] = (uint8_t)(int)fminf(fmaxf(__fmul_rn(lr, 255.f), 0.f), 255.f);   // astype(np.uint8) truncates
    }
}

// float pipeline: the same renormalisation at full size, float32 out (no 2x2 mean, no uint8)
__global__ __launch_bounds__(256) void lowfield_pass2_f32_kernel(const float* __restrict__ mag, const LfExt* __restrict__ ext,
                                                                 float* __restrict__ out, size_t n) {
    const int b = blockIdx.y;
    const LfExt e = ext[b];
    const float mn = __uint_as_float(e.m_min), mx = __uint_as_float(e.m_max);
    const float omin = __uint_as_float(e.x_min), omax = __uint_as_float(e.x_max);
    const float den = __fsub_rn(mx, mn), span = __fsub_rn(omax, omin);
    const float* src = mag + (size_t)b * n;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        float s = omin;                                              // max m == min m: the documented deviation
        if (den > 0.f) s = __fadd_rn(__fmul_rn(__fdiv_rn(__fsub_rn(src[p], mn), den), span), omin);
        out[(size_t)b * n + p] = fminf(fmaxf(s, 0.f), 1.f);         // np.clip(simulated, 0, 1)
    }
}

static int lowfield_half_width(int n, double f) { return (int)((double)n * f) / 2; }

static int lowfield_dirichlet_fill(int n, int a, float* re, float* im) {
    const double two_pi = 6.283185307179586476925286766559;
    for (int d = 0; d < n; ++d) {
        double sr = 0.0, si = 0.0;
        for (int k = -a; k < a; ++k) {
            // the angle from the exactly reduced integer k d mod n: no large-argument loss
            const double ang = two_pi * (double)((((long long)k * d) % n + n) % n) / (double)n;
            sr += cos(ang);
            si += sin(ang);
        }
        re[d] = (float)(sr / n);
        im[d] = (float)(si / n);
    }
    return MRISR_OK;
}

extern "C" int mrisr_lowfield_dirichlet(int n, double crop_factor, float* re, float* im) {
    if (!re || !im) MRISR_FAIL(MRISR_E_ARG, "lowfield_dirichlet: null pointer");
    if (n < 4 || (n & 1)) MRISR_FAIL(MRISR_E_SHAPE, "lowfield_dirichlet: size %d (even, >= 4)", n);
    if (!(crop_factor > 0.0 && crop_factor <= 1.0)) MRISR_FAIL(MRISR_E_ARG, "lowfield_dirichlet: crop_factor %g outside (0, 1]", crop_factor);
    const int a = lowfield_half_width(n, crop_factor);
    if (a == 0) MRISR_FAIL(MRISR_E_ARG, "lowfield_dirichlet: crop_factor %g keeps nothing of %d samples", crop_factor, n);
    return lowfield_dirichlet_fill(n, a, re, im);
}

// any n >= 2: the reference's mask keeps the shifted indices [n/2 - a, n/2 + a) and n / 2 (integer division) is frequency 0
// after fftshift for odd n too, so the kept set is k in [-a, a) whatever the parity
extern "C" int mrisr_lowfield_dirichlet_any(int n, double crop_factor, float* re, float* im) {
    if (!re || !im) MRISR_FAIL(MRISR_E_ARG, "lowfield_dirichlet_any: null pointer");
    if (n < 2) MRISR_FAIL(MRISR_E_SHAPE, "lowfield_dirichlet_any: size %d (>= 2)", n);
    if (!(crop_factor > 0.0 && crop_factor <= 1.0)) MRISR_FAIL(MRISR_E_ARG, "lowfield_dirichlet_any: crop_factor %g outside (0, 1]", crop_factor);
    const int a = lowfield_half_width(n, crop_factor);
    if (a == 0) MRISR_FAIL(MRISR_E_ARG, "lowfield_dirichlet_any: crop_factor %g keeps nothing of %d samples", crop_factor, n);
    return lowfield_dirichlet_fill(n, a, re, im);
}

extern "C" size_t mrisr_lowfield_workspace_bytes(int batch, int H, int W) {
    if (batch < 1 || H < 1 || W < 1) return 0;
    return (size_t)batch * H * W * sizeof(float) + (size_t)batch * sizeof(LfExt);
}

static size_t lowfield_lds_bytes(int H, int W) {
    return (size_t)lf_table_entries(H, W) * sizeof(float2) + (size_t)W * 2 * kTR * sizeof(float);
}

// the extrema's initial values and pass 1 for either input type
template <typename TIn>
static void lowfield_pass1(const TIn* high, int batch, int H, int W, const float* row_re, const float* row_im, const float* col_re,
                           const float* col_im, float sigma, const float* noise_re, const float* noise_im,
                           const unsigned long long* seeds_device, float* mag, LfExt* ext, hipStream_t s) {
    const size_t lds = lowfield_lds_bytes(H, W);
    lowfield_init_kernel<<<ceil_div(batch, 256), 256, 0, s>>>(ext, batch, sizeof(TIn) == 1 ? 255u : 0x7f800000u);
    dim3 grid(ceil_div(H, kTR), batch);
#define LF_LAUNCH(K, T)                                                                                                           \
    do {                                                                                                                         \
        if (lds > 64 * 1024)                                                                                                     \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lowfield_pass1_kernel<K, T, TIn>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
        lowfield_pass1_kernel<K, T, TIn><<<grid, T, lds, s>>>(high, row_re, row_im, col_re, col_im, noise_re, noise_im, seeds_device, sigma, \
                                                             mag, ext, H, W);                                                    \
    } while (0)
    // two columns per thread where the width allows it (half the LDS reads per FMA of one column); wide images take 256
    // threads, so that a workgroup's share of LDS carries four waves
    if (W <= 128) LF_LAUNCH(1, 128);
    else if (W <= 256) LF_LAUNCH(2, 128);
    else if (W <= 512) LF_LAUNCH(2, 256);
    else LF_LAUNCH(4, 256);
#undef LF_LAUNCH
}

extern "C" int mrisr_lowfield_simulate(const uint8_t* high, int batch, int H, int W, double crop_factor, const float* row_re,
                                       const float* row_im, const float* col_re, const float* col_im, float sigma,
                                       const float* noise_re, const float* noise_im, const unsigned long long* seeds_device,
                                       void* workspace, uint8_t* out_u8, float* out_f32, void* stream) {
    if (!high || !row_re || !row_im || !col_re || !col_im || !workspace || (!out_u8 && !out_f32))
        MRISR_FAIL(MRISR_E_ARG, "lowfield_simulate: null pointer (one of out_u8 / out_f32 is needed)");
    if ((noise_re == nullptr) != (noise_im == nullptr)) MRISR_FAIL(MRISR_E_ARG, "lowfield_simulate: noise_re and noise_im go together");
    if (batch < 1 || batch > 65535) MRISR_FAIL(MRISR_E_SHAPE, "lowfield_simulate: batch %d", batch);
    if (H < 4 || W < 4 || (H & 1) || (W & 1)) MRISR_FAIL(MRISR_E_SHAPE, "lowfield_simulate: H %d W %d (even, >= 4)", H, W);
    if (!(crop_factor > 0.0 && crop_factor <= 1.0)) MRISR_FAIL(MRISR_E_ARG, "lowfield_simulate: crop_factor %g outside (0, 1]", crop_factor);
    if (lowfield_half_width(H, crop_factor) == 0 || lowfield_half_width(W, crop_factor) == 0)
        MRISR_FAIL(MRISR_E_ARG, "lowfield_simulate: crop_factor %g keeps nothing of %d x %d", crop_factor, H, W);
    if (!(sigma >= 0.f)) MRISR_FAIL(MRISR_E_ARG, "lowfield_simulate: sigma %g", (double)sigma);
    if (lowfield_lds_bytes(H, W) > 160 * 1024 || ceil_div(H, kTR) > 65535)
        MRISR_FAIL(MRISR_E_SHAPE, "lowfield_simulate: H %d W %d too large (%zu bytes of LDS)", H, W, lowfield_lds_bytes(H, W));
    hipStream_t s = (hipStream_t)stream;
    float* mag = reinterpret_cast<float*>(workspace);
    LfExt* ext = reinterpret_cast<LfExt*>(mag + (size_t)batch * H * W);
    lowfield_pass1(high, batch, H, W, row_re, row_im, col_re, col_im, sigma, noise_re, noise_im, seeds_device, mag, ext, s);
    const size_t n = (size_t)(H / 2) * (W / 2);
    size_t blocks = (n + 256 * 4 - 1) / (256 * 4);
    if (blocks > 1024) blocks = 1024;
    lowfield_pass2_kernel<<<dim3((unsigned)blocks, batch), 256, 0, s>>>(mag, ext, out_u8, out_f32, H / 2, W / 2);
    MRISR_CHECK_LAUNCH("lowfield_simulate");
    return MRISR_OK;
}

extern "C" int mrisr_lowfield_simulate_f32(const float* high, int batch, int H, int W, double crop_factor, const float* row_re,
                                           const float* row_im, const float* col_re, const float* col_im, float sigma,
                                           const float* noise_re, const float* noise_im, const unsigned long long* seeds_device,
                                           void* workspace, float* out_f32, void* stream) {
    if (!high || !row_re || !row_im || !col_re || !col_im || !workspace || !out_f32) MRISR_FAIL(MRISR_E_ARG, "lowfield_simulate_f32: null pointer");
    if ((noise_re == nullptr) != (noise_im == nullptr)) MRISR_FAIL(MRISR_E_ARG, "lowfield_simulate_f32: noise_re and noise_im go together");
    if (batch < 1 || batch > 65535) MRISR_FAIL(MRISR_E_SHAPE, "lowfield_simulate_f32: batch %d", batch);
    if (H < 2 || W < 2) MRISR_FAIL(MRISR_E_SHAPE, "lowfield_simulate_f32: H %d W %d (>= 2)", H, W);
    if (!(crop_factor > 0.0 && crop_factor <= 1.0)) MRISR_FAIL(MRISR_E_ARG, "lowfield_simulate_f32: crop_factor %g outside (0, 1]", crop_factor);
    if (lowfield_half_width(H, crop_factor) == 0 || lowfield_half_width(W, crop_factor) == 0)
        MRISR_FAIL(MRISR_E_ARG, "lowfield_simulate_f32: crop_factor %g keeps nothing of %d x %d", crop_factor, H, W);
    if (!(sigma >= 0.f)) MRISR_FAIL(MRISR_E_ARG, "lowfield_simulate_f32: sigma %g", (double)sigma);
    if (lowfield_lds_bytes(H, W) > 160 * 1024 || ceil_div(H, kTR) > 65535)
        MRISR_FAIL(MRISR_E_SHAPE, "lowfield_simulate_f32: H %d W %d too large (%zu bytes of LDS)", H, W, lowfield_lds_bytes(H, W));
    hipStream_t s = (hipStream_t)stream;
    float* mag = reinterpret_cast<float*>(workspace);
    LfExt* ext = reinterpret_cast<LfExt*>(mag + (size_t)batch * H * W);
    lowfield_pass1(high, batch, H, W, row_re, row_im, col_re, col_im, sigma, noise_re, noise_im, seeds_device, mag, ext, s);
    const size_t n = (size_t)H * W;
    size_t blocks = (n + 256 * 4 - 1) / (256 * 4);
    if (blocks > 1024) blocks = 1024;
    lowfield_pass2_f32_kernel<<<dim3((unsigned)blocks, batch), 256, 0, s>>>(mag, ext, out_f32, n);
    MRISR_CHECK_LAUNCH("lowfield_simulate_f32");
    return MRISR_OK;
}
