// GroupNorm(8,C)+LeakyReLU(0.2) support kernels (HBM-bound element-wise / reduction passes).
//
// Forward: the convolution epilogue accumulates per-(n,group) sums; gn_finalize turns them into the
// per-(n,c) affine (scale, shift) that consumer convolutions apply while loading
// (/root/reference/models/unet_model.py:30-31 and siblings).
// Here also: the materialised blend, pool and bilinear x2 of the activated tensor, the bilinear adjoint, the stand-alone
// statistics and the channel sums.  The GroupNorm + LeakyReLU backward is in norm_bwd*.hip.
#include "common.h"

// ------------------------------------------------------------------------------------------------
__global__ void gn_finalize_kernel(const double* __restrict__ stats, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float* __restrict__ scale,
                                   float* __restrict__ shift, float* __restrict__ meanrstd, int N, int C,
                                   int groups, double count, float eps) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * C) return;
    const int n = idx / C, c = idx - n * C;
    const int gs = C / groups, g = c / gs;
    // the 16 slot pairs as 16-byte loads, all in flight at once (this launch sits between every two convolutions of the
    // forward pass: its latency is paid 20 times per step), summed in slot order
    typedef __attribute__((ext_vector_type(2))) double f64x2;
    f64x2 v[MRISR_STAT_SLOTS];
#pragma unroll
    for (int k = 0; k < MRISR_STAT_SLOTS; ++k) v[k] = *reinterpret_cast<const f64x2*>(stats + ((size_t)(k * N + n) * groups + g) * 2);
    double s = 0.0, ss = 0.0;
#pragma unroll
    for (int k = 0; k < MRISR_STAT_SLOTS; ++k) { s += v[k][0]; ss += v[k][1]; }
    const double mean = s / count;
    double var = ss / count - mean * mean;
    if (var < 0) var = 0;
    // scale and shift are each the float32 rounding of the float64 value: in float32, beta - mean * scale carries the roundings
    // of rstd, scale, mean and the product, 4 ulp of mean * scale where the mean is many deviations from zero
    const double rstd_d = 1.0 / sqrt(var + (double)eps);
    const float rstd = (float)rstd_d;
    const float m = (float)mean;
    const double sc = (double)gamma[c] * rstd_d;
    scale[idx] = (float)sc;
    shift[idx] = (float)((double)beta[c] - mean * sc);
    if (c == g * gs) {
        meanrstd[((size_t)n * groups + g) * 2] = m;
        meanrstd[((size_t)n * groups + g) * 2 + 1] = rstd;
    }
}

extern "C" int mrisr_gn_finalize(const double* stats, const float* gamma, const float* beta, float* scale,
                                 float* shift, float* meanrstd, int N, int C, int groups, double count,
                                 float eps, void* stream) {
    if (!stats || !gamma || !beta || !scale || !shift || !meanrstd) MRISR_FAIL(MRISR_E_ARG, "gn_finalize: null pointer");
    if (groups <= 0 || C % groups) MRISR_FAIL(MRISR_E_SHAPE, "gn_finalize: C %d groups %d", C, groups);
    gn_finalize_kernel<<<ceil_div(N * C, 256), 256, 0, (hipStream_t)stream>>>(stats, gamma, beta, scale, shift,
                                                                             meanrstd, N, C, groups, count, eps);
    MRISR_CHECK_LAUNCH("gn_finalize");
    return MRISR_OK;
}

// ------------------------------------------------------------------------------------------------
// out = sigmoid(alpha) * act0 + (1 - sigmoid(alpha)) * act1, act_i = LeakyReLU(x_i*scale_i+shift_i)  (unet_model.py:206-207):
// the blended input of final_conv.0, materialised.  With 32 channels the conv and its weight gradient are
// staging-bound, and the two-source blending loader doubles that staging; one plain tensor halves it.
// Block = (pixel range, image), thread = (pixel lane, 16-byte channel vector): the four per-(n,c) coefficient vectors are
// loaded once per thread and all index arithmetic is 32-bit.
template <typename T>
__global__ __launch_bounds__(256) void norm_blend_kernel(const T* __restrict__ x0, const float* __restrict__ sc0,
                                                         const float* __restrict__ sh0, const T* __restrict__ x1,
                                                         const float* __restrict__ sc1, const float* __restrict__ sh1,
                                                         const float* __restrict__ alpha, T* __restrict__ out, int HW,
                                                         int C, int pix_per_block) {
    constexpr int VEC = Vec16<T>::N;
    const int t = threadIdx.x, n = blockIdx.y;
    const int nvec = C / VEC, ppb = 256 / nvec;
    const int cv = t % nvec, pl = t / nvec, c = cv * VEC;
    if (pl >= ppb) return;
    const float a = 1.f / (1.f + __expf(-alpha[0])), b = 1.f - a;
    float s0[VEC], t0[VEC], s1[VEC], t1[VEC];
    const size_t k0 = (size_t)n * C + c;
#pragma unroll
    for (int e = 0; e < VEC; ++e) { s0[e] = sc0[k0 + e]; t0[e] = sh0[k0 + e]; s1[e] = sc1[k0 + e]; t1[e] = sh1[k0 + e]; }
    const size_t base = (size_t)n * HW * C + c;
    const int pend = min(HW, (int)(blockIdx.x + 1) * pix_per_block);
    for (int pix = blockIdx.x * pix_per_block + pl; pix < pend; pix += ppb) {
        const size_t o_ = base + (size_t)pix * C;
        const Vec16<T> v0 = load_vec16(x0 + o_), v1 = load_vec16(x1 + o_);
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            o.set(e, a * lrelu(v0.get(e) * s0[e] + t0[e]) + b * lrelu(v1.get(e) * s1[e] + t1[e]));
        store_vec16(out + o_, o);
    }
}

extern "C" int mrisr_norm_blend(int dtype, const void* x0, const float* scale0, const float* shift0, const void* x1,
                                const float* scale1, const float* shift1, const float* alpha, void* out, int N, int H,
                                int W, int C, void* stream) {
    if (!x0 || !scale0 || !shift0 || !x1 || !scale1 || !shift1 || !alpha || !out) MRISR_FAIL(MRISR_E_ARG, "norm_blend: null pointer");
    const int vec = mrisr_vec(dtype);
    if (N <= 0 || N > 65535 || H <= 0 || W <= 0 || C % vec || C / vec > 256) MRISR_FAIL(MRISR_E_SHAPE, "norm_blend: N %d H %d W %d C %d", N, H, W, C);
    if ((size_t)H * W >= (1u << 30)) MRISR_FAIL(MRISR_E_SHAPE, "norm_blend: image %dx%d", H, W);
    const int HW = H * W;
    const PixelBlocks b = pixel_blocks(HW, N, C, vec, 32);
    const bool known = with_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        norm_blend_kernel<T><<<b.grid, 256, 0, (hipStream_t)stream>>>((const T*)x0, scale0, shift0, (const T*)x1, scale1, shift1, alpha, (T*)out, HW, C, b.per_block);
    });
    if (!known) MRISR_FAIL(MRISR_E_DTYPE, "norm_blend: dtype %d", dtype);
    MRISR_CHECK_LAUNCH("norm_blend");
    return MRISR_OK;
}

// ------------------------------------------------------------------------------------------------
// out[c] += sum over pixels of x[pixel][c]   (bias gradient of nn.Conv2d(bias=True), unet_model.py:101)
template <typename T>
__global__ __launch_bounds__(256) void channel_sum_kernel(const T* __restrict__ x, float* __restrict__ out, size_t npix,
                                                          int C, int pix_per_block) {
    constexpr int VEC = Vec16<T>::N;
    __shared__ float lds[256 * VEC];
    const int t = threadIdx.x;
    const int nvec = C / VEC, ppb = 256 / nvec;
    const int cv = t % nvec, pl = t / nvec;
    const bool active = pl < ppb;
    float s[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) s[e] = 0.f;
    const size_t end = min(npix, (size_t)(blockIdx.x + 1) * pix_per_block);
    if (active)
        for (size_t pix = (size_t)blockIdx.x * pix_per_block + pl; pix < end; pix += ppb) {
            const Vec16<T> v = load_vec16(x + pix * C + cv * VEC);
#pragma unroll
            for (int e = 0; e < VEC; ++e) s[e] += v.get(e);
        }
#pragma unroll
    for (int e = 0; e < VEC; ++e) lds[t * VEC + e] = active ? s[e] : 0.f;
    __syncthreads();
    for (int i = t; i < nvec * VEC; i += 256) {
        const int cvj = i / VEC, e = i - cvj * VEC;
        float a = 0.f;
        for (int q = 0; q < ppb; ++q) a += lds[(q * nvec + cvj) * VEC + e];
        atomic_add_f32(&out[i], a);
    }
}

extern "C" int mrisr_channel_sum(int dtype, const void* x, float* out, size_t npix, int C, void* stream) {
    if (!x || !out) MRISR_FAIL(MRISR_E_ARG, "channel_sum: null pointer");
    const int vec = mrisr_vec(dtype);
    if (C % vec || C / vec > 256) MRISR_FAIL(MRISR_E_SHAPE, "channel_sum: C %d", C);
    const int ppb = 256 / (C / vec);
    const int ppblk = ppb * 32;
    const int blocks = (int)((npix + ppblk - 1) / ppblk);
    const bool known = with_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        channel_sum_kernel<T><<<blocks, 256, 0, (hipStream_t)stream>>>((const T*)x, out, npix, C, ppblk);
    });
    if (!known) MRISR_FAIL(MRISR_E_DTYPE, "channel_sum: dtype %d", dtype);
    MRISR_CHECK_LAUNCH("channel_sum");
    return MRISR_OK;
}

// ------------------------------------------------------------------------------------------------
// Stand-alone GroupNorm statistics of an NHWC tensor: stats[n][g] += (sum, sum of squares).  Used by
// conv_forward only when a group has fewer than 4 channels (tiny test networks); otherwise the
// statistics come out of the convolution epilogue.
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* __restrict__ x, double* __restrict__ stats, int HW,
                                                       int C, int groups, int pix_per_block) {
    __shared__ double lds[64 * 2];           // fp64: order-independent to ~1e-16
    const int t = threadIdx.x, n = blockIdx.y;
    const int gs = C / groups;
    for (int i = t; i < groups * 2; i += 256) lds[i] = 0.0;
    __syncthreads();
    const int pend = min(HW, (int)(blockIdx.x + 1) * pix_per_block);
    const T* xb = x + (size_t)n * HW * C;
    const int ppb = 256 / C, c = t % C, pl = t / C;       // C <= 256: one channel per thread column
    if (pl < ppb) {
        float s = 0.f, ss = 0.f;
        for (int pix = blockIdx.x * pix_per_block + pl; pix < pend; pix += ppb) {
            const float v = to_f32(xb[(size_t)pix * C + c]);
            s += v;
            ss += v * v;
        }
        atomicAdd(&lds[2 * (c / gs)], (double)s);
        atomicAdd(&lds[2 * (c / gs) + 1], (double)ss);
    }
    __syncthreads();
    for (int i = t; i < groups * 2; i += 256)
        atomic_add_f64(&stats[stat_slot_off(gridDim.y, groups) + (size_t)n * groups * 2 + i], lds[i]);
}

int launch_gn_stats(int dtype, const void* x, double* stats, int N, int HW, int C, int groups, hipStream_t s) {
    if (groups > 64 || C > 256) MRISR_FAIL(MRISR_E_UNSUPPORTED, "gn_stats: C %d groups %d", C, groups);
    const int ppblk = 1024;
    dim3 grid(ceil_div(HW, ppblk), N);
    auto launch = [&](auto tag) {
        using T = typename decltype(tag)::type;
        gn_stats_kernel<T><<<grid, 256, 0, s>>>((const T*)x, stats, HW, C, groups, ppblk);
    };
    if (!with_dtype16(dtype, launch)) launch(TypeTag<float>{});      // the callers have validated the dtype
    MRISR_CHECK_LAUNCH("gn_stats");
    return MRISR_OK;
}

// ------------------------------------------------------------------------------------------------
// out[n][y][x][c] = max over the 2x2 window of LeakyReLU(x*scale+shift)   (MaxPool2d(2) of the activated tensor,
// unet_model.py:52; floor semantics).  Materialises the (4x smaller) pooled activation so that the encoder
// convolutions and their weight gradients run on the plain prefetching loader.
template <typename T>
__global__ __launch_bounds__(256) void norm_pool2_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, T* __restrict__ out, int H, int W,
                                                         int C, int pix_per_block) {
    constexpr int VEC = Vec16<T>::N;
    const int t = threadIdx.x, n = blockIdx.y;
    const int nvec = C / VEC, ppb = 256 / nvec, Ho = H / 2, Wo = W / 2, HWo = Ho * Wo;
    const int cv = t % nvec, pl = t / nvec, c = cv * VEC;
    if (pl >= ppb) return;
    float sc[VEC], sh[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { sc[e] = scale[(size_t)n * C + c + e]; sh[e] = shift[(size_t)n * C + c + e]; }
    const T* xb = x + (size_t)n * H * W * C + c;
    T* ob = out + (size_t)n * HWo * C + c;
    const int pend = min(HWo, (int)(blockIdx.x + 1) * pix_per_block);
    for (int pp = blockIdx.x * pix_per_block + pl; pp < pend; pp += ppb) {
        const int yo = pp / Wo, xo = pp - yo * Wo;
        const T* b = xb + ((size_t)(2 * yo) * W + 2 * xo) * C;
        const Vec16<T> v00 = load_vec16(b), v01 = load_vec16(b + C), v10 = load_vec16(b + (size_t)W * C), v11 = load_vec16(b + (size_t)W * C + C);
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float a = lrelu(v00.get(e) * sc[e] + sh[e]), bq = lrelu(v01.get(e) * sc[e] + sh[e]);
            const float cq = lrelu(v10.get(e) * sc[e] + sh[e]), d = lrelu(v11.get(e) * sc[e] + sh[e]);
            o.set(e, fmaxf(fmaxf(a, bq), fmaxf(cq, d)));
        }
        store_vec16(ob + (size_t)pp * C, o);
    }
}

extern "C" int mrisr_norm_pool2(int dtype, const void* x, const float* scale, const float* shift, void* out, int N,
                                int H, int W, int C, void* stream) {
    if (!x || !scale || !shift || !out) MRISR_FAIL(MRISR_E_ARG, "norm_pool2: null pointer");
    const int vec = mrisr_vec(dtype);
    if (C % vec || C / vec > 256 || H < 2 || W < 2 || N <= 0 || N > 65535) MRISR_FAIL(MRISR_E_SHAPE, "norm_pool2: N %d C %d H %d W %d", N, C, H, W);
    const PixelBlocks b = pixel_blocks((H / 2) * (W / 2), N, C, vec, 16);
    const bool known = with_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        norm_pool2_kernel<T><<<b.grid, 256, 0, (hipStream_t)stream>>>((const T*)x, scale, shift, (T*)out, H, W, C, b.per_block);
    });
    if (!known) MRISR_FAIL(MRISR_E_DTYPE, "norm_pool2: dtype %d", dtype);
    MRISR_CHECK_LAUNCH("norm_pool2");
    return MRISR_OK;
}

// ------------------------------------------------------------------------------------------------
// Bilinear x2 (align_corners=True) of a raw tensor z_low [N][h][w][C] -> z [N][2h][2w][C] plus the GroupNorm
// statistics of z.  The decoder's "Upsample -> conv1x1" (unet_model.py:71-72) is evaluated as
// "conv1x1 -> Upsample" (both are linear; identical up to fp rounding, 4x fewer conv FLOPs).
template <typename T>
__global__ __launch_bounds__(256) void upsample2_stats_kernel(const T* __restrict__ zl, T* __restrict__ z,
                                                              double* __restrict__ stats, int h, int w, int C,
                                                              int groups, int pix_per_block) {
    constexpr int VEC = Vec16<T>::N;
    __shared__ double lds[64 * 2];
    const int t = threadIdx.x, n = blockIdx.y;
    const int nvec = C / VEC, ppb = 256 / nvec;
    const int cv = t % nvec, pl = t / nvec, c = cv * VEC;
    const int H = 2 * h, W = 2 * w, HW = H * W;
    const int gs = C / groups;
    for (int i = t; i < groups * 2; i += 256) lds[i] = 0.0;
    __syncthreads();
    float s[VEC], ss[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { s[e] = 0.f; ss[e] = 0.f; }
    const T* zb = zl + (size_t)n * h * w * C + c;
    const int pend = min(HW, (int)(blockIdx.x + 1) * pix_per_block);
    if (pl < ppb)
        for (int pix = blockIdx.x * pix_per_block + pl; pix < pend; pix += ppb) {
            const int y = pix / W, x = pix - y * W;
            int y0, y1, x0, x1;
            float wy, wx;
            up2_coord(y, h, y0, y1, wy);
            up2_coord(x, w, x0, x1, wx);
            const Vec16<T> v00 = load_vec16(zb + ((size_t)y0 * w + x0) * C), v01 = load_vec16(zb + ((size_t)y0 * w + x1) * C);
            const Vec16<T> v10 = load_vec16(zb + ((size_t)y1 * w + x0) * C), v11 = load_vec16(zb + ((size_t)y1 * w + x1) * C);
            Vec16<T> o;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float a = (1.f - wy) * ((1.f - wx) * v00.get(e) + wx * v01.get(e)) +
                                wy * ((1.f - wx) * v10.get(e) + wx * v11.get(e));
                o.set(e, a);
                s[e] += a;
                ss[e] += a * a;
            }
            store_vec16(z + ((size_t)n * HW + pix) * C + c, o);
        }
    if (stats) {
        if (pl < ppb) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                atomicAdd(&lds[2 * ((c + e) / gs)], (double)s[e]);
                atomicAdd(&lds[2 * ((c + e) / gs) + 1], (double)ss[e]);
            }
        }
        __syncthreads();
        for (int i = t; i < groups * 2; i += 256)
            atomic_add_f64(&stats[stat_slot_off(gridDim.y, groups) + (size_t)n * groups * 2 + i], lds[i]);
    }
}

extern "C" int mrisr_upsample2_stats(int dtype, const void* z_low, void* z, double* stats, int N, int h, int w, int C,
                                     int groups, void* stream) {
    if (!z_low || !z) MRISR_FAIL(MRISR_E_ARG, "upsample2_stats: null pointer");
    const int vec = mrisr_vec(dtype);
    if (C % vec || C / vec > 256 || groups <= 0 || groups > 64 || C % groups) MRISR_FAIL(MRISR_E_SHAPE, "upsample2_stats: C %d groups %d", C, groups);
    const int ppb = 256 / (C / vec);
    const int ppblk = ppb * 16;
    dim3 grid(ceil_div(4 * h * w, ppblk), N);
    const bool known = with_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        upsample2_stats_kernel<T><<<grid, 256, 0, (hipStream_t)stream>>>((const T*)z_low, (T*)z, stats, h, w, C, groups, ppblk);
    });
    if (!known) MRISR_FAIL(MRISR_E_DTYPE, "upsample2_stats: dtype %d", dtype);
    MRISR_CHECK_LAUNCH("upsample2_stats");
    return MRISR_OK;
}

// adjoint: dz [N][2h][2w][C] -> dz_low [N][h][w][C].  One low-resolution pixel gathers a 4 x 4 neighbourhood of dz; as
// one pixel per thread that is 16 vector loads per output and the pass is bound by the L1 / texture path (2.1 GB of
// loads for a 537 MB tensor: 3 TB/s of HBM traffic).  Here a thread owns a 2 x 2 block of outputs: their 6 x 6
// neighbourhood is read once, row by row (9 loads per output), reduced along x into the two output columns first and
// then along y into the two output rows.  Block = (block range, image), thread = (block lane, 16-byte channel vector).
template <typename T>
__global__ __launch_bounds__(256) void upsample2_adjoint_kernel(const T* __restrict__ dz, T* __restrict__ dzl, int h, int w,
                                                                int C, int blk_per_block) {
    constexpr int VEC = Vec16<T>::N;
    const int t = threadIdx.x, n = blockIdx.y;
    const int nvec = C / VEC, ppb = 256 / nvec, bw = (w + 1) >> 1, nblk = ((h + 1) >> 1) * bw;
    const int cv = t % nvec, pl = t / nvec;
    if (pl >= ppb) return;
    const T* b = dz + (size_t)n * 4 * h * w * C + cv * VEC;
    T* ob = dzl + (size_t)n * h * w * C + cv * VEC;
    const int bend = min(nblk, (int)(blockIdx.x + 1) * blk_per_block);
    for (int bi = blockIdx.x * blk_per_block + pl; bi < bend; bi += ppb) {
        const int by = bi / bw, bx = bi - by * bw;
        const int y0 = 2 * by, x0 = 2 * bx;
        const bool vy1 = y0 + 1 < h, vx1 = x0 + 1 < w;
        // candidate rows / columns of output i: 2(y0+i)-1 .. 2(y0+i)+2 = local index 2i .. 2i+3 of the 6 staged ones
        int iy[2][kUpAdj], ix[2][kUpAdj];
        float wy[2][kUpAdj], wx[2][kUpAdj];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            up2_adjoint_weights(min(y0 + i, h - 1), h, iy[i], wy[i]);
            up2_adjoint_weights(min(x0 + i, w - 1), w, ix[i], wx[i]);
        }
        float acc[2][2][VEC];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[i][j][e] = 0.f;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const int Y = min(max(4 * by - 1 + r, 0), 2 * h - 1);       // clamped: out-of-image rows carry zero weights
            Vec16<T> d[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int X = min(max(4 * bx - 1 + q, 0), 2 * w - 1);
                d[q] = load_vec16(b + (size_t)(Y * (2 * w) + X) * C);
            }
            float hx[2][VEC];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    float v = 0.f;
#pragma unroll
                    for (int k = 0; k < kUpAdj; ++k) v += wx[j][k] * d[2 * j + k].get(e);
                    hx[j][e] = v;
                }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (r < 2 * i || r >= 2 * i + kUpAdj) continue;        // row r is candidate r - 2i of output row i
                const float wv = wy[i][r - 2 * i];
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[i][j][e] += wv * hx[j][e];
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if ((i && !vy1) || (j && !vx1)) continue;
                Vec16<T> o;
#pragma unroll
                for (int e = 0; e < VEC; ++e) o.set(e, acc[i][j][e]);
                store_vec16(ob + (size_t)((y0 + i) * w + x0 + j) * C, o);
            }
    }
}

extern "C" int mrisr_upsample2_adjoint(int dtype, const void* dz, void* dz_low, int N, int h, int w, int C, void* stream) {
    if (!dz || !dz_low) MRISR_FAIL(MRISR_E_ARG, "upsample2_adjoint: null pointer");
    const int vec = mrisr_vec(dtype);
    if (C % vec || C / vec > 256 || N <= 0 || N > 65535 || h <= 0 || w <= 0 || (size_t)h * w >= (1u << 28))
        MRISR_FAIL(MRISR_E_SHAPE, "upsample2_adjoint: N %d h %d w %d C %d", N, h, w, C);
    const PixelBlocks b = pixel_blocks(((h + 1) / 2) * ((w + 1) / 2), N, C, vec, 4);      // 2 x 2 output blocks per lane
    const bool known = with_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        upsample2_adjoint_kernel<T><<<b.grid, 256, 0, (hipStream_t)stream>>>((const T*)dz, (T*)dz_low, h, w, C, b.per_block);
    });
    if (!known) MRISR_FAIL(MRISR_E_DTYPE, "upsample2_adjoint: dtype %d", dtype);
    MRISR_CHECK_LAUNCH("upsample2_adjoint");
    return MRISR_OK;
}

// ------------------------------------------------------------------------------------------------
// out [N][2h][2w][C] = bilinear x2 (align_corners=True) of LeakyReLU(x*scale+shift): materialises the input of
// final_up_bilinear's 3x3 conv (unet_model.py:151-152).  Gathering 4 taps per element inside the conv loader of a
// 32-channel-wide layer is load-bound, so here the interpolated activation is written once and the conv (and
// its weight gradient) run on the plain prefetching loader.
// Thread = (group, 16-byte channel vector); group (gy, gx), gy in [0, h], gx in [0, w], owns the output pixels
// Y in {2gy-1, 2gy}, X in {2gx-1, 2gx}: both rows interpolate between the SAME two source rows (gy-1, gy) and both
// columns between the same two source columns, so the group loads and activates 4 source vectors for its 4 outputs -
// one GroupNorm+LeakyReLU evaluation per output element instead of four (as one output pixel per thread the pass was
// VALU-bound: 24 instructions per element, 3.2 TB/s).  Coordinates and weights are aten's (up2_coord) per output
// row / column; a group whose two rows (columns) do not share their source pair - fp32 rounding of the source
// coordinate at the last row - falls back to one output at a time.
template <typename T>
__global__ __launch_bounds__(256) void norm_upsample2_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, T* __restrict__ out, int N,
                                                             int h, int w, int C, int grp_per_block) {
    constexpr int VEC = Vec16<T>::N;
    const int t = threadIdx.x, n = blockIdx.y;
    const int nvec = C / VEC, ppb = 256 / nvec, H = 2 * h, W = 2 * w, gw = w + 1, ngrp = (h + 1) * gw;
    const int cv = t % nvec, pl = t / nvec, c = cv * VEC;
    if (pl >= ppb) return;
    float sc[VEC], sh[VEC];            // hoisted: one (n, channel vector) per thread
#pragma unroll
    for (int e = 0; e < VEC; ++e) { sc[e] = scale[(size_t)n * C + c + e]; sh[e] = shift[(size_t)n * C + c + e]; }
    const T* b = x + (size_t)n * h * w * C + c;
    T* ob = out + (size_t)n * H * W * C + c;
    auto act = [&](const T* src, float* a) {
        const Vec16<T> v = load_vec16(src);
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = lrelu(v.get(e) * sc[e] + sh[e]);
    };
    const int gend = min(ngrp, (int)(blockIdx.x + 1) * grp_per_block);
    for (int g = blockIdx.x * grp_per_block + pl; g < gend; g += ppb) {
        const int gy = g / gw, gx = g - gy * gw;
        int Y[2] = {2 * gy - 1, 2 * gy}, X[2] = {2 * gx - 1, 2 * gx};
        const bool vy[2] = {Y[0] >= 0, Y[1] < H}, vx[2] = {X[0] >= 0, X[1] < W};
        int y0[2], y1[2], x0[2], x1[2];
        float wy[2], wx[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            up2_coord(min(max(Y[k], 0), H - 1), h, y0[k], y1[k], wy[k]);
            up2_coord(min(max(X[k], 0), W - 1), w, x0[k], x1[k], wx[k]);
        }
        const int ky = vy[0] ? 0 : 1, kx = vx[0] ? 0 : 1;        // the pair the group shares
        const bool shared = (!vy[0] || !vy[1] || (y0[0] == y0[1] && y1[0] == y1[1])) &&
                            (!vx[0] || !vx[1] || (x0[0] == x0[1] && x1[0] == x1[1]));
        if (shared) {
            float a00[VEC], a01[VEC], a10[VEC], a11[VEC];
            act(b + (size_t)(y0[ky] * w + x0[kx]) * C, a00);
            act(b + (size_t)(y0[ky] * w + x1[kx]) * C, a01);
            act(b + (size_t)(y1[ky] * w + x0[kx]) * C, a10);
            act(b + (size_t)(y1[ky] * w + x1[kx]) * C, a11);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (!vy[i] || !vx[j]) continue;
                    Vec16<T> o;
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
                        o.set(e, (1.f - wy[i]) * ((1.f - wx[j]) * a00[e] + wx[j] * a01[e]) + wy[i] * ((1.f - wx[j]) * a10[e] + wx[j] * a11[e]));
                    store_vec16(ob + (size_t)(Y[i] * W + X[j]) * C, o);
                }
        } else {
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) {
                    if (!vy[i] || !vx[j]) continue;
                    float a00[VEC], a01[VEC], a10[VEC], a11[VEC];
                    act(b + (size_t)(y0[i] * w + x0[j]) * C, a00);
                    act(b + (size_t)(y0[i] * w + x1[j]) * C, a01);
                    act(b + (size_t)(y1[i] * w + x0[j]) * C, a10);
                    act(b + (size_t)(y1[i] * w + x1[j]) * C, a11);
                    Vec16<T> o;
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
                        o.set(e, (1.f - wy[i]) * ((1.f - wx[j]) * a00[e] + wx[j] * a01[e]) + wy[i] * ((1.f - wx[j]) * a10[e] + wx[j] * a11[e]));
                    store_vec16(ob + (size_t)(Y[i] * W + X[j]) * C, o);
                }
        }
    }
}

extern "C" int mrisr_norm_upsample2(int dtype, const void* x, const float* scale, const float* shift, void* out, int N,
                                    int h, int w, int C, void* stream) {
    if (!x || !scale || !shift || !out) MRISR_FAIL(MRISR_E_ARG, "norm_upsample2: null pointer");
    const int vec = mrisr_vec(dtype);
    if (C % vec) MRISR_FAIL(MRISR_E_SHAPE, "norm_upsample2: C %d", C);
    if (C / vec > 256 || N <= 0 || N > 65535) MRISR_FAIL(MRISR_E_SHAPE, "norm_upsample2: C %d N %d", C, N);
    if (h <= 0 || w <= 0 || (size_t)h * w >= (1u << 26)) MRISR_FAIL(MRISR_E_SHAPE, "norm_upsample2: h %d w %d", h, w);
    const PixelBlocks b = pixel_blocks((h + 1) * (w + 1), N, C, vec, 8);      // groups (4 output pixels each) per lane
    const bool known = with_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        norm_upsample2_kernel<T><<<b.grid, 256, 0, (hipStream_t)stream>>>((const T*)x, scale, shift, (T*)out, N, h, w, C, b.per_block);
    });
    if (!known) MRISR_FAIL(MRISR_E_DTYPE, "norm_upsample2: dtype %d", dtype);
    MRISR_CHECK_LAUNCH("norm_upsample2");
    return MRISR_OK;
}
