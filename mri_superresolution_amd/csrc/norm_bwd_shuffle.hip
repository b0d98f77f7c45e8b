// GroupNorm(8,C)+LeakyReLU(0.2) backward of the 2x head's nodes: pass 2 of a pixel-shuffled node with dx stored un-shuffled,
// and both alpha-blend branches through the two passes together (pass 1 of a single node is norm_bwd.hip's).
#include "norm_bwd.h"

// Pass 2 of a pixel-shuffled node without the intermediate g tensor: dx is stored un-shuffled, [N][H/2][W/2][4C] with
// channel 4c + 2(Y&1) + (X&1) (the producing conv's own output layout).  Thread = (2x2 window of the shuffled image,
// 16-byte channel vector): eight full-vector loads (x and the consumer's gradient at the four pixels) and 4*VEC
// consecutive destination channels = one contiguous 4*16-byte store.  dbias (optional, [4C]) += channel sums of dx.
template <typename T>
__global__ __launch_bounds__(256) void act_bwd_unshuffle_window_kernel(const ActBwdParams p, T* __restrict__ dx,
                                                                       float* __restrict__ dbias, const FinDev fin) {
    constexpr int VEC = Vec16<T>::N;
    __shared__ float lds[256 * 4 * VEC];
    const int t = threadIdx.x, n = blockIdx.y;
    const int cz = blockIdx.z * 256 * VEC;
    const int nvec = min(256, p.C / VEC - (int)blockIdx.z * 256), ppb = 256 / nvec;
    const int cv = t % nvec, pl = t / nvec, c = cz + cv * VEC;
    const bool active = pl < ppb;
    const int Hp = p.H / 2, Wp = p.W / 2, HWp = Hp * Wp, W = p.W;
    float sc[VEC], sh[VEC], ca[VEC], cb[VEC], cc[VEC], bs[4 * VEC];
    gn_bwd_coefs<VEC>(fin, lds, n, p.C, c, active, blockIdx.x == 0, pl == 0, blockIdx.x + blockIdx.y + blockIdx.z == 0, ca, cb, cc);
    float w0 = 1.f;
    if (p.blend_alpha) {
        const float a = 1.f / (1.f + __expf(-p.blend_alpha[0]));
        w0 = p.cons[0].weight_mode == 0 ? 1.f : (p.cons[0].weight_mode == 1 ? a : 1.f - a);
    }
    const size_t k0 = (size_t)n * p.C + c;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        sc[e] = active ? p.scale[k0 + e] : 0.f;
        sh[e] = active ? p.shift[k0 + e] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4 * VEC; ++i) bs[i] = 0.f;
    const T* xb = (const T*)p.x + (size_t)n * p.H * W * p.C + c;
    const T* db = (const T*)p.cons[0].da + (size_t)n * p.H * W * p.cons[0].C_total + p.cons[0].c_off + c;
    const int Ct = p.cons[0].C_total;
    T* ob = dx + (size_t)n * HWp * 4 * p.C + 4 * c;
    const int pend = min(HWp, (int)(blockIdx.x + 1) * p.pix_per_block);
    if (active) {
        for (int pp = blockIdx.x * p.pix_per_block + pl; pp < pend; pp += ppb) {
            const int py = pp / Wp, px = pp - py * Wp;
            const size_t b0 = (size_t)(2 * py) * W + 2 * px;
            const size_t off[4] = {b0, b0 + 1, b0 + W, b0 + W + 1};
            Vec16<T> xv[4], dv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { xv[q] = load_vec16(xb + off[q] * p.C); dv[q] = load_vec16(db + off[q] * Ct); }
            Vec16<T> ov[4];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float xr = xv[q].get(e);
                    const float pre = xr * sc[e] + sh[e];
                    const float gy = w0 * dv[q].get(e) * (pre > 0.f ? 1.f : LRELU_SLOPE);
                    const int i = 4 * e + q;          // destination channel 4(c + e) + q
                    ov[i / VEC].set(i % VEC, gy * ca[e] + xr * cb[e] + cc[e]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) store_vec16(ob + (size_t)pp * 4 * p.C + j * VEC, ov[j]);
            if (dbias) {
#pragma unroll
                for (int i = 0; i < 4 * VEC; ++i) bs[i] += ov[i / VEC].get(i % VEC);     // (the rounded value the weight-gradient kernel will read)
            }
        }
    }
    if (dbias) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4 * VEC; ++i) lds[t * 4 * VEC + i] = active ? bs[i] : 0.f;
        __syncthreads();
        for (int j = t; j < nvec * 4 * VEC; j += 256) {
            const int cvj = j / (4 * VEC), i = j - cvj * 4 * VEC;
            float v = 0.f;
            for (int q = 0; q < ppb; ++q) v += lds[(q * nvec + cvj) * 4 * VEC + i];
            atomic_add_f32(&dbias[4 * (cz + cvj * VEC) + i], v);
        }
    }
}

extern "C" int mrisr_act_bwd_apply_fused_unshuffle(int dtype, const void* x, const float* scale, const float* shift,
                                                   const mrisr_consumer* consumer, const float* blend_alpha,
                                                   const mrisr_gn_bwd_fin* fin, void* dx, float* dbias, int N, int H, int W,
                                                   int C, void* stream) {
    if (!x || !scale || !shift || !dx || !consumer || !fin) MRISR_FAIL(MRISR_E_ARG, "act_bwd_apply_fused_unshuffle: null pointer");
    FinDev fd;
    int frc = make_fin_dev(fd, fin, C, "act_bwd_apply_fused_unshuffle: fin");
    if (frc) return frc;
    const int vec = mrisr_vec(dtype);
    if (C % vec || ((H | W) & 1)) MRISR_FAIL(MRISR_E_SHAPE, "act_bwd_apply_fused_unshuffle: C %d, H %d, W %d (even dims)", C, H, W);
    if (consumer->spatial != MRISR_SP_NONE || consumer->H != H || consumer->W != W || consumer->off_y || consumer->off_x)
        MRISR_FAIL(MRISR_E_UNSUPPORTED, "act_bwd_apply_fused_unshuffle: one plain consumer with the node's geometry");
    ActBwdParams p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.scale = scale; p.shift = shift; p.blend_alpha = blend_alpha;
    p.ncons = 1; p.N = N; p.H = H; p.W = W; p.C = C;
    int rc = fill_act_bwd_params(p, dtype, 1, consumer, blend_alpha, H, W, C, "act_bwd_apply_fused_unshuffle");
    if (rc) return rc;
    // every block ends in 4C same-row float atomics when the bias gradient is asked for: few, long-running blocks
    const PixelBlocks b = pixel_blocks((H / 2) * (W / 2), N, C, vec, 16);
    p.pix_per_block = b.per_block;
    const bool known = with_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        act_bwd_unshuffle_window_kernel<T><<<b.grid, 256, 0, (hipStream_t)stream>>>(p, (T*)dx, dbias, fd);
    });
    if (!known) MRISR_FAIL(MRISR_E_DTYPE, "act_bwd_apply_fused_unshuffle: dtype %d", dtype);
    MRISR_CHECK_LAUNCH("act_bwd_apply_fused_unshuffle");
    return MRISR_OK;
}

// ------------------------------------------------------------------------------------------------
// The two branches of the 2x head (final_up_pixelshuffle.conv, stored pixel-shuffled, and final_up_bilinear.1, plain) have ONE
// consumer between them: final_conv.0's input gradient, weighted sigmoid(alpha) for one and 1 - sigmoid(alpha) for the other
// (unet_model.py:206-207).  Run as two nodes, each of the four passes (act_bwd_reduce_kernel<T,0> twice, act_bwd_unshuffle_window_kernel,
// act_bwd_apply_fused_kernel) reads that gradient in full; here both nodes go through the two-pass scheme TOGETHER and a pass
// reads it once: 3 tensors instead of 4 in pass 1, 5 instead of 6 in pass 2, two launches instead of four.  No synchronisation
// beyond the launch boundary between the passes.
// Mapping of both kernels = act_bwd_unshuffle_window_kernel's: block = (window range, image), thread = (2x2 window, 16-byte
// channel vector), so the thread that reads the shared gradient also owns one contiguous 64-byte run of the un-shuffled dx.
struct BlendBranchDev {
    const void* x;
    const float* scale;
    const float* shift;
    const float* meanrstd;
    float* red;             // [N][C][2]
    float* alpha_slots;     // [256]
    int weight_mode;        // 1: sigmoid(alpha), 2: 1 - sigmoid(alpha)
};
struct BlendBwdParams {
    const void* da;         // [N][H][W][C]: the blended tensor's gradient
    const float* blend_alpha;
    BlendBranchDev br[2];   // 0: the pixel-shuffled branch, 1: the plain one
    int N, H, W, C, groups, pix_per_block;
};

// Pass 1: per branch what act_bwd_reduce_kernel<T,0> accumulates with g = NULL and alpha_slots set (same formulas, same slot
// spreading, same block reduction in front of the atomics).
template <typename T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void act_bwd_blend_reduce_kernel(const BlendBwdParams p) {
    constexpr int VEC = Vec16<T>::N;
    __shared__ float lds[256 * VEC * 2];
    const int t = threadIdx.x, n = blockIdx.y;
    const int nvec = p.C / VEC, ppb = 256 / nvec;       // host-checked: C / VEC <= 256
    const int cv = t % nvec, pl = t / nvec, c = cv * VEC;
    const bool active = pl < ppb;
    const int Wp = p.W / 2, HWp = (p.H / 2) * Wp, W = p.W;
    const int gs = p.C / p.groups;
    const float a = 1.f / (1.f + __expf(-p.blend_alpha[0]));
    float wgt[2], sc[2][VEC], sh[2][VEC], sA[2][VEC], sB[2][VEC], adot[2] = {0.f, 0.f};
    const T* xb[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        wgt[b] = p.br[b].weight_mode == 1 ? a : 1.f - a;
        xb[b] = (const T*)p.br[b].x + (size_t)n * p.H * W * p.C + c;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            sc[b][e] = p.br[b].scale[(size_t)n * p.C + c + e];
            sh[b][e] = p.br[b].shift[(size_t)n * p.C + c + e];
            sA[b][e] = 0.f;
            sB[b][e] = 0.f;
        }
    }
    const T* db = (const T*)p.da + (size_t)n * p.H * W * p.C + c;
    const int pend = min(HWp, (int)(blockIdx.x + 1) * p.pix_per_block);
    if (active) {
#pragma unroll 1
        for (int pp = blockIdx.x * p.pix_per_block + pl; pp < pend; pp += ppb) {
            const int py = pp / Wp, px = pp - py * Wp;
            const size_t b0 = (size_t)(2 * py) * W + 2 * px;
            // written row by row (two pixels, six 16-byte loads); at two waves per SIMD the compiler has the registers to issue
            // both rows' loads together, and does
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const size_t o0 = b0 + (size_t)r * W;
                Vec16<T> dv[2], xv[2][2];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    dv[q] = load_vec16(db + (o0 + q) * p.C);
                    xv[0][q] = load_vec16(xb[0] + (o0 + q) * p.C);
                    xv[1][q] = load_vec16(xb[1] + (o0 + q) * p.C);
                }
#pragma unroll
                for (int q = 0; q < 2; ++q) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const float d = dv[q].get(e);
#pragma unroll
                        for (int b = 0; b < 2; ++b) {
                            const float xr = xv[b][q].get(e);
                            const float pre = xr * sc[b][e] + sh[b][e];
                            const float gy = wgt[b] * d * (pre > 0.f ? 1.f : LRELU_SLOPE);
                            sA[b][e] += gy;
                            sB[b][e] += gy * xr;                    // sum g*x; turned into sum g*xhat after the loop
                            adot[b] += d * lrelu(pre);              // sum d * act feeds dL/dalpha
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const BlendBranchDev& br = p.br[b];
        // sum g*xhat = rstd * (sum g*x - mean * sum g), per thread (<= 32 pixels each)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int g = (c + e) / gs;
            const float mean = br.meanrstd[((size_t)n * p.groups + g) * 2], rstd = br.meanrstd[((size_t)n * p.groups + g) * 2 + 1];
            sB[b][e] = rstd * (sB[b][e] - mean * sA[b][e]);
        }
        // one atomic per wave, spread over the branch's 256 slots
        const float w = wave_sum(active ? adot[b] : 0.f);
        if ((t & 63) == 0) atomic_add_f32(&br.alpha_slots[(blockIdx.x * 4 + (t >> 6) + blockIdx.y * 37) & 255], w);
        // block reduction over the window lanes that share a channel vector
        if (b) __syncthreads();
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            lds[(t * VEC + e) * 2] = active ? sA[b][e] : 0.f;
            lds[(t * VEC + e) * 2 + 1] = active ? sB[b][e] : 0.f;
        }
        __syncthreads();
        for (int i = t; i < nvec * VEC * 2; i += 256) {
            const int j = i >> 1, which = i & 1;
            const int cvj = j / VEC, e = j - cvj * VEC;
            float s = 0.f;
            for (int q = 0; q < ppb; ++q) s += lds[((q * nvec + cvj) * VEC + e) * 2 + which];
            atomic_add_f32(&br.red[((size_t)n * p.C + cvj * VEC + e) * 2 + which], s);
        }
    }
}

// Pass 2: the finalize step of BOTH nodes in the prologue (gn_bwd_coefs: coefficients, dgamma / dbeta, the branch's term of
// dalpha), then per window the shared gradient once, dx of the pixel-shuffled branch stored un-shuffled ([N][H/2][W/2][4C],
// one 64-byte run per thread, as act_bwd_unshuffle_window_kernel) and dx of the plain branch at the window's four pixels
// (as act_bwd_apply_fused_kernel).  dbias (optional, [4C]) += channel sums of the un-shuffled dx.
// The window's twelve 16-byte loads are issued together; the branches are then worked off one after the other, so that only
// the gradient's four vectors live through both.
template <typename T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void act_bwd_blend_apply_kernel(const BlendBwdParams p, T* __restrict__ dx_ps, T* __restrict__ dx_bil,
                                                                  float* __restrict__ dbias, const FinDev fin_ps, const FinDev fin_bil) {
    constexpr int VEC = Vec16<T>::N;
    __shared__ float lds[256 * 4 * VEC];
    const int t = threadIdx.x, n = blockIdx.y;
    const int nvec = p.C / VEC, ppb = 256 / nvec;
    const int cv = t % nvec, pl = t / nvec, c = cv * VEC;
    const bool active = pl < ppb;
    const int Wp = p.W / 2, HWp = (p.H / 2) * Wp, W = p.W;
    float sc[2][VEC], sh[2][VEC], ca[2][VEC], cb[2][VEC], cc[2][VEC], bs[4 * VEC];
    const bool owner = blockIdx.x == 0, first = blockIdx.x + blockIdx.y == 0;
    gn_bwd_coefs<VEC>(fin_ps, lds, n, p.C, c, active, owner, pl == 0, first, ca[0], cb[0], cc[0]);
    __syncthreads();        // the group sums of the first node have been read
    gn_bwd_coefs<VEC>(fin_bil, lds, n, p.C, c, active, owner, pl == 0, first, ca[1], cb[1], cc[1]);
    const float a = 1.f / (1.f + __expf(-p.blend_alpha[0]));
    float wgt[2];
    const T* xb[2];
    const size_t k0 = (size_t)n * p.C + c;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        wgt[b] = p.br[b].weight_mode == 1 ? a : 1.f - a;
        xb[b] = (const T*)p.br[b].x + (size_t)n * p.H * W * p.C + c;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            sc[b][e] = p.br[b].scale[k0 + e];
            sh[b][e] = p.br[b].shift[k0 + e];
        }
    }
#pragma unroll
    for (int i = 0; i < 4 * VEC; ++i) bs[i] = 0.f;
    const T* db = (const T*)p.da + (size_t)n * p.H * W * p.C + c;
    T* ops = dx_ps + (size_t)n * HWp * 4 * p.C + 4 * c;
    T* obl = dx_bil + (size_t)n * p.H * W * p.C + c;
    const int pend = min(HWp, (int)(blockIdx.x + 1) * p.pix_per_block);
    if (active) {
        for (int pp = blockIdx.x * p.pix_per_block + pl; pp < pend; pp += ppb) {
            const int py = pp / Wp, px = pp - py * Wp;
            const size_t b0 = (size_t)(2 * py) * W + 2 * px;
            const size_t off[4] = {b0, b0 + 1, b0 + W, b0 + W + 1};
            Vec16<T> dv[4], xv[4], yv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                dv[q] = load_vec16(db + off[q] * p.C);
                xv[q] = load_vec16(xb[0] + off[q] * p.C);
                yv[q] = load_vec16(xb[1] + off[q] * p.C);
            }
            Vec16<T> ov[4];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float xr = xv[q].get(e);
                    const float pre = xr * sc[0][e] + sh[0][e];
                    const float gy = wgt[0] * dv[q].get(e) * (pre > 0.f ? 1.f : LRELU_SLOPE);
                    const int i = 4 * e + q;          // destination channel 4(c + e) + q
                    ov[i / VEC].set(i % VEC, gy * ca[0][e] + xr * cb[0][e] + cc[0][e]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) store_vec16(ops + (size_t)pp * 4 * p.C + j * VEC, ov[j]);
            if (dbias) {
#pragma unroll
                for (int i = 0; i < 4 * VEC; ++i) bs[i] += ov[i / VEC].get(i % VEC);     // (the rounded value the weight-gradient kernel will read)
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                Vec16<T> o;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float xr = yv[q].get(e);
                    const float pre = xr * sc[1][e] + sh[1][e];
                    const float gy = wgt[1] * dv[q].get(e) * (pre > 0.f ? 1.f : LRELU_SLOPE);
                    o.set(e, gy * ca[1][e] + xr * cb[1][e] + cc[1][e]);
                }
                store_vec16(obl + off[q] * p.C, o);
            }
        }
    }
    if (dbias) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4 * VEC; ++i) lds[t * 4 * VEC + i] = active ? bs[i] : 0.f;
        __syncthreads();
        for (int j = t; j < nvec * 4 * VEC; j += 256) {
            const int cvj = j / (4 * VEC), i = j - cvj * 4 * VEC;
            float v = 0.f;
            for (int q = 0; q < ppb; ++q) v += lds[(q * nvec + cvj) * 4 * VEC + i];
            atomic_add_f32(&dbias[4 * cvj * VEC + i], v);
        }
    }
}

// 16-bit storage, even H and W, whole 16-byte channel vectors, at most 256 of them (one channel slice per block)
extern "C" int mrisr_act_bwd_blend_ok(int dtype, int N, int H, int W, int C) {
    if (dtype != MRISR_BF16 && dtype != MRISR_F16) return 0;
    if (N < 1 || N > 65535 || H < 2 || W < 2 || ((H | W) & 1) || C < 1) return 0;
    const int vec = mrisr_vec(dtype);
    if (C % vec || C / vec > 256) return 0;
    if ((long)H * W >= (1l << 31)) return 0;
    return 1;
}

static int fill_blend_params(BlendBwdParams& p, int dtype, const void* da, const mrisr_blend_branch* ps, const mrisr_blend_branch* bil,
                             const float* blend_alpha, int N, int H, int W, int C, int groups, const char* who) {
    if (!da || !ps || !bil || !blend_alpha) MRISR_FAIL(MRISR_E_ARG, "%s: null pointer", who);
    if (!mrisr_act_bwd_blend_ok(dtype, N, H, W, C)) MRISR_FAIL(MRISR_E_UNSUPPORTED, "%s: shape does not qualify (mrisr_act_bwd_blend_ok)", who);
    if (groups <= 0 || groups > kMaxGroups || C % groups) MRISR_FAIL(MRISR_E_SHAPE, "%s: C %d groups %d", who, C, groups);
    memset(&p, 0, sizeof(p));
    p.da = da; p.blend_alpha = blend_alpha;
    p.N = N; p.H = H; p.W = W; p.C = C; p.groups = groups;
    const mrisr_blend_branch* src[2] = {ps, bil};
    for (int b = 0; b < 2; ++b) {
        const mrisr_blend_branch& s = *src[b];
        if (!s.x || !s.scale || !s.shift || !s.meanrstd || !s.red || !s.alpha_slots) MRISR_FAIL(MRISR_E_ARG, "%s: branch %d null pointer", who, b);
        if (s.weight_mode != 1 && s.weight_mode != 2) MRISR_FAIL(MRISR_E_ARG, "%s: branch %d weight_mode", who, b);
        p.br[b] = BlendBranchDev{s.x, s.scale, s.shift, s.meanrstd, s.red, s.alpha_slots, s.weight_mode};
    }
    return MRISR_OK;
}

extern "C" int mrisr_act_bwd_blend_reduce(int dtype, const void* da, const mrisr_blend_branch* ps, const mrisr_blend_branch* bil,
                                          const float* blend_alpha, int N, int H, int W, int C, int groups, void* stream) {
    BlendBwdParams p;
    int rc = fill_blend_params(p, dtype, da, ps, bil, blend_alpha, N, H, W, C, groups, "act_bwd_blend_reduce");
    if (rc) return rc;
    // 8 windows = 32 pixels per thread: twice act_bwd_reduce_kernel's, half as many blocks per image
    const PixelBlocks b = pixel_blocks((H / 2) * (W / 2), N, C, mrisr_vec(dtype), 8);
    p.pix_per_block = b.per_block;
    with_dtype16(dtype, [&](auto tag) {      // (16-bit storage: mrisr_act_bwd_blend_ok)
        using T = typename decltype(tag)::type;
        act_bwd_blend_reduce_kernel<T><<<b.grid, 256, 0, (hipStream_t)stream>>>(p);
    });
    MRISR_CHECK_LAUNCH("act_bwd_blend_reduce");
    return MRISR_OK;
}

extern "C" int mrisr_act_bwd_blend_apply(int dtype, const void* da, const mrisr_blend_branch* ps, const mrisr_blend_branch* bil,
                                         const float* blend_alpha, const mrisr_gn_bwd_fin* fin_ps, const mrisr_gn_bwd_fin* fin_bil,
                                         void* dx_ps, void* dx_bil, float* dbias, int N, int H, int W, int C, void* stream) {
    if (!fin_ps || !fin_bil || !dx_ps || !dx_bil) MRISR_FAIL(MRISR_E_ARG, "act_bwd_blend_apply: null pointer");
    if (fin_ps->groups != fin_bil->groups) MRISR_FAIL(MRISR_E_SHAPE, "act_bwd_blend_apply: fin groups %d and %d", fin_ps->groups, fin_bil->groups);
    BlendBwdParams p;
    int rc = fill_blend_params(p, dtype, da, ps, bil, blend_alpha, N, H, W, C, fin_ps->groups, "act_bwd_blend_apply");
    if (rc) return rc;
    const mrisr_gn_bwd_fin* fins[2] = {fin_ps, fin_bil};
    const char* who[2] = {"act_bwd_blend_apply: fin 0", "act_bwd_blend_apply: fin 1"};
    FinDev fd[2];
    for (int b = 0; b < 2; ++b) {      // the sums and the slots are the branch's own; the groups were checked with the branches
        const mrisr_gn_bwd_fin* f = fins[b];
        if (f->red != p.br[b].red) MRISR_FAIL(MRISR_E_ARG, "act_bwd_blend_apply: fin %d red", b);
        int frc = make_fin_dev(fd[b], f, C, who[b]);
        if (frc) return frc;
        if (f->alpha_slots != p.br[b].alpha_slots || !f->alpha || !f->dalpha) MRISR_FAIL(MRISR_E_ARG, "act_bwd_blend_apply: fin %d alpha_slots / alpha / dalpha", b);
    }
    // every block ends in 4C same-row float atomics when the bias gradient is asked for: few, long-running blocks
    const PixelBlocks b = pixel_blocks((H / 2) * (W / 2), N, C, mrisr_vec(dtype), 16);
    p.pix_per_block = b.per_block;
    with_dtype16(dtype, [&](auto tag) {      // (16-bit storage: mrisr_act_bwd_blend_ok)
        using T = typename decltype(tag)::type;
        act_bwd_blend_apply_kernel<T><<<b.grid, 256, 0, (hipStream_t)stream>>>(p, (T*)dx_ps, (T*)dx_bil, dbias, fd[0], fd[1]);
    });
    MRISR_CHECK_LAUNCH("act_bwd_blend_apply");
    return MRISR_OK;
}
