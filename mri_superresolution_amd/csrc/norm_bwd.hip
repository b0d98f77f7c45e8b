// GroupNorm(8,C)+LeakyReLU(0.2) backward, the two-pass form (HBM-bound element-wise / reduction passes):
// aten native_group_norm_backward + leaky_relu_backward + the adjoints of max-pool,
// bilinear upsample, concat and blend, restated as
//   pass 1 (act_bwd_reduce)   g = LeakyReLU'(.) * sum_consumers dL/dact ;  red[n][c] = (sum g, sum g*xhat)
//   finalize                  dgamma, dbeta, and per-(n,c) coefficients A, B, C
//   pass 2 (act_bwd_apply)    dx = g*A + x*B + C
// The one-pass form is in norm_bwd_onepass.hip, the fused un-shuffle and blend-branch forms in norm_bwd_shuffle.hip.
#include "norm_bwd.h"

// PLAIN: every consumer is MRISR_SP_NONE (17 of the 20 nodes of the U-Net) - compiled without the pool / bilinear
// adjoint code, whose 32-float windows cost the generic kernel 155 VGPRs = 3 waves per SIMD, too few loads in
// flight for an HBM-bound pass (measured 3.0 TB/s).
// KIND 3: the single consumer is the output head (MRISR_SP_HEAD): dL/dact = dz * w[c] is formed on the fly from the
// one-channel dz = dL/dout * out * (1 - out), and the head's dW / db fall out of the same pass.
template <typename T, int KIND>   // 0: plain consumers only, 1: plain + 2x2 max-pool, 2: + bilinear adjoint gather, 3: head
__global__ __launch_bounds__(256) void act_bwd_reduce_kernel(const ActBwdParams p) {
    constexpr bool PLAIN = KIND == 0 || KIND == 3;
    constexpr bool HEAD = KIND == 3;
    constexpr int VEC = Vec16<T>::N;
    __shared__ float lds[256 * VEC * 2];
    const int t = threadIdx.x, n = blockIdx.y;
    // blockIdx.z = channel slice of 256 vectors (wide fp32 nodes: C / VEC > 256); one slice everywhere else
    const int cz = blockIdx.z * 256 * VEC;
    const int nvec = min(256, p.C / VEC - (int)blockIdx.z * 256), ppb = 256 / nvec;
    const int cv = t % nvec, pl = t / nvec;
    const bool active = pl < ppb;
    const int c = cz + cv * VEC;
    const int HW = p.H * p.W;
    const int gs = p.C / p.groups;

    float sc[VEC], sh[VEC], sA[VEC], sB[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        sc[e] = p.scale[(size_t)n * p.C + c + e];
        sh[e] = p.shift[(size_t)n * p.C + c + e];
        sA[e] = 0.f;
        sB[e] = 0.f;
    }
    float bw[3] = {1.f, 1.f, 1.f};
    if (p.blend_alpha) {
        const float a = 1.f / (1.f + __expf(-p.blend_alpha[0]));
        bw[1] = a;
        bw[2] = 1.f - a;
    }
    const T* xb = (const T*)p.x + (size_t)n * HW * p.C;
    T* gb = (T*)p.g + (size_t)n * HW * p.C;
    const int pix_end = min(HW, (int)(blockIdx.x + 1) * p.pix_per_block);
    float adot = 0.f;
    float hw[HEAD ? VEC : 1], hdw[HEAD ? VEC : 1], hdb = 0.f;
    if constexpr (HEAD) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) { hw[e] = p.cons[0].head_w[c + e]; hdw[e] = 0.f; }
    }
    if (active) {
        for (int pix = blockIdx.x * p.pix_per_block + pl; pix < pix_end; pix += ppb) {
            const int y = pix / p.W, x = pix - y * p.W;
            const Vec16<T> xv = load_vec16(xb + (size_t)pix * p.C + c);
            float gact[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) gact[e] = 0.f;
            if constexpr (HEAD) {
                const size_t gp = (size_t)n * HW + pix;
                const float o = p.cons[0].head_out[gp];
                const float dz = ((const float*)p.cons[0].da)[gp] * o * (1.f - o);
                if (cv == 0 && blockIdx.z == 0) hdb += dz;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    gact[e] = dz * hw[e];
                    hdw[e] += dz * lrelu(xv.get(e) * sc[e] + sh[e]);
                }
            }
            for (int k = 0; k < (HEAD ? 0 : p.ncons); ++k) {
                const ConsumerDev& cs = p.cons[k];
                const T* dab = (const T*)cs.da + (size_t)n * cs.H * cs.W * cs.C_total + cs.c_off + c;
                const float wgt = cs.weight_mode == 0 ? 1.f : (cs.weight_mode == 1 ? bw[1] : bw[2]);
                if (PLAIN || cs.spatial == MRISR_SP_NONE) {
                    const int yy = y + cs.off_y, xx = x + cs.off_x;
                    if (yy < cs.H && xx < cs.W) {
                        const Vec16<T> d = load_vec16(dab + ((size_t)yy * cs.W + xx) * cs.C_total);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) gact[e] += wgt * d.get(e);
                        if (p.alpha_slots && k == 0) {       // blend branch: sum d * act feeds dL/dalpha
#pragma unroll
                            for (int e = 0; e < VEC; ++e) adot += d.get(e) * lrelu(xv.get(e) * sc[e] + sh[e]);
                        }
                    }
                } else if constexpr (PLAIN) {
                } else if (cs.spatial == MRISR_SP_POOL2) {
                    const int py = y >> 1, px = x >> 1;
                    if (py < cs.H && px < cs.W) {
                        // recompute the 2x2 window's activations one at a time (two 8-float sets live instead of
                        // five): this pixel wins iff it beats every EARLIER window element strictly and every
                        // later one weakly - aten's scan keeps the first maximum
                        const int me = ((y & 1) << 1) | (x & 1);
                        float am[VEC];
                        bool win[VEC];
#pragma unroll
                        for (int e = 0; e < VEC; ++e) { am[e] = lrelu(xv.get(e) * sc[e] + sh[e]); win[e] = true; }
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if (q == me) continue;
                            float aq[VEC];
                            act_of<T>(xb + ((size_t)(2 * py + (q >> 1)) * p.W + 2 * px + (q & 1)) * p.C + c, sc, sh, aq);
#pragma unroll
                            for (int e = 0; e < VEC; ++e) win[e] = win[e] && (q < me ? aq[e] < am[e] : aq[e] <= am[e]);
                        }
                        const Vec16<T> d = load_vec16(dab + ((size_t)py * cs.W + px) * cs.C_total);
#pragma unroll
                        for (int e = 0; e < VEC; ++e)
                            if (win[e]) gact[e] += wgt * d.get(e);
                    }
                } else if constexpr (KIND == 2) {   // adjoint of bilinear x2 (align_corners=True)
                    int iy[kUpAdj], ix[kUpAdj];
                    float wy[kUpAdj], wx[kUpAdj];
                    up2_adjoint_weights(y, p.H, iy, wy);
                    up2_adjoint_weights(x, p.W, ix, wx);
#pragma unroll
                    for (int a = 0; a < kUpAdj; ++a) {
                        if (wy[a] == 0.f) continue;
#pragma unroll
                        for (int b = 0; b < kUpAdj; ++b) {
                            if (wx[b] == 0.f) continue;
                            const int yy = iy[a] + cs.off_y, xx = ix[b] + cs.off_x;
                            const Vec16<T> d = load_vec16(dab + ((size_t)yy * cs.W + xx) * cs.C_total);
                            const float wv = wgt * wy[a] * wx[b];
#pragma unroll
                            for (int e = 0; e < VEC; ++e) gact[e] += wv * d.get(e);
                        }
                    }
                }
            }
            Vec16<T> gv;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float xr = xv.get(e);
                const float pre = xr * sc[e] + sh[e];
                const float gy = gact[e] * (pre > 0.f ? 1.f : LRELU_SLOPE);
                gv.set(e, gy);
                const float gq = p.g ? gv.get(e) : gy;      // the value pass 2 will use (rounded when it goes through g)
                sA[e] += gq;
                sB[e] += gq * xr;                           // sum g*x; turned into sum g*xhat after the loop
            }
            if (p.g) store_vec16(gb + (size_t)pix * p.C + c, gv);
        }
    }
    sums_to_xhat<VEC>(p.meanrstd, n, p.groups, gs, c, sA, sB);      // per thread (<= 16 pixels each)
    if (p.alpha_slots) {      // one atomic per wave, spread over 256 slots (summed by act_bwd_finalize)
        const float w = wave_sum(active ? adot : 0.f);
        if ((t & 63) == 0) atomic_add_f32(&p.alpha_slots[(blockIdx.x * 4 + (t >> 6) + blockIdx.y * 37) & 255], w);
    }
    // block reduction over the pixel lanes that share a channel vector
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        lds[(t * VEC + e) * 2] = active ? sA[e] : 0.f;
        lds[(t * VEC + e) * 2 + 1] = active ? sB[e] : 0.f;
    }
    __syncthreads();
    for (int i = t; i < nvec * VEC * 2; i += 256) {
        const int j = i >> 1, which = i & 1;
        const int cvj = j / VEC, e = j - cvj * VEC;
        float s = 0.f;
        for (int q = 0; q < ppb; ++q) s += lds[((q * nvec + cvj) * VEC + e) * 2 + which];
        atomic_add_f32(&p.red[((size_t)n * p.C + cz + cvj * VEC + e) * 2 + which], s);
    }
    if constexpr (HEAD) {     // the head's weight / bias gradient (what head_bwd_kernel accumulates), per image: all the
        __syncthreads();      // blocks of the launch adding into ONE row of C floats serialise at the memory side
#pragma unroll
        for (int e = 0; e < VEC; ++e) lds[t * VEC + e] = active ? hdw[e] : 0.f;
        const float b = wave_sum(active ? hdb : 0.f);
        if ((t & 63) == 0) lds[256 * VEC + (t >> 6)] = b;
        __syncthreads();
        float* part = p.cons[0].head_part + (size_t)n * (p.C + 1);
        for (int j = t; j < nvec * VEC; j += 256) {
            const int cvj = j / VEC, e = j - cvj * VEC;
            float s = 0.f;
            for (int q = 0; q < ppb; ++q) s += lds[(q * nvec + cvj) * VEC + e];
            atomic_add_f32(&part[cz + cvj * VEC + e], s);
        }
        if (t == 0 && blockIdx.z == 0) atomic_add_f32(&part[p.C], lds[256 * VEC] + lds[256 * VEC + 1] + lds[256 * VEC + 2] + lds[256 * VEC + 3]);
    }
}

// Nodes whose activation is also max-pooled (the encoder skips x1..x3): thread = (pooled pixel, channel vector) owning
// the whole 2x2 window - the four activations and the arg-max are computed ONCE per window (the per-pixel kernel
// recomputed them in each of the window's four threads and needed 120-140 VGPRs), for pass 1 (APPLY = false:
// per-(n,c) sums) and pass 2 (APPLY = true: dx, no intermediate g tensor).  Needs even H, W and - if there is a
// second consumer - a plain one with the node's own geometry (host-checked: act_bwd_window_ok).
template <typename T, bool APPLY>
__global__ __launch_bounds__(256) void act_bwd_pool_window_kernel(const ActBwdParams p, const float* __restrict__ coef,
                                                                  T* __restrict__ dx, const FinDev fin) {
    constexpr int VEC = Vec16<T>::N;
    __shared__ float lds[APPLY ? 2 * kMaxGroups : 256 * VEC * 2];
    const int t = threadIdx.x, n = blockIdx.y;
    const int cz = blockIdx.z * 256 * VEC;        // channel slice, see act_bwd_reduce_kernel
    const int nvec = min(256, p.C / VEC - (int)blockIdx.z * 256), ppb = 256 / nvec;
    const int cv = t % nvec, pl = t / nvec, c = cz + cv * VEC;
    const bool active = pl < ppb;
    const int Hp = p.H / 2, Wp = p.W / 2, HWp = Hp * Wp, W = p.W;
    const int kp = p.cons[0].spatial == MRISR_SP_POOL2 ? 0 : 1, ko = 1 - kp;
    const bool has_o = p.ncons > 1;
    float bw1 = 1.f, bw2 = 1.f;
    if (p.blend_alpha) { bw1 = 1.f / (1.f + __expf(-p.blend_alpha[0])); bw2 = 1.f - bw1; }
    const int mp = p.cons[kp].weight_mode, mo = has_o ? p.cons[ko].weight_mode : 0;
    const float wp = mp == 0 ? 1.f : (mp == 1 ? bw1 : bw2), wo = mo == 0 ? 1.f : (mo == 1 ? bw1 : bw2);
    const size_t k0 = (size_t)n * p.C + c, NC = (size_t)p.N * p.C;
    float sc[VEC], sh[VEC], u0[VEC], u1[VEC], u2[VEC];     // APPLY: u = (cA, cB, cC); reduce: u0 = sum g, u1 = sum g*x
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        sc[e] = p.scale[k0 + e]; sh[e] = p.shift[k0 + e];
        if constexpr (APPLY) {
            if (coef) { u0[e] = coef[k0 + e]; u1[e] = coef[NC + k0 + e]; u2[e] = coef[2 * NC + k0 + e]; }
        } else { u0[e] = 0.f; u1[e] = 0.f; u2[e] = 0.f; }
    }
    if constexpr (APPLY) {
        if (!coef) gn_bwd_coefs<VEC>(fin, lds, n, p.C, c, active, blockIdx.x == 0, pl == 0, blockIdx.x + blockIdx.y + blockIdx.z == 0, u0, u1, u2);
    }
    const T* xb = (const T*)p.x + (size_t)n * p.H * W * p.C + c;
    const T* dpb = (const T*)p.cons[kp].da + (size_t)n * HWp * p.cons[kp].C_total + p.cons[kp].c_off + c;
    const int Cto = has_o ? p.cons[ko].C_total : 0;
    const T* dob = has_o ? (const T*)p.cons[ko].da + (size_t)n * p.H * W * Cto + p.cons[ko].c_off + c : xb;
    T* ob = APPLY ? dx + (size_t)n * p.H * W * p.C + c : nullptr;
    const int pend = min(HWp, (int)(blockIdx.x + 1) * p.pix_per_block);
    if (active) {
        for (int pp = blockIdx.x * p.pix_per_block + pl; pp < pend; pp += ppb) {
            const int py = pp / Wp, px = pp - py * Wp;
            const size_t b0 = (size_t)(2 * py) * W + 2 * px;
            const size_t off[4] = {b0, b0 + 1, b0 + W, b0 + W + 1};
            Vec16<T> xv[4], dv[4], ov[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) xv[q] = load_vec16(xb + off[q] * p.C);
            const Vec16<T> dp = load_vec16(dpb + (size_t)pp * p.cons[kp].C_total);
            if (has_o) {
#pragma unroll
                for (int q = 0; q < 4; ++q) dv[q] = load_vec16(dob + off[q] * Cto);
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                float xr[4], pre[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) { xr[q] = xv[q].get(e); pre[q] = xr[q] * sc[e] + sh[e]; }
                // first maximum of the activations in scan order (aten max_pool2d); LeakyReLU is monotone, so the
                // comparison runs on act = lrelu(pre)
                int win = 0;
                float m = lrelu(pre[0]);
#pragma unroll
                for (int q = 1; q < 4; ++q) {
                    const float a = lrelu(pre[q]);
                    if (a > m) { m = a; win = q; }
                }
                const float gp = wp * dp.get(e);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float gact = q == win ? gp : 0.f;
                    if (has_o) gact += wo * dv[q].get(e);
                    const float gy = gact * (pre[q] > 0.f ? 1.f : LRELU_SLOPE);
                    if constexpr (APPLY) ov[q].set(e, gy * u0[e] + xr[q] * u1[e] + u2[e]);
                    else { u0[e] += gy; u1[e] += gy * xr[q]; }
                }
            }
            if constexpr (APPLY) {
#pragma unroll
                for (int q = 0; q < 4; ++q) store_vec16(ob + off[q] * p.C, ov[q]);
            }
        }
    }
    if constexpr (!APPLY) {
        const int gs = p.C / p.groups;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int g = (c + e) / gs;
            const float mean = p.meanrstd[((size_t)n * p.groups + g) * 2], rstd = p.meanrstd[((size_t)n * p.groups + g) * 2 + 1];
            u1[e] = rstd * (u1[e] - mean * u0[e]);
            lds[(t * VEC + e) * 2] = active ? u0[e] : 0.f;
            lds[(t * VEC + e) * 2 + 1] = active ? u1[e] : 0.f;
        }
        __syncthreads();
        for (int i = t; i < nvec * VEC * 2; i += 256) {
            const int j = i >> 1, which = i & 1;
            const int cvj = j / VEC, e = j - cvj * VEC;
            float s = 0.f;
            for (int q = 0; q < ppb; ++q) s += lds[((q * nvec + cvj) * VEC + e) * 2 + which];
            atomic_add_f32(&p.red[((size_t)n * p.C + cz + cvj * VEC + e) * 2 + which], s);
        }
    }
}

// Pass 2 without the intermediate g tensor (plain consumers only): dL/dact is gathered from the consumers again,
// LeakyReLU' applied, then dx = g*cA + x*cB + cC.  Saves the 2-byte write of pass 1 and reads da instead of g.
// SAME: every consumer gradient has the node's own H x W and no pad offset (all but the odd-size decoder nodes): the
// consumer element is addressed by the linear pixel index - no div/mod per element.
// Block = (pixel range, image), thread = (pixel lane, 16-byte channel vector): the five per-(n,c) coefficient vectors
// are loaded ONCE per thread.  Re-loading them per element put 160 B of L1 traffic next to every 48 B of HBM traffic
// and capped the pass at ~3.7 TB/s.
// No __launch_bounds__: the one this kernel used to carry never took effect (a first declaration without it came before
// the entry that instantiates it), so it has always been compiled for workgroups of up to 1024 threads, and stays so.
template <typename T, bool SAME, bool HEAD>     // HEAD: the single consumer is the output head (MRISR_SP_HEAD)
__global__ void act_bwd_apply_fused_kernel(const ActBwdParams p, const float* __restrict__ coef, T* __restrict__ dx, const FinDev fin) {
    constexpr int VEC = Vec16<T>::N;
    __shared__ float s12[2 * kMaxGroups];
    const int t = threadIdx.x, n = blockIdx.y;
    const int nvec = min(256, p.C / VEC - (int)blockIdx.z * 256), ppb = 256 / nvec;     // blockIdx.z: channel slice
    const int cv = t % nvec, pl = t / nvec, c = blockIdx.z * 256 * VEC + cv * VEC;
    float sc[VEC], sh[VEC], ca[VEC], cb[VEC], cc[VEC];
    if (!coef) gn_bwd_coefs<VEC>(fin, s12, n, p.C, c, pl < ppb, blockIdx.x == 0, pl == 0, blockIdx.x + blockIdx.y + blockIdx.z == 0, ca, cb, cc);
    if (pl >= ppb) return;
    const size_t NC = (size_t)p.N * p.C;
    const int HW = p.H * p.W;
    float bw1 = 1.f, bw2 = 1.f;
    if (p.blend_alpha) {
        bw1 = 1.f / (1.f + __expf(-p.blend_alpha[0]));
        bw2 = 1.f - bw1;
    }
    const int m0 = p.cons[0].weight_mode, m1 = p.cons[1].weight_mode;
    const float w0 = m0 == 0 ? 1.f : (m0 == 1 ? bw1 : bw2), w1 = m1 == 0 ? 1.f : (m1 == 1 ? bw1 : bw2);
    const size_t k0 = (size_t)n * p.C + c;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        sc[e] = p.scale[k0 + e]; sh[e] = p.shift[k0 + e];
        if (coef) { ca[e] = coef[k0 + e]; cb[e] = coef[NC + k0 + e]; cc[e] = coef[2 * NC + k0 + e]; }
    }
    const T* xb = (const T*)p.x + (size_t)n * HW * p.C + c;
    T* ob = dx + (size_t)n * HW * p.C + c;
    const T* d0b = (const T*)p.cons[0].da + (size_t)n * p.cons[0].H * p.cons[0].W * p.cons[0].C_total + p.cons[0].c_off + c;
    const T* d1b = p.ncons > 1 ? (const T*)p.cons[1].da + (size_t)n * p.cons[1].H * p.cons[1].W * p.cons[1].C_total + p.cons[1].c_off + c : d0b;
    float hw[HEAD ? VEC : 1];
    if constexpr (HEAD) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) hw[e] = p.cons[0].head_w[c + e];
    }
    const int pend = min(HW, (int)(blockIdx.x + 1) * p.pix_per_block);
    for (int pix = blockIdx.x * p.pix_per_block + pl; pix < pend; pix += ppb) {
        const Vec16<T> xv = load_vec16(xb + (size_t)pix * p.C);
        float gact[VEC];
        if constexpr (HEAD) {
            const size_t gp = (size_t)n * HW + pix;
            const float o = p.cons[0].head_out[gp];
            const float dz = ((const float*)p.cons[0].da)[gp] * o * (1.f - o);
#pragma unroll
            for (int e = 0; e < VEC; ++e) gact[e] = dz * hw[e];
        } else if constexpr (SAME) {
            const Vec16<T> d0 = load_vec16(d0b + (size_t)pix * p.cons[0].C_total);
            if (p.ncons > 1) {
                const Vec16<T> d1 = load_vec16(d1b + (size_t)pix * p.cons[1].C_total);
#pragma unroll
                for (int e = 0; e < VEC; ++e) gact[e] = w0 * d0.get(e) + w1 * d1.get(e);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) gact[e] = w0 * d0.get(e);
            }
        } else {
            const int y = pix / p.W, x = pix - y * p.W;
#pragma unroll
            for (int e = 0; e < VEC; ++e) gact[e] = 0.f;
            for (int k = 0; k < p.ncons; ++k) {
                const ConsumerDev& cs = p.cons[k];
                const int yy = y + cs.off_y, xx = x + cs.off_x;
                if (yy < cs.H && xx < cs.W) {
                    const Vec16<T> d = load_vec16((k ? d1b : d0b) + ((size_t)yy * cs.W + xx) * cs.C_total);
                    const float wgt = k ? w1 : w0;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) gact[e] += wgt * d.get(e);
                }
            }
        }
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float xr = xv.get(e);
            const float pre = xr * sc[e] + sh[e];
            const float gy = gact[e] * (pre > 0.f ? 1.f : LRELU_SLOPE);
            o.set(e, gy * ca[e] + xr * cb[e] + cc[e]);
        }
        store_vec16(ob + (size_t)pix * p.C, o);
    }
}

extern "C" int mrisr_act_bwd_apply_fused(int dtype, const void* x, const float* scale, const float* shift,
                                         int nconsumers, const mrisr_consumer* consumers, const float* blend_alpha,
                                         const float* coef, const mrisr_gn_bwd_fin* fin, void* dx, int N, int H, int W,
                                         int C, void* stream) {
    if (!x || !scale || !shift || !dx || !consumers) MRISR_FAIL(MRISR_E_ARG, "act_bwd_apply_fused: null pointer");
    if ((coef != nullptr) == (fin != nullptr)) MRISR_FAIL(MRISR_E_ARG, "act_bwd_apply_fused: exactly one of coef / fin");
    FinDev fd;
    memset(&fd, 0, sizeof(fd));
    if (fin) {
        int frc = make_fin_dev(fd, fin, C, "act_bwd_apply_fused: fin");
        if (frc) return frc;
    }
    if (nconsumers < 1 || nconsumers > 2) MRISR_FAIL(MRISR_E_ARG, "act_bwd_apply_fused: %d consumers", nconsumers);
    const int vec = mrisr_vec(dtype);
    if (C % vec) MRISR_FAIL(MRISR_E_SHAPE, "act_bwd_apply_fused: C %d", C);
    int hrc = check_head_consumer(nconsumers, consumers, H, W, C, false, "act_bwd_apply_fused");
    if (hrc) return hrc;
    const bool head = consumers[0].spatial == MRISR_SP_HEAD;
    if (head) {
        if (!fin) MRISR_FAIL(MRISR_E_ARG, "act_bwd_apply_fused: a head consumer needs fin (its dW / db are added up in this launch)");
        fd.head_part = consumers[0].head_part; fd.head_dw = consumers[0].head_dw; fd.head_db = consumers[0].head_db;
    }
    bool plain = true;
    for (int k = 0; k < nconsumers; ++k) plain = plain && (consumers[k].spatial == MRISR_SP_NONE || head);
    const bool window = !plain && act_bwd_window_ok(nconsumers, consumers, H, W);
    if (!plain && !window) MRISR_FAIL(MRISR_E_UNSUPPORTED, "act_bwd_apply_fused: plain consumers (or one 2x2-pool consumer on an even-sized node) only");
    ActBwdParams p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.scale = scale; p.shift = shift; p.blend_alpha = blend_alpha;
    p.ncons = nconsumers; p.N = N; p.H = H; p.W = W; p.C = C;
    int rc = fill_act_bwd_params(p, dtype, nconsumers, consumers, blend_alpha, H, W, C, "act_bwd_apply_fused");
    if (rc) return rc;
    bool same = true;
    for (int k = 0; k < nconsumers; ++k)
        same = same && consumers[k].H == H && consumers[k].W == W && consumers[k].off_y == 0 && consumers[k].off_x == 0;
    // the window kernel takes 16 windows per lane, the per-pixel one 32 pixels
    const PixelBlocks b = window ? pixel_blocks((H / 2) * (W / 2), N, C, vec, 16) : pixel_blocks(H * W, N, C, vec, 32);
    p.pix_per_block = b.per_block;
    hipStream_t s = (hipStream_t)stream;
    const bool known = with_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (window) act_bwd_pool_window_kernel<T, true><<<b.grid, 256, 0, s>>>(p, coef, (T*)dx, fd);
        else if (head) act_bwd_apply_fused_kernel<T, true, true><<<b.grid, 256, 0, s>>>(p, coef, (T*)dx, fd);
        else if (same) act_bwd_apply_fused_kernel<T, true, false><<<b.grid, 256, 0, s>>>(p, coef, (T*)dx, fd);
        else act_bwd_apply_fused_kernel<T, false, false><<<b.grid, 256, 0, s>>>(p, coef, (T*)dx, fd);
    });
    if (!known) MRISR_FAIL(MRISR_E_DTYPE, "act_bwd_apply_fused: dtype %d", dtype);
    MRISR_CHECK_LAUNCH("act_bwd_apply_fused");
    return MRISR_OK;
}

extern "C" int mrisr_act_bwd_reduce(int dtype, const void* x, const float* scale, const float* shift,
                                    const float* meanrstd, int nconsumers, const mrisr_consumer* consumers,
                                    const float* blend_alpha, void* g, float* red, float* alpha_slots, int N, int H,
                                    int W, int C, int groups, void* stream) {
    if (!x || !scale || !shift || !meanrstd || !red || !consumers) MRISR_FAIL(MRISR_E_ARG, "act_bwd_reduce: null pointer");
    if (nconsumers < 1 || nconsumers > 2) MRISR_FAIL(MRISR_E_ARG, "act_bwd_reduce: %d consumers", nconsumers);
    const int vec = mrisr_vec(dtype);
    if (C % vec || groups <= 0 || C % groups) MRISR_FAIL(MRISR_E_SHAPE, "act_bwd_reduce: C %d", C);
    ActBwdParams p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.scale = scale; p.shift = shift; p.meanrstd = meanrstd; p.blend_alpha = blend_alpha; p.g = g; p.red = red;
    p.alpha_slots = alpha_slots;
    if (alpha_slots && (consumers[0].spatial != MRISR_SP_NONE || !blend_alpha)) MRISR_FAIL(MRISR_E_ARG, "act_bwd_reduce: alpha_slots needs a plain first consumer and blend_alpha");
    int hrc = check_head_consumer(nconsumers, consumers, H, W, C, true, "act_bwd_reduce");
    if (hrc) return hrc;
    const bool head = consumers[0].spatial == MRISR_SP_HEAD;
    if (head && g) MRISR_FAIL(MRISR_E_ARG, "act_bwd_reduce: a head consumer goes with g = NULL (mrisr_act_bwd_apply_fused)");
    p.ncons = nconsumers; p.N = N; p.H = H; p.W = W; p.C = C; p.groups = groups;
    int rc = fill_act_bwd_params(p, dtype, nconsumers, consumers, blend_alpha, H, W, C, "act_bwd_reduce");
    if (rc) return rc;
    const bool window = !g && !alpha_slots && act_bwd_window_ok(nconsumers, consumers, H, W);     // pass 1 of the window pair
    if (!window && !g && !head) {
        for (int k = 0; k < nconsumers; ++k)
            if (consumers[k].spatial != MRISR_SP_NONE) MRISR_FAIL(MRISR_E_ARG, "act_bwd_reduce: g = NULL needs plain consumers or a window-eligible pooled node");
    }
    int kind = head ? 3 : 0;
    for (int k = 0; k < nconsumers; ++k) {
        if (consumers[k].spatial == MRISR_SP_POOL2 && kind < 1) kind = 1;
        if (consumers[k].spatial == MRISR_SP_UP2) kind = 2;
    }
    // 16 pixels (or windows) per lane (32 measured slower: fewer blocks, longer tail)
    const PixelBlocks b = pixel_blocks(window ? (H / 2) * (W / 2) : H * W, N, C, vec, 16);
    p.pix_per_block = b.per_block;
    hipStream_t s = (hipStream_t)stream;
    const bool known = with_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (window) act_bwd_pool_window_kernel<T, false><<<b.grid, 256, 0, s>>>(p, nullptr, (T*)nullptr, FinDev{});
        else if (kind == 0) act_bwd_reduce_kernel<T, 0><<<b.grid, 256, 0, s>>>(p);
        else if (kind == 1) act_bwd_reduce_kernel<T, 1><<<b.grid, 256, 0, s>>>(p);
        else if (kind == 3) act_bwd_reduce_kernel<T, 3><<<b.grid, 256, 0, s>>>(p);
        else act_bwd_reduce_kernel<T, 2><<<b.grid, 256, 0, s>>>(p);
    });
    if (!known) MRISR_FAIL(MRISR_E_DTYPE, "act_bwd_reduce: dtype %d", dtype);
    MRISR_CHECK_LAUNCH("act_bwd_reduce");
    return MRISR_OK;
}

// ------------------------------------------------------------------------------------------------
// red[N][C][2] -> dgamma[C] += sum_n B, dbeta[C] += sum_n A, and the pass-2 coefficients
//   dx = g*cA + x*cB + cC  with  cA = rstd*gamma, cB = -rstd^2*S2/M, cC = mean*rstd^2*S2/M - rstd*S1/M
//   S1[n,g] = sum_{c in g} gamma_c A[n,c],  S2[n,g] = sum_{c in g} gamma_c B[n,c],  M = count.
__global__ void act_bwd_finalize_kernel(const float* __restrict__ red, const float* __restrict__ gamma,
                                        const float* __restrict__ meanrstd, float* __restrict__ dgamma,
                                        float* __restrict__ dbeta, float* __restrict__ coef, int N, int C,
                                        int groups, float inv_count, const float* __restrict__ alpha_slots,
                                        const float* __restrict__ alpha, float* __restrict__ dalpha, float alpha_sign) {
    if (alpha_slots && blockIdx.x == 0) dalpha_from_slots(alpha_slots, alpha, dalpha, alpha_sign, threadIdx.x, blockDim.x);
    // one block per (n, group); coef is [3][N][C]
    const int n = blockIdx.x / groups, g = blockIdx.x % groups;
    const int gs = C / groups;
    __shared__ float s1s, s2s;
    if (threadIdx.x == 0) { s1s = 0.f; s2s = 0.f; }
    __syncthreads();
    float s1 = 0.f, s2 = 0.f;
    for (int j = threadIdx.x; j < gs; j += blockDim.x) {
        const int c = g * gs + j;
        const float A = red[((size_t)n * C + c) * 2], B = red[((size_t)n * C + c) * 2 + 1];
        s1 += gamma[c] * A;
        s2 += gamma[c] * B;
        atomic_add_f32(&dbeta[c], A);
        atomic_add_f32(&dgamma[c], B);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&s1s, s1); atomicAdd(&s2s, s2); }
    __syncthreads();
    const float mean = meanrstd[((size_t)n * groups + g) * 2], rstd = meanrstd[((size_t)n * groups + g) * 2 + 1];
    const float S1 = s1s * inv_count, S2 = s2s * inv_count;
    const size_t NC = (size_t)N * C;
    for (int j = threadIdx.x; j < gs; j += blockDim.x) {
        const int c = g * gs + j;
        coef[(size_t)n * C + c] = rstd * gamma[c];
        coef[NC + (size_t)n * C + c] = -rstd * rstd * S2;
        coef[2 * NC + (size_t)n * C + c] = mean * rstd * rstd * S2 - rstd * S1;
    }
}

extern "C" int mrisr_act_bwd_finalize(const float* red, const float* gamma, const float* meanrstd, float* dgamma,
                                      float* dbeta, float* coef, int N, int C, int groups, double count,
                                      const float* alpha_slots, const float* alpha, float* dalpha, float alpha_sign,
                                      void* stream) {
    if (!red || !gamma || !meanrstd || !dgamma || !dbeta || !coef) MRISR_FAIL(MRISR_E_ARG, "act_bwd_finalize: null pointer");
    if (groups <= 0 || C % groups) MRISR_FAIL(MRISR_E_SHAPE, "act_bwd_finalize: C %d groups %d", C, groups);
    if (alpha_slots && (!alpha || !dalpha)) MRISR_FAIL(MRISR_E_ARG, "act_bwd_finalize: alpha_slots without alpha/dalpha");
    act_bwd_finalize_kernel<<<N * groups, 64, 0, (hipStream_t)stream>>>(red, gamma, meanrstd, dgamma, dbeta, coef, N, C,
                                                                       groups, (float)(1.0 / count), alpha_slots, alpha,
                                                                       dalpha, alpha_sign);
    MRISR_CHECK_LAUNCH("act_bwd_finalize");
    return MRISR_OK;
}

// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void act_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ g,
                                                            const float* __restrict__ coef, T* __restrict__ dx, int N,
                                                            int H, int W, int C, int out_mode) {
    constexpr int VEC = Vec16<T>::N;
    const int nvec = C / VEC;
    const size_t NC = (size_t)N * C;
    const size_t total = (size_t)N * H * W * nvec;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int cv = idx % nvec;
        const size_t pix = idx / nvec;             // n*H*W + y*W + x
        const int n = pix / ((size_t)H * W);
        const int c = cv * VEC;
        const Vec16<T> xv = load_vec16(x + pix * C + c), gv = load_vec16(g + pix * C + c);
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const size_t k = (size_t)n * C + c + e;
            o.set(e, gv.get(e) * coef[k] + xv.get(e) * coef[NC + k] + coef[2 * NC + k]);
        }
        if (out_mode == MRISR_OUT_PLAIN) {
            store_vec16(dx + pix * C + c, o);
        } else {   // inverse PixelShuffle(2): (n, Y, X, c') -> (n, Y/2, X/2, 4c' + 2(Y&1) + (X&1))
            const int rem = pix - (size_t)n * H * W;
            const int Y = rem / W, X = rem - Y * W;
            T* dst = dx + (((size_t)n * (H / 2) + (Y >> 1)) * (W / 2) + (X >> 1)) * (4 * C) + 2 * (Y & 1) + (X & 1);
#pragma unroll
            for (int e = 0; e < VEC; ++e) dst[4 * (c + e)] = from_f32<T>(o.get(e));
        }
    }
}

// out_mode PIXEL_SHUFFLE2: dx is stored un-shuffled, [N][H/2][W/2][4C] with channel 4c + 2(Y&1) + (X&1).  Thread =
// one 16-byte vector of the DESTINATION (VEC/4 source channels x the 2x2 source pixels), so the stores are full
// vectors; the (n, Y, X, c) -> destination scatter of 2-byte elements ran at a third of the plain kernel's rate.
template <typename T>
__global__ __launch_bounds__(256) void act_bwd_apply_unshuffle_kernel(const T* __restrict__ x, const T* __restrict__ g,
                                                                      const float* __restrict__ coef, T* __restrict__ dx,
                                                                      int N, int H, int W, int C, float* __restrict__ dbias) {
    constexpr int VEC = Vec16<T>::N, NSC = VEC / 4;      // source channels per thread
    __shared__ float bsum[256 * VEC];
    float bs[VEC];                                       // per-thread channel sums of dx (= the conv's bias gradient)
#pragma unroll
    for (int e = 0; e < VEC; ++e) bs[e] = 0.f;
    const int H2 = H / 2, W2 = W / 2, ndv = 4 * C / VEC;
    const size_t NC = (size_t)N * C;
    const size_t total = (size_t)N * H2 * W2 * ndv;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int dv = idx % ndv;
        size_t r = idx / ndv;
        const int X2 = r % W2; r /= W2;
        const int Y2 = r % H2;
        const int n = r / H2;
        const int c0 = dv * NSC;
        Vec16<T> o;
#pragma unroll
        for (int sc = 0; sc < NSC; ++sc) {
            const size_t k = (size_t)n * C + c0 + sc;
            const float cA = coef[k], cB = coef[NC + k], cC = coef[2 * NC + k];
#pragma unroll
            for (int ij = 0; ij < 4; ++ij) {
                const size_t sp = (((size_t)n * H + 2 * Y2 + (ij >> 1)) * W + 2 * X2 + (ij & 1)) * C + c0 + sc;
                o.set(4 * sc + ij, to_f32(g[sp]) * cA + to_f32(x[sp]) * cB + cC);
            }
        }
        store_vec16(dx + idx * VEC, o);
        if (dbias) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) bs[e] += o.get(e);     // (the rounded value the weight-gradient kernel will read)
        }
    }
    if (dbias) {
        // the grid stride is a multiple of ndv (host-checked), so a thread keeps its destination vector dv = t % ndv
        const int t = threadIdx.x;
#pragma unroll
        for (int e = 0; e < VEC; ++e) bsum[t * VEC + e] = bs[e];
        __syncthreads();
        for (int i = t; i < ndv * VEC; i += 256) {
            const int dv = i / VEC, e = i - dv * VEC;
            float v = 0.f;
            for (int q = dv; q < 256; q += ndv) v += bsum[q * VEC + e];
            atomic_add_f32(&dbias[dv * VEC + e], v);
        }
    }
}

extern "C" int mrisr_act_bwd_apply(int dtype, const void* x, const void* g, const float* coef, void* dx, int N, int H,
                                   int W, int C, int out_mode, float* dbias, void* stream) {
    if (!x || !g || !coef || !dx) MRISR_FAIL(MRISR_E_ARG, "act_bwd_apply: null pointer");
    const int vec = mrisr_vec(dtype);
    if (C % vec) MRISR_FAIL(MRISR_E_SHAPE, "act_bwd_apply: C %d", C);
    if (out_mode == MRISR_OUT_PIXEL_SHUFFLE2 && ((H | W) & 1)) MRISR_FAIL(MRISR_E_SHAPE, "act_bwd_apply: odd dims with pixel shuffle");
    const size_t total = (size_t)N * H * W * (C / vec);
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (dbias && !(out_mode == MRISR_OUT_PIXEL_SHUFFLE2 && (4 * C) % vec == 0 && 256 % (4 * C / vec) == 0))
        MRISR_FAIL(MRISR_E_UNSUPPORTED, "act_bwd_apply: dbias needs the pixel-shuffle output with 4C/vec dividing 256");
    const bool unshuffle = out_mode == MRISR_OUT_PIXEL_SHUFFLE2 && (4 * C) % vec == 0;
    // with the bias gradient every block ends in 4C same-address atomics: 8192 blocks made that tail as long as
    // the pass itself (measured 298 vs 144 us) -> fewer, longer-running blocks
    const int ublocks = dbias ? (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024) : blocks;
    hipStream_t s = (hipStream_t)stream;
    const bool known = with_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (unshuffle) act_bwd_apply_unshuffle_kernel<T><<<ublocks, 256, 0, s>>>((const T*)x, (const T*)g, coef, (T*)dx, N, H, W, C, dbias);
        else act_bwd_apply_kernel<T><<<blocks, 256, 0, s>>>((const T*)x, (const T*)g, coef, (T*)dx, N, H, W, C, out_mode);
    });
    if (!known) MRISR_FAIL(MRISR_E_DTYPE, "act_bwd_apply: dtype %d", dtype);
    MRISR_CHECK_LAUNCH("act_bwd_apply");
    return MRISR_OK;
}
