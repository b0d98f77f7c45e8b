#include "norm_bwd.h"

// ------------------------------------------------------------------------------------------------
// ONE-PASS GroupNorm + LeakyReLU backward (plain consumers with the node's own geometry, 16-bit storage): what
// act_bwd_reduce_kernel<T,0> + act_bwd_apply_fused_kernel<T,true> do in two launches that each read x and every consumer
// gradient from HBM (5 tensor passes for one consumer, 7 for two), in one launch that reads them ONCE (3 / 4 passes):
// a block keeps its pixels' x and consumer-gradient vectors in registers across the reduction.
//   phase 1: per-(n,c) sums of g and g*xhat of the block's pixels -> atomics into red[n][c][2] (as the reduce kernel), and the
//            block's gamma-weighted GROUP sums -> atomics into the image's table of 2 * groups floats behind the barrier words
//   image barrier: the blocks of image n count themselves in arrive[n] and wait until all of them have
//   phase 2: coefficients from the image's group sums (gn_bwd_coefs' formulas), dx from the registers
//   afterwards: the block that completed the image's count turns red[n] into the image's share of dgamma / dbeta
// Only the group sums cross the barrier: dx = g cA + x cB + cC needs S1 and S2 of the group and nothing per channel (cA is
// local), so a block reads 16 x 2 * groups words after the barrier, not 16 x 2 C.
// The barrier is safe because the workgroups of a 2-D grid start in linear order (x fastest): the blocks of image n are
// all dispatched before any block of image n+1, so the ones a waiting block needs are resident or next in line - as long
// as ONE image's blocks fit on the chip together, which the host guarantees with a wide margin (<= 256 blocks of 256
// threads per image against >= 480 resident ones with the weight-gradient stream holding its share of the CUs).  A block
// that waits unreasonably long (~0.3 s) gives up and poisons its output with NaN: a broken assumption must neither hang the
// GPU nor pass silently.
constexpr int kOnePassPPT = 8;       // pixels per thread
constexpr int kOnePassMaxBlocks = 256;
// the per-(n,c) sums are spread over this many copies of red[] (block index mod kOnePassSlots): the blocks of an image all
// add into the same C x 2 words right before they wait for each other, and 256 same-address atomics in a row (performed at
// the memory side) took ~25 us per image
// (an image of fewer blocks uses as many copies as it has blocks: block index mod min(kOnePassSlots, blocks per image))
constexpr int kOnePassSlots = 16;
constexpr int kOnePassGroups = 16;      // block groups of the image barrier
constexpr int kOnePassSyncWords = 544;  // barrier words per image: 16 group counters, the image counter, 16 group flags - 64 bytes apart
// behind them the image's table of gamma-weighted group sums, float [kOnePassSlots][kOnePassTabStride]: a copy holds
// sum gamma g of the groups, then sum gamma g xhat of the groups (2 * groups <= 2 * kMaxGroups words, 256 bytes apart).  Zero
// on entry like the rest (0u reads as 0.0f), and on cache lines of the image's own (2176 + 4096 bytes per image).
constexpr int kOnePassTabStride = 2 * kMaxGroups;
constexpr int kOnePassWords = kOnePassSyncWords + kOnePassSlots * kOnePassTabStride;

// Phase profile (timing builds only: tools/build_src_variant.sh NAME norm_bwd_onepass.hip -DMRISR_ONEPASS_PT, read by tools/gn_bwd_bench.py;
// never compiled into libmrisr.so): s_memtime stamps around the parts of a launch - 0 loads + sums, 1 block reduction + atomics until the
// block may be counted, 2 the wait at the image barrier, 3 barrier -> coefficients, 4 the dx stores, 5 the dgamma / dbeta share - taken by
// thread 0 of the middle block of the middle image; every stamp first waits for the thread's outstanding memory operations.
struct OnePassPT {
#ifdef MRISR_ONEPASS_PT
    unsigned long long t, acc[6];
    __device__ __forceinline__ void start() {
        for (int k = 0; k < 6; ++k) acc[k] = 0;
        t = __builtin_amdgcn_s_memtime();
    }
    __device__ __forceinline__ void mark(int k) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        acc[k] += now - t;
        t = now;
    }
    __device__ __forceinline__ void flush();
#else
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void flush() {}
#endif
};
#ifdef MRISR_ONEPASS_PT
static __device__ unsigned long long g_onepass_cycles[8];      // the six parts, -, launches
__device__ __forceinline__ void OnePassPT::flush() {
    if (threadIdx.x == 0 && blockIdx.x == gridDim.x / 2 && blockIdx.y == gridDim.y / 2) {
        for (int k = 0; k < 6; ++k) atomicAdd(&g_onepass_cycles[k], acc[k]);
        atomicAdd(&g_onepass_cycles[7], 1ull);
    }
}
// out8 == NULL: reset
extern "C" int mrisr_debug_onepass_cycles(unsigned long long* out8) {
    unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!out8) return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_onepass_cycles), v, sizeof(v));
    const int rc = (int)hipMemcpyFromSymbol(v, HIP_SYMBOL(g_onepass_cycles), sizeof(v));
    for (int k = 0; k < 8; ++k) out8[k] = v[k];
    return rc;
}
#endif

__device__ __forceinline__ float ld_coherent(const float* p) {      // red[] is written by other blocks of THIS launch
    return __hip_atomic_load((const GLOBAL_AS float*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The part every one-pass kernel shares.  In: this thread's sums of g (sA) and g*x (sB) over its pixels, channels c .. c+VEC-1 of
// image n.  Block reduction -> atomics into this block's copy of red[] (per channel: for dgamma / dbeta, read by nobody here) and
// into its copy of the image's group table (the block's sum gamma g and sum gamma g xhat per group) -> image barrier ->
// coefficients of dx = g cA + x cB + cC for the thread's channels (act_bwd_finalize_kernel's formulas) from the group table.
// Every thread of the block calls it.  lds: 256 * VEC * 2 + 2 * kMaxGroups floats.  state (LDS): bit 0 the block gave up
// waiting, bit 1 the block completed the image's count (it owes the image's onepass_affine_grads).
template <int VEC>
__device__ __forceinline__ void onepass_meet(const ActBwdParams& p, const FinDev& fin, unsigned* __restrict__ arrive, float* lds,
                                             int* state, int n, int c, int nvec, int ppb, float* sA, float* sB,
                                             float* ca, float* cb, float* cc, OnePassPT& pt) {
    // (groups is a power of two - the entry point checks it - and so is C / 8, hence the group size: shifts, not divisions,
    // next to 130 live registers)
    const int t = threadIdx.x, gs = p.C / p.groups, gs_sh = __ffs(gs) - 1, g2 = 2 * p.groups, g2_sh = __ffs(g2) - 1;
    const int nslots = min((int)gridDim.x, kOnePassSlots), slot = blockIdx.x % nslots;
    unsigned* img = arrive + (size_t)n * kOnePassWords;
    float* tab = (float*)(img + kOnePassSyncWords);      // [kOnePassSlots][kOnePassTabStride]
    float* part = lds + 256 * VEC * 2;                   // [2][groups]: this block's gamma-weighted group sums
    sums_to_xhat<VEC>(p.meanrstd, n, p.groups, gs, c, sA, sB);      // per thread (8 pixels)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        lds[(t * VEC + e) * 2] = sA[e];
        lds[(t * VEC + e) * 2 + 1] = sB[e];
    }
    if (t < 2 * kMaxGroups) part[t] = 0.f;
    if (t == 0) *state = 0;
    __syncthreads();
    for (int i = t; i < nvec * VEC * 2; i += 256) {
        const int j = i >> 1, which = i & 1;
        const int cvj = j / VEC, e = j - cvj * VEC;
        float s = 0.f;
        for (int q = 0; q < ppb; ++q) s += lds[((q * nvec + cvj) * VEC + e) * 2 + which];
        atomicAdd(&part[which * p.groups + (j >> gs_sh)], fin.gamma[j] * s);
        lds[i] = s;      // row 0 of the column only this thread reads: kept for the red[] atomics below
    }
    __syncthreads();
    // The group table first, then red[]: no load stands behind an atomic (vmcnt counts in order, so the wait for a gamma load
    // issued after an atomic is a wait for that atomic's acknowledgement), and all of them are in flight together.
    if (t < g2) atomic_add_f32(&tab[slot * kOnePassTabStride + t], part[t]);
    for (int i = t; i < nvec * VEC * 2; i += 256) atomic_add_f32(&p.red[((size_t)slot * p.N + n) * p.C * 2 + i], lds[i]);
    // ---- image barrier.  Everything that crosses it goes through agent-scope RELAXED atomics (the sums above, the counter,
    // the reads of the group table below), which are performed at the memory side: no release / acquire fences - on this
    // multi-XCD part each of them writes back or invalidates a whole L2, and with 4096 blocks doing so the launch ran 8x
    // slower than the two launches it replaces.  `s_waitcnt vmcnt(0)`: this thread's atomics - group table AND red[], which
    // the image's last block reads once it has seen everybody counted - have been acknowledged before it is counted.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    pt.mark(1);
    if (t == 0) {
        // Two-level count, then a release flag per group of blocks: 256 blocks bumping and then polling ONE word is a chain of
        // 256 same-address atomics at the memory side (~40 us per image, measured).  Block b belongs to group b % 16: it bumps
        // its group's counter; the block that completes a group bumps the image's counter; the block that completes the image
        // sets the 16 group flags; everybody polls its own group's flag (16 pollers per word, one cache line per word).
        const unsigned nblk = gridDim.x, g = blockIdx.x % kOnePassGroups;
        const unsigned ngroups = min(nblk, (unsigned)kOnePassGroups), members = (nblk - g + kOnePassGroups - 1) / kOnePassGroups;
        if (__hip_atomic_fetch_add(img + g * 16, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == members) {
            if (__hip_atomic_fetch_add(img + 256, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == ngroups) {
                for (unsigned k = 0; k < ngroups; ++k)
                    __hip_atomic_store(img + 272 + k * 16, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                *state |= 2;
            }
        }
        int spin = 0;
        while (__hip_atomic_load(img + 272 + g * 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
            __builtin_amdgcn_s_sleep(16);      // ~0.5 us between polls
            if (++spin > 600000) { *state |= 1; break; }
        }
    }
    asm volatile("" ::: "memory");
    __syncthreads();
    const bool bad = (*state & 1) != 0;
    pt.mark(2);

    // ---- coefficients of image n (act_bwd_finalize_kernel's formulas; the table read around the L1): the copies in use,
    // one word per thread at the network's 8 groups, added up in copy order
    float* s12 = part;
    for (int i = t; i < nslots * g2; i += 256) {
        lds[i] = ld_coherent(tab + (i >> g2_sh) * kOnePassTabStride + (i & (g2 - 1)));
    }
    __syncthreads();
    if (t < g2) {
        float v = 0.f;
        for (int sl = 0; sl < nslots; ++sl) v += lds[sl * g2 + t];
        s12[t] = v;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int g = (c + e) >> gs_sh;
        const float mean = fin.meanrstd[((size_t)n * fin.groups + g) * 2], rstd = fin.meanrstd[((size_t)n * fin.groups + g) * 2 + 1];
        const float S1 = s12[g] * fin.inv_count, S2 = s12[fin.groups + g] * fin.inv_count;
        ca[e] = rstd * fin.gamma[c + e];
        cb[e] = -rstd * rstd * S2;
        cc[e] = bad ? __builtin_nanf("") : mean * rstd * rstd * S2 - rstd * S1;
    }
    pt.mark(3);
}

// After the block's dx stores: the block that completed image n's count (every block's red[] atomics had been acknowledged
// before it was counted) adds the image's share of dgamma / dbeta - the per-channel sums of all copies in use.  Nobody waits
// for it.  Every thread of the block calls it.
__device__ __forceinline__ void onepass_affine_grads(const ActBwdParams& p, const FinDev& fin, const int* state, int n) {
    if (!(*state & 2)) return;
    const int nslots = min((int)gridDim.x, kOnePassSlots);
    const float* rn = fin.red + (size_t)n * p.C * 2;
    const size_t slot_stride = (size_t)p.N * p.C * 2;
    for (int j = threadIdx.x; j < 2 * p.C; j += 256) {
        float v = 0.f;
        if (nslots == kOnePassSlots) {      // all 16 loads in flight together: this block is the tail of the image
#pragma unroll
            for (int sl = 0; sl < kOnePassSlots; ++sl) v += ld_coherent(rn + sl * slot_stride + j);
        } else {
            for (int sl = 0; sl < nslots; ++sl) v += ld_coherent(rn + sl * slot_stride + j);
        }
        atomic_add_f32(((j & 1) ? fin.dgamma : fin.dbeta) + (j >> 1), v);
    }
}

template <typename T, int NCONS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void act_bwd_onepass_kernel(const ActBwdParams p, T* __restrict__ dx, const FinDev fin,
                                                              unsigned* __restrict__ arrive) {
    constexpr int VEC = Vec16<T>::N, PPT = kOnePassPPT;
    __shared__ float lds[256 * VEC * 2 + 2 * kMaxGroups];
    __shared__ int meet_state;
    const int t = threadIdx.x, n = blockIdx.y;
    OnePassPT pt;
    pt.start();
    const int nvec = p.C / VEC, ppb = 256 / nvec;             // host-checked: nvec is a power of two <= 256
    const int cv = t & (nvec - 1), pl = t / nvec, c = cv * VEC;
    const int HW = p.H * p.W, gs = p.C / p.groups;
    const int pix0 = blockIdx.x * (ppb * PPT) + pl;

    float sc[VEC], sh[VEC];
    const size_t k0 = (size_t)n * p.C + c;
#pragma unroll
    for (int e = 0; e < VEC; ++e) { sc[e] = p.scale[k0 + e]; sh[e] = p.shift[k0 + e]; }
    const T* xb = (const T*)p.x + (size_t)n * HW * p.C + c;
    const T* d0b = (const T*)p.cons[0].da + (size_t)n * HW * p.cons[0].C_total + p.cons[0].c_off + c;
    const T* d1b = NCONS > 1 ? (const T*)p.cons[1].da + (size_t)n * HW * p.cons[1].C_total + p.cons[1].c_off + c : d0b;
    const int ct0 = p.cons[0].C_total, ct1 = NCONS > 1 ? p.cons[1].C_total : ct0;

    // ---- phase 1: everything this thread will need, loaded once
    Vec16<T> xv[PPT], d0[PPT], d1[NCONS > 1 ? PPT : 1];
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const int pix = min(pix0 + i * ppb, HW - 1);          // (the tail block re-reads the last pixel; masked below)
        xv[i] = load_vec16(xb + (size_t)pix * p.C);
        d0[i] = load_vec16(d0b + (size_t)pix * ct0);
        if (NCONS > 1) d1[i] = load_vec16(d1b + (size_t)pix * ct1);
    }
    float sA[VEC], sB[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { sA[e] = 0.f; sB[e] = 0.f; }
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        if (pix0 + i * ppb < HW) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float xr = xv[i].get(e);
                const float pre = xr * sc[e] + sh[e];
                const float ga = NCONS > 1 ? d0[i].get(e) + d1[i].get(e) : d0[i].get(e);
                const float gy = ga * (pre > 0.f ? 1.f : LRELU_SLOPE);
                sA[e] += gy;
                sB[e] += gy * xr;
            }
        }
    }
    float ca[VEC], cb[VEC], cc[VEC];
    pt.mark(0);
    onepass_meet<VEC>(p, fin, arrive, lds, &meet_state, n, c, nvec, ppb, sA, sB, ca, cb, cc, pt);
    T* ob = dx + (size_t)n * HW * p.C + c;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const int pix = pix0 + i * ppb;
        if (pix < HW) {
            Vec16<T> o;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float xr = xv[i].get(e);
                const float pre = xr * sc[e] + sh[e];
                const float ga = NCONS > 1 ? d0[i].get(e) + d1[i].get(e) : d0[i].get(e);
                const float gy = ga * (pre > 0.f ? 1.f : LRELU_SLOPE);
                o.set(e, gy * ca[e] + xr * cb[e] + cc[e]);
            }
            store_vec16(ob + (size_t)pix * p.C, o);
        }
    }
    pt.mark(4);
    onepass_affine_grads(p, fin, &meet_state, n);
    pt.mark(5);
    pt.flush();
}

// The same for a node whose activation is ALSO max-pooled (the encoder skips: one 2x2-pool consumer + at most one plain
// consumer of the node's geometry; even H, W).  Thread = (pooled pixel, channel vector) owning whole 2x2 windows as in
// act_bwd_pool_window_kernel: two windows per thread = 8 pixels' x, their plain-consumer gradients and two pooled gradients
// in registers across the barrier; the arg-max is recomputed in phase 2 (a few vector instructions per element).
constexpr int kOnePassWPT = 2;       // windows per thread
template <typename T, bool HAS_O>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void act_bwd_onepass_window_kernel(const ActBwdParams p, T* __restrict__ dx,
                                                                                                                  const FinDev fin, unsigned* __restrict__ arrive) {
    constexpr int VEC = Vec16<T>::N, WPT = kOnePassWPT;
    __shared__ float lds[256 * VEC * 2 + 2 * kMaxGroups];
    __shared__ int meet_state;
    const int t = threadIdx.x, n = blockIdx.y;
    OnePassPT pt;
    pt.start();
    const int nvec = p.C / VEC, ppb = 256 / nvec;
    const int cv = t & (nvec - 1), pl = t / nvec, c = cv * VEC;
    const int W = p.W, Hp = p.H / 2, Wp = W / 2, HWp = Hp * Wp;
    const int kp = p.cons[0].spatial == MRISR_SP_POOL2 ? 0 : 1, ko = 1 - kp;
    const int w0 = blockIdx.x * (ppb * WPT) + pl;
    float sc[VEC], sh[VEC];
    const size_t k0 = (size_t)n * p.C + c;
#pragma unroll
    for (int e = 0; e < VEC; ++e) { sc[e] = p.scale[k0 + e]; sh[e] = p.shift[k0 + e]; }
    const T* xb = (const T*)p.x + (size_t)n * p.H * W * p.C + c;
    const T* dpb = (const T*)p.cons[kp].da + (size_t)n * HWp * p.cons[kp].C_total + p.cons[kp].c_off + c;
    const int Cto = HAS_O ? p.cons[ko].C_total : 0;
    const T* dob = HAS_O ? (const T*)p.cons[ko].da + (size_t)n * p.H * W * Cto + p.cons[ko].c_off + c : xb;

    Vec16<T> xv[WPT][4], dv[HAS_O ? WPT : 1][4], dp[WPT];
    unsigned off[WPT];                  // pixel index of the window's top-left corner
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
        const int pp = min(w0 + i * ppb, HWp - 1);              // (the tail block re-reads the last window; masked below)
        const int py = pp / Wp, px = pp - py * Wp;
        off[i] = (unsigned)(2 * py) * W + 2 * px;
        const unsigned o4[4] = {off[i], off[i] + 1, off[i] + (unsigned)W, off[i] + (unsigned)W + 1};
#pragma unroll
        for (int q = 0; q < 4; ++q) xv[i][q] = load_vec16(xb + (size_t)o4[q] * p.C);
        dp[i] = load_vec16(dpb + (size_t)pp * p.cons[kp].C_total);
        if (HAS_O) {
#pragma unroll
            for (int q = 0; q < 4; ++q) dv[i][q] = load_vec16(dob + (size_t)o4[q] * Cto);
        }
    }
    // gradient w.r.t. the GroupNorm output at the four pixels of window i, channel e (act_bwd_pool_window_kernel's arithmetic:
    // first maximum of the activations in scan order takes the pooled gradient)
    auto window_g = [&](int i, int e, float* xr, float* gy) {
        float pre[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { xr[q] = xv[i][q].get(e); pre[q] = xr[q] * sc[e] + sh[e]; }
        int win = 0;
        float m = lrelu(pre[0]);
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            const float a = lrelu(pre[q]);
            if (a > m) { m = a; win = q; }
        }
        const float gp = dp[i].get(e);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float gact = q == win ? gp : 0.f;
            if (HAS_O) gact += dv[i][q].get(e);
            gy[q] = gact * (pre[q] > 0.f ? 1.f : LRELU_SLOPE);
        }
    };
    float sA[VEC], sB[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { sA[e] = 0.f; sB[e] = 0.f; }
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
        if (w0 + i * ppb < HWp) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                float xr[4], gy[4];
                window_g(i, e, xr, gy);
#pragma unroll
                for (int q = 0; q < 4; ++q) { sA[e] += gy[q]; sB[e] += gy[q] * xr[q]; }
            }
        }
    }
    float ca[VEC], cb[VEC], cc[VEC];
    pt.mark(0);
    onepass_meet<VEC>(p, fin, arrive, lds, &meet_state, n, c, nvec, ppb, sA, sB, ca, cb, cc, pt);
    T* ob = dx + (size_t)n * p.H * W * p.C + c;
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
        if (w0 + i * ppb < HWp) {
            Vec16<T> ov[4];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                float xr[4], gy[4];
                window_g(i, e, xr, gy);
#pragma unroll
                for (int q = 0; q < 4; ++q) ov[q].set(e, gy[q] * ca[e] + xr[q] * cb[e] + cc[e]);
            }
            const unsigned o4[4] = {off[i], off[i] + 1, off[i] + (unsigned)W, off[i] + (unsigned)W + 1};
#pragma unroll
            for (int q = 0; q < 4; ++q) store_vec16(ob + (size_t)o4[q] * p.C, ov[q]);
        }
    }
    pt.mark(4);
    onepass_affine_grads(p, fin, &meet_state, n);
    pt.mark(5);
    pt.flush();
}

// Does a node qualify for the one-pass kernel?  (16-bit storage, plain consumers of the node's own geometry without blend
// weights, C / 8 a power of two <= 256, at most kOnePassMaxBlocks blocks per image)
// 0 = no, 1 = plain consumers (act_bwd_onepass_kernel), 2 = one 2x2-pool consumer (+ at most one plain one): window kernel
extern "C" int mrisr_act_bwd_onepass_ok(int dtype, int nconsumers, const mrisr_consumer* consumers, int N, int H, int W, int C) {
    if (dtype != MRISR_BF16 && dtype != MRISR_F16) return 0;
    if (!consumers || nconsumers < 1 || nconsumers > 2 || N < 1) return 0;
    const int vec = mrisr_vec(dtype);
    if (C % vec) return 0;
    const int nvec = C / vec;
    if (nvec > 256 || (nvec & (nvec - 1))) return 0;
    const long HW = (long)H * W;
    if (HW * C >= (1l << 30)) return 0;
    bool plain = true;
    for (int k = 0; k < nconsumers; ++k) {
        const mrisr_consumer& c = consumers[k];
        if (c.weight_mode) return 0;
        if (c.spatial != MRISR_SP_NONE || c.H != H || c.W != W || c.off_y || c.off_x) plain = false;
    }
    if (plain) {
        const int ppblk = (256 / nvec) * kOnePassPPT;
        return (HW + ppblk - 1) / ppblk <= kOnePassMaxBlocks ? 1 : 0;
    }
    if (!act_bwd_window_ok(nconsumers, consumers, H, W)) return 0;
    for (int k = 0; k < nconsumers; ++k)
        if (consumers[k].spatial == MRISR_SP_POOL2 && (consumers[k].H != H / 2 || consumers[k].W != W / 2)) return 0;
    const int wpblk = (256 / nvec) * kOnePassWPT;
    return (HW / 4 + wpblk - 1) / wpblk <= kOnePassMaxBlocks ? 2 : 0;
}

// red: [kOnePassSlots = 16][N][C][2] floats and arrive: [N][kOnePassWords = 1568] words (barrier words + group table), both ZERO on entry (the engine's per-backward arena).
extern "C" int mrisr_act_bwd_onepass_slots(void) { return kOnePassSlots; }
extern "C" int mrisr_act_bwd_onepass_barrier_words(void) { return kOnePassWords; }
extern "C" int mrisr_act_bwd_onepass(int dtype, const void* x, const float* scale, const float* shift, const float* meanrstd,
                                     int nconsumers, const mrisr_consumer* consumers, float* red, unsigned* arrive,
                                     const mrisr_gn_bwd_fin* fin, void* dx, int N, int H, int W, int C, void* stream) {
    if (!x || !scale || !shift || !meanrstd || !consumers || !red || !arrive || !fin || !dx) MRISR_FAIL(MRISR_E_ARG, "act_bwd_onepass: null pointer");
    if (!mrisr_act_bwd_onepass_ok(dtype, nconsumers, consumers, N, H, W, C))
        MRISR_FAIL(MRISR_E_UNSUPPORTED, "act_bwd_onepass: node does not qualify (mrisr_act_bwd_onepass_ok)");
    if (fin->red != red) MRISR_FAIL(MRISR_E_ARG, "act_bwd_onepass: fin->red is not red");
    FinDev fd;
    int frc = make_fin_dev(fd, fin, C, "act_bwd_onepass: fin", false);
    if (frc) return frc;
    if (fin->alpha_slots) MRISR_FAIL(MRISR_E_UNSUPPORTED, "act_bwd_onepass: blend branches take the two-pass kernels");
    // onepass_meet indexes the group table with shifts and masks.  (groups divides C and C / 8 is a power of two, so this
    // holds for every node that qualifies today; checked on its own so that relaxing either rule cannot corrupt the table.)
    if (fin->groups & (fin->groups - 1)) MRISR_FAIL(MRISR_E_UNSUPPORTED, "act_bwd_onepass: groups %d is not a power of two", fin->groups);
    ActBwdParams p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.scale = scale; p.shift = shift; p.meanrstd = meanrstd; p.red = red;
    p.ncons = nconsumers; p.N = N; p.H = H; p.W = W; p.C = C; p.groups = fin->groups;
    int rc = fill_act_bwd_params(p, dtype, nconsumers, consumers, nullptr, H, W, C, "act_bwd_onepass");
    if (rc) return rc;
    const int kind = mrisr_act_bwd_onepass_ok(dtype, nconsumers, consumers, N, H, W, C);
    const int nvec = C / mrisr_vec(dtype);
    hipStream_t s = (hipStream_t)stream;
    // every lane takes its whole share at once (the operands stay in registers): no pixel blocking beyond the grid
    const dim3 grid(kind == 2 ? ceil_div(H * W / 4, (256 / nvec) * kOnePassWPT) : ceil_div(H * W, (256 / nvec) * kOnePassPPT), N);
    with_dtype16(dtype, [&](auto tag) {      // (16-bit storage: mrisr_act_bwd_onepass_ok)
        using T = typename decltype(tag)::type;
        if (kind == 2) {
            if (nconsumers > 1) act_bwd_onepass_window_kernel<T, true><<<grid, 256, 0, s>>>(p, (T*)dx, fd, arrive);
            else act_bwd_onepass_window_kernel<T, false><<<grid, 256, 0, s>>>(p, (T*)dx, fd, arrive);
        } else if (nconsumers == 1) act_bwd_onepass_kernel<T, 1><<<grid, 256, 0, s>>>(p, (T*)dx, fd, arrive);
        else act_bwd_onepass_kernel<T, 2><<<grid, 256, 0, s>>>(p, (T*)dx, fd, arrive);
    });
    MRISR_CHECK_LAUNCH(kind == 2 ? "act_bwd_onepass(window)" : "act_bwd_onepass");
    return MRISR_OK;
}
