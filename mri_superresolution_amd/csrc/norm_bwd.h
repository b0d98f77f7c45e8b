// What the GroupNorm(8,C)+LeakyReLU(0.2) backward files share (norm_bwd.hip: the two passes, norm_bwd_onepass.hip: the one-pass
// form, norm_bwd_shuffle.hip: the un-shuffled and blend-branch forms): the kernels' parameter blocks, the in-kernel finalize
// step, and the host-side checks that turn the C structs of include/mrisr.h into them.
#pragma once
#include "common.h"

struct ConsumerDev {
    const void* da;
    int C_total, c_off, H, W, spatial, off_y, off_x, weight_mode;
    const float* head_out;      // MRISR_SP_HEAD: sigmoid output, 1x1 weight, per-image partial sums [N][C+1], and the
    const float* head_w;        // head's own gradient accumulators
    float* head_part;
    float* head_dw;
    float* head_db;
};
struct ActBwdParams {
    const void* x;
    const float* scale;
    const float* shift;
    const float* meanrstd;
    const float* blend_alpha;
    void* g;
    float* red;      // [N][C][2]
    ConsumerDev cons[2];
    int ncons, N, H, W, C, groups, pix_per_block;
    int nvec_shift;  // log2(C / VEC) when that is a power of two, else -1
    float* alpha_slots;   // [256] partial sums of (first consumer's gradient) * activation, or NULL (blend alpha gradient)
};

// Pass-2 coefficients computed inside the apply kernels (mrisr_gn_bwd_fin): what act_bwd_finalize_kernel does for the
// g-tensor path, without its launch in the middle of the gradient chain.
struct FinDev {
    const float* red;        // [N][C][2], complete (written by the pass-1 launch)
    const float* gamma;
    const float* meanrstd;
    float* dgamma;
    float* dbeta;
    const float* alpha_slots;
    const float* alpha;
    float* dalpha;
    float inv_count, alpha_sign;
    int groups;
    const float* head_part;   // MRISR_SP_HEAD consumer: per-image partial sums [N][C+1] -> head_dw [C], head_db [1]
    float* head_dw;
    float* head_db;
};
constexpr int kMaxGroups = 32;

// dalpha += sign * sigmoid'(alpha) * sum d*act  (unet_model.py:206-207): the 256 slots of a blend branch, summed by the
// first wave of one block (thread t of `width`, at most 64)
__device__ __forceinline__ void dalpha_from_slots(const float* alpha_slots, const float* alpha, float* dalpha, float alpha_sign, int t, int width) {
    float v = 0.f;
    for (int i = t; i < 256; i += width) v += alpha_slots[i];
    v = wave_sum(v);
    if (t == 0) {
        const float sg = 1.f / (1.f + __expf(-alpha[0]));
        atomic_add_f32(dalpha, alpha_sign * sg * (1.f - sg) * v);
    }
}

// sum g*x -> sum g*xhat = rstd * (sum g*x - mean * sum g) for a thread's sums of channels c .. c+VEC-1 of image n (a few
// pixels each: no cancellation to speak of); the group statistics are only needed here, so they stay out of the streaming
// loops' register budget
template <int VEC>
__device__ __forceinline__ void sums_to_xhat(const float* meanrstd, int n, int groups, int gs, int c, const float* sA, float* sB) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int g = (c + e) / gs;
        const float mean = meanrstd[((size_t)n * groups + g) * 2], rstd = meanrstd[((size_t)n * groups + g) * 2 + 1];
        sB[e] = rstd * (sB[e] - mean * sA[e]);
    }
}

// Every thread of the block calls this (two barriers inside).  s12 = 2 * kMaxGroups floats of LDS.  Fills the
// coefficients of channels c .. c+VEC-1 of image n (see act_bwd_finalize_kernel for the formulas); the block with
// `owner` set adds image n's share to dgamma / dbeta for the channels its threads with `lead` set hold, and the block
// with `first` set turns the blend-alpha slots into dalpha.
template <int VEC>
__device__ __forceinline__ void gn_bwd_coefs(const FinDev& f, float* s12, int n, int C, int c, bool valid, bool owner,
                                             bool lead, bool first, float* ca, float* cb, float* cc) {
    const int t = threadIdx.x, gs = C / f.groups;
    if (t < 2 * kMaxGroups) s12[t] = 0.f;
    __syncthreads();
    const float* rn = f.red + (size_t)n * C * 2;
    for (int j = t; j < C; j += blockDim.x) {
        const float gm = f.gamma[j];
        atomicAdd(&s12[j / gs], gm * rn[2 * j]);
        atomicAdd(&s12[kMaxGroups + j / gs], gm * rn[2 * j + 1]);
    }
    __syncthreads();
    if (valid) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int g = (c + e) / gs;
            const float mean = f.meanrstd[((size_t)n * f.groups + g) * 2], rstd = f.meanrstd[((size_t)n * f.groups + g) * 2 + 1];
            const float S1 = s12[g] * f.inv_count, S2 = s12[kMaxGroups + g] * f.inv_count;
            ca[e] = rstd * f.gamma[c + e];
            cb[e] = -rstd * rstd * S2;
            cc[e] = mean * rstd * rstd * S2 - rstd * S1;
            if (owner && lead) {
                atomic_add_f32(&f.dbeta[c + e], rn[2 * (c + e)]);
                atomic_add_f32(&f.dgamma[c + e], rn[2 * (c + e) + 1]);
                if (f.head_part) atomic_add_f32(&f.head_dw[c + e], f.head_part[(size_t)n * (C + 1) + c + e]);
            }
        }
        if (owner && lead && f.head_part && c == 0) atomic_add_f32(f.head_db, f.head_part[(size_t)n * (C + 1) + C]);
    }
    if (first && f.alpha_slots && t < 64) dalpha_from_slots(f.alpha_slots, f.alpha, f.dalpha, f.alpha_sign, t, 64);
}

template <typename T>
__device__ __forceinline__ void act_of(const T* p, const float* sc, const float* sh, float* o) {
    const Vec16<T> v = load_vec16(p);
#pragma unroll
    for (int e = 0; e < Vec16<T>::N; ++e) o[e] = lrelu(v.get(e) * sc[e] + sh[e]);
}

// window kernels apply when: one 2x2-pool consumer, even H and W, and the optional second consumer is plain with the
// node's own geometry
static inline bool act_bwd_window_ok(int nconsumers, const mrisr_consumer* cs, int H, int W) {
    if ((H | W) & 1) return false;
    int npool = 0;
    for (int k = 0; k < nconsumers; ++k) {
        if (cs[k].spatial == MRISR_SP_POOL2) ++npool;
        else if (cs[k].spatial != MRISR_SP_NONE || cs[k].H != H || cs[k].W != W || cs[k].off_y || cs[k].off_x) return false;
    }
    return npool == 1;
}

// MRISR_SP_HEAD: the only consumer, same geometry as the node, no blend weight
static inline int check_head_consumer(int nconsumers, const mrisr_consumer* cs, int H, int W, int C, bool reduce, const char* who) {
    bool head = false;
    for (int k = 0; k < nconsumers; ++k) head = head || cs[k].spatial == MRISR_SP_HEAD;
    if (!head) return MRISR_OK;
    const mrisr_consumer& c = cs[0];
    if (nconsumers != 1 || c.H != H || c.W != W || c.off_y || c.off_x || c.weight_mode || c.c_off || c.C_total != C)
        MRISR_FAIL(MRISR_E_ARG, "%s: a head consumer is the only consumer and has the node's geometry", who);
    if (!c.head_out || !c.head_w || !c.head_part || (!reduce && (!c.head_dw || !c.head_db))) MRISR_FAIL(MRISR_E_ARG, "%s: head consumer null pointer", who);
    return MRISR_OK;
}

static inline int fill_act_bwd_params(ActBwdParams& p, int dtype, int nconsumers, const mrisr_consumer* consumers,
                                      const float* blend_alpha, int H, int W, int C, const char* who) {
    const int vec = mrisr_vec(dtype);
    for (int k = 0; k < nconsumers; ++k) {
        const mrisr_consumer& c = consumers[k];
        if (!c.da) MRISR_FAIL(MRISR_E_ARG, "%s: consumer %d null", who, k);
        if (c.weight_mode < 0 || c.weight_mode > 2 || (c.weight_mode && !blend_alpha)) MRISR_FAIL(MRISR_E_ARG, "%s: weight_mode", who);
        if (c.c_off % vec || c.C_total % vec || c.c_off + C > c.C_total) MRISR_FAIL(MRISR_E_SHAPE, "%s: consumer %d channels", who, k);
        if (c.spatial == MRISR_SP_UP2 && (c.off_y + 2 * H > c.H || c.off_x + 2 * W > c.W)) MRISR_FAIL(MRISR_E_SHAPE, "%s: consumer %d UP2 extent", who, k);
        if (c.spatial == MRISR_SP_POOL2 && (c.H != H / 2 || c.W != W / 2)) MRISR_FAIL(MRISR_E_SHAPE, "%s: consumer %d POOL2 extent", who, k);
        p.cons[k] = ConsumerDev{c.da, c.C_total, c.c_off, c.H, c.W, c.spatial, c.off_y, c.off_x, c.weight_mode, c.head_out, c.head_w, c.head_part, c.head_dw, c.head_db};
    }
    return MRISR_OK;
}

// A mrisr_gn_bwd_fin, checked and in the kernels' form (the head fields stay NULL: mrisr_act_bwd_apply_fused sets them).
// `who` names the entry and the fin ("act_bwd_apply_fused: fin").  with_alpha = false: the entry takes no blend branch -
// the alpha fields are neither checked nor passed on (the entry refuses a fin that sets them, after these checks).
static inline int make_fin_dev(FinDev& fd, const mrisr_gn_bwd_fin* fin, int C, const char* who, bool with_alpha = true) {
    if (!fin->red || !fin->gamma || !fin->meanrstd || !fin->dgamma || !fin->dbeta) MRISR_FAIL(MRISR_E_ARG, "%s null pointer", who);
    if (fin->groups <= 0 || fin->groups > kMaxGroups || C % fin->groups) MRISR_FAIL(MRISR_E_SHAPE, "%s groups %d", who, fin->groups);
    if (!(fin->count > 0)) MRISR_FAIL(MRISR_E_SHAPE, "%s count", who);
    if (with_alpha && fin->alpha_slots && (!fin->alpha || !fin->dalpha)) MRISR_FAIL(MRISR_E_ARG, "%s alpha_slots without alpha/dalpha", who);
    fd = FinDev{fin->red, fin->gamma, fin->meanrstd, fin->dgamma, fin->dbeta, with_alpha ? fin->alpha_slots : nullptr,
                with_alpha ? fin->alpha : nullptr, with_alpha ? fin->dalpha : nullptr,
                (float)(1.0 / fin->count), fin->alpha_sign, fin->groups, nullptr, nullptr, nullptr};
    return MRISR_OK;
}
