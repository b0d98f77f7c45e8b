// Convolution forward / input-gradient entry points: descriptor validation and the dispatcher over the kernel families
// (ring: conv_ring.hip, producer / consumer: conv_pc.hip, 1x1 GEMM: conv1x1.hip, classic implicit GEMM: conv_igemm.h).
#include <stdlib.h>
#include <string.h>

#include "conv_common.h"

// ------------------------------------------------------------------------------------------------
int num_cus();
int conv_fill_params(const mrisr_conv_desc* d, ConvParams& p, const char* who) {
    if (!d) MRISR_FAIL(MRISR_E_ARG, "%s: null descriptor", who);
    if (!mrisr_dtype_ok(d->dtype)) MRISR_FAIL(MRISR_E_DTYPE, "%s: dtype %d", who, d->dtype);
    if (d->ksize != 1 && d->ksize != 3) MRISR_FAIL(MRISR_E_UNSUPPORTED, "%s: ksize %d", who, d->ksize);
    if (d->nsrc < 1 || d->nsrc > 2) MRISR_FAIL(MRISR_E_ARG, "%s: nsrc %d", who, d->nsrc);
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0)
        MRISR_FAIL(MRISR_E_SHAPE, "%s: bad dims N%d H%d W%d Cin%d Cout%d", who, d->N, d->H, d->W, d->Cin, d->Cout);
    const int vec = mrisr_vec(d->dtype);
    memset(&p, 0, sizeof(p));
    int csum = 0;
    for (int s = 0; s < d->nsrc; ++s) {
        const mrisr_src& a = d->src[s];
        if (!a.ptr) MRISR_FAIL(MRISR_E_ARG, "%s: src%d null", who, s);
        if (a.C % vec) MRISR_FAIL(MRISR_E_SHAPE, "%s: src%d channels %d not a multiple of %d", who, s, a.C, vec);
        if (a.mode == MRISR_SRC_NORM && (!a.scale || !a.shift)) MRISR_FAIL(MRISR_E_ARG, "%s: src%d NORM without scale/shift", who, s);
        if (s > 0 && a.spatial != MRISR_SP_NONE) MRISR_FAIL(MRISR_E_UNSUPPORTED, "%s: spatial transform on src1", who);
        if (d->nsrc > 1 && a.spatial != MRISR_SP_NONE) MRISR_FAIL(MRISR_E_UNSUPPORTED, "%s: spatial transform with 2 sources", who);
        int vh = a.H, vw = a.W;                                  // virtual extent inside the conv input
        if (a.spatial == MRISR_SP_POOL2) { vh = a.H / 2; vw = a.W / 2; }
        if (a.spatial == MRISR_SP_UP2) { vh = 2 * a.H; vw = 2 * a.W; }
        if (a.off_y < 0 || a.off_x < 0 || a.off_y + vh > d->H || a.off_x + vw > d->W)
            MRISR_FAIL(MRISR_E_SHAPE, "%s: src%d extent %dx%d (+%d,%d) exceeds conv input %dx%d", who, s, vh, vw, a.off_y, a.off_x, d->H, d->W);
        if (a.spatial == MRISR_SP_POOL2 && (vh != d->H || vw != d->W || a.off_y || a.off_x))
            MRISR_FAIL(MRISR_E_SHAPE, "%s: pooled src%d %dx%d != conv input %dx%d", who, s, vh, vw, d->H, d->W);
        if ((size_t)d->N * a.H * a.W * a.C >= (1ull << 31)) MRISR_FAIL(MRISR_E_SHAPE, "%s: src%d exceeds 2^31 elements", who, s);
        // ranges of the 24-bit / 32-bit offset arithmetic of the plain loader
        const size_t esz = d->dtype == MRISR_F32 ? 4 : 2;
        if ((size_t)a.H * a.W >= (1u << 24) || a.W >= 32768 || (size_t)a.C * esz >= (1u << 24) || (size_t)a.H * a.W * a.C * esz >= (1ull << 32))
            MRISR_FAIL(MRISR_E_SHAPE, "%s: src%d image %dx%dx%d exceeds the loader's offset range", who, s, a.H, a.W, a.C);
        p.src[s] = SrcDev{a.ptr, a.scale, a.shift, a.C, a.H, a.W, a.mode, a.off_y, a.off_x, (unsigned)((size_t)a.H * a.W * a.C * esz)};
        csum += a.C;
    }
    if (d->combine == MRISR_COMBINE_BLEND) {
        if (d->nsrc != 2 || d->src[0].C != d->src[1].C || !d->blend_alpha) MRISR_FAIL(MRISR_E_ARG, "%s: blend needs 2 equal sources + alpha", who);
        csum = d->src[0].C;
    }
    if (csum != d->Cin) MRISR_FAIL(MRISR_E_SHAPE, "%s: sources carry %d channels, Cin=%d", who, csum, d->Cin);
    const int BK = conv_bk(d->dtype), BN = conv_choose_bn(d->Cout);
    p.blend_alpha = d->blend_alpha; p.wpacked = d->wpacked; p.bias = d->bias; p.out = d->out; p.stats = d->stats;
    p.mask = d->relu_mask;
    p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.Cout = d->Cout;
    p.nchunks = ceil_div(d->Cin, BK); p.CinP = p.nchunks * BK;
    p.ncb = ceil_div(d->Cout, BN); p.CoutP = p.ncb * BN;
    p.nsrc = d->nsrc; p.combine = d->combine; p.out_mode = d->out_mode; p.groups = d->stats ? d->groups : 0;
    p.relu_out = d->relu_out;
    p.cus = d->cu_limit > 0 && d->cu_limit < num_cus() ? d->cu_limit : num_cus();
#ifdef MRISR_TUNING
    { static const int dbg_env = [] { const char* e = getenv("MRISR_DEBUG"); return e ? atoi(e) : 0; }(); p.dbg = dbg_env; }
#endif
    conv_choose_tile(d->W, p.th, p.tw_log2);
    p.tiles_x = ceil_div(d->W, 1 << p.tw_log2); p.tiles_y = ceil_div(d->H, p.th);
    return MRISR_OK;
}

// CU count of the current device (read once; one process drives one GPU - mrisr.h threading contract)
int num_cus() {
    static const int n = [] {
        int dev = 0, cus = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        return cus > 0 ? cus : 256;
    }();
    return n;
}

// conv_upadj.hip: low-resolution input gradient of bilinear x2 + conv
int conv_upadj_variant(const mrisr_conv_desc* d, char* out, size_t n);
// conv_ring.hip: the deep-ring raw-source kernel
bool conv_ring_eligible(const mrisr_conv_desc* d, const ConvParams& p);
int launch_conv_ring(const mrisr_conv_desc* d, const ConvParams& cp, hipStream_t s);
// conv_pc.hip: producer / consumer waves (GroupNorm or stored sources, 128-channel output blocks)
bool conv_pc_eligible(const mrisr_conv_desc* d, const ConvParams& p);
int conv_pc_kind(const mrisr_conv_desc* d, const ConvParams& p);
int launch_conv_pc(const mrisr_conv_desc* d, const ConvParams& cp, hipStream_t s);
// conv1x1.hip: 1x1 convolutions as a plain GEMM
bool conv1x1_gemm_eligible(const mrisr_conv_desc* d, const ConvParams& p);
int launch_conv1x1_gemm(const mrisr_conv_desc* d, const ConvParams& cp, hipStream_t s);
// conv_wgrad_rows.hip: the row-streaming weight-gradient kernel (named by mrisr_conv_variant)
bool conv_wgrad_rows_ok(const mrisr_conv_desc* d);
// conv_igemm_{bf16,f16,f32}.hip: the classic implicit-GEMM kernel, one translation unit per storage type
int launch_conv_igemm_bf16(ConvParams& p, int bn, int spatial, int ks, hipStream_t s);
int launch_conv_igemm_f16(ConvParams& p, int bn, int spatial, int ks, hipStream_t s);
int launch_conv_igemm_f32(ConvParams& p, int bn, int spatial, int ks, hipStream_t s);

#ifdef MRISR_PHASE_TIMING
// phase profile of the classic kernel (conv_igemm.h): every igemm unit has its own counters; cleared and summed here
int conv_igemm_phase_bf16(unsigned long long* out96);
int conv_igemm_phase_f16(unsigned long long* out96);
int conv_igemm_phase_f32(unsigned long long* out96);
extern "C" int mrisr_debug_phase_reset() {
    const int rc[3] = {conv_igemm_phase_bf16(nullptr), conv_igemm_phase_f16(nullptr), conv_igemm_phase_f32(nullptr)};
    return rc[0] ? rc[0] : rc[1] ? rc[1] : rc[2];
}
extern "C" int mrisr_debug_phase_cycles(unsigned long long* out96) {
    memset(out96, 0, sizeof(unsigned long long) * 96);
    const int rc[3] = {conv_igemm_phase_bf16(out96), conv_igemm_phase_f16(out96), conv_igemm_phase_f32(out96)};
    return rc[0] ? rc[0] : rc[1] ? rc[1] : rc[2];
}
#endif

// Name of the template instantiation the dispatcher picks for a descriptor (the grouping rocprofv3 reports).
extern "C" int mrisr_conv_variant(const mrisr_conv_desc* d, int wgrad, char* out, size_t n) {
    if (d && wgrad == 2) {
        if (!out || n < 8) MRISR_FAIL(MRISR_E_ARG, "conv_variant: bad buffer");
        return conv_upadj_variant(d, out, n);
    }
    ConvParams p;
    int rc = conv_fill_params(d, p, "conv_variant");
    if (rc) return rc;
    if (!out || n < 8) MRISR_FAIL(MRISR_E_ARG, "conv_variant: bad buffer");
    const char* t = d->dtype == MRISR_BF16 ? "bf16" : (d->dtype == MRISR_F16 ? "f16" : "f32");
    const int loader = d->combine == MRISR_COMBINE_BLEND ? 3 : d->src[0].spatial;
    if (wgrad && conv_wgrad_rows_ok(d)) {
        bool raw = true;
        for (int i = 0; i < d->nsrc; ++i) raw = raw && d->src[i].mode == MRISR_SRC_RAW;
        snprintf(out, n, "conv_wgrad_rows_kernel<%s,%d,%d,%d>", t, d->Cout % 64 ? 1 : 2, d->Cin % 64 ? 1 : 2, raw ? 1 : 0);
    } else if (wgrad) {
        snprintf(out, n, "conv_wgrad_kernel<%s,%d,%d,%d>", t, loader, d->ksize,
                 conv_wgrad_fast(d->dtype, loader, d->ksize, p.tw_log2, d->Cout, d->Cin));
    } else if (conv_ring_eligible(d, p)) {
        snprintf(out, n, "conv_ring_kernel<%s,2,4>", t);
    } else if (conv_pc_eligible(d, p)) {
        // (",64": the 64-channel blocks on tall tiles)
        snprintf(out, n, "conv_pc_kernel<%s,%d%s>", t, d->src[0].mode == MRISR_SRC_NORM ? 1 : 0, conv_pc_kind(d, p) == 2 ? ",64" : "");
    } else if (conv1x1_gemm_eligible(d, p)) {
        snprintf(out, n, "conv1x1_gemm_kernel<%s,%d>", t, d->src[0].mode == MRISR_SRC_NORM ? 1 : 0);
    } else {
        const int BN = conv_choose_bn(d->Cout);
        const size_t wimg = (size_t)d->ksize * d->ksize * BN * kRowBytes;
        const bool dma = conv_dma_halo(p, d->src[0].spatial);
        const int ws = conv_weights_stationary(p.nchunks, wimg, dma) ? 1 : 0;
        snprintf(out, n, "conv_igemm_kernel<%s,%d,%d,%d,%d,%d,%d>", t, BN, loader, d->ksize, ws,
                 d->out_mode == MRISR_OUT_PIXEL_SHUFFLE2 ? 1 : (d->relu_mask ? kEpiMask : 0), dma ? 1 : 0);
    }
    return MRISR_OK;
}

extern "C" int mrisr_conv_forward(const mrisr_conv_desc* d, void* stream) {
    ConvParams p;
    int rc = conv_fill_params(d, p, "conv_forward");
    if (rc) return rc;
    if (!d->wpacked || !d->out) MRISR_FAIL(MRISR_E_ARG, "conv_forward: null weights/out");
    if (d->out_mode == MRISR_OUT_PIXEL_SHUFFLE2 && (d->Cout % 16)) MRISR_FAIL(MRISR_E_SHAPE, "conv_forward: pixel shuffle needs Cout%%16==0");
    if (d->relu_mask && (d->out_mode != MRISR_OUT_PLAIN || d->Cout % (mrisr_vec(d->dtype))))
        MRISR_FAIL(MRISR_E_UNSUPPORTED, "conv_forward: relu_mask needs a plain output with Cout a multiple of the 16-byte vector");
    if (d->stats && (d->groups <= 0 || d->Cout % d->groups)) MRISR_FAIL(MRISR_E_SHAPE, "conv_forward: Cout %d not divisible by groups %d", d->Cout, d->groups);
    // the statistics are those of the SHUFFLED tensor (Cout / 4 channels): fewer channels than groups would reach the
    // stand-alone gn_stats pass with a group size of zero (Cout 16, 8 groups)
    if (d->stats && d->out_mode == MRISR_OUT_PIXEL_SHUFFLE2 && (d->Cout / 4) % d->groups)
        MRISR_FAIL(MRISR_E_SHAPE, "conv_forward: pixel shuffle leaves %d channels, not divisible by groups %d", d->Cout / 4, d->groups);
    if (conv_ring_eligible(d, p)) return launch_conv_ring(d, p, (hipStream_t)stream);
    if (conv_pc_eligible(d, p)) return launch_conv_pc(d, p, (hipStream_t)stream);
    if (conv1x1_gemm_eligible(d, p)) return launch_conv1x1_gemm(d, p, (hipStream_t)stream);
    // square 16 x 16 output tiles (324-pixel halo, 18-pixel rows) instead of 8 x 32 (340, 34): the kernels are bound by the
    // operand bytes they stage (profiles/NOTES.md R2-13/14).  32 -> 32 at 512^2: 167 -> 130 us, 64 -> 32 / 32 -> 64: 3-5 %, wide
    // layers +-2 % each, the training step -0.8 % with every 3x3 layer on 16 x 16 (A/B on one box).  The weight-gradient
    // kernel keeps 8 x 32: its fast paths are built on it.
    if (d->ksize == 3 && d->W > 16 && d->H >= 16) {
        p.th = 16; p.tw_log2 = 4;
        p.tiles_x = ceil_div(d->W, 16); p.tiles_y = ceil_div(d->H, 16);
    }
    const int sp = d->src[0].spatial;
    hipStream_t s = (hipStream_t)stream;
    const int BN = conv_choose_bn(d->Cout);
    if (d->dtype == MRISR_BF16) return launch_conv_igemm_bf16(p, BN, sp, d->ksize, s);
    if (d->dtype == MRISR_F16) return launch_conv_igemm_f16(p, BN, sp, d->ksize, s);
    return launch_conv_igemm_f32(p, BN, sp, d->ksize, s);
}
