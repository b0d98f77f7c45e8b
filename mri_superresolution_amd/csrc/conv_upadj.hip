// Input gradient of final_up_bilinear (bilinear x2, align_corners=True, then a 3x3 conv f -> f/2; unet_model.py:151-152)
// computed at LOW resolution.
//
// With U the bilinear x2, W_t the Cout x Cin matrix of tap t = (ky-1, kx-1) and g = dL/d(conv output) [N][2h][2w][Cout]:
//     d_a(q) = sum_P U[P, q] * sum_t W_t^T g(P - t) = sum_t W_t^T h_t(q),     h_t(q) = sum_P U[P, q] g(P - t)
// (channel mixing commutes with the per-channel spatial operator U^T).  h has 9 * Cout channels at h x w, so the
// input gradient is a K = 9 * Cout GEMM at low resolution (4x fewer MFMA flops than the conv-dgrad at 2h x 2w) plus a
// separable 6 x 6 gather per low-resolution pixel, and neither the 2h x 2w input gradient nor h ever reaches HBM.
//
// Workgroup = 512 threads, persistent over a contiguous range of 8 x 16 low-resolution tiles (XCD-aware order as in
// conv_ring.hip).  Per tile:
//   1. the g halo (rows 2 y0 - 2 .. 2 y0 + 17, columns 2 x0 - 2 .. 2 x0 + 33), prefetched into registers during the
//      previous tile's GEMM, is written to LDS; pixels outside the 2h x 2w image are stored as zeros;
//   2. h is formed in LDS as the A operand [pixel][tap * Cout + c] (fp32 accumulation, one rounding to T):
//      a thread owns two vertically adjacent pixels and 4 channels; it runs the column pass (3 horizontal taps) over
//      the 8 halo rows the two pixels share, then the row pass (3 vertical taps) into both pixels' 9 taps;
//   3. D[pixel][ci] = sum_k h[pixel][k] * W^T[k][ci] with v_mfma_f32_16x16x32_{bf16,f16}; W^T (mrisr_pack_weights with
//      MRISR_PACK_UPADJ) stays in LDS for the whole launch;
//   4. D goes through LDS (over the halo buffer) and out as 16-byte NHWC stores.
#include "conv_upadj.h"

#include <mutex>

int num_cus();

namespace {

constexpr int kUaTY = 8, kUaTX = 16, kUaTP = kUaTY * kUaTX;    // low-resolution tile
constexpr int kUaHR = 2 * kUaTY + 4, kUaHC = 2 * kUaTX + 4;    // g halo rows / columns
constexpr int kUaThreads = 512;

template <int CG, int CA> struct UpAdjLds {
    static constexpr int RS = upadj_rs(CG), CRS = CA + 8;
    static constexpr int W = CA * RS, H = kUaTP * RS;
    static constexpr int G = kUaHR * kUaHC * CG > kUaTP * CRS ? kUaHR * kUaHC * CG : kUaTP * CRS;
    static constexpr size_t bytes = (size_t)(W + H + G) * 2;
};

template <typename T> struct UpAdjMma;
template <> struct UpAdjMma<bf16_t> {
    typedef bf16x8 frag;
    typedef bf16x4 quad;
    static __device__ __forceinline__ f32x4 run(frag a, frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct UpAdjMma<f16_t> {
    typedef f16x8 frag;
    typedef f16x4 quad;
    static __device__ __forceinline__ f32x4 run(frag a, frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

struct UpAdjParams {
    const void* g;       // [N][2h][2w][CG]
    const void* wt;      // packed W^T image [CA][RS]
    void* out;           // [N][h][w][CA]
    int N, h, w;
    int tiles_x, tiles_y, ntiles, tiles_per_block;
};

template <typename T, int CG, int CA>
__global__ __launch_bounds__(kUaThreads) void conv_upadj_kernel(const UpAdjParams p) {
    typedef UpAdjLds<CG, CA> L;
    typedef typename UpAdjMma<T>::frag frag;
    typedef typename UpAdjMma<T>::quad quad;
    constexpr int RS = L::RS, CRS = L::CRS, KP = upadj_kp(CG), K9 = 9 * CG;
    constexpr int GV = CG / 8;                                     // 16-byte vectors per g pixel
    constexpr int NPRE = (kUaHR * kUaHC * GV + kUaThreads - 1) / kUaThreads;
    constexpr int NB = CA / 16, NW = NB >= 2 ? 2 : 1, WN = NB / NW, WM = 8 / WN, MW = 8 / WM;
    static_assert(CG % 8 == 0 && CA % 16 == 0 && WN * WM == 8 && MW * WM == 8, "conv_upadj: width");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* ws = reinterpret_cast<T*>(smem);
    T* hs = ws + L::W;
    T* gs = hs + L::H;                       // g halo [HR][HC][CG]; after the h pass the output tile [TP][CRS]

    const int t = threadIdx.x;
    const int H2 = 2 * p.h, W2 = 2 * p.w;
    int bid = blockIdx.x;
    if ((gridDim.x & 7) == 0) bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);
    const int bt0 = bid * p.tiles_per_block, bt1 = min(bt0 + p.tiles_per_block, p.ntiles);
    if (bt0 >= bt1) return;

    // W^T image -> LDS (once), zero K padding of the h image (never written by the h pass)
    for (int v = t; v < L::W / 8; v += kUaThreads)
        *reinterpret_cast<u32x4*>(ws + v * 8) = gload<u32x4>((const char*)p.wt + (size_t)v * 16);
    if (KP > K9) {
        constexpr int PADV = (KP - K9) / 4;  // 8-byte pieces per row
        for (int v = t; v < kUaTP * PADV; v += kUaThreads)
            *reinterpret_cast<u32x2*>(hs + (v / PADV) * RS + K9 + (v % PADV) * 4) = u32x2{0u, 0u};
    }

    auto tile_origin = [&](int tile, int& n, int& y0, int& x0) {
        const int tx = tile % p.tiles_x, r = tile / p.tiles_x;
        x0 = tx * kUaTX;
        y0 = (r % p.tiles_y) * kUaTY;
        n = r / p.tiles_y;
    };
    // g halo of a tile -> registers (zeros outside the 2h x 2w image: the conv's zero padding of g)
    u32x4 pre[NPRE];
    auto prefetch = [&](int tile) {
        int n, y0, x0;
        tile_origin(tile, n, y0, x0);
        const char* gb = (const char*)p.g + (size_t)n * H2 * W2 * CG * sizeof(T);
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int v = t + i * kUaThreads;
            pre[i] = u32x4{0u, 0u, 0u, 0u};
            if (v < kUaHR * kUaHC * GV) {
                const int cv = v % GV, px = v / GV, hc = px % kUaHC, hr = px / kUaHC;
                const int Y = 2 * y0 - 2 + hr, X = 2 * x0 - 2 + hc;
                if (Y >= 0 && Y < H2 && X >= 0 && X < W2)
                    pre[i] = gload<u32x4>(gb + ((size_t)Y * W2 + X) * CG * sizeof(T) + cv * 16);
            }
        }
    };
    prefetch(bt0);

    const int lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;

    for (int tile = bt0; tile < bt1; ++tile) {
        int n, y0, x0;
        tile_origin(tile, n, y0, x0);
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int v = t + i * kUaThreads;
            if (v < kUaHR * kUaHC * GV) *reinterpret_cast<u32x4*>(gs + v * 8) = pre[i];
        }
        __syncthreads();

        // ---- h pass.  Item = (pixel pair: rows 2py, 2py+1 of the tile, column px; 4 channels c4*4 ..)
        for (int it = t; it < (kUaTP / 2) * (CG / 4); it += kUaThreads) {
            const int c4 = it % (CG / 4), pair = it / (CG / 4), px = pair % kUaTX, py = pair / kUaTX;
            const int qx = x0 + px, qy = y0 + 2 * py;
            // adjoint weights of the candidate rows 2q-1 .. 2q+2 (up2_adjoint_weights: aten's fp32 source coordinate,
            // zero for rows outside the 2h x 2w image).  Two masks apply: P inside the image (these weights) and
            // P - t inside it (the zeros of the halo); a pixel outside the h x w image gets zero weights.
            int idx[kUpAdj];
            float wx[kUpAdj], wy[2][kUpAdj];
            up2_adjoint_weights(min(qx, p.w - 1), p.w, idx, wx);
            up2_adjoint_weights(min(qy, p.h - 1), p.h, idx, wy[0]);
            up2_adjoint_weights(min(qy + 1, p.h - 1), p.h, idx, wy[1]);
#pragma unroll
            for (int k = 0; k < kUpAdj; ++k) {
                if (qx >= p.w) wx[k] = 0.f;
                if (qy >= p.h) wy[0][k] = 0.f;
                if (qy + 1 >= p.h) wy[1][k] = 0.f;
            }
            float hacc[2][9][4];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int tp = 0; tp < 9; ++tp)
#pragma unroll
                    for (int e = 0; e < 4; ++e) hacc[i][tp][e] = 0.f;
            // halo row r = 4py + rr (rr = 0..7) is g row 2qy - 2 + rr; halo column 2px + c is g column 2qx - 2 + c.
            // h_t(q) = sum_{a,b} wy[a] wx[b] g(2qy - 1 + a - ty, 2qx - 1 + b - tx):  row rr = a - ky + 2 (+2 for the
            // second pixel), column c = b - kx + 2.
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                float gv[6][4];
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const quad q = *reinterpret_cast<const quad*>(gs + ((4 * py + rr) * kUaHC + 2 * px + c) * CG + c4 * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) gv[c][e] = (float)q[e];
                }
                float cx[3][4];      // column pass: the 3 horizontal taps of this row
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float s = 0.f;
#pragma unroll
                        for (int b = 0; b < kUpAdj; ++b) s += wx[b] * gv[b - kx + 2][e];
                        cx[kx][e] = s;
                    }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) {
                        const int a = rr - 2 * i + ky - 2;     // candidate row of pixel i this halo row is, for tap ky
                        if (a < 0 || a >= kUpAdj) continue;
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                            for (int e = 0; e < 4; ++e) hacc[i][ky * 3 + kx][e] += wy[i][a] * cx[kx][e];
                    }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                T* hp = hs + ((2 * py + i) * kUaTX + px) * RS + c4 * 4;
#pragma unroll
                for (int tp = 0; tp < 9; ++tp) {
                    quad q;
#pragma unroll
                    for (int e = 0; e < 4; ++e) q[e] = from_f32<T>(hacc[i][tp][e]);
                    *reinterpret_cast<quad*>(hp + tp * CG) = q;
                }
            }
        }
        __syncthreads();

        if (tile + 1 < bt1) prefetch(tile + 1);        // in flight during the GEMM

        // ---- GEMM: wave (wm, wn) owns M blocks wm*MW .. and N blocks wn*NW .. of 16 x 16
        f32x4 acc[MW][NW];
#pragma unroll
        for (int mi = 0; mi < MW; ++mi)
#pragma unroll
            for (int ni = 0; ni < NW; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kl = (lane >> 4) * 8;
#pragma unroll 3
        for (int ks = 0; ks < KP / 32; ++ks) {
            frag a[MW], b[NW];
#pragma unroll
            for (int mi = 0; mi < MW; ++mi)
                a[mi] = *reinterpret_cast<const frag*>(hs + ((wm * MW + mi) * 16 + (lane & 15)) * RS + ks * 32 + kl);
#pragma unroll
            for (int ni = 0; ni < NW; ++ni)
                b[ni] = *reinterpret_cast<const frag*>(ws + ((wn * NW + ni) * 16 + (lane & 15)) * RS + ks * 32 + kl);
#pragma unroll
            for (int mi = 0; mi < MW; ++mi)
#pragma unroll
                for (int ni = 0; ni < NW; ++ni) acc[mi][ni] = UpAdjMma<T>::run(a[mi], b[ni], acc[mi][ni]);
        }
        // D (col = lane & 15, rows (lane >> 4) * 4 + j) -> output tile in LDS
#pragma unroll
        for (int mi = 0; mi < MW; ++mi)
#pragma unroll
            for (int ni = 0; ni < NW; ++ni)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    gs[((wm * MW + mi) * 16 + (lane >> 4) * 4 + j) * CRS + (wn * NW + ni) * 16 + (lane & 15)] =
                        from_f32<T>(acc[mi][ni][j]);
        __syncthreads();

        // ---- 16-byte NHWC stores of the pixels inside the image
        char* ob = (char*)p.out + (size_t)n * p.h * p.w * CA * sizeof(T);
        for (int v = t; v < kUaTP * (CA / 8); v += kUaThreads) {
            const int cv = v % (CA / 8), pix = v / (CA / 8);
            const int y = y0 + pix / kUaTX, x = x0 + pix % kUaTX;
            if (y < p.h && x < p.w)
                gstore(ob + ((size_t)y * p.w + x) * CA * sizeof(T) + cv * 16,
                       *reinterpret_cast<const u32x4*>(gs + pix * CRS + cv * 8));
        }
        __syncthreads();
    }
}

template <typename T, int CG, int CA>
int launch_upadj(const mrisr_conv_desc* d, const void* g, void* dlow, hipStream_t s) {
    UpAdjParams p;
    p.g = g; p.wt = d->wpacked; p.out = dlow;
    p.N = d->N; p.h = d->H / 2; p.w = d->W / 2;
    p.tiles_x = ceil_div(p.w, kUaTX); p.tiles_y = ceil_div(p.h, kUaTY);
    p.ntiles = p.N * p.tiles_x * p.tiles_y;
    const int cus = d->cu_limit > 0 && d->cu_limit < num_cus() ? d->cu_limit : num_cus();
    p.tiles_per_block = ceil_div(p.ntiles, cus);
    const int grid = ceil_div(p.ntiles, p.tiles_per_block);
    constexpr size_t lds = UpAdjLds<CG, CA>::bytes;
    static_assert(lds <= 160 * 1024, "conv_upadj: LDS");
    static std::once_flag once;
    std::call_once(once, [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_upadj_kernel<T, CG, CA>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    hipLaunchKernelGGL((conv_upadj_kernel<T, CG, CA>), dim3(grid), dim3(kUaThreads), lds, s, p);
    MRISR_CHECK_LAUNCH("conv_upadj");
    return MRISR_OK;
}

}  // namespace

int conv_upadj_variant(const mrisr_conv_desc* d, char* out, size_t n) {
    if (!conv_upadj_width_ok(d->dtype, d->Cout, d->Cin, d->ksize)) MRISR_FAIL(MRISR_E_UNSUPPORTED, "conv_variant: no upadj kernel");
    snprintf(out, n, "conv_upadj_kernel<%s,%d,%d>", d->dtype == MRISR_BF16 ? "bf16" : "f16", d->Cout, d->Cin);
    return MRISR_OK;
}

extern "C" size_t mrisr_packed_weight_bytes_upadj(int dtype, int Cout, int Cin, int ksize) {
    return conv_upadj_image_bytes(dtype, Cout, Cin, ksize);
}

extern "C" int mrisr_conv_upadj(const mrisr_conv_desc* d, const void* g, void* d_low, void* stream) {
    if (!d || !g || !d_low || !d->wpacked) MRISR_FAIL(MRISR_E_ARG, "conv_upadj: null pointer");
    if (!conv_upadj_width_ok(d->dtype, d->Cout, d->Cin, d->ksize))
        MRISR_FAIL(MRISR_E_UNSUPPORTED, "conv_upadj: %d -> %d k%d dtype %d", d->Cin, d->Cout, d->ksize, d->dtype);
    if (d->N <= 0 || d->N > 65535 || d->H < 2 || d->W < 2 || (d->H | d->W) & 1 || (size_t)d->H * d->W >= (1u << 28))
        MRISR_FAIL(MRISR_E_SHAPE, "conv_upadj: N %d H %d W %d (even high-resolution size)", d->N, d->H, d->W);
    hipStream_t s = (hipStream_t)stream;
    const bool b = d->dtype == MRISR_BF16;
    switch (d->Cout) {
        case 8: return b ? launch_upadj<bf16_t, 8, 16>(d, g, d_low, s) : launch_upadj<f16_t, 8, 16>(d, g, d_low, s);
        case 16: return b ? launch_upadj<bf16_t, 16, 32>(d, g, d_low, s) : launch_upadj<f16_t, 16, 32>(d, g, d_low, s);
        default: return b ? launch_upadj<bf16_t, 32, 64>(d, g, d_low, s) : launch_upadj<f16_t, 32, 64>(d, g, d_low, s);
    }
}
