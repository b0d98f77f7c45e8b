// Table-driven separable resampler with a letter-box epilogue (gfx950; extension): the resize of the
// reference's slice extraction (utils/preprocessing.py:23-57 letterbox_resize, INTER_LANCZOS4 for the high-resolution and
// INTER_AREA for the low-resolution image).  utils/extraction.py:resample_letterbox_host is the float64 restatement the
// tests compare against; parity with cv2.resize's own code path is not claimed (cv2 is absent).
//
// A resize along one axis is a table: for every output sample K consecutive (border-replicated) source indices and their
// weights.  mrisr_resample_taps fills it on the host in double; the kernel knows nothing about the method.
//
// One workgroup (256 threads) = one 16 x 64 tile of one image's output canvas:
//   stage   the tile's share of both tables goes to LDS (weights slot-major: lanes read consecutive words)
//   H pass  the source rows the tile's vertical taps reach, four at a time: their column segment is copied to LDS with
//           coalesced loads, then thread (row, column) sums its K_x taps out of LDS into the intermediate T[row][column]
//   V pass  thread = one column, four rows: K_y taps out of T
//   store   the block at (y_off, x_off), pad_value elsewhere; optional clip to [0,1] and / or uint8 by truncation
// Both sums start at 0 and take their taps in ascending slot order with fmaf: bitwise reproducible, whatever the tile.
// Compiled with -ffp-contract=off (build.py): the epilogue restates the host's  clip(v * 255, 0, 255).astype(uint8).
#include <math.h>

#include "common.h"

constexpr int kRsTH = 16, kRsTW = 64, kRsChunk = 4, kRsMaxTaps = 16;

struct RsAxis {
    const short* index;      // [n][taps]
    const float* weight;     // [n][taps]
    int taps, n, src, off;   // taps per sample, output samples, source samples, offset of the block on the canvas
};

__global__ __launch_bounds__(256) void resample_letterbox_kernel(const float* __restrict__ in, RsAxis ya, RsAxis xa, int outH, int outW,
                                                                 int rows_cap, int cols_cap, float pad_value, int clip,
                                                                 float* __restrict__ out_f32, uint8_t* __restrict__ out_u8) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* yw = reinterpret_cast<float*>(smem);                   // [kRsMaxTaps][kRsTH]
    float* xw = yw + kRsMaxTaps * kRsTH;                          // [kRsMaxTaps][kRsTW]
    int* yi = reinterpret_cast<int*>(xw + kRsMaxTaps * kRsTW);    // [kRsMaxTaps][kRsTH], relative to the first staged row
    int* xi = yi + kRsMaxTaps * kRsTH;                            // [kRsMaxTaps][kRsTW], relative to the first staged column
    float* raw = reinterpret_cast<float*>(xi + kRsMaxTaps * kRsTW);   // [kRsChunk][cols_cap]
    float* T = raw + kRsChunk * cols_cap;                         // [rows_cap][kRsTW]
    const int t = threadIdx.x, b = blockIdx.z;
    const int ty0 = blockIdx.y * kRsTH, tx0 = blockIdx.x * kRsTW;
    // the part of the block this tile holds, in block coordinates
    const int by0 = max(ty0 - ya.off, 0), by1 = min(ty0 + kRsTH - ya.off, ya.n);
    const int bx0 = max(tx0 - xa.off, 0), bx1 = min(tx0 + kRsTW - xa.off, xa.n);
    const bool any = by0 < by1 && bx0 < bx1;          // uniform over the workgroup
    float acc[kRsTH * kRsTW / 256];
#pragma unroll
    for (int j = 0; j < kRsTH * kRsTW / 256; ++j) acc[j] = 0.f;
    const int col = t & (kRsTW - 1);
    if (any) {
        // source window of the tile: indices do not decrease with the output sample, slot by slot
        int rmin = ya.src - 1, rmax = 0, cmin = xa.src - 1, cmax = 0;
        for (int k = 0; k < ya.taps; ++k) {
            rmin = min(rmin, (int)ya.index[(size_t)by0 * ya.taps + k]);
            rmax = max(rmax, (int)ya.index[(size_t)(by1 - 1) * ya.taps + k]);
        }
        for (int k = 0; k < xa.taps; ++k) {
            cmin = min(cmin, (int)xa.index[(size_t)bx0 * xa.taps + k]);
            cmax = max(cmax, (int)xa.index[(size_t)(bx1 - 1) * xa.taps + k]);
        }
        rmin = min(max(rmin, 0), ya.src - 1);
        cmin = min(max(cmin, 0), xa.src - 1);
        // never past the staged window, whatever the tables hold (tables of mrisr_resample_taps stay inside it)
        const int nR = min(min(max(rmax, rmin), ya.src - 1) - rmin + 1, rows_cap);
        const int nC = min(min(max(cmax, cmin), xa.src - 1) - cmin + 1, cols_cap);
        for (int e = t; e < ya.taps * kRsTH; e += 256) {
            const int k = e / kRsTH, i = e - k * kRsTH, y = min(by0 + i, by1 - 1);
            yw[e] = ya.weight[(size_t)y * ya.taps + k];
            yi[e] = min(max((int)ya.index[(size_t)y * ya.taps + k] - rmin, 0), nR - 1);
        }
        for (int e = t; e < xa.taps * kRsTW; e += 256) {
            const int k = e / kRsTW, i = e - k * kRsTW, x = min(bx0 + i, bx1 - 1);
            xw[e] = xa.weight[(size_t)x * xa.taps + k];
            xi[e] = min(max((int)xa.index[(size_t)x * xa.taps + k] - cmin, 0), nC - 1);
        }
        const float* src = in + (size_t)b * ya.src * xa.src;
        const int hrow = t / kRsTW;                   // row of the chunk this thread sums in the H pass
        for (int r0 = 0; r0 < nR; r0 += kRsChunk) {
            __syncthreads();                          // tables staged (first turn); the previous chunk's raw rows are read
            for (int e = t; e < kRsChunk * nC; e += 256) {
                const int rr = e / nC, c = e - rr * nC;
                if (r0 + rr < nR) raw[rr * cols_cap + c] = src[(size_t)(rmin + r0 + rr) * xa.src + cmin + c];
            }
            __syncthreads();
            if (r0 + hrow < nR) {
                float a = 0.f;
                for (int k = 0; k < xa.taps; ++k) a = fmaf(xw[k * kRsTW + col], raw[hrow * cols_cap + xi[k * kRsTW + col]], a);
                T[(r0 + hrow) * kRsTW + col] = a;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kRsTH * kRsTW / 256; ++j) {
            const int i = t / kRsTW + j * (256 / kRsTW);     // row of the tile's share of the block
            for (int k = 0; k < ya.taps; ++k) acc[j] = fmaf(yw[k * kRsTH + i], T[yi[k * kRsTH + i] * kRsTW + col], acc[j]);
        }
    }
    // A thread sums block pixels (by0 + i, bx0 + col) but stores canvas pixels (ty0 + dy, tx0 + col).  The two numberings
    // differ by the tile's lead-in (fy - ty0, fx - tx0), so the results cross lanes through LDS.
    const int fy = any ? ya.off + by0 : 0, fx = any ? xa.off + bx0 : 0;
    __syncthreads();
    float* R = T;                                      // [kRsTH][kRsTW] results, reusing the intermediate (rows_cap >= kRsTH)
    if (any) {
#pragma unroll
        for (int j = 0; j < kRsTH * kRsTW / 256; ++j) R[(t / kRsTW + j * (256 / kRsTW)) * kRsTW + col] = acc[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kRsTH * kRsTW / 256; ++j) {
        const int dy = t / kRsTW + j * (256 / kRsTW);
        const int y = ty0 + dy, x = tx0 + col;
        if (y >= outH || x >= outW) continue;
        const int iy = y - fy, ix = x - fx;
        const bool inside = any && iy >= 0 && iy < by1 - by0 && ix >= 0 && ix < bx1 - bx0;
        float v = pad_value;
        if (inside) {
            v = R[iy * kRsTW + ix];
            if (clip) v = fminf(fmaxf(v, 0.f), 1.f);
        }
        const size_t o = ((size_t)b * outH + y) * outW + x;
        if (out_f32) out_f32[o] = v;
        if (out_u8) out_u8[o] = (uint8_t)(int)fminf(fmaxf(__fmul_rn(v, 255.f), 0.f), 255.f);     // astype(np.uint8) truncates
    }
}

// ---------------------------------------------------------------- tap tables (host, double)
static double rs_sinc(double x) {
    if (x == 0.0) return 1.0;
    if (x == floor(x)) return 0.0;            // exact zeros at the integers: src == dst is the identity
    const double px = 3.14159265358979323846 * x;
    return sin(px) / px;
}
static double rs_keys(double x) {             // Keys cubic, A = -0.75
    const double A = -0.75;
    x = fabs(x);
    if (x <= 1.0) return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0;
    if (x < 2.0) return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A;
    return 0.0;
}

extern "C" int mrisr_resample_taps(int method, int src, int dst, int max_taps, int* ntaps, short* index, float* weight) {
    if (!ntaps || !index || !weight) MRISR_FAIL(MRISR_E_ARG, "resample_taps: null pointer");
    if (src < 1 || dst < 1 || src > 32767 || dst > 32767) MRISR_FAIL(MRISR_E_SHAPE, "resample_taps: src %d dst %d (1..32767)", src, dst);
    if (method != MRISR_RESAMPLE_LINEAR && method != MRISR_RESAMPLE_CUBIC && method != MRISR_RESAMPLE_AREA &&
        method != MRISR_RESAMPLE_LANCZOS4)
        MRISR_FAIL(MRISR_E_ARG, "resample_taps: method %d", method);
    if (method == MRISR_RESAMPLE_AREA && dst > src) method = MRISR_RESAMPLE_LINEAR;      // documented deviation
    int K;
    if (method == MRISR_RESAMPLE_AREA) {
        K = 1;
        for (int d = 0; d < dst; ++d) {
            const double lo = (double)((long long)d * src) / dst, hi = (double)((long long)(d + 1) * src) / dst;
            const int n = (int)ceil(hi) - (int)floor(lo);
            if (n > K) K = n;
        }
    } else {
        K = method == MRISR_RESAMPLE_LINEAR ? 2 : method == MRISR_RESAMPLE_CUBIC ? 4 : 8;
    }
    if (K > kRsMaxTaps) MRISR_FAIL(MRISR_E_UNSUPPORTED, "resample_taps: %d -> %d needs %d taps per sample (at most %d)", src, dst, K, kRsMaxTaps);
    if (K > max_taps) MRISR_FAIL(MRISR_E_SHAPE, "resample_taps: %d taps per sample, room for %d", K, max_taps);
    *ntaps = K;
    const double scale = (double)src / dst;
    for (int d = 0; d < dst; ++d) {
        double w[kRsMaxTaps];
        int first;
        if (method == MRISR_RESAMPLE_AREA) {
            const double lo = (double)((long long)d * src) / dst, hi = (double)((long long)(d + 1) * src) / dst;
            const double den = fmin(scale, (double)src - lo);
            first = (int)floor(lo);
            for (int k = 0; k < K; ++k) {
                const double ov = fmin((double)(first + k + 1), hi) - fmax((double)(first + k), lo);
                w[k] = ov > 0.0 ? ov / den : 0.0;
            }
        } else {
            const double s = ((double)d + 0.5) * scale - 0.5, fl = floor(s), fr = s - fl;
            first = (int)fl - (K / 2 - 1);
            double sum = 0.0;
            for (int k = 0; k < K; ++k) {
                const double x = fr - (double)(k - (K / 2 - 1));      // distance of the sample point from tap k
                if (method == MRISR_RESAMPLE_LINEAR) w[k] = 1.0 - fabs(x);
                else if (method == MRISR_RESAMPLE_CUBIC) w[k] = rs_keys(x);
                else w[k] = fabs(x) < 4.0 ? rs_sinc(x) * rs_sinc(x / 4.0) : 0.0;
                sum += w[k];
            }
            if (method == MRISR_RESAMPLE_LANCZOS4)
                for (int k = 0; k < K; ++k) w[k] /= sum;
        }
        for (int k = 0; k < max_taps; ++k) {
            const int kk = k < K ? k : K - 1;
            const int i = first + kk;
            index[(size_t)d * max_taps + k] = (short)(i < 0 ? 0 : i > src - 1 ? src - 1 : i);      // replicated border
            weight[(size_t)d * max_taps + k] = k < K ? (float)w[k] : 0.f;
        }
    }
    return MRISR_OK;
}

extern "C" int mrisr_f32_resample_letterbox(const float* in, int batch, int H, int W, const short* y_index, const float* y_weight,
                                            int y_taps, int new_h, const short* x_index, const float* x_weight, int x_taps, int new_w,
                                            int out_h, int out_w, int y_off, int x_off, float pad_value, int clip, float* out_f32,
                                            uint8_t* out_u8, void* stream) {
    if (!in || !y_index || !y_weight || !x_index || !x_weight || (!out_f32 && !out_u8))
        MRISR_FAIL(MRISR_E_ARG, "f32_resample_letterbox: null pointer (one of out_f32 / out_u8 is needed)");
    if (batch < 1 || batch > 65535) MRISR_FAIL(MRISR_E_SHAPE, "f32_resample_letterbox: batch %d", batch);
    if (H < 1 || W < 1 || new_h < 1 || new_w < 1 || out_h < 1 || out_w < 1 || H > 32767 || W > 32767 || new_h > 32767 || new_w > 32767 ||
        out_h > 32767 || out_w > 32767)
        MRISR_FAIL(MRISR_E_SHAPE, "f32_resample_letterbox: %d x %d -> %d x %d on %d x %d", H, W, new_h, new_w, out_h, out_w);
    if (y_off < 0 || x_off < 0 || (long long)y_off + new_h > out_h || (long long)x_off + new_w > out_w)
        MRISR_FAIL(MRISR_E_SHAPE, "f32_resample_letterbox: block %d x %d at (%d, %d) does not fit the %d x %d canvas", new_h, new_w,
                   y_off, x_off, out_h, out_w);
    if (y_taps < 1 || y_taps > kRsMaxTaps || x_taps < 1 || x_taps > kRsMaxTaps)
        MRISR_FAIL(MRISR_E_UNSUPPORTED, "f32_resample_letterbox: %d / %d taps per sample (1..%d)", y_taps, x_taps, kRsMaxTaps);
    // source window of a tile: T consecutive output samples reach at most (T - 1) max(scale, 1) + taps + 1 source samples
    auto window = [](int tile, int src, int dst, int taps) {
        const double scale = (double)src / dst;
        const long long span = (long long)ceil((tile - 1) * (scale > 1.0 ? scale : 1.0)) + taps + 2;
        return (int)(span < src ? span : src);
    };
    int rows_cap = window(kRsTH, H, new_h, y_taps), cols_cap = window(kRsTW, W, new_w, x_taps);
    if (rows_cap < kRsTH) rows_cap = kRsTH;           // the intermediate doubles as the tile's result buffer
    const size_t lds = (size_t)kRsMaxTaps * (kRsTH + kRsTW) * 8 + ((size_t)kRsChunk * cols_cap + (size_t)rows_cap * kRsTW) * sizeof(float);
    if (lds > 160 * 1024)
        MRISR_FAIL(MRISR_E_UNSUPPORTED, "f32_resample_letterbox: %d x %d -> %d x %d needs %zu bytes of LDS per tile", H, W, new_h, new_w, lds);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(resample_letterbox_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const RsAxis ya{y_index, y_weight, y_taps, new_h, H, y_off}, xa{x_index, x_weight, x_taps, new_w, W, x_off};
    const dim3 grid(ceil_div(out_w, kRsTW), ceil_div(out_h, kRsTH), batch);
    resample_letterbox_kernel<<<grid, 256, lds, (hipStream_t)stream>>>(in, ya, xa, out_h, out_w, rows_cap, cols_cap, pad_value, clip,
                                                                      out_f32, out_u8);
    MRISR_CHECK_LAUNCH("f32_resample_letterbox");
    return MRISR_OK;
}
