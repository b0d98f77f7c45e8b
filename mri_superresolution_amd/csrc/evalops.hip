// Device-side interpolation baselines of the evaluation harness (gfx950, HBM-bound), SURVEY.md 8(f) rank 4.
//
// Replaces the host code of the reference's scripts/test_comparison.py:92-134 as scripts/evaluate.py:upscale_array
// restates it for a scale factor of 2 on 8-bit images:
//   cv2.resize(INTER_LINEAR / INTER_CUBIC): source coordinate (dst + 0.5) / 2 - 0.5, border replication (index clamp),
//   Keys cubic a = -0.75, result rounded half to even and saturated to uint8;
//   'sharp_bilinear': cv2.filter2D([[-1,-1,-1],[-1,9,-1],[-1,-1,-1]], BORDER_REFLECT_101) on the ROUNDED bilinear image.
// For the factor 2 the fractional position is 0.75 (even output index) or 0.25 (odd), so every weight is a multiple of
// 1/256 and both separable passes are exact in int32: v / 65536 with |v| < 2^26, rounded on the integer.  The host's
// float64 arithmetic is exact on the same values, hence the two agree bit for bit (tests/test_gpu_eval.py); no float lerp.
//
// One block = one 32 x 128 output tile of one image: source patch (index clamp applied on IMAGE coordinates) -> LDS,
// horizontal pass -> LDS int32, vertical pass + rounding -> LDS uint8; the sharp method filters a tile with a one-pixel
// halo (reflect-101 on IMAGE coordinates) out of LDS, so the bilinear image never goes to HBM.
#include "common.h"

constexpr int kUR = 32, kUC = 128;                    // output tile
constexpr int kPH = kUR / 2 + 4, kPW = kUC / 2 + 4;   // source patch: rows sy0 = oy0/2 - 2 .. oy0/2 + kUR/2 + 1 (bicubic taps i0-1 .. i0+2)
constexpr int kPS = kPW + 4;                          // LDS patch row stride; column c sits at byte c + 2, so that the 16-byte
                                                      // aligned middle part (source column ox0/2) starts on a 4-byte boundary
constexpr int kHW = kUC + 2;                          // widest horizontal-pass row (sharp: tile + halo)

// weight tables, first tap at i0 (bilinear) / i0 - 1 (bicubic) with i0 = (k - 1) >> 1; [k & 1][tap], in 1/256
__constant__ int kLinW[2][2] = {{64, 192}, {192, 64}};
__constant__ int kCubW[2][4] = {{-9, 67, 225, -27}, {-27, 225, 67, -9}};

__device__ __forceinline__ int reflect101(int i, int n) {      // n >= 2; positions further out than one period are never used
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return min(max(i, 0), n - 1);
}
__device__ __forceinline__ int round_even_sat_u8(int v) {      // rint(v / 65536) clipped to 0..255
    int q = v >> 16;
    const int r = v & 0xffff;
    if (r > 0x8000 || (r == 0x8000 && (q & 1))) ++q;
    return min(max(q, 0), 255);
}

// kTaps 2: bilinear, 4: bicubic; kSharp: bilinear + 3x3 sharpening
template <int kTaps, bool kSharp>
__global__ __launch_bounds__(256) void u8_upscale2_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out_u8,
                                                          float* __restrict__ out_f32, int h, int w) {
    constexpr int kHalo = kSharp ? 1 : 0;
    constexpr int kTH = kUR + 2 * kHalo, kTW = kUC + 2 * kHalo;      // interpolated tile incl. halo
    __shared__ __attribute__((aligned(16))) uint8_t patch[kPH * kPS];
    __shared__ int hz[kPH][kHW];
    __shared__ __attribute__((aligned(16))) uint8_t res[kUR * kUC];
    __shared__ uint8_t bil[kSharp ? kTH * kTW : 1];
    const int t = threadIdx.x, b = blockIdx.z;
    const int H2 = 2 * h, W2 = 2 * w;
    const int ox0 = blockIdx.x * kUC, oy0 = blockIdx.y * kUR;
    const int sx0 = ox0 / 2 - 2, sy0 = oy0 / 2 - 2;
    const uint8_t* src = in + (size_t)b * h * w;

    // ---- source patch: 16 bytes per lane for the aligned middle columns, single bytes for the rest
    if (t < kPH * 4) {
        const int pr = t >> 2, seg = t & 3;
        const int sy = min(max(sy0 + pr, 0), h - 1), sx = ox0 / 2 + seg * 16;
        const uint8_t* rowp = src + (size_t)sy * w;
        uint8_t* dst = patch + pr * kPS + 4 + seg * 16;
        if (sx + 16 <= w && (((uintptr_t)(rowp + sx)) & 15) == 0) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(rowp + sx);
#pragma unroll
            for (int k = 0; k < 4; ++k) reinterpret_cast<unsigned*>(dst)[k] = v[k];
        } else {
            for (int k = 0; k < 16; ++k) dst[k] = rowp[min(sx + k, w - 1)];
        }
    } else if (t < kPH * 8) {
        const int e = t - kPH * 4, pr = e >> 2, k = e & 3;
        const int pc = k < 2 ? k : kPW - 4 + k;              // patch columns 0, 1, kPW-2, kPW-1
        const int sy = min(max(sy0 + pr, 0), h - 1), sx = min(max(sx0 + pc, 0), w - 1);
        patch[pr * kPS + 2 + pc] = src[(size_t)sy * w + sx];
    }
    __syncthreads();

    // ---- horizontal pass: hz[pr][j] for the output columns ox0 - kHalo + j
    for (int e = t; e < kPH * kTW; e += 256) {
        const int pr = e / kTW, j = e - pr * kTW;
        int gx = ox0 - kHalo + j;
        if (kSharp) gx = reflect101(gx, W2);
        const int i0 = ((gx - 1) >> 1) - (kTaps == 4 ? 1 : 0);
        const int pc = min(max(i0 - sx0, 0), kPW - kTaps);   // in range for every column inside the image
        const uint8_t* p = patch + pr * kPS + 2 + pc;
        int s = 0;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) s += (kTaps == 4 ? kCubW[gx & 1][k] : kLinW[gx & 1][k]) * (int)p[k];
        hz[pr][j] = s;
    }
    __syncthreads();

    // ---- vertical pass + rounding
    for (int e = t; e < kTH * kTW; e += 256) {
        const int i = e / kTW, j = e - i * kTW;
        int gy = oy0 - kHalo + i;
        if (kSharp) gy = reflect101(gy, H2);
        const int i0 = ((gy - 1) >> 1) - (kTaps == 4 ? 1 : 0);
        const int pr = min(max(i0 - sy0, 0), kPH - kTaps);
        int s = 0;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) s += (kTaps == 4 ? kCubW[gy & 1][k] : kLinW[gy & 1][k]) * hz[pr + k][j];
        const uint8_t v = (uint8_t)round_even_sat_u8(s);
        if (kSharp) bil[e] = v; else res[e] = v;
    }
    __syncthreads();

    if (kSharp) {      // 9 * centre - the 8 neighbours = 10 * centre - the 3x3 sum, saturated
        for (int e = t; e < kUR * kUC; e += 256) {
            const int i = e / kUC, j = e - i * kUC;
            const uint8_t* p = bil + i * kTW + j;
            int s = 0;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) s += (int)p[dy * kTW + dx];
            res[e] = (uint8_t)min(max(10 * (int)p[kTW + 1] - s, 0), 255);
        }
        __syncthreads();
    }

    // ---- write-out: 16 bytes per lane where the row is aligned, else the element tail
    if (out_u8) {
        const int i = t >> 3, j = (t & 7) * 16;
        const int gy = oy0 + i, gx = ox0 + j;
        if (gy < H2 && gx < W2) {
            uint8_t* o = out_u8 + ((size_t)b * H2 + gy) * W2 + gx;
            if (gx + 16 <= W2 && ((uintptr_t)o & 15) == 0) {
                *reinterpret_cast<u32x4*>(o) = *reinterpret_cast<const u32x4*>(res + i * kUC + j);
            } else {
                const int nrem = min(16, W2 - gx);
                for (int k = 0; k < nrem; ++k) o[k] = res[i * kUC + j + k];
            }
        }
    }
    if (out_f32) {
#pragma unroll
        for (int q = 0; q < kUR * kUC / 4 / 256; ++q) {
            const int g = t + q * 256, i = g / (kUC / 4), j = (g - i * (kUC / 4)) * 4;
            const int gy = oy0 + i, gx = ox0 + j;
            if (gy >= H2 || gx >= W2) continue;
            float* o = out_f32 + ((size_t)b * H2 + gy) * W2 + gx;
            const uint8_t* r = res + i * kUC + j;
            if (gx + 4 <= W2 && ((uintptr_t)o & 15) == 0) {
                f32x4 v;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = __fdiv_rn((float)r[k], 255.f);
                *reinterpret_cast<f32x4*>(o) = v;
            } else {
                const int nrem = min(4, W2 - gx);
                for (int k = 0; k < nrem; ++k) o[k] = __fdiv_rn((float)r[k], 255.f);
            }
        }
    }
}

extern "C" int mrisr_u8_upscale2(const uint8_t* in, uint8_t* out_u8, float* out_f32, int batch, int h, int w, int method,
                                 void* stream) {
    if (!in || (!out_u8 && !out_f32)) MRISR_FAIL(MRISR_E_ARG, "u8_upscale2: null pointer (one of out_u8 / out_f32 is needed)");
    if (batch < 1 || batch > 65535 || h < 1 || w < 1 || h > (1 << 20) || w > (1 << 20) || ceil_div(2 * h, kUR) > 65535)
        MRISR_FAIL(MRISR_E_SHAPE, "u8_upscale2: batch %d h %d w %d", batch, h, w);
    dim3 grid(ceil_div(2 * w, kUC), ceil_div(2 * h, kUR), batch);
    hipStream_t s = (hipStream_t)stream;
    switch (method) {
        case MRISR_UP2_BILINEAR: u8_upscale2_kernel<2, false><<<grid, 256, 0, s>>>(in, out_u8, out_f32, h, w); break;
        case MRISR_UP2_BICUBIC: u8_upscale2_kernel<4, false><<<grid, 256, 0, s>>>(in, out_u8, out_f32, h, w); break;
        case MRISR_UP2_SHARP_BILINEAR: u8_upscale2_kernel<2, true><<<grid, 256, 0, s>>>(in, out_u8, out_f32, h, w); break;
        default: MRISR_FAIL(MRISR_E_UNSUPPORTED, "u8_upscale2: method %d (0 bilinear, 1 bicubic, 2 sharp bilinear)", method);
    }
    MRISR_CHECK_LAUNCH("u8_upscale2");
    return MRISR_OK;
}

// ToTensor of an 8-bit image: out[i] = img[i] / 255 in float32 (evaluate.py:_load01's last step)
__global__ __launch_bounds__(256) void u8_to_unit_f32_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, size_t n) {
    const size_t nv = (((uintptr_t)img & 3) == 0 && ((uintptr_t)out & 15) == 0) ? n / 4 : 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const unsigned v = *reinterpret_cast<const unsigned*>(img + i * 4);
        f32x4 r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = __fdiv_rn((float)((v >> (8 * k)) & 255u), 255.f);
        *reinterpret_cast<f32x4*>(out + i * 4) = r;
    }
    for (size_t i = nv * 4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = __fdiv_rn((float)img[i], 255.f);
}

extern "C" int mrisr_u8_to_unit_f32(const uint8_t* img, float* out, size_t n, void* stream) {
    if (!img || !out) MRISR_FAIL(MRISR_E_ARG, "u8_to_unit_f32: null pointer");
    if (n == 0) return MRISR_OK;
    size_t blocks = (n + 256 * 16 - 1) / (256 * 16);
    if (blocks > 4096) blocks = 4096;
    u8_to_unit_f32_kernel<<<(int)blocks, 256, 0, (hipStream_t)stream>>>(img, out, n);
    MRISR_CHECK_LAUNCH("u8_to_unit_f32");
    return MRISR_OK;
}
