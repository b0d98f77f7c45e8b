// x2 degradation and x2 interpolation baselines of whole volumes on the device (gfx950; extension).
//
// Both restate a numpy specification of mri_superresolution_amd/volume_eval.py operation by operation and are tested bit for
// bit against it (compiled with -ffp-contract=off).  A volume is (X, Y, Z) float32 in C order, Z fastest; bit 0 / 1 / 2 of
// axes_mask selects axis X / Y / Z.
//
//   down2 (downsample2_np)   mean over pairs along the set axes: for the set axes in ascending order v = v[even] + v[odd] (one
//                            rounded float32 sum each), then ONE product with 0.5^k, which is exact.  Output voxel i covers
//                            source voxels 2i, 2i + 1: the model's half-pixel-centred geometry.  One thread per output voxel,
//                            lanes along z; with the z axis set a lane reads its pairs as 8-byte loads.
//   up2 (upscale2_np)        doubles the set axes in ascending order, each on the float32 result of the one before, border
//                            replicated (index clamp).  LINEAR is volume._up2_np: u[2i] = 0.75 e[i] + 0.25 e[i - 1],
//                            u[2i + 1] = 0.75 e[i] + 0.25 e[i + 1] (product, product, sum).  CUBIC is Keys with A = -0.75 (the
//                            rule of resample.hip) at the fractions 0.75 / 0.25, weights exact in float32: u[2i] takes taps
//                            i - 2 .. i + 1 with (-0.03515625, 0.26171875, 0.87890625, -0.10546875), u[2i + 1] taps
//                            i - 1 .. i + 2 with the mirrored weights; four rounded products summed in ascending tap order.
//                            One launch: a thread owns ONE input voxel and emits the up to 2 x 2 x 2 output voxels that belong
//                            to it.  It walks the (2R + 1)^3 source neighbourhood (R = 1 linear, 2 cubic; 1 wide on an unset
//                            axis) z tap by z tap: the x pass of a 5 x 5 slab, then its y pass, both in registers, leaves
//                            2 x 2 values per z tap; the z pass over the five of them gives the outputs.  Every intermediate is
//                            the float32 value the per-axis specification holds at that place, so the result is bit-equal.
//                            Lanes run along z: a wave reads runs of 256 contiguous bytes and stores runs of 512 (z doubled:
//                            one 8-byte pair per lane).
#include "volume_common.h"

#include <math.h>

constexpr int kLinear = MRISR_RESAMPLE_LINEAR, kCubic = MRISR_RESAMPLE_CUBIC;

typedef float __attribute__((ext_vector_type(2))) f32x2;

// ---------------------------------------------------------------- down2
template <bool AX, bool AY, bool AZ>
__global__ __launch_bounds__(256) void volume_down2_kernel(const float* __restrict__ src, int Y, int Z, int OX, int OY, int OZ,
                                                           float scale, float* __restrict__ dst) {
    const int k = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (k >= OZ || j >= OY) return;
    constexpr int NX = AX ? 2 : 1, NY = AY ? 2 : 1, NZ = AZ ? 2 : 1;
    for (int i = blockIdx.z; i < OX; i += gridDim.z) {
        float v[NX][NY][NZ];
#pragma unroll
        for (int p = 0; p < NX; ++p)
#pragma unroll
            for (int q = 0; q < NY; ++q) {
                const float* s = src + ((size_t)(NX * i + p) * Y + (NY * j + q)) * Z + (size_t)NZ * k;
                if constexpr (AZ) {
                    const f32x2 pair = *reinterpret_cast<const f32x2*>(s);      // Z even, base 8-byte aligned
                    v[p][q][0] = pair[0];
                    v[p][q][1] = pair[1];
                } else {
                    v[p][q][0] = *s;
                }
            }
        if constexpr (AX)
#pragma unroll
            for (int q = 0; q < NY; ++q)
#pragma unroll
                for (int r = 0; r < NZ; ++r) v[0][q][r] = __fadd_rn(v[0][q][r], v[1][q][r]);
        if constexpr (AY)
#pragma unroll
            for (int r = 0; r < NZ; ++r) v[0][0][r] = __fadd_rn(v[0][0][r], v[0][1][r]);
        if constexpr (AZ) v[0][0][0] = __fadd_rn(v[0][0][0], v[0][0][1]);
        dst[((size_t)i * OY + j) * OZ + k] = __fmul_rn(v[0][0][0], scale);
    }
}

extern "C" int mrisr_f32_volume_down2(const float* src, int X, int Y, int Z, int axes_mask, float* dst, void* stream) {
    if (!src || !dst) MRISR_FAIL(MRISR_E_ARG, "f32_volume_down2: null pointer");
    if (axes_mask < 1 || axes_mask > 7) MRISR_FAIL(MRISR_E_ARG, "f32_volume_down2: axes_mask %d (1..7)", axes_mask);
    if (const int rc = check_volume_extents("f32_volume_down2", X, Y, Z)) return rc;
    const bool ax = axes_mask & 1, ay = axes_mask & 2, az = axes_mask & 4;
    if ((ax && (X & 1)) || (ay && (Y & 1)) || (az && (Z & 1)))
        MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_down2: volume %d x %d x %d has an odd extent on an axis of mask %d", X, Y, Z, axes_mask);
    if (!aligned_to(src, az ? 8 : 4) || !aligned_to(dst, 4)) MRISR_FAIL(MRISR_E_ARG, "f32_volume_down2: misaligned pointer");
    const int OX = ax ? X / 2 : X, OY = ay ? Y / 2 : Y, OZ = az ? Z / 2 : Z;
    const float scale = 1.0f / (float)(1 << ((int)ax + (int)ay + (int)az));
    const dim3 block(64, 4), grid(ceil_div(OZ, 64), ceil_div(OY, 4), OX);
    hipStream_t st = (hipStream_t)stream;
#define MRISR_DOWN2(AX, AY, AZ) volume_down2_kernel<AX, AY, AZ><<<grid, block, 0, st>>>(src, Y, Z, OX, OY, OZ, scale, dst)
    switch (axes_mask) {
        case 1: MRISR_DOWN2(true, false, false); break;
        case 2: MRISR_DOWN2(false, true, false); break;
        case 3: MRISR_DOWN2(true, true, false); break;
        case 4: MRISR_DOWN2(false, false, true); break;
        case 5: MRISR_DOWN2(true, false, true); break;
        case 6: MRISR_DOWN2(false, true, true); break;
        default: MRISR_DOWN2(true, true, true); break;
    }
#undef MRISR_DOWN2
    MRISR_CHECK_LAUNCH("f32_volume_down2");
    return MRISR_OK;
}

// ---------------------------------------------------------------- up2
// v: the 2R + 1 taps i - R .. i + R of one axis (already clamped); output 2i + parity
template <int METHOD>
__device__ __forceinline__ float up2_tap(const float* v, int parity) {
    if constexpr (METHOD == kLinear) {
        return __fadd_rn(__fmul_rn(0.75f, v[1]), __fmul_rn(0.25f, parity ? v[2] : v[0]));
    } else {
        constexpr float w0 = -0.03515625f, w1 = 0.26171875f, w2 = 0.87890625f, w3 = -0.10546875f;
        float acc;
        if (parity == 0) {      // taps i - 2 .. i + 1
            acc = __fmul_rn(w0, v[0]);
            acc = __fadd_rn(acc, __fmul_rn(w1, v[1]));
            acc = __fadd_rn(acc, __fmul_rn(w2, v[2]));
            acc = __fadd_rn(acc, __fmul_rn(w3, v[3]));
        } else {                // taps i - 1 .. i + 2
            acc = __fmul_rn(w3, v[1]);
            acc = __fadd_rn(acc, __fmul_rn(w2, v[2]));
            acc = __fadd_rn(acc, __fmul_rn(w1, v[3]));
            acc = __fadd_rn(acc, __fmul_rn(w0, v[4]));
        }
        return acc;
    }
}

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// block (64, 4): x over z, y over y; grid z (strided) over x.  X, Y, Z: the INPUT extents.
template <int METHOD, bool AX, bool AY, bool AZ>
__global__ __launch_bounds__(256) void volume_up2_kernel(const float* __restrict__ src, int X, int Y, int Z, float* __restrict__ dst) {
    constexpr int R = METHOD == kCubic ? 2 : 1;
    constexpr int RX = AX ? R : 0, RY = AY ? R : 0, RZ = AZ ? R : 0;
    constexpr int NX = AX ? 2 : 1, NY = AY ? 2 : 1, NZ = AZ ? 2 : 1;
    const int k = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (k >= Z || j >= Y) return;
    const size_t OY = (size_t)NY * Y, OZ = (size_t)NZ * Z;
    for (int i = blockIdx.z; i < X; i += gridDim.z) {
        float zc[NX][NY][2 * RZ + 1];                              // after the x and the y pass, per z tap
#pragma unroll
        for (int dz = 0; dz < 2 * RZ + 1; ++dz) {
            const int kk = clampi(k + dz - RZ, Z);
            float yc[NX][2 * RY + 1];                              // after the x pass, per y tap
#pragma unroll
            for (int dy = 0; dy < 2 * RY + 1; ++dy) {
                const int jj = clampi(j + dy - RY, Y);
                float xs[2 * RX + 1];
#pragma unroll
                for (int dx = 0; dx < 2 * RX + 1; ++dx) xs[dx] = src[((size_t)clampi(i + dx - RX, X) * Y + jj) * Z + kk];
#pragma unroll
                for (int p = 0; p < NX; ++p) {
                    if constexpr (AX) yc[p][dy] = up2_tap<METHOD>(xs, p);
                    else yc[p][dy] = xs[0];
                }
            }
#pragma unroll
            for (int p = 0; p < NX; ++p)
#pragma unroll
                for (int q = 0; q < NY; ++q) {
                    if constexpr (AY) zc[p][q][dz] = up2_tap<METHOD>(yc[p], q);
                    else zc[p][q][dz] = yc[p][0];
                }
        }
#pragma unroll
        for (int p = 0; p < NX; ++p)
#pragma unroll
            for (int q = 0; q < NY; ++q) {
                float* o = dst + ((size_t)(NX * i + p) * OY + (size_t)(NY * j + q)) * OZ + (size_t)NZ * k;
                if constexpr (AZ) {
                    f32x2 u;
                    u[0] = up2_tap<METHOD>(zc[p][q], 0);
                    u[1] = up2_tap<METHOD>(zc[p][q], 1);
                    *reinterpret_cast<f32x2*>(o) = u;              // 2Z even, base 8-byte aligned
                } else {
                    *o = zc[p][q][0];
                }
            }
    }
}

template <int METHOD>
static void launch_up2(const float* src, int X, int Y, int Z, int mask, float* dst, hipStream_t st) {
    const dim3 block(64, 4), grid(ceil_div(Z, 64), ceil_div(Y, 4), X);
#define MRISR_UP2(AX, AY, AZ) volume_up2_kernel<METHOD, AX, AY, AZ><<<grid, block, 0, st>>>(src, X, Y, Z, dst)
    switch (mask) {
        case 1: MRISR_UP2(true, false, false); break;
        case 2: MRISR_UP2(false, true, false); break;
        case 3: MRISR_UP2(true, true, false); break;
        case 4: MRISR_UP2(false, false, true); break;
        case 5: MRISR_UP2(true, false, true); break;
        case 6: MRISR_UP2(false, true, true); break;
        default: MRISR_UP2(true, true, true); break;
    }
#undef MRISR_UP2
}

extern "C" int mrisr_f32_volume_up2(const float* src, int X, int Y, int Z, int axes_mask, int method, float* dst, void* stream) {
    if (!src || !dst) MRISR_FAIL(MRISR_E_ARG, "f32_volume_up2: null pointer");
    if (axes_mask < 1 || axes_mask > 7) MRISR_FAIL(MRISR_E_ARG, "f32_volume_up2: axes_mask %d (1..7)", axes_mask);
    if (method != kLinear && method != kCubic)
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_up2: method %d (MRISR_RESAMPLE_LINEAR or MRISR_RESAMPLE_CUBIC)", method);
    if (const int rc = check_volume_extents("f32_volume_up2", X, Y, Z)) return rc;
    if (!aligned_to(src, 4) || !aligned_to(dst, (axes_mask & 4) ? 8 : 4)) MRISR_FAIL(MRISR_E_ARG, "f32_volume_up2: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    if (method == kLinear) launch_up2<kLinear>(src, X, Y, Z, axes_mask, dst, st);
    else launch_up2<kCubic>(src, X, Y, Z, axes_mask, dst, st);
    MRISR_CHECK_LAUNCH("f32_volume_up2");
    return MRISR_OK;
}
