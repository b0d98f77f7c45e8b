// Multi-planar blend of whole-volume inference on the device (gfx950; extension).
//
// enhance_volume doubles the two in-plane axes of the slices it runs; an isotropic x2 volume is the mean of up to three such
// passes (slices across axis 0, 1 and 2), each brought to the full (2X, 2Y, 2Z) grid by doubling its one remaining axis with
// the model's own half-pixel-centred linear rule (output o at input o/2 - 1/4, replicated border):
//
//     u[2s]     = 0.75f * e[s] + 0.25f * e[max(s - 1, 0)]
//     u[2s + 1] = 0.75f * e[s] + 0.25f * e[min(s + 1, S - 1)]
//
// One launch per plane reads the plane's slice-major result [S][R][C] once, interpolates along s in registers and
// read-modify-writes the C-order accumulator once: SET (acc = U), ADD (acc += U), FINISH (out = (acc + U) / count as float32 or
// int16; count == 1: out = U, acc is not read).  The arithmetic restates volume.combine_planes_np operation by operation
// (compiled with -ffp-contract=off): a rounded product, a rounded product, a rounded sum; sums in plane order; one division.
//
//   stream form (axes 0 and 1)   plane and acc share the fastest axis.  Axis 1: acc[r][2s + p][c] <- plane[s][r][c]; axis 0 is
//                                the same map with R = 1 and C = 2Y * 2Z (whole slices are contiguous in both).  A thread owns
//                                one 16-byte column of c, walks kRun slices with (prev, cur, next) in registers and emits both
//                                outputs of every slice: kRun + 2 loads per 2 kRun stores.  C is a doubled extent and so even;
//                                where it is no multiple of 4 every other row starts 8 bytes off a 16-byte boundary and the
//                                kernel runs in its 8-byte form (VEC = 2): no access crosses the end of a row in either form.
//   transposing form (axis 2)    plane is contiguous along c (= y), acc along z, the interpolated axis:
//                                acc[r][c][2s + p] <- plane[s][r][c].  One workgroup stages, for one r, kTileS + 2 slices (a halo
//                                of one either side, clamped to the volume: the replicated border) x kTileC columns in LDS,
//                                written with lanes along c and read with lanes along s; every lane then stores its two
//                                outputs as one 8-byte pair, a wave 512 contiguous bytes of one z run.
//                                LDS banks (ds_write_b32 / ds_read_b32: bank = dword address mod 32, conflicts within a 32-lane
//                                half): the write puts the 32 lanes of a half on 32 consecutive dwords of one tile row - 32
//                                banks whatever the row pitch.  The read puts lane l of a half on dword (l + k) * P + c: the 32
//                                lanes are on 32 different banks iff P is odd, and all on ONE bank with the unpadded P = 32.
//                                Tile 64 (s) x 32 (c), pitch P = kTileC + 1 = 33 dwords: (64 + 2) * 33 * 4 = 8712 bytes.
#include "volume_common.h"

#include <math.h>

constexpr int kModeSet = MRISR_VOLBLEND_SET, kModeAdd = MRISR_VOLBLEND_ADD, kModeFinish = MRISR_VOLBLEND_FINISH;
constexpr int kRun = 8;            // slices a thread of the stream form walks
constexpr int kTileS = 64;         // transposing form: slices per tile = lanes of a wave along z
constexpr int kTileC = 32;         // columns per tile
constexpr int kPitch = kTileC + 1; // odd: see above

template <int N> struct VecOf {
    typedef float __attribute__((ext_vector_type(N))) f32;
    typedef short __attribute__((ext_vector_type(N))) s16;
};

__device__ __forceinline__ float up2_tap(float centre, float side) {       // product, product, sum: three roundings
    return __fadd_rn(__fmul_rn(0.75f, centre), __fmul_rn(0.25f, side));
}
__device__ __forceinline__ short to_i16(float v) { return (short)(int)fminf(fmaxf(rintf(v), -32768.f), 32767.f); }   // np.rint, saturated

// u: N consecutive values of U(plane) at element offset idx of the accumulator.  acc and out may be the same buffer (float32
// FINISH in place): every element is read and then written by the one thread that owns it.
template <int N, int MODE, typename T>
__device__ __forceinline__ void blend_store(typename VecOf<N>::f32 u, float* acc, T* out, size_t idx, int count) {
    typedef typename VecOf<N>::f32 fvec;
    if constexpr (MODE == kModeSet) {
        *reinterpret_cast<fvec*>(acc + idx) = u;
    } else if constexpr (MODE == kModeAdd) {
        const fvec a = *reinterpret_cast<const fvec*>(acc + idx);
        fvec r;
#pragma unroll
        for (int k = 0; k < N; ++k) r[k] = __fadd_rn(a[k], u[k]);
        *reinterpret_cast<fvec*>(acc + idx) = r;
    } else {
        fvec r = u;
        if (count > 1) {
            const fvec a = *reinterpret_cast<const fvec*>(acc + idx);
            const float div = (float)count;
#pragma unroll
            for (int k = 0; k < N; ++k) r[k] = __fdiv_rn(__fadd_rn(a[k], u[k]), div);
        }
        if constexpr (sizeof(T) == 2) {
            typename VecOf<N>::s16 q;
#pragma unroll
            for (int k = 0; k < N; ++k) q[k] = to_i16(r[k]);
            *reinterpret_cast<typename VecOf<N>::s16*>(out + idx) = q;
        } else {
            *reinterpret_cast<fvec*>(out + idx) = r;
        }
    }
}

// block (bx, by): x over the C / VEC vector columns, y over r; grid z (strided) over runs of kRun slices
template <int VEC, int MODE, typename T>
__global__ __launch_bounds__(256) void up2_blend_stream_kernel(const float* __restrict__ plane, int S, int R, int CV, float* acc, T* out,
                                                               int count) {
    typedef typename VecOf<VEC>::f32 fvec;
    const int cv = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y * blockDim.y + threadIdx.y;
    if (cv >= CV || r >= R) return;
    const size_t C = (size_t)CV * VEC, col = (size_t)cv * VEC;
    auto load = [&](int s) { return *reinterpret_cast<const fvec*>(plane + ((size_t)s * R + r) * C + col); };
    for (int s0 = blockIdx.z * kRun; s0 < S; s0 += gridDim.z * kRun) {
        const int s1 = s0 + kRun < S ? s0 + kRun : S;
        fvec prev = load(s0 > 0 ? s0 - 1 : 0), cur = load(s0);
        for (int s = s0; s < s1; ++s) {
            const fvec next = load(s + 1 < S ? s + 1 : S - 1);
            fvec lo, hi;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                lo[k] = up2_tap(cur[k], prev[k]);
                hi[k] = up2_tap(cur[k], next[k]);
            }
            const size_t o = ((size_t)r * 2 * S + 2 * s) * C + col;
            blend_store<VEC, MODE, T>(lo, acc, out, o, count);
            blend_store<VEC, MODE, T>(hi, acc, out, o + C, count);
            prev = cur;
            cur = next;
        }
    }
}

// grid (s tiles, c tiles, r); 256 threads
template <int MODE, typename T>
__global__ __launch_bounds__(256) void up2_blend_transpose_kernel(const float* __restrict__ plane, int S, int R, int C, float* acc, T* out,
                                                                  int count) {
    __shared__ float tile[(kTileS + 2) * kPitch];
    const int s0 = blockIdx.x * kTileS, c0 = blockIdx.y * kTileC, r = blockIdx.z;
    const int t = threadIdx.x;
    {   // stage: lanes along c (32 consecutive floats of one slice row per half wave); row j holds slice clamp(s0 - 1 + j)
        const int ci = t & (kTileC - 1);
        if (c0 + ci < C)
            for (int j = t / kTileC; j < kTileS + 2; j += 256 / kTileC) {
                int s = s0 - 1 + j;
                s = s < 0 ? 0 : (s > S - 1 ? S - 1 : s);
                tile[j * kPitch + ci] = plane[((size_t)s * R + r) * C + c0 + ci];
            }
    }
    __syncthreads();
    const int lane = t & 63, s = s0 + lane;
    if (s >= S) return;
    for (int ci = t >> 6; ci < kTileC && c0 + ci < C; ci += 4) {      // lanes along s: one z run of 2 * kTileS outputs per wave
        const float prev = tile[lane * kPitch + ci], cur = tile[(lane + 1) * kPitch + ci], next = tile[(lane + 2) * kPitch + ci];
        typename VecOf<2>::f32 u;
        u[0] = up2_tap(cur, prev);
        u[1] = up2_tap(cur, next);
        blend_store<2, MODE, T>(u, acc, out, ((size_t)r * C + c0 + ci) * 2 * S + 2 * s, count);
    }
}

template <int VEC, int MODE, typename T>
static void launch_stream(const float* plane, int S, int R, int C, float* acc, void* out, int count, hipStream_t st) {
    const int CV = C / VEC;
    // one wave per 64 vector columns; the other threads of the block go to r where there is more than one row per slice
    const dim3 block(R > 1 ? 64 : 256, R > 1 ? 4 : 1);
    const int runs = ceil_div(S, kRun);
    const dim3 grid(ceil_div(CV, (int)block.x), ceil_div(R, (int)block.y), runs < 65535 ? runs : 65535);
    up2_blend_stream_kernel<VEC, MODE, T><<<grid, block, 0, st>>>(plane, S, R, CV, acc, (T*)out, count);
}

template <int VEC>
static void dispatch_stream(const float* plane, int S, int R, int C, float* acc, int mode, int count, int out_dtype, void* out, hipStream_t st) {
    if (mode == kModeSet) launch_stream<VEC, kModeSet, float>(plane, S, R, C, acc, nullptr, count, st);
    else if (mode == kModeAdd) launch_stream<VEC, kModeAdd, float>(plane, S, R, C, acc, nullptr, count, st);
    else if (out_dtype == MRISR_WINDOW_F32) launch_stream<VEC, kModeFinish, float>(plane, S, R, C, acc, out, count, st);
    else launch_stream<VEC, kModeFinish, int16_t>(plane, S, R, C, acc, out, count, st);
}

template <int MODE, typename T>
static void launch_transpose(const float* plane, int S, int R, int C, float* acc, void* out, int count, hipStream_t st) {
    const dim3 grid(ceil_div(S, kTileS), ceil_div(C, kTileC), R);
    up2_blend_transpose_kernel<MODE, T><<<grid, 256, 0, st>>>(plane, S, R, C, acc, (T*)out, count);
}

// acc and out are optional in some modes: a pointer that is not there is not misaligned
static bool aligned(const void* p, size_t bytes) { return p == nullptr || aligned_to(p, bytes); }

extern "C" int mrisr_f32_volume_up2_blend(const float* plane, int axis, int X, int Y, int Z, float* acc, int mode, int count,
                                          int out_dtype, void* out, void* stream) {
    if (axis < 0 || axis > 2) MRISR_FAIL(MRISR_E_ARG, "f32_volume_up2_blend: axis %d", axis);
    if (mode != kModeSet && mode != kModeAdd && mode != kModeFinish) MRISR_FAIL(MRISR_E_ARG, "f32_volume_up2_blend: mode %d", mode);
    const bool finish = mode == kModeFinish;
    if (finish && out_dtype != MRISR_WINDOW_F32 && out_dtype != MRISR_WINDOW_I16)
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_up2_blend: out_dtype %d", out_dtype);
    if (finish && count < 1) MRISR_FAIL(MRISR_E_ARG, "f32_volume_up2_blend: count %d", count);
    const bool needs_acc = !finish || count > 1;      // a single-plane FINISH neither reads nor writes it
    if (!plane || (finish && !out) || (needs_acc && !acc)) MRISR_FAIL(MRISR_E_ARG, "f32_volume_up2_blend: null pointer");
    if (const int rc = check_volume_extents("f32_volume_up2_blend", X, Y, Z)) return rc;
    if (!finish) out = nullptr;
    const size_t out_elem = finish && out_dtype == MRISR_WINDOW_I16 ? 2 : 4;
    hipStream_t st = (hipStream_t)stream;
    if (axis == 2) {
        if (!aligned(plane, 4) || !aligned(acc, 8) || !aligned(out, 2 * out_elem)) MRISR_FAIL(MRISR_E_ARG, "f32_volume_up2_blend: misaligned pointer");
        const int S = Z, R = 2 * X, C = 2 * Y;
        if (mode == kModeSet) launch_transpose<kModeSet, float>(plane, S, R, C, acc, nullptr, count, st);
        else if (mode == kModeAdd) launch_transpose<kModeAdd, float>(plane, S, R, C, acc, nullptr, count, st);
        else if (out_dtype == MRISR_WINDOW_F32) launch_transpose<kModeFinish, float>(plane, S, R, C, acc, out, count, st);
        else launch_transpose<kModeFinish, int16_t>(plane, S, R, C, acc, out, count, st);
    } else {
        // axis 0: whole slices are contiguous in plane and acc alike, so one "row" of 2Y * 2Z (a multiple of 4) per slice
        const int S = axis == 0 ? X : Y, R = axis == 0 ? 1 : 2 * X;
        const size_t row = axis == 0 ? (size_t)4 * Y * Z : (size_t)2 * Z;
        if (row > 0x7ffffffcull) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_up2_blend: doubled slice of %zu voxels (at most 2^31 - 4)", row);
        const int C = (int)row;
        if (C % 4 == 0 && aligned(plane, 16) && aligned(acc, 16) && aligned(out, 4 * out_elem))
            dispatch_stream<4>(plane, S, R, C, acc, mode, count, out_dtype, out, st);
        else if (aligned(plane, 8) && aligned(acc, 8) && aligned(out, 2 * out_elem))
            dispatch_stream<2>(plane, S, R, C, acc, mode, count, out_dtype, out, st);
        else
            MRISR_FAIL(MRISR_E_ARG, "f32_volume_up2_blend: misaligned pointer");
    }
    MRISR_CHECK_LAUNCH("f32_volume_up2_blend");
    return MRISR_OK;
}
