// Zero-filled x2 interpolation and k-space truncation of volumes (extension): one dense circulant transform
// along one axis.  The specification is mri_superresolution_amd/volume_kspace.py (zerofill2_np, truncate2_np); the tables come from
// the host (zerofill_table, truncate_table: float64, rounded once) and no cosine is evaluated here.
//
//   up2    out[2i + s] = sum_j D_s[(i - j) mod n] v[j]      s = 0, 1; a line of n samples becomes 2n
//   down2  out[i]      = sum_j T[(2i - j) mod N] v[j]       a line of N = 2n samples becomes n
//
// Every output is  0 + t v[0] + t v[1] + ...  over j ascending, each product and each sum rounded to float32 (this file is compiled
// with -ffp-contract=off and the two operations are written as __fmul_rn / __fadd_rn).  The blocking is over outputs, never over j, so
// the order of a sum does not depend on the launch shape.
//
// A workgroup takes a bundle of W lines: for the axes 0 and 1 lines that are neighbours along axis 2 (loads and stores coalesced
// across the bundle), for axis 2 W consecutive rows, which are one contiguous piece of memory and go through LDS transposed.  LDS
// holds the W source lines (sample j of line c at tile[j (W + 1) + c]) and the table row(s), unrolled to E[x] = row[(x + 1) mod
// period] so that the index  x = step i - j + period - 1  needs no modulo.  Thread (c, q) produces R consecutive outputs i of line c
// per chunk, both parities in up2 mode: per block of R source samples it reads its window of the table once (2R - 1 entries per row,
// 3R - 2 in down2 mode - the same address in all lanes of one q: a broadcast) and each v[j] once (lanes of one q read neighbouring
// words), and spends 2 R R (R R) multiply-add pairs on them.  No atomics, nothing data-dependent in control flow.
#include "volume_common.h"

namespace {

constexpr int kCircMaxUp = 512;            // the longest line of up2
constexpr int kCircMaxDown = 1024;         // the longest line of down2
constexpr int kCircR = 8;                  // outputs i per thread and chunk
constexpr long long kCircMaxVoxels = 2147483647LL;

// LDS floats of a launch: the unrolled table rows, the tile, and for axis 2 the output staging of one chunk
template <int W, bool UP, bool AXIS2> struct CircLayout {
    static constexpr int P = W + 1, Q = 256 / W, CH = Q * kCircR;       // tile pitch; threads per line; outputs i per chunk
    static constexpr int SEG = UP ? 2 * CH : CH, SP = SEG + 1;         // output samples of one line and chunk; staging pitch
    static constexpr int WIN = UP ? 2 * kCircR - 1 : 3 * kCircR - 2;    // table entries a block of R source samples needs
    __host__ __device__ static constexpr int ext(int n_in) { return 2 * n_in + 2 * kCircR; }      // floats of one unrolled row
    __host__ __device__ static constexpr size_t floats(int n_in) {
        return (size_t)(UP ? 2 : 1) * ext(n_in) + (size_t)n_in * P + (AXIS2 ? (size_t)W * SP : 0);
    }
};

// axes 0, 1: line position j of column m (< M) of outer index o lies at src[o * src_outer + j * line_stride + m]; workgroup
// blockIdx.x = o * ceil(M / W) + m / W.  axis 2: line_stride = 1, M = the number of rows, workgroup b takes the rows b W ... b W + W - 1.
template <int W, bool UP, bool AXIS2>
__global__ __launch_bounds__(256) void line_circulant_kernel(const float* __restrict__ src, const float* __restrict__ table,
                                                             float* __restrict__ dst, int n_in, size_t line_stride, long long M,
                                                             size_t src_outer, size_t dst_outer) {
    using Lay = CircLayout<W, UP, AXIS2>;
    constexpr int P = Lay::P, Q = Lay::Q, R = kCircR, CH = Lay::CH, WIN = Lay::WIN, SEG = Lay::SEG, SP = Lay::SP;
    extern __shared__ float lds[];
    const int n = UP ? n_in : n_in / 2;                      // outputs i per line
    const int n_out = UP ? 2 * n_in : n;
    const int ext = Lay::ext(n_in);
    float* E0 = lds;
    float* E1 = lds + (UP ? ext : 0);
    float* tile = lds + (UP ? 2 : 1) * ext;
    float* stage = tile + (size_t)n_in * P;                  // AXIS2 only
    const int tid = threadIdx.x, c = tid % W, q = tid / W;

    // E[x] = row[(x + 1) mod n_in]: every index the loops below form lies in [0, ext)
    for (int x = tid; x < ext; x += 256) {
        const int d = (x + 1) % n_in;
        E0[x] = table[d];
        if constexpr (UP) E1[x] = table[n_in + d];
    }

    bool in = false;
    float* out_base = dst;
    long long row0 = 0;
    if (AXIS2) {
        row0 = (long long)blockIdx.x * W;
        const long long left = M - row0;                     // rows of this bundle that exist (>= 1)
        const size_t total = (size_t)W * n_in, have = (size_t)(left < W ? left : W) * n_in;
        const float* base = src + (size_t)row0 * n_in;
        for (size_t e = tid; e < total; e += 256) {
            const int row = (int)(e / n_in), j = (int)(e - (size_t)row * n_in);
            tile[j * P + row] = e < have ? base[e] : 0.f;
        }
    } else {
        const long long chunks = (M + W - 1) / W;
        const long long o = blockIdx.x / chunks, m = (blockIdx.x - o * chunks) * W + c;
        in = m < M;
        const float* base = src + (size_t)o * src_outer + (size_t)(in ? m : 0);
        for (int j = q; j < n_in; j += Q) tile[j * P + c] = in ? base[(size_t)j * line_stride] : 0.f;
        out_base = dst + (size_t)o * dst_outer + (size_t)(in ? m : 0);
    }
    __syncthreads();

    const float* col = tile + c;
    const int full = n_in - n_in % R;                        // source samples taken in blocks of R
    for (int ib = 0; ib < n; ib += CH) {
        const int i0 = ib + q * R;
        const int ic = i0 < n ? i0 : 0;                      // a thread past the end works on output 0 and stores nothing
        const int x0 = (UP ? ic : 2 * ic) + n_in - 1;        // the table index of output ic at j = 0
        float a0[R], a1[R];
#pragma unroll
        for (int r = 0; r < R; ++r) a0[r] = a1[r] = 0.f;
        for (int j0 = 0; j0 < full; j0 += R) {
            // output ic + r at source sample j0 + u reads E[xb + (UP ? r : 2 r) - u + R - 1]
            const int xb = x0 - j0 - (R - 1);
            float w0[WIN], w1[UP ? WIN : 1];
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                w0[k] = E0[xb + k];
                if constexpr (UP) w1[k] = E1[xb + k];
            }
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const float v = col[(j0 + u) * P];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int k = (UP ? r : 2 * r) - u + R - 1;
                    a0[r] = __fadd_rn(a0[r], __fmul_rn(w0[k], v));
                    if constexpr (UP) a1[r] = __fadd_rn(a1[r], __fmul_rn(w1[k], v));
                }
            }
        }
        for (int j = full; j < n_in; ++j) {                  // the last n_in mod R source samples, one at a time
            const float v = col[j * P];
            const int x = x0 - j;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int k = x + (UP ? r : 2 * r);
                a0[r] = __fadd_rn(a0[r], __fmul_rn(E0[k], v));
                if constexpr (UP) a1[r] = __fadd_rn(a1[r], __fmul_rn(E1[k], v));
            }
        }
        if (AXIS2) {
            // through LDS, so that a row's outputs leave in order: stage[c][the output's position inside this chunk]
            float* s = stage + c * SP + (UP ? 2 : 1) * q * R;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (UP) {
                    s[2 * r] = a0[r];
                    s[2 * r + 1] = a1[r];
                } else {
                    s[r] = a0[r];
                }
            }
            __syncthreads();
            const int obase = (UP ? 2 : 1) * ib;             // the chunk's first output sample
            for (int e = tid; e < W * SEG; e += 256) {
                const int cc = e / SEG, o = e - cc * SEG;
                const long long orow = row0 + cc;
                if (orow < M && obase + o < n_out) dst[(size_t)orow * n_out + obase + o] = stage[cc * SP + o];
            }
            __syncthreads();
        } else if (in && i0 < n) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (i0 + r < n) {
                    if (UP) {
                        out_base[(size_t)(2 * (i0 + r)) * line_stride] = a0[r];
                        out_base[(size_t)(2 * (i0 + r) + 1) * line_stride] = a1[r];
                    } else {
                        out_base[(size_t)(i0 + r) * line_stride] = a0[r];
                    }
                }
            }
        }
    }
}

template <int W, bool UP, bool AXIS2>
static void launch_bundles(const float* src, const float* table, float* dst, int n_in, size_t line_stride, long long M, long long outer,
                           size_t src_outer, size_t dst_outer, hipStream_t s) {
    const long long bundles = outer * ((M + W - 1) / W);     // at most the voxel count: inside int
    const size_t lds = CircLayout<W, UP, AXIS2>::floats(n_in) * sizeof(float);      // below 64 KiB for every W the caller picks
    line_circulant_kernel<W, UP, AXIS2><<<(unsigned)bundles, 256, lds, s>>>(src, table, dst, n_in, line_stride, M, src_outer, dst_outer);
}

// the bundle width by the line's length: the tile of W lines stays near 34 KiB, two workgroups per CU
template <bool UP, bool AXIS2>
static void launch_circulant(const float* src, const float* table, float* dst, int n_in, size_t line_stride, long long M, long long outer,
                             size_t src_outer, size_t dst_outer, hipStream_t s) {
    if (n_in <= 128) launch_bundles<64, UP, AXIS2>(src, table, dst, n_in, line_stride, M, outer, src_outer, dst_outer, s);
    else if (n_in <= 256) launch_bundles<32, UP, AXIS2>(src, table, dst, n_in, line_stride, M, outer, src_outer, dst_outer, s);
    else if (n_in <= 512) launch_bundles<16, UP, AXIS2>(src, table, dst, n_in, line_stride, M, outer, src_outer, dst_outer, s);
    else launch_bundles<8, UP, AXIS2>(src, table, dst, n_in, line_stride, M, outer, src_outer, dst_outer, s);
}

template <bool UP>
static void run_circulant(const float* src, int X, int Y, int Z, int axis, const float* table, float* dst, hipStream_t s) {
    const int ext[3] = {X, Y, Z};
    const int n_in = ext[axis], n_out = UP ? 2 * n_in : n_in / 2;
    if (axis == 2) {
        launch_circulant<UP, true>(src, table, dst, n_in, 1, (long long)X * Y, 1, 0, 0, s);
    } else if (axis == 1) {
        launch_circulant<UP, false>(src, table, dst, n_in, (size_t)Z, Z, X, (size_t)Y * Z, (size_t)n_out * Z, s);
    } else {
        launch_circulant<UP, false>(src, table, dst, n_in, (size_t)Y * Z, (long long)Y * Z, 1, 0, 0, s);
    }
}

}  // namespace

extern "C" int mrisr_f32_volume_line_circulant(const float* src, int X, int Y, int Z, int axis, int mode, const float* table, float* dst,
                                               void* stream) {
    if (!src || !table || !dst) MRISR_FAIL(MRISR_E_ARG, "f32_volume_line_circulant: null pointer");
    if (!aligned_to(src, 4) || !aligned_to(table, 4) || !aligned_to(dst, 4)) MRISR_FAIL(MRISR_E_ARG, "f32_volume_line_circulant: misaligned pointer");
    if (src == dst) MRISR_FAIL(MRISR_E_ARG, "f32_volume_line_circulant: src and dst must be two buffers");
    if (axis < 0 || axis > 2) MRISR_FAIL(MRISR_E_ARG, "f32_volume_line_circulant: axis %d (0..2)", axis);
    if (mode != MRISR_CIRCULANT_UP2 && mode != MRISR_CIRCULANT_DOWN2) MRISR_FAIL(MRISR_E_ARG, "f32_volume_line_circulant: unknown mode %d", mode);
    if (const int rc = check_volume_extents("f32_volume_line_circulant", X, Y, Z)) return rc;
    const int n = axis == 0 ? X : (axis == 1 ? Y : Z);
    const long long voxels = (long long)X * Y * Z;
    if (mode == MRISR_CIRCULANT_UP2) {
        if (n > kCircMaxUp) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_line_circulant: a line of %d samples (up2: 1..%d)", n, kCircMaxUp);
        if (2 * voxels > kCircMaxVoxels) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_line_circulant: more than 2^31 - 1 voxels in dst");
        run_circulant<true>(src, X, Y, Z, axis, table, dst, (hipStream_t)stream);
    } else {
        if (n > kCircMaxDown || n % 2) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_line_circulant: a line of %d samples (down2: even, 2..%d)", n, kCircMaxDown);
        if (voxels > kCircMaxVoxels) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_line_circulant: more than 2^31 - 1 voxels in src");
        run_circulant<false>(src, X, Y, Z, axis, table, dst, (hipStream_t)stream);
    }
    MRISR_CHECK_LAUNCH("f32_volume_line_circulant");
    return MRISR_OK;
}
