// Surface distances between label volumes on the device (gfx950; extension): the boundary voxels of a label
// volume, the exact squared Euclidean distance transform of a voxel set with anisotropic voxel sizes, and the gather that turns
// the transform into the distances of one surface to another with their count, float64 sum and maximum.  The specification is
// mri_superresolution_amd/volume_surface.py; every kernel here is bit-equal to it.  Compiled with -ffp-contract=off (build.py): a
// candidate of the transform is a rounded float32 product (the weight times the exactly representable d * d) and a rounded
// float32 sum, never an fma.
//
// A volume is (X, Y, Z) in C order, Z fastest.
//
//   label_boundary   one thread per voxel: the label where one of the 6 face neighbours differs, else 0; optionally counts the voxels
//                    whose label lies above `classes`.
//   edt_sq           three launches, in place in `out`, no scratch volume.  g = 0 at the sites, +inf elsewhere; then along axis 2,
//                    1, 0:  g'[i] = min_j fl32(g[j] + fl32(w * fl32((i - j)^2))).  Rounding is monotone, so the result is the minimum
//                    of a set and no order of the candidates changes a bit; infinities take part like numbers (inf + t = inf).
//       axis 2       a wave owns a line (a row of Z voxels) in LDS, formed from the bytes while staging; lane l owns the voxels l,
//                    l + 64, ...  At distance d the lanes read g[i - d] and g[i + d]: consecutive LDS words.
//       axes 1, 0    a workgroup stages a tile of whole lines, n x W floats (W = 64, 32 or 16 neighbouring columns of the contiguous
//                    axis, n * W * 4 <= 64 KB), so that global accesses are W * 4 contiguous bytes and lane (column c, line
//                    position i) reads tile[(i -+ d) * W + c]: the 64 lanes of a wave read 64 consecutive words.  For axis 0 the
//                    columns run over the flattened (y, z) plane.  The tile is read completely before any of it is written back,
//                    and tiles are disjoint: the pass works in place.
//       the walk     from a voxel outwards, d = 1, 2, ...: both candidates at distance d share t = fl32(w * d^2), and
//                    min(a + t, b + t) = min(a, b) + t bit for bit (monotone rounding).  Without `full_scan` the walk ends once
//                    t >= best for every lane of the wave: g >= 0, so no candidate further out can be smaller, and t does not
//                    fall as d grows.  The vote is wave-uniform: no lane leaves the loop alone.  A line without a site is +inf
//                    and skips the walk in the first pass.
//   surface_gather   dist = sqrtf(d2) and sel = 1 where query == value, both 0 elsewhere; the count, the float64 sum of the finite
//                    distances and the maximum (as the integer maximum of the bits: the values are not negative) per workgroup
//                    in a fixed slot, thread t of workgroup b taking b chunk + t, + 256, ... in that order; a second launch of one
//                    thread adds the slots in ascending order.  No floating-point atomics: every run gives the same bits.
// No kernel reads or writes outside its volume: extents of 1, odd extents, fewer lines than a tile and lines shorter than a wave
// take the same code with idle lanes.
#include "volume_common.h"

constexpr int kEdtMaxDim = 1024;           // longest line: 1024 floats x 16 columns = 64 KB of LDS
constexpr int kEdtMaxBlocks = 1 << 16;
constexpr int kBoundaryPerBlock = 2048;
constexpr int kBoundaryMaxBlocks = 1 << 16;
constexpr int kGatherSlots = 1024;
constexpr int kGatherPerThread = 16;
#define EDT_INF __builtin_huge_valf()

struct SurfaceSlot {
    long long count;
    double sum;
    unsigned long long max_bits;
};

// ---------------------------------------------------------------- the boundary of a label volume

__global__ __launch_bounds__(256) void label_boundary_kernel(const uint8_t* __restrict__ labels, int X, int Y, int Z, int background,
                                                             int classes, uint8_t* __restrict__ out,
                                                             unsigned long long* __restrict__ above) {
    const size_t n = (size_t)X * Y * Z, plane = (size_t)Y * Z;
    unsigned nabove = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned l = labels[i];
        if (l > (unsigned)classes) ++nabove;
        unsigned edge = 0u;
        if (l) {
            const int x = (int)(i / plane);
            const size_t r = i - (size_t)x * plane;
            const int y = (int)(r / (size_t)Z), z = (int)(r - (size_t)y * Z);
            auto differs = [&](bool inside, size_t j) -> unsigned {
                if (!inside) return background ? 1u : 0u;
                const unsigned m = labels[j];
                return m != l && (background || m != 0u) ? 1u : 0u;
            };
            edge = differs(x > 0, i - plane) | differs(x < X - 1, i + plane) | differs(y > 0, i - Z) | differs(y < Y - 1, i + Z) |
                   differs(z > 0, i - 1) | differs(z < Z - 1, i + 1);
        }
        out[i] = (uint8_t)(edge ? l : 0u);
    }
    if (above) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nabove += (unsigned)__shfl_xor((int)nabove, o, 64);
        if ((threadIdx.x & 63) == 0 && nabove) atomicAdd(above, (unsigned long long)nabove);
    }
}

// ---------------------------------------------------------------- the distance transform

// The minimum over a line of n values `stride` floats apart in LDS for position i, starting from best = line[i] (d = 0: t = 0).
// Every lane of the wave calls it; an idle lane passes i = 0 and best = 0 and never holds the others back.
template <bool FULL>
__device__ __forceinline__ float edt_walk(const float* line, int stride, int i, int n, float w, float best) {
    for (int d = 1; d < n; ++d) {
        const float t = __fmul_rn(w, (float)(d * d));                  // d <= 1023: d * d is exact in float32
        if (!FULL && __all(t >= best)) break;
        const int lo = i - d, hi = i + d;
        const float a = lo >= 0 ? line[lo * stride] : EDT_INF;
        const float b = hi < n ? line[hi * stride] : EDT_INF;
        best = fminf(best, __fadd_rn(fminf(a, b), t));
    }
    return best;
}

// axis 2: wave v of workgroup b takes the rows 4 b + v, + 4 gridDim.x, ...
template <bool FULL>
__global__ __launch_bounds__(256) void edt_first_kernel(const uint8_t* __restrict__ sites, long long rows, int Z, int value, float w,
                                                        float* __restrict__ out) {
    __shared__ float g[4][kEdtMaxDim];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* line = g[wave];
    for (long long r0 = (long long)blockIdx.x * 4; r0 < rows; r0 += (long long)gridDim.x * 4) {
        const long long row = r0 + wave;
        const bool valid = row < rows;                                 // wave-uniform
        int found = 0;
        if (valid) {
            const uint8_t* src = sites + (size_t)row * Z;
            for (int z = lane; z < Z; z += 64) {
                const unsigned s = src[z];
                const bool site = value ? s == (unsigned)value : s != 0u;
                line[z] = site ? 0.f : EDT_INF;
                found |= site;
            }
        }
        __syncthreads();
        if (valid) {
            const bool any = __any(found);
            float* dst = out + (size_t)row * Z;
            for (int z0 = 0; z0 < Z; z0 += 64) {
                const int z = z0 + lane;
                const bool active = z < Z;
                float best = active ? line[z] : 0.f;
                if (any) best = edt_walk<FULL>(line, 1, active ? z : 0, Z, w, best);
                if (active) dst[z] = best;
            }
        }
        __syncthreads();
    }
}

// axes 1 and 0, in place: line position j of column m of outer index o lies at vol[o * outer_stride + j * line_stride + m], m < M
template <int W, bool FULL>
__global__ __launch_bounds__(256) void edt_axis_kernel(float* vol, int n, size_t line_stride, long long M, long long outer,
                                                       size_t outer_stride, float w) {
    extern __shared__ float tile[];                                    // n x W
    constexpr int Q = 256 / W;
    const int c = threadIdx.x % W, q = threadIdx.x / W;
    const long long chunks = (M + W - 1) / W, tiles = outer * chunks;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long o = t / chunks, m = (t - o * chunks) * W + c;
        const bool in = m < M;
        float* base = vol + (size_t)o * outer_stride + (size_t)(in ? m : 0);
        for (int j = q; j < n; j += Q) tile[j * W + c] = in ? base[(size_t)j * line_stride] : 0.f;
        __syncthreads();
        for (int i0 = 0; i0 < n; i0 += Q) {
            const int i = i0 + q;
            const bool active = in && i < n;
            float best = active ? tile[i * W + c] : 0.f;
            best = edt_walk<FULL>(tile + c, W, active ? i : 0, n, w, best);
            if (active) base[(size_t)i * line_stride] = best;
        }
        __syncthreads();
    }
}

template <bool FULL>
static void launch_edt_axis(float* vol, int n, size_t line_stride, long long M, long long outer, size_t outer_stride, float w,
                            hipStream_t s) {
    const int W = n <= 256 && M > 32 ? 64 : (n <= 512 && M > 16 ? 32 : 16);      // n * W * 4 <= 64 KB
    const long long tiles = outer * ((M + W - 1) / W);
    const int grid = (int)(tiles < kEdtMaxBlocks ? tiles : kEdtMaxBlocks);
    const size_t lds = (size_t)n * W * sizeof(float);
    if (W == 64) edt_axis_kernel<64, FULL><<<grid, 256, lds, s>>>(vol, n, line_stride, M, outer, outer_stride, w);
    else if (W == 32) edt_axis_kernel<32, FULL><<<grid, 256, lds, s>>>(vol, n, line_stride, M, outer, outer_stride, w);
    else edt_axis_kernel<16, FULL><<<grid, 256, lds, s>>>(vol, n, line_stride, M, outer, outer_stride, w);
}

// ---------------------------------------------------------------- the gather

// workgroup b owns the elements [b chunk, (b + 1) chunk); thread t of it the elements b chunk + t, + 256, ... in that order
__global__ __launch_bounds__(256) void surface_gather_kernel(const float* __restrict__ d2, const uint8_t* __restrict__ query, int value,
                                                             size_t n, size_t chunk, float* __restrict__ dist, uint8_t* __restrict__ sel,
                                                             SurfaceSlot* __restrict__ slots) {
    __shared__ double ssum[4];
    __shared__ long long scount[4];
    __shared__ unsigned smax[4];
    const size_t lo = (size_t)blockIdx.x * chunk;
    const size_t hi = lo + chunk < n ? lo + chunk : n;
    double s = 0.0;
    long long cnt = 0;
    unsigned mx = 0u;
    for (size_t i = lo + threadIdx.x; i < hi; i += 256) {
        const bool on = query[i] == (uint8_t)value;
        // the float64 root rounded to float32 is the correctly rounded float32 root (53 >= 2 * 24 + 2 bits), as in volume_denoise.hip
        const float d = on ? (float)__dsqrt_rn((double)d2[i]) : 0.f;
        dist[i] = d;
        sel[i] = on ? 1 : 0;
        if (on) {
            ++cnt;
            if (d < EDT_INF) s += (double)d;                           // an infinity never reaches the sum
            const unsigned bits = __float_as_uint(d);                  // d >= 0: the order of the bits is the order of the values
            mx = bits > mx ? bits : mx;
        }
    }
    s = wave_sum_d(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        const unsigned other = (unsigned)__shfl_xor((int)mx, o, 64);
        mx = other > mx ? other : mx;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        ssum[wave] = s;
        scount[wave] = cnt;
        smax[wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        slots[blockIdx.x].sum = ((ssum[0] + ssum[1]) + ssum[2]) + ssum[3];
        slots[blockIdx.x].count = ((scount[0] + scount[1]) + scount[2]) + scount[3];
        const unsigned m01 = smax[0] > smax[1] ? smax[0] : smax[1], m23 = smax[2] > smax[3] ? smax[2] : smax[3];
        slots[blockIdx.x].max_bits = m01 > m23 ? m01 : m23;
    }
}

// result: 3 words of 8 bytes - the count (int64), the sum (float64), the maximum (float32 in the low half, 0 in the high half)
__global__ void surface_gather_finish_kernel(const SurfaceSlot* __restrict__ slots, int nslots, unsigned long long* __restrict__ result) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    long long c = 0;
    unsigned long long mx = 0ull;
    for (int b = 0; b < nslots; ++b) {
        s += slots[b].sum;
        c += slots[b].count;
        mx = slots[b].max_bits > mx ? slots[b].max_bits : mx;
    }
    result[0] = (unsigned long long)c;
    result[1] = (unsigned long long)__double_as_longlong(s);
    result[2] = mx;
}

// ---------------------------------------------------------------- entries

static inline bool weight_ok(float w) { return w > 0.f && isfinite(w); }

extern "C" int mrisr_u8_volume_label_boundary(const unsigned char* labels, int X, int Y, int Z, int background, int classes,
                                              unsigned char* out, unsigned long long* above, void* stream) {
    if (!labels || !out) MRISR_FAIL(MRISR_E_ARG, "u8_volume_label_boundary: null pointer");
    if (above && !aligned_to(above, 8)) MRISR_FAIL(MRISR_E_ARG, "u8_volume_label_boundary: misaligned pointer");
    if (labels == out) MRISR_FAIL(MRISR_E_ARG, "u8_volume_label_boundary: labels and out must be two buffers");
    if (background != 0 && background != 1) MRISR_FAIL(MRISR_E_ARG, "u8_volume_label_boundary: background %d (0 or 1)", background);
    if (classes < 1 || classes > 255) MRISR_FAIL(MRISR_E_ARG, "u8_volume_label_boundary: %d classes (1..255)", classes);
    if (const int rc = check_volume_extents("u8_volume_label_boundary", X, Y, Z)) return rc;
    const size_t n = (size_t)X * Y * Z;
    label_boundary_kernel<<<capped_grid(n, kBoundaryPerBlock, kBoundaryMaxBlocks), 256, 0, (hipStream_t)stream>>>(labels, X, Y, Z, background,
                                                                                                                classes, out, above);
    MRISR_CHECK_LAUNCH("u8_volume_label_boundary");
    return MRISR_OK;
}

// passes: bit a set = the pass along axis a is made
template <bool FULL>
static int run_edt(const unsigned char* sites, int X, int Y, int Z, int value, float wx, float wy, float wz, float* out, int passes,
                   hipStream_t s) {
    const long long rows = (long long)X * Y;
    const int grid = (int)((rows + 3) / 4 < kEdtMaxBlocks ? (rows + 3) / 4 : kEdtMaxBlocks);
    const size_t plane = (size_t)Y * Z;
    if (passes & 4) {
        edt_first_kernel<FULL><<<grid, 256, 0, s>>>(sites, rows, Z, value, wz, out);
        MRISR_CHECK_LAUNCH("u8_volume_edt_sq (axis 2)");
    }
    if (passes & 2) {
        launch_edt_axis<FULL>(out, Y, (size_t)Z, Z, X, plane, wy, s);
        MRISR_CHECK_LAUNCH("u8_volume_edt_sq (axis 1)");
    }
    if (passes & 1) {
        launch_edt_axis<FULL>(out, X, plane, (long long)plane, 1, 0, wx, s);
        MRISR_CHECK_LAUNCH("u8_volume_edt_sq (axis 0)");
    }
    return MRISR_OK;
}

extern "C" int mrisr_u8_volume_edt_sq(const unsigned char* sites, int X, int Y, int Z, int value, float wx, float wy, float wz, float* out,
                                      int passes, int full_scan, void* stream) {
    if (!sites || !out) MRISR_FAIL(MRISR_E_ARG, "u8_volume_edt_sq: null pointer");
    if (!aligned_to(out, 4)) MRISR_FAIL(MRISR_E_ARG, "u8_volume_edt_sq: misaligned pointer");
    if (value < 0 || value > 255) MRISR_FAIL(MRISR_E_ARG, "u8_volume_edt_sq: value %d (0..255)", value);
    if (!weight_ok(wx) || !weight_ok(wy) || !weight_ok(wz))
        MRISR_FAIL(MRISR_E_ARG, "u8_volume_edt_sq: weights %g, %g, %g (finite, positive)", (double)wx, (double)wy, (double)wz);
    if (passes < 1 || passes > 7) MRISR_FAIL(MRISR_E_ARG, "u8_volume_edt_sq: passes %d (a mask of the axes, 1..7; 7: the transform)", passes);
    if (full_scan != 0 && full_scan != 1) MRISR_FAIL(MRISR_E_ARG, "u8_volume_edt_sq: full_scan %d (0 or 1)", full_scan);
    if (X < 1 || Y < 1 || Z < 1 || X > kEdtMaxDim || Y > kEdtMaxDim || Z > kEdtMaxDim)
        MRISR_FAIL(MRISR_E_SHAPE, "u8_volume_edt_sq: volume %d x %d x %d (every axis 1..%d: a line is staged in LDS)", X, Y, Z, kEdtMaxDim);
    return full_scan ? run_edt<true>(sites, X, Y, Z, value, wx, wy, wz, out, passes, (hipStream_t)stream)
                     : run_edt<false>(sites, X, Y, Z, value, wx, wy, wz, out, passes, (hipStream_t)stream);
}

extern "C" size_t mrisr_f32_volume_surface_workspace_bytes(void) { return (size_t)kGatherSlots * sizeof(SurfaceSlot); }

extern "C" int mrisr_f32_volume_surface_gather(const float* d2, const unsigned char* query, int value, size_t n, float* dist,
                                               unsigned char* sel, void* ws, unsigned long long* result, void* stream) {
    if (!d2 || !query || !dist || !sel || !ws || !result) MRISR_FAIL(MRISR_E_ARG, "f32_volume_surface_gather: null pointer");
    if (!aligned_to(d2, 4) || !aligned_to(dist, 4) || !aligned_to(ws, 8) || !aligned_to(result, 8))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_surface_gather: misaligned pointer");
    if (sel == query || dist == d2) MRISR_FAIL(MRISR_E_ARG, "f32_volume_surface_gather: dist and sel must be buffers of their own");
    if (value < 1 || value > 255) MRISR_FAIL(MRISR_E_ARG, "f32_volume_surface_gather: value %d (1..255)", value);
    if (n == 0 || n > 0xffffffffull) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_surface_gather: %zu voxels (1..2^32 - 1)", n);
    hipStream_t s = (hipStream_t)stream;
    SurfaceSlot* slots = (SurfaceSlot*)ws;
    const int nslots = capped_grid(n, (size_t)256 * kGatherPerThread, kGatherSlots);
    const size_t chunk = (n + (size_t)nslots - 1) / (size_t)nslots;
    surface_gather_kernel<<<nslots, 256, 0, s>>>(d2, query, value, n, chunk, dist, sel, slots);
    MRISR_CHECK_LAUNCH("f32_volume_surface_gather (sums)");
    surface_gather_finish_kernel<<<1, 64, 0, s>>>(slots, nslots, result);
    MRISR_CHECK_LAUNCH("f32_volume_surface_gather");
    return MRISR_OK;
}
