// Deformable registration of volumes on the device (gfx950; extension): Thirion's demons with an additive
// update and a Gaussian regularisation of the field, and its diffeomorphic variant.  The specification is volume_deform.warp_np /
// demons_force_np / smooth_field_np / jacobian_stats_np / compose_np / demons_update_np / warp_matrix_np; every kernel here is
// bit-equal to it.  Compiled with -ffp-contract=off (build.py): every product, sum, difference and division is rounded on its own,
// never an fma.
//
// A volume is (X, Y, Z) in C order, Z fastest; a field u is (3, X, Y, Z) float32 in voxels: fixed(x) is compared with
// moving(x + u(x)).  The coordinate of a voxel is p_a = (double)i_a + (double)u_a, the inside test, the taps and the reduction
// are reslice_np's (volume_taps.h); a NaN or infinite displacement fails the inside test.
//
//   f32_volume_warp            one thread per voxel, a workgroup per 2 x 2 x 64 brick as in volume_reslice.hip: the three
//                              displacement loads and the store of a wave are runs of 64 floats, and since a field is smooth
//                              the taps of a wave fall into a few rows of the moving volume (vector cache and L2).
//   f32_volume_demons_force    the hot path, one launch: the linear gather of moving at x + u, the 6-neighbour stencil of fixed,
//                              the force and v = u + upd; 5 floats read and 3 written per voxel, no d and no gradient volume.
//                              At most kSlots workgroups walk the bricks with a stride of the grid; a thread adds the squares of
//                              its finite differences as a float64 pair (sum, rounding error: two_sum), the waves and the
//                              workgroup add their pairs in a fixed order and every workgroup leaves (sum, error, count) in its
//                              slot.  The slots are added in a fixed order by one wave of a LATER launch - the first workgroup of
//                              the smoothing pass that follows, or a launch of one wave when the caller wants the row at once -
//                              so nothing is handed between workgroups inside a launch and there is no floating-point atomic:
//                              the same bits on every run.
//   f32_volume_demons_update   the same kernel under a template flag, writing w = upd * scale (scale = 2^-K) instead of u + upd: the
//                              update of the diffeomorphic variant, which is squared K times and composed with the field.
//   f32_volume_field_compose   out = v + (u at x + v(x)), compose_np: one thread per voxel on the warp kernel's bricks; the three
//                              coordinates - clamped into the grid by comparisons, a field continues constantly past its faces -
//                              and the eight taps once per voxel for all three components: 3 coalesced loads of v, 24 gathered
//                              loads of u, 3 stores.  u and v may be one buffer (squaring).
//   f32_volume_warp_matrix     moving at M (x + u(x)), warp_matrix_np: the warp kernel with the 3 x 4 matrix of the reslice by value
//                              between the field and the inside test - one interpolation instead of a reslice and a warp.
//   f32_volume_field_smooth    one pass along one axis, all three components (they are the slowest axis of the field: the z and y
//                              passes see a volume of 3 X slabs, the x pass three slabs with columns of Y Z).  A workgroup stages
//                              its tile plus the halo in LDS once, the index of a staged element clamped into the axis (the border
//                              is replicated, not zero: a zero border drags the field to zero at the faces).  Radius at most 16:
//                              at most 16 KB of LDS per workgroup, far from the CU's 160 KB.
//   f32_volume_jacobian_stats  det(I + grad u) by the gradient rule of the force, its minimum and the count of det <= 0 through the
//                              same slots, finalised by a launch of one wave.
// The brick walk, the slots and the volume check are volume_bricks.h's (through volume_deform.h), gather and gather_at volume_taps.h's.
#include "volume_deform.h"
#include "volume_taps.h"

// the coordinate of voxel (i, j, k) under the field and the inside test
__device__ __forceinline__ bool field_coordinate(const float* __restrict__ u, size_t n, size_t idx, int i, int j, int k, int X, int Y,
                                                 int Z, float* ua, double* p) {
    const int at[3] = {i, j, k}, ext[3] = {X, Y, Z};
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ua[a] = u[a * n + idx];
        p[a] = __dadd_rn((double)at[a], (double)ua[a]);
        inside = inside && p[a] >= -0.5 && p[a] <= (double)ext[a] - 0.5;      // NaN compares false
    }
    return inside;
}

template <int METHOD>
__global__ __launch_bounds__(256) void warp_kernel(const float* __restrict__ moving, const float* __restrict__ u, int X, int Y, int Z,
                                                   float fill, float* __restrict__ out, unsigned nby, unsigned nbz) {
    int i, j, k;
    if (!brick_voxel(blockIdx.x, nby, nbz, X, Y, Z, i, j, k)) return;
    const size_t n = (size_t)X * Y * Z, idx = ((size_t)i * Y + j) * Z + k;
    float ua[3];
    double p[3];
    const bool inside = field_coordinate(u, n, idx, i, j, k, X, Y, Z, ua, p);
    out[idx] = inside ? gather<METHOD>(moving, X, Y, Z, p) : fill;
}

// moving (SX, SY, SZ) at M (x + u(x)): the coordinate under the field, then grid_coordinate's order, then the inside test of the source
template <int METHOD>
__global__ __launch_bounds__(256) void warp_matrix_kernel(const float* __restrict__ moving, int SX, int SY, int SZ,
                                                          const float* __restrict__ u, int X, int Y, int Z, Matrix34 g, float fill,
                                                          float* __restrict__ out, unsigned nby, unsigned nbz) {
    int i, j, k;
    if (!brick_voxel(blockIdx.x, nby, nbz, X, Y, Z, i, j, k)) return;
    const size_t n = (size_t)X * Y * Z, idx = ((size_t)i * Y + j) * Z + k;
    const int at[3] = {i, j, k}, ext[3] = {SX, SY, SZ};
    double q[3], p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = __dadd_rn((double)at[a], (double)u[a * n + idx]);
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = grid_coordinate(g.m[a], q[0], q[1], q[2]);
        inside = inside && p[a] >= -0.5 && p[a] <= (double)ext[a] - 0.5;      // NaN compares false
    }
    out[idx] = inside ? gather<METHOD>(moving, SX, SY, SZ, p) : fill;
}

// out = v + (u at x + v(x)): the three coordinates, clamped into the grid by comparisons (the field continues constantly past the
// faces), and the eight taps are computed once and serve all three components; a coordinate that is not a number makes all three NaN
__global__ __launch_bounds__(256) void compose_kernel(const float* __restrict__ u, const float* __restrict__ v, int X, int Y, int Z,
                                                      float* __restrict__ out, unsigned nby, unsigned nbz) {
    int i, j, k;
    if (!brick_voxel(blockIdx.x, nby, nbz, X, Y, Z, i, j, k)) return;
    const size_t n = (size_t)X * Y * Z, idx = ((size_t)i * Y + j) * Z + k;
    const int at[3] = {i, j, k}, ext[3] = {X, Y, Z};
    float va[3];
    double p[3];
    bool number = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        va[a] = v[a * n + idx];
        const double q = __dadd_rn((double)at[a], (double)va[a]), last = (double)(ext[a] - 1);
        p[a] = q < 0.0 ? 0.0 : (q > last ? last : q);      // NaN fails both and stays
        number = number && p[a] == p[a];
    }
    if (!number) {                                           // nothing of it is converted to an integer
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a * n + idx] = __uint_as_float(0x7fc00000u);
        return;
    }
    int ix[2], iy[2], iz[2];
    float wx[2], wy[2], wz[2];
    axis_taps<kLinear>(p[0], X, ix, wx);
    axis_taps<kLinear>(p[1], Y, iy, wy);
    axis_taps<kLinear>(p[2], Z, iz, wz);
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a * n + idx] = __fadd_rn(va[a], gather_at<2>(u + a * n, Y, Z, ix, iy, iz, wx, wy, wz));
}

// UPDATE: w = upd * scale (mrisr_f32_volume_demons_update); else v = u + upd (mrisr_f32_volume_demons_force, scale unused)
template <bool UPDATE>
__global__ __launch_bounds__(256) void demons_kernel(const float* __restrict__ fixed, const float* __restrict__ moving,
                                                     const float* __restrict__ u, int X, int Y, int Z, float max_step, float fill,
                                                     float scale, float* __restrict__ v, unsigned nbricks, unsigned nby, unsigned nbz,
                                                     DeformSlot* __restrict__ slots) {
    __shared__ DeformSlot part[4];
    const size_t n = (size_t)X * Y * Z;
    PairSum acc = {0.0, 0.0, 0};
    for (unsigned b = blockIdx.x; b < nbricks; b += gridDim.x) {
        int i, j, k;
        if (!brick_voxel(b, nby, nbz, X, Y, Z, i, j, k)) continue;
        const size_t idx = ((size_t)i * Y + j) * Z + k;
        float ua[3], upd[3] = {0.f, 0.f, 0.f};
        double p[3];
        const bool inside = field_coordinate(u, n, idx, i, j, k, X, Y, Z, ua, p);
        if (inside) {
            const float d = __fsub_rn(gather<kLinear>(moving, X, Y, Z, p), fixed[idx]);
            const float g[3] = {axis_gradient(fixed, idx, i, X, (size_t)Y * Z), axis_gradient(fixed, idx, j, Y, (size_t)Z),
                                axis_gradient(fixed, idx, k, Z, 1)};
            const float g2 = __fadd_rn(__fadd_rn(__fmul_rn(g[0], g[0]), __fmul_rn(g[1], g[1])), __fmul_rn(g[2], g[2]));
            const float den = __fadd_rn(g2, __fmul_rn(d, d));
            const float s = den > MRISR_DEFORM_DEN_MIN ? __fdiv_rn(d, den) : 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                float x = -__fmul_rn(s, g[a]);
                x = x > max_step ? max_step : (x < -max_step ? -max_step : x);
                upd[a] = x == x ? x : 0.f;
            }
            if (isfinite(d)) acc.add((double)d * (double)d, 0.0, 1);      // the square of a float is exact in double
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a * n + idx] = UPDATE ? __fmul_rn(upd[a], scale) : __fadd_rn(ua[a], upd[a]);
    }
    block_sum_to_slot(acc, part, &slots[blockIdx.x]);
}

// rows of Z floats, the filter along them; grid (blocks of kZRows rows, tiles of kZTile outputs)
__global__ __launch_bounds__(256) void smooth_z_kernel(const float* __restrict__ in, float* __restrict__ out, long long rows, int Z,
                                                       const float* __restrict__ taps, int R, const DeformSlot* slots, int nslots,
                                                       StatsRow* row_out) {
    __shared__ float tile[kZRows][kZTile + 2 * kMaxRadius];
    __shared__ float wl[2 * kMaxRadius + 1];
    const int t = threadIdx.x;
    if (slots && blockIdx.x == 0 && blockIdx.y == 0 && t < 64) finalize_force(slots, nslots, row_out);
    const long long row0 = (long long)blockIdx.x * kZRows;
    const int z0 = blockIdx.y * kZTile, Lt = kZTile + 2 * R;
    if (t <= 2 * R) wl[t] = taps[t];
    for (int e = t; e < kZRows * Lt; e += 256) {
        const int r = e / Lt, q = e - r * Lt;
        const long long row = row0 + r;
        if (row < rows) tile[r][q] = in[(size_t)row * Z + clampi(z0 - R + q, Z)];      // position q is z0 - R + q, the border replicated
    }
    __syncthreads();
    const int r = t >> 6, lane = t & 63;
    const long long row = row0 + r;
    if (row >= rows) return;
#pragma unroll
    for (int j = 0; j < kZTile / 64; ++j) {
        const int q = lane + 64 * j, z = z0 + q;
        if (z >= Z) break;
        float acc = 0.f;
        for (int k = 0; k <= 2 * R; ++k) acc = __fadd_rn(acc, __fmul_rn(wl[k], tile[r][q + k]));
        out[(size_t)row * Z + z] = acc;
    }
}

// [A][S][C] floats, the filter along S; grid (A x column groups of kSCols, tiles of kSGroups kSPer outputs)
__global__ __launch_bounds__(256) void smooth_stream_kernel(const float* __restrict__ in, float* __restrict__ out, int S, long long C,
                                                            unsigned ncg, const float* __restrict__ taps, int R,
                                                            const DeformSlot* slots, int nslots, StatsRow* row_out) {
    constexpr int T = kSGroups * kSPer;
    __shared__ float tile[T + 2 * kMaxRadius][kSCols];
    __shared__ float wl[2 * kMaxRadius + 1];
    const int t = threadIdx.x;
    if (slots && blockIdx.x == 0 && blockIdx.y == 0 && t < 64) finalize_force(slots, nslots, row_out);
    const unsigned a = blockIdx.x / ncg, cg = blockIdx.x - a * ncg;
    const long long c0 = (long long)cg * kSCols;
    const int s0 = blockIdx.y * T;
    const size_t slab = (size_t)a * (size_t)S * (size_t)C;
    if (t <= 2 * R) wl[t] = taps[t];
    const int col = t & 63, sg = t >> 6;
    const long long c = c0 + col;
    if (c < C)
        for (int q = sg; q < T + 2 * R; q += kSGroups)      // tile row q is s0 - R + q, the border replicated
            tile[q][col] = in[slab + (size_t)clampi(s0 - R + q, S) * (size_t)C + (size_t)c];
    __syncthreads();
    const int so = s0 + sg * kSPer;
    if (c >= C || so >= S) return;
    float acc[kSPer];
#pragma unroll
    for (int j = 0; j < kSPer; ++j) acc[j] = 0.f;
    for (int kp = 0; kp < 2 * R + kSPer; ++kp) {            // output j takes its tap kp - j from tile row sg kSPer + kp: ascending
        const float x = tile[sg * kSPer + kp][col];
#pragma unroll
        for (int j = 0; j < kSPer; ++j) {
            const int k = kp - j;
            if (k >= 0 && k <= 2 * R) acc[j] = __fadd_rn(acc[j], __fmul_rn(wl[k], x));
        }
    }
#pragma unroll
    for (int j = 0; j < kSPer; ++j)
        if (so + j < S) out[slab + (size_t)(so + j) * (size_t)C + (size_t)c] = acc[j];
}

__global__ __launch_bounds__(256) void jacobian_kernel(const float* __restrict__ u, int X, int Y, int Z, unsigned nbricks, unsigned nby,
                                                       unsigned nbz, DeformSlot* __restrict__ slots) {
    __shared__ float smin[4];
    __shared__ long long scount[4];
    const size_t n = (size_t)X * Y * Z;
    float m = __uint_as_float(0x7f800000u);      // +inf: a determinant that is not a number never enters
    long long c = 0;
    for (unsigned b = blockIdx.x; b < nbricks; b += gridDim.x) {
        int i, j, k;
        if (!brick_voxel(b, nby, nbz, X, Y, Z, i, j, k)) continue;
        const size_t idx = ((size_t)i * Y + j) * Z + k;
        float J[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float* ua = u + a * n;
            J[a][0] = axis_gradient(ua, idx, i, X, (size_t)Y * Z);
            J[a][1] = axis_gradient(ua, idx, j, Y, (size_t)Z);
            J[a][2] = axis_gradient(ua, idx, k, Z, 1);
            J[a][a] = __fadd_rn(1.f, J[a][a]);
        }
        const float c0 = __fsub_rn(__fmul_rn(J[1][1], J[2][2]), __fmul_rn(J[1][2], J[2][1]));
        const float c1 = __fsub_rn(__fmul_rn(J[1][0], J[2][2]), __fmul_rn(J[1][2], J[2][0]));
        const float c2 = __fsub_rn(__fmul_rn(J[1][0], J[2][1]), __fmul_rn(J[1][1], J[2][0]));
        const float det = __fadd_rn(__fsub_rn(__fmul_rn(J[0][0], c0), __fmul_rn(J[0][1], c1)), __fmul_rn(J[0][2], c2));
        if (det < m) m = det;
        if (det <= 0.f) ++c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        if (om < m) m = om;
        c += __shfl_xor(c, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) smin[wave] = m, scount[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            if (smin[w] < m) m = smin[w];
            c += scount[w];
        }
        slots[blockIdx.x] = DeformSlot{0.0, 0.0, c, m, 0};
    }
}

__global__ __launch_bounds__(64) void jacobian_stats_kernel(const DeformSlot* slots, int nslots, float* min_det, long long* count) {
    const int lane = threadIdx.x;
    float m = __uint_as_float(0x7f800000u);
    long long c = 0;
    for (int s = lane; s < nslots; s += 64) {
        if (slots[s].min_det < m) m = slots[s].min_det;
        c += slots[s].count;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        if (om < m) m = om;
        c += __shfl_xor(c, o, 64);
    }
    if (lane == 0) {
        *min_det = __fadd_rn(m, 0.f);      // -0.0 and +0.0 are one minimum
        *count = c;
    }
}

// ---------------------------------------------------------------- entry points

extern "C" size_t mrisr_f32_volume_deform_workspace_bytes(void) { return (size_t)kSlots * sizeof(DeformSlot); }

extern "C" int mrisr_f32_volume_warp(const float* moving, const float* u, int X, int Y, int Z, int method, float fill, float* out,
                                     void* stream) {
    if (!moving || !u || !out) MRISR_FAIL(MRISR_E_ARG, "f32_volume_warp: null pointer");
    if (method != kLinear && method != kCubic) MRISR_FAIL(MRISR_E_ARG, "f32_volume_warp: method %d (MRISR_RESAMPLE_LINEAR or _CUBIC)", method);
    BrickGrid g;
    if (const int rc = check_field_volume("f32_volume_warp", X, Y, Z, &g)) return rc;
    if (!aligned_to(moving, 4) || !aligned_to(u, 4) || !aligned_to(out, 4)) MRISR_FAIL(MRISR_E_ARG, "f32_volume_warp: misaligned pointer");
    if (out == moving || out == u) MRISR_FAIL(MRISR_E_ARG, "f32_volume_warp: out must be a buffer of its own");
    hipStream_t s = (hipStream_t)stream;
    if (method == kLinear) warp_kernel<kLinear><<<g.nbricks, 256, 0, s>>>(moving, u, X, Y, Z, fill, out, g.nby, g.nbz);
    else warp_kernel<kCubic><<<g.nbricks, 256, 0, s>>>(moving, u, X, Y, Z, fill, out, g.nby, g.nbz);
    MRISR_CHECK_LAUNCH("f32_volume_warp");
    return MRISR_OK;
}

// the force and the update-only force: one set of checks, one kernel
template <bool UPDATE>
static int launch_demons(const char* name, const float* fixed, const float* moving, const float* u, int X, int Y, int Z, float max_step,
                         float fill, float scale, float* v, void* workspace, void* stats_row, void* stream) {
    if (!fixed || !moving || !u || !v || !workspace) MRISR_FAIL(MRISR_E_ARG, "%s: null pointer", name);
    if (!(max_step >= 0.f) || !isfinite(max_step)) MRISR_FAIL(MRISR_E_ARG, "%s: max_step %g (finite, not negative)", name, (double)max_step);
    if (!(scale > 0.f) || !isfinite(scale)) MRISR_FAIL(MRISR_E_ARG, "%s: scale %g (finite, positive)", name, (double)scale);
    BrickGrid g;
    if (const int rc = check_field_volume(name, X, Y, Z, &g)) return rc;
    if (!aligned_to(fixed, 4) || !aligned_to(moving, 4) || !aligned_to(u, 4) || !aligned_to(v, 4) || !aligned_to(workspace, 8) ||
        !aligned_to(stats_row, 8))
        MRISR_FAIL(MRISR_E_ARG, "%s: misaligned pointer", name);
    if (v == u || v == fixed || v == moving) MRISR_FAIL(MRISR_E_ARG, "%s: %s must be a buffer of its own", name, UPDATE ? "w" : "v");
    hipStream_t s = (hipStream_t)stream;
    DeformSlot* slots = (DeformSlot*)workspace;
    demons_kernel<UPDATE><<<g.nslots, 256, 0, s>>>(fixed, moving, u, X, Y, Z, max_step, fill, scale, v, g.nbricks, g.nby, g.nbz, slots);
    MRISR_CHECK_LAUNCH(name);
    if (stats_row) {
        force_stats_kernel<<<1, 64, 0, s>>>(slots, g.nslots, (StatsRow*)stats_row);
        MRISR_CHECK_LAUNCH(name);
    }
    return MRISR_OK;
}

extern "C" int mrisr_f32_volume_demons_force(const float* fixed, const float* moving, const float* u, int X, int Y, int Z, float max_step,
                                             float fill, float* v, void* workspace, void* stats_row, void* stream) {
    return launch_demons<false>("f32_volume_demons_force", fixed, moving, u, X, Y, Z, max_step, fill, 1.f, v, workspace, stats_row, stream);
}

extern "C" int mrisr_f32_volume_demons_update(const float* fixed, const float* moving, const float* u, int X, int Y, int Z, float max_step,
                                              float fill, float scale, float* w, void* workspace, void* stats_row, void* stream) {
    return launch_demons<true>("f32_volume_demons_update", fixed, moving, u, X, Y, Z, max_step, fill, scale, w, workspace, stats_row, stream);
}

extern "C" int mrisr_f32_volume_field_compose(const float* u, const float* v, int X, int Y, int Z, float* out, void* stream) {
    if (!u || !v || !out) MRISR_FAIL(MRISR_E_ARG, "f32_volume_field_compose: null pointer");
    BrickGrid g;
    if (const int rc = check_field_volume("f32_volume_field_compose", X, Y, Z, &g)) return rc;
    if (!aligned_to(u, 4) || !aligned_to(v, 4) || !aligned_to(out, 4)) MRISR_FAIL(MRISR_E_ARG, "f32_volume_field_compose: misaligned pointer");
    if (out == u || out == v) MRISR_FAIL(MRISR_E_ARG, "f32_volume_field_compose: out must be a buffer of its own (u and v may be one)");
    compose_kernel<<<g.nbricks, 256, 0, (hipStream_t)stream>>>(u, v, X, Y, Z, out, g.nby, g.nbz);
    MRISR_CHECK_LAUNCH("f32_volume_field_compose");
    return MRISR_OK;
}

extern "C" int mrisr_f32_volume_warp_matrix(const float* moving, int SX, int SY, int SZ, const float* u, int X, int Y, int Z,
                                            const double* m12, int method, float fill, float* out, void* stream) {
    if (!moving || !u || !m12 || !out) MRISR_FAIL(MRISR_E_ARG, "f32_volume_warp_matrix: null pointer");
    if (method != kLinear && method != kCubic)
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_warp_matrix: method %d (MRISR_RESAMPLE_LINEAR or _CUBIC)", method);
    Matrix34 m;
    if (const int rc = check_matrix34("f32_volume_warp_matrix", m12, m.m)) return rc;
    BrickGrid source, g;
    if (const int rc = check_field_volume("f32_volume_warp_matrix (moving)", SX, SY, SZ, &source)) return rc;
    if (const int rc = check_field_volume("f32_volume_warp_matrix", X, Y, Z, &g)) return rc;
    if (!aligned_to(moving, 4) || !aligned_to(u, 4) || !aligned_to(out, 4)) MRISR_FAIL(MRISR_E_ARG, "f32_volume_warp_matrix: misaligned pointer");
    if (out == moving || out == u) MRISR_FAIL(MRISR_E_ARG, "f32_volume_warp_matrix: out must be a buffer of its own");
    hipStream_t s = (hipStream_t)stream;
    if (method == kLinear) warp_matrix_kernel<kLinear><<<g.nbricks, 256, 0, s>>>(moving, SX, SY, SZ, u, X, Y, Z, m, fill, out, g.nby, g.nbz);
    else warp_matrix_kernel<kCubic><<<g.nbricks, 256, 0, s>>>(moving, SX, SY, SZ, u, X, Y, Z, m, fill, out, g.nby, g.nbz);
    MRISR_CHECK_LAUNCH("f32_volume_warp_matrix");
    return MRISR_OK;
}

extern "C" int mrisr_f32_volume_field_smooth(const float* in, float* out, int X, int Y, int Z, int axis, const float* taps, int radius,
                                             const void* workspace, void* stats_row, void* stream) {
    if (!in || !out || !taps) MRISR_FAIL(MRISR_E_ARG, "f32_volume_field_smooth: null pointer");
    if (axis < 0 || axis > 2) MRISR_FAIL(MRISR_E_ARG, "f32_volume_field_smooth: axis %d (0, 1 or 2)", axis);
    if ((workspace == nullptr) != (stats_row == nullptr))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_field_smooth: workspace and stats_row go together (both or neither)");
    if (radius < 0 || radius > kMaxRadius) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_field_smooth: radius %d (0..%d)", radius, kMaxRadius);
    BrickGrid g;
    if (const int rc = check_field_volume("f32_volume_field_smooth", X, Y, Z, &g)) return rc;
    if (!aligned_to(in, 4) || !aligned_to(out, 4) || !aligned_to(taps, 4) || !aligned_to(workspace, 8) || !aligned_to(stats_row, 8))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_field_smooth: misaligned pointer");
    if (in == out) MRISR_FAIL(MRISR_E_ARG, "f32_volume_field_smooth: in and out must be two buffers");
    hipStream_t s = (hipStream_t)stream;
    const DeformSlot* slots = (const DeformSlot*)workspace;
    StatsRow* row = (StatsRow*)stats_row;
    static_assert(kZRows * 64 == 256 && kZTile % 64 == 0 && kSCols == 64 && kSGroups * 64 == 256, "a wave per row / per output group");
    if (axis == 2) {
        const long long rows = 3LL * X * Y;                     // at most 3 (2^31 - 1): its quarter is inside grid.x
        const dim3 grid((unsigned)((rows + kZRows - 1) / kZRows), (unsigned)ceil_div(Z, kZTile));
        smooth_z_kernel<<<grid, 256, 0, s>>>(in, out, rows, Z, taps, radius, slots, g.nslots, row);
    } else {
        const int A = axis == 1 ? 3 * X : 3, S = axis == 1 ? Y : X;
        const long long C = axis == 1 ? (long long)Z : (long long)Y * Z;
        const long long ncg = (C + kSCols - 1) / kSCols;        // A ncg <= 3 (2^31 - 1) / 64 + 3 X: inside grid.x
        const dim3 grid((unsigned)(ncg * A), (unsigned)ceil_div(S, kSGroups * kSPer));
        smooth_stream_kernel<<<grid, 256, 0, s>>>(in, out, S, C, (unsigned)ncg, taps, radius, slots, g.nslots, row);
    }
    MRISR_CHECK_LAUNCH("f32_volume_field_smooth");
    return MRISR_OK;
}

extern "C" int mrisr_f32_volume_jacobian_stats(const float* u, int X, int Y, int Z, float* min_det, long long* count, void* workspace,
                                               void* stream) {
    if (!u || !min_det || !count || !workspace) MRISR_FAIL(MRISR_E_ARG, "f32_volume_jacobian_stats: null pointer");
    BrickGrid g;
    if (const int rc = check_field_volume("f32_volume_jacobian_stats", X, Y, Z, &g)) return rc;
    if (!aligned_to(u, 4) || !aligned_to(min_det, 4) || !aligned_to(count, 8) || !aligned_to(workspace, 8))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_jacobian_stats: misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    DeformSlot* slots = (DeformSlot*)workspace;
    jacobian_kernel<<<g.nslots, 256, 0, s>>>(u, X, Y, Z, g.nbricks, g.nby, g.nbz, slots);
    MRISR_CHECK_LAUNCH("f32_volume_jacobian_stats");
    jacobian_stats_kernel<<<1, 64, 0, s>>>(slots, g.nslots, min_det, count);
    MRISR_CHECK_LAUNCH("f32_volume_jacobian_stats (finalise)");
    return MRISR_OK;
}
