// Super-resolution reconstruction from orthogonal thick-slice stacks by iterative back-projection on the device (gfx950; extension,
// DESIGN.md section 7).
//
// Restates stack_residual_np / stack_update_np of mri_superresolution_amd/volume_stacks.py operation by operation and is tested bit
// for bit against them (compiled with -ffp-contract=off).  A volume is (X, Y, Z) in C order, Z fastest.  Both directions are gathers
// through the taps of volume_taps.h - the coordinate rule, the inside test, the clamp and the reduction of csrc/volume_reslice.hip:
//
//   f32_volume_stack_residual   one launch per stack, one thread per STACK voxel: the T samples of its slice profile lie on a line
//                               along the slice axis; each sample inside the estimate adds w_t times the linear gather of the
//                               estimate to acc and w_t to wsum (float32, t ascending); r = y - acc / wsum where wsum >= 0.5, else +0.
//                               The float64 sum of r^2 and the count of such voxels leave the launch as in
//                               mrisr_f32_volume_demons_force: a thread's (sum, rounding error) pair, the waves and the workgroup in
//                               a fixed order, one slot per workgroup (volume_bricks.h), added by one wave of a LATER launch.
//   f32_volume_stack_update     ONE launch for all stacks, one thread per OUTPUT voxel: for k ascending, the linear gather of r_k
//                               where the voxel lies inside stack k; x' = x + step * (sum / cnt) where cnt > 0, clamped from below
//                               there.  The views (pointer, extents, matrix) travel by value in the kernel arguments.  Its first
//                               wave adds the slots the K residual launches left: an iteration is K + 1 launches.
//   f32_volume_stack_update_reg the same update with the Huber prior of stack_update_np (reg_lambda > 0): the mean of the residuals
//                               plus lambda times the sum, over the covered face neighbours, of c_a times the difference to the
//                               neighbour clipped at +-delta.  Still ONE launch; the neighbours are read from the estimate before
//                               the update (Jacobi), so out is a buffer of its own.  A workgroup owns an 8 x 8 x 32 tile, a thread
//                               the 8 voxels along x at its (y, z); the tile of x with a halo of one (10 x 10 x 34: 1.66 staged
//                               elements per voxel, 16.6 KB with the flags) and, per staged voxel, whether it lies in the grid and
//                               a stack covers it, are staged in LDS once.  The gathers are those of the plain kernel.
//
// The brick walk, the coordinate, the gather, the forward model, the residual of a voxel, the parts of an update kernel (stats
// prologue, gather over the views, step-clamp-store epilogue) and the shared host checks are those of volume_stacks.h, shared with
// csrc/volume_slices.hip.
// The first two kernels walk the 2 x 2 x 64 bricks of the reslice and warp kernels, z fastest.  Nothing is uploaded and nothing
// synchronises (HIP-graph capturable); no floating-point atomics: the same bits on every run.
#include "volume_stacks.h"

struct StackMatrix {
    double m[3][4];
};

// at most kSlots workgroups walk the bricks of the STACK with a stride of the grid
__global__ __launch_bounds__(256) void stack_residual_kernel(const float* __restrict__ x, int X, int Y, int Z, const float* __restrict__ y,
                                                             int SX, int SY, int SZ, StackMatrix g, int axis, StackProfile pr, int T,
                                                             float* __restrict__ r, unsigned nbricks, unsigned nby, unsigned nbz,
                                                             DeformSlot* __restrict__ slots) {
    __shared__ DeformSlot part[4];
    PairSum sq = {0.0, 0.0, 0};
    for (unsigned b = blockIdx.x; b < nbricks; b += gridDim.x) {
        int i, j, k;
        if (!brick_voxel(b, nby, nbz, SX, SY, SZ, i, j, k)) continue;
        stack_residual_voxel(x, X, Y, Z, y, g.m, axis, pr, T, i, j, k, ((size_t)i * SY + j) * SZ + k, r, sq);
    }
    block_sum_to_slot(sq, part, &slots[blockIdx.x]);
}

// one brick per workgroup; x is read once and out written once at the thread's own voxel, so out may be x
__global__ __launch_bounds__(256) void stack_update_kernel(const float* x, float* out, unsigned char* __restrict__ cover, int X, int Y,
                                                           int Z, StackViews v, int K, float step, int use_clamp, float lo, unsigned nby,
                                                           unsigned nbz, const DeformSlot* __restrict__ slots, StatsRow* __restrict__ rows) {
    stack_update_stats(slots, v.nslots, K, rows);
    int i, j, k;
    if (!brick_voxel(blockIdx.x, nby, nbz, X, Y, Z, i, j, k)) return;
    const size_t idx = ((size_t)i * Y + j) * Z + k;
    float sum;
    const int cnt = stack_gather_views(v, K, (double)i, (double)j, (double)k, sum);
    stack_update_store(x[idx], cnt, step, use_clamp, lo, out, cover, idx, [&] { return __fdiv_rn(sum, (float)cnt); });
}

// the tile of the regularised update and its staged image (a halo of one on every side)
constexpr int kRX = 8, kRY = 8, kRZ = 32;
constexpr int kHX = kRX + 2, kHY = kRY + 2, kHZ = kRZ + 2, kHalo = kHX * kHY * kHZ;

struct StackPrior {
    float lambda, delta, c[3];
};

// one tile per workgroup (tiles numbered along z, then y, then x); thread t owns the voxels (0..7, t / 32, t % 32) of the tile
__global__ __launch_bounds__(256) void stack_update_reg_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                               const unsigned char* __restrict__ cover_in, unsigned char* __restrict__ cover,
                                                               int X, int Y, int Z, StackViews v, int K, float step, int use_clamp, float lo,
                                                               StackPrior pr, unsigned nty, unsigned ntz, const DeformSlot* __restrict__ slots,
                                                               StatsRow* __restrict__ rows) {
    __shared__ float sx[kHalo];
    __shared__ unsigned char sok[kHalo];                    // 1: inside the grid and covered by a stack
    stack_update_stats(slots, v.nslots, K, rows);
    const unsigned tz = blockIdx.x % ntz, rest = blockIdx.x / ntz, ty = rest % nty, tx = rest / nty;
    const int x0 = (int)tx * kRX, y0 = (int)ty * kRY, z0 = (int)tz * kRZ;
    for (int e = threadIdx.x; e < kHalo; e += 256) {
        const int hz = e % kHZ, hy = e / kHZ % kHY, hx = e / (kHZ * kHY);
        const int i = x0 + hx - 1, j = y0 + hy - 1, k = z0 + hz - 1;
        // only face neighbours are read: the edges and corners of the halo are not fetched
        const int faces = (hx == 0 || hx == kHX - 1) + (hy == 0 || hy == kHY - 1) + (hz == 0 || hz == kHZ - 1);
        float val = 0.f;
        unsigned char ok = 0;
        if (faces <= 1 && i >= 0 && i < X && j >= 0 && j < Y && k >= 0 && k < Z) {
            const size_t idx = ((size_t)i * Y + j) * Z + k;
            val = x[idx];
            ok = cover_in[idx] != 0;
        }
        sx[e] = val;
        sok[e] = ok;
    }
    __syncthreads();
    const int lz = threadIdx.x % kRZ, ly = threadIdx.x / kRZ;
    const int j = y0 + ly, k = z0 + lz;
    if (j >= Y || k >= Z) return;
    const double dj = (double)j, dk = (double)k;
    constexpr int kStride[3] = {kHY * kHZ, kHZ, 1};
#pragma unroll 1
    for (int lx = 0; lx < kRX && x0 + lx < X; ++lx) {
        const int i = x0 + lx;
        const size_t idx = ((size_t)i * Y + j) * Z + k;
        float sum;
        const int cnt = stack_gather_views(v, K, (double)i, dj, dk, sum);
        const int h = ((lx + 1) * kHY + ly + 1) * kHZ + lz + 1;
        const float xv = sx[h];
        stack_update_store(xv, cnt, step, use_clamp, lo, out, cover, idx, [&] {
            float reg = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int side = -1; side <= 1; side += 2) {
                    const int n = h + side * kStride[a];
                    if (!sok[n]) continue;
                    const float d = __fsub_rn(sx[n], xv);
                    const float psi = d > pr.delta ? pr.delta : (d < -pr.delta ? -pr.delta : d);      // a NaN stays
                    reg = __fadd_rn(reg, __fmul_rn(pr.c[a], psi));
                }
            }
            return __fadd_rn(__fdiv_rn(sum, (float)cnt), __fmul_rn(pr.lambda, reg));
        });
    }
}

extern "C" size_t mrisr_f32_volume_stack_workspace_bytes(int K) {
    return K >= 1 && K <= kMaxStacks ? (size_t)K * kSlots * sizeof(DeformSlot) : 0;
}

extern "C" int mrisr_f32_volume_stack_residual(const float* x, int X, int Y, int Z, const float* y, int SX, int SY, int SZ, const double* m12,
                                               int slice_axis, const double* offsets, const float* weights, int T, float* r, void* workspace,
                                               void* stats_row, void* stream) {
    const char* name = "f32_volume_stack_residual";
    if (!x || !y || !m12 || !offsets || !weights || !r || !workspace) MRISR_FAIL(MRISR_E_ARG, "%s: null pointer", name);
    if (T < 1 || T > kMaxSamples) MRISR_FAIL(MRISR_E_ARG, "%s: %d profile samples (1..%d)", name, T, kMaxSamples);      // before the axis and matrix checks, as before; check_profile repeats it
    if (slice_axis < 0 || slice_axis > 2) MRISR_FAIL(MRISR_E_ARG, "%s: slice axis %d (0..2)", name, slice_axis);
    StackMatrix g;
    if (const int rc = check_matrix34(name, m12, g.m)) return rc;
    StackProfile pr;
    if (const int rc = check_profile(name, offsets, weights, T, &pr)) return rc;
    BrickGrid out_grid, grid;
    if (const int rc = check_field_volume(name, X, Y, Z, &out_grid)) return rc;
    if (const int rc = check_field_volume(name, SX, SY, SZ, &grid)) return rc;
    if (!aligned_to(x, 4) || !aligned_to(y, 4) || !aligned_to(r, 4) || !aligned_to(workspace, 8) || !aligned_to(stats_row, 8))
        MRISR_FAIL(MRISR_E_ARG, "%s: misaligned pointer", name);
    if (r == x || r == y) MRISR_FAIL(MRISR_E_ARG, "%s: r must be a buffer of its own", name);
    hipStream_t st = (hipStream_t)stream;
    DeformSlot* slots = (DeformSlot*)workspace;
    stack_residual_kernel<<<grid.nslots, 256, 0, st>>>(x, X, Y, Z, y, SX, SY, SZ, g, slice_axis, pr, T, r, grid.nbricks, grid.nby, grid.nbz,
                                                        slots);
    MRISR_CHECK_LAUNCH(name);
    if (stats_row) {
        force_stats_kernel<<<1, 64, 0, st>>>(slots, grid.nslots, (StatsRow*)stats_row);
        MRISR_CHECK_LAUNCH(name);
    }
    return MRISR_OK;
}

// the views of an update entry into the kernel argument: every stack's pointer (not null, aligned, neither out nor cover), matrix
// and extents
static int fill_stack_views(const char* name, const mrisr_stack_view* views, int K, const float* out, const unsigned char* cover,
                            StackViews* v) {
    *v = StackViews{};
    for (int s = 0; s < K; ++s) {
        const mrisr_stack_view& in = views[s];
        if (!in.data) MRISR_FAIL(MRISR_E_ARG, "%s: stack %d: null pointer", name, s);
        if (!aligned_to(in.data, 4)) MRISR_FAIL(MRISR_E_ARG, "%s: stack %d: misaligned pointer", name, s);
        if (in.data == out || (const void*)in.data == (const void*)cover)
            MRISR_FAIL(MRISR_E_ARG, "%s: stack %d: out and cover must be buffers of their own", name, s);
        if (const int rc = check_matrix34(name, in.m, v->m[s])) return rc;
        BrickGrid sg;
        if (const int rc = check_field_volume(name, in.nx, in.ny, in.nz, &sg)) return rc;
        v->data[s] = in.data;
        v->n[s][0] = in.nx, v->n[s][1] = in.ny, v->n[s][2] = in.nz;
        v->nslots[s] = sg.nslots;
    }
    return MRISR_OK;
}

extern "C" int mrisr_f32_volume_stack_update(const float* x, int X, int Y, int Z, const mrisr_stack_view* views, int K, float step,
                                             int use_clamp, float lo, float* out, unsigned char* cover, const void* workspace,
                                             void* stats_rows, void* stream) {
    const char* name = "f32_volume_stack_update";
    if (!x || !views || !out) MRISR_FAIL(MRISR_E_ARG, "%s: null pointer", name);
    if (const int rc = check_update_step(name, K, step, use_clamp, lo)) return rc;
    BrickGrid grid;
    if (const int rc = check_update_volume(name, x, X, Y, Z, out, workspace, stats_rows, &grid)) return rc;
    StackViews v;
    if (const int rc = fill_stack_views(name, views, K, out, cover, &v)) return rc;
    if ((const void*)cover == (const void*)x || (const void*)cover == (const void*)out)
        MRISR_FAIL(MRISR_E_ARG, "%s: cover must be a buffer of its own", name);
    stack_update_kernel<<<grid.nbricks, 256, 0, (hipStream_t)stream>>>(x, out, cover, X, Y, Z, v, K, step, use_clamp, lo, grid.nby, grid.nbz,
                                                                        (const DeformSlot*)workspace, (StatsRow*)stats_rows);
    MRISR_CHECK_LAUNCH(name);
    return MRISR_OK;
}

extern "C" int mrisr_f32_volume_stack_update_reg(const float* x, int X, int Y, int Z, const mrisr_stack_view* views, int K, float step,
                                                 int use_clamp, float lo, float lambda, float delta, const float* coeffs,
                                                 const unsigned char* cover_in, float* out, unsigned char* cover, const void* workspace,
                                                 void* stats_rows, void* stream) {
    const char* name = "f32_volume_stack_update_reg";
    if (!x || !views || !out || !coeffs || !cover_in) MRISR_FAIL(MRISR_E_ARG, "%s: null pointer", name);
    if (const int rc = check_update_step(name, K, step, use_clamp, lo)) return rc;
    if (!isfinite(lambda) || lambda < 0.f) MRISR_FAIL(MRISR_E_ARG, "%s: lambda %g (finite, not negative)", name, (double)lambda);
    if (!(delta > 0.f)) MRISR_FAIL(MRISR_E_ARG, "%s: delta %g (positive, may be infinite)", name, (double)delta);
    StackPrior pr = {lambda, delta, {coeffs[0], coeffs[1], coeffs[2]}};
    for (int a = 0; a < 3; ++a)
        if (!isfinite(pr.c[a]) || !(pr.c[a] > 0.f)) MRISR_FAIL(MRISR_E_ARG, "%s: coefficient %d is %g (finite, positive)", name, a, (double)pr.c[a]);
    const double bound = (double)step * (double)lambda * (((double)pr.c[0] + (double)pr.c[1]) + (double)pr.c[2]);
    if (!(bound <= 0.5))
        MRISR_FAIL(MRISR_E_ARG, "%s: step * lambda * (c_0 + c_1 + c_2) = %g breaks the stability bound <= 0.5", name, bound);
    BrickGrid grid;
    if (const int rc = check_update_volume(name, x, X, Y, Z, out, workspace, stats_rows, &grid)) return rc;
    if (out == x) MRISR_FAIL(MRISR_E_ARG, "%s: out must differ from x (the neighbours are read before the update)", name);
    StackViews v;
    if (const int rc = fill_stack_views(name, views, K, out, cover, &v)) return rc;
    if ((const void*)cover_in == (const void*)x || (const void*)cover_in == (const void*)out)
        MRISR_FAIL(MRISR_E_ARG, "%s: cover_in must be a buffer of its own", name);
    if (cover && ((const void*)cover == (const void*)x || (const void*)cover == (const void*)out || cover == cover_in))
        MRISR_FAIL(MRISR_E_ARG, "%s: cover must be a buffer of its own", name);
    // at most ceil(2^31 / 2048) tiles plus the remainder tiles of every row: far inside unsigned
    const unsigned ntx = ceil_div(X, kRX), nty = ceil_div(Y, kRY), ntz = ceil_div(Z, kRZ);
    stack_update_reg_kernel<<<ntx * nty * ntz, 256, 0, (hipStream_t)stream>>>(x, out, cover_in, cover, X, Y, Z, v, K, step, use_clamp, lo, pr, nty,
                                                                              ntz, (const DeformSlot*)workspace, (StatsRow*)stats_rows);
    MRISR_CHECK_LAUNCH(name);
    return MRISR_OK;
}
