// Slice-to-volume motion correction of the stack reconstruction on the device (gfx950; extension): the forward
// and the back projection of csrc/volume_stacks.hip with one matrix PER SLICE, and the cost of a dozen candidate poses for every
// slice of a stack in one launch.
//
// Restates stack_residual_slices_np / stack_update_slices_np / slice_cost_np of mri_superresolution_amd/volume_slices.py operation by
// operation (compiled with -ffp-contract=off); the first two are tested bit for bit, the float64 sums of the third are those of
// another order of addition and the same bits on every run.  The tables of matrices are DEVICE arrays of 12 doubles per slice (row
// major 3 x 4), written by the host before the launch; nothing is uploaded and nothing synchronises here (HIP-graph capturable).  A
// table entry that is not finite fails every inside test (a NaN compares false), so no kernel reads outside its arrays.
//
//   f32_volume_stack_residual_slices   stack_residual_kernel with the matrix of the voxel's slice fetched from the table: the same
//                                      stack_residual_voxel; the slots and the stats row are those of the plain kernel.
//   f32_volume_stack_update_slices     ONE launch for all stacks, one thread per OUTPUT voxel.  Per stack the workgroup stages the
//                                      slice-axis rows of its table (4 doubles per slice, at most 8 KB) in LDS; a thread walks the
//                                      slices in ascending order and computes the through-plane coordinate z alone (three products)
//                                      - d = |z - s| >= 1 rejects most slices; only then the two in-plane rows are read from the
//                                      table.  A slice that passes adds w = float32(1 - d) times the bilinear gather of ITS plane of
//                                      the residual (the higher in-plane axis reduced first) to acc and w to wk; the stack covers
//                                      the voxel when wk >= 0.5 and adds acc / wk.  Step, clamp, cover and the stats rows as in
//                                      stack_update_kernel.
//   f32_volume_slice_cost              one launch for the S x C (slice, candidate) pairs of a stack.  A workgroup owns slice
//                                      blockIdx / groups and every groups-th tile of 256 strided in-plane voxels of it.  A thread
//                                      reads y once, then, candidate by candidate, simulates its voxel through that candidate's matrix
//                                      (stack_simulate: the forward model of the residual kernel) and forms n, y, m, y^2, m^2, ym in
//                                      double (the products of two floats are exact).  The six values are added over the wave in
//                                      the fixed tree of wave_sum_d, lane 0 adds them to the wave's cell in LDS, the four waves are
//                                      added in order into the workgroup's slot, and a second launch adds the slots of a slice in
//                                      ascending order.  No atomics, no scratch; the order depends on the shapes alone.
#include "volume_stacks.h"

constexpr int kMaxSlices = MRISR_SLICES_MAX, kMaxCandidates = MRISR_SLICE_CANDIDATES_MAX;
constexpr int kCostGroups = 16;            // workgroups per slice of the cost launch at most
constexpr int kCostSums = 6;

struct SliceViews {
    const float* data[kMaxStacks];
    const double* table[kMaxStacks];       // (slices, 12): output index -> stack index, per slice
    int n[kMaxStacks][3];
    int axis[kMaxStacks];
    int nslots[kMaxStacks];
};

__device__ __forceinline__ void load_matrix(const double* __restrict__ m12, double (*g)[4]) {
#pragma unroll
    for (int e = 0; e < 12; ++e) g[e / 4][e % 4] = m12[e];
}

// at most kSlots workgroups walk the bricks of the STACK with a stride of the grid
__global__ __launch_bounds__(256) void stack_residual_slices_kernel(const float* __restrict__ x, int X, int Y, int Z,
                                                                    const float* __restrict__ y, int SX, int SY, int SZ,
                                                                    const double* __restrict__ table, int axis, StackProfile pr, int T,
                                                                    float* __restrict__ r, unsigned nbricks, unsigned nby, unsigned nbz,
                                                                    DeformSlot* __restrict__ slots) {
    __shared__ DeformSlot part[4];
    PairSum sq = {0.0, 0.0, 0};
    for (unsigned b = blockIdx.x; b < nbricks; b += gridDim.x) {
        int i, j, k;
        if (!brick_voxel(b, nby, nbz, SX, SY, SZ, i, j, k)) continue;
        const int slice = axis == 0 ? i : (axis == 1 ? j : k);
        double g[3][4];
        load_matrix(table + (size_t)slice * 12, g);
        stack_residual_voxel(x, X, Y, Z, y, g, axis, pr, T, i, j, k, ((size_t)i * SY + j) * SZ + k, r, sq);
    }
    block_sum_to_slot(sq, part, &slots[blockIdx.x]);
}

// one brick per workgroup; x is read once and out written once at the thread's own voxel, so out may be x
__global__ __launch_bounds__(256) void stack_update_slices_kernel(const float* x, float* out, unsigned char* __restrict__ cover, int X,
                                                                  int Y, int Z, SliceViews v, int K, float step, int use_clamp, float lo,
                                                                  unsigned nby, unsigned nbz, const DeformSlot* __restrict__ slots,
                                                                  StatsRow* __restrict__ rows) {
    __shared__ double zrow[kMaxSlices][4];
    stack_update_stats(slots, v.nslots, K, rows);
    int i, j, k;
    const bool valid = brick_voxel(blockIdx.x, nby, nbz, X, Y, Z, i, j, k);      // every thread stays for the barriers
    const double di = (double)i, dj = (double)j, dk = (double)k;
    float sum = 0.f;
    int cnt = 0;
#pragma unroll 1
    for (int s = 0; s < K; ++s) {
        const int axis = v.axis[s], S = v.n[s][axis];
        const double* __restrict__ table = v.table[s];
        __syncthreads();                                    // the rows of the stack before are read
        for (int e = threadIdx.x; e < S * 4; e += 256) zrow[e >> 2][e & 3] = table[(size_t)(e >> 2) * 12 + axis * 4 + (e & 3)];
        __syncthreads();
        if (!valid) continue;
        const int a = axis == 0 ? 1 : 0, b = axis == 2 ? 1 : 2;      // the in-plane axes, a < b
        const int ny = v.n[s][1], nz = v.n[s][2];
        const int na = v.n[s][a], nb = v.n[s][b];
        const size_t stride_s = axis == 0 ? (size_t)ny * nz : (axis == 1 ? (size_t)nz : 1);
        const size_t stride_a = a == 0 ? (size_t)ny * nz : (size_t)nz, stride_b = b == 2 ? 1 : (size_t)nz;
        float acc = 0.f, wk = 0.f;
#pragma unroll 1
        for (int sl = 0; sl < S; ++sl) {
            const double z = grid_coordinate(zrow[sl], di, dj, dk);
            const double d = fabs(__dsub_rn(z, (double)sl));
            if (!(d < 1.0)) continue;                       // a NaN is skipped too
            const double* m = table + (size_t)sl * 12;
            const double pa = grid_coordinate(m + a * 4, di, dj, dk), pb = grid_coordinate(m + b * 4, di, dj, dk);
            if (!(pa >= -0.5 && pa <= (double)na - 0.5 && pb >= -0.5 && pb <= (double)nb - 0.5)) continue;
            const float w = (float)__dsub_rn(1.0, d);
            int ia[2], ib[2];
            float wa[2], wb[2];
            axis_taps<kLinear>(pa, na, ia, wa);
            axis_taps<kLinear>(pb, nb, ib, wb);
            const float* plane = v.data[s] + (size_t)sl * stride_s;
            float ra[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float* row = plane + (size_t)ia[u] * stride_a;
                const float val[2] = {row[(size_t)ib[0] * stride_b], row[(size_t)ib[1] * stride_b]};
                ra[u] = weighted_sum<2>(wb, val);
            }
            acc = __fadd_rn(acc, __fmul_rn(w, weighted_sum<2>(wa, ra)));
            wk = __fadd_rn(wk, w);
        }
        if (wk >= 0.5f) {
            sum = __fadd_rn(sum, __fdiv_rn(acc, wk));
            ++cnt;
        }
    }
    if (!valid) return;
    const size_t idx = ((size_t)i * Y + j) * Z + k;
    stack_update_store(x[idx], cnt, step, use_clamp, lo, out, cover, idx, [&] { return __fdiv_rn(sum, (float)cnt); });
}

// workgroup blockIdx.x owns slice blockIdx.x / groups and the tiles blockIdx.x % groups, + groups, ... of its strided plane of
// npts = rows x cols voxels; slots: (slices, groups, C, 6)
__global__ __launch_bounds__(256) void slice_cost_kernel(const float* __restrict__ x, int X, int Y, int Z, const float* __restrict__ y,
                                                         int SY, int SZ, const double* __restrict__ cand, int axis, StackProfile pr, int T,
                                                         int C, int stride, unsigned cols, unsigned npts, unsigned ntiles, unsigned groups,
                                                         double* __restrict__ slots) {
    __shared__ double part[4][kMaxCandidates * kCostSums];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int per = C * kCostSums;
    for (int e = lane; e < per; e += 64) part[wave][e] = 0.0;
    __syncthreads();                                        // from here to the last barrier lane 0 alone touches its wave's cell
    const unsigned slice = blockIdx.x / groups;
    for (unsigned tile = blockIdx.x % groups; tile < ntiles; tile += groups) {
        const unsigned e = tile * 256u + threadIdx.x;
        const bool in = e < npts;
        const int qa = in ? (int)(e / cols) * stride : 0, qb = in ? (int)(e % cols) * stride : 0;
        const int i = axis == 0 ? (int)slice : qa, j = axis == 1 ? (int)slice : (axis == 0 ? qa : qb), k = axis == 2 ? (int)slice : qb;
        const float yv = in ? y[((size_t)i * SY + j) * SZ + k] : 0.f;
        const double di = (double)i, dj = (double)j, dk = (double)k;
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
            double g[3][4];
            load_matrix(cand + ((size_t)slice * C + c) * 12, g);
            float sim = 0.f;
            const bool ok = in && stack_simulate(x, X, Y, Z, g, axis, pr, T, di, dj, dk, sim);
            const double dy = ok ? (double)yv : 0.0, dm = ok ? (double)sim : 0.0;
            const double v6[kCostSums] = {ok ? 1.0 : 0.0, dy, dm, dy * dy, dm * dm, dy * dm};      // exact: 48 bits
#pragma unroll
            for (int u = 0; u < kCostSums; ++u) {
                const double t = wave_sum_d(v6[u]);
                if (lane == 0) part[wave][c * kCostSums + u] += t;
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < per; e += 256)
        slots[(size_t)blockIdx.x * per + e] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
}

// thread e = (slice, candidate, sum) adds the slots of its slice in ascending order
__global__ __launch_bounds__(256) void slice_cost_finish_kernel(const double* __restrict__ slots, int groups, int per, int total,
                                                                double* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int slice = e / per, rest = e % per;
    double t = slots[((size_t)slice * groups) * per + rest];
    for (int g = 1; g < groups; ++g) t += slots[((size_t)slice * groups + g) * per + rest];
    out[e] = t;
}

static int check_slices(const char* name, int slices, int extent) {
    if (slices < 1 || slices > kMaxSlices) MRISR_FAIL(MRISR_E_ARG, "%s: %d slices (1..%d)", name, slices, kMaxSlices);
    if (slices != extent) MRISR_FAIL(MRISR_E_ARG, "%s: a table of %d slices for a stack of %d along its slice axis", name, slices, extent);
    return MRISR_OK;
}

extern "C" int mrisr_f32_volume_stack_residual_slices(const float* x, int X, int Y, int Z, const float* y, int SX, int SY, int SZ,
                                                      const double* to_output, int slices, int slice_axis, const double* offsets,
                                                      const float* weights, int T, float* r, void* workspace, void* stats_row, void* stream) {
    const char* name = "f32_volume_stack_residual_slices";
    if (!x || !y || !to_output || !offsets || !weights || !r || !workspace) MRISR_FAIL(MRISR_E_ARG, "%s: null pointer", name);
    if (slice_axis < 0 || slice_axis > 2) MRISR_FAIL(MRISR_E_ARG, "%s: slice axis %d (0..2)", name, slice_axis);
    StackProfile pr;
    if (const int rc = check_profile(name, offsets, weights, T, &pr)) return rc;
    BrickGrid out_grid, grid;
    if (const int rc = check_field_volume(name, X, Y, Z, &out_grid)) return rc;
    if (const int rc = check_field_volume(name, SX, SY, SZ, &grid)) return rc;
    if (const int rc = check_slices(name, slices, slice_axis == 0 ? SX : (slice_axis == 1 ? SY : SZ))) return rc;
    if (!aligned_to(x, 4) || !aligned_to(y, 4) || !aligned_to(r, 4) || !aligned_to(to_output, 8) || !aligned_to(workspace, 8) ||
        !aligned_to(stats_row, 8))
        MRISR_FAIL(MRISR_E_ARG, "%s: misaligned pointer", name);
    if (r == x || r == y) MRISR_FAIL(MRISR_E_ARG, "%s: r must be a buffer of its own", name);
    hipStream_t st = (hipStream_t)stream;
    DeformSlot* slots = (DeformSlot*)workspace;
    stack_residual_slices_kernel<<<grid.nslots, 256, 0, st>>>(x, X, Y, Z, y, SX, SY, SZ, to_output, slice_axis, pr, T, r, grid.nbricks,
                                                               grid.nby, grid.nbz, slots);
    MRISR_CHECK_LAUNCH(name);
    if (stats_row) {
        force_stats_kernel<<<1, 64, 0, st>>>(slots, grid.nslots, (StatsRow*)stats_row);
        MRISR_CHECK_LAUNCH(name);
    }
    return MRISR_OK;
}

extern "C" int mrisr_f32_volume_stack_update_slices(const float* x, int X, int Y, int Z, const mrisr_stack_slices_view* views, int K,
                                                    float step, int use_clamp, float lo, float* out, unsigned char* cover,
                                                    const void* workspace, void* stats_rows, void* stream) {
    const char* name = "f32_volume_stack_update_slices";
    if (!x || !views || !out) MRISR_FAIL(MRISR_E_ARG, "%s: null pointer", name);
    if (const int rc = check_update_step(name, K, step, use_clamp, lo)) return rc;
    BrickGrid grid;
    if (const int rc = check_update_volume(name, x, X, Y, Z, out, workspace, stats_rows, &grid)) return rc;
    SliceViews v = {};
    for (int s = 0; s < K; ++s) {
        const mrisr_stack_slices_view& in = views[s];
        if (!in.data || !in.from_output) MRISR_FAIL(MRISR_E_ARG, "%s: stack %d: null pointer", name, s);
        if (!aligned_to(in.data, 4) || !aligned_to(in.from_output, 8)) MRISR_FAIL(MRISR_E_ARG, "%s: stack %d: misaligned pointer", name, s);
        if (in.data == out || (const void*)in.data == (const void*)cover)
            MRISR_FAIL(MRISR_E_ARG, "%s: stack %d: out and cover must be buffers of their own", name, s);
        if (in.slice_axis < 0 || in.slice_axis > 2) MRISR_FAIL(MRISR_E_ARG, "%s: stack %d: slice axis %d (0..2)", name, s, in.slice_axis);
        BrickGrid sg;
        if (const int rc = check_field_volume(name, in.nx, in.ny, in.nz, &sg)) return rc;
        if (const int rc = check_slices(name, in.slices, in.slice_axis == 0 ? in.nx : (in.slice_axis == 1 ? in.ny : in.nz))) return rc;
        v.data[s] = in.data;
        v.table[s] = in.from_output;
        v.n[s][0] = in.nx, v.n[s][1] = in.ny, v.n[s][2] = in.nz;
        v.axis[s] = in.slice_axis;
        v.nslots[s] = sg.nslots;
    }
    if ((const void*)cover == (const void*)x || (const void*)cover == (const void*)out)
        MRISR_FAIL(MRISR_E_ARG, "%s: cover must be a buffer of its own", name);
    stack_update_slices_kernel<<<grid.nbricks, 256, 0, (hipStream_t)stream>>>(x, out, cover, X, Y, Z, v, K, step, use_clamp, lo, grid.nby,
                                                                               grid.nbz, (const DeformSlot*)workspace, (StatsRow*)stats_rows);
    MRISR_CHECK_LAUNCH(name);
    return MRISR_OK;
}

static inline bool cost_shape_ok(int slices, int candidates) {
    return slices >= 1 && slices <= kMaxSlices && candidates >= 1 && candidates <= kMaxCandidates;
}

extern "C" size_t mrisr_f32_volume_slice_cost_workspace_bytes(int slices, int candidates) {
    return cost_shape_ok(slices, candidates) ? (size_t)slices * kCostGroups * candidates * kCostSums * sizeof(double) : 0;
}

extern "C" int mrisr_f32_volume_slice_cost(const float* x, int X, int Y, int Z, const float* y, int SX, int SY, int SZ,
                                           const double* candidates, int slices, int count, int slice_axis, const double* offsets,
                                           const float* weights, int T, int stride, void* workspace, double* out, void* stream) {
    const char* name = "f32_volume_slice_cost";
    if (!x || !y || !candidates || !offsets || !weights || !workspace || !out) MRISR_FAIL(MRISR_E_ARG, "%s: null pointer", name);
    if (slice_axis < 0 || slice_axis > 2) MRISR_FAIL(MRISR_E_ARG, "%s: slice axis %d (0..2)", name, slice_axis);
    if (count < 1 || count > kMaxCandidates) MRISR_FAIL(MRISR_E_ARG, "%s: %d candidates (1..%d)", name, count, kMaxCandidates);
    if (stride != 1 && stride != 2 && stride != 4) MRISR_FAIL(MRISR_E_ARG, "%s: stride %d (1, 2 or 4)", name, stride);
    StackProfile pr;
    if (const int rc = check_profile(name, offsets, weights, T, &pr)) return rc;
    BrickGrid out_grid, grid;
    if (const int rc = check_field_volume(name, X, Y, Z, &out_grid)) return rc;
    if (const int rc = check_field_volume(name, SX, SY, SZ, &grid)) return rc;
    if (const int rc = check_slices(name, slices, slice_axis == 0 ? SX : (slice_axis == 1 ? SY : SZ))) return rc;
    if (!aligned_to(x, 4) || !aligned_to(y, 4) || !aligned_to(candidates, 8) || !aligned_to(workspace, 8) || !aligned_to(out, 8))
        MRISR_FAIL(MRISR_E_ARG, "%s: misaligned pointer", name);
    const int na = slice_axis == 0 ? SY : SX, nb = slice_axis == 2 ? SY : SZ;      // the in-plane extents, lower axis first
    const unsigned rows = ceil_div(na, stride), cols = ceil_div(nb, stride);       // rows * cols <= 2^31 - 1 (check_field_volume)
    const unsigned npts = rows * cols, ntiles = (npts + 255u) / 256u;
    const unsigned groups = ntiles < (unsigned)kCostGroups ? ntiles : (unsigned)kCostGroups;
    hipStream_t st = (hipStream_t)stream;
    double* slots = (double*)workspace;
    slice_cost_kernel<<<(unsigned)slices * groups, 256, 0, st>>>(x, X, Y, Z, y, SY, SZ, candidates, slice_axis, pr, T, count, stride, cols,
                                                                  npts, ntiles, groups, slots);
    MRISR_CHECK_LAUNCH(name);
    const int per = count * kCostSums, total = slices * per;
    slice_cost_finish_kernel<<<ceil_div(total, 256), 256, 0, st>>>(slots, (int)groups, per, total, out);
    MRISR_CHECK_LAUNCH(name);
    return MRISR_OK;
}
