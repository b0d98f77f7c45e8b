// What the kernels that walk a volume in bricks share, one definition each (csrc/volume_deform.hip,
// csrc/volume_lcc.hip and, through volume_stacks.h, csrc/volume_stacks.hip and csrc/volume_slices.hip): the voxel of a thread in a
// brick, the brick grid of a volume with its host check, and the fixed slots of the float64 sums (a thread's pair, the wave's and
// the workgroup's order, the wave of a later launch that adds the slots).
#pragma once
#include "volume_common.h"

constexpr int kBX = 2, kBY = 2, kBZ = 64;              // the brick of the field and stack kernels: that of volume_reslice.hip
constexpr int kSlots = 2048;                           // workgroups of the force and the Jacobian kernels: 8 per CU
constexpr long long kMaxVoxels = 2147483647LL;         // 2^31 - 1

// voxel of thread tid in brick b (bricks numbered along z, then y, then x)
__device__ __forceinline__ bool brick_voxel(unsigned b, unsigned nby, unsigned nbz, int X, int Y, int Z, int& i, int& j, int& k) {
    const unsigned bz = b % nbz, rest = b / nbz, by = rest % nby, bx = rest / nby;
    const int tid = threadIdx.x;
    k = (int)bz * kBZ + tid % kBZ, j = (int)by * kBY + tid / kBZ % kBY, i = (int)bx * kBX + tid / (kBZ * kBY);
    return i < X && j < Y && k < Z;
}

struct DeformSlot {
    double hi, lo;
    long long count;
    float min_det;
    int pad_;
};
struct StatsRow {
    double sum;
    long long count;
};

// s = fl(a + b) and its rounding error e: a + b = s + e exactly (Knuth)
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
struct PairSum {
    double hi, lo;
    long long count;
    __device__ __forceinline__ void add(double ohi, double olo, long long ocount) {
        double s, e;
        two_sum(hi, ohi, s, e);
        lo = (lo + olo) + e;
        hi = s;
        count += ocount;
    }
    __device__ __forceinline__ void wave_reduce() {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) add(__shfl_xor(hi, o, 64), __shfl_xor(lo, o, 64), __shfl_xor(count, o, 64));
    }
};

// the pairs of a workgroup of 4 waves into its slot: the lanes of a wave, then the waves in order (part: 4 slots of LDS)
__device__ __forceinline__ void block_sum_to_slot(PairSum acc, DeformSlot* part, DeformSlot* slot) {
    acc.wave_reduce();
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) part[wave] = DeformSlot{acc.hi, acc.lo, acc.count, 0.f, 0};
    __syncthreads();
    if (threadIdx.x == 0) {
        PairSum t = {part[0].hi, part[0].lo, part[0].count};
        for (int w = 1; w < 4; ++w) t.add(part[w].hi, part[w].lo, part[w].count);
        *slot = DeformSlot{t.hi, t.lo, t.count, 0.f, 0};
    }
}

// one wave: lane l adds the slots l, l + 64, ... in that order, then the lanes are added as in the kernels
__device__ __forceinline__ void finalize_force(const DeformSlot* slots, int nslots, StatsRow* row) {
    const int lane = threadIdx.x & 63;
    PairSum t = {0.0, 0.0, 0};
    for (int s = lane; s < nslots; s += 64) t.add(slots[s].hi, slots[s].lo, slots[s].count);
    t.wave_reduce();
    if (lane == 0) {
        row->sum = t.hi + t.lo;
        row->count = t.count;
    }
}

static __global__ __launch_bounds__(64) void force_stats_kernel(const DeformSlot* slots, int nslots, StatsRow* row) {
    finalize_force(slots, nslots, row);
}

struct BrickGrid {
    unsigned nby, nbz, nbricks;
    int nslots;
};

// the checks shared by the entries that walk bricks; nothing is launched unless this returns MRISR_OK
static inline int check_field_volume(const char* name, int X, int Y, int Z, BrickGrid* g) {
    if (X < 1 || Y < 1 || Z < 1) MRISR_FAIL(MRISR_E_SHAPE, "%s: volume %d x %d x %d (every extent at least 1)", name, X, Y, Z);
    const long long xy = (long long)X * Y;
    if (xy > kMaxVoxels || xy * Z > kMaxVoxels) MRISR_FAIL(MRISR_E_SHAPE, "%s: %d x %d x %d: more than 2^31 - 1 voxels", name, X, Y, Z);
    // at most ceil(2^31 / 256) bricks plus the remainder bricks of every row: far inside unsigned
    const unsigned nbx = ceil_div(X, kBX);
    g->nby = ceil_div(Y, kBY), g->nbz = ceil_div(Z, kBZ);
    g->nbricks = nbx * g->nby * g->nbz;
    g->nslots = g->nbricks < (unsigned)kSlots ? (int)g->nbricks : kSlots;
    return MRISR_OK;
}
