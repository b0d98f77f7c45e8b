// Reslicing of whole volumes between voxel grids through an affine on the device (gfx950; extension).
//
// Restates reslice_np / reslice_mask_np of mri_superresolution_amd/volume_reslice.py operation by operation and is tested bit for
// bit against them (compiled with -ffp-contract=off).  A volume is (X, Y, Z) in C order, Z fastest.  m is the row-major 3 x 4
// double matrix that maps a destination voxel index (i, j, k) to a continuous source voxel index:
//
//   coordinate   p_a = ((m[a][0] i + m[a][1] j) + m[a][2] k) + m[a][3] in double, one rounded operation at a time, evaluated
//                directly from the indices of the voxel (never stepped from a neighbour's value)
//   inside       -0.5 <= p_a <= n_a - 0.5 on all three axes, in double, before anything is converted to an integer; every other
//                voxel is `fill`
//   NEAREST      source index clip(floor(p_a + 0.5), 0, n_a - 1)
//   LINEAR       f_a = floor(p_a), t_a = (float)(p_a - f_a); weights (1 - t_a, t_a) on the taps f_a, f_a + 1, clamped (border
//                replicated)
//   CUBIC        taps f_a - 1 .. f_a + 2, clamped; Keys weights with A = -0.75 in float32 at the distances 1 + t, t, 1 - t, 2 - t:
//                x <= 1: ((1.25 x - 2.25) x) x + 1, else ((-0.75 x + 3.75) x - 6) x + 3; not renormalised
//   reduction    along z, then y, then x; each stage ((w0 v0 + w1 v1) + w2 v2) + w3 v3 in float32, every product and sum rounded
//
// A gather: one thread per destination voxel.  A workgroup of 256 threads owns a compact kBX x kBY x kBZ brick of the destination,
// z fastest (a wave stores runs of min(kBZ, 64) floats), so that under any rotation its source footprint is a small box - the 64 taps
// of CUBIC are served by the vector cache and L2, not by HBM.  The bricks are numbered along z, then y, then x in a 1-D grid.  The
// matrix travels by value in the kernel arguments: nothing is uploaded, nothing synchronises (HIP-graph capturable).
// The clamp, the Keys weights, the taps of an axis and the tap sum live in volume_taps.h (shared with volume_register.hip).
#include "volume_taps.h"

// the brick (x, y, z): 256 voxels, one wave per 64-voxel run along z.  2 x 2 x 64 measured against 1 x 4 x 64, 2 x 4 x 32,
// 4 x 4 x 16 and 8 x 8 x 4 (profiles/NOTES.md, "Reslice"); tools/reslice_bench.py --variant_libs times builds with other values
#ifndef MRISR_RESLICE_BX
#define MRISR_RESLICE_BX 2
#define MRISR_RESLICE_BY 2
#define MRISR_RESLICE_BZ 64
#endif
constexpr int kBX = MRISR_RESLICE_BX, kBY = MRISR_RESLICE_BY, kBZ = MRISR_RESLICE_BZ;
static_assert(kBX * kBY * kBZ == 256, "a brick is one workgroup of 256 threads");
constexpr long long kMaxVoxels = 2147483647LL;      // 2^31 - 1 on either side

struct GridMatrix {
    double m[3][4];
};

template <int METHOD, typename T>
__global__ __launch_bounds__(256) void volume_reslice_kernel(const T* __restrict__ src, int SX, int SY, int SZ, T* __restrict__ dst,
                                                             int DX, int DY, int DZ, GridMatrix g, T fill, unsigned nby, unsigned nbz) {
    const unsigned bz = blockIdx.x % nbz, rest = blockIdx.x / nbz, by = rest % nby, bx = rest / nby;
    const int tid = threadIdx.x;
    const int k = (int)bz * kBZ + tid % kBZ, j = (int)by * kBY + tid / kBZ % kBY, i = (int)bx * kBX + tid / (kBZ * kBY);
    if (i >= DX || j >= DY || k >= DZ) return;
    const double di = (double)i, dj = (double)j, dk = (double)k;
    const int n[3] = {SX, SY, SZ};
    double p[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(g.m[a][0], di), __dmul_rn(g.m[a][1], dj)), __dmul_rn(g.m[a][2], dk)), g.m[a][3]);
        inside = inside && p[a] >= -0.5 && p[a] <= (double)n[a] - 0.5;
    }
    T* o = dst + ((size_t)i * DY + j) * DZ + k;
    if (!inside) {
        *o = fill;
        return;
    }
    if constexpr (METHOD == kNearest) {
        int q[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = clampi((int)floor(__dadd_rn(p[a], 0.5)), n[a]);
        *o = src[((size_t)q[0] * SY + q[1]) * SZ + q[2]];
    } else {
        constexpr int N = METHOD == kLinear ? 2 : 4;
        int ix[N], iy[N], iz[N];
        float wx[N], wy[N], wz[N];
        axis_taps<METHOD>(p[0], SX, ix, wx);
        axis_taps<METHOD>(p[1], SY, iy, wy);
        axis_taps<METHOD>(p[2], SZ, iz, wz);
        float rx[N];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            float ry[N];
#pragma unroll
            for (int b = 0; b < N; ++b) {
                const T* row = src + ((size_t)ix[a] * SY + iy[b]) * SZ;
                float v[N];
#pragma unroll
                for (int c = 0; c < N; ++c) v[c] = row[iz[c]];
                ry[b] = weighted_sum<N>(wz, v);
            }
            rx[a] = weighted_sum<N>(wy, ry);
        }
        *o = weighted_sum<N>(wx, rx);
    }
}

// the checks shared by both entries; nothing is launched unless this returns MRISR_OK
static int check_reslice(const char* name, const void* src, int SX, int SY, int SZ, const void* dst, int DX, int DY, int DZ,
                         const double* m12, GridMatrix* g) {
    if (!src || !dst || !m12) MRISR_FAIL(MRISR_E_ARG, "%s: null pointer", name);
    if (const int rc = check_matrix34(name, m12, g->m)) return rc;
    if (SX < 1 || SY < 1 || SZ < 1 || DX < 1 || DY < 1 || DZ < 1)
        MRISR_FAIL(MRISR_E_SHAPE, "%s: %d x %d x %d -> %d x %d x %d (every extent at least 1)", name, SX, SY, SZ, DX, DY, DZ);
    const long long sxy = (long long)SX * SY, dxy = (long long)DX * DY;
    if (sxy > kMaxVoxels || sxy * SZ > kMaxVoxels || dxy > kMaxVoxels || dxy * DZ > kMaxVoxels)
        MRISR_FAIL(MRISR_E_UNSUPPORTED, "%s: %d x %d x %d -> %d x %d x %d: more than 2^31 - 1 voxels on one side", name, SX, SY, SZ, DX,
                   DY, DZ);
    return MRISR_OK;
}

template <int METHOD, typename T>
static void launch_reslice(const T* src, int SX, int SY, int SZ, T* dst, int DX, int DY, int DZ, const GridMatrix& g, T fill,
                           hipStream_t st) {
    // at most ceil(2^31 / 256) + a remainder brick per row: far inside the 2^31 - 1 blocks of grid.x
    const unsigned nbx = ceil_div(DX, kBX), nby = ceil_div(DY, kBY), nbz = ceil_div(DZ, kBZ);
    volume_reslice_kernel<METHOD, T><<<dim3(nbx * nby * nbz), dim3(256), 0, st>>>(src, SX, SY, SZ, dst, DX, DY, DZ, g, fill, nby, nbz);
}

extern "C" int mrisr_f32_volume_reslice(const float* src, int SX, int SY, int SZ, float* dst, int DX, int DY, int DZ, const double* m12,
                                        int method, float fill, void* stream) {
    GridMatrix g;
    const int rc = check_reslice("f32_volume_reslice", src, SX, SY, SZ, dst, DX, DY, DZ, m12, &g);
    if (rc != MRISR_OK) return rc;
    if (method != kNearest && method != kLinear && method != kCubic)
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_reslice: method %d (MRISR_RESAMPLE_NEAREST, _LINEAR or _CUBIC)", method);
    hipStream_t st = (hipStream_t)stream;
    if (method == kNearest) launch_reslice<kNearest, float>(src, SX, SY, SZ, dst, DX, DY, DZ, g, fill, st);
    else if (method == kLinear) launch_reslice<kLinear, float>(src, SX, SY, SZ, dst, DX, DY, DZ, g, fill, st);
    else launch_reslice<kCubic, float>(src, SX, SY, SZ, dst, DX, DY, DZ, g, fill, st);
    MRISR_CHECK_LAUNCH("f32_volume_reslice");
    return MRISR_OK;
}

extern "C" int mrisr_u8_volume_reslice_nearest(const uint8_t* src, int SX, int SY, int SZ, uint8_t* dst, int DX, int DY, int DZ,
                                               const double* m12, uint8_t fill, void* stream) {
    GridMatrix g;
    const int rc = check_reslice("u8_volume_reslice_nearest", src, SX, SY, SZ, dst, DX, DY, DZ, m12, &g);
    if (rc != MRISR_OK) return rc;
    launch_reslice<kNearest, uint8_t>(src, SX, SY, SZ, dst, DX, DY, DZ, g, fill, (hipStream_t)stream);
    MRISR_CHECK_LAUNCH("u8_volume_reslice_nearest");
    return MRISR_OK;
}
