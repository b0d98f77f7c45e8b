// Demons across contrasts (gfx950; extension): the locally normalised correlation force.  The specification
// is volume_deform.lcc_force_np / lcc_update_np; the kernel here is bit-equal to it.  Compiled with -ffp-contract=off (build.py):
// every product, sum, difference and division is rounded on its own, never an fma.
//
// Every voxel regresses warped on fixed over the cube of radius R around it (clipped to the grid, invalid voxels left out) and
// only what that local affine relation cannot explain drives the field:
//     n, sF, sM, sFF, sMM, sFM      window sums of 1, F, M, F F, M M, F M in float64 (the products of two floats are exact),
//                                   separable: along axis 2, then 1, then 0, each over ascending index into a sum that starts at +0.0
//     mF = sF / n, mM = sM / n, A = sFM - mM sF, B = sFF - mF sF, C = sMM - mM sM
//     d = (M - mM) (B / A) - (F - mF),  w = min(A A / (B C), 1)
// then Thirion's rule of the demons force in float32 with the step scaled by w.  An invalid voxel (fixed or warped not finite -
// the warp is run with a NaN fill, so outside the moving volume is invalid) has all channels +0.0; adding +0.0 to a sum that
// started at +0.0 changes nothing, so "clipped" and "padded with zeros" are the same bits.
//
//   f32_volume_lcc_force   ONE launch after the warp.  A workgroup of 256 threads owns a footprint of 8 x 32 voxels (axes 1, 2),
//                          a thread per column, and marches along axis 0 through a chunk of 32 planes.  Per input plane it
//                            a. stages the five float64 channels and the validity of the footprint plus its halo in LDS
//                               ((8 + 2R) x (32 + 2R) elements: fixed and warped are read once per plane and workgroup),
//                            b. forms the axis-2 sums of the 8 + 2R rows from LDS into LDS,
//                            c. forms the axis-1 sums of its own column from those, into a ring of 2R + 1 planes in registers,
//                          and once the ring is full
//                            d. adds the ring in order (axis 0), runs the regression and the epilogue for plane i - R: the
//                               6-neighbour gradient of fixed, a coalesced read of u and a coalesced write of three components.
//                          The count n is an integer sum (exact either way).  Float64 adds only, no atomics: a thread adds
//                          float64(w) of its ok voxels as a pair (volume_bricks.h), the workgroup leaves its slot, the smoothing
//                          pass that follows (or a launch of one wave) adds the slots - the same bits on every run.
//
// LDS per workgroup: 40 (8 + 2R)(32 + 2R) + 40 (8 + 2R) 32 bytes of channels and sums plus 4 bytes per element of counts:
//   R = 2: 17.3 + 15.4 + 3.3 = 36 KB  -> 4 workgroups per CU of the 160 KB;   R = 4: 25.6 + 20.5 + 4.6 = 51 KB -> 3 per CU.
// A half-wave reads 32 consecutive doubles of one row in steps b and c: 256 B, one bank row, no conflict with 8-byte elements.
// Work per voxel at R = 2: (1.5 + 1 + 1) x 5 x 5 = 88 float64 adds (gfx950's vector FP64 rate is half its FP32 rate), far below the
// time of the 8 floats per voxel the launch moves; the halo costs (8 + 2R)(32 + 2R) / 256 = 1.7 reads per voxel from L2.
#include "volume_deform.h"

constexpr int kLccMaxRadius = 4;
constexpr int kLX = 32, kLY = 8, kLZ = 32;      // chunk of planes along axis 0; footprint of a workgroup on axes 1 and 2
static_assert(kLY * kLZ == 256, "a thread per column of the footprint");

template <int R>
__global__ __launch_bounds__(256) void lcc_kernel(const float* __restrict__ fixed, const float* __restrict__ warped,
                                                  const float* __restrict__ u, int X, int Y, int Z, float max_step, float scale,
                                                  int update, float* __restrict__ v, unsigned ntiles, unsigned nty, unsigned ntz,
                                                  int nslots, DeformSlot* __restrict__ slots) {
    constexpr int W = 2 * R + 1, HY = kLY + 2 * R, HZ = kLZ + 2 * R;
    __shared__ double ch[5][HY][HZ];          // F, M, F F, M M, F M of the plane; +0.0 where invalid or off the grid
    __shared__ int chn[HY][HZ];               // 1 where valid
    __shared__ double rs[5][HY][kLZ];         // axis-2 sums
    __shared__ int rsn[HY][kLZ];
    __shared__ DeformSlot part[4];
    const int t = threadIdx.x, tj = t / kLZ, tk = t % kLZ;
    const size_t n = (size_t)X * Y * Z;
    PairSum acc = {0.0, 0.0, 0};
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned tz = tile % ntz, rest = tile / ntz, ty = rest % nty, tx = rest / nty;
        const int i0 = (int)tx * kLX, j0 = (int)ty * kLY, k0 = (int)tz * kLZ;
        const int i1 = i0 + kLX < X ? i0 + kLX : X;
        const int j = j0 + tj, k = k0 + tk;
        double ring[W][5];                    // axis-1 sums of this column on planes ip - 2R .. ip
        int ringn[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            ringn[w] = 0;
#pragma unroll
            for (int c = 0; c < 5; ++c) ring[w][c] = 0.0;
        }
        for (int ip = i0 - R; ip < i1 + R; ++ip) {
#pragma unroll
            for (int w = 0; w + 1 < W; ++w) {
                ringn[w] = ringn[w + 1];
#pragma unroll
                for (int c = 0; c < 5; ++c) ring[w][c] = ring[w + 1][c];
            }
            ringn[W - 1] = 0;
#pragma unroll
            for (int c = 0; c < 5; ++c) ring[W - 1][c] = 0.0;
            if (ip >= 0 && ip < X) {                                   // the same for the whole workgroup: the barriers are met by all
                for (int e = t; e < HY * HZ; e += 256) {               // a. the channels of plane ip
                    const int jj = e / HZ, kk = e - jj * HZ;
                    const int js = j0 - R + jj, ks = k0 - R + kk;
                    double F = 0.0, M = 0.0;
                    int valid = 0;
                    if (js >= 0 && js < Y && ks >= 0 && ks < Z) {
                        const size_t at = ((size_t)ip * Y + js) * Z + ks;
                        const float f = fixed[at], m = warped[at];
                        if (isfinite(f) && isfinite(m)) F = (double)f, M = (double)m, valid = 1;
                    }
                    ch[0][jj][kk] = F, ch[1][jj][kk] = M;
                    ch[2][jj][kk] = __dmul_rn(F, F), ch[3][jj][kk] = __dmul_rn(M, M), ch[4][jj][kk] = __dmul_rn(F, M);
                    chn[jj][kk] = valid;
                }
                __syncthreads();
                for (int e = t; e < HY * kLZ; e += 256) {              // b. along axis 2, ascending
                    const int jj = e / kLZ, kk = e - jj * kLZ;
#pragma unroll
                    for (int c = 0; c < 5; ++c) {
                        double s = 0.0;
#pragma unroll
                        for (int w = 0; w < W; ++w) s = __dadd_rn(s, ch[c][jj][kk + w]);
                        rs[c][jj][kk] = s;
                    }
                    int sn = 0;
#pragma unroll
                    for (int w = 0; w < W; ++w) sn += chn[jj][kk + w];
                    rsn[jj][kk] = sn;
                }
                __syncthreads();
#pragma unroll
                for (int c = 0; c < 5; ++c) {                          // c. along axis 1, ascending
                    double s = 0.0;
#pragma unroll
                    for (int w = 0; w < W; ++w) s = __dadd_rn(s, rs[c][tj + w][tk]);
                    ring[W - 1][c] = s;
                }
                int sn = 0;
#pragma unroll
                for (int w = 0; w < W; ++w) sn += rsn[tj + w][tk];
                ringn[W - 1] = sn;
            }
            const int i = ip - R;                                      // d. the ring holds planes i - R .. i + R
            if (i < i0 || j >= Y || k >= Z) continue;                  // no barrier below
            double S[5];
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                double s = 0.0;
#pragma unroll
                for (int w = 0; w < W; ++w) s = __dadd_rn(s, ring[w][c]);
                S[c] = s;
            }
            int cnt = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) cnt += ringn[w];
            const size_t idx = ((size_t)i * Y + j) * Z + k;
            const float f = fixed[idx], m = warped[idx];
            float d = 0.f, wt = 0.f;
            bool ok = false;
            if (isfinite(f) && isfinite(m) && cnt >= 2) {
                const double F = (double)f, M = (double)m, nn = (double)cnt;
                const double mF = __ddiv_rn(S[0], nn), mM = __ddiv_rn(S[1], nn);
                const double A = __dsub_rn(S[4], __dmul_rn(mM, S[0]));
                const double B = __dsub_rn(S[2], __dmul_rn(mF, S[0]));
                const double C = __dsub_rn(S[3], __dmul_rn(mM, S[1]));
                if (B > 0.0 && C > 0.0 && A != 0.0) {
                    const double d64 = __dsub_rn(__dmul_rn(__dsub_rn(M, mM), __ddiv_rn(B, A)), __dsub_rn(F, mF));
                    const double q = __ddiv_rn(__dmul_rn(A, A), __dmul_rn(B, C));
                    const double w64 = q > 1.0 ? 1.0 : q;
                    if (isfinite(d64) && isfinite(w64)) ok = true, d = (float)d64, wt = (float)w64;
                }
            }
            float upd[3] = {0.f, 0.f, 0.f};
            if (ok) {
                const float g[3] = {axis_gradient(fixed, idx, i, X, (size_t)Y * Z), axis_gradient(fixed, idx, j, Y, (size_t)Z),
                                    axis_gradient(fixed, idx, k, Z, 1)};
                const float g2 = __fadd_rn(__fadd_rn(__fmul_rn(g[0], g[0]), __fmul_rn(g[1], g[1])), __fmul_rn(g[2], g[2]));
                const float den = __fadd_rn(g2, __fmul_rn(d, d));
                const float s = __fmul_rn(den > MRISR_DEFORM_DEN_MIN ? __fdiv_rn(d, den) : 0.f, wt);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    float x = -__fmul_rn(s, g[a]);
                    x = x > max_step ? max_step : (x < -max_step ? -max_step : x);
                    upd[a] = x == x ? x : 0.f;
                }
                acc.add((double)wt, 0.0, 1);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) v[a * n + idx] = update ? __fmul_rn(upd[a], scale) : __fadd_rn(u[a * n + idx], upd[a]);
        }
    }
    block_sum_to_slot(acc, part, &slots[blockIdx.x]);
    if (blockIdx.x == 0)                                               // the wave that adds the slots reads nslots of them
        for (int s = (int)gridDim.x + t; s < nslots; s += 256) slots[s] = DeformSlot{0.0, 0.0, 0, 0.f, 0};
}

extern "C" int mrisr_f32_volume_lcc_force(const float* fixed, const float* warped, const float* u, int X, int Y, int Z, int radius,
                                          float max_step, float scale, int update, float* v, void* workspace, void* stats_row,
                                          void* stream) {
    const char* name = "f32_volume_lcc_force";
    if (!fixed || !warped || !u || !v || !workspace) MRISR_FAIL(MRISR_E_ARG, "%s: null pointer", name);
    if (radius < 1 || radius > kLccMaxRadius) MRISR_FAIL(MRISR_E_SHAPE, "%s: radius %d (1..%d)", name, radius, kLccMaxRadius);
    if (!(max_step >= 0.f) || !isfinite(max_step)) MRISR_FAIL(MRISR_E_ARG, "%s: max_step %g (finite, not negative)", name, (double)max_step);
    if (!(scale > 0.f) || !isfinite(scale)) MRISR_FAIL(MRISR_E_ARG, "%s: scale %g (finite, positive)", name, (double)scale);
    if (update != 0 && update != 1) MRISR_FAIL(MRISR_E_ARG, "%s: update %d (0: v = u + upd, 1: w = upd * scale)", name, update);
    BrickGrid g;
    if (const int rc = check_field_volume(name, X, Y, Z, &g)) return rc;
    if (!aligned_to(fixed, 4) || !aligned_to(warped, 4) || !aligned_to(u, 4) || !aligned_to(v, 4) || !aligned_to(workspace, 8) ||
        !aligned_to(stats_row, 8))
        MRISR_FAIL(MRISR_E_ARG, "%s: misaligned pointer", name);
    if (v == u || v == fixed || v == warped) MRISR_FAIL(MRISR_E_ARG, "%s: the output must be a buffer of its own", name);
    // tiles of 32 x 8 x 32 voxels: never more than the 2 x 2 x 64 bricks of the same volume, far inside unsigned
    const unsigned ntx = ceil_div(X, kLX), nty = ceil_div(Y, kLY), ntz = ceil_div(Z, kLZ);
    const unsigned ntiles = ntx * nty * ntz;
    const unsigned grid = ntiles < (unsigned)g.nslots ? ntiles : (unsigned)g.nslots;
    hipStream_t s = (hipStream_t)stream;
    DeformSlot* slots = (DeformSlot*)workspace;
#define MRISR_LCC_LAUNCH(R) \
    lcc_kernel<R><<<grid, 256, 0, s>>>(fixed, warped, u, X, Y, Z, max_step, scale, update, v, ntiles, nty, ntz, g.nslots, slots)
    switch (radius) {
        case 1: MRISR_LCC_LAUNCH(1); break;
        case 2: MRISR_LCC_LAUNCH(2); break;
        case 3: MRISR_LCC_LAUNCH(3); break;
        default: MRISR_LCC_LAUNCH(4); break;
    }
#undef MRISR_LCC_LAUNCH
    MRISR_CHECK_LAUNCH(name);
    if (stats_row) {
        force_stats_kernel<<<1, 64, 0, s>>>(slots, g.nslots, (StatsRow*)stats_row);
        MRISR_CHECK_LAUNCH(name);
    }
    return MRISR_OK;
}
