// Rician non-local-means denoising of volumes on the device (gfx950; extension).  The specification is
// volume_denoise.denoise_np / estimate_sigma_np / noise_params_np; f32_volume_nlm is bit-equal to denoise_np.  Compiled with
// -ffp-contract=off (build.py): every product, sum and division is one rounded float32 operation, never an fma.
//
// A volume is (X, Y, Z) in C order, Z fastest.  Patch radius 1, search radius R in 1..5.
//
//   f32_volume_nlm   one workgroup of 512 threads (8 waves) per tile of 8 x 16 x 32 voxels (axis 0, 1, 2).  The tile plus a halo
//     of R + 1 is staged in LDS once, clamped at the volume's edges (edge replication: position q holds v[c(q)]), next to the
//     4096 weights of the table.  A thread owns one (y, z) column of the tile, the 32 lanes of a half-wave lie along z - the 32
//     dwords of one LDS row, whatever the row stride, so every ds_read_b32 of the loop is conflict-free - and walks the 8 voxels
//     of its column along axis 0 for each candidate t in ascending (t0, t1, t2) order: a plane sum is 9 squared differences
//     ((row + row) + row of (sq + sq) + sq), three plane sums in registers give d = (plane(x - 1) + plane(x)) + plane(x + 1), and
//     each step forms one new plane - 10 planes for 8 voxels instead of 24.  num, den and wmax of the 8 voxels stay in registers
//     over all candidates; no atomics.  Global traffic: the tile plus halo read once, the tile written once.
//   f32_volume_noise_params   the Rayleigh estimate of sigma over a background mask - float64 partial sums and counts of at most
//     1024 workgroups in fixed slots, every element in a fixed slot and a fixed place of its order - and a last launch of one
//     workgroup that adds the slots in order and writes params = (inv_h2, two_sigma2, sigma, beta) by noise_params_np's rule.
#include "volume_common.h"

constexpr int kNlmMaxRadius = 5;
constexpr int kNlmTable = 4096;                        // weights: exp(-(k + 0.5) / 256), x = k / 256 in [0, 16)
constexpr int kNlmT0 = 8, kNlmT1 = 16, kNlmT2 = 32;    // the tile: axis 0 (walked by a thread), axis 1, axis 2 (the lanes)
constexpr int kNlmThreads = kNlmT1 * kNlmT2;
constexpr int kNoiseSlots = 1024;                      // workgroups of the noise sums
constexpr int kNoisePerThread = 16;

static inline size_t nlm_lds_bytes(int R) {
    const int h = R + 1;
    return ((size_t)(kNlmT0 + 2 * h) * (kNlmT1 + 2 * h) * (kNlmT2 + 2 * h) + kNlmTable) * sizeof(float);
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// grid (z tiles, y tiles, x tiles); dynamic LDS nlm_lds_bytes(R)
__global__ __launch_bounds__(kNlmThreads) void nlm_kernel(const float* __restrict__ vol, int X, int Y, int Z, int R, int rician,
                                                          const float* __restrict__ params, const float* __restrict__ table,
                                                          float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int h = R + 1;
    const int P1 = kNlmT1 + 2 * h, P2 = kNlmT2 + 2 * h;
    const int S0 = P1 * P2;                            // floats of a staged plane
    const int total = (kNlmT0 + 2 * h) * S0;
    float* tab = lds;
    float* tile = lds + kNlmTable;                     // tile[(qx P1 + qy) P2 + qz] = v[c(x0 - h + qx, y0 - h + qy, z0 - h + qz)]
    const int t = threadIdx.x;
    const int x0 = blockIdx.z * kNlmT0, y0 = blockIdx.y * kNlmT1, z0 = blockIdx.x * kNlmT2;
    for (int e = t; e < kNlmTable; e += kNlmThreads) tab[e] = table[e];
    for (int e = t; e < total; e += kNlmThreads) {
        const int qz = e % P2, r = e / P2;
        const int qy = r % P1, qx = r / P1;
        const int gx = clampi(x0 - h + qx, X - 1), gy = clampi(y0 - h + qy, Y - 1), gz = clampi(z0 - h + qz, Z - 1);
        tile[e] = vol[((size_t)gx * Y + gy) * Z + gz];
    }
    __syncthreads();
    const int tz = t % kNlmT2, ty = t / kNlmT2;
    const int y = y0 + ty, z = z0 + tz;
    if (y >= Y || z >= Z) return;                      // no barrier follows
    const int steps = X - x0 < kNlmT0 ? X - x0 : kNlmT0;      // voxels of this column inside the volume, >= 1
    const float inv_h2 = params[0], two_sigma2 = params[1];
    const float* centre = tile + (h * P1 + h + ty) * P2 + h + tz;      // voxel i of the column: centre[i S0]
    float num[kNlmT0], den[kNlmT0], wmax[kNlmT0];
#pragma unroll
    for (int i = 0; i < kNlmT0; ++i) num[i] = den[i] = wmax[i] = 0.f;
    for (int t0 = -R; t0 <= R; ++t0)
        for (int t1 = -R; t1 <= R; ++t1) {
            const bool in1 = y + t1 >= 0 && y + t1 < Y;
            for (int t2 = -R; t2 <= R; ++t2) {
                if (t0 == 0 && t1 == 0 && t2 == 0) continue;
                const bool in12 = in1 && z + t2 >= 0 && z + t2 < Z;
                const int off = (t0 * P1 + t1) * P2 + t2;      // |off| stays inside the halo: |t| <= R, the patch adds 1
                // the sum of the 9 squared differences of the plane through voxel i of the column (i = -1 .. kNlmT0)
                auto plane = [&](int i) -> float {
                    const float* a = centre + i * S0;
                    const float* b = a + off;
                    float rows[3];
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy) {
                        const float* ar = a + dy * P2;
                        const float* br = b + dy * P2;
                        const float e0 = ar[-1] - br[-1], e1 = ar[0] - br[0], e2 = ar[1] - br[1];
                        rows[dy + 1] = (e0 * e0 + e1 * e1) + e2 * e2;
                    }
                    return (rows[0] + rows[1]) + rows[2];
                };
                float prev = plane(-1), cur = plane(0);
#pragma unroll
                for (int i = 0; i < kNlmT0; ++i) {
                    if (i < steps) {                   // uniform across the workgroup
                        const float next = plane(i + 1);
                        const float d = (prev + cur) + next;
                        const float x = d * inv_h2;
                        const int gx = x0 + i + t0;
                        if (in12 && gx >= 0 && gx < X && x >= 0.f && x < 16.f) {      // NaN and inf compare false
                            const float w = tab[(int)(x * 256.f)];                     // 0 .. 4095: x * 256 is exact and below 4096
                            float val = centre[i * S0 + off];
                            if (rician) val = val * val;
                            num[i] = num[i] + w * val;
                            den[i] = den[i] + w;
                            wmax[i] = wmax[i] > w ? wmax[i] : w;
                        }
                        prev = cur;
                        cur = next;
                    }
                }
            }
        }
#pragma unroll
    for (int i = 0; i < kNlmT0; ++i) {
        if (i >= steps) continue;
        const float c = centre[i * S0];
        float o = c;                                   // a voxel that is not finite is copied through
        if (isfinite(c)) {
            const float cv = rician ? c * c : c;
            const float wc = wmax[i] > 0.f ? wmax[i] : 1.f;
            const float n = num[i] + wc * cv;
            const float dn = den[i] + wc;
            const float m = __fdiv_rn(n, dn);
            o = m;
            if (rician) {
                const float u = m - two_sigma2;
                // the float32 square root, correctly rounded: a float64 square root rounded once more (53 >= 2 * 24 + 2 bits)
                o = u > 0.f ? (float)__dsqrt_rn((double)u) : 0.f;
            }
        }
        out[((size_t)(x0 + i) * Y + y) * Z + z] = o;
    }
}

extern "C" int mrisr_f32_volume_nlm(const float* vol, int X, int Y, int Z, int radius, int rician, const float* params, const float* table,
                                    float* out, void* stream) {
    if (!vol || !params || !table || !out) MRISR_FAIL(MRISR_E_ARG, "f32_volume_nlm: null pointer");
    if (radius < 1 || radius > kNlmMaxRadius) MRISR_FAIL(MRISR_E_ARG, "f32_volume_nlm: radius %d (1..%d)", radius, kNlmMaxRadius);
    if (const int rc = check_volume_extents("f32_volume_nlm", X, Y, Z)) return rc;
    if (!aligned_to(vol, 4) || !aligned_to(params, 4) || !aligned_to(table, 4) || !aligned_to(out, 4))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_nlm: misaligned pointer");
    if (vol == out) MRISR_FAIL(MRISR_E_ARG, "f32_volume_nlm: vol and out must be two buffers");
    static_assert(kNlmT2 == 32 && kNlmThreads == 512, "nlm_kernel: the 32 lanes of a half-wave along axis 2, 8 waves");
    const size_t lds = nlm_lds_bytes(radius);
    // a tile past the default 64 KB needs the limit raised on the CURRENT device: asked for at every such launch (a host-side
    // attribute, not a stream operation)
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(nlm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)nlm_lds_bytes(kNlmMaxRadius)) != hipSuccess)
        MRISR_FAIL(MRISR_E_HIP, "f32_volume_nlm: cannot raise the LDS limit");
    const dim3 grid((unsigned)ceil_div(Z, kNlmT2), (unsigned)ceil_div(Y, kNlmT1), (unsigned)ceil_div(X, kNlmT0));
    nlm_kernel<<<grid, kNlmThreads, lds, (hipStream_t)stream>>>(vol, X, Y, Z, radius, rician != 0, params, table, out);
    MRISR_CHECK_LAUNCH("f32_volume_nlm");
    return MRISR_OK;
}

// ---------------------------------------------------------------- sigma from the background, the filter's parameters

struct NoiseSlot {
    double sum;
    long long count;
};

// workgroup b owns the elements [b chunk, (b + 1) chunk); thread t of it the elements b chunk + t, + 256, ... in that order
__global__ __launch_bounds__(256) void noise_sums_kernel(const float* __restrict__ vol, const uint8_t* __restrict__ background, size_t n,
                                                         size_t chunk, NoiseSlot* __restrict__ slots) {
    __shared__ double ssum[4];
    __shared__ long long scount[4];
    const size_t lo = (size_t)blockIdx.x * chunk;
    const size_t hi = lo + chunk < n ? lo + chunk : n;
    double s = 0.0;
    long long c = 0;
    for (size_t i = lo + threadIdx.x; i < hi; i += 256) {
        const float v = vol[i];
        if (background[i] && isfinite(v)) {
            s += (double)v * (double)v;
            ++c;
        }
    }
    s = wave_sum_d(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        ssum[wave] = s;
        scount[wave] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        slots[blockIdx.x].sum = ((ssum[0] + ssum[1]) + ssum[2]) + ssum[3];
        slots[blockIdx.x].count = ((scount[0] + scount[1]) + scount[2]) + scount[3];
    }
}

__global__ void noise_params_kernel(const NoiseSlot* __restrict__ slots, int nslots, float beta, float sigma_given,
                                    float* __restrict__ params, long long* __restrict__ count) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float sigma = sigma_given;
    long long c = 0;
    if (nslots > 0) {
        double s = 0.0;
        for (int b = 0; b < nslots; ++b) {
            s += slots[b].sum;
            c += slots[b].count;
        }
        sigma = c > 0 ? (float)__dsqrt_rn(s / (2.0 * (double)c)) : 0.f;
    }
    const float two_sigma2 = (sigma * sigma) * 2.f;
    const float h2 = (two_sigma2 * beta) * 27.f;
    params[0] = __fdiv_rn(1.f, h2);                    // sigma == 0: inf, every weight is then 0
    params[1] = two_sigma2;
    params[2] = sigma;
    params[3] = beta;
    *count = c;
}

extern "C" size_t mrisr_f32_volume_noise_workspace_bytes(void) { return (size_t)kNoiseSlots * sizeof(NoiseSlot); }

extern "C" int mrisr_f32_volume_noise_params(const float* vol, const unsigned char* background, size_t n, float beta, float sigma_given,
                                             float* params, long long* count, void* ws, void* stream) {
    const bool given = sigma_given > 0.f;
    if (!params || !count || !ws || (!given && (!vol || !background))) MRISR_FAIL(MRISR_E_ARG, "f32_volume_noise_params: null pointer");
    if (!given && n == 0) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_noise_params: no voxels");
    if (!(beta > 0.f) || !isfinite(beta)) MRISR_FAIL(MRISR_E_ARG, "f32_volume_noise_params: beta %g (finite, positive)", (double)beta);
    if (!(sigma_given >= 0.f) || !isfinite(sigma_given))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_noise_params: sigma %g (finite; 0: estimate it)", (double)sigma_given);
    if (!aligned_to(params, 4) || !aligned_to(count, 8) || !aligned_to(ws, 8) || (!given && !aligned_to(vol, 4)))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_noise_params: misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    NoiseSlot* slots = (NoiseSlot*)ws;
    int nslots = 0;
    if (!given) {
        nslots = capped_grid(n, (size_t)256 * kNoisePerThread, kNoiseSlots);
        const size_t chunk = (n + (size_t)nslots - 1) / (size_t)nslots;
        noise_sums_kernel<<<nslots, 256, 0, s>>>(vol, background, n, chunk, slots);
        MRISR_CHECK_LAUNCH("f32_volume_noise_params (sums)");
    }
    noise_params_kernel<<<1, 64, 0, s>>>(slots, nslots, beta, sigma_given, params, count);
    MRISR_CHECK_LAUNCH("f32_volume_noise_params");
    return MRISR_OK;
}
