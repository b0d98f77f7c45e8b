// 3-D Gaussian-window SSIM, absolute and squared error of a pair of float32 volumes in ONE pass (gfx950; extension, DESIGN.md
// section 7).  The SSIM map is the reference's utils/losses.py:27-70 taken to three dimensions: the window is the outer product
// of the same normalised 1-D Gaussian along X, Y and Z, the padding is zero on every side (border windows truncated, not
// renormalised), C1 = (0.01 R)^2, C2 = (0.03 R)^2, and the map has the size of the volume.  Written with torch this is five
// moment volumes (a, b, a^2, b^2, ab) times three separable conv3d passes; here no moment ever reaches HBM.
//
// A volume is (X, Y, Z) in C order, Z fastest.  One workgroup owns a 16 (y) x 32 (z) tile and marches along x over its chunk
// [x0, x1) plus the window's halo on both sides (planes outside the volume are the zero padding and are not read):
//   stage     tile + halo of plane x of a and b, (16 + 2h) x (32 + 2h) values each, zero outside the volume, go from registers
//             (loaded one plane ahead, so that the HBM latency of plane x + 1 hides behind the arithmetic of plane x) to LDS.
//             The thread that stages an interior voxel of a plane of the chunk adds its |a - b| and (a - b)^2, in double.
//   z pass    thread = 4 consecutive z outputs of one staged row (register blocking as in loss.hip): W + 3 values of a and of b
//             from LDS -> the five z-filtered moments of the 4 outputs -> LDS, one 16-byte store per moment.
//   y pass    thread = one z column, 2 consecutive y outputs: W + 1 values per moment from LDS -> P[2][5], the (y, z)-filtered
//             moments of plane x at its two voxels.
//   x pass    in registers, scatter form: acc[j] holds the partial x sum of output plane x - h + j;
//                 acc[j] <- fmaf(g[W - 1 - j], P, acc[j + 1])   (j = 0 .. W - 2),   acc[W - 1] <- g[0] * P
//             is update and shift of the ring in one instruction per entry, with static register indices.  After plane x the
//             entry acc[0] is complete for output plane x - h (its taps arrived in ascending order); inside the chunk it becomes
//             an SSIM term, summed in double.
// Two barriers per plane.  Block partial sums: wave shuffle, then one double atomic per block and quantity, as loss.hip.
//
// Masked form (mrisr_f32_volume_metrics_masked; the kernel is a template on kMasked, every addition under if constexpr, so that the
// kMasked = false instantiation is the kernel it was): a uint8 mask volume is read as well and seven sums are kept - the three above
// over the whole volume, the same three over the mask's voxels, and the number of mask voxels.  |a - b| and (a - b)^2 take the
// mask byte of the staged interior voxel (fetched one plane ahead with a and b, for planes of the chunk only); the SSIM term takes
// the byte of the voxel it belongs to, (x - h, gy + o, gz), with one direct global read per output issued before the filter passes.
// The SSIM map itself is the unmasked one (full windows, zero padding): only the averaging is masked.
//
// LDS banks (ds_read_b32 / ds_write_b32: bank = dword address mod 32... conflicts within a 32-lane half): the z pass puts
// lane (row r, segment s) on dword r * P + 4 s + k; with the pitch P = 1 (mod 4) the four rows of a half wave start on
// 4 different residues mod 4 and the 32 lanes on 32 different banks.  The y pass reads 32 consecutive dwords per half wave.
#include "volume_common.h"

#include <math.h>

constexpr int kMaxWin = 15;                        // odd window sizes 3 .. 15 (the rule of utils/losses.py:_check_window)
constexpr int kTY = 16, kTZ = 32;                  // tile: 256 threads = 32 z columns x 8 pairs of y rows
constexpr int kMinChunk = 32;                      // shortest x chunk: bounds the x halo overhead to (32 + 2h) / 32
constexpr int kTargetBlocks = 2048;                // 256 CUs x 8

struct GaussWin3 { float g[kMaxWin]; };

static GaussWin3 make_window(float sigma, int win) {   // losses.py:10-18 in fp32, as loss.hip
    GaussWin3 w;
    float sum = 0.f;
    for (int i = 0; i < kMaxWin; ++i) w.g[i] = 0.f;
    for (int i = 0; i < win; ++i) {
        const float c = (float)(i - win / 2);
        w.g[i] = expf(-(c * c) / (2.0f * sigma * sigma));
        sum += w.g[i];
    }
    for (int i = 0; i < win; ++i) w.g[i] /= sum;
    return w;
}

// One SSIM term from the five filtered moments.  Every rounding is spelled out (no contraction left to the compiler), so that
// the masked and the unmasked instantiation of the kernel form bit-equal terms whatever else surrounds this code: one product
// is fused - mu1^2 into mu1^2 + mu2^2, the form the compiler chose for this expression under -ffp-contract=fast before there
// was a second instantiation - and every other product, difference and sum is rounded on its own.
__device__ __forceinline__ float ssim_term(float mu1, float mu2, float e11, float e22, float e12, float c1, float c2) {
#pragma clang fp contract(off)
    const float mu1sq = mu1 * mu1, mu2sq = mu2 * mu2, mu12 = mu1 * mu2;
    const float s11 = e11 - mu1sq, s22 = e22 - mu2sq, s12 = e12 - mu12;
    const float A1 = 2.f * mu12 + c1, A2 = 2.f * s12 + c2, B1 = fmaf(mu1, mu1, mu2sq) + c1, B2 = s11 + s22 + c2;
    return A1 * A2 / (B1 * B2);
}

// kMasked: mask (uint8, non-zero = foreground; the LAST parameter, so that the kernel arguments of the unmasked instantiation
// sit where they always sat) is read as well and sums has 7 entries instead of 3 (see the top of the file)
template <int kWin, bool kMasked>
__global__ __launch_bounds__(256) void volume_metrics_kernel(const float* __restrict__ a, const float* __restrict__ b, int X, int Y, int Z,
                                                             int chunk, float c1, float c2, const GaussWin3 win,
                                                             double* __restrict__ sums, const uint8_t* __restrict__ mask) {
    constexpr int kSums = kMasked ? 7 : 3;
    constexpr int kH = kWin / 2, kRows = kTY + 2 * kH, kCols = kTZ + 2 * kH;
    constexpr int kP = (kCols + 3) / 4 * 4 + 1;                    // 1 (mod 4): see above
    constexpr int kElems = kRows * kCols, kLoads = (kElems + 255) / 256;
    static_assert(kRows * (kTZ / 4) <= 256, "one z-pass segment per thread");
    __shared__ float ta[kRows * kP], tb[kRows * kP];
    __shared__ __attribute__((aligned(16))) float hz[5][kRows][kTZ];
    __shared__ double part[4][kSums];
    const int t = threadIdx.x;
    const int z0 = blockIdx.x * kTZ, y0 = blockIdx.y * kTY;
    const int x0 = blockIdx.z * chunk, x1 = min(x0 + chunk, X);
    const int xs = max(x0 - kH, 0), xlast = x1 - 1 + kH;           // planes xs .. xlast; those >= X are zero padding

    // what this thread stages, the same for every plane: offset inside a plane (-1: outside the volume or no element),
    // LDS slot, and whether the element is an interior voxel of the tile
    int poff[kLoads], slot[kLoads];
    bool interior[kLoads];
#pragma unroll
    for (int l = 0; l < kLoads; ++l) {
        const int e = t + l * 256, r = e / kCols, c = e - r * kCols;
        const int gy = y0 + r - kH, gz = z0 + c - kH;
        const bool in = e < kElems && gy >= 0 && gy < Y && gz >= 0 && gz < Z;
        poff[l] = in ? gy * Z + gz : -1;                           // Y * Z < 2^30
        slot[l] = e < kElems ? r * kP + c : -1;
        interior[l] = in && r >= kH && r < kH + kTY && c >= kH && c < kH + kTZ;
    }
    float ra[kLoads], rb[kLoads];
    uint8_t rm[kMasked ? kLoads : 1];                              // mask bytes of the interior voxels of a plane of the chunk
    auto fetch = [&](int x) {
        const bool plane = x < X;
        const size_t base = (size_t)(plane ? x : 0) * Y * Z;
#pragma unroll
        for (int l = 0; l < kLoads; ++l) {
            const bool in = plane && poff[l] >= 0;
            ra[l] = in ? a[base + poff[l]] : 0.f;
            rb[l] = in ? b[base + poff[l]] : 0.f;
            if constexpr (kMasked) rm[l] = x >= x0 && x < x1 && interior[l] ? mask[base + poff[l]] : (uint8_t)0;
        }
    };

    float acc[2][5][kWin];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < kWin; ++j) acc[o][q][j] = 0.f;
    double s_abs = 0.0, s_ssim = 0.0, s_sq = 0.0;
    double m_abs = 0.0, m_ssim = 0.0, m_sq = 0.0;                  // kMasked: the same three over the mask's voxels
    unsigned m_count = 0u;                                         // at most kLoads voxels per plane and thread: 32 bits suffice
    const int lz = t & (kTZ - 1), ly = (t >> 5) * 2;               // y / x pass: column lz, rows ly, ly + 1 of the tile
    const int gz = z0 + lz, gy = y0 + ly;

    fetch(xs);
    for (int x = xs; x <= xlast; ++x) {
        const bool plane = x < X;                                  // uniform over the block
        float P[2][5];
        // the SSIM output plane lags the staged plane by kH: its mask bytes are those of plane x - kH, read directly (one byte per
        // voxel against the eight of a and b) at the top of the iteration, so that the filter passes hide the latency.  An LDS
        // ring of the last kH + 1 planes' bytes was measured 1 to 6 % slower (profiles/NOTES.md): LDS is what bounds this kernel
        uint8_t mk[2] = {0, 0};
        if constexpr (kMasked) {
            if (x - kH >= x0 && gz < Z) {
                const size_t mbase = (size_t)(x - kH) * Y * Z + (size_t)gy * Z + gz;
                if (gy < Y) mk[0] = mask[mbase];
                if (gy + 1 < Y) mk[1] = mask[mbase + Z];
            }
        }
        if (plane) {
            const bool own = x >= x0 && x < x1;
#pragma unroll
            for (int l = 0; l < kLoads; ++l) {
                if (slot[l] >= 0) {
                    ta[slot[l]] = ra[l];
                    tb[slot[l]] = rb[l];
                }
                if (own && interior[l]) {
                    const double d = (double)ra[l] - (double)rb[l];      // exact
                    s_abs += fabs(d);
                    s_sq += d * d;
                    if constexpr (kMasked) {
                        if (rm[l]) {
                            m_abs += fabs(d);
                            m_sq += d * d;
                            ++m_count;
                        }
                    }
                }
            }
            __syncthreads();
            if (x < xlast) fetch(x + 1);
            if (t < kRows * (kTZ / 4)) {                           // z pass
                const int r = t >> 3, c = (t & 7) * 4;
                float u[kWin + 3], v[kWin + 3];
#pragma unroll
                for (int k = 0; k < kWin + 3; ++k) {
                    u[k] = ta[r * kP + c + k];
                    v[k] = tb[r * kP + c + k];
                }
                f32x4 h0, h1, h2, h3, h4;
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
                    for (int k = 0; k < kWin; ++k) {
                        const float uu = u[o + k], vv = v[o + k], g = win.g[k];
                        m0 = fmaf(g, uu, m0);
                        m1 = fmaf(g, vv, m1);
                        m2 = fmaf(g, uu * uu, m2);
                        m3 = fmaf(g, vv * vv, m3);
                        m4 = fmaf(g, uu * vv, m4);
                    }
                    h0[o] = m0; h1[o] = m1; h2[o] = m2; h3[o] = m3; h4[o] = m4;
                }
                *reinterpret_cast<f32x4*>(&hz[0][r][c]) = h0;
                *reinterpret_cast<f32x4*>(&hz[1][r][c]) = h1;
                *reinterpret_cast<f32x4*>(&hz[2][r][c]) = h2;
                *reinterpret_cast<f32x4*>(&hz[3][r][c]) = h3;
                *reinterpret_cast<f32x4*>(&hz[4][r][c]) = h4;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 5; ++q) {                          // y pass
                float col[kWin + 1];
#pragma unroll
                for (int k = 0; k < kWin + 1; ++k) col[k] = hz[q][ly + k][lz];
#pragma unroll
                for (int o = 0; o < 2; ++o) {
                    float m = 0.f;
#pragma unroll
                    for (int k = 0; k < kWin; ++k) m = fmaf(win.g[k], col[o + k], m);
                    P[o][q] = m;
                }
            }
        } else {
#pragma unroll
            for (int o = 0; o < 2; ++o)
#pragma unroll
                for (int q = 0; q < 5; ++q) P[o][q] = 0.f;
        }
        // x pass: update and shift
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int q = 0; q < 5; ++q) {
#pragma unroll
                for (int j = 0; j < kWin - 1; ++j) acc[o][q][j] = fmaf(win.g[kWin - 1 - j], P[o][q], acc[o][q][j + 1]);
                acc[o][q][kWin - 1] = win.g[0] * P[o][q];
            }
        if (x - kH >= x0 && gz < Z) {                              // output plane x - kH of the chunk is complete
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                if (gy + o < Y) {
                    const double term = (double)ssim_term(acc[o][0][0], acc[o][1][0], acc[o][2][0], acc[o][3][0], acc[o][4][0], c1, c2);
                    s_ssim += term;
                    if constexpr (kMasked) m_ssim += mk[o] ? term : 0.0;      // a select, no branch: the float32 code above stays the unmasked one
                }
            }
        }
    }
    s_abs = wave_sum_d(s_abs);
    s_ssim = wave_sum_d(s_ssim);
    s_sq = wave_sum_d(s_sq);
    double m_cnt = 0.0;
    if constexpr (kMasked) {
        m_abs = wave_sum_d(m_abs);
        m_ssim = wave_sum_d(m_ssim);
        m_sq = wave_sum_d(m_sq);
        m_cnt = wave_sum_d((double)m_count);                       // integers below 2^53: exact in any order
    }
    if ((t & 63) == 0) {
        part[t >> 6][0] = s_abs; part[t >> 6][1] = s_ssim; part[t >> 6][2] = s_sq;
        if constexpr (kMasked) {
            part[t >> 6][3] = m_abs; part[t >> 6][4] = m_ssim; part[t >> 6][5] = m_sq; part[t >> 6][6] = m_cnt;
        }
    }
    __syncthreads();
    if (t < kSums) atomic_add_f64(&sums[t], part[0][t] + part[1][t] + part[2][t] + part[3][t]);
}

template <int WIN>
static void launch_volume_metrics(dim3 grid, hipStream_t s, const float* a, const float* b, const uint8_t* mask, int X, int Y, int Z,
                                  int chunk, float c1, float c2, float sigma, double* sums) {
    if (mask) volume_metrics_kernel<WIN, true><<<grid, 256, 0, s>>>(a, b, X, Y, Z, chunk, c1, c2, make_window(sigma, WIN), sums, mask);
    else volume_metrics_kernel<WIN, false><<<grid, 256, 0, s>>>(a, b, X, Y, Z, chunk, c1, c2, make_window(sigma, WIN), sums, nullptr);
}

// the checks and the launch of both entry points; mask == nullptr: the unmasked kernel
static int volume_metrics_run(const char* name, const float* a, const float* b, const uint8_t* mask, int X, int Y, int Z, float val_range,
                              float sigma, int window_size, double* sums, void* stream) {
    if (window_size < 3 || window_size > kMaxWin || !(window_size & 1))
        MRISR_FAIL(MRISR_E_ARG, "%s: window_size %d (odd, 3..15)", name, window_size);
    if (!(sigma > 0.f) || !(val_range > 0.f)) MRISR_FAIL(MRISR_E_ARG, "%s: sigma %g, val_range %g (both positive)", name, sigma, val_range);
    if (const int rc = check_volume_extents(name, X, Y, Z)) return rc;
    const int tz = ceil_div(Z, kTZ), ty = ceil_div(Y, kTY);
    // x chunks: enough workgroups to fill the device, none shorter than kMinChunk planes
    long long want = (kTargetBlocks + (long long)tz * ty - 1) / ((long long)tz * ty);
    const int most = X / kMinChunk > 1 ? X / kMinChunk : 1;
    int nchunks = want < 1 ? 1 : (want > most ? most : (int)want);
    const int chunk = ceil_div(X, nchunks);
    nchunks = ceil_div(X, chunk);
    const float c1 = (0.01f * val_range) * (0.01f * val_range), c2 = (0.03f * val_range) * (0.03f * val_range);
    dim3 grid(tz, ty, nchunks);
    hipStream_t s = (hipStream_t)stream;
#define MRISR_CALL(WIN) launch_volume_metrics<WIN>(grid, s, a, b, mask, X, Y, Z, chunk, c1, c2, sigma, sums)
    switch (window_size) {
        case 3: MRISR_CALL(3); break;
        case 5: MRISR_CALL(5); break;
        case 7: MRISR_CALL(7); break;
        case 9: MRISR_CALL(9); break;
        case 11: MRISR_CALL(11); break;
        case 13: MRISR_CALL(13); break;
        default: MRISR_CALL(15); break;
    }
#undef MRISR_CALL
    MRISR_CHECK_LAUNCH(name);
    return MRISR_OK;
}

extern "C" int mrisr_f32_volume_metrics(const float* a, const float* b, int X, int Y, int Z, float val_range, float sigma,
                                        int window_size, double* sums, void* stream) {
    if (!a || !b || !sums) MRISR_FAIL(MRISR_E_ARG, "f32_volume_metrics: null pointer");
    return volume_metrics_run("f32_volume_metrics", a, b, nullptr, X, Y, Z, val_range, sigma, window_size, sums, stream);
}

extern "C" int mrisr_f32_volume_metrics_masked(const float* a, const float* b, const uint8_t* mask, int X, int Y, int Z, float val_range,
                                               float sigma, int window_size, double* sums7, void* stream) {
    if (!a || !b || !mask || !sums7) MRISR_FAIL(MRISR_E_ARG, "f32_volume_metrics_masked: null pointer");
    return volume_metrics_run("f32_volume_metrics_masked", a, b, mask, X, Y, Z, val_range, sigma, window_size, sums7, stream);
}

// out = (ssim, mse, rmse, mae, psnr); the voxel count is carried in double (a volume may hold more than 2^31 voxels)
__global__ void volume_metrics_finalize_kernel(const double* __restrict__ sums, double inv_voxels, double range2, double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double mae = sums[0] * inv_voxels, ssim = sums[1] * inv_voxels, mse = sums[2] * inv_voxels;
    out[0] = ssim;
    out[1] = mse;
    out[2] = __dsqrt_rn(mse);
    out[3] = mae;
    out[4] = mse < 1e-10 ? 100.0 : 10.0 * log10(range2 / mse);
}

extern "C" int mrisr_volume_metrics_finalize(const double* sums, int X, int Y, int Z, float val_range, double* out, void* stream) {
    if (!sums || !out) MRISR_FAIL(MRISR_E_ARG, "volume_metrics_finalize: null pointer");
    if (X < 1 || Y < 1 || Z < 1) MRISR_FAIL(MRISR_E_SHAPE, "volume_metrics_finalize: volume %d x %d x %d", X, Y, Z);
    volume_metrics_finalize_kernel<<<1, 64, 0, (hipStream_t)stream>>>(sums, 1.0 / ((double)X * (double)Y * (double)Z),
                                                                       (double)val_range * (double)val_range, out);
    MRISR_CHECK_LAUNCH("volume_metrics_finalize");
    return MRISR_OK;
}

// out[0..4]: the five metrics of the whole volume (as above); out[5..9]: the same five over the mask's voxels, every mean a
// division by the count sums[6], so that an empty mask gives five NaNs (0 / 0) without a host check; out[10]: the count
__global__ void volume_metrics_finalize_masked_kernel(const double* __restrict__ sums, double inv_voxels, double range2,
                                                      double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double count = sums[6];
#pragma unroll
    for (int region = 0; region < 2; ++region) {
        const double* q = sums + 3 * region;
        const double mae = region ? q[0] / count : q[0] * inv_voxels, ssim = region ? q[1] / count : q[1] * inv_voxels;
        const double mse = region ? q[2] / count : q[2] * inv_voxels;
        double* o = out + 5 * region;
        o[0] = ssim;
        o[1] = mse;
        o[2] = __dsqrt_rn(mse);
        o[3] = mae;
        o[4] = mse < 1e-10 ? 100.0 : 10.0 * log10(range2 / mse);      // NaN < 1e-10 is false: NaN stays NaN
    }
    out[10] = count;
}

extern "C" int mrisr_volume_metrics_finalize_masked(const double* sums7, int X, int Y, int Z, float val_range, double* out11, void* stream) {
    if (!sums7 || !out11) MRISR_FAIL(MRISR_E_ARG, "volume_metrics_finalize_masked: null pointer");
    if (X < 1 || Y < 1 || Z < 1) MRISR_FAIL(MRISR_E_SHAPE, "volume_metrics_finalize_masked: volume %d x %d x %d", X, Y, Z);
    volume_metrics_finalize_masked_kernel<<<1, 64, 0, (hipStream_t)stream>>>(sums7, 1.0 / ((double)X * (double)Y * (double)Z),
                                                                              (double)val_range * (double)val_range, out11);
    MRISR_CHECK_LAUNCH("volume_metrics_finalize_masked");
    return MRISR_OK;
}
