// Edge sharpness across tissue interfaces on the device (gfx950; extension): the two sides of the interface
// between the classes 1..k and k+1..K of a label volume, the signed distance of every voxel to that interface from the two distance
// transforms of csrc/volume_surface.hip, and the edge-spread function of a volume across up to five interfaces in one pass.  The
// specification is mri_superresolution_amd/volume_sharpness.py; the sides, the signed distance and the counts of a profile are
// bit-equal to it, the float64 sums of a profile are those of another order of addition and the same bits on every run.  Compiled
// with -ffp-contract=off (build.py): the bin of a voxel is a rounded float32 sum and a rounded float32 quotient, never fused.
//
// A volume is (X, Y, Z) in C order; every kernel here is elementwise in the flattened index.
//
//   interface_sides   0 where the label is 0, 1 where it is in 1..k, 2 above k.
//   signed_distance   +sqrt(dA2) on side 2, -sqrt(dB2) on side 1, NaN on side 0; the root is the float64 root rounded to float32,
//                     which is the correctly rounded float32 root (53 >= 2 * 24 + 2 bits).
//   edge_profile      a wave owns a fixed contiguous run of voxels (a multiple of 64) and walks it 64 at a time, lane l the voxel
//                     base + l.  (Interleaving the waves' steps instead, to spread the voxels near an interface over more waves,
//                     was measured and is 10 % slower: DESIGN.md.)  It reads the J signed distances of its voxels first;
//                     bin b = floor(fl32(fl32(s + R) / w)).  If no lane has a bin in 0..nb-1 for any interface - most of a volume -
//                     the wave goes on without reading the volume.  Otherwise, per interface, it loops over the bins present
//                     among its lanes (by ballot, the bin of the lowest lane first): the lanes of that bin are added in the fixed
//                     tree of wave_sum_d, the others contribute 0.0, and lane 0 adds the three float64 sums and the count to the
//                     wave's private bins in LDS (J nb <= 320 bins x 28 bytes per wave, 35 KB per workgroup at most).  At the end
//                     the four waves' bins are added in wave order into the workgroup's fixed slot; a second launch, one wave per
//                     bin, adds the slots: lane l takes the slots l, l + 64, ... in ascending order, then the same fixed tree.  No
//                     atomics at all: voxels, lanes, waves and slots meet in an order that depends on the size of the volume alone.
// No kernel reads or writes outside its arrays: the last wave's run ends at n, a wave whose run starts past n does nothing.
#include "volume_common.h"

constexpr int kEdgeMaxInterfaces = 5;
constexpr int kEdgeMinBins = 2, kEdgeMaxBins = 64;
constexpr int kEdgeSlots = 1024;           // workgroups of the profile pass at most
constexpr int kEdgePerThread = 16;         // voxels per thread below which a workgroup is not worth its slot
constexpr int kElementwisePerBlock = 2048;
constexpr int kElementwiseMaxBlocks = 1 << 16;

struct EdgeBin {
    long long count;
    double sum_v, sum_s, sum_vv;
};

// ---------------------------------------------------------------- the sides and the signed distance

__global__ __launch_bounds__(256) void interface_sides_kernel(const uint8_t* __restrict__ labels, size_t n, int k, uint8_t* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned l = labels[i];
        out[i] = (uint8_t)(l == 0u ? 0u : (l <= (unsigned)k ? 1u : 2u));
    }
}

__device__ __forceinline__ float sqrt_rn_f32(float x) { return (float)__dsqrt_rn((double)x); }

__global__ __launch_bounds__(256) void signed_distance_kernel(const uint8_t* __restrict__ sides, const float* __restrict__ da2,
                                                              const float* __restrict__ db2, size_t n, float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned side = sides[i];
        float s = __uint_as_float(0x7fc00000u);
        if (side == 2u) s = sqrt_rn_f32(da2[i]);
        else if (side == 1u) s = -sqrt_rn_f32(db2[i]);
        out[i] = s;
    }
}

// ---------------------------------------------------------------- the profile

// LDS of a workgroup: 4 waves x B bins x 3 doubles, then 4 waves x B counts
static inline size_t edge_lds_bytes(int B) { return (size_t)4 * B * (3 * sizeof(double) + sizeof(unsigned)); }

template <int J>
__global__ __launch_bounds__(256) void edge_profile_kernel(const float* __restrict__ vol, const float* __restrict__ sdist, size_t n,
                                                           size_t chunk, float R, float w, int nb, EdgeBin* __restrict__ slots) {
    extern __shared__ double edge_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int B = J * nb;
    double* sums = edge_lds + (size_t)wave * B * 3;
    unsigned* counts = reinterpret_cast<unsigned*>(edge_lds + (size_t)4 * B * 3) + (size_t)wave * B;
    for (int i = lane; i < B; i += 64) {
        sums[3 * i] = 0.0;
        sums[3 * i + 1] = 0.0;
        sums[3 * i + 2] = 0.0;
        counts[i] = 0u;
    }
    __syncthreads();
    const size_t lo = ((size_t)blockIdx.x * 4 + wave) * chunk;         // chunk is a multiple of 64
    const size_t hi = lo + chunk < n ? lo + chunk : n;
    const float nbf = (float)nb;
    for (size_t base = lo; base < hi; base += 64) {
        const size_t i = base + lane;
        const bool in = i < hi;
        float s[J], bin[J];
        bool ok[J];
        bool any = false;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            s[j] = in ? sdist[(size_t)j * n + i] : 0.f;
            bin[j] = floorf(__fdiv_rn(__fadd_rn(s[j], R), w));
            ok[j] = in && isfinite(s[j]) && bin[j] >= 0.f && bin[j] < nbf;      // NaN fails every comparison
            any |= ok[j];
        }
        if (!__any(any)) continue;                                     // wave-uniform: no lane leaves alone
        const float v = any ? vol[i] : 0.f;
        const bool finite_v = isfinite(v);
        const double dv = (double)v, dvv = dv * dv;                    // exact: 48 bits
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const bool valid = ok[j] && finite_v;
            const int b = valid ? (int)bin[j] : -1;
            const double ds = (double)s[j];
            unsigned long long todo = __ballot(valid);
            while (todo) {                                             // wave-uniform
                const int leader = __ffsll((long long)todo) - 1;
                const int lb = __shfl(b, leader, 64);
                const bool mine = b == lb;                             // lb >= 0: only valid lanes
                const unsigned long long members = __ballot(mine);
                const double sv = wave_sum_d(mine ? dv : 0.0);
                const double ss = wave_sum_d(mine ? ds : 0.0);
                const double svv = wave_sum_d(mine ? dvv : 0.0);
                if (lane == 0) {
                    double* cell = sums + 3 * (j * nb + lb);
                    cell[0] += sv;
                    cell[1] += ss;
                    cell[2] += svv;
                    counts[j * nb + lb] += (unsigned)__popcll(members);
                }
                todo &= ~members;
            }
        }
    }
    __syncthreads();
    const double* all = edge_lds;
    const unsigned* call = reinterpret_cast<const unsigned*>(edge_lds + (size_t)4 * B * 3);
    for (int i = threadIdx.x; i < B; i += 256) {
        EdgeBin r;
        r.count = (long long)(((unsigned long long)call[i] + call[B + i]) + call[2 * B + i]) + call[3 * B + i];
        r.sum_v = ((all[3 * i] + all[3 * (B + i)]) + all[3 * (2 * B + i)]) + all[3 * (3 * B + i)];
        r.sum_s = ((all[3 * i + 1] + all[3 * (B + i) + 1]) + all[3 * (2 * B + i) + 1]) + all[3 * (3 * B + i) + 1];
        r.sum_vv = ((all[3 * i + 2] + all[3 * (B + i) + 2]) + all[3 * (2 * B + i) + 2]) + all[3 * (3 * B + i) + 2];
        slots[(size_t)blockIdx.x * B + i] = r;
    }
}

// one wave per bin: lane l adds the slots l, l + 64, ... in ascending order, then the fixed tree.
// result: 4 words of 8 bytes per bin - the count (int64) and the float64 sums of v, s and v * v
__global__ __launch_bounds__(64) void edge_profile_finish_kernel(const EdgeBin* __restrict__ slots, int nslots, int B,
                                                                 unsigned long long* __restrict__ result) {
    const int bin = blockIdx.x, lane = threadIdx.x;
    long long c = 0;
    double sv = 0.0, ss = 0.0, svv = 0.0;
    for (int s = lane; s < nslots; s += 64) {
        const EdgeBin r = slots[(size_t)s * B + bin];
        c += r.count;
        sv += r.sum_v;
        ss += r.sum_s;
        svv += r.sum_vv;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    sv = wave_sum_d(sv);
    ss = wave_sum_d(ss);
    svv = wave_sum_d(svv);
    if (lane == 0) {
        unsigned long long* out = result + (size_t)bin * 4;
        out[0] = (unsigned long long)c;
        out[1] = (unsigned long long)__double_as_longlong(sv);
        out[2] = (unsigned long long)__double_as_longlong(ss);
        out[3] = (unsigned long long)__double_as_longlong(svv);
    }
}

// ---------------------------------------------------------------- entries

extern "C" int mrisr_u8_volume_interface_sides(const unsigned char* labels, size_t n, int k, unsigned char* out, void* stream) {
    if (!labels || !out) MRISR_FAIL(MRISR_E_ARG, "u8_volume_interface_sides: null pointer");
    if (k < 1 || k > 254) MRISR_FAIL(MRISR_E_ARG, "u8_volume_interface_sides: k %d (1..254)", k);
    if (n == 0 || n > 0xffffffffull) MRISR_FAIL(MRISR_E_SHAPE, "u8_volume_interface_sides: %zu voxels (1..2^32 - 1)", n);
    interface_sides_kernel<<<capped_grid(n, kElementwisePerBlock, kElementwiseMaxBlocks), 256, 0, (hipStream_t)stream>>>(labels, n, k, out);
    MRISR_CHECK_LAUNCH("u8_volume_interface_sides");
    return MRISR_OK;
}

extern "C" int mrisr_f32_volume_signed_distance(const unsigned char* sides, const float* da2, const float* db2, size_t n, float* out,
                                                void* stream) {
    if (!sides || !da2 || !db2 || !out) MRISR_FAIL(MRISR_E_ARG, "f32_volume_signed_distance: null pointer");
    if (!aligned_to(da2, 4) || !aligned_to(db2, 4) || !aligned_to(out, 4))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_signed_distance: misaligned pointer");
    if (n == 0 || n > 0xffffffffull) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_signed_distance: %zu voxels (1..2^32 - 1)", n);
    signed_distance_kernel<<<capped_grid(n, kElementwisePerBlock, kElementwiseMaxBlocks), 256, 0, (hipStream_t)stream>>>(sides, da2, db2, n, out);
    MRISR_CHECK_LAUNCH("f32_volume_signed_distance");
    return MRISR_OK;
}

static inline bool edge_shape_ok(int interfaces, int bins) {
    return interfaces >= 1 && interfaces <= kEdgeMaxInterfaces && bins >= kEdgeMinBins && bins <= kEdgeMaxBins;
}

extern "C" size_t mrisr_f32_volume_edge_workspace_bytes(int interfaces, int bins) {
    return edge_shape_ok(interfaces, bins) ? (size_t)kEdgeSlots * interfaces * bins * sizeof(EdgeBin) : 0;
}

extern "C" int mrisr_f32_volume_edge_profile(const float* vol, const float* sdist, int interfaces, size_t n, float radius, float bin_width,
                                             int bins, void* ws, unsigned long long* result, void* stream) {
    if (!vol || !sdist || !ws || !result) MRISR_FAIL(MRISR_E_ARG, "f32_volume_edge_profile: null pointer");
    if (!aligned_to(vol, 4) || !aligned_to(sdist, 4) || !aligned_to(ws, 8) || !aligned_to(result, 8))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_edge_profile: misaligned pointer");
    if (!edge_shape_ok(interfaces, bins))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_edge_profile: %d interfaces (1..%d), %d bins (%d..%d)", interfaces, kEdgeMaxInterfaces, bins,
                   kEdgeMinBins, kEdgeMaxBins);
    if (!(radius > 0.f && isfinite(radius) && bin_width > 0.f && isfinite(bin_width)))
        MRISR_FAIL(MRISR_E_ARG, "f32_volume_edge_profile: radius %g, bin width %g (finite, positive)", (double)radius, (double)bin_width);
    if (n == 0 || n > 0xffffffffull) MRISR_FAIL(MRISR_E_SHAPE, "f32_volume_edge_profile: %zu voxels (1..2^32 - 1)", n);
    hipStream_t s = (hipStream_t)stream;
    EdgeBin* slots = (EdgeBin*)ws;
    const int nslots = capped_grid(n, (size_t)256 * kEdgePerThread, kEdgeSlots);
    const size_t waves = (size_t)nslots * 4;
    const size_t chunk = ((n + waves - 1) / waves + 63) / 64 * 64;     // a wave's run: whole steps of 64 voxels
    const int B = interfaces * bins;
    const size_t lds = edge_lds_bytes(B);
    switch (interfaces) {
        case 1: edge_profile_kernel<1><<<nslots, 256, lds, s>>>(vol, sdist, n, chunk, radius, bin_width, bins, slots); break;
        case 2: edge_profile_kernel<2><<<nslots, 256, lds, s>>>(vol, sdist, n, chunk, radius, bin_width, bins, slots); break;
        case 3: edge_profile_kernel<3><<<nslots, 256, lds, s>>>(vol, sdist, n, chunk, radius, bin_width, bins, slots); break;
        case 4: edge_profile_kernel<4><<<nslots, 256, lds, s>>>(vol, sdist, n, chunk, radius, bin_width, bins, slots); break;
        default: edge_profile_kernel<5><<<nslots, 256, lds, s>>>(vol, sdist, n, chunk, radius, bin_width, bins, slots); break;
    }
    MRISR_CHECK_LAUNCH("f32_volume_edge_profile (bins)");
    edge_profile_finish_kernel<<<B, 64, 0, s>>>(slots, nslots, B, result);
    MRISR_CHECK_LAUNCH("f32_volume_edge_profile");
    return MRISR_OK;
}
