// Connected components of a uint8 mask volume on the device (gfx950; extension), and the two clean-up steps
// built on them: keep the largest component, fill the holes.  Integer only.  The specifications are
// volume_eval.label_components_np / largest_component_np / fill_holes_np; every result here is bit-equal to them.
//
// A mask is (X, Y, Z) uint8 in C order, Z fastest, non-zero = foreground.  A voxel's index is its C-order linear index.
// THE LABEL of a foreground voxel is 1 + the smallest index of its component; background is 0.  That rule needs no renumbering
// and makes the result independent of the order in which anything below happens.
//
// The labels buffer is the union-find parent array from the first launch on: labels[v] = 1 + parent(v), 0 for background, a
// root has labels[v] = v + 1.  Two invariants hold at every moment, for every value a slot has ever held:
//   (I1) parent(v) <= v, and a slot's value only ever decreases (every write is an atomicMin or stores a proven ancestor);
//   (I2) parent(v) lies in the component (of the final partition) of v.
// Hence every chain v, parent(v), ... is strictly decreasing until it stops at a root: every loop is bounded, and an index read
// from the array is < the index it was read at, so no access leaves the array.
//
// Three launches, no host synchronisation, no workgroup ever waits for another (no spin, no grid barrier, no flag):
//   local    one workgroup per tile of 8 x 8 x 32 voxels: union-find in LDS over the neighbour pairs inside the tile (LDS
//            atomicMin hooks the larger root under the smaller), then every voxel's local root - the smallest index of its
//            component inside the tile, local and global order agree - goes to labels as a global index.
//   merge    one thread per voxel on a tile's surface unions it with its neighbours in other tiles: find both roots, atomicMin
//            on the larger root's slot; when the value returned shows that the slot was no root any more, go on with that value
//            (the link it replaced must not be lost).  a + b decreases with every turn.
//   flatten  every voxel is compressed to its root; roots no longer change in this launch.  The same launch counts the
//            component sizes (one atomicAdd per run of equal roots inside a wave: runs along z are long) or marks the components
//            that touch the border, for the two uses below.
// Only "backward" neighbours are visited (the 13, 3, 4 or 2 offsets that are lexicographically negative): every pair once.
//
// STALE READS.  merge and flatten read slots that other workgroups write in the same launch.  Those reads are agent-scope relaxed
// atomic loads (a plain load may be served from a stale line of this CU's L1 or this XCD's L2), but the algorithm does not rely on
// their being fresh: by (I1) and (I2) an old value of a slot is still an ancestor-or-self in the same component with a smaller
// index, so a find that reads old values returns SOME node of the right component, the atomicMin that follows is executed on the
// current value and its return value tells whether that node was a root; if not, the loop goes on from the returned parent.
// In flatten no root changes and a non-root slot never reads as a root (it was below its own index before the launch began),
// so the root found is exact whatever mixture of old and new values is read on the way.
//
// keep_largest   sizes by root during flatten; one launch reduces (size << 32 | 0xffffffff - root) with a per-workgroup maximum
//                and ONE 64-bit atomicMax per workgroup - the larger size wins, then the smaller root - and counts the roots;
//                one launch writes dst = (label == kept label) and the three statistics.
// fill_holes     labels the ZERO voxels (invert, 6-connected, or 4-connected in the planes across plane_axis), marks during
//                flatten the components that own a voxel on a face of the volume (an edge of the plane), then
//                dst = mask != 0 or (zero voxel whose component is unmarked); the filled voxels are counted per workgroup.
#include "volume_common.h"

constexpr long long kMaxVoxels = 2147483646ll;          // 2^31 - 2: index + 1 fits a positive int32
constexpr int kTX = 8, kTY = 8, kTZ = 32;                // the tile; kTX * kTY * kTZ = 8 voxels for each of 256 threads
constexpr int kTile = kTX * kTY * kTZ;
constexpr unsigned kNone = 0xffffffffu;                  // LDS: background or outside the volume
constexpr int kBackward = 13;                            // offset k: dx = k / 9 - 1, dy = k / 3 % 3 - 1, dz = k % 3 - 1

enum { FLAT_PLAIN = 0, FLAT_SIZES = 1, FLAT_BORDER = 2 };

struct LabelHeader {                                     // first 64 bytes of the workspace
    unsigned long long best;                             // size << 32 | 0xffffffff - root of the largest component
    unsigned long long components;
    unsigned long long pad_[6];
};

__device__ __forceinline__ unsigned ld_agent(const unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned ld_lds(const unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---------------------------------------------------------------- LDS union-find (local indices, a root has P[i] == i)

__device__ __forceinline__ unsigned lds_find(const unsigned* P, unsigned i) {
    unsigned p = ld_lds(P + i);
    while (p < i) {                                      // (I1): strictly decreasing
        i = p;
        p = ld_lds(P + i);
    }
    return i;
}

__device__ __forceinline__ void lds_union(unsigned* P, unsigned a, unsigned b) {
    for (;;) {                                           // a + b decreases with every turn
        a = lds_find(P, a);
        b = lds_find(P, b);
        if (a == b) return;
        if (a < b) {
            const unsigned t = a;
            a = b;
            b = t;
        }
        const unsigned old = atomicMin(P + a, b);
        if (old >= a) return;                            // a was a root (old == a): hooked
        a = old;                                         // it was not: its former parent still has to meet b
    }
}

// labels[v] = 1 + the global index of the local root, 0 for background.  aux (may be null) is cleared for the flatten pass.
__global__ __launch_bounds__(256) void label_local_kernel(const uint8_t* __restrict__ mask, int X, int Y, int Z, unsigned nbmask,
                                                          int invert, unsigned* __restrict__ labels, unsigned* __restrict__ aux,
                                                          unsigned long long* __restrict__ zero_words, int zero_count) {
    __shared__ unsigned P[kTile];
    const int t = threadIdx.x;
    const int lz = t & (kTZ - 1), ly = t >> 5;           // voxel j of this thread: (lx = j, ly, lz), local index t + 256 j
    const int x0 = blockIdx.z * kTX, y = blockIdx.y * kTY + ly, z = blockIdx.x * kTZ + lz;
    if (zero_words && t < zero_count && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) zero_words[t] = 0ull;
    const bool column = y < Y && z < Z;
    unsigned fg = 0;                                     // bit j: voxel j is labelled
#pragma unroll
    for (int j = 0; j < kTX; ++j) {
        const int x = x0 + j;
        bool f = false;
        if (column && x < X) f = (mask[((size_t)x * Y + y) * Z + z] != 0) != (invert != 0);
        fg |= (f ? 1u : 0u) << j;
        P[t + 256 * j] = f ? (unsigned)(t + 256 * j) : kNone;
    }
    __syncthreads();
    for (int j = 0; j < kTX; ++j) {                      // not unrolled: 13 inlined unions are enough code
        if (!(fg >> j & 1u)) continue;
#pragma unroll
        for (int k = 0; k < kBackward; ++k) {
            if (!(nbmask >> k & 1u)) continue;
            const int nx = j + k / 9 - 1, ny = ly + k / 3 % 3 - 1, nz = lz + k % 3 - 1;
            if (nx < 0 || ny < 0 || ny >= kTY || nz < 0 || nz >= kTZ) continue;      // nx <= j: never past the tile
            const unsigned nb = (unsigned)(nx * 256 + ny * kTZ + nz);
            if (ld_lds(P + nb) != kNone) lds_union(P, (unsigned)(t + 256 * j), nb);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTX; ++j) {
        const int x = x0 + j;
        if (!column || x >= X) continue;
        const size_t g = ((size_t)x * Y + y) * Z + z;
        unsigned lab = 0;
        if (fg >> j & 1u) {
            const unsigned r = lds_find(P, (unsigned)(t + 256 * j));
            const int rx = (int)(r >> 8), ry = (int)(r >> 5) & (kTY - 1), rz = (int)r & (kTZ - 1);
            lab = (unsigned)(((size_t)(x0 + rx) * Y + (blockIdx.y * kTY + ry)) * Z + (blockIdx.x * kTZ + rz)) + 1u;
        }
        labels[g] = lab;
        if (aux) aux[g] = 0u;
    }
}

// ---------------------------------------------------------------- global union-find (P[v] = parent + 1, 0 = background)

// -> the root reached from x (0-based).  x must be a labelled voxel.  With compress, nodes on a path of more than two links are
// pointed at the root found (atomicMin: a slot never rises).
__device__ __forceinline__ unsigned label_find(unsigned* P, unsigned x, bool compress) {
    const unsigned start = x;
    int hops = 0;
    unsigned p = ld_agent(P + x) - 1u;
    while (p < x) {                                      // (I1); a background slot would give 0xffffffff and stop as well
        x = p;
        p = ld_agent(P + x) - 1u;
        ++hops;
    }
    if (compress && hops > 2) {
        unsigned y = start;
        for (;;) {                                       // y strictly decreases
            const unsigned q = ld_agent(P + y) - 1u;
            if (q <= x || q >= y) break;
            atomicMin(P + y, x + 1u);
            y = q;
        }
    }
    return x;
}

__device__ __forceinline__ void label_union(unsigned* P, unsigned a, unsigned b) {
    for (;;) {                                           // a + b decreases with every turn
        a = label_find(P, a, true);
        b = label_find(P, b, true);
        if (a == b) return;
        if (a < b) {
            const unsigned t = a;
            a = b;
            b = t;
        }
        const unsigned old = atomicMin(P + a, b + 1u) - 1u;
        if (old >= a) return;                            // a was a root: hooked under b
        a = old;                                         // a stale root: its former parent still has to meet b
    }
}

__global__ __launch_bounds__(256) void label_merge_kernel(int X, int Y, int Z, unsigned n, unsigned nbmask, unsigned* __restrict__ labels) {
    const unsigned long long gid = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n) return;
    const unsigned g = (unsigned)gid;
    const int z = (int)(g % (unsigned)Z);
    const unsigned row = g / (unsigned)Z;
    const int y = (int)(row % (unsigned)Y), x = (int)(row / (unsigned)Y);
    const int lx = x & (kTX - 1), ly = y & (kTY - 1), lz = z & (kTZ - 1);
    if (lx > 0 && ly > 0 && ly < kTY - 1 && lz > 0 && lz < kTZ - 1) return;      // no backward neighbour leaves the tile
    if (ld_agent(labels + g) == 0u) return;
#pragma unroll
    for (int k = 0; k < kBackward; ++k) {
        if (!(nbmask >> k & 1u)) continue;
        const int nx = x + k / 9 - 1, ny = y + k / 3 % 3 - 1, nz = z + k % 3 - 1;
        if (nx < 0 || ny < 0 || ny >= Y || nz < 0 || nz >= Z) continue;          // nx <= x < X
        if ((nx >> 3) == (x >> 3) && (ny >> 3) == (y >> 3) && (nz >> 5) == (z >> 5)) continue;      // the local pass did it
        const unsigned nb = (unsigned)(((size_t)nx * Y + ny) * Z + nz);
        if (ld_agent(labels + nb) != 0u) label_union(labels, g, nb);
    }
}

// labels[v] = root + 1.  FLAT_SIZES: aux[root] = voxels of the component.  FLAT_BORDER: aux[root] != 0 when the component owns a
// voxel with a coordinate at 0 or at its extent - 1 on an axis other than plane_axis.
template <int MODE>
__global__ __launch_bounds__(256) void label_flatten_kernel(int X, int Y, int Z, unsigned n, int plane_axis, unsigned* __restrict__ labels,
                                                            unsigned* __restrict__ aux) {
    const unsigned long long gid = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const bool inside = gid < n;
    const unsigned g = (unsigned)gid;
    unsigned root = kNone;
    if (inside && ld_agent(labels + g) != 0u) {
        root = label_find(labels, g, false);
        labels[g] = root + 1u;                           // an ancestor: (I1), (I2) hold for readers in this launch
    }
    if constexpr (MODE == FLAT_SIZES) {                  // every lane of the wave is here: runs of equal roots among the 64 lanes
        const int lane = threadIdx.x & 63;
        const unsigned prev = (unsigned)__shfl_up((int)root, 1, 64);
        const bool head = lane == 0 || prev != root;
        const unsigned long long heads = __ballot(head);
        if (head && root != kNone) {
            const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
            const int len = above ? __ffsll((long long)above) : 64 - lane;
            atomicAdd(aux + root, (unsigned)len);
        }
    }
    if constexpr (MODE == FLAT_BORDER) {
        if (root != kNone) {
            const int z = (int)(g % (unsigned)Z);
            const unsigned row = g / (unsigned)Z;
            const int y = (int)(row % (unsigned)Y), x = (int)(row / (unsigned)Y);
            const bool bx = x == 0 || x == X - 1, by = y == 0 || y == Y - 1, bz = z == 0 || z == Z - 1;
            if ((bx && plane_axis != 0) || (by && plane_axis != 1) || (bz && plane_axis != 2)) atomicOr(aux + root, 1u);
        }
    }
}

// ---------------------------------------------------------------- the two uses

__global__ __launch_bounds__(256) void label_largest_kernel(const unsigned* __restrict__ labels, const unsigned* __restrict__ sizes,
                                                            unsigned n, LabelHeader* __restrict__ hdr) {
    __shared__ unsigned long long skey[4];
    __shared__ unsigned scount[4];
    unsigned long long key = 0ull;
    unsigned roots = 0u;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const unsigned g = (unsigned)i;
        if (labels[g] == g + 1u) {                       // a root
            const unsigned long long k = (unsigned long long)sizes[g] << 32 | (unsigned long long)(0xffffffffu - g);
            key = k > key ? k : key;
            ++roots;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)key, o, 64);
        key = other > key ? other : key;
        roots += (unsigned)__shfl_xor((int)roots, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        skey[threadIdx.x >> 6] = key;
        scount[threadIdx.x >> 6] = roots;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            key = skey[w] > key ? skey[w] : key;
            roots += scount[w];
        }
        if (key) atomicMax(&hdr->best, key);
        if (roots) atomicAdd(&hdr->components, (unsigned long long)roots);
    }
}

// four consecutive voxels per thread; vec: dst on a 4-byte boundary (whole words are stored where all four voxels exist)
__global__ __launch_bounds__(256) void label_select_kernel(const unsigned* __restrict__ labels, unsigned n, const LabelHeader* __restrict__ hdr,
                                                           int vec, uint8_t* __restrict__ dst, double* __restrict__ stats3) {
    const unsigned long long best = hdr->best;
    const unsigned kept = best ? 0xffffffffu - (unsigned)(best & 0xffffffffull) + 1u : 0u;      // the label, 0: no component
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats3[0] = (double)hdr->components;
        stats3[1] = (double)(best >> 32);
        stats3[2] = (double)kept;
    }
    const unsigned long long i = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i + k < n) word |= (kept != 0u && labels[i + k] == kept ? 1u : 0u) << 8 * k;
    if (vec && i + 3 < n) {
        *reinterpret_cast<unsigned*>(dst + i) = word;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < n) dst[i + k] = (uint8_t)(word >> 8 * k);
    }
}

// filled (a double, zeroed by the local pass) += the zero voxels that became one
__global__ __launch_bounds__(256) void label_fill_kernel(const uint8_t* __restrict__ mask, const unsigned* __restrict__ labels,
                                                         const unsigned* __restrict__ touches, unsigned n, int vec, uint8_t* __restrict__ dst,
                                                         double* __restrict__ filled) {
    __shared__ unsigned scount[4];
    const unsigned long long i = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * 4;
    unsigned word = 0, count = 0;
    if (i < n) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i + k >= n) continue;
            unsigned bit = mask[i + k] != 0 ? 1u : 0u;
            const unsigned lab = labels[i + k];          // of the zero voxels: a root + 1 after flatten
            if (lab != 0u && touches[lab - 1u] == 0u) {
                bit = 1u;
                ++count;
            }
            word |= bit << 8 * k;
        }
        if (vec && i + 3 < n) {
            *reinterpret_cast<unsigned*>(dst + i) = word;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < n) dst[i + k] = (uint8_t)(word >> 8 * k);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += (unsigned)__shfl_xor((int)count, o, 64);
    if ((threadIdx.x & 63) == 0) scount[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = scount[0] + scount[1] + scount[2] + scount[3];
        if (total) atomic_add_f64(filled, (double)total);       // integers below 2^53: exact in any order
    }
}

// ---------------------------------------------------------------- host

static int check_shape(const char* name, int X, int Y, int Z) {
    if (const int rc = check_volume_extents(name, X, Y, Z)) return rc;
    if ((long long)X * Y * Z > kMaxVoxels)
        MRISR_FAIL(MRISR_E_UNSUPPORTED, "%s: volume %d x %d x %d has more than 2^31 - 2 voxels (labels are int32)", name, X, Y, Z);
    return MRISR_OK;
}

// bit k: backward offset k is a neighbour
static unsigned neighbour_mask(int connectivity, int plane_axis) {
    unsigned m = 0;
    for (int k = 0; k < kBackward; ++k) {
        const int d[3] = {k / 9 - 1, k / 3 % 3 - 1, k % 3 - 1};
        const int nonzero = (d[0] != 0) + (d[1] != 0) + (d[2] != 0);
        if (connectivity == 6 && nonzero != 1) continue;
        if (plane_axis >= 0 && d[plane_axis] != 0) continue;
        m |= 1u << k;
    }
    return m;
}

template <int MODE>
static int label_launches(const char* name, const uint8_t* mask, int X, int Y, int Z, int connectivity, int plane_axis, int invert,
                          unsigned* labels, unsigned* aux, unsigned long long* zero_words, int zero_count, hipStream_t s) {
    const unsigned n = (unsigned)((size_t)X * Y * Z);
    const unsigned nbmask = neighbour_mask(connectivity, plane_axis);
    const dim3 tiles(ceil_div(Z, kTZ), ceil_div(Y, kTY), ceil_div(X, kTX));
    const unsigned blocks = (unsigned)(((unsigned long long)n + 255) / 256);
    char what[96];
    snprintf(what, sizeof(what), "%s (local)", name);
    label_local_kernel<<<tiles, 256, 0, s>>>(mask, X, Y, Z, nbmask, invert, labels, aux, zero_words, zero_count);
    MRISR_CHECK_LAUNCH(what);
    snprintf(what, sizeof(what), "%s (merge)", name);
    label_merge_kernel<<<blocks, 256, 0, s>>>(X, Y, Z, n, nbmask, labels);
    MRISR_CHECK_LAUNCH(what);
    snprintf(what, sizeof(what), "%s (flatten)", name);
    label_flatten_kernel<MODE><<<blocks, 256, 0, s>>>(X, Y, Z, n, plane_axis, labels, aux);
    MRISR_CHECK_LAUNCH(what);
    return MRISR_OK;
}

extern "C" size_t mrisr_u8_volume_label_workspace_bytes(int X, int Y, int Z) {
    if (!volume_extents_ok(X, Y, Z) || (long long)X * Y * Z > kMaxVoxels) return 0;      // a size query sets no error text
    return sizeof(LabelHeader) + 8 * ((size_t)X * Y * Z);
}

extern "C" int mrisr_u8_volume_label(const uint8_t* mask, int X, int Y, int Z, int connectivity, int plane_axis, int invert,
                                     int32_t* labels, void* stream) {
    if (!mask || !labels) MRISR_FAIL(MRISR_E_ARG, "u8_volume_label: null pointer");
    if (!aligned_to(labels, 4)) MRISR_FAIL(MRISR_E_ARG, "u8_volume_label: misaligned pointer");
    if (connectivity != 6 && connectivity != 26) MRISR_FAIL(MRISR_E_ARG, "u8_volume_label: connectivity %d (6 or 26)", connectivity);
    if (plane_axis < -1 || plane_axis > 2) MRISR_FAIL(MRISR_E_ARG, "u8_volume_label: plane_axis %d (-1, 0, 1 or 2)", plane_axis);
    if (invert != 0 && invert != 1) MRISR_FAIL(MRISR_E_ARG, "u8_volume_label: invert %d (0 or 1)", invert);
    const int rc = check_shape("u8_volume_label", X, Y, Z);
    if (rc != MRISR_OK) return rc;
    return label_launches<FLAT_PLAIN>("u8_volume_label", mask, X, Y, Z, connectivity, plane_axis, invert, (unsigned*)labels, nullptr,
                                      nullptr, 0, (hipStream_t)stream);
}

extern "C" int mrisr_u8_volume_keep_largest(const uint8_t* mask, int X, int Y, int Z, int connectivity, uint8_t* dst, double* stats3,
                                            void* workspace, void* stream) {
    if (!mask || !dst || !stats3 || !workspace) MRISR_FAIL(MRISR_E_ARG, "u8_volume_keep_largest: null pointer");
    if (!aligned_to(stats3, 8) || !aligned_to(workspace, 16)) MRISR_FAIL(MRISR_E_ARG, "u8_volume_keep_largest: misaligned pointer");
    if (dst == mask) MRISR_FAIL(MRISR_E_ARG, "u8_volume_keep_largest: dst must not be the mask");
    if (connectivity != 6 && connectivity != 26) MRISR_FAIL(MRISR_E_ARG, "u8_volume_keep_largest: connectivity %d (6 or 26)", connectivity);
    const int rc = check_shape("u8_volume_keep_largest", X, Y, Z);
    if (rc != MRISR_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const unsigned n = (unsigned)((size_t)X * Y * Z);
    LabelHeader* hdr = (LabelHeader*)workspace;
    unsigned* labels = (unsigned*)(hdr + 1);
    unsigned* sizes = labels + n;
    const int rc2 = label_launches<FLAT_SIZES>("u8_volume_keep_largest", mask, X, Y, Z, connectivity, -1, 0, labels, sizes,
                                               (unsigned long long*)hdr, 2, s);
    if (rc2 != MRISR_OK) return rc2;
    unsigned long long blocks = ((unsigned long long)n + 4095) / 4096;      // 16 voxels per thread and grid-stride step
    if (blocks > 65536) blocks = 65536;
    label_largest_kernel<<<(unsigned)blocks, 256, 0, s>>>(labels, sizes, n, hdr);
    MRISR_CHECK_LAUNCH("u8_volume_keep_largest (largest)");
    label_select_kernel<<<(unsigned)(((unsigned long long)n + 1023) / 1024), 256, 0, s>>>(labels, n, hdr, aligned_to(dst, 4) ? 1 : 0, dst, stats3);
    MRISR_CHECK_LAUNCH("u8_volume_keep_largest (select)");
    return MRISR_OK;
}

extern "C" int mrisr_u8_volume_fill_holes(const uint8_t* mask, int X, int Y, int Z, int plane_axis, uint8_t* dst, double* stats1,
                                          void* workspace, void* stream) {
    if (!mask || !dst || !stats1 || !workspace) MRISR_FAIL(MRISR_E_ARG, "u8_volume_fill_holes: null pointer");
    if (!aligned_to(stats1, 8) || !aligned_to(workspace, 16)) MRISR_FAIL(MRISR_E_ARG, "u8_volume_fill_holes: misaligned pointer");
    if (dst == mask) MRISR_FAIL(MRISR_E_ARG, "u8_volume_fill_holes: dst must not be the mask");
    if (plane_axis < -1 || plane_axis > 2) MRISR_FAIL(MRISR_E_ARG, "u8_volume_fill_holes: plane_axis %d (-1, 0, 1 or 2)", plane_axis);
    const int rc = check_shape("u8_volume_fill_holes", X, Y, Z);
    if (rc != MRISR_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const unsigned n = (unsigned)((size_t)X * Y * Z);
    unsigned* labels = (unsigned*)((LabelHeader*)workspace + 1);
    unsigned* touches = labels + n;
    const int rc2 = label_launches<FLAT_BORDER>("u8_volume_fill_holes", mask, X, Y, Z, 6, plane_axis, 1, labels, touches,
                                                (unsigned long long*)stats1, 1, s);
    if (rc2 != MRISR_OK) return rc2;
    label_fill_kernel<<<(unsigned)(((unsigned long long)n + 1023) / 1024), 256, 0, s>>>(mask, labels, touches, n, aligned_to(dst, 4) ? 1 : 0, dst,
                                                                                       stats1);
    MRISR_CHECK_LAUNCH("u8_volume_fill_holes (fill)");
    return MRISR_OK;
}
