// Weight packers of the convolution kernels: fp32 master weights -> the LDS images the kernels read.
#include "conv_common.h"
#include "conv_upadj.h"

// Weight packer: fp32 [Cout][k][k][Cin] -> sequence of LDS images [cout block][cin chunk][tap][BN][64 B]
// (swizzled exactly as the kernel reads them).  transpose_flip: the dgrad operand, i.e. the image of
// W'[ci][2-r][2-s][co] with the roles of Cin and Cout exchanged.
template <typename T>
__global__ void pack_weights_kernel(const float* __restrict__ w, T* __restrict__ out, int Cout, int Cin,
                                    int KS, int flip, int BN, int ncb, int nchunks) {
    constexpr int BK = kRowBytes / (int)sizeof(T);
    const int ntaps = KS * KS;
    const size_t total = (size_t)ncb * nchunks * ntaps * BN * BK;
    const int Co = flip ? Cin : Cout, Ci = flip ? Cout : Cin;   // logical (output, input) of the image
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
        size_t r = idx;
        const int e = r % BK; r /= BK;          // position inside the 64-B row (after swizzle)
        const int row = r % BN; r /= BN;
        const int tap = r % ntaps; r /= ntaps;
        const int kc = r % nchunks;
        const int cb = r / nchunks;
        constexpr int EPC = 16 / (int)sizeof(T);         // elements per 16-B chunk
        const int q = tap * BN + row;
        const int chunk_pos = e / EPC, chunk = chunk_pos ^ ((q >> 2) & 3);
        const int k = kc * BK + chunk * EPC + (e % EPC);  // logical input channel
        const int co = cb * BN + row;
        float v = 0.f;
        if (co < Co && k < Ci) {
            if (!flip) v = w[((size_t)co * ntaps + tap) * Cin + k];
            else v = w[((size_t)k * ntaps + (ntaps - 1 - tap)) * Cin + co];   // W[k][mirrored tap][co]
        }
        out[idx] = from_f32<T>(v);
    }
}

// All layers of a model in one launch (the optimiser rewrites every master weight each step): blockIdx.y = job.
// Thread = one 16-byte chunk of a packed image (EPC consecutive input channels of one (tap, output channel) row): the index
// arithmetic is paid once per chunk, the fp32 masters are read as EPC consecutive floats (forward operand) or EPC floats
// one output-channel row apart (mirrored input-gradient operand), the chunk is stored with one 16-byte store.
// (one thread per ELEMENT with five integer divisions each ran at 1 TB/s: 62 us per training step.)
struct PackJobDev { const float* w; void* packed; int Cout, Cin, ksize, flip; };
template <typename T>
__global__ void pack_weights_batched_kernel(const PackJobDev* __restrict__ jobs) {
    constexpr int BK = kRowBytes / (int)sizeof(T);
    constexpr int EPC = 16 / (int)sizeof(T);         // elements per 16-B chunk
    const PackJobDev j = jobs[blockIdx.y];
    const int KS = j.ksize, ntaps = KS * KS, Cin = j.Cin, Cout = j.Cout, flip = j.flip & 1;
    const int Co = flip ? Cin : Cout, Ci = flip ? Cout : Cin;   // logical (output, input) of the image
    const float* __restrict__ w = j.w;
    // source element of (output channel co, tap, input channel k) of the image: forward W[co][tap][k], mirrored W[k][ntaps-1-tap][co]
    auto gather = [&](int co, int tap, int k0, Vec16<T>& v) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const int k = k0 + e;
            float x = 0.f;
            if (co < Co && k < Ci) x = !flip ? w[((size_t)co * ntaps + tap) * Cin + k] : w[((size_t)k * ntaps + (ntaps - 1 - tap)) * Cin + co];
            v.set(e, x);
        }
    };
    if (j.flip & MRISR_PACK_UPADJ) {
        // W^T image of the low-resolution input gradient of bilinear x2 + conv (conv_upadj.hip): [Cin][RS] rows of
        // k = tap * Cout + co, element W[co][tap][ci]; zero past k = 9 Cout (the GEMM's K padding and the row padding)
        if (!conv_upadj_image_bytes(TypeTraits<T>::kDtype, Cout, Cin, KS)) return;
        const int RS = upadj_rs(Cout), K9 = ntaps * Cout;
        const size_t nchunk = (size_t)Cin * RS / EPC;
        for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < nchunk; idx += (size_t)gridDim.x * blockDim.x) {
            const int ci = (int)(idx * EPC / RS), k0 = (int)(idx * EPC % RS);
            Vec16<T> v;
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const int k = k0 + e;
                v.set(e, k < K9 ? w[((size_t)(k % Cout) * ntaps + k / Cout) * Cin + ci] : 0.f);
            }
            store_vec16((T*)j.packed + idx * EPC, v);
        }
        return;
    }
    if (j.flip & MRISR_PACK_RING) {
        // ring layout (conv_ring.hip): [cout block][cin chunk of 16][tap][BN rows][32 B]; the 16-B slot s of row r sits at
        // position s ^ ((r >> 3) & 1), so that a row fragment reads conflict-free and a DMA piece is a linear copy
        const int RBN = conv_ring_bn(TypeTraits<T>::kDtype, Co, Ci, KS);
        if (RBN == 0) return;
        const int rnch = Ci / 16;
        const size_t nchunk = (size_t)(Co / RBN) * rnch * ntaps * RBN * 2;      // 16-B chunks (8 elements of a 16-bit type)
        for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < nchunk; idx += (size_t)gridDim.x * blockDim.x) {
            size_t r = idx;
            const int pos = r & 1; r >>= 1;
            const int row = r % RBN; r /= RBN;
            const int tap = r % ntaps; r /= ntaps;
            const int kc = r % rnch;
            const int cb = r / rnch;
            const int slot = pos ^ ((row >> 3) & 1);
            Vec16<T> v;
            gather(cb * RBN + row, tap, kc * 16 + slot * 8, v);
            store_vec16((T*)j.packed + idx * EPC, v);
        }
        return;
    }
    const int BN = Co >= 64 ? 64 : 32;                          // conv_choose_bn
    const int ncb = (Co + BN - 1) / BN, nchunks = (Ci + BK - 1) / BK;
    const size_t nchunk = (size_t)ncb * nchunks * ntaps * BN * 4;     // four 16-B chunks per 64-B row
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < nchunk; idx += (size_t)gridDim.x * blockDim.x) {
        size_t r = idx;
        const int pos = r & 3; r >>= 2;            // chunk position inside the row (after the swizzle)
        const int row = r % BN; r /= BN;
        const int tap = r % ntaps; r /= ntaps;
        const int kc = r % nchunks;
        const int cb = r / nchunks;
        const int q = tap * BN + row;
        const int chunk = pos ^ ((q >> 2) & 3);
        Vec16<T> v;
        gather(cb * BN + row, tap, kc * BK + chunk * EPC, v);
        store_vec16((T*)j.packed + idx * EPC, v);
    }
}

extern "C" int mrisr_pack_weights_batched(int dtype, const mrisr_pack_job* jobs_device, int njobs, void* stream) {
    static_assert(sizeof(PackJobDev) == sizeof(mrisr_pack_job), "mrisr_pack_job layout");
    if (!jobs_device || njobs <= 0 || njobs > 65535) MRISR_FAIL(MRISR_E_ARG, "pack_weights_batched: bad job table");
    dim3 grid(256, njobs);     // small jobs leave their surplus blocks immediately; the largest image decides the time
    if (dtype == MRISR_BF16)
        pack_weights_batched_kernel<bf16_t><<<grid, 256, 0, (hipStream_t)stream>>>((const PackJobDev*)jobs_device);
    else if (dtype == MRISR_F16)
        pack_weights_batched_kernel<f16_t><<<grid, 256, 0, (hipStream_t)stream>>>((const PackJobDev*)jobs_device);
    else if (dtype == MRISR_F32)
        pack_weights_batched_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>((const PackJobDev*)jobs_device);
    else
        MRISR_FAIL(MRISR_E_DTYPE, "pack_weights_batched: dtype %d", dtype);
    MRISR_CHECK_LAUNCH("pack_weights_batched");
    return MRISR_OK;
}

extern "C" size_t mrisr_packed_weight_bytes(int dtype, int Cout, int Cin, int ksize) {
    const int BN = conv_choose_bn(Cout), BK = conv_bk(dtype);
    const size_t ncb = ceil_div(Cout, BN), nch = ceil_div(Cin, BK);
    return ncb * nch * (size_t)(ksize * ksize) * BN * kRowBytes;
}

extern "C" int mrisr_pack_weights(int dtype, const float* w, int Cout, int Cin, int ksize, int transpose_flip,
                                  void* packed, void* stream) {
    if (!w || !packed) MRISR_FAIL(MRISR_E_ARG, "pack_weights: null pointer");
    if (ksize != 1 && ksize != 3) MRISR_FAIL(MRISR_E_UNSUPPORTED, "pack_weights: ksize %d", ksize);
    if (transpose_flip & (MRISR_PACK_RING | MRISR_PACK_UPADJ)) {
        const int flip = transpose_flip & 1;
        if ((transpose_flip & MRISR_PACK_UPADJ) && !conv_upadj_image_bytes(dtype, Cout, Cin, ksize))
            MRISR_FAIL(MRISR_E_UNSUPPORTED, "pack_weights: no upadj layout for %d -> %d k%d dtype %d", Cin, Cout, ksize, dtype);
        if (!(transpose_flip & MRISR_PACK_UPADJ) && !mrisr_conv_ring_bn(dtype, flip ? Cin : Cout, flip ? Cout : Cin, ksize))
            MRISR_FAIL(MRISR_E_UNSUPPORTED, "pack_weights: no ring layout for %d -> %d k%d dtype %d", Cin, Cout, ksize, dtype);
        const PackJobDev job{w, packed, Cout, Cin, ksize, transpose_flip};
        PackJobDev* dj = nullptr;      // (stand-alone packing is a test / tool path: the training step uses the batched entry)
        if (hipMalloc(&dj, sizeof(job)) != hipSuccess) MRISR_FAIL(MRISR_E_HIP, "pack_weights: hipMalloc");
        (void)hipMemcpyAsync(dj, &job, sizeof(job), hipMemcpyHostToDevice, (hipStream_t)stream);
        const int rc = mrisr_pack_weights_batched(dtype, (const mrisr_pack_job*)dj, 1, stream);
        (void)hipStreamSynchronize((hipStream_t)stream);
        (void)hipFree(dj);
        return rc;
    }
    transpose_flip &= 1;
    const int Co = transpose_flip ? Cin : Cout, Ci = transpose_flip ? Cout : Cin;
    const int BN = conv_choose_bn(Co), BK = conv_bk(dtype);
    const int ncb = ceil_div(Co, BN), nch = ceil_div(Ci, BK);
    const size_t total = (size_t)ncb * nch * ksize * ksize * BN * BK;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    if (dtype == MRISR_BF16)
        pack_weights_kernel<bf16_t><<<blocks, 256, 0, (hipStream_t)stream>>>(w, (bf16_t*)packed, Cout, Cin, ksize,
                                                                            transpose_flip, BN, ncb, nch);
    else if (dtype == MRISR_F16)
        pack_weights_kernel<f16_t><<<blocks, 256, 0, (hipStream_t)stream>>>(w, (f16_t*)packed, Cout, Cin, ksize,
                                                                           transpose_flip, BN, ncb, nch);
    else if (dtype == MRISR_F32)
        pack_weights_kernel<float><<<blocks, 256, 0, (hipStream_t)stream>>>(w, (float*)packed, Cout, Cin, ksize,
                                                                           transpose_flip, BN, ncb, nch);
    else
        MRISR_FAIL(MRISR_E_DTYPE, "pack_weights: dtype %d", dtype);
    MRISR_CHECK_LAUNCH("pack_weights");
    return MRISR_OK;
}
