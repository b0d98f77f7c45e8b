// Classic implicit-GEMM convolution, bf16 storage: instantiates and launches conv_igemm_kernel<bf16_t, ...>.
#include "conv_igemm.h"

int launch_conv_igemm_bf16(ConvParams& p, int bn, int spatial, int ks, hipStream_t s) {
    return bn == 64 ? dispatch_conv_sp<bf16_t, 64>(p, spatial, ks, s) : dispatch_conv_sp<bf16_t, 32>(p, spatial, ks, s);
}
#ifdef MRISR_PHASE_TIMING
int conv_igemm_phase_bf16(unsigned long long* out96) { return conv_igemm_phase(out96); }
#endif
