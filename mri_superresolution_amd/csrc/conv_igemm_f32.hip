// Classic implicit-GEMM convolution, f32 storage: instantiates and launches conv_igemm_kernel<float, ...>.
#include "conv_igemm.h"

int launch_conv_igemm_f32(ConvParams& p, int bn, int spatial, int ks, hipStream_t s) {
    return bn == 64 ? dispatch_conv_sp<float, 64>(p, spatial, ks, s) : dispatch_conv_sp<float, 32>(p, spatial, ks, s);
}
#ifdef MRISR_PHASE_TIMING
int conv_igemm_phase_f32(unsigned long long* out96) { return conv_igemm_phase(out96); }
#endif
