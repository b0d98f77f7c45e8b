#include "common.h"
thread_local char g_mrisr_err[512] = "";
extern "C" const char* mrisr_last_error(void) { return g_mrisr_err; }
extern "C" int mrisr_version(void) { return 311; }   // 311: mrisr_f32_volume_{down2,up2,metrics}, mrisr_volume_metrics_finalize;  310: mrisr_f32_volume_up2_blend;  309: mrisr_act_bwd_blend_{ok,reduce,apply}, mrisr_blend_branch;  308: mrisr_resample_taps, mrisr_f32_resample_letterbox, mrisr_lowfield_{dirichlet_any,simulate_f32}; 307: mrisr_f32_percentile_{workspace_bytes,bounds}, mrisr_f32_window_{normalise,restore}; 306: mrisr_lowfield_{dirichlet,workspace_bytes,simulate}; 305: mrisr_conv_upadj, MRISR_PACK_UPADJ; 304: mrisr_{stem,head}_*_multi; 303: mrisr_ssim_l1_{forward,backward}_win; 302: mrisr_act_bwd_onepass(_ok); 301: mrisr_up_conv1x1_fused; 300: mrisr_conv_desc.wpacked_ring, ring weight layout (MRISR_PACK_RING), mrisr_conv_ring_bn
extern "C" int mrisr_stat_slots(void) { return MRISR_STAT_SLOTS; }
