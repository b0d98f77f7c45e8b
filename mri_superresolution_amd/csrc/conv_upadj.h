// Shapes of the low-resolution input gradient of bilinear x2 + 3x3 conv (conv_upadj.hip) and of its W^T weight image,
// shared with the weight packer (conv_fwd.hip).
#pragma once
#include "common.h"

// widths the kernel is instantiated for: (Cout, Cin) of the forward conv = (f/2, f), f = 16, 32, 64
__host__ __device__ inline bool conv_upadj_width_ok(int dtype, int Cout, int Cin, int ksize) {
    if ((dtype != MRISR_BF16 && dtype != MRISR_F16) || ksize != 3 || Cin != 2 * Cout) return false;
    return Cout == 8 || Cout == 16 || Cout == 32;
}
// K of the GEMM (9 Cout) padded to the MFMA step, and the row length of the W^T image / the LDS h image (16 bytes of
// padding: the 16 lanes of a ds_read_b128 operand read then start 4 banks apart, conflict-free)
constexpr __host__ __device__ int upadj_kp(int Cout) { return (9 * Cout + 31) / 32 * 32; }
constexpr __host__ __device__ int upadj_rs(int Cout) { return upadj_kp(Cout) + 8; }
// W^T image [Cin][upadj_rs(Cout)] of 16-bit elements: (ci, k = tap * Cout + co) = W[co][tap][ci], zero for k >= 9 Cout
__host__ __device__ inline size_t conv_upadj_image_bytes(int dtype, int Cout, int Cin, int ksize) {
    return conv_upadj_width_ok(dtype, Cout, Cin, ksize) ? (size_t)Cin * upadj_rs(Cout) * 2 : 0;
}
