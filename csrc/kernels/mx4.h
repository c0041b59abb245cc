// OCP Microscaling FP4 on the device (wquant.hip, gemv.hip): a 16-byte chunk
// is one MX block, 32 E2M1 weights (element 2i in bits 3:0 of byte i, element
// 2i+1 in bits 7:4) under one E8M0 scale byte.  The quantiser never writes
// bytes 0 or 255, so the fp32 scale is always the byte moved into the
// exponent field.
#pragma once
#include "common.h"

namespace lsd {

typedef __bf16 mx4_pair __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float mx4_scale(unsigned int e8m0) { return __builtin_bit_cast(float, e8m0 << 23); }

// The GEMV's LDS activation image under MXFP4 weights (gemv.hip has the bank
// argument): 16-byte chunk u of a row is stored at chunk (u & ~3) | ((u ^ (u >> 4)) & 3),
// i.e. the four chunks of block c = u >> 2 are permuted by XOR with (c >> 2) & 3.
__device__ __forceinline__ int mx4_swz(int u) { return (u & ~3) | ((u ^ (u >> 4)) & 3); }

// 16 bytes x scale -> the block's 16 dequantised bf16 pairs: pair 4 d + s is
// elements 8 d + 2 s, 8 d + 2 s + 1 (byte s of dword d).  v_cvt_scalef32_pk_bf16_fp4
// multiplies by the scale in the convert; e2m1 x 2^X is exact in bf16.
__device__ __forceinline__ void mx4_cvt32(u32x4 w, float scale, mx4_pair (&o)[16]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    o[4 * d + 0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[d], scale, 0);
    o[4 * d + 1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[d], scale, 1);
    o[4 * d + 2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[d], scale, 2);
    o[4 * d + 3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[d], scale, 3);
  }
}

}  // namespace lsd
