// The 8-logit segment of the mask passes ahead of the sampler (allow_mask.hip,
// guide.hip): one mask byte is one segment, linear_f32's segmax granule.
#pragma once
#include "common.h"

namespace lsd {

template <bool VEC>
__device__ __forceinline__ void allow_load8(const float* p, float (&x)[8]) {
  if constexpr (VEC) {
    const f32x4 a = reinterpret_cast<const f32x4*>(p)[0], b = reinterpret_cast<const f32x4*>(p)[1];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = a[i], x[4 + i] = b[i];
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = p[i];
  }
}

// One whole segment whose byte m has a clear bit: m == 0 stores eight -inf
// without x; a mixed m selects from x (the segment as loaded), stores what
// changed and takes the maximum from the registers.
template <bool VEC>
__device__ __forceinline__ void allow_put8(float* p, float* sm, unsigned m, float (&x)[8]) {
  const float ninf = -__builtin_inff();
  if (m == 0) {
    if constexpr (VEC) {
      const f32x4 z = {ninf, ninf, ninf, ninf};
      reinterpret_cast<f32x4*>(p)[0] = z;
      reinterpret_cast<f32x4*>(p)[1] = z;
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) p[i] = ninf;
    }
    if (sm) *sm = ninf;
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = (m >> i) & 1u ? x[i] : ninf;
  if constexpr (VEC) {
    // a half without a cleared bit is not stored
    if ((m & 0xFu) != 0xFu) reinterpret_cast<f32x4*>(p)[0] = f32x4{x[0], x[1], x[2], x[3]};
    if ((m & 0xF0u) != 0xF0u) reinterpret_cast<f32x4*>(p)[1] = f32x4{x[4], x[5], x[6], x[7]};
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (!((m >> i) & 1u)) p[i] = ninf;
  }
  if (sm) {
    float mx = x[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) mx = fmaxf(mx, x[i]);
    *sm = mx;
  }
}

}  // namespace lsd
