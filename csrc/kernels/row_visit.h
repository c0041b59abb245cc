// Row-visit helpers shared by the kernels that walk one fp32 logit row per
// 1024-thread workgroup: the sampler (sample.hip) and the logprob pass
// (logprob.hip).
#pragma once
#include "common.h"

namespace lsd {

constexpr int NT = 1024;     // threads per row

// Order-preserving key of the radix select.  -0.0 takes +0.0's key: every
// other comparison here (threshold filter, rank selection, bitonic network,
// greedy) is numeric, where the two are equal and the lower index goes first;
// keyed apart, a k boundary among zeros would select the +0.0 entries ahead of
// lower-index -0.0 ones and the radix path would differ from the threshold
// paths on the same row.  Every other input keeps its key.
__device__ __forceinline__ unsigned fkey(float x) {
  unsigned u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Visit every (value, index) of the row in chunks of CH float4 per thread:
// all CH loads of a chunk are issued before the first visit (addresses
// clamped, not guarded, so no load sits behind a branch).  CH = 13 covers a
// GPT-2 row (50257 <= 13 x 4096) in ONE L2 round trip per pass instead of 13
// (one per float4 step of the plain loop: ~54 us per 128-row batch, almost all
// latency); Llama-3's 128 K vocabulary takes 3.  90 VGPRs, no spills.
// The row stride is a multiple of 64 floats, so a float4 never leaves the row.
constexpr int CH = 13;
template <typename F>
__device__ __forceinline__ void for_row(const float* x, int V, F&& f) {
  const int last = ((V - 1) >> 2) << 2;  // last float4 that starts inside the row
  for (int b0 = 0; b0 < V; b0 += CH * NT * 4) {
    f32x4 q[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i)
      q[i] = *reinterpret_cast<const f32x4*>(x + min(b0 + ((int)threadIdx.x + i * NT) * 4, last));
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int b = b0 + ((int)threadIdx.x + i * NT) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (b + j < V) f(q[i][j], b + j);
    }
  }
}

// k-th largest of the 64 16-thread group maxima of mx (ties by group): with
// every group maximum an element of the row (or -inf), a lower bound of the
// row's k-th largest element -- the top-k group maxima are k distinct
// elements >= it.  Two block barriers.
__device__ __forceinline__ float kth_group_max(float mx, int k, float* cval, float* redv) {
  const int tid = threadIdx.x;
  mx = fmaxf(mx, wave_xchg<1>(mx));
  mx = fmaxf(mx, wave_xchg<2>(mx));
  mx = fmaxf(mx, wave_xchg<4>(mx));
  mx = fmaxf(mx, wave_xchg<8>(mx));
  if ((tid & 15) == 0) cval[tid >> 4] = mx;
  __syncthreads();
  if (tid < 64) {  // rank of group `tid` among the 64 maxima
    const float sv = cval[tid];
    int rank = 0;
#pragma unroll
    for (int j4 = 0; j4 < 16; ++j4) {
      const f32x4 o = reinterpret_cast<const f32x4*>(cval)[j4];
#pragma unroll
      for (int e = 0; e < 4; ++e) rank += (o[e] > sv || (o[e] == sv && 4 * j4 + e < tid)) ? 1 : 0;
    }
    if (rank == k - 1) redv[0] = sv;
  }
  __syncthreads();
  return redv[0];
}

// Block-wide slot assignment for `cnt` entries of this thread: wave-inclusive
// scan, one LDS atomic per wave on `s_cnt`; returns the thread's first slot.
__device__ __forceinline__ unsigned claim_slots(int cnt, unsigned* s_cnt) {
  const int lane = lane_id();
  int incl = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  unsigned base = 0;
  if (lane == 63) base = atomicAdd(s_cnt, (unsigned)incl);
  return __shfl(base, 63, 64) + (unsigned)(incl - cnt);
}

}  // namespace lsd
