// The in-launch split-K combine of the GEMM kernels (gemm_sk, gemm_ring8 VAR 2,
// gemm_d256 in gemm.hip; gemm_w8, gemm_w8_d256 in gemm_w8.hip), once.  Every
// split of a tile publishes its raw fp32 partial tile, takes a ticket, and the
// last arriver sums all S partials and goes on to the fused epilogue: any
// epilogue works with any split count, in one launch (guide §5 "In-launch
// split-K reduction").
//  * Slab layout.  Tile `tile` owns S slabs of NA * NB * THREADS f32x4;
//    accumulator (a, b) of a thread lies at base + (a * NB + b) * STRIDE bytes
//    of its split's slab.  `base` and STRIDE are the caller's, lane-major: a
//    wave moves 64 consecutive 16-byte vectors, whole lines per access.
//  * sc1, no fence.  Stores are write-through (sc1) and every reducer load is
//    sc1, so they meet in memory all XCDs share and no agent-scope release /
//    acquire fence is needed (a buffer_wbl2 release per workgroup cost ~5 us
//    in gemm_sk_kernel): each thread drains its stores (vmcnt(0)), the barrier
//    collects the workgroup's, then thread 0 takes the relaxed agent ticket.
//  * Ticket.  The last arriver (ticket S - 1) re-arms the counter for the next
//    launch; the others leave on the flag in LDS.
//  * All S partials are re-read, the last arriver's own included: no per-load
//    register-or-load select, one code path whoever arrives last.
//  * Clamped index x 0/1 mask.  The loads of a group of RG splits are all
//    issued before the first add: one round trip per group, not per split.  A
//    runtime "if (s < S) load" makes the compiler branch around each load and
//    wait for it alone (guide §5 trap (c)), so splits past S re-load slab
//    S - 1 times 0.  RG bounds the VGPRs in flight: RG * NA * NB * 4.
//  * Fixed order.  Splits are summed 0 .. S - 1, whichever arrived last.
// Workspace contract: plan_gemm() (gemm_plan.h) sizes the workspace as
// combine_tiles * splits * GemmPlan::tile_floats, and tile_floats must equal
// 4 * NA * NB * THREADS: 16 * mt * 64 * nw (sk, w8: [MT][NW] x 256), 256 * tn
// (d256: [2][tn / 16], w8_d256: [4][tn / 32], x 512), 128 * 64 (ring8: [2][2] x 512).
#pragma once
#include "common.h"

namespace lsd {

// Returns true in the last-arriving workgroup, with the S-way sum in `acc`;
// false in every other one, which has nothing left to do.  All THREADS threads
// call it; s_flag is a word of LDS nobody else uses until it returns.
// Barriers are block_sync(): the FP8 kernels are built without packed fp32 ops.
template <int THREADS, int STRIDE, int RG, int NA, int NB>
__device__ __forceinline__ bool splitk_combine(f32x4 (&acc)[NA][NB], float* ws, int* cnt, int tile, int split, int S,
                                               int base, int* s_flag) {
  constexpr int PER = NA * NB * THREADS;  // f32x4 per split slab
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(ws + (long)tile * S * PER * 4, (short)0, S * PER * 16, 0x00020000);
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[a][b]), rs,
                                             split * PER * 16 + base + (a * NB + b) * STRIDE, 0, 16);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  block_sync();
  if (threadIdx.x == 0) {
    const int t = __hip_atomic_fetch_add(cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_flag = (t == S - 1);
    if (t == S - 1) __hip_atomic_store(cnt + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  block_sync();
  if (*s_flag == 0) return false;
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s0 = 0; s0 < S; s0 += RG) {
    f32x4 v[RG][NA][NB];
#pragma unroll
    for (int u = 0; u < RG; ++u) {
      const int s2 = min(s0 + u, S - 1);
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
          v[u][a][b] = __builtin_bit_cast(
              f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, s2 * PER * 16 + base + (a * NB + b) * STRIDE, 0, 16));
    }
#pragma unroll
    for (int u = 0; u < RG; ++u) {
      const float msk = (s0 + u < S) ? 1.f : 0.f;
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] += v[u][a][b] * msk;
    }
  }
  return true;
}

}  // namespace lsd
