// HF-style repetition_penalty and no_repeat_ngram_size of the on-device
// sampler (CDNA4): the two rules that read the prompt.
//
// The last stage keeps, per KV slot, the context of the sequence on it:
//   plen[slot]    prompt tokens (int32 [slots])
//   rpen[slot]    repetition_penalty r (fp32 [slots]; 1 = off)
//   ngram[slot]   no_repeat_ngram_size G (int32 [slots]; 0 = off)
//   tok[slot, j]  prompt tokens [0, plen), then the generated ones: the token
//                 of the draw with sampler counter c at plen + c (int32
//                 [slots, L])
// Before the draw of a row with counter c (step[row], read before the sampler
// advances it; step null = draw 0) the context is x = tok[slot, 0 .. n), n =
// min(plen + c, L), and -- ahead of the penalty pass, the logit edits and the
// sampler --
//   1. r != 1: every distinct token t of x in [0, V) is rewritten once:
//      logit[t] <- logit[t] * r if logit[t] < 0 else logit[t] / r, one fp32
//      rounding, IEEE division (this file is built without fast-math);
//   2. G > 0, n >= G - 1: with tail = x[n - G + 1 .. n), every i in [0, n - G]
//      with x[i .. i + G - 1) == tail bans the token that followed:
//      logit[x[i + G - 1]] <- -inf when it is in [0, V)
// bit-equal to ops/reference.py repetition.
//
//   repeat_kernel          one workgroup of 256 threads per row.  Rows whose
//                          slot has r == 1 and G == 0 (default rows, every pad
//                          row: the scratch slot keeps the defaults) return at
//                          once, uniformly.  Distinct tokens go through an
//                          open-addressing LDS key set (atomicCAS): the thread
//                          whose insert wins rewrites the logit, so no logit is
//                          rewritten twice and the result does not depend on
//                          arrival order; with r == 1 the set is skipped.
//                          After a block barrier -- a token can be penalised
//                          and banned, the ban comes last -- thread tid takes
//                          the start positions i = tid + 256 k of the n-gram
//                          scan against the tail in LDS.  Then, after a fence
//                          and a barrier, since two rewritten tokens can share
//                          a segment, the maximum of every 8-logit segment
//                          holding one is recomputed from its 8 stored logits
//                          (linear_f32's segmax, which the sampler's fast path
//                          trusts), padding columns included, as
//                          penalize_kernel does.
//   record_context_kernel  tok[slots[i], plen[slots[i]] + step[i] - back] =
//                          tokens[i] for active rows, after the draw.
//
// LDS budget: tbl = 2^k >= 2 L keys of 4 bytes (load <= 1/2, so linear
// probing always ends) plus a 32-word tail: L = 1024 (GPT-2) 8 KB, L = 8192
// (Llama-3) 64 KB + 128 B of the CU's 160 KB; a longer context is refused by
// the host wrapper.  A row clears and probes only the 2^j >= 2 n keys it
// needs.  L <= 8192 also bounds a thread's scan to 32 start positions, which
// it remembers in a 32-bit mask across the barrier.
#include "common.h"

namespace lsd {

constexpr int REP_NT = 256;
constexpr int REP_MAX_L = 8192;
constexpr int REP_MAX_G = 32;

__device__ __forceinline__ unsigned rep_hash(int t, int shift) {
  return ((unsigned)t * 2654435761u) >> shift;
}

// the maximum of segment s of the row, from its 8 stored logits
__device__ __forceinline__ void rep_segment(float* lg, float* sm, int s) {
  // volatile: written by other threads of this block (lg is __restrict__ in the kernel)
  const volatile float* q = lg + 8 * (long)s;
  float m = q[0];
#pragma unroll
  for (int e = 1; e < 8; ++e) m = fmaxf(m, q[e]);
  sm[s] = m;  // tokens sharing the segment store the same value
}

__global__ __launch_bounds__(REP_NT) void repeat_kernel(float* __restrict__ logits, long ld, int V,
                                                        const int* __restrict__ plen,
                                                        const float* __restrict__ rpen,
                                                        const int* __restrict__ ngram,
                                                        const int* __restrict__ tok, int L, int nslots,
                                                        const int* __restrict__ slots,
                                                        const long long* __restrict__ step,
                                                        float* __restrict__ segmax, long ldseg, int tbl_max) {
  extern __shared__ int rep_lds[];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int slot = slots[row];
  if (slot < 0 || slot >= nslots) return;  // uniform
  const float r = rpen[slot];
  int G = ngram[slot];
  if (r == 1.f && G <= 0) return;  // uniform: default and pad rows
  if (G > REP_MAX_G) G = REP_MAX_G;
  const long long c = step ? step[row] : 0;
  long long n64 = (long long)plen[slot] + c;
  if (n64 > (long long)L) n64 = L;
  const int n = (int)n64;
  if (n <= 0) return;  // uniform: an empty context rewrites and bans nothing
  const bool pen = r != 1.f;
  // key set of this row: the smallest power of two >= 2 n (>= 64), <= tbl_max
  int bits = 6;
  while ((1 << bits) < 2 * n) ++bits;
  const int tbl = 1 << bits;
  if (tbl > tbl_max) return;  // cannot happen: the host sizes tbl_max >= 2 L
  const int shift = 32 - bits, mask = tbl - 1;
  int* keys = rep_lds;
  int* tail = rep_lds + tbl_max;
  const int* x = tok + (long)slot * L;
  float* lg = logits + (long)row * ld;
  const bool scan = G > 0 && n >= G;  // n == G - 1: a tail, but no start position
  if (pen)
    for (int i = tid; i < tbl; i += REP_NT) keys[i] = -1;
  if (scan && tid < G - 1) tail[tid] = x[n - G + 1 + tid];
  __syncthreads();
  if (pen) {
    for (int j = tid; j < n; j += REP_NT) {
      const int t = x[j];
      if (t < 0 || t >= V) continue;
      unsigned i = rep_hash(t, shift);
      for (;;) {
        const int prev = atomicCAS(&keys[i], -1, t);
        if (prev == -1) {  // this thread inserted t: the one rewrite
          const float l = lg[t];
          lg[t] = l < 0.f ? l * r : l / r;
          break;
        }
        if (prev == t) break;
        i = (i + 1) & mask;
      }
    }
    // the bans below may hit a token rewritten above by another thread
    __threadfence_block();
    __syncthreads();
  }
  unsigned banned = 0;  // bit k: this thread's k-th start position banned a token
  if (scan) {
    int k = 0;
    for (int i = tid; i <= n - G; i += REP_NT, ++k) {
      bool eq = true;
      for (int j = 0; j < G - 1; ++j) {
        if (x[i + j] != tail[j]) {
          eq = false;
          break;
        }
      }
      if (!eq) continue;
      const int t = x[i + G - 1];
      if (t < 0 || t >= V) continue;
      lg[t] = -INFINITY;
      banned |= 1u << k;
    }
  }
  if (segmax == nullptr) return;  // uniform
  // every logit write of the row before any segment is read back
  __threadfence_block();
  __syncthreads();
  float* sm = segmax + (long)row * ldseg;
  if (pen) {
    for (int i = tid; i < tbl; i += REP_NT) {
      const int t = keys[i];
      if (t >= 0) rep_segment(lg, sm, t >> 3);
    }
  }
  for (int k = 0; banned != 0; ++k, banned >>= 1)
    if (banned & 1u) rep_segment(lg, sm, x[tid + k * REP_NT + G - 1] >> 3);
}

__global__ __launch_bounds__(256) void record_context_kernel(int* __restrict__ tok, int L, int nslots,
                                                             const int* __restrict__ plen,
                                                             const int* __restrict__ slots,
                                                             const long long* __restrict__ step, int back,
                                                             const int* __restrict__ tokens,
                                                             const int* __restrict__ active, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  if (active != nullptr && active[i] == 0) return;
  const int slot = slots[i];
  if (slot < 0 || slot >= nslots) return;
  const long long j = (long long)plen[slot] + (step ? step[i] - back : 0);
  if (j < 0 || j >= L) return;
  tok[(long)slot * L + j] = tokens[i];
}

}  // namespace lsd

// logits [B, ld] fp32 (V <= ld); plen / rpen / ngram [nslots], tok [nslots, L];
// slots [B]; step null = draw 0; segmax null or [B, ldseg] with ldseg >= ld / 8
// (then ld % 8 == 0).
extern "C" hipError_t lsd_repeat_penalty(float* logits, long ld, int B, int V, const int* plen, const float* rpen,
                                         const int* ngram, const int* tok, int L, int nslots, const int* slots,
                                         const long long* step, float* segmax, long ldseg, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (L <= 0 || L > lsd::REP_MAX_L || nslots <= 0 || V > ld ||
      (segmax != nullptr && (ld % 8 != 0 || ldseg * 8 < ld)))
    return hipErrorInvalidValue;
  int tbl = 64;
  while (tbl < 2 * L) tbl <<= 1;
  const size_t lds = ((size_t)tbl + lsd::REP_MAX_G) * sizeof(int);
  if (lds > 64 * 1024) {
    // more than the default 64 KB of dynamic LDS: raised once per device (to
    // the largest key set plus the tail), on the first such launch -- an eager
    // one, the engine runs a new decode bucket once before capturing it
    static bool raised[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !raised[dev]) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(lsd::repeat_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (2 * lsd::REP_MAX_L + lsd::REP_MAX_G) * (int)sizeof(int));
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < 64) raised[dev] = true;
    }
  }
  hipLaunchKernelGGL(lsd::repeat_kernel, dim3(B), dim3(lsd::REP_NT), lds, st, logits, ld, V, plen, rpen, ngram, tok,
                     L, nslots, slots, step, segmax, ldseg, tbl);
  return hipGetLastError();
}

// back = 1 when `step` was already advanced by the sampler (sample_into), so
// the entry written is the one of the counter the draw used; step null = draw 0.
extern "C" hipError_t lsd_record_context(int* tok, int L, int nslots, const int* plen, const int* slots,
                                         const long long* step, int back, const int* tokens, const int* active,
                                         int B, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (L <= 0 || nslots <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lsd::record_context_kernel, dim3((B + 255) / 256), dim3(256), 0, st, tok, L, nslots, plen, slots,
                     step, back, tokens, active, B);
  return hipGetLastError();
}
