// Presence / frequency penalties of the on-device sampler (CDNA4).
//
// The last stage keeps, per KV slot, the tokens a sequence has drawn so far:
//   hist[slot, j] = the j-th generated token (int32 [slots, L], j = the
//   sampler counter of the draw; the prompt is not in it).
// Before the draw of a penalised row, with c(t) = occurrences of t in
// hist[slot, 0 .. count):
//   logit[t] <- logit[t] - (presence + frequency * float(c(t)))   for c(t) > 0
// in fp32 with three roundings (product, sum, difference; FMA contraction is
// switched off for this file) -- bit-equal to ops/reference.py penalize, which
// seeded draws rely on.
//
//   penalize_kernel       one workgroup per row.  Rows with presence == 0 and
//                         frequency == 0 (every pad row) or an empty history
//                         return at once, uniformly.  Otherwise the history is
//                         counted in an open-addressing LDS table (key =
//                         token, integer count; atomicCAS / atomicAdd, so the
//                         result does not depend on arrival order), each
//                         distinct token's logit is rewritten once, and --
//                         after a block barrier, since two history tokens can
//                         share a segment -- the maximum of every touched
//                         8-logit segment is recomputed from its 8 stored
//                         logits (linear_f32's segmax, which the sampler's
//                         fast path trusts).
//   record_tokens_kernel  hist[slots[i], step[i] - back] = tokens[i] for
//                         active rows, after the draw.
//
// LDS budget: the table has tbl = 2^k >= 2 * L slots of 8 bytes (load <= 1/2,
// so linear probing always ends): L = 1024 (GPT-2) 16 KB, L = 4096 64 KB,
// L = 8192 (Llama-3) 128 KB of the CU's 160 KB; a longer history is refused by
// the host wrapper.  A row clears and probes only the 2^j >= 2 * count slots
// it needs.
#include "common.h"

// hipcc contracts a + b * c into one FMA by default, and through the inlined
// __fmul_rn / __fadd_rn too (their bodies carry the header's contraction
// flag): plain operators with contraction off keep the three roundings.
#pragma clang fp contract(off)

namespace lsd {

constexpr int PEN_NT = 256;

__device__ __forceinline__ unsigned pen_hash(int t, int shift) {
  return ((unsigned)t * 2654435761u) >> shift;
}

__global__ __launch_bounds__(PEN_NT) void penalize_kernel(float* __restrict__ logits, long ld, int V,
                                                          const int* __restrict__ hist, int L, int nslots,
                                                          const int* __restrict__ slots,
                                                          const long long* __restrict__ counts,
                                                          const float* __restrict__ presence,
                                                          const float* __restrict__ frequency,
                                                          float* __restrict__ segmax, long ldseg, int tbl_max) {
  extern __shared__ int pen_lds[];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float pres = presence[row], freq = frequency[row];
  if (pres == 0.f && freq == 0.f) return;  // uniform: default and pad rows
  const long long cnt64 = counts ? counts[row] : 0;
  const int n = (int)(cnt64 < (long long)L ? cnt64 : (long long)L);
  const int slot = slots[row];
  if (n <= 0 || slot < 0 || slot >= nslots) return;  // uniform
  // table of this row: the smallest power of two >= 2 n (>= 64), <= tbl_max
  int bits = 6;
  while ((1 << bits) < 2 * n) ++bits;
  int tbl = 1 << bits;
  if (tbl > tbl_max) return;  // cannot happen: the host sizes tbl_max >= 2 L
  const int shift = 32 - bits, mask = tbl - 1;
  int* keys = pen_lds;
  int* cnts = pen_lds + tbl_max;
  for (int i = tid; i < tbl; i += PEN_NT) {
    keys[i] = -1;
    cnts[i] = 0;
  }
  __syncthreads();
  const int* h = hist + (long)slot * L;
  for (int j = tid; j < n; j += PEN_NT) {
    const int t = h[j];
    if (t < 0 || t >= V) continue;
    unsigned i = pen_hash(t, shift);
    for (;;) {
      const int prev = atomicCAS(&keys[i], -1, t);
      if (prev == -1 || prev == t) {
        atomicAdd(&cnts[i], 1);
        break;
      }
      i = (i + 1) & mask;
    }
  }
  __syncthreads();
  float* lg = logits + (long)row * ld;
  for (int i = tid; i < tbl; i += PEN_NT) {
    const int t = keys[i];
    if (t < 0) continue;
    const float prod = freq * (float)cnts[i];  // three roundings: contraction is off (above)
    const float pen = pres + prod;
    lg[t] = lg[t] - pen;
  }
  if (segmax == nullptr) return;  // uniform
  // every logit write of the row before any segment is read back
  __threadfence_block();
  __syncthreads();
  float* sm = segmax + (long)row * ldseg;
  for (int i = tid; i < tbl; i += PEN_NT) {
    const int t = keys[i];
    if (t < 0) continue;
    const int s = t >> 3;
    // volatile: written above by other threads of this block (lg is __restrict__)
    const volatile float* q = lg + 8 * (long)s;
    float m = q[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) m = fmaxf(m, q[e]);
    sm[s] = m;  // tokens sharing the segment store the same value
  }
}

__global__ __launch_bounds__(256) void record_tokens_kernel(int* __restrict__ hist, int L, int nslots,
                                                            const int* __restrict__ slots,
                                                            const long long* __restrict__ step, int back,
                                                            const int* __restrict__ tokens,
                                                            const int* __restrict__ active, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  if (active != nullptr && active[i] == 0) return;
  const long long j = step ? step[i] - back : 0;
  const int slot = slots[i];
  if (j < 0 || j >= L || slot < 0 || slot >= nslots) return;
  hist[(long)slot * L + j] = tokens[i];
}

}  // namespace lsd

// logits [B, ld] fp32 (V <= ld), hist [nslots, L]; segmax null or [B, ldseg]
// with ldseg >= ld / 8 (then ld % 8 == 0).  counts null = empty histories.
extern "C" hipError_t lsd_penalize(float* logits, long ld, int B, int V, const int* hist, int L, int nslots,
                                   const int* slots, const long long* counts, const float* presence,
                                   const float* frequency, float* segmax, long ldseg, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (L <= 0 || L > 8192 || V > ld || (segmax != nullptr && (ld % 8 != 0 || ldseg * 8 < ld)))
    return hipErrorInvalidValue;
  int tbl = 64;
  while (tbl < 2 * L) tbl <<= 1;
  const size_t lds = (size_t)tbl * 2 * sizeof(int);
  if (lds > 64 * 1024) {
    // more than the default 64 KB of dynamic LDS: raised once per device (to
    // the largest table, 128 KB), on the first such launch -- an eager one,
    // the engine runs a new decode bucket once before capturing it
    static bool raised[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !raised[dev]) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(lsd::penalize_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < 64) raised[dev] = true;
    }
  }
  hipLaunchKernelGGL(lsd::penalize_kernel, dim3(B), dim3(lsd::PEN_NT), lds, st, logits, ld, V, hist, L, nslots, slots,
                     counts, presence, frequency, segmax, ldseg, tbl);
  return hipGetLastError();
}

// back = 1 when `step` was already advanced by the sampler (sample_into), so
// the entry written is the counter the draw used; step null = draw 0.
extern "C" hipError_t lsd_record_tokens(int* hist, int L, int nslots, const int* slots, const long long* step,
                                        int back, const int* tokens, const int* active, int B, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (L <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lsd::record_tokens_kernel, dim3((B + 255) / 256), dim3(256), 0, st, hist, L, nslots, slots, step,
                     back, tokens, active, B);
  return hipGetLastError();
}
