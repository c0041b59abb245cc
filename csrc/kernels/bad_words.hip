// Per-request bad_words of the on-device sampler (CDNA4): token sequences that
// may never be completed (HF bad_words_ids, vLLM bad_words).
//
// The last stage keeps, per KV slot, the request's sequences back to back:
//   cnt[slot]      sequences (int32 [slots]; 0 = the request gave none)
//   end[slot, e]   exclusive end offset of sequence e in the slot's token row:
//                  sequence e is tok[slot, end[e - 1] .. end[e]), end[-1] = 0
//                  (int32 [slots, N])
//   tok[slot, j]   the sequences' tokens (int32 [slots, T])
// and reads the context table of repeat.hip: plen[slot] and ctok[slot, :], the
// prompt and then the generated tokens.  Before the draw of a row with counter
// c (step[row], read before the sampler advances it; step null = draw 0) the
// context is x = ctok[slot, 0 .. n), n = min(plen + c, L), and every sequence
// w of m tokens with m - 1 <= n and x[n - m + 1 .. n) == w[0 .. m - 1) bans its
// last token: logit[w[m - 1]] <- -inf when it is in [0, V) (m = 1: always) --
// after the repetition pass, ahead of the penalties, the logit edits, the
// allowed-token mask and the sampler; bit-equal to ops/reference.py bad_words.
// There is no arithmetic on logits.  Columns at or past V are never written.
//
//   bad_words_kernel   one workgroup of 256 threads per row.  Rows whose slot
//                      is out of range or has cnt == 0 (default rows, every pad
//                      row: the scratch slot's count stays 0) return at once,
//                      uniformly.  The last min(n, 31) context tokens go into
//                      LDS once; thread e < cnt compares sequence e's first
//                      m - 1 tokens with the tail and stores -inf on a match.
//                      Several threads may store the same -inf to one logit:
//                      identical plain vector stores, no atomics.  Then, after
//                      a fence and a barrier, since two banned tokens can
//                      share a segment, each matching thread recomputes the
//                      maximum of its token's 8-logit segment from its 8
//                      stored logits (linear_f32's segmax, which the sampler's
//                      fast path trusts), padding columns included, as
//                      repeat_kernel does.
//
// A sequence whose offsets do not describe 1 to 32 tokens inside the row is
// skipped: the kernel never reads outside the tables whatever they hold.
#include "common.h"

namespace lsd {

constexpr int BAD_NT = 256;      // threads, and the most sequences a slot can hold
constexpr int BAD_MAX_M = 32;    // tokens of the longest sequence
constexpr int BAD_MAX_L = 8192;  // the context table's own limit (repeat.hip)

__global__ __launch_bounds__(BAD_NT) void bad_words_kernel(float* __restrict__ logits, long ld, int V,
                                                           const int* __restrict__ cnt,
                                                           const int* __restrict__ end, int N,
                                                           const int* __restrict__ btok, int T,
                                                           const int* __restrict__ plen,
                                                           const int* __restrict__ ctok, int L, int nslots,
                                                           const int* __restrict__ slots,
                                                           const long long* __restrict__ step,
                                                           float* __restrict__ segmax, long ldseg) {
  __shared__ int tail[BAD_MAX_M];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int slot = slots[row];
  if (slot < 0 || slot >= nslots) return;  // uniform
  int ns = cnt[slot];
  if (ns <= 0) return;  // uniform: default and pad rows
  if (ns > N) ns = N;
  const long long c = step ? step[row] : 0;
  long long n64 = (long long)plen[slot] + c;
  if (n64 > (long long)L) n64 = L;
  if (n64 < 0) n64 = 0;
  const int n = (int)n64;
  const int k = n < BAD_MAX_M - 1 ? n : BAD_MAX_M - 1;  // tail[j] = x[n - k + j]
  if (tid < k) tail[tid] = ctok[(long)slot * L + (n - k) + tid];
  __syncthreads();
  float* lg = logits + (long)row * ld;
  int t = -1;  // the token this thread banned
  if (tid < ns) {
    const int* en = end + (long)slot * N;
    const int b = tid ? en[tid - 1] : 0, e = en[tid];
    const int m = e - b;
    // m - 1 <= k: the context holds the prefix (m - 1 <= 31 always)
    if (b >= 0 && e <= T && m >= 1 && m <= BAD_MAX_M && m - 1 <= k) {
      const int* w = btok + (long)slot * T + b;
      bool eq = true;
      for (int j = 0; j < m - 1; ++j) {
        if (w[j] != tail[k - (m - 1) + j]) {
          eq = false;
          break;
        }
      }
      const int last = w[m - 1];
      if (eq && last >= 0 && last < V) {
        lg[last] = -INFINITY;
        t = last;
      }
    }
  }
  if (segmax == nullptr) return;  // uniform
  // every ban of the row before any segment is read back
  __threadfence_block();
  __syncthreads();
  if (t >= 0) {
    // volatile: written by other threads of this block (lg is __restrict__)
    const volatile float* q = lg + 8 * (long)(t >> 3);
    float mx = q[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) mx = fmaxf(mx, q[i]);
    segmax[(long)row * ldseg + (t >> 3)] = mx;  // tokens sharing the segment store the same value
  }
}

}  // namespace lsd

// logits [B, ld] fp32 (V <= ld); cnt [nslots], end [nslots, N], btok [nslots,
// T]; plen [nslots], ctok [nslots, L] of the context table; slots [B]; step
// null = draw 0; segmax null or [B, ldseg] with ldseg >= ld / 8 (then ld % 8
// == 0).
extern "C" hipError_t lsd_bad_words(float* logits, long ld, int B, int V, const int* cnt, const int* end, int N,
                                    const int* btok, int T, const int* plen, const int* ctok, int L, int nslots,
                                    const int* slots, const long long* step, float* segmax, long ldseg,
                                    hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (N <= 0 || N > lsd::BAD_NT || T <= 0 || L <= 0 || L > lsd::BAD_MAX_L || nslots <= 0 || V < 0 || V > ld ||
      (segmax != nullptr && (ld % 8 != 0 || ldseg * 8 < ld)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(lsd::bad_words_kernel, dim3(B), dim3(lsd::BAD_NT), 0, st, logits, ld, V, cnt, end, N, btok, T,
                     plen, ctok, L, nslots, slots, step, segmax, ldseg);
  return hipGetLastError();
}
