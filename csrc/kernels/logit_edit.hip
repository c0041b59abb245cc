// Per-request logit edits of the on-device sampler (CDNA4): logit_bias, banned
// tokens and min_new_tokens.
//
// The last stage keeps, per KV slot, a small table of edits (E = max_logit_edits
// columns; the host sorts a request's entries by token):
//   cnt[slot]                       entries in use (int32 [slots])
//   tok / val / until [slot, e]     logit[tok] <- logit[tok] + val while the
//                                   draw's sampler counter is below `until`
//                                   (int32 / fp32 / int32 [slots, E]); a ban is
//                                   val = -inf, a permanent entry until =
//                                   INT32_MAX, min_new_tokens = m is the entry
//                                   (eos, -inf, m)
// Before the draw of a row -- after the penalty pass, ahead of the sampler --
// every entry whose `until` exceeds the row's counter (step[row], read before
// the sampler advances it; step null = draw 0) is added in fp32, one rounding
// per addition, in table order: bit-equal to ops/reference.py logit_edits.
//
//   logit_edit_kernel   one workgroup of 256 threads per row.  Rows whose slot
//                       has no entry (default rows, every pad row: the scratch
//                       slot's count stays 0) return at once, uniformly.
//                       Thread e takes entry e only when it opens a run of
//                       equal tokens: it adds the run's active values to the
//                       logit in one register and stores once, and only if
//                       some entry of the run was active -- no two threads
//                       write one logit, so the result does not depend on
//                       arrival order.  Tokens outside [0, V) are ignored.
//                       Then -- after a block barrier, since two entries can
//                       share a segment -- the maximum of every 8-logit
//                       segment an active run touched is recomputed from its 8
//                       stored logits (linear_f32's segmax, which the
//                       sampler's fast path trusts), the last segment's
//                       padding columns past V included, as penalize_kernel does.
//
// E <= 1024: no LDS table, a thread makes at most 4 trips (their active runs
// are remembered in a 4-bit mask across the barrier).
#include "common.h"

namespace lsd {

constexpr int EDIT_NT = 256;
constexpr int EDIT_MAX = 1024;

__global__ __launch_bounds__(EDIT_NT) void logit_edit_kernel(float* __restrict__ logits, long ld, int V,
                                                             const int* __restrict__ cnt,
                                                             const int* __restrict__ tok,
                                                             const float* __restrict__ val,
                                                             const int* __restrict__ until, int E, int nslots,
                                                             const int* __restrict__ slots,
                                                             const long long* __restrict__ step,
                                                             float* __restrict__ segmax, long ldseg) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const int slot = slots[row];
  if (slot < 0 || slot >= nslots) return;  // uniform
  int n = cnt[slot];
  if (n <= 0) return;  // uniform: default and pad rows
  if (n > E) n = E;
  const long long ctr = step ? step[row] : 0;
  const int* tk = tok + (long)slot * E;
  const float* vl = val + (long)slot * E;
  const int* un = until + (long)slot * E;
  float* lg = logits + (long)row * ld;
  unsigned wrote = 0;  // bit k: this thread's k-th trip stored a logit
  int k = 0;
  for (int e = tid; e < n; e += EDIT_NT, ++k) {
    const int t = tk[e];
    if (t < 0 || t >= V) continue;
    if (e > 0 && tk[e - 1] == t) continue;  // the run's first entry does the work
    float x = lg[t];
    bool any = false;
    for (int j = e; j < n && tk[j] == t; ++j) {
      if (ctr < (long long)un[j]) {
        x = x + vl[j];
        any = true;
      }
    }
    if (any) {
      lg[t] = x;
      wrote |= 1u << k;
    }
  }
  if (segmax == nullptr) return;  // uniform
  // every logit write of the row before any segment is read back
  __threadfence_block();
  __syncthreads();
  float* sm = segmax + (long)row * ldseg;
  k = 0;
  for (int e = tid; e < n; e += EDIT_NT, ++k) {
    if (!(wrote & (1u << k))) continue;
    const int s = tk[e] >> 3;
    // volatile: written above by other threads of this block (lg is __restrict__)
    const volatile float* q = lg + 8 * (long)s;
    float m = q[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) m = fmaxf(m, q[i]);
    sm[s] = m;  // runs sharing the segment store the same value
  }
}

}  // namespace lsd

// logits [B, ld] fp32 (V <= ld); cnt [nslots], tok / val / until [nslots, E];
// slots [B]; step null = draw 0; segmax null or [B, ldseg] with ldseg >= ld / 8
// (then ld % 8 == 0).
extern "C" hipError_t lsd_logit_edits(float* logits, long ld, int B, int V, const int* cnt, const int* tok,
                                      const float* val, const int* until, int E, int nslots, const int* slots,
                                      const long long* step, float* segmax, long ldseg, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (E <= 0 || E > lsd::EDIT_MAX || nslots <= 0 || V > ld ||
      (segmax != nullptr && (ld % 8 != 0 || ldseg * 8 < ld)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(lsd::logit_edit_kernel, dim3(B), dim3(lsd::EDIT_NT), 0, st, logits, ld, V, cnt, tok, val, until,
                     E, nslots, slots, step, segmax, ldseg);
  return hipGetLastError();
}
