// Per-request allowed_token_ids of the on-device sampler (CDNA4): a vocabulary
// bitmask ahead of the draw.
//
// The last stage keeps, per KV slot, one flag and one bitmask over the logits'
// columns (W = ceil(width / 32) int32 words per slot):
//   on[slot]        the slot's request gave an allowed list (int32 [slots])
//   bits[slot, w]   token t is allowed when bit (t & 31) of word (t >> 5) is
//                   set (int32 [slots, W])
// Before the draw of a row -- after the repetition pass, the penalties and the
// logit edits, ahead of the sampler and the logprob kernel -- every token of
// [0, V) whose bit is clear gets logit -inf: a pure select, bit-equal to
// ops/reference.py allow_mask.  Columns at or past V are never written.
//
//   allow_mask_kernel   one workgroup of 256 threads per row, no LDS.  Rows
//                       whose slot is out of range or has on == 0 (default
//                       rows, every pad row: the scratch slot's flag stays 0)
//                       return at once, uniformly.  One mask byte is one
//                       8-logit segment (linear_f32's segmax granule): a thread
//                       takes segments 256 apart, consecutive threads
//                       consecutive segments -- 32 contiguous bytes of logits
//                       per lane, two 16-byte accesses.  By the byte of the
//                       bits below V:
//                         all set    the segment is skipped, not even read
//                         all clear  eight -inf and a segment maximum of -inf
//                                    are stored without reading the logits
//                                    (a last segment with padding columns
//                                    goes the mixed way: they stay)
//                         mixed      load, select, store, and the segment
//                                    maximum from the registers, padding
//                                    columns included, as penalize_kernel does
//                       A thread works on four segments at a time, so that
//                       the loads of its mixed ones are in flight together.
//                       A segment and its maximum belong to one thread, so the
//                       pass needs no barrier and no fence.
//
// VEC: the row base and stride allow 16-byte accesses (every caller with
// segment maxima; any 16-byte aligned logits with a stride that is a multiple
// of 4); otherwise the same walk with dword accesses.
#include "common.h"
#include "mask8.h"

namespace lsd {

constexpr int ALLOW_NT = 256;
constexpr int ALLOW_UN = 4;  // segments a thread has in flight

template <bool VEC>
__global__ __launch_bounds__(ALLOW_NT) void allow_mask_kernel(float* __restrict__ logits, long ld, int V,
                                                              const int* __restrict__ on,
                                                              const int* __restrict__ bits, int W, int nslots,
                                                              const int* __restrict__ slots,
                                                              float* __restrict__ segmax, long ldseg) {
  const int row = blockIdx.x;
  const int slot = slots[row];
  if (slot < 0 || slot >= nslots) return;  // uniform
  if (on[slot] == 0) return;               // uniform: default and pad rows
  // little-endian words: byte s holds the bits of tokens [8 s, 8 s + 8)
  const unsigned char* mk = reinterpret_cast<const unsigned char*>(bits + (long)slot * W);
  float* lg = logits + (long)row * ld;
  float* sm = segmax ? segmax + (long)row * ldseg : nullptr;
  const int nfull = V >> 3;  // segments wholly below V
  // ALLOW_UN trips at a time: the mask bytes first, then the loads of the
  // mixed segments -- all in flight together: one workgroup per row leaves a
  // CU four waves to hide the latency with -- then the selects and stores
  for (int s0 = threadIdx.x; s0 < nfull; s0 += ALLOW_UN * ALLOW_NT) {
    unsigned m[ALLOW_UN];
    float x[ALLOW_UN][8];
#pragma unroll
    for (int u = 0; u < ALLOW_UN; ++u) {
      const int s = s0 + u * ALLOW_NT;
      m[u] = s < nfull ? mk[s] : 0xFFu;  // past the end: as an all-set byte, skipped
    }
#pragma unroll
    for (int u = 0; u < ALLOW_UN; ++u)
      if (m[u] != 0xFFu && m[u] != 0) allow_load8<VEC>(lg + 8 * (long)(s0 + u * ALLOW_NT), x[u]);
#pragma unroll
    for (int u = 0; u < ALLOW_UN; ++u) {
      const int s = s0 + u * ALLOW_NT;
      if (m[u] != 0xFFu) allow_put8<VEC>(lg + 8 * (long)s, sm ? sm + s : nullptr, m[u], x[u]);
    }
  }
  // the last segment of a V that is no multiple of 8, one thread's: columns
  // [nv, 8) are padding (all present whenever there are segment maxima: ld % 8
  // == 0), read for the maximum and never written
  const int nv = V & 7;
  if (nv == 0 || threadIdx.x != (nfull & (ALLOW_NT - 1))) return;
  const unsigned full = (1u << nv) - 1u;
  const unsigned mt = mk[nfull] & full;
  if (mt == full) return;
  const float ninf = -__builtin_inff();
  float* p = lg + 8 * (long)nfull;
  float mx = ninf;
  for (int i = 0; i < 8 && 8 * (long)nfull + i < ld; ++i) {
    float v = p[i];
    if (i < nv && !((mt >> i) & 1u)) p[i] = v = ninf;
    mx = fmaxf(mx, v);
  }
  if (sm) sm[nfull] = mx;
}

}  // namespace lsd

// logits [B, ld] fp32 (V <= ld); on [nslots], bits [nslots, W] with W * 32 >=
// ld; slots [B]; segmax null or [B, ldseg] with ldseg >= ld / 8 (then ld % 8
// == 0).
extern "C" hipError_t lsd_allow_mask(float* logits, long ld, int B, int V, const int* on, const int* bits, int W,
                                     int nslots, const int* slots, float* segmax, long ldseg, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (V < 0 || V > ld || (long)W * 32 < ld || nslots <= 0 ||
      (segmax != nullptr && (ld % 8 != 0 || ldseg * 8 < ld)))
    return hipErrorInvalidValue;
  const bool vec = reinterpret_cast<uintptr_t>(logits) % 16 == 0 && ld % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(lsd::allow_mask_kernel<true>, dim3(B), dim3(lsd::ALLOW_NT), 0, st, logits, ld, V, on, bits, W,
                       nslots, slots, segmax, ldseg);
  else
    hipLaunchKernelGGL(lsd::allow_mask_kernel<false>, dim3(B), dim3(lsd::ALLOW_NT), 0, st, logits, ld, V, on, bits, W,
                       nslots, slots, segmax, ldseg);
  return hipGetLastError();
}
