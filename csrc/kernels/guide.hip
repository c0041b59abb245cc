// Per-request guided decoding of the on-device sampler (CDNA4): a token
// automaton whose state lives on the device, masks the logits ahead of the draw
// and advances behind it, inside the captured decode graphs.
//
// The last stage keeps G guide rows and, per KV slot, which row the slot's
// request follows and the state it is in:
//   gcls [G, Vp]     int16  class of every logits column (token -> [0, C))
//   gnext[G, cells]  int16  row-major next[S, C] of guide g: the state after a
//                           token of class c in state s is cell s * C + c, -1
//                           when the token may not be drawn there
//   gdim [G, 2]      int32  (S, C) of guide g
//   gsl  [slots, 2]  int32  (guide row or -1, current state) of a KV slot
// Both kernels act on a slot only when it lies in the table, its g in [0, G),
// its state in [0, S), C in [1, GUIDE_MAXC] and (state + 1) * C <= cells, so
// every index they form is bounded by the tables' fixed capacities (G, Vp,
// cells, slots) whatever gdim and gsl hold: bit-equal to ops/reference.py
// guide_mask / guide_advance.
//
//   guide_mask_kernel     one workgroup of 256 threads per row; rows on other
//                         slots return at once, uniformly.  The state's row of
//                         C cells goes into LDS as one drawable flag per class
//                         (a byte each, at most 4 KB), one barrier.  Then the
//                         walk of allow_mask_kernel: segments of 8 logits, a
//                         thread's segments 256 apart, four in flight.  Per
//                         segment the 8 classes are one 16-byte load and the
//                         mask byte 8 LDS byte reads (a class at or past C is
//                         not drawable); by that byte the segment is skipped
//                         unread (all set), stored as eight -inf with a
//                         maximum of -inf unread (all clear), or loaded,
//                         selected and stored with its maximum from the
//                         registers (mixed), padding columns included.
//                         Columns at or past V are never written.  A pure
//                         select; the tables are only read.
//   guide_advance_kernel  one thread per row, behind the draw: an active row
//                         on such a slot whose token t lies in [0, V) and has
//                         a class c < C stores gnext[g, state * C + c] as its
//                         slot's state, a plain vector store; each row owns
//                         its slot.  Everything else is left alone.
//
// VEC: the logits' row base and stride and the class rows allow 16-byte
// accesses (every caller with segment maxima and a padded vocabulary);
// otherwise the same walk with dword and 2-byte accesses.
#include "common.h"
#include "mask8.h"

namespace lsd {

constexpr int GUIDE_NT = 256;
constexpr int GUIDE_UN = 4;       // segments a thread has in flight
constexpr int GUIDE_MAXC = 4096;  // classes whose flags the LDS array holds

typedef short s16x8 __attribute__((ext_vector_type(8)));

// (g, state, C) of a slot the passes act on; false otherwise.
__device__ __forceinline__ bool guide_state(const int* __restrict__ gdim, int G, long cells,
                                            const int* __restrict__ gsl, int nslots, int slot, int& g, int& s, int& C) {
  if (slot < 0 || slot >= nslots) return false;
  g = gsl[2 * (long)slot];
  s = gsl[2 * (long)slot + 1];
  if (g < 0 || g >= G) return false;
  const int S = gdim[2 * g];
  C = gdim[2 * g + 1];
  return s >= 0 && s < S && C >= 1 && C <= GUIDE_MAXC && ((long)s + 1) * C <= cells;
}

// The mask byte of the 8 classes c: bit i set when class c[i] is drawable.
__device__ __forceinline__ unsigned guide_byte(const short (&c)[8], const unsigned char* ok, int C) {
  unsigned m = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned k = (unsigned)(int)c[i];  // a negative class compares past C
    m |= (k < (unsigned)C && ok[k < (unsigned)C ? k : 0] ? 1u : 0u) << i;
  }
  return m;
}

template <bool VEC>
__global__ __launch_bounds__(GUIDE_NT) void guide_mask_kernel(float* __restrict__ logits, long ld, int V,
                                                              const short* __restrict__ gcls, long Vp,
                                                              const short* __restrict__ gnext, long cells,
                                                              const int* __restrict__ gdim, int G,
                                                              const int* __restrict__ gsl, int nslots,
                                                              const int* __restrict__ slots,
                                                              float* __restrict__ segmax, long ldseg) {
  __shared__ unsigned char ok[GUIDE_MAXC];
  const int row = blockIdx.x;
  int g, s, C;
  if (!guide_state(gdim, G, cells, gsl, nslots, slots[row], g, s, C)) return;  // uniform
  const short* nx = gnext + (long)g * cells + (long)s * C;  // (s + 1) * C <= cells
  for (int c = threadIdx.x; c < C; c += GUIDE_NT) ok[c] = nx[c] >= 0;
  __syncthreads();
  const short* cl = gcls + (long)g * Vp;  // V <= ld <= Vp
  float* lg = logits + (long)row * ld;
  float* sm = segmax ? segmax + (long)row * ldseg : nullptr;
  const int nfull = V >> 3;  // segments wholly below V
  // GUIDE_UN trips at a time: the class loads first, then the flags, then the
  // loads of the mixed segments -- all in flight together -- then the selects
  // and stores
  for (int s0 = threadIdx.x; s0 < nfull; s0 += GUIDE_UN * GUIDE_NT) {
    short c[GUIDE_UN][8];
    unsigned m[GUIDE_UN];
    float x[GUIDE_UN][8];
#pragma unroll
    for (int u = 0; u < GUIDE_UN; ++u) {
      const int sg = s0 + u * GUIDE_NT;
      if (sg < nfull) {
        if constexpr (VEC) {
          const s16x8 v = *reinterpret_cast<const s16x8*>(cl + 8 * (long)sg);
#pragma unroll
          for (int i = 0; i < 8; ++i) c[u][i] = v[i];
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) c[u][i] = cl[8 * (long)sg + i];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < GUIDE_UN; ++u)
      m[u] = s0 + u * GUIDE_NT < nfull ? guide_byte(c[u], ok, C) : 0xFFu;  // past the end: skipped
#pragma unroll
    for (int u = 0; u < GUIDE_UN; ++u)
      if (m[u] != 0xFFu && m[u] != 0) allow_load8<VEC>(lg + 8 * (long)(s0 + u * GUIDE_NT), x[u]);
#pragma unroll
    for (int u = 0; u < GUIDE_UN; ++u) {
      const int sg = s0 + u * GUIDE_NT;
      if (m[u] != 0xFFu) allow_put8<VEC>(lg + 8 * (long)sg, sm ? sm + sg : nullptr, m[u], x[u]);
    }
  }
  // the last segment of a V that is no multiple of 8, one thread's: columns
  // [nv, 8) are padding (all present whenever there are segment maxima: ld % 8
  // == 0), read for the maximum and never written; their classes are not read
  const int nv = V & 7;
  if (nv == 0 || threadIdx.x != (nfull & (GUIDE_NT - 1))) return;
  unsigned mt = 0;
  for (int i = 0; i < nv; ++i) {
    const unsigned k = (unsigned)(int)cl[8 * (long)nfull + i];
    mt |= (k < (unsigned)C && ok[k < (unsigned)C ? k : 0] ? 1u : 0u) << i;
  }
  if (mt == (1u << nv) - 1u) return;
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

__global__ __launch_bounds__(GUIDE_NT) void guide_advance_kernel(int* __restrict__ gsl, int nslots,
                                                                 const short* __restrict__ gcls, long Vp,
                                                                 const short* __restrict__ gnext, long cells,
                                                                 const int* __restrict__ gdim, int G, int V,
                                                                 const int* __restrict__ slots,
                                                                 const int* __restrict__ tokens,
                                                                 const int* __restrict__ active, int B) {
  const int i = blockIdx.x * GUIDE_NT + threadIdx.x;
  if (i >= B) return;
  if (active && active[i] == 0) return;
  const int slot = slots[i], t = tokens[i];
  int g, s, C;
  if (!guide_state(gdim, G, cells, gsl, nslots, slot, g, s, C)) return;
  if (t < 0 || t >= V) return;  // V <= Vp
  const unsigned c = (unsigned)(int)gcls[(long)g * Vp + t];
  if (c >= (unsigned)C) return;
  gsl[2 * (long)slot + 1] = gnext[(long)g * cells + (long)s * C + c];
}

}  // namespace lsd

// logits [B, ld] fp32 (V <= ld <= Vp); gcls [G, Vp], gnext [G, cells] int16,
// gdim [G, 2], gsl [nslots, 2] int32; slots [B]; segmax null or [B, ldseg] with
// ldseg >= ld / 8 (then ld % 8 == 0).
extern "C" hipError_t lsd_guide_mask(float* logits, long ld, int B, int V, const short* gcls, long Vp,
                                     const short* gnext, long cells, const int* gdim, int G, const int* gsl,
                                     int nslots, const int* slots, float* segmax, long ldseg, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (V < 0 || V > ld || Vp < ld || cells <= 0 || nslots <= 0 || G <= 0 ||
      (segmax != nullptr && (ld % 8 != 0 || ldseg * 8 < ld)))
    return hipErrorInvalidValue;
  const bool vec = reinterpret_cast<uintptr_t>(logits) % 16 == 0 && ld % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(gcls) % 16 == 0 && Vp % 8 == 0;
  if (vec)
    hipLaunchKernelGGL(lsd::guide_mask_kernel<true>, dim3(B), dim3(lsd::GUIDE_NT), 0, st, logits, ld, V, gcls, Vp,
                       gnext, cells, gdim, G, gsl, nslots, slots, segmax, ldseg);
  else
    hipLaunchKernelGGL(lsd::guide_mask_kernel<false>, dim3(B), dim3(lsd::GUIDE_NT), 0, st, logits, ld, V, gcls, Vp,
                       gnext, cells, gdim, G, gsl, nslots, slots, segmax, ldseg);
  return hipGetLastError();
}

// gsl [nslots, 2] (rewritten), the tables as above (V <= Vp); slots, tokens
// [B]; active null or [B].
extern "C" hipError_t lsd_guide_advance(int* gsl, int nslots, const short* gcls, long Vp, const short* gnext,
                                        long cells, const int* gdim, int G, int V, const int* slots,
                                        const int* tokens, const int* active, int B, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (V < 0 || V > Vp || cells <= 0 || nslots <= 0 || G <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lsd::guide_advance_kernel, dim3((B + lsd::GUIDE_NT - 1) / lsd::GUIDE_NT), dim3(lsd::GUIDE_NT), 0,
                     st, gsl, nslots, gcls, Vp, gnext, cells, gdim, G, V, slots, tokens, active, B);
  return hipGetLastError();
}
