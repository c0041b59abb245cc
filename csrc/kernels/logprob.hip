// Per-request token logprobs and top-N alternatives (CDNA4), after the sampler.
//
// One 1024-thread workgroup per row of the fp32 logits the sampler drew from
// (after the penalties, at temperature 1, before the top-k / top-p / min-p
// cuts).  Over the real vocabulary [0, V) -- padding columns [V, ld) are never
// counted and never selected, whatever they hold:
//   m   = row maximum
//   lse = m + log(sum exp(x - m))        -inf entries add 0
//   lp(x) = x - lse                      (-inf for x = -inf)
// and the record of the draw, slot = slots[row], j = step[row] - back:
//   lp_tok[slot, j]        = lp(x[tokens[row]])
//   lp_top_id[slot, j, e]  = id of the e-th most likely token    e < n = nlp[row]
//   lp_top[slot, j, e]     = its lp
// in the sampler's contract order (value descending by numeric comparison, so
// -0.0 == +0.0; index ascending).  Entries e in [n, W), and entries past the
// row's last token (V < n), are PADDED with id -1 and -inf, so a record never
// shows what an earlier sequence on the slot left there.  The drawn token's
// logprob and its entry among the alternatives are the same fl(x - lse) of the
// same two floats: bit-equal.
//
// Rows with nlp < 0 (every pad row, every row that did not ask) return at
// once, uniformly; so do inactive rows, a slot outside [0, nslots) and a j
// outside [0, L) -- record_tokens_kernel's guards.
//
// Memory traffic: a row of <= CH * NT * 4 floats (GPT-2's) is loaded once and
// the maximum, the sum, the threshold and the filter all run from registers;
// a longer row (Llama-3's) is read three times, twice of them from L2.
// Arithmetic: per-thread partial sums in index order, a wave butterfly, then
// the 16 wave sums in wave order -- no floating-point atomics, two launches
// give the same bits.
// Selection: threshold tau = n-th largest of the 64 16-thread group maxima (a
// lower bound of the n-th largest logit, as in the sampler's k <= 64 path),
// candidates {x >= tau} compacted into LDS, each ranked exactly.  More
// candidates than the LDS list holds (flat rows; tau = -inf when fewer than n
// groups hold a finite logit) take n rounds of block arg-max, each excluding
// what the rounds before it took: slower, exact.
#include "row_visit.h"

namespace lsd {

constexpr int LP_MAXW = 20;     // alternatives per record (host validates)
constexpr int LP_CAND = 1024;   // candidate list in LDS

__device__ __forceinline__ float lp_of(float x, float lse) {
  return x == -INFINITY ? -INFINITY : x - lse;
}

// The row from registers (one: loaded by the caller, CH float4 per thread) or
// streamed (for_row), in the same per-thread order: chunk, then element.
template <bool ONE, typename F>
__device__ __forceinline__ void lp_visit(const f32x4 (&q)[CH], const float* x, int V, F&& f) {
  if constexpr (ONE) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int b = ((int)threadIdx.x + i * NT) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (b + j < V) f(q[i][j], b + j);
    }
  } else {
    for_row(x, V, f);
  }
}

// ONE: the row fits CH float4 per thread (the host picks the instance by V)
template <bool ONE>
__global__ __launch_bounds__(NT) void logprob_kernel(const float* __restrict__ logits, long ld, int V,
                                                     const int* __restrict__ tokens, const int* __restrict__ nlp,
                                                     const int* __restrict__ slots,
                                                     const long long* __restrict__ step, int back,
                                                     const int* __restrict__ active, float* __restrict__ lp_tok,
                                                     int* __restrict__ lp_top_id, float* __restrict__ lp_top, int L,
                                                     int nslots, int W) {
  __shared__ __attribute__((aligned(16))) float cval[LP_CAND];
  __shared__ __attribute__((aligned(16))) int cidx[LP_CAND];
  __shared__ __attribute__((aligned(16))) float gmax[64];
  __shared__ float redv[16];
  __shared__ int redi[16];
  __shared__ unsigned s_cnt;
  __shared__ float s_pv;
  __shared__ int s_pi;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int want = nlp[row];
  if (want < 0) return;  // uniform: pad rows and rows that did not ask
  if (active != nullptr && active[row] == 0) return;
  const long long j = step ? step[row] - back : 0;
  const int slot = slots[row];
  if (j < 0 || j >= L || slot < 0 || slot >= nslots) return;  // uniform
  const int n = min(want, W);
  const long rec = (long)slot * L + j;
  const float* x = logits + (long)row * ld;
  const int tok = tokens[row];

  f32x4 q[CH];
  if constexpr (ONE) {
    const int last = ((V - 1) >> 2) << 2;
#pragma unroll
    for (int i = 0; i < CH; ++i) q[i] = *reinterpret_cast<const f32x4*>(x + min((tid + i * NT) * 4, last));
  }
  // ---- maximum, and the threshold of the n alternatives
  float mx = -INFINITY;
  lp_visit<ONE>(q, x, V, [&](float v, int) { mx = fmaxf(mx, v); });
  if (tid == 0) s_cnt = 0;
  const float tau = kth_group_max(mx, max(n, 1), gmax, redv);  // two barriers: s_cnt and gmax are visible
  float m = -INFINITY;
#pragma unroll
  for (int g4 = 0; g4 < 16; ++g4) {
    const f32x4 o = reinterpret_cast<const f32x4*>(gmax)[g4];
    m = fmaxf(fmaxf(m, fmaxf(o[0], o[1])), fmaxf(o[2], o[3]));
  }
  // ---- sum of exp(x - m) and the candidate count, one visit
  float part = 0.f;
  int cnt = 0;
  lp_visit<ONE>(q, x, V, [&](float v, int) {
    part += __expf(v - m);
    cnt += v >= tau ? 1 : 0;
  });
  part = wave_sum(part);
  __syncthreads();  // kth_group_max's readers of redv[0] are done
  if (lane_id() == 0) redv[tid >> 6] = part;
  __syncthreads();
  float sum = 0.f;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) sum += redv[w];
  const float lse = m == -INFINITY ? -INFINITY : m + logf(sum);
  if (tid == 0) lp_tok[rec] = (tok >= 0 && tok < V) ? lp_of(x[tok], lse) : -INFINITY;
  if (W == 0) return;  // uniform
  int* oid = lp_top_id + rec * W;
  float* olp = lp_top + rec * W;
  if (n == 0) {  // uniform
    if (tid < W) { oid[tid] = -1; olp[tid] = -INFINITY; }
    return;
  }
  // ---- compaction: wave scan of the counts, one LDS atomic per wave
  unsigned at = claim_slots(cnt, &s_cnt);
  __syncthreads();
  const unsigned ncand = s_cnt;  // uniform
  if (ncand <= (unsigned)LP_CAND) {
    lp_visit<ONE>(q, x, V, [&](float v, int idx) {
      if (v >= tau) {
        cval[at] = v;
        cidx[at] = idx;
        ++at;
      }
    });
    __syncthreads();
    // exact rank of every candidate in (value desc, index asc) order; the
    // first n land in the record, what the row cannot fill is padded
    const int nsel = (int)ncand;
    if (tid < nsel) {
      const float cv = cval[tid];
      const int ci = cidx[tid];
      int rk = 0;
      for (int j4 = 0; j4 < nsel; j4 += 4) {
        const f32x4 vv = *reinterpret_cast<const f32x4*>(cval + j4);
        const int4 ii = *reinterpret_cast<const int4*>(cidx + j4);
        const float vj[4] = {vv[0], vv[1], vv[2], vv[3]};
        const int ij[4] = {ii.x, ii.y, ii.z, ii.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          rk += (j4 + e < nsel && (vj[e] > cv || (vj[e] == cv && ij[e] < ci))) ? 1 : 0;
      }
      if (rk < n) { oid[rk] = ci; olp[rk] = lp_of(cv, lse); }
    }
    if (tid >= min(nsel, n) && tid < W) { oid[tid] = -1; olp[tid] = -INFINITY; }
    return;
  }
  // ---- more candidates than the list holds: n rounds of block arg-max over
  // the entries that come after the previous pick in contract order
  float pv = INFINITY;
  int pi = -1;
  for (int r = 0; r < n; ++r) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    lp_visit<ONE>(q, x, V, [&](float v, int idx) {
      const bool left = r == 0 || v < pv || (v == pv && idx > pi);
      if (left && (v > best || (v == best && idx < bi))) { best = v; bi = idx; }
    });
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) {
      const float ov = shfl_xor(best, msk);
      const int oi = shfl_xor(bi, msk);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    __syncthreads();  // the previous round's readers of s_pv / s_pi are done
    if (lane_id() == 0) { redv[tid >> 6] = best; redi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < NT / 64; ++w)
        if (redv[w] > best || (redv[w] == best && redi[w] < bi)) { best = redv[w]; bi = redi[w]; }
      const bool none = bi == 0x7fffffff;  // the row has fewer than r + 1 entries
      oid[r] = none ? -1 : bi;
      olp[r] = none ? -INFINITY : lp_of(best, lse);
      s_pv = best;
      s_pi = bi;
    }
    __syncthreads();
    pv = s_pv;
    pi = s_pi;
  }
  if (tid >= n && tid < W) { oid[tid] = -1; olp[tid] = -INFINITY; }
}

}  // namespace lsd

// logits [B, ld] fp32 (V <= ld, ld % 4 == 0); tokens / nlp / slots [B]; step
// null = draw 0, else [B] with back = 1 when the sampler has already advanced
// it (the record_tokens convention); active null = every row.  Records:
// lp_tok [nslots, L], lp_top_id / lp_top [nslots, L, W], W <= 20.
extern "C" hipError_t lsd_logprobs(const float* logits, long ld, int B, int V, const int* tokens, const int* nlp,
                                   const int* slots, const long long* step, int back, const int* active,
                                   float* lp_tok, int* lp_top_id, float* lp_top, int L, int nslots, int W,
                                   hipStream_t st) {
  if (W < 0 || W > lsd::LP_MAXW || V < 1 || V > ld || ld % 4 != 0 || L <= 0 || nslots <= 0)
    return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  auto kern = V <= lsd::CH * lsd::NT * 4 ? lsd::logprob_kernel<true> : lsd::logprob_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(lsd::NT), 0, st, logits, ld, V, tokens, nlp, slots, step, back, active, lp_tok,
                     lp_top_id, lp_top, L, nslots, W);
  return hipGetLastError();
}
