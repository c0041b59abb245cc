// Sequence scoring (CDNA4): lm_head GEMM fused with the row's log-softmax.
//
//   logit[r, c] = xn[r, :] . w[c, :]          bf16 products, fp32 accumulation
// and, over the real vocabulary c in [0, V) of every row r (padding columns
// [V, Vp) take part in nothing, whatever the padded weight rows hold):
//   m   = row maximum,  lse = m + log(sum exp(logit - m))
//   tok_lp[r] = logit[r, targets[r]] - lse
//   top_id[r] = argmax (lowest index on ties, numeric comparison: -0.0 == +0.0)
//   top_lp[r] = logit[r, top_id[r]] - lse     bit-equal to tok_lp where the two ids agree
// No logit is ever stored: scoring a T-token sequence needs 3 T numbers, not
// the [T, Vp] fp32 matrix (4.2 GB at 8192 x 128256).
//
// lm_head_score_kernel, grid (row blocks, vocabulary slices), 4 waves:
//   * a workgroup owns 128 rows and walks the 128-column tiles of its slice;
//     wave (wm, wn) holds the 64 x 64 quadrant as 4 x 4 MFMA 16x16x32 tiles;
//   * A and W tiles of 64 k go through LDS by LDS-DMA, XOR-swizzled, two
//     buffers; the (tile, k) steps form ONE pipeline, so the first k-step of
//     the next tile loads while this tile's accumulators are folded.  The A
//     block is re-read (from L2: <= 1 MB) for every column tile;
//   * at a tile's last k-step every lane folds its accumulators -- 16 rows x 4
//     columns -- into per-row running state in registers: (m, l, index of m,
//     target logit), l rescaled online as the attention kernels do.  The best
//     value IS the running maximum, so it has no register of its own.  Columns
//     >= V are -inf before the fold; loads of rows past T / Vp are clamped to
//     the last row, never issued out of bounds;
//   * once per slice the 16 lanes that share a row merge by DPP, the two
//     column waves merge through LDS in column order, and one 16-byte partial
//     (m, l, index, target logit) per (row, slice) is written.
// lm_head_score_combine_kernel: one thread per row merges its S partials in
// ascending slice order and writes the three outputs.
// No atomics anywhere and every merge order is fixed by (T, Vp, S): two
// launches on the same input give the same bits.
#include "common.h"
#include "api.h"

namespace lsd {

constexpr int SC_BM = 128, SC_BN = 128, SC_BK = 64;
constexpr int SC_TILE = SC_BM * SC_BK * 2;  // 16 KiB per operand tile
constexpr float SC_L2E = 1.4426950408889634f;
constexpr int SC_NOIDX = 0x7fffffff;

typedef __attribute__((address_space(3))) void sc_lds_void;
typedef __attribute__((address_space(1))) const void sc_gbl_cvoid;

// s_waitcnt immediate for vmcnt(0) alone (gfx9 layout)
constexpr int SC_VM0 = (0x7 << 4) | (0xF << 8);

// [128 rows][64 k] bf16 tile: 128-byte LDS rows, 16-byte chunk index XORed with
// (row >> 1) & 7 on the source address (LDS-DMA writes lane-linear) and on the
// read.  Rows past row_max load row_max's data (masked or unused downstream).
__device__ __forceinline__ void sc_stage(char* lds_tile, const bf16* src, long ld, int row0, int row_max, int k0) {
  const int lane = lane_id(), w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int inst = w * 4 + q;
    const int row = inst * 8 + (lane >> 3);
    const int lch = (lane & 7) ^ ((row >> 1) & 7);
    const int grow = min(row0 + row, row_max);
    const bf16* gp = src + (long)grow * ld + k0 + lch * 8;
    __builtin_amdgcn_global_load_lds((sc_gbl_cvoid*)gp, (sc_lds_void*)(lds_tile + inst * 1024), 16, 0, 0);
  }
}

__device__ __forceinline__ bf16x8 sc_frag(const char* tile, int row, int chunk) {
  const int pch = chunk ^ ((row >> 1) & 7);
  return *reinterpret_cast<const bf16x8*>(tile + row * 128 + pch * 16);
}

// exp(a - b) for a <= b; 0 for a = -inf (also when b = -inf: an empty state)
__device__ __forceinline__ float sc_exp(float a, float b) {
  return a == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((a - b) * SC_L2E);
}

// Index bits carried in a float lane / vector slot.  By value: a bit cast
// applied straight to a vector element reads element 0.
__device__ __forceinline__ int sc_f2i(float f) { return __builtin_bit_cast(int, f); }
__device__ __forceinline__ float sc_i2f(int i) { return __builtin_bit_cast(float, i); }

// Row state: m = maximum so far (= the best value), l = sum exp(x - m), bi =
// lowest index of m, tg = the target's logit (-inf until its column is met).
struct ScState {
  float m, l;
  int bi;
  float tg;
};

// union of two column sets: ties in m go to the lower index
__device__ __forceinline__ ScState sc_merge(ScState a, ScState b) {
  ScState o;
  o.m = fmaxf(a.m, b.m);
  o.l = a.l * sc_exp(a.m, o.m) + b.l * sc_exp(b.m, o.m);
  o.bi = b.m > a.m ? b.bi : (b.m == a.m ? min(a.bi, b.bi) : a.bi);
  o.tg = fmaxf(a.tg, b.tg);
  return o;
}

template <int OFF>
__device__ __forceinline__ ScState sc_xchg(ScState s) {
  ScState o;
  o.m = wave_xchg<OFF>(s.m);
  o.l = wave_xchg<OFF>(s.l);
  o.bi = sc_f2i(wave_xchg<OFF>(sc_i2f(s.bi)));
  o.tg = wave_xchg<OFF>(s.tg);
  return o;
}

__global__ LSD_NO_PK_F32 __launch_bounds__(256) void lm_head_score_kernel(
    const bf16* __restrict__ A, long lda, const bf16* __restrict__ W, long ldw, const int* __restrict__ targets,
    int T, int V, int Vp, int K, int S, f32x4* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) char smem[4 * SC_TILE];  // [buf][A | W]
  __shared__ __attribute__((aligned(16))) f32x4 red[2][SC_BM];    // [column wave][row]
  const int m0 = blockIdx.x * SC_BM, sl = blockIdx.y;
  const int NT = (Vp + SC_BN - 1) / SC_BN;
  const int tb = (int)((long)NT * sl / S), te = (int)((long)NT * (sl + 1) / S);
  const int KT = K / SC_BK;
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int r = lane & 15, g = lane >> 4;

  // lane's rows: wm * 64 + i * 16 + 4 g + q, state index i * 4 + q
  ScState st[16];
  int tr[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    st[e] = ScState{-INFINITY, 0.f, SC_NOIDX, -INFINITY};
    const int row = m0 + wm * 64 + (e >> 2) * 16 + 4 * g + (e & 3);
    tr[e] = targets[min(row, T - 1)];
  }

  f32x4 acc[4][4];
  const int steps = (te - tb) * KT;
  if (steps > 0) {
    sc_stage(smem, A, lda, m0, T - 1, 0);
    sc_stage(smem + SC_TILE, W, ldw, tb * SC_BN, Vp - 1, 0);
    __builtin_amdgcn_s_waitcnt(SC_VM0);
    block_sync();
  }
  int cur = 0, kt = 0, tile = tb;
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) {  // the next k-step, or the next tile's first
      const int nk = kt + 1 < KT ? kt + 1 : 0;
      const int ntile = kt + 1 < KT ? tile : tile + 1;
      char* nb = smem + (cur ^ 1) * 2 * SC_TILE;
      sc_stage(nb, A, lda, m0, T - 1, nk * SC_BK);
      sc_stage(nb + SC_TILE, W, ldw, ntile * SC_BN, Vp - 1, nk * SC_BK);
    }
    if (kt == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const char* ta = smem + cur * 2 * SC_TILE;
    const char* tw = ta + SC_TILE;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], wf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = sc_frag(ta, wm * 64 + i * 16 + r, kk * 4 + g);
#pragma unroll
      for (int j = 0; j < 4; ++j) wf[j] = sc_frag(tw, wn * 64 + j * 16 + r, kk * 4 + g);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(af[i], wf[j], acc[i][j]);
    }
    if (kt == KT - 1) {
      // fold: C layout col = r, row = 4 g + q; this lane's columns of the tile
      // are c0 + 16 j, ascending, so a strict > keeps the lowest index
      const int c0 = tile * SC_BN + wn * 64 + r;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          ScState& z = st[i * 4 + q];
          const int t = tr[i * 4 + q];
          float x[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] = c0 + 16 * j < V ? acc[i][j][q] : -INFINITY;
          float tm = x[0];
          int ti = c0;
#pragma unroll
          for (int j = 1; j < 4; ++j)
            if (x[j] > tm) { tm = x[j]; ti = c0 + 16 * j; }
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (c0 + 16 * j == t) z.tg = x[j];
          if (tm > z.m) z.bi = ti;
          const float mn = fmaxf(z.m, tm);
          z.l = z.l * sc_exp(z.m, mn) + ((sc_exp(x[0], mn) + sc_exp(x[1], mn)) + (sc_exp(x[2], mn) + sc_exp(x[3], mn)));
          z.m = mn;
        }
    }
    __builtin_amdgcn_s_waitcnt(SC_VM0);  // this wave's LDS-DMA of the next step landed
    block_sync();                        // everyone's did, and buffer `cur` has no reader left
    cur ^= 1;
    if (++kt == KT) { kt = 0; ++tile; }
  }

  // the 16 lanes of a row (same g, r = 0..15): butterfly; lane r = 0 holds the merge
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    ScState z = st[e];
    z = sc_merge(z, sc_xchg<1>(z));
    z = sc_merge(z, sc_xchg<2>(z));
    z = sc_merge(z, sc_xchg<4>(z));
    z = sc_merge(z, sc_xchg<8>(z));
    if (r == 0) {
      const int row = wm * 64 + (e >> 2) * 16 + 4 * g + (e & 3);
      red[wn][row] = f32x4{z.m, z.l, sc_i2f(z.bi), z.tg};
    }
  }
  block_sync();
  if (threadIdx.x < SC_BM && m0 + (int)threadIdx.x < T) {
    const f32x4 a = red[0][threadIdx.x], b = red[1][threadIdx.x];
    const ScState z = sc_merge(ScState{a[0], a[1], sc_f2i(a[2]), a[3]},
                               ScState{b[0], b[1], sc_f2i(b[2]), b[3]});
    part[(long)(m0 + threadIdx.x) * S + sl] = f32x4{z.m, z.l, sc_i2f(z.bi), z.tg};
  }
}

__global__ LSD_NO_PK_F32 __launch_bounds__(256) void lm_head_score_combine_kernel(
    const f32x4* __restrict__ part, int T, int S, float* __restrict__ tok_lp, int* __restrict__ top_id,
    float* __restrict__ top_lp) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= T) return;
  float m = -INFINITY, l = 0.f, tg = -INFINITY;
  int bi = SC_NOIDX;
  for (int s = 0; s < S; ++s) {  // ascending slices = ascending columns
    const f32x4 p = part[(long)row * S + s];
    const float mn = fmaxf(m, p[0]);
    l = l * sc_exp(m, mn) + p[1] * sc_exp(p[0], mn);
    if (p[0] > m) bi = sc_f2i(p[2]);
    m = mn;
    tg = fmaxf(tg, p[3]);
  }
  const float lse = m + __builtin_amdgcn_logf(l) * 0.6931471805599453f;  // v_log_f32 is log2
  tok_lp[row] = tg == -INFINITY ? -INFINITY : tg - lse;
  top_id[row] = bi;
  top_lp[row] = m - lse;
}

}  // namespace lsd

// Slices of the vocabulary for a [T, K] x [Vp, K] scoring launch: row blocks x
// slices fills the 256 CUs about twice, a slice keeps >= 4 column tiles.
extern "C" int lsd_score_slices(int T, int Vp) {
  const int rb = (T + lsd::SC_BM - 1) / lsd::SC_BM, nt = (Vp + lsd::SC_BN - 1) / lsd::SC_BN;
  int s = (512 + rb - 1) / (rb > 0 ? rb : 1);
  if (s > nt / 4) s = nt / 4;
  return s < 1 ? 1 : s;
}

// xn [T, K] bf16 (row stride lda), w [Vp, K] bf16 (row stride ldw), targets [T];
// part: workspace of T * S * 4 floats, S = slices clamped to the column tiles
// (slices <= 0: lsd_score_slices).  K % 64 == 0, Vp % 64 == 0, 1 <= V <= Vp,
// rows 16-byte aligned.
extern "C" hipError_t lsd_lm_head_score(const void* xn, long lda, const void* w, long ldw, const int* targets, int T,
                                        int V, int Vp, int K, int S, float* part, float* tok_lp, int* top_id,
                                        float* top_lp, hipStream_t st) {
  using namespace lsd;
  const int nt = (Vp + SC_BN - 1) / SC_BN;
  if (T < 0 || K < SC_BK || K % SC_BK != 0 || Vp < 64 || Vp % 64 != 0 || V < 1 || V > Vp || lda % 8 != 0 ||
      ldw % 8 != 0 || S < 1 || S > nt)
    return hipErrorInvalidValue;
  if (T == 0) return hipSuccess;
  hipLaunchKernelGGL(lm_head_score_kernel, dim3((T + SC_BM - 1) / SC_BM, S), dim3(256), 0, st, (const bf16*)xn, lda,
                     (const bf16*)w, ldw, targets, T, V, Vp, K, S, reinterpret_cast<f32x4*>(part));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lm_head_score_combine_kernel, dim3((T + 255) / 256), dim3(256), 0, st,
                     reinterpret_cast<const f32x4*>(part), T, S, tok_lp, top_id, top_lp);
  return hipGetLastError();
}
