// FP8-weight decode GEMM (W8A16):
//   C[M,N] = A[M,K] (bf16) . (Wq[N,K] (OCP E4M3 bytes) * scale[N])^T  (+ epilogue)
//
// The weight rows of `weight_dtype="fp8_e4m3"` (wquant.hip) go straight into
// the bf16 MFMA loop: no bf16 copy of the weight is ever written.  Activations
// stay bf16, the MFMA is v_mfma_f32_16x16x32_bf16, accumulation is fp32, and
// the row scale is applied to the fp32 accumulator -- the arithmetic of
// reference.linear over the dequantised weights.  Two kernels: gemm_w8_kernel
// (split-K, kind-0 plans; described here) and, further down, gemm_w8_d256_kernel
// (one workgroup per 256-row block x column tile, kind-2 / 3 plans).
//
// Work split, staging and combine are gemm_sk_kernel's (gemm.hip): grid =
// (column tiles of 64 NW, K splits, row blocks of 16 MT rows), 4 waves, wave w
// owns 16 NW columns; A through LDS by 16-byte LDS-DMA in swizzled 256-byte
// rows (one image per 128 k); W from HBM to VGPRs once; rounds double-buffered
// (two register sets, two LDS buffers) behind counted vmcnt waits; split-K
// partials published lane-major and summed by the last arriver in fixed split
// order; epilogue through an fp32 LDS tile (epilogue8 / store_pass) or straight
// from the accumulators (SiLU*up).  plan_gemm(kind = 0) sizes its grid,
// counters and workspace as it does for that kernel.
//
// What differs is the unit of K, a block of 64:
//   * Lane (r = lane & 15, g = lane >> 4) loads 16 BYTES of W row
//     n_w + 16 ns + r: k = 64 blk + 16 g .. + 15.  The low 8 bytes are the B
//     fragment of MFMA step s = 0 of the block, the high 8 bytes that of s = 1.
//   * A dot product may visit k in any order as long as both operands agree, so
//     in step s lane group g reads the A fragment holding k = 64 blk + 16 g +
//     8 s .. + 7: 16-byte chunk 8 blk + 2 g + s of the row, i.e. chunk
//     8 (blk & 1) + 2 g + s of the block's 256-byte image row, through the same
//     ^ (row & 15) swizzle the DMA wrote it with.  Bank check: within one
//     ds_read_b128 the 16 lanes of a group read rows 16 mt + r, r = 0..15, at
//     chunk c ^ r with c fixed, so they hit 16 distinct 16-byte chunks, and as a
//     row is exactly 64 banks wide those are all 64 banks once: conflict-free,
//     as in the bf16 kernel (only which c a group uses has changed).
//   * v_cvt_scalef32_pk_bf16_fp8 with scale 1.0 turns two bytes into one exact
//     bf16x2; four of them make the B fragment, shared by the MT row tiles.
//     Step j + 1's fragment is converted while step j's MFMAs issue; nothing is
//     converted a round ahead (that would give back the registers FP8 saved).
//     Blocks past the round end multiply a zeroed fragment (byte 0 is +0.0).
//   * K % 64 == 0; splits cut at kb = (K / 64) split / S, in blocks.
//
// Round depth (blocks of 64 k per round).  A weight register holds twice the k
// it held, so the same registers would fetch twice the k per round -- but the
// bf16 kernel's two A images already fill 64 KiB of LDS for MT = 2, 4, 8, and
// twice the k per round doubles them.  So only MT = 1 (32 KiB there) doubles its
// round to 1024 k and keeps the bf16 kernel's 256 weight bytes per lane per
// round in flight; every other MT keeps the bf16 kernel's k per round (512 /
// 256 / 128), its LDS, and half its weight registers and bytes in flight.
//
// Row scale: every accumulator acc[mt][ns] of a lane belongs to one column
// n = n_w + 16 ns + r, so scale[n] is one register per ns, fetched at kernel
// start ahead of the weight stream.  It multiplies the accumulator exactly
// once, at one line of code that is three sites of the data flow:
//   * S = 1: ahead of the LDS C tile / epilogue4;
//   * in-kernel combine: raw partials are published, the last arriver scales
//     the fixed-order sum;
//   * EPI_SLAB (the next norm sums the slabs and knows no scales): every
//     split scales its own partial before storing it.
// Gate and up columns of SiLU*up and RoPE's partner column carry their own
// scales, so the epilogues (gemm_epilogue.h) run unchanged behind it.
//
// Compiled without the packed fp32 VALU forms (LSD_NO_PK_F32, common.h), hence
// block_sync() for __syncthreads() and always-inline lambdas.
#include "common.h"
#include "gemm_params.h"
#include "gemm_plan.h"
#include "api.h"
#include "gemm_epilogue.h"
#include "gemm_combine.h"

namespace lsd {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// 64-k blocks per round
template <int MT, int NW>
constexpr int w8_round_blocks() {
  return MT == 1 ? (NW == 1 ? 16 : 8) : (MT == 2 ? 8 : (MT <= 4 ? 4 : 2));
}

// bytes 8 s .. 8 s + 7 of a lane's 16 -> the bf16 B fragment of step s
template <int S>
__device__ __forceinline__ bf16x8 w8_frag(u32x4 w) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[2 * S], 1.0f, false);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[2 * S], 1.0f, true);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[2 * S + 1], 1.0f, false);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[2 * S + 1], 1.0f, true);
  const bf16x4 lo = __builtin_shufflevector(p0, p1, 0, 1, 2, 3);
  const bf16x4 hi = __builtin_shufflevector(p2, p3, 0, 1, 2, 3);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// 64-column tiles hold 2 workgroups per CU (2 waves per SIMD: at most 256 registers)
template <int MT, int NW, int EPI>
__global__ LSD_NO_PK_F32 __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NW == 1 ? 2 : 1)))
void gemm_w8_kernel(GemmParams p, const float* __restrict__ wscale,
                                                                     int* __restrict__ cnt, float* __restrict__ ws) {
  constexpr int ROWS = MT * 16;
  constexpr int CHUNK_BYTES = ROWS * 256;  // one [ROWS][128 k] bf16 image = two blocks
  constexpr int BNB = 64 * NW;
  constexpr int BLK = w8_round_blocks<MT, NW>();
  constexpr int STEPS = 2 * BLK;  // 32-k MFMA steps per round
  constexpr int NCHUNK = BLK / 2;
  constexpr int BUF_BYTES = NCHUNK * CHUNK_BYTES;
  static_assert(BLK % 2 == 0 && 2 * BUF_BYTES <= 64 * 1024, "two A images within 64 KiB (2 blocks / CU)");
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF_BYTES + 16];
  int* s_flag = reinterpret_cast<int*>(smem + 2 * BUF_BYTES);

  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int split = blockIdx.y, S = p.splits;
  const int rb0 = blockIdx.z * ROWS;
  const int tile = blockIdx.x;
  const int tile_id = blockIdx.z * gridDim.x + tile;  // ticket / workspace index
  const int n_w = tile * BNB + w * 16 * NW;
  const int KT = p.K >> 6;  // 64-k blocks
  const int kb = (int)((long)KT * split / S), ke = (int)((long)KT * (split + 1) / S);

  // p.W / p.ldw: byte pointer and byte stride.  A partial last tile re-reads
  // row N-1 (and its scale); those columns are never stored.
  const unsigned char* wrow[NW];
  float sc[NW];
#pragma unroll
  for (int ns = 0; ns < NW; ++ns) {
    const int n = min(n_w + 16 * ns + r, p.N - 1);
    wrow[ns] = reinterpret_cast<const unsigned char*>(p.W) + (long)n * p.ldw + g * 16;
    sc[ns] = wscale[n];
  }

  f32x4 acc[MT][NW];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int ns = 0; ns < NW; ++ns) acc[mt][ns] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Every round issues the same number of loads per thread (partial rounds
  // re-load clamped addresses), so "round rd has landed" is vmcnt(LOADS) once
  // round rd + 1 is issued; raw s_barrier, so the next round's DMA stays in flight.
  constexpr int LOADS = BLK * NW + NCHUNK * MT;
  static_assert(LOADS <= 63, "vmcnt holds at most 63 outstanding loads");
  constexpr int WAIT_PREV = vmcnt_imm(LOADS);
  constexpr int WAIT_ALL = vmcnt_imm(0);
  const int nrounds = (ke - kb + BLK - 1) / BLK;

  auto issue = [&](int rd, u32x4 (&wv)[BLK][NW], char* buf) LSD_INL {
    const int k0 = kb + rd * BLK;
    const int nb = min(BLK, ke - k0);
    // no per-load guard: blocks past the round end re-load the last valid one
#pragma unroll
    for (int j = 0; j < BLK; ++j)
#pragma unroll
      for (int ns = 0; ns < NW; ++ns)
        wv[j][ns] = *reinterpret_cast<const u32x4*>(wrow[ns] + (long)(k0 + min(j, nb - 1)) * 64);
    // A: MT * 4 wave-instructions (1 KiB = 4 rows of 256 B) per 128-k image
#pragma unroll
    for (int i = 0; i < NCHUNK * MT; ++i) {
      const int inst = w + 4 * i;
      const int c = inst / (MT * 4), q = inst % (MT * 4);
      const int row = q * 4 + (lane >> 4);
      const int lch = (lane & 15) ^ (row & 15);
      const int kk = min((k0 + min(c * 2, nb - 1)) * 64 + lch * 8, p.K - 8);
      glds16(p.A + (long)min(rb0 + row, p.M - 1) * p.lda + kk, buf + c * CHUNK_BYTES + q * 1024);
    }
  };
  auto compute = [&](int rd, u32x4 (&wv)[BLK][NW], const char* buf) LSD_INL {
    const int nb = min(BLK, ke - (kb + rd * BLK));
    const int nst = 2 * nb;
    // step t = 2 blk + s: image t / 4, chunk 8 (blk & 1) + 2 g + s
    auto read_a = [&](int t, bf16x8 (&a)[MT]) LSD_INL {
      const char* img = buf + (t >> 2) * CHUNK_BYTES;
      const int lch = ((t >> 1) & 1) * 8 + 2 * g + (t & 1);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int row = mt * 16 + r;
        a[mt] = *reinterpret_cast<const bf16x8*>(img + row * 256 + ((lch ^ (row & 15)) << 4));
      }
    };
    // B fragments of step t; blocks past the round end are zero bytes (+0.0)
    auto frag = [&](int t, bf16x8 (&b)[NW]) LSD_INL {
      const int j = t >> 1;
#pragma unroll
      for (int ns = 0; ns < NW; ++ns) {
        const u32x4 z = {0u, 0u, 0u, 0u};
        const u32x4 wb = j < nb ? wv[j][ns] : z;
        b[ns] = (t & 1) ? w8_frag<1>(wb) : w8_frag<0>(wb);
      }
    };
    bf16x8 a_cur[MT], b_cur[NW];
    read_a(0, a_cur);
    frag(0, b_cur);
#pragma unroll
    for (int t = 0; t < STEPS; ++t) {
      bf16x8 a_nxt[MT], b_nxt[NW];
      read_a(min(t + 1, nst - 1), a_nxt);
      if (t + 1 < STEPS) frag(t + 1, b_nxt);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int ns = 0; ns < NW; ++ns) acc[mt][ns] = mfma16(a_cur[mt], b_cur[ns], acc[mt][ns]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a_cur[mt] = a_nxt[mt];
      if (t + 1 < STEPS) {
#pragma unroll
        for (int ns = 0; ns < NW; ++ns) b_cur[ns] = b_nxt[ns];
      }
    }
    // every wave's reads of `buf` retire before anyone re-fills it
    __builtin_amdgcn_s_waitcnt(LGKM0_SK);
    __builtin_amdgcn_s_barrier();
  };
  auto body_more = [&](int rd, u32x4 (&cur)[BLK][NW], char* cbuf, u32x4 (&nxt)[BLK][NW], char* nbuf) LSD_INL {
    issue(rd + 1, nxt, nbuf);
    __builtin_amdgcn_s_waitcnt(WAIT_PREV);  // this thread's round-rd loads landed
    __builtin_amdgcn_s_barrier();           // ... and every other wave's A DMA
    compute(rd, cur, cbuf);
  };
  auto body_last = [&](int rd, u32x4 (&cur)[BLK][NW], char* cbuf) LSD_INL {
    __builtin_amdgcn_s_waitcnt(WAIT_ALL);
    __builtin_amdgcn_s_barrier();
    compute(rd, cur, cbuf);
  };

  u32x4 wv0[BLK][NW], wv1[BLK][NW];
  char* buf0 = smem;
  char* buf1 = smem + BUF_BYTES;
  int rd = 0;
  if (nrounds > 0) issue(0, wv0, buf0);
  for (; rd + 2 < nrounds; rd += 2) {
    body_more(rd, wv0, buf0, wv1, buf1);
    body_more(rd + 1, wv1, buf1, wv0, buf0);
  }
  if (nrounds - rd == 2) {
    body_more(rd, wv0, buf0, wv1, buf1);
    body_last(rd + 1, wv1, buf1);
  } else if (nrounds - rd == 1) {
    body_last(rd, wv0, buf0);
  }

  if (S > 1 && EPI != EPI_SLAB) {
    // RAW partials are combined (gemm_combine.h); base: wave w's block of
    // MT * NW accumulators, 64 lanes each (1024 B apart); <= 128 VGPRs in flight
    constexpr int RG = (32 / (MT * NW)) < 4 ? 4 : ((32 / (MT * NW)) > 16 ? 16 : 32 / (MT * NW));
    if (!splitk_combine<256, 1024, RG>(acc, ws, cnt, tile_id, split, S, ((w * MT * NW) * 64 + lane) * 16, s_flag))
      return;
  }

  // The row scale, once: the whole sum (S = 1, or the last arriver's), or this
  // split's own partial on its way to a slab.
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int ns = 0; ns < NW; ++ns) acc[mt][ns] *= sc[ns];

  // Epilogue through an fp32 [ROWS][BNB] LDS tile (the last round ended with
  // every DMA drained and a barrier), row-contiguous 16-byte stores; SiLU*up
  // pairs two accumulator tiles of one lane instead.
  constexpr int CLD = BNB + 4;
  if constexpr (EPI != EPI_SILU_MUL) {
    // always: epilogue4's 16-column sub-tiles would overrun a last tile of 8 live columns
    static_assert(ROWS * CLD * 4 <= 2 * BUF_BYTES, "C tile fits the A buffers");
    sk_tile_store<EPI, ROWS, BNB, 256>(p, acc, smem, rb0, tile * BNB, split);
  } else {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int ns = 0; ns < NW; ns += 2)  // N % (64 NW) == 0 (host-checked): no partial tile
        epilogue4<EPI>(p, rb0 + mt * 16 + 4 * g, n_w + 16 * ns + r, acc[mt][ns], acc[mt][ns + 1], 0);
  }
}

// ---------------------------------------------------------------------------
// FP8-weight all-rows decode GEMM, 129-1024 rows: one workgroup owns every row
// of a 256-row block x BN columns
// ---------------------------------------------------------------------------
// The split-K kernel above reads A once per 128-row block and column tile and
// is LDS-bound from MT = 2 on; the bf16 path covers this row range with
// gemm_d256_kernel (gemm.hip).  This is that kernel's work split on E4M3
// weight rows: plan_gemm(kind 2 / 3) sizes grid, counters and workspace for
// both (512 threads, tile = remapped id / S, column-major over 256-row blocks,
// k-step 64, S-way split K, lane-major partials of 256 x BN floats per tile).
//
// W through LDS as FP8, staged 128 k at a time.  An E4M3 row is 64 B per
// k-step, half a cache line, so W is staged once per PAIR of k-steps: one
// LDS-DMA wave-instruction (64 lanes x 16 B) reads 8 rows x 128 B, full lines.
// The LDS holds two rings in ONE array: SLOTS A images of [256][64 k] bf16
// (32 KiB, gemm_d256's) and NWS = SLOTS / 2 + 1 W images of [BN][128 k] bytes
// (BN x 128 B = the bytes of ONE bf16 k-step image, for two steps).  With
// D = SLOTS - 1 steps in flight, the pair issued with step 2P meets the pairs
// of steps 2P - D .. 2P - 1 alive: ceil(D / 2) + 1 = NWS images.  LDS per
// (BN, SLOTS): (64,2) 80, (64,3) 112, (64,4) 152, (128,2) 96 -> 132 (C tile),
// (128,3) 128 -> 132 KiB.  A pair's second half past the end of K re-reads the
// last block (never multiplied); a split's odd last step wastes 64 B per row.
// Steps are counted from the split's first, so even steps issue 4 + BN / 64
// DMAs per thread and odd steps 4: the counted vmcnt of step t allows the
// loads of the `later` steps after it, by the parity of t.  One raw barrier
// per step, as in gemm_d256_kernel (its comments say why).
//
// LDS images, both conflict-free.  Both are 128-byte rows of eight 16-byte
// chunks with chunk c of row `row` at position c ^ ((row >> 1) & 7) (the DMA
// swizzles the SOURCE address, the reads apply the same XOR: lds_frag's
// image).  A ds_read_b128 serves 16 lanes at a time, lanes r = 0..15 of one
// group g: rows 16 t + r at one logical chunk c.  16-byte bank group =
// 8 (row & 1) + (c ^ (row >> 1) & 7); over r, (row >> 1) & 7 takes every value
// once per parity of row, so the 16 lanes hit 16 distinct bank groups.
//   * A, MFMA step s of the k-step: chunk 2 g + s (k = 16 g + 8 s .. + 7);
//   * W: chunk 4 h + g of the pair's half h = 16 BYTES = k 16 g .. + 15 of the
//     step: low 8 bytes are step 0's B fragment, high 8 step 1's -- the
//     k-permutation of gemm_w8_kernel, A and B agree on it.
//
// Wave grid 4 (M) x 2 (N): wave w owns rows 64 (w >> 1) .. + 63 x columns
// BN / 2 (w & 1) .. -- 4 x BN / 32 accumulator tiles, as many registers as the
// bf16 kernel's 8 x 1 grid (2 x BN / 16), so the lane-major partial tile keeps
// its size.  Per MFMA step a wave converts BN / 32 fragments (4 converts
// each) for 4 x BN / 32 MFMAs: ONE v_cvt_scalef32_pk_bf16_fp8 PER MFMA (8 x 1
// would convert the whole W tile in every wave: 2 per MFMA), and per k-step
// 8 + BN / 32 ds_read_b128 (bf16 kernel: 4 + BN / 4).  A bf16 LDS image
// converted once would cost an LDS write, a second barrier per step and the
// bf16 kernel's LDS bytes again.  (64, 2), at 127 VGPRs and 80 KiB, happens to
// let two workgroups share a CU; no default reaches it (d256_slots = 3) and
// nothing here is tuned for that.  Step 1's fragments are converted ahead of
// step 0's MFMAs, which cover them; step 0's own converts are covered by the
// SIMD's other wave (a step's bytes only become visible at its barrier).
//
// Row scale: one register per column tile of the lane, applied at the three
// sites of gemm_w8_kernel.  Combine: gemm_d256_kernel's (fixed split order,
// counter re-armed by the last arriver).
template <int BN, int SLOTS>
constexpr int w8d_smem() {
  constexpr int ring = SLOTS * 256 * 128 + (SLOTS / 2 + 1) * BN * 128;
  return ring > 256 * (BN + 4) * 4 ? ring : 256 * (BN + 4) * 4;
}

template <int EPI, int BN, int SLOTS>
__global__ LSD_NO_PK_F32 __launch_bounds__(512)
void gemm_w8_d256_kernel(GemmParams p, const float* __restrict__ wscale, int* __restrict__ cnt,
                         float* __restrict__ ws) {
  constexpr int NJ = BN / 32;            // 16-column MFMA tiles per wave
  constexpr int A_BYTES = 256 * 128;     // [256][64 k] bf16
  constexpr int W_BYTES = BN * 128;      // [BN][128 k] E4M3
  constexpr int NWS = SLOTS / 2 + 1;     // W images
  constexpr int LA = 4, LW = BN / 64;    // DMAs per thread: an A image, a W image
  constexpr int D = SLOTS - 1;           // k-steps in flight
  constexpr int SMEM = w8d_smem<BN, SLOTS>();
  static_assert(SLOTS >= 2 && SLOTS <= 4 && SLOTS * A_BYTES + NWS * W_BYTES <= 160 * 1024, "LDS rings");
  static_assert(2 * LA + LW <= 63, "vmcnt range");
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  int* s_flag = reinterpret_cast<int*>(smem);  // the rings are dead by then
  char* const wring = smem + SLOTS * A_BYTES;

  const int S = p.splits;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile = bid / S, split = bid % S;
  const int RB = (p.M + 255) / 256;
  const int rb = tile % RB, n0 = (tile / RB) * BN, m0 = rb * 256;
  const int KT = p.K >> 6;
  const int kb = (int)((long)KT * split / S), ke = (int)((long)KT * (split + 1) / S);
  const int nst = ke - kb;
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wr = w >> 1, wc = w & 1;

  // a partial last tile re-reads row N - 1 and its scale; never stored
  float sc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) sc[j] = wscale[min(n0 + wc * (BN / 2) + j * 16 + r, p.N - 1)];

  f32x4 acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // step t (from the split's first): A image into slot `slot`; even t: the W
  // image of steps t, t + 1.  Wave-instruction = 1 KiB = 8 rows of 128 B.
  const int srow = lane >> 3;
  auto issue = [&](int t, int slot) LSD_INL {
#pragma unroll
    for (int q = 0; q < LA; ++q) {
      const int inst = w * LA + q, row = inst * 8 + srow;
      const int lch = (lane & 7) ^ ((row >> 1) & 7);
      glds16(p.A + (long)min(m0 + row, p.M - 1) * p.lda + (kb + t) * 64 + lch * 8,
             smem + slot * A_BYTES + inst * 1024);
    }
    if (t & 1) return;
    char* wd = wring + ((t >> 1) % NWS) * W_BYTES;
#pragma unroll
    for (int q = 0; q < LW; ++q) {
      const int inst = w * LW + q, row = inst * 8 + srow;
      const int lch = (lane & 7) ^ ((row >> 1) & 7);
      const int blk = min(kb + t + (lch >> 2), KT - 1);
      glds16(reinterpret_cast<const unsigned char*>(p.W) + (long)min(n0 + row, p.N - 1) * p.ldw + blk * 64 +
                 (lch & 3) * 16,
             wd + inst * 1024);
    }
  };
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (d < nst) issue(d, d);
  int slot = 0;
  for (int t = 0; t < nst; ++t) {
    // this thread's DMAs of step t landed; those of the later steps stay in flight
    const int later = min(D - 1, nst - 1 - t);
    if (D >= 3 && later >= 2) __builtin_amdgcn_s_waitcnt(vmcnt_imm(2 * LA + LW));
    else if (later == 1 && (t & 1)) __builtin_amdgcn_s_waitcnt(vmcnt_imm(LA + LW));
    else if (later == 1) __builtin_amdgcn_s_waitcnt(vmcnt_imm(LA));
    else __builtin_amdgcn_s_waitcnt(vmcnt_imm(0));
    // publishes every wave's DMA of step t AND proves every wave is done with
    // step t - 1, whose A slot (and, t even, W image) is refilled right after
    __builtin_amdgcn_s_barrier();
    if (t + D < nst) issue(t + D, slot == 0 ? SLOTS - 1 : slot - 1);
    const char* ta = smem + slot * A_BYTES;
    const char* tw = wring + ((t >> 1) % NWS) * W_BYTES;
    u32x4 wb[NJ];
    bf16x8 a0[4], a1[4], b0[NJ], b1[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int row = wc * (BN / 2) + j * 16 + r;
      wb[j] = *reinterpret_cast<const u32x4*>(tw + row * 128 + (((4 * (t & 1) + g) ^ ((row >> 1) & 7)) << 4));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wr * 64 + i * 16 + r;
      a0[i] = *reinterpret_cast<const bf16x8*>(ta + row * 128 + (((2 * g) ^ ((row >> 1) & 7)) << 4));
      a1[i] = *reinterpret_cast<const bf16x8*>(ta + row * 128 + (((2 * g + 1) ^ ((row >> 1) & 7)) << 4));
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) b0[j] = w8_frag<0>(wb[j]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) b1[j] = w8_frag<1>(wb[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = mfma16(a0[i], b0[j], acc[i][j]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = mfma16(a1[i], b1[j], acc[i][j]);
    slot = slot == SLOTS - 1 ? 0 : slot + 1;
  }

  if (S > 1 && EPI != EPI_SLAB) {
    // RAW partials are combined (gemm_combine.h); base: thread-major, 512
    // threads x 16 B (8192 B) per accumulator; 32 f32x4 (128 VGPRs) in flight
    if (!splitk_combine<512, 8192, 8 / NJ>(acc, ws, cnt, tile, split, S, threadIdx.x * 16, s_flag)) return;
  }

  // The row scale, once: the whole sum (S = 1, or the last arriver's), or this
  // split's own partial on its way to a slab.
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] *= sc[j];

  // Epilogue through the fp32 [256][BN + 4] C tile over the rings (every DMA
  // waited for; the barrier keeps it off a slot another wave still reads).
  constexpr int CLD = BN + 4;
  block_sync();
  float* ct = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        ct[(wr * 64 + i * 16 + 4 * g + q) * CLD + wc * (BN / 2) + j * 16 + r] = acc[i][j][q];
  block_sync();
  ct_store<EPI, BN, 256, 512>(p, ct, m0, n0, split);
}

template <int EPI>
static hipError_t launch_w8_d256(const GemmParams& p, const float* wscale, const GemmPlan& pl, int* cnt, float* ws,
                                 hipStream_t st) {
  const dim3 grid(pl.grid[0]), block(512);
#define LSD_W8D(BN_, SLOTS_)                                                                            \
  if (pl.tn == BN_ && pl.slots == SLOTS_) {                                                             \
    lsd_gemm_note_launch("w8d256<" #BN_ "," #SLOTS_ ">");                                               \
    hipLaunchKernelGGL((gemm_w8_d256_kernel<EPI, BN_, SLOTS_>), grid, block, 0, st, p, wscale, cnt, ws); \
    return hipGetLastError();                                                                           \
  }
  LSD_W8D(64, 2) LSD_W8D(64, 3) LSD_W8D(64, 4) LSD_W8D(128, 2) LSD_W8D(128, 3)
#undef LSD_W8D
  return hipErrorInvalidValue;
}

template <int EPI, int NW>
static hipError_t launch_w8(const GemmParams& p, const float* wscale, const GemmPlan& pl, int* cnt, float* ws,
                            hipStream_t st) {
  const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]), block(256);
  static constexpr const char* tags[2][9] = {
      {"", "w8<1,1>", "w8<2,1>", "w8<3,1>", "w8<4,1>", "", "w8<6,1>", "", "w8<8,1>"},
      {"", "w8<1,2>", "w8<2,2>", "w8<3,2>", "w8<4,2>", "", "w8<6,2>", "", "w8<8,2>"}};
#define LSD_W8(MT_)                                                                             \
  case MT_:                                                                                     \
    lsd_gemm_note_launch(tags[NW - 1][MT_]);                                                    \
    hipLaunchKernelGGL((gemm_w8_kernel<MT_, NW, EPI>), grid, block, 0, st, p, wscale, cnt, ws); \
    return hipGetLastError();
  switch (pl.mt) {
    LSD_W8(1) LSD_W8(2) LSD_W8(3) LSD_W8(4) LSD_W8(6) LSD_W8(8)
  }
#undef LSD_W8
  return hipErrorInvalidValue;
}

template <int EPI>
static hipError_t launch_w8_epi(const GemmParams& p, const float* wscale, const GemmPlan& pl, int* cnt, float* ws,
                                hipStream_t st) {
  if constexpr (EPI == EPI_SILU_MUL)  // gate / up pairs: wide tiles only
    return pl.nw == 2 ? launch_w8<EPI, 2>(p, wscale, pl, cnt, ws, st) : hipErrorInvalidValue;
  else
    return pl.nw == 1 ? launch_w8<EPI, 1>(p, wscale, pl, cnt, ws, st) : hipErrorInvalidValue;
}

}  // namespace lsd

using namespace lsd;

// Shapes the kernel takes: whole 64-k blocks, 8-column store chunks (whole
// 128-column tiles for SiLU*up's gate / up pairs), any M >= 1.
extern "C" int lsd_gemm_w8_ok(int M, int N, int K, int epi) {
  if (M < 1 || N < 8 || K < 64 || K % 64 != 0 || epi < EPI_BF16 || epi > EPI_QKV) return 0;
  return epi == EPI_SILU_MUL ? N % 128 == 0 : N % 8 == 0;
}

// Launches a plan of plan_gemm() on an FP8-weight kernel: kind 0 (GK_SK) on
// gemm_w8_kernel, kind 2 / 3 (GK_D256) on gemm_w8_d256_kernel.  p->W holds
// E4M3 bytes, p->ldw is the row stride in bytes.  No launch on a refusal.
extern "C" hipError_t lsd_gemm_w8(const GemmParams* p, const float* wscale, const GemmPlan* plan, int* cnt, float* ws,
                                  hipStream_t st) {
  const GemmPlan& pl = *plan;
  const bool rows = pl.kernel == GK_D256;
  if (!pl.valid || (rows ? pl.block != 512 : pl.kernel != GK_SK || pl.block != 256))
    return hipErrorInvalidValue;
  if (pl.M != p->M || pl.N != p->N || pl.K != p->K || pl.splits != p->splits) return hipErrorInvalidValue;
  if (!lsd_gemm_w8_ok(p->M, p->N, p->K, pl.epi) || p->splits > p->K / 64) return hipErrorInvalidValue;
  if (wscale == nullptr || p->ldw % 16 != 0 || p->ldw < p->K) return hipErrorInvalidValue;
  if (pl.combine_tiles > 0 && (cnt == nullptr || ws == nullptr)) return hipErrorInvalidValue;
  if (rows && pl.combine_tiles > 0 && pl.tile_floats != 256L * pl.tn) return hipErrorInvalidValue;
  return dispatch_epi(pl.epi, [&](auto e) {
    constexpr int EPI = decltype(e)::value;
    return rows ? launch_w8_d256<EPI>(*p, wscale, pl, cnt, ws, st) : launch_w8_epi<EPI>(*p, wscale, pl, cnt, ws, st);
  });
}
