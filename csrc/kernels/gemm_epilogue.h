// The fused GEMM epilogues and the LDS-DMA helper shared by the GEMM kernels
// (gemm.hip, gemm_w8.hip): bias, gelu_new, silu(gate)*up, fp32 store (+ segment
// maxima), residual add, split-K slab, and the QKV epilogue that applies RoPE
// and scatters K/V into the bf16 or FP8 KV cache.
#pragma once
#include "common.h"
#include "gemm_params.h"
#include "gemm_plan.h"

namespace lsd {

// (head, dim) of column c inside the q / k / v block: shifts and a mask for the
// power-of-two head dims of every model here (a wave-uniform branch; integer
// division by a runtime divisor is a ~40-instruction sequence per call, paid
// for every 16-byte chunk of the prefill QKV epilogue)
__device__ __forceinline__ void hd_split(int hd, int c, int& head, int& d) {
  if ((hd & (hd - 1)) == 0) {
    head = c >> __builtin_ctz(hd);
    d = c & (hd - 1);
  } else {
    head = c / hd;
    d = c % hd;
  }
}

// Stores the 4 accumulator values of one 16x16 MFMA tile owned by this lane:
// column n, rows row0 + i.  All lanes of the wave must call it (RoPE uses a
// cross-lane exchange).  `v2` carries the paired tile for EPI_SILU_MUL.
template <int EPI>
__device__ __forceinline__ void epilogue4(const GemmParams& p, int row0, int n, f32x4 v, f32x4 v2,
                                          int split) {
  if constexpr (EPI == EPI_SLAB) {
    if (p.slab_bf16) {
      bf16* s = reinterpret_cast<bf16*>(p.slab) + (long)split * p.M * p.N;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (row0 + i < p.M) s[(long)(row0 + i) * p.N + n] = f2bf(v[i]);
      return;
    }
    float* s = p.slab + (long)split * p.M * p.N;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (row0 + i < p.M) s[(long)(row0 + i) * p.N + n] = v[i];
    return;
  }
  if constexpr (EPI == EPI_F32) {
    float* o = reinterpret_cast<float*>(p.out);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (row0 + i < p.M) o[(long)(row0 + i) * p.ldo + n] = v[i];
    return;
  }
  const float b = p.bias ? bf2f(p.bias[n]) : 0.f;
  if constexpr (EPI == EPI_RESID) {
    float* x = reinterpret_cast<float*>(p.out);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (row0 + i < p.M) x[(long)(row0 + i) * p.ldo + n] += v[i] + b;
    return;
  }
  if constexpr (EPI == EPI_BF16 || EPI == EPI_GELU) {
    bf16* o = reinterpret_cast<bf16*>(p.out);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float y = v[i] + b;
      if constexpr (EPI == EPI_GELU) y = gelu_new(y);
      if (row0 + i < p.M) o[(long)(row0 + i) * p.ldo + n] = f2bf(y);
    }
    return;
  }
  if constexpr (EPI == EPI_SILU_MUL) {
    // n is the gate column inside an interleaved [gate16 | up16] 32-row block
    bf16* o = reinterpret_cast<bf16*>(p.out);
    const int col = (n >> 5) * 16 + (n & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (row0 + i < p.M) o[(long)(row0 + i) * p.ldo + col] = f2bf(silu(v[i]) * v2[i]);
    return;
  }
  if constexpr (EPI == EPI_QKV) {
    float y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = v[i] + b;
    const int qk = p.q_size + p.kv_size;
    if (p.rope != nullptr && n < qk) {  // uniform per 16-column tile (q/k sizes are multiples of hd)
      int hh, d;
      hd_split(p.hd, n < p.q_size ? n : n - p.q_size, hh, d);
      const int half = p.hd >> 1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float partner = shfl_xor(y[i], 1);
        const int m = min(row0 + i, p.M - 1);
        const int pos = p.tpos[m];
        const float* cs = p.rope + ((long)pos * half + (d >> 1)) * 2;
        const float c = cs[0], s = cs[1];
        y[i] = (d & 1) ? (y[i] * c + partner * s) : (y[i] * c - partner * s);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = row0 + i;
      if (m >= p.M) continue;
      if (n < p.q_size) {
        reinterpret_cast<bf16*>(p.out)[(long)m * p.ldo + n] = f2bf(y[i]);
      } else {
        const int c = n < qk ? n - p.q_size : n - qk;
        int head, d;
        hd_split(p.hd, c, head, d);
        bf16* cache = n < qk ? p.kc : p.vc;
        const long idx = (((long)p.tslot[m] * p.n_kv + head) * p.max_seq + p.tpos[m]) * p.hd + d;
        if (p.kv_fp8) reinterpret_cast<unsigned char*>(cache)[idx] = fp8_enc(y[i]);  // uniform: FP8 E4M3 cache
        else cache[idx] = f2bf(y[i]);
      }
    }
  }
}

// Row-contiguous epilogue of 8 consecutive columns [n, n+8) of row m (the
// tiled kernel's LDS-transposed output): every store is one 16-byte vector.
// n % 8 == 0; bias / out / x / caches are 16-byte aligned (host-checked).
//
// Split in three so a store pass can issue the global reads of ALL its chunks
// before its first store (store_pass below): CDNA4's vmcnt counts loads and
// stores in one in-order counter, so a load issued after a store is waited for
// together with that store, and a chunk-at-a-time loop (load bias / residual,
// wait, compute, store) serialises one store round trip per chunk (the p8
// epilogue: 16 per thread, most of its 6-12 us).
//   epi8_pre  -- bias, residual x, QKV position / slot      (independent loads)
//   epi8_pre2 -- QKV RoPE (cos, sin) of that position        (dependent loads)
//   epi8_post -- the math and the stores
// s_waitcnt immediate for vmcnt(n) alone (gfx9 layout: vmcnt[3:0] | vmcnt[5:4] << 14)
constexpr int vmcnt_imm(int n) { return (n & 0xF) | ((n >> 4) << 14) | (0x7 << 4) | (0xF << 8); }

struct Epi8Pre {
  bf16x8 b;
  f32x4 x0, x1, cs0, cs1;
  int pos, slot;
};

template <int EPI>
__device__ __forceinline__ void epi8_pre(const GemmParams& p, int m, int n, Epi8Pre& e) {
  if constexpr (EPI == EPI_SLAB || EPI == EPI_F32 || EPI == EPI_SILU_MUL) return;
  if (p.bias) e.b = ld8(p.bias + n);
  if constexpr (EPI == EPI_RESID) {
    const f32x4* x = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.out) + (long)m * p.ldo + n);
    e.x0 = x[0];
    e.x1 = x[1];
  }
  if constexpr (EPI == EPI_QKV) {
    e.pos = p.tpos[m];
    e.slot = n >= p.q_size ? p.tslot[m] : 0;
  }
}

template <int EPI>
__device__ __forceinline__ void epi8_pre2(const GemmParams& p, int n, Epi8Pre& e) {
  if constexpr (EPI == EPI_QKV) {
    if (p.rope != nullptr && n < p.q_size + p.kv_size) {
      int hh, d0;
      hd_split(p.hd, n < p.q_size ? n : n - p.q_size, hh, d0);
      const f32x4* cs = reinterpret_cast<const f32x4*>(p.rope + ((long)e.pos * (p.hd >> 1) + (d0 >> 1)) * 2);
      e.cs0 = cs[0];
      e.cs1 = cs[1];
    }
  }
}

template <int EPI>
__device__ __forceinline__ void epi8_post(const GemmParams& p, int m, int n, const float* v, int split,
                                          const Epi8Pre& e) {
  if constexpr (EPI == EPI_SLAB) {
    if (p.slab_bf16) {  // half the slab bytes for the GEMM to write and the norm to read
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2bf(v[j]);
      st8(reinterpret_cast<bf16*>(p.slab) + (long)split * p.M * p.N + (long)m * p.N + n, o);
      return;
    }
  }
  if constexpr (EPI == EPI_SLAB || EPI == EPI_F32) {
    float* o = EPI == EPI_SLAB ? p.slab + (long)split * p.M * p.N + (long)m * p.N + n
                               : reinterpret_cast<float*>(p.out) + (long)m * p.ldo + n;
    reinterpret_cast<f32x4*>(o)[0] = f32x4{v[0], v[1], v[2], v[3]};
    reinterpret_cast<f32x4*>(o)[1] = f32x4{v[4], v[5], v[6], v[7]};
    if constexpr (EPI == EPI_F32) {
      // lm_head: the chunk's maximum for the sampler (one float per 8 logits)
      if (p.segmax) {
        const float m01 = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
        const float m23 = fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7]));
        p.segmax[(long)m * p.ldseg + (n >> 3)] = fmaxf(m01, m23);
      }
    }
    return;
  }
  float y[8];
  if (p.bias) {
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = v[j] + bf2f(e.b[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = v[j];
  }
  if constexpr (EPI == EPI_RESID) {
    f32x4* x = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.out) + (long)m * p.ldo + n);
    f32x4 x0 = e.x0, x1 = e.x1;
#pragma unroll
    for (int j = 0; j < 4; ++j) { x0[j] += y[j]; x1[j] += y[4 + j]; }
    x[0] = x0;
    x[1] = x1;
    return;
  }
  if constexpr (EPI == EPI_BF16 || EPI == EPI_GELU) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(EPI == EPI_GELU ? gelu_new(y[j]) : y[j]);
    st8(reinterpret_cast<bf16*>(p.out) + (long)m * p.ldo + n, o);
    return;
  }
  if constexpr (EPI == EPI_QKV) {
    const int qk = p.q_size + p.kv_size;
    if (p.rope != nullptr && n < qk) {  // adjacent (even, odd) pairs rotate together
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 t = h ? e.cs1 : e.cs0;  // (cos, sin) of pairs d0/2 + 2h, d0/2 + 2h + 1
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const float c = t[2 * q], sn = t[2 * q + 1];
          const float a = y[4 * h + 2 * q], b = y[4 * h + 2 * q + 1];
          y[4 * h + 2 * q] = a * c - b * sn;
          y[4 * h + 2 * q + 1] = b * c + a * sn;
        }
      }
    }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(y[j]);
    if (n < p.q_size) {
      st8(reinterpret_cast<bf16*>(p.out) + (long)m * p.ldo + n, o);
    } else {
      const int c = n < qk ? n - p.q_size : n - qk;
      bf16* cache = n < qk ? p.kc : p.vc;
      int head, d;
      hd_split(p.hd, c, head, d);
      const long idx = (((long)e.slot * p.n_kv + head) * p.max_seq + e.pos) * p.hd + d;
      if (p.kv_fp8)  // uniform: FP8 E4M3 cache, the 8 columns are one 8-byte store (from fp32, not via bf16)
        *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned char*>(cache) + idx) = fp8x8_from_f32(y);
      else
        st8(cache + idx, o);
    }
  }
}

template <int EPI>
__device__ __forceinline__ void epilogue8(const GemmParams& p, int m, int n, const float* v, int split) {
  Epi8Pre e;
  epi8_pre<EPI>(p, m, n, e);
  epi8_pre2<EPI>(p, n, e);
  epi8_post<EPI>(p, m, n, v, split, e);
}

// One store pass over the 8-column row chunks c = threadIdx.x + i * NT (i < NCH,
// c < nchunks) of an fp32 C image in LDS.  at(c, m, n, src) maps a chunk to its
// output row / column and its 8 floats in LDS (false: out of range).  Every
// global read of the thread's chunks is issued before its first store (see
// epi8_pre); SiLU·up pairs each gate chunk with the up chunk 16 columns right
// (interleaved [gate16 | up16] 32-column blocks in one tile: `up` = src + UPOFF).
template <int EPI, int NCH, int NT, class At>
__device__ __forceinline__ void store_pass(const GemmParams& p, int nchunks, int split, At at) {
  Epi8Pre e[NCH];
  int mm[NCH], nn[NCH];
  const float* sp[NCH];
  bool ok[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (int)threadIdx.x + i * NT;
    ok[i] = c < nchunks && at(c, mm[i], nn[i], sp[i]);
    if (ok[i]) epi8_pre<EPI>(p, mm[i], nn[i], e[i]);
  }
  // one explicit wait for all of them: the compiler's own waits after the
  // branchy chunk bodies below would be vmcnt(0) per chunk (joins lose count),
  // i.e. one store round trip per chunk again
  __builtin_amdgcn_s_waitcnt(vmcnt_imm(0));
  if constexpr (EPI == EPI_QKV) {
    if (p.rope != nullptr) {  // wave-uniform: GPT-2 has no RoPE loads to wait for
#pragma unroll
      for (int i = 0; i < NCH; ++i)
        if (ok[i]) epi8_pre2<EPI>(p, nn[i], e[i]);
      __builtin_amdgcn_s_waitcnt(vmcnt_imm(0));
    }
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    if (!ok[i]) continue;
    const f32x4 lo = *reinterpret_cast<const f32x4*>(sp[i]);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(sp[i] + 4);
    const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    epi8_post<EPI>(p, mm[i], nn[i], v, split, e[i]);
  }
}

// lambdas that must inline into a kernel built with LSD_NO_PK_F32 (common.h)
#define LSD_INL __attribute__((always_inline))

// Store loop of an fp32 [TM][TN + 4] C tile in LDS: NT threads, one 8-column
// row chunk each per pass, 16-byte global stores (epilogue8).  SiLU*up:
// interleaved [gate16 | up16] 32-column blocks, a gate chunk pairs with the up
// chunk 16 columns right (same tile: TN % 32 == 0).
template <int EPI, int TN, int TM, int NT>
__device__ __forceinline__ void ct_store(const GemmParams& p, const float* ct, int m0, int n0, int split) {
  constexpr int CLD = TN + 4;
  constexpr int CPR = TN / 8;  // 8-column chunks per row
  if constexpr (EPI != EPI_SILU_MUL) {
    store_pass<EPI, (TM * CPR + NT - 1) / NT, NT>(
        p, TM * CPR, split, [&](int c, int& m, int& n, const float*& src) LSD_INL {
          const int row = c / CPR, ch = c % CPR;
          m = m0 + row;
          n = n0 + ch * 8;
          src = ct + row * CLD + ch * 8;
          return m < p.M && n < p.N;
        });
  } else {
    for (int c = threadIdx.x; c < TM * CPR; c += NT) {
      const int row = c / CPR, n = n0 + (c % CPR) * 8, m = m0 + row;
      if (m >= p.M || n >= p.N) continue;
      const float* src = ct + row * CLD + (c % CPR) * 8;
      const f32x4 lo = *reinterpret_cast<const f32x4*>(src);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(src + 4);
      float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      if ((c & 3) >= 2) continue;  // up chunks are read by their gate chunk (CPR % 4 == 0)
      const float* up = src + 16;
      const f32x4 ulo = *reinterpret_cast<const f32x4*>(up);
      const f32x4 uhi = *reinterpret_cast<const f32x4*>(up + 4);
      const float u[8] = {ulo[0], ulo[1], ulo[2], ulo[3], uhi[0], uhi[1], uhi[2], uhi[3]};
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(silu(v[e]) * u[e]);
      st8(reinterpret_cast<bf16*>(p.out) + (long)m * p.ldo + (n >> 5) * 16 + (n & 15), o);
    }
  }
}

// C tile of the split-K pair (gemm_sk_kernel, gemm_w8_kernel): NT / 64 waves
// side by side, wave w owns columns [w, w + 1) * BNB / (NT / 64) of every row.
// The MFMA layout gives a lane 4 rows x 1 column; transposed through the fp32
// [ROWS][BNB + 4] tile (4 rows x 16 columns hit 64 distinct banks), every
// global store is a row-contiguous 16-byte vector.  The caller's LDS is idle.
template <int EPI, int ROWS, int BNB, int NT>
__device__ __forceinline__ void sk_tile_store(const GemmParams& p, const f32x4 (&acc)[ROWS / 16][BNB / (NT / 4)],
                                              char* smem, int m0, int n0, int split) {
  constexpr int CLD = BNB + 4, MT = ROWS / 16, NW = BNB / (NT / 4);
  const int lane = lane_id(), w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  float* ct = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int ns = 0; ns < NW; ++ns)
#pragma unroll
      for (int q = 0; q < 4; ++q) ct[(mt * 16 + 4 * g + q) * CLD + w * 16 * NW + ns * 16 + r] = acc[mt][ns][q];
  block_sync();
  ct_store<EPI, BNB, ROWS, NT>(p, ct, m0, n0, split);
}

// s_waitcnt simm16 (gfx9 layout) for lgkmcnt(0) alone
constexpr int LGKM0_SK = 0xC07F;

__device__ __forceinline__ void glds16(const void* g, void* lds) {
  __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) const void*)g,
                                   (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}

}  // namespace lsd
