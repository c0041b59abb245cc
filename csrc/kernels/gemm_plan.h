// The one place a GEMM launch is decided: which kernel instance of
// csrc/kernels/gemm.hip runs, on which grid, and how many ticket counters and
// fp32 workspace floats its in-kernel split-K combine needs.
//
// plan_gemm() is a pure function of the shape and a GemmTuning snapshot.
// csrc/bindings.cpp sizes the counters and the workspace from the GemmPlan and
// hands the same plan to lsd_gemm(), which launches it without deciding
// anything again -- sizing and launch cannot disagree.
//
// Plain C++17, no HIP header: tests/test_gemm_plan.py compiles it alone.
#pragma once

namespace lsd {

enum Epi : int {
  EPI_BF16 = 0,      // out bf16 = acc + bias
  EPI_GELU = 1,      // out bf16 = gelu_new(acc + bias)
  EPI_SILU_MUL = 2,  // out bf16 [M, N/2] = silu(gate) * up; W rows interleaved in 16-row blocks
  EPI_F32 = 3,       // out f32 = acc
  EPI_RESID = 4,     // x f32 += acc + bias
  EPI_SLAB = 5,      // slab[split][M][N] = acc
  EPI_QKV = 6,       // q -> out bf16, k/v -> KV cache (+ RoPE)
};

// Block tiles of the 128x128 (tiled / ring) and the 256x256 (big / p8) kernels.
constexpr int TBM = 128, TBN = 128;
constexpr int GBM = 256, GBN = 256;

// Tuning knobs (lsd_gemm_set_*: tuning runs and tests).  The defaults are the
// kernels' own; the engine applies ops/routing.py's on top.
struct GemmTuning {
  int big_min_blocks = 160;  // tiled launches with >= this many 256x256 tiles run the 256x256 kernel
  // tile_order() group (0 = M-fastest).  4: XL prefill GEMMs 10-25 % faster
  // than M-fastest, 8 equal, 16+ slower (profiles/r2_prefill_tile_order.log)
  int big_group = 4;
  // 0 = BK=32 ring kernel (gemm_big), 1 = phase-pipelined BK=64 (gemm_p8) with
  // global_load_lds, 4 = the same with buffer_load ... lds staging (+6 % on the
  // GPT-2 XL prefill projections and +25 % at 4096^3 over kind 1;
  // profiles/r3_p8_buffer_lds.log)
  int big_kind = 4;
  // 128x128 launches of at most this many workgroups use the 3-slot ring kernel
  // (1 block/CU); larger grids keep the 2-blocks/CU double-buffered one.  0 = off
  int tiled3_max_blocks = 0;
  int ring_slots = 3;   // 3 or 4
  int ring_tn = 128;    // ring tile columns, 128, 64, 32 or 0 (auto 32/64)
  int ring_fill = 128;  // auto: 32-wide tiles below this many 64-wide workgroups
  int ring_m96 = 0;     // largest 96-row-tile ring grid (0 = off)
  int ring8 = 0;        // 128x64 decode ring on 8 waves (gemm_ring8_kernel): 0 off, 1 loader waves, 2 all compute
  int ring8_flags = 0;  // A/B bits, 1 = rotate each tile's K start, 2 = weights staged nt, 4 = buffer_load staging
  int ring8_pack = 0;   // operands in k-block-packed layouts (bit 0 W, bit 1 A; A/B only)
  int d256_slots = 3;   // gemm_d256 ring depth 2..4 (BN 128: at most 3)
  // Decode GEMM row blocking: when the column tiles x K splits leave the chip
  // under-filled (< rb_fill workgroups, e.g. the deferred-residual projections
  // with N = H), M > sk_rows rows run as ceil(M / sk_rows) row blocks (grid z)
  // that share each W tile through L2 -- more workgroups without more split-K
  // slab traffic (tools/microbench.py rows: H x H projection at M = 128
  // 14.1 -> 12.1 us; well-filled grids gain nothing, lm_head loses).
  int sk_rows = 64;
  int rb_fill = 192;
  // Split-K column tile width 64 * NW.  Wide tiles (NW = 2) read A half as
  // often but double the weight fragments per wave; measured slower at M = 128
  // on every GPT-2 XL shape (tools/microbench.py rows), so only silu_mul
  // (gate/up pairs) uses them by default; above this many rows every epilogue does.
  int nw2_rows = 1 << 30;

  void set_big_group(int v) { big_group = v < 0 ? 0 : v; }
  void set_big_kind(int v) { big_kind = (v == 1 || v == 4) ? v : 0; }
  void set_ring_slots(int v) { ring_slots = v == 4 ? 4 : 3; }
  void set_ring_tn(int v) { ring_tn = (v == 64 || v == 32 || v == 0) ? v : 128; }
  void set_ring8(int v) { ring8 = (v == 1 || v == 2) ? v : 0; }
  void set_ring8_flags(int v) { ring8_flags = v & 7; }
  void set_ring8_pack(int v) { ring8_pack = v & 3; }
  void set_d256_slots(int v) { d256_slots = v < 2 ? 2 : (v > 4 ? 4 : v); }
  void set_sk_rows(int v) { sk_rows = v < 16 ? 16 : (v > 128 ? 128 : v); }
};

enum GemmKernel : int {
  GK_SK,     // gemm_sk_kernel<mt, nw>
  GK_D256,   // gemm_d256_kernel<tn, slots>
  GK_BIG,    // gemm_big_kernel
  GK_P8,     // gemm_p8_kernel<var>
  GK_TILED,  // gemm_tiled_kernel
  GK_RING,   // gemm_ring_kernel<slots, tn> (m96: 96-row tiles)
  GK_RING8,  // gemm_ring8_kernel<var, 3, stage == 1, pack, stage == 2>
};

struct GemmPlan {
  int valid;  // 0: no kernel takes this shape under this tuning (nothing else is meaningful)
  int M, N, K, splits, epi;  // what the plan was made for: lsd_gemm() refuses other params
  int kernel;                // GemmKernel, then the template selectors of its instance:
  int mt, nw;                // sk: 16-row tiles per row block {1, 2, 3, 4, 6, 8}, 64-column tiles per workgroup
  int slots;                 // ring 3 | 4, d256 2..4
  int tn;                    // tile columns: ring 32 | 64 | 128, d256 64 | 128
  int m96;                   // ring: 96-row tiles
  int var;                   // ring8 1 | 2, p8 0 | 4
  int pack;                  // ring8 operand packing 0..3
  int stage;                 // ring8 weight staging: 0 default, 1 non-temporal, 2 buffer_load
  const char* tag;           // what lsd_gemm_last_launch() reports (a string literal)
  unsigned grid[3], block;
  int tiles_m, tiles_n, G, rot;  // scalar kernel arguments (those the kernel takes)
  // in-kernel combine: ticket counters needed (0: none) and the fp32 floats of
  // one partial tile; the workspace holds combine_tiles * splits * tile_floats
  long combine_tiles, tile_floats;
};

inline GemmPlan plan_gemm(int M, int N, int K, int splits, int epi, int kind, const GemmTuning& t) {
  GemmPlan pl{};
  pl.M = M; pl.N = N; pl.K = K; pl.splits = splits; pl.epi = epi;
  pl.grid[0] = pl.grid[1] = pl.grid[2] = 1;
  pl.tag = "";
  if (M < 1 || N < 1 || K < 1 || splits < 1 || epi < EPI_BF16 || epi > EPI_QKV) return pl;
  const bool combine = splits > 1 && epi != EPI_SLAB;
  const auto flat = [&](int kernel, const char* tag, int wgs, int block, int tm, int tn) {
    pl.kernel = kernel; pl.tag = tag;
    pl.grid[0] = wgs; pl.block = block;
    pl.tiles_m = tm; pl.tiles_n = tn;
    pl.valid = 1;
    return pl;
  };

  // Launch kinds: 0 split-K decode kernel, 1 tiled family (ring / 128x128 /
  // 256x256 by shape), 2 / 3 gemm_d256 with 64 / 128-column tiles (M <= 1024
  // in 256-row blocks, K % 64 == 0; the caller picks it per GEMM).
  if (kind == 0) {
    // At most 128 rows (MT = 8) per row block: M up to 256 always runs as >= 2
    // row blocks.
    int rb = (M + 127) / 128;
    if (M > t.sk_rows && (N / 64) * splits < t.rb_fill) {
      const int by_rows = (M + t.sk_rows - 1) / t.sk_rows;
      if (by_rows > rb) rb = by_rows;
    }
    // Row tiles (16 rows each) of one row block: instantiated for {1, 2, 3, 4, 6, 8}.
    int mt = ((M + rb - 1) / rb + 15) / 16;
    if (mt == 5 || mt == 7) ++mt;
    if (mt > 8) return pl;
    static constexpr const char* tags[2][9] = {
        {"", "sk<1,1>", "sk<2,1>", "sk<3,1>", "sk<4,1>", "", "sk<6,1>", "", "sk<8,1>"},
        {"", "sk<1,2>", "sk<2,2>", "sk<3,2>", "sk<4,2>", "", "sk<6,2>", "", "sk<8,2>"}};
    pl.mt = mt;
    pl.nw = (epi == EPI_SILU_MUL || M > t.nw2_rows) ? 2 : 1;
    const int cols = (N + 64 * pl.nw - 1) / (64 * pl.nw);  // partial last tile masked
    if (combine) {
      pl.combine_tiles = (long)cols * rb;
      pl.tile_floats = 16L * mt * 64 * pl.nw;
    }
    flat(GK_SK, tags[pl.nw - 1][mt], cols, 256, 0, 0);
    pl.grid[1] = splits; pl.grid[2] = rb;
    return pl;
  }

  if (kind >= 2) {
    if (M > 1024 || K % 64 != 0) return pl;
    pl.tn = kind == 3 && N % 128 == 0 ? 128 : 64;
    pl.slots = t.d256_slots == 2 ? 2 : (t.d256_slots == 4 && pl.tn == 64 ? 4 : 3);
    const int tiles = ((N + pl.tn - 1) / pl.tn) * ((M + 255) / 256);
    if (combine) {
      pl.combine_tiles = tiles;
      pl.tile_floats = 256L * pl.tn;
    }
    static constexpr const char* tags[2][3] = {{"d256<64,2>", "d256<64,3>", "d256<64,4>"},
                                               {"d256<128,2>", "d256<128,3>", ""}};
    return flat(GK_D256, tags[pl.tn == 128][pl.slots - 2], tiles * splits, 512, 0, 0);
  }

  // 256x256 pipelined kernel once the problem fills the chip with 1-block/CU
  // tiles; the 128x128 kernels (2 blocks/CU) for smaller M / N.
  const int bm = (M + GBM - 1) / GBM, bn = (N + GBN - 1) / GBN;
  if (M >= GBM && K % 64 == 0 && bm * bn * splits >= t.big_min_blocks) {
    pl.G = t.big_group;
    if (t.big_kind != 1 && t.big_kind != 4) return flat(GK_BIG, "big", bm * bn * splits, 512, bm, bn);
    pl.var = t.big_kind == 1 ? 0 : 4;
    return flat(GK_P8, pl.var ? "p8<4>" : "p8<0>", bm * bn * splits, 512, bm, bn);
  }
  const int tm = (M + TBM - 1) / TBM;
  if (t.ring_tn == 64 || t.ring_tn == 32 || t.ring_tn == 0) {
    // narrow ring tiles: twice the workgroups of the 128-column grid; 32-wide
    // (2 blocks/CU) when 64-wide tiles leave the chip under-filled (auto, 0)
    const int tn64 = (N + 63) / 64;
    const bool narrow = t.ring_tn == 32 || (t.ring_tn == 0 && tm * tn64 * splits < t.ring_fill);
    if (narrow && (N % 32) == 0) {
      const int tn = (N + 31) / 32;
      if (tm * tn * splits <= 2L * t.tiled3_max_blocks) {  // long: the tests' "no cap" is 1 << 30
        pl.slots = 3; pl.tn = 32;
        return flat(GK_RING, "ring<3,32>", tm * tn * splits, 256, tm, tn);
      }
    }
    // 96-row tiles above 128 rows while 3 x the column tiles fit one round
    // on the chip (GPT-2 XL QKV at 256 rows: 225 workgroups of 512 KB of
    // operand traffic instead of 150 of 614 KB; the ring GEMMs are bound by
    // L2 -> CU bytes per workgroup, profiles/r2_decode_gemm_limits.log).
    // Alone 10-12 % faster (QKV 16.3 -> 14.7 us at 256 rows, MLP-up 17.1 ->
    // 15.0 at 192), but beside the other microbatch lane the extra
    // workgroups cost more than they save (bench: 384 sequences -1 to -1.4 %,
    // 512 within +-0.5 %; profiles/r2_ring_m96.log) -- off by default.
    if (splits == 1 && M > TBM && t.ring_m96 > 0) {
      const int tm96 = (M + 95) / 96;
      if (tm96 * tn64 <= t.ring_m96) {
        pl.slots = 3; pl.tn = 64; pl.m96 = 1;
        return flat(GK_RING, "ring<3,64,m96>", tm96 * tn64, 256, tm96, tn64);
      }
    }
    if (tm * tn64 * splits <= t.tiled3_max_blocks) {
      // only the all-compute 8-wave ring has the in-kernel combine
      if (combine && t.ring8 != 2) return pl;
      pl.slots = 3; pl.tn = 64;
      if (t.ring8 != 1 && t.ring8 != 2) return flat(GK_RING, "ring<3,64>", tm * tn64 * splits, 256, tm, tn64);
      pl.var = t.ring8;
      pl.rot = (t.ring8_flags & 1) != 0;
      if (combine) {
        pl.combine_tiles = (long)tm * tn64;
        pl.tile_floats = 128L * 64;
      }
      const char* tag = "ring8<1,3>";
      if (t.ring8 == 2) {
        static constexpr const char* tags[3] = {"ring8<2,3>", "ring8<2,3,nt>", "ring8<2,3,bl>"};
        static constexpr const char* packed[4] = {"", "ring8<2,3,pk1>", "ring8<2,3,pk2>", "ring8<2,3,pk3>"};
        pl.pack = t.ring8_pack >= 1 && t.ring8_pack <= 3 ? t.ring8_pack : 0;
        if (pl.pack == 0) pl.stage = (t.ring8_flags & 4) ? 2 : ((t.ring8_flags & 2) ? 1 : 0);
        tag = pl.pack ? packed[pl.pack] : tags[pl.stage];
      }
      return flat(GK_RING8, tag, tm * tn64 * splits, 512, tm, tn64);
    }
  }
  const int tn = (N + TBN - 1) / TBN;
  // the cap counts 128x64 tiles whatever ring_tn says: a 128x128 ring grid
  // gets half as many workgroups (vocab-wide lm_head grids stay on the
  // 2-blocks/CU kernel; profiles/r1_ab_ring_n64.log)
  if (tm * tn * splits <= t.tiled3_max_blocks / 2) {
    pl.slots = t.ring_slots == 4 ? 4 : 3; pl.tn = 128;
    return flat(GK_RING, pl.slots == 4 ? "ring<4,128>" : "ring<3,128>", tm * tn * splits, 256, tm, tn);
  }
  return flat(GK_TILED, "tiled", tm * tn * splits, 256, tm, tn);
}

}  // namespace lsd
