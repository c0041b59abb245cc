// Small-M decode GEMV (M <= 8 rows): C[M,N] = norm?(A)[M,K] . W[N,K]^T (+ epilogue)
//
// Single-stream and small-batch decode (SURVEY.md §7.4 hard part 1: "decode
// GEMMs are skinny") is pure weight streaming: every W byte is used M <= 8
// times, so the only goal is to keep HBM busy and pay as few kernel
// boundaries as possible.  The split-K MFMA kernel (gemm.hip, gemm_sk) pays a
// cross-workgroup combine (release/acquire ticket) per launch and needs a
// separate norm kernel in front of every QKV / MLP-up / lm_head GEMM; at
// M = 1 that was ~7 us of fixed cost per launch (profiles/r1_microbench_gemm_m1_256.log).
//
// Design (guide §5 "GEMV / M <= 16 decode weights": load straight to VGPRs,
// deep unroll, late vmcnt):
//   * one wave owns CPW whole W rows (output columns) over the FULL K: no
//     split-K, no partial slabs, no cross-workgroup hand-off at all;
//   * every 16-byte W chunk of the wave's rows is issued up front (NB x 4
//     chunks per lane per row, fully unrolled), the activation rows are
//     requested BEFORE them (L2-resident, they land first), so the input
//     prologue below runs while the weight stream is in flight;
//   * fused input norm (NORM = LayerNorm / RMSNorm): the workgroup normalises
//     the fp32 residual rows itself (block-wide two-pass statistics) and
//     writes the bf16 result to LDS -- the separate norm launch disappears;
//   * dot products with v_dot2c_f32_bf16 against the LDS image (zero-padded
//     past K, so the clamped tail chunks contribute nothing);
//   * butterfly reduce-scatter across the 64 lanes (CPW*MR values, one value
//     per lane group at the end), then the fused epilogue: bias, gelu_new,
//     silu(gate)*up, fp32 logits, residual add, or QKV + RoPE + KV-cache append.
// Replaces, for decode at M <= 8, the reference's per-token HF Conv1D /
// nn.Linear calls (`[tf5.15] modeling_gpt2.py:185,223,239,241`, `server.py:102`).
//
// FP8 weights (W8, gemv_fp8_kernel): the same kernel over W stored as OCP E4M3
// bytes with one fp32 scale per row (wquant.hip) -- half the bytes streamed.
//   * a 16-byte chunk is 16 weights, so a row needs half the chunks per lane:
//     SLOTS = 2 NB instead of 4 NB over the same K buckets and the same LDS
//     image (KS = 2048 NB elements per activation row); the weight registers
//     halve (8 NB dwords per row per lane instead of 16 NB);
//   * v_cvt_scalef32_pk_bf16_fp8 (scale operand 1.0: exact) turns two bytes
//     into the bf16x2 operand of v_dot2c_f32_bf16 in one instruction, once per
//     chunk and W row, reused by all MR activation rows;
//   * the row scale is an epilogue operand fetched with the bias in step 0:
//     y = acc * scale[n] + bias (one fma), ahead of GELU / SiLU / RoPE / the
//     residual add / the KV store; SiLU's gate and up rows and RoPE's partner
//     row bring their own scales; segmax repeats the same fma.
// The bf16 instantiations are the code they were (W8 = false folds every
// branch below away).
//
// MXFP4 weights (WK = 2, gemv_mxfp4_kernel): the same kernel over W stored as
// OCP Microscaling FP4 (wquant.hip, mx4.h) -- 17/64 of the bf16 bytes.
//   * a lane's 16-byte load is one MX block: 32 E2M1 weights under one E8M0
//     scale byte.  SLOTS = NB chunks per lane per row over the same K buckets
//     and the same KS = 2048 NB element LDS image.  The scale byte of chunk c
//     of a row is e[row][c]: the wave reads 64 consecutive bytes, requested in
//     the same loop as the chunk itself (step 2), never after it.
//   * v_cvt_scalef32_pk_bf16_fp4 takes the scale (the byte moved into an fp32
//     exponent field) as its scale operand: the 16 converts of a chunk yield
//     the exact dequantised bf16x2 pairs, shared by all MR activation rows.
//     Nothing of the scale reaches the epilogue: y = acc + bias as on bf16; the
//     FP8 kernel's e_sc / e_scp operands and its segmax fma have no counterpart.
//   * LDS image.  A lane reads the 64 contiguous bytes of block c = lane + 64 i
//     as four ds_read_b128 (16-byte chunks u = 4 c + d, d = 0..3), so in a
//     linear image consecutive lanes are 64 bytes apart.  LDS serves a
//     ds_read_b128 in groups of 16 lanes over 64 banks of 4 bytes, i.e. 16
//     bank groups of 16 bytes, bank group = chunk address % 16; linear, the 16
//     lanes of a group at one d hit chunks 4 c + d: only 4 distinct bank groups,
//     a 4-way conflict.  The image is therefore stored swizzled (this kernel
//     writes it itself in step 3): chunk u lives at
//         (u & ~3) | ((u ^ (u >> 4)) & 3)    =  4 c + (d ^ ((c >> 2) & 3)).
//     Bank check: a group is c = 16 g + t, t = 0..15; its bank group is
//     4 (t & 3) + (d ^ (t >> 2)).  (t & 3, t >> 2) runs over all 16 pairs and
//     XOR with the fixed d permutes the second member, so the 16 lanes hit 16
//     distinct bank groups: every ds_read_b128 is conflict-free.  An
//     activation row is 4096 NB bytes, a multiple of the 256-byte bank row, so
//     the row m does not enter.  The step-3 stores write 16 consecutive chunks
//     per 16 lanes; the swizzle permutes them inside one 256-byte bank row, so
//     the stores stay conflict-free too (the norm prologue's 8-byte stores
//     likewise move only inside their 64-byte block).
//   * rows per wave.  At the bf16 kernel's CPW a lane has a quarter of its
//     weight bytes outstanding and every workgroup still pays the whole
//     activation prologue, so the MXFP4 kernel may own more rows per wave where
//     V = CPW MR <= 16.  Measured (profiles/weight_mxfp4_ab.log, README "MXFP4
//     weights"): the residual epilogue at CPW = 2 is faster than, or within 2 % of,
//     the bf16 kernel's 1 on all four residual shapes (0.98-1.33x), SiLU at 4
//     rows is faster at CPW = 4 (1.08x); the bf16 / GELU epilogues at CPW = 4
//     lost to CPW = 2 (0.88-0.98x) and keep 2, as do QKV (same stream) and the
//     fp32 logits (a workgroup stays one 8-column sampler segment).  mx4_cpw
//     below is that rule; lsd_gemv_set_mx4_wide(0) launches the bf16 kernel's
//     CPW instead (A/B).
#include "common.h"
#include "mx4.h"
#include "gemm_params.h"
#include "api.h"

namespace lsd {
namespace gv {
enum : int { BF16 = 0, GELU = 1, SILU = 2, F32 = 3, RESID = 4, QKV = 6 };
enum : int { NONE = 0, LN = 1, RMS = 2 };
}  // namespace gv

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// Pairs (2j, 2j+1) of a bf16x8 as the bf16x2 operand of v_dot2c_f32_bf16.
// (A __builtin_bit_cast of a u32x4 element to bf16x2 miscompiles on ROCm 7.2:
// hipcc loads one dword and feeds it to all four dot2 instructions.)
#define LSD_PAIR(v, j) __builtin_shufflevector(v, v, 2 * (j), 2 * (j) + 1)
__device__ __forceinline__ float dot8(bf16x8 a, bf16x8 b, float acc) {
  acc = __builtin_amdgcn_fdot2_f32_bf16(LSD_PAIR(a, 0), LSD_PAIR(b, 0), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(LSD_PAIR(a, 1), LSD_PAIR(b, 1), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(LSD_PAIR(a, 2), LSD_PAIR(b, 2), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(LSD_PAIR(a, 3), LSD_PAIR(b, 3), acc, false);
  return acc;
}

// W row j (0..CPW-1) of global wave gw.  SiLU: the gate/up rows are
// interleaved in 16-row blocks (ops/hip.py interleave_gate_up), so output
// column c needs rows 32*(c/16) + c%16 (gate) and that + 16 (up).
template <int EPI, int CPW>
__device__ __forceinline__ int gv_row(int gw, int j) {
  if constexpr (EPI == gv::SILU) {
    const int col = gw * (CPW / 2) + (j >> 1);
    return (col >> 4) * 32 + (col & 15) + (j & 1) * 16;
  } else {
    return gw * CPW + j;
  }
}

// One butterfly step at lane bit OFF over the first N live values: lanes with
// the bit set keep the upper half, the others the lower half, each adding
// the partner's copy of the half it keeps (N == 1: plain pairwise sum).
template <int OFF, int N, int V>
__device__ __forceinline__ void gv_step(float (&acc)[V], int& idx, int lane) {
  if constexpr (N == 1) {
    acc[0] += wave_xchg<OFF>(acc[0]);
  } else {
    constexpr int h = N / 2;
    const bool up = (lane & OFF) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const float send = up ? acc[i] : acc[i + h];
      const float keep = up ? acc[i + h] : acc[i];
      acc[i] = keep + wave_xchg<OFF>(send);
    }
    if (up) idx += h;
  }
}

// Block-wide sums of MR values at once (one LDS round for all rows).
// 16 E4M3 bytes . 16 bf16 (two LDS chunks), as eight bf16x2 dot products
__device__ __forceinline__ void cvt16(u32x4 w, bf16x2 (&o)[8]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    o[2 * d] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[d], 1.0f, false);
    o[2 * d + 1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[d], 1.0f, true);
  }
}
__device__ __forceinline__ float dot16(const bf16x2 (&w)[8], bf16x8 x0, bf16x8 x1, float acc) {
  acc = __builtin_amdgcn_fdot2_f32_bf16(w[0], LSD_PAIR(x0, 0), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(w[1], LSD_PAIR(x0, 1), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(w[2], LSD_PAIR(x0, 2), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(w[3], LSD_PAIR(x0, 3), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(w[4], LSD_PAIR(x1, 0), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(w[5], LSD_PAIR(x1, 1), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(w[6], LSD_PAIR(x1, 2), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(w[7], LSD_PAIR(x1, 3), acc, false);
  return acc;
}

template <int MR>
__device__ __forceinline__ void block_sums(float (&v)[MR], float* red) {
#pragma unroll
  for (int m = 0; m < MR; ++m) v[m] = wave_sum(v[m]);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if (lane_id() == 0) {
#pragma unroll
    for (int m = 0; m < MR; ++m) red[w * MR + m] = v[m];
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < MR; ++m) v[m] = red[m] + red[MR + m] + red[2 * MR + m] + red[3 * MR + m];
}

// the same over block_sync() (common.h), for the FP8-weight kernel
template <int MR>
__device__ __forceinline__ void block_sums_nopk(float (&v)[MR], float* red) {
#pragma unroll
  for (int m = 0; m < MR; ++m) v[m] = wave_sum(v[m]);
  const int w = threadIdx.x >> 6;
  block_sync();
  if (lane_id() == 0) {
#pragma unroll
    for (int m = 0; m < MR; ++m) red[w * MR + m] = v[m];
  }
  block_sync();
#pragma unroll
  for (int m = 0; m < MR; ++m) v[m] = red[m] + red[MR + m] + red[2 * MR + m] + red[3 * MR + m];
}

template <int MR, int NB, int NORM>
constexpr bool gv_ok() {
  return MR * NB <= 16 && (NORM == gv::NONE || MR * NB <= 4);
}

template <int MR, int CPW, int EPI, int NORM, int NB>
__global__ __launch_bounds__(256) void gemv_kernel(GemvParams p) {
  constexpr int WK = 0;
  constexpr const float* wscale = nullptr;
  constexpr const unsigned char* wexp = nullptr;
#define LSD_GV_SYNC() __syncthreads()
#define LSD_GV_BLOCK_SUMS block_sums
#include "gemv_body.h"
#undef LSD_GV_SYNC
#undef LSD_GV_BLOCK_SUMS
}

// FP8 E4M3 weight rows with per-row scales; compiled without the packed fp32
// VALU forms (common.h LSD_NO_PK_F32), where HIP's __syncthreads() stays a call.
template <int MR, int CPW, int EPI, int NORM, int NB>
__global__ LSD_NO_PK_F32 __launch_bounds__(256) void gemv_fp8_kernel(GemvParams p, const float* wscale) {
  constexpr int WK = 1;
  constexpr const unsigned char* wexp = nullptr;
#define LSD_GV_SYNC() block_sync()
#define LSD_GV_BLOCK_SUMS block_sums_nopk
#include "gemv_body.h"
#undef LSD_GV_SYNC
#undef LSD_GV_BLOCK_SUMS
}

// MXFP4 blocks with E8M0 scale bytes wexp [N][K / 32]; compiled like the FP8 kernel.
template <int MR, int CPW, int EPI, int NORM, int NB>
__global__ LSD_NO_PK_F32 __launch_bounds__(256) void gemv_mxfp4_kernel(GemvParams p, const unsigned char* wexp) {
  constexpr int WK = 2;
  constexpr const float* wscale = nullptr;
#define LSD_GV_SYNC() block_sync()
#define LSD_GV_BLOCK_SUMS block_sums_nopk
#include "gemv_body.h"
#undef LSD_GV_SYNC
#undef LSD_GV_BLOCK_SUMS
}

// W rows per wave of the MXFP4 kernel (header comment, "rows per wave")
template <int EPI, int MR, int NB>
constexpr int mx4_cpw() {
  return EPI == gv::SILU && MR == 4 && NB == 2 ? 4 : 2;
}

template <int MR, int CPW, int EPI, int NORM, int NB>
hipError_t gemv_mxfp4_go(const GemvParams& p, const unsigned char* wexp, hipStream_t st) {
  hipLaunchKernelGGL((gemv_mxfp4_kernel<MR, CPW, EPI, NORM, NB>), dim3((p.N + 4 * CPW - 1) / (4 * CPW)), dim3(256),
                     0, st, p, wexp);
  return hipGetLastError();
}

template <int EPI, int NORM>
hipError_t gemv_mxfp4_launch(const GemvParams& p, const unsigned char* wexp, int mr, int nb, bool wide,
                             hipStream_t st) {
#define LSD_GV(MR_, NB_)                                                                          \
  if (mr == MR_ && nb == NB_) {                                                                   \
    if constexpr (!gv_ok<MR_, NB_, NORM>()) {                                                     \
      return hipErrorInvalidValue;                                                                \
    } else {                                                                                      \
      constexpr int NARROW = EPI == gv::RESID ? 1 : 2, WIDE = mx4_cpw<EPI, MR_, NB_>();           \
      if (wide && WIDE != NARROW) return gemv_mxfp4_go<MR_, WIDE, EPI, NORM, NB_>(p, wexp, st);   \
      return gemv_mxfp4_go<MR_, NARROW, EPI, NORM, NB_>(p, wexp, st);                             \
    }                                                                                             \
  }
  LSD_GV(1, 1) LSD_GV(1, 2) LSD_GV(1, 4) LSD_GV(1, 7)
  LSD_GV(2, 1) LSD_GV(2, 2) LSD_GV(2, 4) LSD_GV(2, 7)
  LSD_GV(4, 1) LSD_GV(4, 2) LSD_GV(4, 4)
  LSD_GV(8, 1) LSD_GV(8, 2)
#undef LSD_GV
  return hipErrorInvalidValue;
}

template <int EPI, int NORM, bool W8>
hipError_t gemv_launch(const GemvParams& p, const float* wscale, int mr, int nb, hipStream_t st) {
  constexpr int CPW = EPI == gv::RESID ? 1 : 2;
  const int grid = (p.N + 4 * CPW - 1) / (4 * CPW);
#define LSD_GV(MR_, NB_)                                                                          \
  if (mr == MR_ && nb == NB_) {                                                                   \
    if constexpr (!gv_ok<MR_, NB_, NORM>()) {                                                     \
      return hipErrorInvalidValue;                                                                \
    } else if constexpr (W8) {                                                                    \
      hipLaunchKernelGGL((gemv_fp8_kernel<MR_, CPW, EPI, NORM, NB_>), dim3(grid), dim3(256), 0,   \
                         st, p, wscale);                                                          \
      return hipGetLastError();                                                                   \
    } else {                                                                                      \
      hipLaunchKernelGGL((gemv_kernel<MR_, CPW, EPI, NORM, NB_>), dim3(grid), dim3(256), 0,       \
                         st, p);                                                                  \
      return hipGetLastError();                                                                   \
    }                                                                                             \
  }
  LSD_GV(1, 1) LSD_GV(1, 2) LSD_GV(1, 4) LSD_GV(1, 7)
  LSD_GV(2, 1) LSD_GV(2, 2) LSD_GV(2, 4) LSD_GV(2, 7)
  LSD_GV(4, 1) LSD_GV(4, 2) LSD_GV(4, 4)
  LSD_GV(8, 1) LSD_GV(8, 2)
#undef LSD_GV
  return hipErrorInvalidValue;
}

}  // namespace lsd

using namespace lsd;

// Row bucket and K bucket of a GEMV launch; 0 when the shape is not eligible.
static int gv_mr(int M) { return M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : M <= 8 ? 8 : 0; }
static int gv_nb(int K) { return K <= 2048 ? 1 : K <= 4096 ? 2 : K <= 8192 ? 4 : K <= 14336 ? 7 : 0; }

static int lsd_gemv_ok(int M, int K, int epi, int norm) {  // host code asks lsd_gemv_ok_w
  const int mr = gv_mr(M), nb = gv_nb(K);
  if (M < 1 || mr == 0 || nb == 0 || K % 8 != 0) return 0;
  if (mr * nb > 16) return 0;
  if (norm != gv::NONE && mr * nb > 4) return 0;
  if (epi == 5) return 0;  // no slab epilogue: the GEMV never splits K
  // exactly the (epilogue, norm) pairs lsd_gemv dispatches: a pair it does not
  // instantiate must read "not ok" so the caller materialises the norm first
  switch (epi * 4 + norm) {
    case gv::BF16 * 4 + gv::NONE: case gv::GELU * 4 + gv::NONE: case gv::GELU * 4 + gv::LN:
    case gv::SILU * 4 + gv::NONE: case gv::SILU * 4 + gv::RMS: case gv::F32 * 4 + gv::NONE:
    case gv::F32 * 4 + gv::LN: case gv::F32 * 4 + gv::RMS: case gv::RESID * 4 + gv::NONE:
    case gv::QKV * 4 + gv::NONE: case gv::QKV * 4 + gv::LN: case gv::QKV * 4 + gv::RMS:
      return 1;
    default:
      return 0;
  }
}

// The same question for a weight kind: 0 bf16, 1 FP8 E4M3 rows with per-row
// scales, 2 MXFP4 blocks.  Both variants keep the K buckets and the LDS image
// of the bf16 one (a 16-byte chunk is 16 / 32 weights, so a row takes half / a
// quarter of the chunks), so they accept what the bf16 kernel accepts wherever
// a row is whole chunks.
extern "C" int lsd_gemv_ok_w(int M, int K, int epi, int norm, int wkind) {
  if (wkind < 0 || wkind > 2) return 0;
  if (wkind && K % (16 * wkind) != 0) return 0;
  return lsd_gemv_ok(M, K, epi, norm);
}

static int g_gemv_nt = 0;
extern "C" void lsd_gemv_set_nt(int v) { g_gemv_nt = v; }
static int g_mx4_wide = 1;
extern "C" void lsd_gemv_set_mx4_wide(int v) { g_mx4_wide = v; }

// wscale != null: W holds E4M3 bytes (p.ldw in bytes) with those row scales
template <bool W8>
static hipError_t gemv_dispatch(const GemvParams& p, const float* wscale, int epi, int norm, hipStream_t st) {
  const int mr = gv_mr(p.M), nb = gv_nb(p.K);
  switch (epi * 4 + norm) {
    case gv::BF16 * 4 + gv::NONE: return gemv_launch<gv::BF16, gv::NONE, W8>(p, wscale, mr, nb, st);
    case gv::GELU * 4 + gv::NONE: return gemv_launch<gv::GELU, gv::NONE, W8>(p, wscale, mr, nb, st);
    case gv::GELU * 4 + gv::LN: return gemv_launch<gv::GELU, gv::LN, W8>(p, wscale, mr, nb, st);
    case gv::SILU * 4 + gv::NONE: return gemv_launch<gv::SILU, gv::NONE, W8>(p, wscale, mr, nb, st);
    case gv::SILU * 4 + gv::RMS: return gemv_launch<gv::SILU, gv::RMS, W8>(p, wscale, mr, nb, st);
    case gv::F32 * 4 + gv::NONE: return gemv_launch<gv::F32, gv::NONE, W8>(p, wscale, mr, nb, st);
    case gv::F32 * 4 + gv::LN: return gemv_launch<gv::F32, gv::LN, W8>(p, wscale, mr, nb, st);
    case gv::F32 * 4 + gv::RMS: return gemv_launch<gv::F32, gv::RMS, W8>(p, wscale, mr, nb, st);
    case gv::RESID * 4 + gv::NONE: return gemv_launch<gv::RESID, gv::NONE, W8>(p, wscale, mr, nb, st);
    case gv::QKV * 4 + gv::NONE: return gemv_launch<gv::QKV, gv::NONE, W8>(p, wscale, mr, nb, st);
    case gv::QKV * 4 + gv::LN: return gemv_launch<gv::QKV, gv::LN, W8>(p, wscale, mr, nb, st);
    case gv::QKV * 4 + gv::RMS: return gemv_launch<gv::QKV, gv::RMS, W8>(p, wscale, mr, nb, st);
    default: return hipErrorInvalidValue;
  }
}

extern "C" hipError_t lsd_gemv(const GemvParams* pin, int epi, int norm, hipStream_t st) {
  if (!lsd_gemv_ok(pin->M, pin->K, epi, norm)) return hipErrorInvalidValue;
  GemvParams q = *pin;
  q.nt = g_gemv_nt;
  return gemv_dispatch<false>(q, nullptr, epi, norm, st);
}

extern "C" hipError_t lsd_gemv_fp8(const GemvParams* pin, const float* wscale, int epi, int norm, hipStream_t st) {
  if (!lsd_gemv_ok_w(pin->M, pin->K, epi, norm, 1) || wscale == nullptr) return hipErrorInvalidValue;
  GemvParams q = *pin;
  q.nt = g_gemv_nt;
  return gemv_dispatch<true>(q, wscale, epi, norm, st);
}

extern "C" hipError_t lsd_gemv_mxfp4(const GemvParams* pin, const void* wexp, int epi, int norm, hipStream_t st) {
  if (!lsd_gemv_ok_w(pin->M, pin->K, epi, norm, 2) || wexp == nullptr) return hipErrorInvalidValue;
  GemvParams p = *pin;
  p.nt = g_gemv_nt;
  const unsigned char* e = static_cast<const unsigned char*>(wexp);
  const int mr = gv_mr(p.M), nb = gv_nb(p.K);
  const bool wide = g_mx4_wide != 0;
  switch (epi * 4 + norm) {
    case gv::BF16 * 4 + gv::NONE: return gemv_mxfp4_launch<gv::BF16, gv::NONE>(p, e, mr, nb, wide, st);
    case gv::GELU * 4 + gv::NONE: return gemv_mxfp4_launch<gv::GELU, gv::NONE>(p, e, mr, nb, wide, st);
    case gv::GELU * 4 + gv::LN: return gemv_mxfp4_launch<gv::GELU, gv::LN>(p, e, mr, nb, wide, st);
    case gv::SILU * 4 + gv::NONE: return gemv_mxfp4_launch<gv::SILU, gv::NONE>(p, e, mr, nb, wide, st);
    case gv::SILU * 4 + gv::RMS: return gemv_mxfp4_launch<gv::SILU, gv::RMS>(p, e, mr, nb, wide, st);
    case gv::F32 * 4 + gv::NONE: return gemv_mxfp4_launch<gv::F32, gv::NONE>(p, e, mr, nb, wide, st);
    case gv::F32 * 4 + gv::LN: return gemv_mxfp4_launch<gv::F32, gv::LN>(p, e, mr, nb, wide, st);
    case gv::F32 * 4 + gv::RMS: return gemv_mxfp4_launch<gv::F32, gv::RMS>(p, e, mr, nb, wide, st);
    case gv::RESID * 4 + gv::NONE: return gemv_mxfp4_launch<gv::RESID, gv::NONE>(p, e, mr, nb, wide, st);
    case gv::QKV * 4 + gv::NONE: return gemv_mxfp4_launch<gv::QKV, gv::NONE>(p, e, mr, nb, wide, st);
    case gv::QKV * 4 + gv::LN: return gemv_mxfp4_launch<gv::QKV, gv::LN>(p, e, mr, nb, wide, st);
    case gv::QKV * 4 + gv::RMS: return gemv_mxfp4_launch<gv::QKV, gv::RMS>(p, e, mr, nb, wide, st);
    default: return hipErrorInvalidValue;
  }
}
