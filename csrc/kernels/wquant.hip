// Weight-only FP8: the row quantiser and the row dequantiser.
//
// Format: W[N, K] bf16 -> q[N, K] OCP E4M3 bytes + scale[N] fp32, one scale
// per output row:
//   amax_n   = max |W[n, :]|                  (fp32)
//   scale[n] = amax_n / 448                   (IEEE fp32 division; 1.0 when amax_n == 0)
//   q[n, k]  = e4m3_rne(clamp(W[n, k] / scale[n], +-448))   (IEEE division again)
//   W'[n, k] = float(q[n, k]) * scale[n]
// ops/reference.py quantize_rows is the same arithmetic in torch fp32 ops; the
// quantiser here is bit-equal to it (bytes and scales).
//
//   * quantize_rows_fp8: one 256-thread workgroup per row.  Each lane reads
//     16 weights (2 x 16 bytes) per step and writes them back as 16 bytes.
//     Rows of up to 4096 elements stay in registers between the amax pass and
//     the encode; longer rows are read a second time (L2-hot: a row is at most
//     28 KB).
//   * dequant_rows_fp8: the route of GEMMs the FP8 GEMV does not take
//     (ops/hip.py): q, scale -> bf16 [N, K] in a caller's scratch, 16 bytes in
//     and 2 x 16 bytes out per lane, one rounding (bf16(float(q) * scale)).
//
// Weight-only MXFP4 (mx4.h): W[N, K] bf16, K % 32 == 0 -> q[N, K/2] E2M1
// nibbles + e[N, K/32] E8M0 bytes, one per 32 consecutive k of a row:
//   amax = f 2^p, f in [1, 2)     (read off the fp32 bits of the block's max |w|)
//   X    = p - 2 + (f > 1.5)      (smallest power of two with amax <= 6 2^X;
//                                  clamped to [-126, 127]; 0 for a block of zeros)
//   e    = X + 127,  q = e2m1_rne(w 2^-X) with w's sign bit,  W' = e2m1(q) 2^X
// ops/reference.py quantize_mx4 is the same integer and exact-fp32 steps.
//   * quantize_rows_mxfp4: a lane owns a whole block: 4 x 16 bytes in, 16
//     bytes and one scale byte out, no cross-lane step.  Blocks are numbered
//     row-major, so a wave covers 64 consecutive blocks (4 KiB of a row in, 1
//     KiB + 64 scale bytes out, each contiguous).
//   * dequant_rows_mxfp4: the route of every GEMM the MXFP4 GEMV does not
//     take: 16 bytes + 1 in, 4 x 16 bytes out per lane through the convert the
//     GEMV uses (v_cvt_scalef32_pk_bf16_fp4); exact, nothing is rounded.
#include "common.h"
#include "mx4.h"
#include "api.h"

namespace lsd {

__device__ __forceinline__ float amax8(bf16x8 v, float m) {
#pragma unroll
  for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(bf2f(v[e])));
  return m;
}

// 16 weights / scale -> 16 E4M3 bytes
__device__ __forceinline__ u32x4 quant16(bf16x8 a, bf16x8 b, float scale) {
  float y[16];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    y[e] = bf2f(a[e]) / scale;
    y[8 + e] = bf2f(b[e]) / scale;
  }
  return u32x4{fp8_pack4(y[0], y[1], y[2], y[3]), fp8_pack4(y[4], y[5], y[6], y[7]),
               fp8_pack4(y[8], y[9], y[10], y[11]), fp8_pack4(y[12], y[13], y[14], y[15])};
}

__global__ LSD_NO_PK_F32 __launch_bounds__(256) void quantize_rows_fp8_kernel(
    const bf16* __restrict__ W, long ldw, unsigned char* __restrict__ q, float* __restrict__ scale, int K) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const long n = blockIdx.x;
  const bf16* wr = W + n * ldw;
  unsigned char* qr = q + n * (long)K;
  const int KC = K >> 4;  // 16-weight chunks of the row
  // the row's first 256 chunks (all of it up to K = 4096) stay in registers
  const bool own = tid < KC;
  bf16x8 a = {}, b = {};
  if (own) {
    a = ld8(wr + tid * 16);
    b = ld8(wr + tid * 16 + 8);
  }
  float m = amax8(b, amax8(a, 0.f));
  for (int c = tid + 256; c < KC; c += 256) m = amax8(ld8(wr + c * 16 + 8), amax8(ld8(wr + c * 16), m));
#pragma unroll
  for (int o = 1; o <= 32; o <<= 1) m = fmaxf(m, wave_xchg_n(m, o));
  if (lane_id() == 0) red[tid >> 6] = m;
  block_sync();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float s = m == 0.f ? 1.f : m / FP8_MAX;
  if (tid == 0) scale[n] = s;
  if (own) *reinterpret_cast<u32x4*>(qr + tid * 16) = quant16(a, b, s);
  for (int c = tid + 256; c < KC; c += 256)
    *reinterpret_cast<u32x4*>(qr + c * 16) = quant16(ld8(wr + c * 16), ld8(wr + c * 16 + 8), s);
}

__global__ LSD_NO_PK_F32 __launch_bounds__(256) void dequant_rows_fp8_kernel(
    const unsigned char* __restrict__ q, const float* __restrict__ scale, bf16* __restrict__ out, int KC,
    long chunks) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;  // 16-weight chunk of the [N, K] matrix
  if (c >= chunks) return;
  const float s = scale[c / KC];
  const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(q) + c);
  bf16x8 o[2];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const f32x2 lo = fp8_dec2<false>(v[d]), hi = fp8_dec2<true>(v[d]);
    o[d >> 1][4 * (d & 1) + 0] = f2bf(lo[0] * s);
    o[d >> 1][4 * (d & 1) + 1] = f2bf(lo[1] * s);
    o[d >> 1][4 * (d & 1) + 2] = f2bf(hi[0] * s);
    o[d >> 1][4 * (d & 1) + 3] = f2bf(hi[1] * s);
  }
  st8(out + c * 16, o[0]);
  st8(out + c * 16 + 8, o[1]);
}

// |w| 2^-X -> E2M1 code 0..7 of {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the even mantissa bit
__device__ __forceinline__ unsigned int e2m1_code(float v) {
  return (v > 0.25f) + (v >= 0.75f) + (v > 1.25f) + (v >= 1.75f) + (v > 2.5f) + (v >= 3.5f) + (v > 5.f);
}

__global__ LSD_NO_PK_F32 __launch_bounds__(256) void quantize_rows_mxfp4_kernel(
    const bf16* __restrict__ W, long ldw, u32x4* __restrict__ q, unsigned char* __restrict__ e, int KB,
    long blocks) {
  const long b = (long)blockIdx.x * 256 + threadIdx.x;  // MX block of the [N, K / 32] grid
  if (b >= blocks) return;
  const bf16* src = W + (b / KB) * ldw + (b % KB) * 32;
  bf16x8 v[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) v[d] = ld8(src + 8 * d);
  float m = 0.f;
#pragma unroll
  for (int d = 0; d < 4; ++d) m = amax8(v[d], m);
  const int bits = __builtin_bit_cast(int, m);
  int X = (bits >> 23) - 129 + ((bits & 0x7FFFFF) > 0x400000 ? 1 : 0);
  X = bits == 0 ? 0 : min(max(X, -126), 127);
  const float inv = __builtin_bit_cast(float, (127 - X) << 23);  // 2^-X: the product below is exact
  u32x4 o;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    unsigned int word = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float f = bf2f(v[d][i]);  // the sign is read off the fp32 (-0 keeps its bit)
      word |= (e2m1_code(fabsf(f) * inv) | (__builtin_bit_cast(unsigned int, f) >> 31 << 3)) << (4 * i);
    }
    o[d] = word;
  }
  q[b] = o;
  e[b] = (unsigned char)(X + 127);
}

__global__ LSD_NO_PK_F32 __launch_bounds__(256) void dequant_rows_mxfp4_kernel(
    const u32x4* __restrict__ q, const unsigned char* __restrict__ e, bf16* __restrict__ out, long blocks) {
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  if (b >= blocks) return;
  const float s = mx4_scale(e[b]);
  mx4_pair pr[16];
  mx4_cvt32(__builtin_nontemporal_load(q + b), s, pr);
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[2 * i] = pr[4 * d + i][0];
      o[2 * i + 1] = pr[4 * d + i][1];
    }
    st8(out + b * 32 + 8 * d, o);
  }
}

}  // namespace lsd

using namespace lsd;

// W bf16 [N][K] (row stride ldw elements, rows 16-byte aligned), K % 16 == 0
extern "C" hipError_t lsd_quantize_rows_fp8(const void* W, long ldw, void* q, float* scale, int N, int K,
                                            hipStream_t st) {
  if (N < 1 || K < 16 || K % 16 != 0 || ldw % 8 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(quantize_rows_fp8_kernel, dim3(N), dim3(256), 0, st, static_cast<const bf16*>(W), ldw,
                     static_cast<unsigned char*>(q), scale, K);
  return hipGetLastError();
}

// q [N][K] bytes and out bf16 [N][K], both contiguous and 16-byte aligned
extern "C" hipError_t lsd_dequant_rows_fp8(const void* q, const float* scale, void* out, int N, int K,
                                           hipStream_t st) {
  if (N < 1 || K < 16 || K % 16 != 0) return hipErrorInvalidValue;
  const long chunks = (long)N * (K >> 4);
  hipLaunchKernelGGL(dequant_rows_fp8_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st,
                     static_cast<const unsigned char*>(q), scale, static_cast<bf16*>(out), K >> 4, chunks);
  return hipGetLastError();
}

// W bf16 [N][K] (row stride ldw elements, rows 16-byte aligned), K % 32 == 0;
// q [N][K / 2] bytes and e [N][K / 32] bytes, both contiguous, q 16-byte aligned
extern "C" hipError_t lsd_quantize_rows_mxfp4(const void* W, long ldw, void* q, void* e, int N, int K,
                                              hipStream_t st) {
  if (N < 1 || K < 32 || K % 32 != 0 || ldw % 8 != 0) return hipErrorInvalidValue;
  const long blocks = (long)N * (K >> 5);
  hipLaunchKernelGGL(quantize_rows_mxfp4_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st,
                     static_cast<const bf16*>(W), ldw, static_cast<u32x4*>(q), static_cast<unsigned char*>(e),
                     K >> 5, blocks);
  return hipGetLastError();
}

// q, e as above and out bf16 [N][K] contiguous, 16-byte aligned
extern "C" hipError_t lsd_dequant_rows_mxfp4(const void* q, const void* e, void* out, int N, int K, hipStream_t st) {
  if (N < 1 || K < 32 || K % 32 != 0) return hipErrorInvalidValue;
  const long blocks = (long)N * (K >> 5);
  hipLaunchKernelGGL(dequant_rows_mxfp4_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st,
                     static_cast<const u32x4*>(q), static_cast<const unsigned char*>(e), static_cast<bf16*>(out),
                     blocks);
  return hipGetLastError();
}
