// Fork a prompt's KV into other slots (CDNA4): the copy behind per-request n.
//
// A stage's KV cache is one allocation
//   buf[layer, K|V, slot, kv_head, position, head_dim]
// so for one (layer, K|V, head) -- a "run" -- the positions [0, L) of a slot
// are L * head_dim * elt contiguous bytes.  Fork f of a launch copies, for
// every run, the first len[f] * head_dim * elt bytes of slot src[f]'s run to
// the same offset of slot dst[f]'s run: a pure streaming copy of bytes, any KV
// dtype.  Bytes at or past len[f] of dst[f], and every other slot, are never
// written; len[f] == 0 copies nothing.  A source may repeat within a launch;
// destinations are distinct and never sources (the host wrapper checks:
// ops/hip.py kv_fork), so no two workgroups write one byte and none reads what
// another writes.  Bit-equal to ops/reference.py kv_fork.
//
//   kv_fork_kernel<W>   256 threads, W bytes per lane per access, KVF_UN
//                       accesses in flight per thread, loads before stores.
//                       A workgroup owns one piece (256 * W * KVF_UN bytes: 16
//                       KiB at W = 16) of one run of one fork: grid.x = runs *
//                       pieces, grid.y = forks.  The host sizes `pieces` from
//                       the longest len of the launch; a workgroup whose piece
//                       starts at or past its own fork's length returns at
//                       once, uniformly.  Plain loads and plain stores: the
//                       fork's first chunk reads the copy back on the same
//                       stream, and plain stores keep the lines in L2.
//
// W = 16 when the allocation's base and a position's bytes (head_dim * elt)
// are multiples of 16 -- then every run base and every length is; W = 4
// likewise for 4; else bytes.  The test models' head dims are small, and a
// view of a larger tensor may start anywhere.
#include "common.h"

namespace lsd {

constexpr int KVF_NT = 256;
constexpr int KVF_UN = 4;  // accesses a thread has in flight

template <int W>
struct kvf_word;
template <>
struct kvf_word<16> {
  using type = uint4;
};
template <>
struct kvf_word<4> {
  using type = unsigned;
};
template <>
struct kvf_word<1> {
  using type = unsigned char;
};

template <int W>
__global__ __launch_bounds__(KVF_NT) void kv_fork_kernel(unsigned char* __restrict__ buf, int outer, int slots,
                                                         int heads, int max_seq, long row_bytes,
                                                         const int* __restrict__ src, const int* __restrict__ dst,
                                                         const int* __restrict__ len, int pieces) {
  using T = typename kvf_word<W>::type;
  const int f = blockIdx.y;
  const int s = src[f], d = dst[f];
  int L = len[f];
  // uniform: a bad index copies nothing rather than touching another allocation
  if (s < 0 || s >= slots || d < 0 || d >= slots || s == d || L <= 0) return;
  if (L > max_seq) L = max_seq;
  const long n = (long)L * row_bytes;  // bytes of this fork per run
  const int piece = blockIdx.x % pieces;
  const int run = blockIdx.x / pieces;  // (layer, K|V) * heads + head
  const long at = (long)piece * (KVF_NT * W * KVF_UN);
  if (at >= n) return;  // uniform
  const int o = run / heads, h = run % heads;
  if (o >= outer) return;
  const long stride = (long)max_seq * row_bytes;  // bytes of one run
  const unsigned char* ps = buf + (((long)o * slots + s) * heads + h) * stride;
  unsigned char* pd = buf + (((long)o * slots + d) * heads + h) * stride;
  T v[KVF_UN];
  long off[KVF_UN];
#pragma unroll
  for (int u = 0; u < KVF_UN; ++u) {
    off[u] = at + ((long)u * KVF_NT + threadIdx.x) * W;
    if (off[u] < n) v[u] = *reinterpret_cast<const T*>(ps + off[u]);  // n is a multiple of W
  }
#pragma unroll
  for (int u = 0; u < KVF_UN; ++u)
    if (off[u] < n) *reinterpret_cast<T*>(pd + off[u]) = v[u];
}

}  // namespace lsd

// buf: the allocation [outer = layers * 2, slots, heads, max_seq, row_bytes];
// src, dst, len: device int32 [F]; max_len: the longest len of the launch (the
// host knows it), which sizes the grid.
extern "C" hipError_t lsd_kv_fork(void* buf, int outer, int slots, int heads, int max_seq, long row_bytes,
                                  const int* src, const int* dst, const int* len, int F, int max_len,
                                  hipStream_t st) {
  if (F == 0 || max_len == 0) return hipSuccess;
  if (outer <= 0 || slots <= 0 || heads <= 0 || max_seq <= 0 || row_bytes <= 0 || F < 0 || F > 65535 ||
      max_len < 0 || max_len > max_seq)
    return hipErrorInvalidValue;
  const long runs = (long)outer * heads;
  const long n = (long)max_len * row_bytes;
  const bool a16 = reinterpret_cast<uintptr_t>(buf) % 16 == 0 && row_bytes % 16 == 0;
  const bool a4 = reinterpret_cast<uintptr_t>(buf) % 4 == 0 && row_bytes % 4 == 0;
  const int W = a16 ? 16 : a4 ? 4 : 1;
  const long per = (long)lsd::KVF_NT * W * lsd::KVF_UN;
  const long pieces = (n + per - 1) / per;
  if (pieces <= 0 || runs * pieces > 0x7fffffffL) return hipErrorInvalidValue;
  unsigned char* p = static_cast<unsigned char*>(buf);
  const dim3 grid((unsigned)(runs * pieces), (unsigned)F);
  if (W == 16)
    hipLaunchKernelGGL(lsd::kv_fork_kernel<16>, grid, dim3(lsd::KVF_NT), 0, st, p, outer, slots, heads, max_seq,
                       row_bytes, src, dst, len, (int)pieces);
  else if (W == 4)
    hipLaunchKernelGGL(lsd::kv_fork_kernel<4>, grid, dim3(lsd::KVF_NT), 0, st, p, outer, slots, heads, max_seq,
                       row_bytes, src, dst, len, (int)pieces);
  else
    hipLaunchKernelGGL(lsd::kv_fork_kernel<1>, grid, dim3(lsd::KVF_NT), 0, st, p, outer, slots, heads, max_seq,
                       row_bytes, src, dst, len, (int)pieces);
  return hipGetLastError();
}
