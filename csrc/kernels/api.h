// Host API of the kernels: the one declaration of every launcher, tuning knob
// and query a .hip file defines for host code (csrc/bindings.cpp,
// csrc/stage_exec.cpp).  Each .hip file includes this header too, so a
// definition that drifts from its declaration is a compile error (conflicting
// declarations of a C function) rather than a launch with garbage arguments.
// The loopback channel's three launchers are declared with its structs in
// loopback.h.  Compiles under g++ and hipcc: bf16 pointers are lsd_bf16_t
// (gemm_params.h; __bf16 under clang, the kernels' lsd::bf16).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "gemm_params.h"
#include "gemm_plan.h"

extern "C" {

// gemm.hip: the one launch decision (gemm_plan.h) under the current tuning, and the launch of exactly that plan
void lsd_gemm_plan(int M, int N, int K, int splits, int epi, int kind, lsd::GemmPlan* out);
hipError_t lsd_gemm(const lsd::GemmParams* p, const lsd::GemmPlan* plan, int* cnt, float* ws, hipStream_t st);
const char* lsd_gemm_last_launch();
void lsd_gemm_note_launch(const char* tag);  // tag: a string literal
void lsd_gemm_set_big_min(int v);
void lsd_gemm_set_big_group(int v);
void lsd_gemm_set_big_kind(int v);
void lsd_gemm_set_tiled3_max(int v);
void lsd_gemm_set_ring_slots(int v);
void lsd_gemm_set_ring_tn(int v);
void lsd_gemm_set_ring_fill(int v);
void lsd_gemm_set_ring_m96(int v);
void lsd_gemm_set_d256_slots(int v);
void lsd_gemm_set_ring8(int v);
void lsd_gemm_set_ring8_flags(int v);
void lsd_gemm_set_ring8_pack(int v);
void lsd_gemm_set_nw2_rows(int v);
void lsd_gemm_set_sk_rows(int v);
int lsd_gemm_d256_bn(int kind, int M, int N, int K);
int lsd_gemm_ring8_tiles(int M, int N, int K, int S);
int lsd_gemm_sk_rblocks(int M, int N, int S);
int lsd_gemm_sk_nw(int M, int epi);

// gemm_w8.hip: a kind-0 or kind-2 / 3 plan on FP8 E4M3 weight rows (p->W bytes, p->ldw in bytes) with fp32 row scales
int lsd_gemm_w8_ok(int M, int N, int K, int epi);
hipError_t lsd_gemm_w8(const lsd::GemmParams* p, const float* wscale, const lsd::GemmPlan* plan, int* cnt, float* ws,
                       hipStream_t st);

// gemv.hip
int lsd_gemv_ok_w(int M, int K, int epi, int norm, int wkind);  // 0 bf16, 1 FP8 E4M3, 2 MXFP4
void lsd_gemv_set_nt(int v);
hipError_t lsd_gemv(const lsd::GemvParams* p, int epi, int norm, hipStream_t st);
hipError_t lsd_gemv_fp8(const lsd::GemvParams* p, const float* wscale, int epi, int norm, hipStream_t st);
// MXFP4 rows (p->W nibble bytes, p->ldw in bytes) with E8M0 scale bytes wexp [N][K / 32]
hipError_t lsd_gemv_mxfp4(const lsd::GemvParams* p, const void* wexp, int epi, int norm, hipStream_t st);
void lsd_gemv_set_mx4_wide(int v);

// wquant.hip
hipError_t lsd_quantize_rows_fp8(const void* W, long ldw, void* q, float* scale, int N, int K, hipStream_t st);
hipError_t lsd_dequant_rows_fp8(const void* q, const float* scale, void* out, int N, int K, hipStream_t st);
hipError_t lsd_quantize_rows_mxfp4(const void* W, long ldw, void* q, void* e, int N, int K, hipStream_t st);
hipError_t lsd_dequant_rows_mxfp4(const void* q, const void* e, void* out, int N, int K, hipStream_t st);

// norm.hip
hipError_t lsd_embed(const int* ids, const int* pos, const lsd_bf16_t* wte, const lsd_bf16_t* wpe, float* out, int T,
                     int H, int vocab, hipStream_t st);
hipError_t lsd_norm(float* x, const void* slab, int slab_bf16, int splits, const lsd_bf16_t* pbias,
                    const lsd_bf16_t* w, const lsd_bf16_t* b, lsd_bf16_t* out, int T, int H, float eps, int rms,
                    const int* rows, int nrows, hipStream_t st);
const char* lsd_norm_last_launch();
void lsd_norm_set_wave_min(int v);
void lsd_norm_set_wave_narrow_min(int v);

// attention.hip
hipError_t lsd_attn_decode(const lsd_bf16_t* q, long ldq, const lsd_bf16_t* kc, const lsd_bf16_t* vc,
                           const int* seq_slots, const int* qpos, lsd_bf16_t* out, long ldo, float* part_o,
                           float* part_ml, int B, int nh, int n_kv, int hd, int max_seq, int splits,
                           float scale_log2, int kv_elt, hipStream_t st);
hipError_t lsd_attn_prefill(const lsd_bf16_t* q, long ldq, const lsd_bf16_t* kc, const lsd_bf16_t* vc,
                            const int* tiles, int n_tiles, const int* seq_slots, const int* q_start,
                            const int* cu_q, lsd_bf16_t* out, long ldo, int nh, int n_kv, int hd, int max_seq,
                            float scale_log2, int kv_elt, hipStream_t st);
hipError_t lsd_attn_oproj(const lsd_bf16_t* q, long ldq, const lsd_bf16_t* kc, const lsd_bf16_t* vc,
                          const int* seq_slots, const int* qpos, int B, int nh, int n_kv, int hd, int max_seq,
                          float scale_log2, const lsd_bf16_t* W, long ldw, const lsd_bf16_t* bias, float* x, int N,
                          int NC, float* part, int* cnt, hipStream_t st);
void lsd_attn_set_max_wg(int v);
void lsd_attn_set_small_waves(int v);
void lsd_attn_set_small_waves128(int v);
void lsd_attn_set_large_waves(int hd, int v);
void lsd_attn_set_mfma_min(int v);

// elementwise.hip
hipError_t lsd_silu_mul(const lsd_bf16_t* y, long ldy, lsd_bf16_t* out, long ldo, int M, int F, hipStream_t st);
hipError_t lsd_qkv_post(const float* y, long ldy, const lsd_bf16_t* bias, const int* tslot, const int* tpos,
                        const float* rope, lsd_bf16_t* q, lsd_bf16_t* kc, lsd_bf16_t* vc, int M, int q_size,
                        int kv_size, int hd, int n_kv, int max_seq, int kv_fp8, hipStream_t st);
hipError_t lsd_apply_rows(const int64_t* args, int nargs, int b, hipStream_t st);

// sample.hip
hipError_t lsd_sample(const float* logits, long ld, int B, int V, const float* temp, const int* topk,
                      const int* greedy, const long long* seeds, long long* step, int* out, int advance,
                      const int* active, int* pos, const float* segmax, long ldseg, const float* top_p,
                      const float* min_p, hipStream_t st);

// penalty.hip
hipError_t lsd_penalize(float* logits, long ld, int B, int V, const int* hist, int L, int nslots, const int* slots,
                        const long long* counts, const float* presence, const float* frequency, float* segmax,
                        long ldseg, hipStream_t st);
hipError_t lsd_record_tokens(int* hist, int L, int nslots, const int* slots, const long long* step, int back,
                             const int* tokens, const int* active, int B, hipStream_t st);

// repeat.hip
hipError_t lsd_repeat_penalty(float* logits, long ld, int B, int V, const int* plen, const float* rpen,
                              const int* ngram, const int* tok, int L, int nslots, const int* slots,
                              const long long* step, float* segmax, long ldseg, hipStream_t st);
hipError_t lsd_record_context(int* tok, int L, int nslots, const int* plen, const int* slots, const long long* step,
                              int back, const int* tokens, const int* active, int B, hipStream_t st);

// bad_words.hip
hipError_t lsd_bad_words(float* logits, long ld, int B, int V, const int* cnt, const int* end, int N, const int* btok,
                         int T, const int* plen, const int* ctok, int L, int nslots, const int* slots,
                         const long long* step, float* segmax, long ldseg, hipStream_t st);

// logit_edit.hip
hipError_t lsd_logit_edits(float* logits, long ld, int B, int V, const int* cnt, const int* tok, const float* val,
                           const int* until, int E, int nslots, const int* slots, const long long* step,
                           float* segmax, long ldseg, hipStream_t st);

// allow_mask.hip
hipError_t lsd_allow_mask(float* logits, long ld, int B, int V, const int* on, const int* bits, int W, int nslots,
                          const int* slots, float* segmax, long ldseg, hipStream_t st);

// guide.hip
hipError_t lsd_guide_mask(float* logits, long ld, int B, int V, const short* gcls, long Vp, const short* gnext,
                          long cells, const int* gdim, int G, const int* gsl, int nslots, const int* slots,
                          float* segmax, long ldseg, hipStream_t st);
hipError_t lsd_guide_advance(int* gsl, int nslots, const short* gcls, long Vp, const short* gnext, long cells,
                             const int* gdim, int G, int V, const int* slots, const int* tokens, const int* active,
                             int B, hipStream_t st);

// kv_fork.hip
hipError_t lsd_kv_fork(void* buf, int outer, int slots, int heads, int max_seq, long row_bytes, const int* src,
                       const int* dst, const int* len, int F, int max_len, hipStream_t st);

// logprob.hip
hipError_t lsd_logprobs(const float* logits, long ld, int B, int V, const int* tokens, const int* nlp,
                        const int* slots, const long long* step, int back, const int* active, float* lp_tok,
                        int* lp_top_id, float* lp_top, int L, int nslots, int W, hipStream_t st);

// score.hip
int lsd_score_slices(int T, int Vp);
hipError_t lsd_lm_head_score(const void* xn, long lda, const void* w, long ldw, const int* targets, int T, int V,
                             int Vp, int K, int S, float* part, float* tok_lp, int* top_id, float* top_lp,
                             hipStream_t st);

}  // extern "C"
