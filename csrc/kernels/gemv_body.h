// The body of the small-M GEMV kernels (gemv.hip), included once per weight
// type so that each kernel is compiled from the text itself: the bf16 kernel
// stays the code it was, the FP8-weight kernel carries its own target
// attribute, and so does the MXFP4-weight kernel.  The including kernel provides
//   WK                  constexpr int, the weight kind: 0 bf16; 1 W holds E4M3
//                       bytes (p.W a byte pointer, p.ldw in bytes) and `wscale`
//                       the rows' fp32 scales; 2 W holds MXFP4 blocks (16 bytes
//                       = 32 weights, p.W / p.ldw in bytes again) and `wexp`
//                       their E8M0 scale bytes [N][K / 32]
//   LSD_GV_SYNC()       the workgroup barrier
//   LSD_GV_BLOCK_SUMS   block_sums over that barrier
// and the template parameters MR, CPW, EPI, NORM, NB and `GemvParams p`.
  if constexpr (!gv_ok<MR, NB, NORM>()) {
    return;
  } else {
    constexpr bool W8 = WK == 1, W4 = WK == 2;
    constexpr int SLOTS = W4 ? NB : W8 ? 2 * NB : 4 * NB;  // 16-byte chunks per lane per W row
    constexpr int KS = NB * 2048;                // LDS image row length (elements), zero past K
    constexpr int XCH = KS / 8;                  // 8-element chunks of an LDS image row
    constexpr int V = CPW * MR;      // partial sums per lane
    static_assert((V & (V - 1)) == 0 && V <= 16, "V must be a power of two <= 16");
    __shared__ __attribute__((aligned(16))) bf16 xs[MR * KS];
    __shared__ float red[4 * 16];
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const int gw = blockIdx.x * 4 + w;
    const int KC = p.K >> 3;  // valid 16-byte chunks per row
    const int KW = W4 ? p.K >> 5 : W8 ? p.K >> 4 : KC;  // ... per W row
    const int M = p.M;

    // ---- 0. the epilogue's own operands, fetched NOW (they do not depend on
    // the dot products): bias, the residual value the RESID epilogue adds to,
    // the QKV rows' position / cache slot and the RoPE partner's bias.  Loaded
    // after the reduction they cost one dependent memory round trip at the
    // tail of every launch (the single-stream layer is five such tails).
    constexpr int NOUT = EPI == gv::SILU ? V / 2 : V;
    const bool epi_thread = tid < 4 * NOUT;
    const int e_w2 = tid / NOUT, e_o = tid % NOUT;
    const int e_j = e_o / MR, e_m = e_o % MR;
    const int e_n = (blockIdx.x * 4 + e_w2) * CPW + e_j;  // output column (non-SiLU)
    const bool e_live = epi_thread && e_m < M && e_n < p.N;
    float e_bias = 0.f, e_biasp = 0.f, e_x = 0.f;
    float e_sc = 1.f, e_scp = 1.f;  // W8: the row scale (SiLU: gate, up; RoPE: row, partner)
    int e_pos = 0, e_slot = 0;
    if constexpr (W8 && EPI == gv::SILU) {
      const int col = (blockIdx.x * 4 + e_w2) * (CPW / 2) + e_j;
      if (epi_thread && col < (p.N >> 1)) {
        e_sc = wscale[(col >> 4) * 32 + (col & 15)];
        e_scp = wscale[(col >> 4) * 32 + (col & 15) + 16];
      }
    }
    if constexpr (EPI != gv::SILU) {
      if (e_live) {
        if (p.bias) e_bias = bf2f(p.bias[e_n]);
        if constexpr (W8) e_sc = wscale[e_n];
        if constexpr (EPI == gv::RESID) e_x = reinterpret_cast<const float*>(p.out)[(long)e_m * p.ldo + e_n];
        if constexpr (EPI == gv::QKV) {
          e_pos = p.tpos[e_m];
          if (e_n >= p.q_size) e_slot = p.tslot[e_m];
          if (CPW % 2 == 0 && p.rope != nullptr && p.bias && e_n < p.q_size + p.kv_size) e_biasp = bf2f(p.bias[e_n ^ 1]);
          if constexpr (W8)
            if (CPW % 2 == 0 && p.rope != nullptr && e_n < p.q_size + p.kv_size) e_scp = wscale[e_n ^ 1];
        }
      }
    }

    // ---- 1. activation rows first (L2-resident: they land before the weights)
    constexpr int NV = NORM != gv::NONE ? 2 * NB : 1;  // f32x4 per thread per row
    constexpr int NA = NORM != gv::NONE ? 1 : MR * NB;  // bf16x8 copy chunks per thread
    f32x4 xr[NORM != gv::NONE ? MR : 1][NV];
    bf16x4 gmv[NV], btv[NV];
    bf16x8 av[NA];
    if constexpr (NORM != gv::NONE) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = min((tid + 256 * i) * 4, p.K - 4);  // clamped: always a valid address
        gmv[i] = ld4(p.gamma + c);
        if constexpr (NORM == gv::LN) btv[i] = ld4(p.beta + c);
#pragma unroll
        for (int m = 0; m < MR; ++m)
          xr[m][i] = *reinterpret_cast<const f32x4*>(p.X + (long)min(m, M - 1) * p.ldx + c);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int q = tid + 256 * i;
        const int m = q / XCH, c = q % XCH;
        av[i] = ld8(p.A + (long)min(m, M - 1) * p.lda + min(c, KC - 1) * 8);
      }
    }

    // ---- 2. the weight stream: every chunk of this wave's rows, issued now
    bf16x8 wv[W8 ? 1 : CPW][W8 ? 1 : SLOTS];
    u32x4 wq[W8 || W4 ? CPW : 1][W8 || W4 ? SLOTS : 1];  // W8: 16 weights per chunk, W4: 32
    unsigned char we[W4 ? CPW : 1][W4 ? SLOTS : 1];      // W4: the chunks' scale bytes
    // waves past N re-read row N-1 (never stored)
    if constexpr (W4) {
      // chunk c of a row and its scale byte e[row][c] are requested together: a
      // wave's 64 lanes read 1 KiB of nibbles and 64 consecutive scale bytes
      const unsigned char* wb = reinterpret_cast<const unsigned char*>(p.W);
#pragma unroll
      for (int j = 0; j < CPW; ++j) {
        const long row = min(gv_row<EPI, CPW>(gw, j), p.N - 1);
        const unsigned char* wr = wb + row * p.ldw;
        const unsigned char* er = wexp + row * KW;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
          const int c = min(lane + 64 * i, KW - 1);
          if (p.nt) wq[j][i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wr + c * 16));
          else wq[j][i] = *reinterpret_cast<const u32x4*>(wr + c * 16);
          we[j][i] = er[c];
        }
      }
    } else if constexpr (W8) {
      const unsigned char* wb = reinterpret_cast<const unsigned char*>(p.W);
      if (p.nt) {
#pragma unroll
        for (int j = 0; j < CPW; ++j) {
          const unsigned char* wr = wb + (long)min(gv_row<EPI, CPW>(gw, j), p.N - 1) * p.ldw;
#pragma unroll
          for (int i = 0; i < SLOTS; ++i)
            wq[j][i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wr + min(lane + 64 * i, KW - 1) * 16));
        }
      } else {
#pragma unroll
        for (int j = 0; j < CPW; ++j) {
          const unsigned char* wr = wb + (long)min(gv_row<EPI, CPW>(gw, j), p.N - 1) * p.ldw;
#pragma unroll
          for (int i = 0; i < SLOTS; ++i)
            wq[j][i] = *reinterpret_cast<const u32x4*>(wr + min(lane + 64 * i, KW - 1) * 16);
        }
      }
    } else if (p.nt) {  // wave-uniform: weights read once per token need not stay cached
#pragma unroll
      for (int j = 0; j < CPW; ++j) {
        const bf16* wr = p.W + (long)min(gv_row<EPI, CPW>(gw, j), p.N - 1) * p.ldw;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) wv[j][i] = ld8_nt(wr + min(lane + 64 * i, KC - 1) * 8);
      }
    } else {
#pragma unroll
      for (int j = 0; j < CPW; ++j) {
        const bf16* wr = p.W + (long)min(gv_row<EPI, CPW>(gw, j), p.N - 1) * p.ldw;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) wv[j][i] = ld8(wr + min(lane + 64 * i, KC - 1) * 8);
      }
    }

    // ---- 3. input prologue -> LDS (runs while the weights are in flight)
    if constexpr (NORM != gv::NONE) {
      float mean[MR], rstd[MR];
#pragma unroll
      for (int m = 0; m < MR; ++m) mean[m] = 0.f;
      if constexpr (NORM == gv::LN) {
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          float s = 0.f;
#pragma unroll
          for (int i = 0; i < NV; ++i)
            if ((tid + 256 * i) * 4 < p.K) s += xr[m][i][0] + xr[m][i][1] + xr[m][i][2] + xr[m][i][3];
          mean[m] = s;
        }
        LSD_GV_BLOCK_SUMS<MR>(mean, red);
#pragma unroll
        for (int m = 0; m < MR; ++m) mean[m] /= p.K;
      }
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
          if ((tid + 256 * i) * 4 < p.K) {
            const f32x4 d = xr[m][i] - mean[m];
            s += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
          }
        rstd[m] = s;
      }
      LSD_GV_BLOCK_SUMS<MR>(rstd, red);
#pragma unroll
      for (int m = 0; m < MR; ++m) rstd[m] = rsqrtf(rstd[m] / p.K + p.eps);
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const int c = (tid + 256 * i) * 4;  // covers [0, KS): zero past K and for rows >= M
          bf16x4 r;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float z = (xr[m][i][e] - mean[m]) * rstd[m] * bf2f(gmv[i][e]);
            if constexpr (NORM == gv::LN) z += bf2f(btv[i][e]);
            r[e] = f2bf((c < p.K && m < M) ? z : 0.f);
          }
          if constexpr (W4) st4(xs + m * KS + mx4_swz(c >> 3) * 8 + (c & 7), r);
          else st4(xs + m * KS + c, r);
        }
    } else {
      const bf16x8 zero = {};
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int q = tid + 256 * i;
        const int m = q / XCH, c = q % XCH;
        if constexpr (W4) st8(xs + m * KS + mx4_swz(c) * 8, (m < M && c < KC) ? av[i] : zero);
        else st8(xs + m * KS + c * 8, (m < M && c < KC) ? av[i] : zero);
      }
    }
    LSD_GV_SYNC();

    // the RoPE (cos, sin) of this epilogue thread's position: issued before the
    // dot products (its position arrived with the first loads)
    float e_cs0 = 0.f, e_cs1 = 0.f;
    if constexpr (EPI == gv::QKV) {
      if (CPW % 2 == 0 && p.rope != nullptr && e_live && e_n < p.q_size + p.kv_size) {
        const int d = (e_n < p.q_size ? e_n : e_n - p.q_size) % p.hd;
        const float* cs = p.rope + ((long)e_pos * (p.hd >> 1) + (d >> 1)) * 2;
        e_cs0 = cs[0];
        e_cs1 = cs[1];
      }
    }

    // ---- 4. dot products (W from registers, x from LDS)
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
    if constexpr (W4) {
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        const int c = lane + 64 * i;  // one MX block against LDS elements [32 c, 32 c + 32), swizzled
        mx4_pair wb2[CPW][16];        // the exact dequantised pairs, shared by the MR rows
#pragma unroll
        for (int j = 0; j < CPW; ++j) mx4_cvt32(wq[j][i], mx4_scale(we[j][i]), wb2[j]);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          bf16x8 x[4];
#pragma unroll
          for (int d = 0; d < 4; ++d)
            x[d] = *reinterpret_cast<const bf16x8*>(xs + m * KS + mx4_swz(4 * c + d) * 8);
#pragma unroll
          for (int j = 0; j < CPW; ++j)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              float a = acc[j * MR + m];
              a = __builtin_amdgcn_fdot2_f32_bf16(wb2[j][4 * d + 0], LSD_PAIR(x[d], 0), a, false);
              a = __builtin_amdgcn_fdot2_f32_bf16(wb2[j][4 * d + 1], LSD_PAIR(x[d], 1), a, false);
              a = __builtin_amdgcn_fdot2_f32_bf16(wb2[j][4 * d + 2], LSD_PAIR(x[d], 2), a, false);
              a = __builtin_amdgcn_fdot2_f32_bf16(wb2[j][4 * d + 3], LSD_PAIR(x[d], 3), a, false);
              acc[j * MR + m] = a;
            }
        }
      }
    } else if constexpr (W8) {
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        const int c = lane + 64 * i;  // 16 weights against LDS elements [16 c, 16 c + 16)
        bf16x2 wb2[CPW][8];
#pragma unroll
        for (int j = 0; j < CPW; ++j) cvt16(wq[j][i], wb2[j]);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(xs + m * KS + c * 16);
          const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(xs + m * KS + c * 16 + 8);
#pragma unroll
          for (int j = 0; j < CPW; ++j) acc[j * MR + m] = dot16(wb2[j], x0, x1, acc[j * MR + m]);
        }
      }
    } else {
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int c = lane + 64 * i;
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const bf16x8 xv = *reinterpret_cast<const bf16x8*>(xs + m * KS + c * 8);
#pragma unroll
        for (int j = 0; j < CPW; ++j) acc[j * MR + m] = dot8(wv[j][i], xv, acc[j * MR + m]);
      }
    }
    }

    // ---- 5. butterfly reduce-scatter over the wave (DPP / permlane swaps):
    // halving steps leave each lane group with the full sum of one value
    // idx; the remaining steps are plain pairwise sums
    int idx = 0;
    gv_step<32, V>(acc, idx, lane);
    gv_step<16, (V > 1 ? V / 2 : 1)>(acc, idx, lane);
    gv_step<8, (V > 2 ? V / 4 : 1)>(acc, idx, lane);
    gv_step<4, (V > 4 ? V / 8 : 1)>(acc, idx, lane);
    gv_step<2, (V > 8 ? V / 16 : 1)>(acc, idx, lane);
    gv_step<1, 1>(acc, idx, lane);
    if ((lane & (64 / V - 1)) == 0) red[w * 16 + idx] = acc[0];
    LSD_GV_SYNC();

    // ---- 6. fused epilogue, one thread per (wave, output); operands prefetched in step 0
    if (epi_thread) {
      const int w2 = e_w2, o = e_o;
      const int gw2 = blockIdx.x * 4 + w2;
      const float* rv = red + w2 * 16;
      if constexpr (EPI == gv::SILU) {
        const int jj = o / MR, m = o % MR;
        const int col = gw2 * (CPW / 2) + jj;
        if (m < M && col < (p.N >> 1)) {
          float g = rv[(2 * jj) * MR + m], u = rv[(2 * jj + 1) * MR + m];
          if constexpr (W8) {
            g *= e_sc;
            u *= e_scp;
          }
          reinterpret_cast<bf16*>(p.out)[(long)m * p.ldo + col] = f2bf(silu(g) * u);
        }
      } else if (e_live) {
        const int j = e_j, m = e_m, n = e_n;
        float y;
        if constexpr (W8) y = fmaf(rv[j * MR + m], e_sc, e_bias);
        else y = rv[j * MR + m] + e_bias;
        if constexpr (EPI == gv::F32) {
          reinterpret_cast<float*>(p.out)[(long)m * p.ldo + n] = y;
          if (p.segmax && tid == 0) {
            // this workgroup's 8 columns are one sampler segment: its maximum
            // per row, from the same fp32 values stored above (bit-equal to a
            // max over the stored logits)
#pragma unroll
            for (int mm = 0; mm < MR; ++mm) {
              if (mm >= M) break;
              float mx = -INFINITY;
#pragma unroll
              for (int w3 = 0; w3 < 4; ++w3)
#pragma unroll
                for (int j3 = 0; j3 < CPW; ++j3) {
                  const int n3 = (blockIdx.x * 4 + w3) * CPW + j3;
                  if constexpr (W8) {
                    if (n3 < p.N) mx = fmaxf(mx, fmaf(red[w3 * 16 + j3 * MR + mm], wscale[n3], p.bias ? bf2f(p.bias[n3]) : 0.f));
                  } else {
                  if (n3 < p.N) mx = fmaxf(mx, red[w3 * 16 + j3 * MR + mm] + (p.bias ? bf2f(p.bias[n3]) : 0.f));
                  }
                }
              p.segmax[(long)mm * p.ldseg + blockIdx.x] = mx;
            }
          }
        } else if constexpr (EPI == gv::RESID) {
          reinterpret_cast<float*>(p.out)[(long)m * p.ldo + n] = e_x + y;
        } else if constexpr (EPI == gv::BF16 || EPI == gv::GELU) {
          reinterpret_cast<bf16*>(p.out)[(long)m * p.ldo + n] = f2bf(EPI == gv::GELU ? gelu_new(y) : y);
        } else if constexpr (EPI == gv::QKV) {
          const int qk = p.q_size + p.kv_size;
          const int pos = e_pos;
          if (CPW % 2 == 0 && p.rope != nullptr && n < qk) {
            // RoPE pairs (2i, 2i+1) are this wave's rows j, j^1 (ops/hip.py
            // rope_pair_permutation makes the rotated pairs adjacent)
            float yp;
            if constexpr (W8) yp = fmaf(rv[(j ^ 1) * MR + m], e_scp, e_biasp);
            else yp = rv[(j ^ 1) * MR + m] + e_biasp;
            const int d = (n < p.q_size ? n : n - p.q_size) % p.hd;
            y = (d & 1) ? (y * e_cs0 + yp * e_cs1) : (y * e_cs0 - yp * e_cs1);
          }
          if (n < p.q_size) {
            reinterpret_cast<bf16*>(p.out)[(long)m * p.ldo + n] = f2bf(y);
          } else {
            const int c = n < qk ? n - p.q_size : n - qk;
            bf16* cache = n < qk ? p.kc : p.vc;
            const long idx = (((long)e_slot * p.n_kv + c / p.hd) * p.max_seq + pos) * p.hd + c % p.hd;
            if (p.kv_fp8) reinterpret_cast<unsigned char*>(cache)[idx] = fp8_enc(y);  // uniform: FP8 E4M3 cache
            else cache[idx] = f2bf(y);
          }
        }
      }
    }
  }
