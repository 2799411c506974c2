// Weight-streaming GEMV for small batches (B <= 4 rows, or P pairs of rows): the LDS-staged streaming kernel, the
// register-resident kernel of the LLM decode shapes, and the routing between them.
//
// Replaces the Linear layers of LlamaTransformerBlock / TransformerBlock.local_kvcache_inference
// (landiff/llm/modules/transformer_blocks.py:22-40,67-88,128-236), the head of GPT.sample (landiff/llm/models/transformer.py:91-119)
// and the batch-2 Linear layers of the DiT's conditioning path (time_embed / adaLN_modulation,
// landiff/diffusion/dit_video_concat.py:568,764-768).
//
// MI355X notes: the decode step is pure weight streaming (4.06 GB bf16 per step); every weight row is
// read exactly once with 16-byte loads straight into VGPRs (no LDS round trip for an operand that is
// not shared across waves), one wave64 per output row, activations (<= 4 x K bf16) stay in L1/L2.
#include "ld_llm.h"
#include <stdlib.h>
#include "../../include/landiff_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------
// GEMV: y[b][n] = epi( sum_k in_act(x[b][k]) * W[n][k] ), one wave per output row.
// ---------------------------------------------------------------------------------------------
struct GemvParams {
  const void* x;        // [B][ldx] bf16 or f32
  const void* W;        // [N][K] bf16 or f32
  const void* W2;       // optional second matrix (gated MLP: act(W x) * (W2 x))
  const bf16_t* bias;   // [N] or null
  const void* resid;    // [B][ldr] or null (bf16, or f32 when out_f32)
  void* out;            // [B][ldo]
  int B, N, K;
  long ldx, ldo, ldr;
  int x_f32, w_f32, out_f32;
  int in_act, act;
  const float* norm_w;  // optional fused RMSNorm of x (bf16 x only, never with in_act: gemv_check): xn = bf16(x * rsqrt(mean(x^2)+eps) * norm_w)
  float norm_eps;
  ChainSync cs;         // dependent-launch form (ld_gemv_reg_kernel<..., CHAIN = true> only)
};

// Weight-streaming GEMV.  One workgroup = 4 waves x R rows.  The activation rows (B x K, optionally RMS-normalised,
// optionally passed through in_act) are staged ONCE per workgroup in LDS as bf16/fp32 -- letting every wave re-read x
// from L2 made all CUs hammer the same few cache lines -- and the first trip's weight loads are issued BEFORE the
// staging so the HBM latency of the weights overlaps it.  Each lane keeps R*U 16-byte weight loads in flight.
template <int B, bool WF32, int R, int U = 4>     // U: 16-byte loads per lane, row and trip (short rows, K <= 512: U = 1 and more rows per wave)
__global__ __launch_bounds__(256) void ld_gemv_kernel(GemvParams p) {
  extern __shared__ __attribute__((aligned(16))) char gsm[];   // x staged: [B][K] (bf16, or f32 when WF32) + 64 B scratch
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool gated = !WF32 && p.W2 != nullptr;       // gated form runs with R == 1: rows n0 of W and of W2
  const int nchunk = p.K >> 3;                       // 8 elements per chunk
  const int nrow = p.N;

  // work item = (row group, K trip); a wave walks its items in order, always holding the NEXT item's weight vectors
  // in registers (raw 16-byte loads, converted to fp32 only when consumed)
  const int ntrip = (nchunk + 64 * U - 1) / (64 * U);
  const int ngroups = (nrow + R - 1) / R;
  const int wave_global = blockIdx.x * 4 + wave, nwaves = gridDim.x * 4;
  // epilogue operands of an item (lane r < R owns output row grp * R + r): requested with the item's last weight trip, so
  // that their latency is not paid per item after the reduction (it was: 1.3 TB/s on short rows)
  float e_bias_n = 0.f, e_res_n[B];
#pragma unroll
  for (int b = 0; b < B; ++b) e_res_n[b] = 0.f;
  auto load_w = [&](u32x4_t (&w)[R][U], u32x4_t (&w2)[U], int grp, int trip) {
    if (trip == ntrip - 1 && lane < R && grp < ngroups && grp * R + lane < nrow) {
      const int n = grp * R + lane;
      if (p.bias) e_bias_n = bf2f(p.bias[n]);
      if (p.resid) {
#pragma unroll
        for (int b = 0; b < B; ++b)
          e_res_n[b] = p.out_f32 ? ((const float*)p.resid)[b * p.ldr + n] : bf2f(((const bf16_t*)p.resid)[b * p.ldr + n]);
      }
    }
    const int c0 = lane + trip * 64 * U;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = c0 + 64 * u;
      const bool ok = (c < nchunk) && (grp < ngroups);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int n = (grp * R + r < nrow) ? grp * R + r : nrow - 1;
        w[r][u] = (u32x4_t){0u, 0u, 0u, 0u};
        if (ok) {
          if (WF32) {
            // fp32 weights: two 16-byte halves are fetched at use time (head GEMV only; not worth double buffering)
          } else {
            w[r][u] = __builtin_nontemporal_load((const u32x4_t*)((const bf16_t*)p.W + (long)n * p.K + c * 8));
          }
        }
      }
      if (gated) {
        const int n = (grp < nrow) ? grp : nrow - 1;
        w2[u] = (u32x4_t){0u, 0u, 0u, 0u};
        if (ok) w2[u] = __builtin_nontemporal_load((const u32x4_t*)((const bf16_t*)p.W2 + (long)n * p.K + c * 8));
      }
    }
  };

  u32x4_t wn[R][U], w2n[U];
  int grp = wave_global, trip = 0;
  load_w(wn, w2n, grp, trip);                        // first item in flight while x is staged

  // ---- stage x (with the optional fused RMSNorm / input activation) ----
  float* red = (float*)(gsm + (size_t)B * p.K * (WF32 ? 4 : 2));
  float rs[B];
#pragma unroll
  for (int b = 0; b < B; ++b) rs[b] = 1.f;
  if (p.norm_w) {                                    // RMSNorm scale per row (transformer_blocks.py:22-40)
    float ss[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      ss[b] = 0.f;
      for (int c = tid; c < nchunk; c += 256) {
        const u32x4_t a = *(const u32x4_t*)((const bf16_t*)p.x + b * p.ldx + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float lo = bf_lo(a[e]), hi = bf_hi(a[e]); ss[b] += lo * lo + hi * hi; }
      }
      ss[b] = wave_sum(ss[b]);
      if (lane == 0) red[wave * B + b] = ss[b];
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < B; ++b)
      rs[b] = rsqrtf((red[b] + red[B + b] + red[2 * B + b] + red[3 * B + b]) / (float)p.K + p.norm_eps);
  }
  for (int i = tid; i < B * nchunk; i += 256) {
    const int b = i / nchunk, c = i - b * nchunk;
    float xv[8];
    if (p.x_f32) {
      const f32x4_t a = *(const f32x4_t*)((const float*)p.x + b * p.ldx + c * 8);
      const f32x4_t b4 = *(const f32x4_t*)((const float*)p.x + b * p.ldx + c * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { xv[e] = a[e]; xv[4 + e] = b4[e]; }
    } else {
      const u32x4_t a = *(const u32x4_t*)((const bf16_t*)p.x + b * p.ldx + c * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) { xv[2 * e] = bf_lo(a[e]); xv[2 * e + 1] = bf_hi(a[e]); }
    }
    if (p.in_act) {
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[e] = rbf(apply_act(p.in_act, xv[e]));
    }
    if (p.norm_w) {
      const f32x4_t g0 = *(const f32x4_t*)(p.norm_w + c * 8), g1 = *(const f32x4_t*)(p.norm_w + c * 8 + 4);
      float r1 = rs[0];
#pragma unroll
      for (int bb = 1; bb < B; ++bb) r1 = (b == bb) ? rs[bb] : r1;
#pragma unroll
      for (int e = 0; e < 4; ++e) { xv[e] = xv[e] * r1 * g0[e]; xv[4 + e] = xv[4 + e] * r1 * g1[e]; }
    }
    if (WF32) {
      float* d = (float*)gsm + (long)b * p.K + c * 8;
      *(f32x4_t*)d = (f32x4_t){xv[0], xv[1], xv[2], xv[3]};
      *(f32x4_t*)(d + 4) = (f32x4_t){xv[4], xv[5], xv[6], xv[7]};
    } else {
      u32x4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(xv[2 * e], xv[2 * e + 1]);     // bf16 rounding of the normed x
      *(u32x4_t*)((bf16_t*)gsm + (long)b * p.K + c * 8) = o;
    }
  }
  __syncthreads();

  float acc[R][B], acc2[B];
  while (grp < ngroups) {
    u32x4_t wc[R][U], w2c[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int r = 0; r < R; ++r) wc[r][u] = wn[r][u];
      w2c[u] = w2n[u];
    }
    const int cgrp = grp, ctrip = trip;
    const float e_bias = e_bias_n;
    float e_res[B];
#pragma unroll
    for (int b = 0; b < B; ++b) e_res[b] = e_res_n[b];
    if (++trip == ntrip) { trip = 0; grp += nwaves; }
    load_w(wn, w2n, grp, trip);                       // prefetch the next item
    if (ctrip == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int b = 0; b < B; ++b) acc[r][b] = 0.f;
#pragma unroll
      for (int b = 0; b < B; ++b) acc2[b] = 0.f;
    }
    const int c0 = lane + ctrip * 64 * U;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = c0 + 64 * u;
      if (c >= nchunk) continue;
      float wf[R][8], w2f[8];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (WF32) {
          const int n = (cgrp * R + r < nrow) ? cgrp * R + r : nrow - 1;
          const f32x4_t a = *(const f32x4_t*)((const float*)p.W + (long)n * p.K + c * 8);
          const f32x4_t b4 = *(const f32x4_t*)((const float*)p.W + (long)n * p.K + c * 8 + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) { wf[r][e] = a[e]; wf[r][4 + e] = b4[e]; }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) { wf[r][2 * e] = bf_lo(wc[r][u][e]); wf[r][2 * e + 1] = bf_hi(wc[r][u][e]); }
        }
      }
      if (gated) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { w2f[2 * e] = bf_lo(w2c[u][e]); w2f[2 * e + 1] = bf_hi(w2c[u][e]); }
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        float xv[8];
        if (WF32) {
          const float* d = (const float*)gsm + (long)b * p.K + c * 8;
          const f32x4_t a = *(const f32x4_t*)d, b4 = *(const f32x4_t*)(d + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) { xv[e] = a[e]; xv[4 + e] = b4[e]; }
        } else {
          const u32x4_t a = *(const u32x4_t*)((const bf16_t*)gsm + (long)b * p.K + c * 8);
#pragma unroll
          for (int e = 0; e < 4; ++e) { xv[2 * e] = bf_lo(a[e]); xv[2 * e + 1] = bf_hi(a[e]); }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[r][b] = fmaf(xv[e], wf[r][e], acc[r][b]);
        if (gated) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc2[b] = fmaf(xv[e], w2f[e], acc2[b]);
        }
      }
    }
    if (ctrip == ntrip - 1) {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int b = 0; b < B; ++b) acc[r][b] = wave_sum(acc[r][b]);
      if (gated) {
#pragma unroll
        for (int b = 0; b < B; ++b) acc2[b] = wave_sum(acc2[b]);
      }
      // every lane holds all R x B totals after the butterflies: lane r finishes row r
      const int n = cgrp * R + lane;
      if (lane < R && n < nrow) {
#pragma unroll
        for (int b = 0; b < B; ++b) {
          float v = 0.f, v2 = 0.f;
#pragma unroll
          for (int r = 0; r < R; ++r) v = (lane == r) ? acc[r][b] : v;
          if (gated) v2 = acc2[b];
          if (p.bias) v += e_bias;
          if (!WF32) v = rbf(v);                         // bf16 Linear output
          if (p.act) v = rbf(apply_act(p.act, v));
          if (gated) v = rbf(v * rbf(v2));
          if (p.resid) v = p.out_f32 ? e_res[b] + v : rbf(e_res[b] + v);
          if (p.out_f32) ((float*)p.out)[b * p.ldo + n] = v;
          else ((bf16_t*)p.out)[b * p.ldo + n] = f2bf(v);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Register-resident GEMV for bf16 x / bf16 W (the LLM decode shapes).  One workgroup = R consecutive output rows; its
// 256 threads split K (thread t owns the 16-byte chunks t, t+256, ...: J of them), so every load instruction of the
// workgroup covers 4 KB of one weight row.  There is no loop: each thread issues its x chunks, then ALL of its R*J
// (x2 when gated) weight loads, and only then starts on the RMSNorm -- the whole matrix is in flight across the
// resident workgroups from the first microsecond, which is what a 5-25 us kernel needs to get near the HBM rate
// (tools/probe/hbm_probe.hip: 5.0 / 5.9 / 6.4 TB/s for 25 / 45 / 90 MB reads at this launch granularity).
// Dot products use v_dot2_f32_bf16 on the packed operands (bf16 products are exact in fp32); the R*B (x2) partial
// sums are reduced across the wave with a transposing butterfly (V + 6 - log2 V shuffles for V values instead of
// 6 V) and across the 4 waves through LDS.
// ---------------------------------------------------------------------------------------------
// CHAIN: the dependent-launch form (ld_llm_dev.h: ChainSync) -- the first batch of weight rows is requested BEFORE the wait for
// the previous operation, x / residual / outputs go through sc1 accesses, the workgroup arrives on its counter at the end;
// at most 128 registers so that two such launches are always resident side by side (grids capped at 512 workgroups).
template <int B, int R, int J, bool GATED, bool NORM, bool CHAIN = false>
__global__ __launch_bounds__(256, CHAIN ? 4 : 1) void ld_gemv_reg_kernel(GemvParams p, int nbatch) {
  constexpr int NV = R * B * (GATED ? 2 : 1), V = ceil_pow2(NV), LOGV = ilog2(V);
  constexpr int XAUX = CHAIN ? 16 : 0;                 // sc1 on the activation loads
  __shared__ float red[2][4][V];
  __shared__ float ssq[4][B];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunk = p.K >> 3;
  const int er = tid / B, eb = tid - er * B;          // this thread's epilogue output within a batch: (row er, batch row eb)

  u32x4_t wn[R][J], w2n[GATED ? R : 1][J];
  // epilogue operands are kept as loaded (raw bits) until the epilogue converts them: a conversion here would make wave 0 wait
  // for the batch it has just requested (loads return in order) before it computes the current one
  uint32_t e_bias_n = 0u, e_res_n = 0u;
  // request one batch (R consecutive weight rows + the epilogue operands of its outputs)
  auto request = [&](int batch) {
    const int n0 = batch * R;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long row = (n0 + r < p.N) ? n0 + r : p.N - 1;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int c = j * 256 + tid;
        wn[r][j] = (u32x4_t){0u, 0u, 0u, 0u};
        if (c < nchunk) wn[r][j] = __builtin_nontemporal_load((const u32x4_t*)((const bf16_t*)p.W + row * p.K + c * 8));
        if (GATED) {
          w2n[r][j] = (u32x4_t){0u, 0u, 0u, 0u};
          if (c < nchunk) w2n[r][j] = __builtin_nontemporal_load((const u32x4_t*)((const bf16_t*)p.W2 + row * p.K + c * 8));
        }
      }
    }
    const int en = n0 + er;
    if (tid < R * B && en < p.N) {
      if (p.bias) e_bias_n = p.bias[en];
      if (p.resid) {
        if (CHAIN) e_res_n = __hip_atomic_load((const bf16_t*)p.resid + eb * p.ldr + en, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else e_res_n = p.out_f32 ? ((const uint32_t*)p.resid)[eb * p.ldr + en] : (uint32_t)((const bf16_t*)p.resid)[eb * p.ldr + en];
      }
    }
  };

  // ---- x (L2) and the RMSNorm gains first, then the first batch of weight rows (HBM): all in flight together ----
  u32x4_t xq[B][J];
  f32x4_t g0[NORM ? J : 1], g1[NORM ? J : 1];
  // bounds-checked buffer loads (chunks past K read as zero): no branch and no zero-initialised destination -- with predicated
  // global loads the register allocator placed a v_mov behind every x load and the wave waited for each load in turn BEFORE the
  // first weight row had been requested (one L2 round trip per launch, six in the K = 11008 form)
  int batch = blockIdx.x;
  if (CHAIN) {                                         // weights do not depend on the previous operation: request, then wait for it
    request(batch);
    chain_wait(p.cs, tid);
  }
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)((const bf16_t*)p.x + b * p.ldx), 0, p.K * 2, 0x00020000);
#pragma unroll
    for (int j = 0; j < J; ++j) xq[b][j] = __builtin_amdgcn_raw_buffer_load_b128(rx, (j * 256 + tid) * 16, 0, XAUX);
  }
  if (NORM) {
    const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)p.norm_w, 0, p.K * 4, 0x00020000);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const u32x4_t a = __builtin_amdgcn_raw_buffer_load_b128(rg, (j * 256 + tid) * 32, 0, 0);
      const u32x4_t b = __builtin_amdgcn_raw_buffer_load_b128(rg, (j * 256 + tid) * 32 + 16, 0, 0);
      g0[j] = __builtin_bit_cast(f32x4_t, a); g1[j] = __builtin_bit_cast(f32x4_t, b);
    }
  }
  if (!CHAIN) request(batch);

  // ---- x: optional fused RMSNorm (transformer_blocks.py:22-40), back to packed bf16 ----
  if (NORM) {
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const float ss = wave_sum(chunks_sumsq<J>(xq[b]));
      if (lane == 0) ssq[wave][b] = ss;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const float r1 = rsqrtf((ssq[0][b] + ssq[1][b] + ssq[2][b] + ssq[3][b]) / (float)p.K + p.norm_eps);
#pragma unroll
      for (int j = 0; j < J; ++j) {
        if (j * 256 + tid < nchunk) {
          const u32x4_t a = xq[b][j];
          xq[b][j] = (u32x4_t){pack_bf16x2(bf_lo(a[0]) * r1 * g0[j][0], bf_hi(a[0]) * r1 * g0[j][1]),
                               pack_bf16x2(bf_lo(a[1]) * r1 * g0[j][2], bf_hi(a[1]) * r1 * g0[j][3]),
                               pack_bf16x2(bf_lo(a[2]) * r1 * g1[j][0], bf_hi(a[2]) * r1 * g1[j][1]),
                               pack_bf16x2(bf_lo(a[3]) * r1 * g1[j][2], bf_hi(a[3]) * r1 * g1[j][3])};
        }
      }
    }
  }

  // ---- batches batch, batch + gridDim.x, ...: the next batch's rows are requested before this one is consumed ----
  int par = 0;
#pragma unroll 1
  for (; batch < nbatch; batch += gridDim.x, par ^= 1) {
    u32x4_t w[R][J], w2[GATED ? R : 1][J];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < J; ++j) { w[r][j] = wn[r][j]; if (GATED) w2[r][j] = w2n[r][j]; }
    const uint32_t e_bias_raw = e_bias_n, e_res_raw = e_res_n;
    if (batch + (int)gridDim.x < nbatch) request(batch + gridDim.x);

    float v[V];
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < J; ++j)
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[r * B + b] = dot2_bf16(w[r][j][e], xq[b][j][e], v[r * B + b]);
            if (GATED) v[R * B + r * B + b] = dot2_bf16(w2[r][j][e], xq[b][j][e], v[R * B + r * B + b]);
          }
    wave_sum_multi<V>(v, lane);
    if ((lane & ((64 >> LOGV) - 1)) == 0) red[par][wave][lane >> (6 - LOGV)] = v[0];
    __syncthreads();
    const int en = batch * R + er;
    if (tid < R * B && en < p.N) {
      const float(&rd)[4][V] = red[par];
      float a = rd[0][tid] + rd[1][tid] + rd[2][tid] + rd[3][tid];
      const float e_bias = bf2f((bf16_t)e_bias_raw), e_res = p.out_f32 ? __uint_as_float(e_res_raw) : bf2f((bf16_t)e_res_raw);
      if (p.bias) a += e_bias;
      a = rbf(a);                                        // bf16 Linear output
      if (p.act) a = rbf(apply_act(p.act, a));
      if (GATED) a = rbf(a * rbf(rd[0][R * B + tid] + rd[1][R * B + tid] + rd[2][R * B + tid] + rd[3][R * B + tid]));
      if (p.resid) a = p.out_f32 ? e_res + a : rbf(e_res + a);
      if (CHAIN) __hip_atomic_store((bf16_t*)p.out + eb * p.ldo + en, f2bf(a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else if (p.out_f32) ((float*)p.out)[eb * p.ldo + en] = a;
      else ((bf16_t*)p.out)[eb * p.ldo + en] = f2bf(a);
    }
  }
  if (CHAIN) chain_arrive(p.cs, tid, blockIdx.x);
}

template <int B, bool WF32, int R, int U = 4>
int launch_gemv_cfg(const GemvParams& p, hipStream_t st) {
  const size_t smem = (size_t)B * p.K * (WF32 ? 4 : 2) + 64;
  static thread_local LdSmemCache cache{};      // per instantiation
  if (int rc = ld_ensure_dyn_smem((const void*)ld_gemv_kernel<B, WF32, R, U>, smem, &cache)) return rc;
  // persistent grid: ~2 workgroups per CU (or fewer when there are not enough rows); every wave loops over row groups
  long blocks = (p.N + 4 * R - 1) / (4 * R);
  if (blocks > 512) blocks = 512;
  hipLaunchKernelGGL((ld_gemv_kernel<B, WF32, R, U>), dim3((unsigned)blocks), dim3(256), smem, st, p);
  return ld_check_launch("ld_gemv");
}

template <int B, int R, int J, bool GATED, bool NORM, bool CHAIN = false>
int launch_gemv_reg(const GemvParams& p, hipStream_t st, int* grid_out = nullptr) {
  // nbatch batches of R rows over at most `cap` workgroups (the chained form: 512, see the kernel), every workgroup taking the same
  // number of batches
  static const int cap_env = getenv("LD_GEMV_WGS") ? atoi(getenv("LD_GEMV_WGS")) : 768;
  const int cap = CHAIN ? 512 : cap_env;
  const int nbatch = (p.N + R - 1) / R;
  const int trips = (nbatch + cap - 1) / cap;
  const int grid = (nbatch + trips - 1) / trips;
  if (grid_out) *grid_out = grid;
  hipLaunchKernelGGL((ld_gemv_reg_kernel<B, R, J, GATED, NORM, CHAIN>), dim3((unsigned)grid), dim3(256), 0, st, p, nbatch);
  return ld_check_launch(CHAIN ? "ld_gemv(chained)" : "ld_gemv");
}

int gemv_mode() {
  static const int mode = getenv("LD_GEMV_MODE") ? atoi(getenv("LD_GEMV_MODE")) : 0;     // 1 = streaming-loop kernel only
  return mode;
}

int gemv_forced_r() {
  static const int forced_r = getenv("LD_GEMV_R") ? atoi(getenv("LD_GEMV_R")) : 0;       // rows per batch of the register kernel
  return forced_r;
}

// What a call will do (ld_gemv_route reports it; launch_gemv_b switches on it): the kernel and its template parameters.
enum { GEMV_STREAM = 0, GEMV_REG = 1 };
struct GemvPlan {
  int kind;   // GEMV_STREAM: ld_gemv_kernel<B, w_f32, R, U>; GEMV_REG: ld_gemv_reg_kernel<B, R, J, gated, normed>
  int J, R, U;
};

// The rows per batch the register kernel is instantiated with when `want` are asked for: R*J (x2 gated) 16-byte loads per thread
// in flight per batch, two batches deep.
constexpr int gemv_reg_rows(int B, int J, bool gated, int want) {
  const int L1 = J * (gated ? 2 : 1);                // loads per thread per row
  if (L1 <= 2 && B <= 2 && want >= 8) return 8;
  if (L1 <= 4 && want >= 4) return 4;
  return want >= 2 ? 2 : 1;
}

// The one statement of the dispatch.  Host logic only.
GemvPlan gemv_plan(int B, int N, int K, bool x_f32, bool w_f32, bool gated, bool in_act) {
  const int nchunk = K >> 3, forced_r = gemv_forced_r();
  if (gemv_mode() != 1 && !w_f32 && !x_f32 && !in_act) {
    int J = 0, want = 0;
    if (nchunk <= 256) { J = 1; want = 4; }                                    // measured: tools/gemv_shapes.py
    else if (nchunk <= 512) { J = 2; want = gated ? 2 : 4; }
    else if (B <= 2 && nchunk <= 1536 && !gated) { J = 6; want = 2; }
    if (J) return {GEMV_REG, J, gemv_reg_rows(B, J, gated, forced_r ? forced_r : want), 0};
  }
  if (w_f32) return {GEMV_STREAM, 0, 1, 4};
  // short rows (one 16-byte load per lane covers a row: the DiT's adaLN modulations, K = 512): eight rows per wave and trip
  // keep eight loads per lane in flight (1.3 -> 4+ TB/s on the 708 MB all-layers matrix)
  if (!gated && nchunk <= 64 && N >= 4096) return {GEMV_STREAM, 0, 8, 1};
  if (gated || N < 4096) return {GEMV_STREAM, 0, 1, 4};   // gated MLP, or few rows: keep all 256 CUs busy
  return {GEMV_STREAM, 0, 2, 4};                          // (one row per wave measured slower at N = 6144: 12.4 vs 11.5 us)
}

template <int B, int J, bool GATED, bool NORM>
int launch_gemv_reg_r(const GemvParams& p, int R, hipStream_t st) {
  if constexpr (gemv_reg_rows(B, J, GATED, 8) == 8) { if (R == 8) return launch_gemv_reg<B, 8, J, GATED, NORM>(p, st); }
  if constexpr (gemv_reg_rows(B, J, GATED, 4) == 4) { if (R == 4) return launch_gemv_reg<B, 4, J, GATED, NORM>(p, st); }
  if (R == 2) return launch_gemv_reg<B, 2, J, GATED, NORM>(p, st);
  return launch_gemv_reg<B, 1, J, GATED, NORM>(p, st);
}

template <int B, int J>
int launch_gemv_reg_j(const GemvParams& p, int R, hipStream_t st) {
  const bool gated = p.W2 != nullptr, norm = p.norm_w != nullptr;
  if constexpr (J <= 2) {
    if (gated) return norm ? launch_gemv_reg_r<B, J, true, true>(p, R, st) : launch_gemv_reg_r<B, J, true, false>(p, R, st);
  }
  return norm ? launch_gemv_reg_r<B, J, false, true>(p, R, st) : launch_gemv_reg_r<B, J, false, false>(p, R, st);
}

GemvPlan gemv_plan(const GemvParams& p, int B) { return gemv_plan(B, p.N, p.K, p.x_f32 != 0, p.w_f32 != 0, p.W2 != nullptr, p.in_act != 0); }

// J of the register form launch_gemv_b<2> takes for these operands (0: it takes the LDS-staged kernel).  J fixes the bits of a
// row's dot product (chunk ownership c = j * 256 + tid, the order of a thread's dot2 chain, the RMSNorm partial sums); R and B
// do not: every (weight row, activation row) has its own accumulator, wave_sum_multi pairs lanes 32, 16, ..., 1 apart for any V.
int gemv_pair_reg_j(const GemvParams& p) {
  const GemvPlan pl = gemv_plan(p, 2);
  return pl.kind == GEMV_REG ? pl.J : 0;
}

// ld_gemv_pairs, B = 2 P in {4, 6, 8}: ld_gemv_reg_kernel at the B = 2 route's J with all B activation rows in registers (B * J
// 16-byte chunks per thread; 8 x 11008 bf16 would not fit the LDS) -- a batch of R weight rows is requested once, held in
// registers and consumed by every pair, so the matrix is streamed from HBM once per call whatever P is.  R: rows per batch, by the
// register budget of one workgroup per CU (B * J * 4 for x, 2 * R * J * 4 (x2 gated) for two batches of weights, R * B (x2)
// partial sums).
template <int B>
int launch_gemv_pairs_b(const GemvParams& p, int J, hipStream_t st) {
  const bool gated = p.W2 != nullptr, norm = p.norm_w != nullptr;
  if (J == 1) {
    if (gated) return norm ? launch_gemv_reg<B, 4, 1, true, true>(p, st) : launch_gemv_reg<B, 4, 1, true, false>(p, st);
    return norm ? launch_gemv_reg<B, 4, 1, false, true>(p, st) : launch_gemv_reg<B, 4, 1, false, false>(p, st);
  }
  if (J == 2) {
    if (gated) return norm ? launch_gemv_reg<B, 2, 2, true, true>(p, st) : launch_gemv_reg<B, 2, 2, true, false>(p, st);
    return norm ? launch_gemv_reg<B, 4, 2, false, true>(p, st) : launch_gemv_reg<B, 4, 2, false, false>(p, st);
  }
  constexpr int R6 = B <= 4 ? 2 : 1;
  if constexpr (B <= 4) { if (norm) return launch_gemv_reg<B, R6, 6, false, true>(p, st); }
  return launch_gemv_reg<B, R6, 6, false, false>(p, st);     // (B > 4 with the norm: not here, see gemv_pairs_in_one_launch)
}

// J = 6 with the fused RMSNorm (gains in registers too) does not fit the register file beyond two pairs without spilling: those
// calls (no decode shape: the K = mlp projection has no norm in front) take the B = 2 route per pair like the non-register forms
bool gemv_pairs_in_one_launch(const GemvParams& p, int J) { return p.B > 2 && J != 0 && !(J == 6 && p.norm_w && p.B > 4); }

template <int B>
int launch_gemv_b(const GemvParams& p, hipStream_t st) {
  const GemvPlan pl = gemv_plan(p, B);
  if (pl.kind == GEMV_REG) {
    if (pl.J == 1) return launch_gemv_reg_j<B, 1>(p, pl.R, st);
    if (pl.J == 2) return launch_gemv_reg_j<B, 2>(p, pl.R, st);
    if constexpr (B <= 2) return launch_gemv_reg_j<B, 6>(p, pl.R, st);
    return ld_set_error(LD_ERR_UNSUPPORTED, "ld_gemv: no register form J = %d for B = %d", pl.J, B);
  }
  if (p.w_f32) return launch_gemv_cfg<B, true, 1>(p, st);
  if (pl.R == 8) return launch_gemv_cfg<B, false, 8, 1>(p, st);
  if (pl.R == 2) return launch_gemv_cfg<B, false, 2>(p, st);
  return launch_gemv_cfg<B, false, 1>(p, st);
}

// The argument rules of ld_gemv (ld_gemv_route answers with the same codes and messages; it has no ldx: 0).
int gemv_check(int64_t B, int64_t N, int64_t K, int64_t ldx, int32_t x_f32, int32_t w_f32, int32_t out_f32, bool gated, bool normed,
               int32_t in_act) {
  LD_REQUIRE(B >= 1 && B <= MAXB, "ld_gemv: batch %ld not in [1,%d]", (long)B, MAXB);
  LD_REQUIRE(N >= 1 && K >= 8 && K % 8 == 0 && ldx % 8 == 0, "ld_gemv: K and ldx must be multiples of 8");
  LD_REQUIRE((size_t)B * K * (w_f32 ? 4 : 2) + 64 <= 160 * 1024, "ld_gemv: B*K too large for the LDS-staged activations");
  LD_REQUIRE(!(w_f32 && gated), "ld_gemv: gated form needs bf16 weights");
  LD_REQUIRE(!w_f32 || (x_f32 && out_f32), "ld_gemv: fp32 weights need fp32 in/out");
  LD_REQUIRE(!normed || (!x_f32 && !w_f32), "ld_gemv: fused RMSNorm needs bf16 x and weights");
  LD_REQUIRE(!(in_act && normed), "ld_gemv: in_act with a fused RMSNorm is not a form (no caller has one)");
  return 0;
}

GemvParams make_gemv_params(const void* x, int64_t ldx, int32_t x_f32, const void* W, const void* W2, int32_t w_f32, const void* bias,
                            const void* resid, int64_t ldr, void* out, int64_t ldo, int32_t out_f32, int64_t B, int64_t N, int64_t K,
                            int32_t in_act, int32_t act, const float* norm_w, float norm_eps) {
  GemvParams p{};
  p.x = x; p.W = W; p.W2 = W2; p.bias = (const bf16_t*)bias; p.resid = resid; p.out = out;
  p.B = (int)B; p.N = (int)N; p.K = (int)K; p.ldx = ldx; p.ldo = ldo; p.ldr = ldr;
  p.x_f32 = x_f32; p.w_f32 = w_f32; p.out_f32 = out_f32; p.in_act = in_act; p.act = act;
  p.norm_w = norm_w; p.norm_eps = norm_eps;
  return p;
}

}  // namespace

LD_API int ld_gemv(const void* x, int64_t ldx, int32_t x_f32, const void* W, const void* W2, int32_t w_f32,
                   const void* bias, const void* resid, int64_t ldr, void* out, int64_t ldo, int32_t out_f32,
                   int64_t B, int64_t N, int64_t K, int32_t in_act, int32_t act, const float* norm_w, float norm_eps,
                   void* stream) {
  LD_REQUIRE(x && W && out, "ld_gemv: null pointer");
  if (int rc = gemv_check(B, N, K, ldx, x_f32, w_f32, out_f32, W2 != nullptr, norm_w != nullptr, in_act)) return rc;
  const GemvParams p = make_gemv_params(x, ldx, x_f32, W, W2, w_f32, bias, resid, ldr, out, ldo, out_f32, B, N, K, in_act, act, norm_w, norm_eps);
  hipStream_t st = (hipStream_t)stream;
  switch (B) {
    case 1: return launch_gemv_b<1>(p, st);
    case 2: return launch_gemv_b<2>(p, st);
    case 3: return launch_gemv_b<3>(p, st);
    default: return launch_gemv_b<4>(p, st);
  }
}

// ld_gemv's dispatch run dry: no HIP call.
LD_API int ld_gemv_route(int64_t B, int64_t N, int64_t K, int32_t x_f32, int32_t w_f32, int32_t out_f32, int32_t gated, int32_t normed,
                         int32_t in_act, int32_t* J, int32_t* R, int32_t* U) {
  if (int rc = gemv_check(B, N, K, 0, x_f32, w_f32, out_f32, gated != 0, normed != 0, in_act)) return rc;
  const GemvPlan pl = gemv_plan((int)B, (int)N, (int)K, x_f32 != 0, w_f32 != 0, gated != 0, in_act != 0);
  if (J) *J = pl.J;
  if (R) *R = pl.R;
  if (U) *U = pl.U;
  return pl.kind;
}

// ld_gemv for P = B / 2 pairs of activation rows (P samples of one prompt decoded side by side): rows (2p, 2p+1) come out with
// the bits ld_gemv(B = 2) gives for them.  Register forms: one launch, every weight row read once.  Everything else (the fp32
// head, LD_GEMV_MODE=1, K beyond the register forms): the B = 2 route once per pair.
LD_API int ld_gemv_pairs(const void* x, int64_t ldx, int32_t x_f32, const void* W, const void* W2, int32_t w_f32,
                         const void* bias, const void* resid, int64_t ldr, void* out, int64_t ldo, int32_t out_f32,
                         int64_t B, int64_t N, int64_t K, int32_t in_act, int32_t act, const float* norm_w, float norm_eps,
                         void* stream) {
  LD_REQUIRE(x && W && out, "ld_gemv_pairs: null pointer");
  LD_REQUIRE(B >= 2 && B % 2 == 0, "ld_gemv_pairs: %ld rows are not pairs", (long)B);
  if (B > 2 * LD_LLM_MAX_PAIRS) return ld_set_error(LD_ERR_UNSUPPORTED, "ld_gemv_pairs: %ld pairs, at most %d", (long)(B / 2), LD_LLM_MAX_PAIRS);
  LD_REQUIRE(N >= 1 && K >= 8 && K % 8 == 0 && ldx % 8 == 0, "ld_gemv_pairs: K and ldx must be multiples of 8");
  LD_REQUIRE((size_t)2 * K * (w_f32 ? 4 : 2) + 64 <= 160 * 1024, "ld_gemv_pairs: K too large for the LDS-staged activations");
  LD_REQUIRE(!(w_f32 && W2), "ld_gemv_pairs: gated form needs bf16 weights");
  LD_REQUIRE(!w_f32 || (x_f32 && out_f32), "ld_gemv_pairs: fp32 weights need fp32 in/out");
  LD_REQUIRE(!norm_w || (!x_f32 && !w_f32), "ld_gemv_pairs: fused RMSNorm needs bf16 x and weights");
  LD_REQUIRE(!(in_act && norm_w), "ld_gemv_pairs: in_act with a fused RMSNorm is not a form (no caller has one)");
  const GemvParams p = make_gemv_params(x, ldx, x_f32, W, W2, w_f32, bias, resid, ldr, out, ldo, out_f32, B, N, K, in_act, act, norm_w, norm_eps);
  hipStream_t st = (hipStream_t)stream;
  const int J = gemv_pair_reg_j(p);
  if (gemv_pairs_in_one_launch(p, J)) {
    switch (B) {
      case 4: return launch_gemv_pairs_b<4>(p, J, st);
      case 6: return launch_gemv_pairs_b<6>(p, J, st);
      default: return launch_gemv_pairs_b<8>(p, J, st);
    }
  }
  const long xs = x_f32 ? 4 : 2, os = out_f32 ? 4 : 2;
  for (int64_t b = 0; b < B; b += 2) {
    const int rc = ld_gemv((const char*)x + b * ldx * xs, ldx, x_f32, W, W2, w_f32, bias, resid ? (const char*)resid + b * ldr * os : nullptr,
                           ldr, (char*)out + b * ldo * os, ldo, out_f32, 2, N, K, in_act, act, norm_w, norm_eps, stream);
    if (rc) return rc;
  }
  return 0;
}

#ifdef LD_VARIANTS   // the dependent-launch form of a decode step: measured slower, only in the variants build
// the register GEMV in its dependent-launch form (B = 2): variant choice of launch_gemv_b, <= 128 registers, <= 512 workgroups
template <int R, int J, bool GATED, bool NORM>
static int launch_gemv_chain(const GemvParams& p, hipStream_t st, int* grid_out) { return launch_gemv_reg<2, R, J, GATED, NORM, true>(p, st, grid_out); }

int ld_gemv_chain_launch(const void* x, int64_t ldx, const void* W, const void* W2, const void* resid, void* out, int64_t ldo,
                         int64_t N, int64_t K, int act, const float* norm_w, float norm_eps, ChainSync cs, hipStream_t st,
                         int* grid_out) {
  GemvParams p = make_gemv_params(x, ldx, 0, W, W2, 0, nullptr, resid, ldo, out, ldo, 0, 2, N, K, 0, act, norm_w, norm_eps);
  p.cs = cs;
  const int nchunk = p.K >> 3;
  const bool gated = p.W2 != nullptr, norm = p.norm_w != nullptr;
  if (nchunk <= 256) {
    if (gated) return norm ? launch_gemv_chain<4, 1, true, true>(p, st, grid_out) : ld_set_error(LD_ERR_UNSUPPORTED, "chained gemv: gated without norm");
    return norm ? launch_gemv_chain<4, 1, false, true>(p, st, grid_out) : launch_gemv_chain<4, 1, false, false>(p, st, grid_out);
  }
  if (nchunk <= 512) {
    if (gated) return norm ? launch_gemv_chain<2, 2, true, true>(p, st, grid_out) : ld_set_error(LD_ERR_UNSUPPORTED, "chained gemv: gated without norm");
    return norm ? launch_gemv_chain<4, 2, false, true>(p, st, grid_out) : launch_gemv_chain<4, 2, false, false>(p, st, grid_out);
  }
  if (nchunk <= 1536 && !gated && !norm) return launch_gemv_chain<1, 6, false, false>(p, st, grid_out);
  return ld_set_error(LD_ERR_UNSUPPORTED, "chained gemv: K = %d outside the register forms", p.K);
}
#endif  // LD_VARIANTS
