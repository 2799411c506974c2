// Weight-streaming skinny GEMM on v_mfma_f32_32x32x16_bf16: the second engine of the batched AR decode (ld_gemv_wide).
//
// out[b][n] = epi( sum_k xn[b][k] * W[n][k] ) for B <= 32 activation rows (up to 16 (cond, uncond) pairs of one prompt, Semantic1DLM.sample
// once per seed, lm_model.py:417-508, over the cached blocks of transformer_blocks.py:128-236).  The register GEMV of ld_llm_gemv.hip
// (ld_gemv_pairs) keeps all B activation rows in registers and stops at B = 8; here 32 weight rows are the MFMA's 32-row operand and
// the B activation rows are its 32 columns (columns >= B are zero operands), so every weight byte is read from HBM once for all rows.
//
// Decomposition: one workgroup of 8 waves = one tile of 32 weight rows over the WHOLE of K.  K is walked in slices of 2048; within a
// slice wave w owns the 16 MFMA steps (16 k each) [16w, 16w + 16): 256 contiguous bytes of each of its 32 rows, one 16-byte nontemporal
// load per lane and step, HBM -> VGPR (no LDS round trip for an operand no other wave shares); the next slice's loads are issued
// before this slice's MFMAs.  The activations are the shared operand: staged per slice through the LDS as bf16 (RMS-normalised on
// the way, the scale computed once per workgroup).  The 8 partial tiles are summed through the LDS in wave order 0..7.
// There is no split of K across workgroups and no second pass: N = 2048 runs on 64 workgroups of 512 threads.
//
// Bits: output column b of an MFMA depends on operand column b alone, and the order of the fp32 sum (step order inside a wave, wave
// order in the merge, thread / wave order of the RMSNorm sum of squares) is a function of K alone -- what row b gets does not depend
// on B, on the row's index or on the other rows.  Rounding points are ld_gemv_kernel's: bf16 normalised activations, fp32
// accumulation, fp32 epilogue, one rounding to bf16 per Linear output / activation / product / residual sum.
#include "ld_common.h"
#include "../../include/landiff_hip.h"

namespace {

constexpr int WIDE_WAVES = 8;                           // waves per workgroup (two per SIMD: 256 registers each)
constexpr int WIDE_SPW = 16;                            // MFMA steps (16 k) per wave and slice
constexpr int WIDE_SLICE = WIDE_WAVES * WIDE_SPW * 16;  // k per slice: 2048
constexpr int WIDE_XLD = WIDE_SLICE * 2 + 16;           // bytes per staged activation row (+16: the 32 columns of a B fragment start in different banks)
constexpr int WIDE_RLD = 33;                            // words per 32-column group of a partial tile in the merge buffer

struct WideParams {
  const bf16_t* x;       // [B][ldx]
  const bf16_t* W;       // [N][K]
  const bf16_t* W2;      // gated form: act(W x) * (W2 x)
  const bf16_t* bias;    // [N] or null
  const bf16_t* resid;   // [B][ldr] or null (may be out)
  bf16_t* out;           // [B][ldo]
  int B, N, K;
  long ldx, ldo, ldr;
  int act;
  const float* norm_w;   // optional fused RMSNorm of x: xn = bf16(x * rsqrt(mean(x^2) + eps) * norm_w)
  float norm_eps;
};

template <bool GATED>
__global__ __launch_bounds__(WIDE_WAVES * 64) void ld_gemv_wide_kernel(WideParams p) {
  constexpr int NT = WIDE_WAVES * 64, G = GATED ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) char wsm[];   // activations of a slice [32][WIDE_XLD]; later the partial tiles
  __shared__ float ssq[WIDE_WAVES][32];
  __shared__ float rs_s[32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;              // fragment row (weights) / column (activations), and k half
  const int B = p.B, K = p.K;
  const int n0 = blockIdx.x * 32;
  const long wrow = (n0 + r < p.N) ? n0 + r : p.N - 1; // rows past N are read from the last row and never stored
  const int nslice = (K + WIDE_SLICE - 1) / WIDE_SLICE;

  u32x4_t wn[WIDE_SPW], w2n[GATED ? WIDE_SPW : 1];
  auto request = [&](int sl) {                         // this wave's 16 steps of slice sl (a step lies inside K as a whole: K % 16 == 0)
#pragma unroll
    for (int j = 0; j < WIDE_SPW; ++j) {
      const int k = sl * WIDE_SLICE + (wave * WIDE_SPW + j) * 16;
      wn[j] = (u32x4_t){0u, 0u, 0u, 0u};
      if (GATED) w2n[j] = (u32x4_t){0u, 0u, 0u, 0u};
      if (k < K) {
        wn[j] = __builtin_nontemporal_load((const u32x4_t*)(p.W + wrow * K + k + h * 8));
        if (GATED) w2n[j] = __builtin_nontemporal_load((const u32x4_t*)(p.W2 + wrow * K + k + h * 8));
      }
    }
  };
  request(0);                                          // the first slice's weights are in flight while x is normalised and staged

  // ---- RMSNorm scale per activation row (transformer_blocks.py:22-40): thread t sums chunks t, t + 512, ... of a row ----
  if (p.norm_w) {
    const int nchunk = K >> 3;
    for (int b = 0; b < B; ++b) {
      float ss = 0.f;
      for (int c = tid; c < nchunk; c += NT) {
        const u32x4_t a = *(const u32x4_t*)(p.x + b * p.ldx + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float lo = bf_lo(a[e]), hi = bf_hi(a[e]); ss += lo * lo + hi * hi; }
      }
      ss = wave_sum(ss);
      if (lane == 0) ssq[wave][b] = ss;
    }
    __syncthreads();
    if (tid < B) {
      float t = ssq[0][tid];
#pragma unroll
      for (int w = 1; w < WIDE_WAVES; ++w) t += ssq[w][tid];
      rs_s[tid] = rsqrtf(t / (float)K + p.norm_eps);
    }
    __syncthreads();
  }

  f32x16_t acc, acc2;
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc[e] = 0.f; acc2[e] = 0.f; }

#pragma unroll 1
  for (int sl = 0; sl < nslice; ++sl) {
    const int k0 = sl * WIDE_SLICE;
    const int kw = (K - k0 < WIDE_SLICE) ? K - k0 : WIDE_SLICE;
    const int nch = kw >> 3;
    if (sl > 0) __syncthreads();                       // the previous slice's fragments have been read
    // ---- stage activations [B][kw] of this slice: bf16, normalised with ld_gemv_kernel's expression and rounding ----
    for (int i = tid; i < B * nch; i += NT) {
      const int b = i / nch, c = i - b * nch;
      u32x4_t a = *(const u32x4_t*)(p.x + b * p.ldx + k0 + c * 8);
      if (p.norm_w) {
        const f32x4_t g0 = *(const f32x4_t*)(p.norm_w + k0 + c * 8), g1 = *(const f32x4_t*)(p.norm_w + k0 + c * 8 + 4);
        const float r1 = rs_s[b];
        a = (u32x4_t){pack_bf16x2(bf_lo(a[0]) * r1 * g0[0], bf_hi(a[0]) * r1 * g0[1]),
                      pack_bf16x2(bf_lo(a[1]) * r1 * g0[2], bf_hi(a[1]) * r1 * g0[3]),
                      pack_bf16x2(bf_lo(a[2]) * r1 * g1[0], bf_hi(a[2]) * r1 * g1[1]),
                      pack_bf16x2(bf_lo(a[3]) * r1 * g1[2], bf_hi(a[3]) * r1 * g1[3])};
      }
      *(u32x4_t*)(wsm + b * WIDE_XLD + c * 16) = a;
    }
    __syncthreads();
    // ---- the MFMA steps of this wave.  Plain form: the slice's weights leave the prefetch registers and the next slice's are
    //      requested before the MFMAs.  Gated form: two matrices' fragments fill most of a wave's registers, so the
    //      next request follows the MFMAs (its K is one slice in the decode) ----
    auto steps = [&](const u32x4_t (&wa)[WIDE_SPW], const u32x4_t (&wb)[GATED ? WIDE_SPW : 1]) {
#pragma unroll
      for (int j = 0; j < WIDE_SPW; ++j) {
        const int st = wave * WIDE_SPW + j;            // step within the slice (wave-uniform)
        if (k0 + st * 16 < K) {
          u32x4_t xb = (u32x4_t){0u, 0u, 0u, 0u};      // columns >= B: zero operands (their LDS rows are never written or read)
          if (r < B) xb = *(const u32x4_t*)(wsm + r * WIDE_XLD + st * 32 + h * 16);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, wa[j]), __builtin_bit_cast(bf16x8_t, xb), acc, 0, 0, 0);
          if (GATED)
            acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, wb[j]), __builtin_bit_cast(bf16x8_t, xb), acc2, 0, 0, 0);
        }
      }
    };
    if constexpr (GATED) {
      steps(wn, w2n);
      if (sl + 1 < nslice) request(sl + 1);
    } else {
      u32x4_t wc[WIDE_SPW];
#pragma unroll
      for (int j = 0; j < WIDE_SPW; ++j) wc[j] = wn[j];
      if (sl + 1 < nslice) request(sl + 1);
      steps(wc, w2n);
    }
  }

  // ---- merge the 8 partial tiles in wave order; element (row i, column b) of a tile sits at group (e * 2 + h) = f(i), word b ----
  __syncthreads();                                     // every wave is done with the staged activations
  float* red = (float*)wsm;                            // [8 waves][G][32 groups][WIDE_RLD]
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    red[((wave * G) * 32 + e * 2 + h) * WIDE_RLD + r] = acc[e];
    if (GATED) red[((wave * G + 1) * 32 + e * 2 + h) * WIDE_RLD + r] = acc2[e];
  }
  __syncthreads();
  // output -> (activation row b, tile row i): consecutive lanes write consecutive n of one output row
#pragma unroll
  for (int o = 0; o < 1024 / NT; ++o) {
    const int idx = tid + o * NT;
    const int b = idx >> 5, i = idx & 31;
    const int grp = ((i & 3) + 4 * (i >> 3)) * 2 + ((i >> 2) & 1);    // inverse of row = (e & 3) + 8 * (e >> 2) + 4 * h
    const int n = n0 + i;
    if (b < B && n < p.N) {
      float v = red[grp * WIDE_RLD + b], v2 = 0.f;
#pragma unroll
      for (int w = 1; w < WIDE_WAVES; ++w) v += red[((w * G) * 32 + grp) * WIDE_RLD + b];
      if (GATED) {
        v2 = red[(32 + grp) * WIDE_RLD + b];
#pragma unroll
        for (int w = 1; w < WIDE_WAVES; ++w) v2 += red[((w * G + 1) * 32 + grp) * WIDE_RLD + b];
      }
      // ld_gemv_kernel's epilogue
      if (p.bias) v += bf2f(p.bias[n]);
      v = rbf(v);                                      // bf16 Linear output
      if (p.act) v = rbf(apply_act(p.act, v));
      if (GATED) v = rbf(v * rbf(v2));
      if (p.resid) v = rbf(bf2f(p.resid[b * p.ldr + n]) + v);
      p.out[b * p.ldo + n] = f2bf(v);
    }
  }
}

template <bool GATED>
int launch_wide(const WideParams& p, hipStream_t st) {
  constexpr size_t x_bytes = (size_t)32 * WIDE_XLD, red_bytes = (size_t)WIDE_WAVES * (GATED ? 2 : 1) * 32 * WIDE_RLD * 4;
  constexpr size_t smem = x_bytes > red_bytes ? x_bytes : red_bytes;
  static thread_local LdSmemCache cache{};             // per instantiation
  if (int rc = ld_ensure_dyn_smem((const void*)ld_gemv_wide_kernel<GATED>, smem, &cache)) return rc;
  hipLaunchKernelGGL((ld_gemv_wide_kernel<GATED>), dim3((unsigned)((p.N + 31) / 32)), dim3(WIDE_WAVES * 64), smem, st, p);
  return ld_check_launch("ld_gemv_wide");
}

}  // namespace

LD_API int ld_gemv_wide(const void* x, int64_t ldx, int32_t x_f32, const void* W, const void* W2, int32_t w_f32,
                        const void* bias, const void* resid, int64_t ldr, void* out, int64_t ldo, int32_t out_f32,
                        int64_t B, int64_t N, int64_t K, int32_t in_act, int32_t act, const float* norm_w, float norm_eps,
                        void* stream) {
  LD_REQUIRE(x && W && out, "ld_gemv_wide: null pointer");
  LD_REQUIRE(B >= 2 && B % 2 == 0, "ld_gemv_wide: %ld rows are not pairs", (long)B);
  if (B > 32) return ld_set_error(LD_ERR_UNSUPPORTED, "ld_gemv_wide: %ld rows, at most 32 (the columns of one MFMA)", (long)B);
  if (x_f32 || w_f32 || out_f32 || in_act)
    return ld_set_error(LD_ERR_UNSUPPORTED, "ld_gemv_wide: bf16 x, weights and output only, no input activation (x_f32=%d w_f32=%d out_f32=%d in_act=%d)",
                        (int)x_f32, (int)w_f32, (int)out_f32, (int)in_act);
  LD_REQUIRE(N >= 1 && N <= 0x7fffffff - 32 && K >= 8 && K <= 0x7fffffff - WIDE_SLICE, "ld_gemv_wide: N=%ld K=%ld", (long)N, (long)K);
  if (K % 16 != 0) return ld_set_error(LD_ERR_UNSUPPORTED, "ld_gemv_wide: K=%ld is not a multiple of 16 (one MFMA step)", (long)K);
  LD_REQUIRE(ldx % 8 == 0 && ldx >= K && ldo >= N && (!resid || ldr >= N), "ld_gemv_wide: ldx must be a multiple of 8, row strides no shorter than a row");
  LD_REQUIRE((((uintptr_t)x | (uintptr_t)W | (uintptr_t)W2) & 15) == 0 && (!norm_w || ((uintptr_t)norm_w & 15) == 0),
             "ld_gemv_wide: x, W, W2 and norm_w must be 16-byte aligned");
  WideParams p{};
  p.x = (const bf16_t*)x; p.W = (const bf16_t*)W; p.W2 = (const bf16_t*)W2; p.bias = (const bf16_t*)bias;
  p.resid = (const bf16_t*)resid; p.out = (bf16_t*)out;
  p.B = (int)B; p.N = (int)N; p.K = (int)K; p.ldx = ldx; p.ldo = ldo; p.ldr = ldr; p.act = act;
  p.norm_w = norm_w; p.norm_eps = norm_eps;
  hipStream_t st = (hipStream_t)stream;
  return W2 ? launch_wide<true>(p, st) : launch_wide<false>(p, st);
}
