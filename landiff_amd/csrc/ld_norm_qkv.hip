// qkv head split with QK-LayerNorm or 3D RoPE and V transposition: an HBM-bound streaming pass.
//
// Replaces: query/key_layernorm (landiff/diffusion/dit_video_concat.py:649-653), sat's
// _transpose_for_scores; MultiheadAttention's head split + apply_rope (landiff/tokenizer/modules/blocks.py:172-180).
//
// Built with -fno-slp-vectorize (build.sh, the ld_norm*.hip case): the RoPE expression below is the one the vectoriser turns into
// v_pk_*_f32 with op_sel operands.
#include "ld_common.h"
#include "../../include/landiff_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------
// qkv [B*N][3*H*64] (thirds q|k|v) -> Q,K [B][H][Npad][64] and V^T [B][H][64][Npad].
// mode 0: per-head LayerNorm(64) on q and k (DiT);  mode 1: interleaved-pair RoPE with a [N][32] table (TiTok);
// mode 2: the plain split (ViT of the Theia extractor: biased q/k/v, no QK-LN, no RoPE).
// One workgroup = 64 tokens x 1 head.
// ---------------------------------------------------------------------------------------------
struct SplitParams {
  const bf16_t* qkv; bf16_t* Q; bf16_t* K; bf16_t* Vt;
  const bf16_t* qw; const bf16_t* qb; const bf16_t* kw; const bf16_t* kb;
  const float* cos_t; const float* sin_t;
  int B, N, H, Npad, mode;
  float eps;
};

__global__ __launch_bounds__(256) void ld_qkv_split_kernel(SplitParams p) {
  __shared__ bf16_t vt[64][72];     // V tile [token][d] (+pad) for the transposed write
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  const long row_stride = 3L * p.H * 64;
  // ---- q and k: 8 lanes per (token, tensor), 8 elements per lane ----
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int task = it * 256 + tid;        // 0..1023 = 64 tokens x 2 tensors x 8 lanes
    const int sub = task & 7;
    const int which = (task >> 3) & 1;      // 0 = q, 1 = k
    const int tok = task >> 4;
    const int n = n0 + tok;
    float v[8];
    const bool valid = n < p.N;
    if (valid) {
      const u32x4_t a = *(const u32x4_t*)(p.qkv + ((long)b * p.N + n) * row_stride + (long)which * p.H * 64 + h * 64 + sub * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[2 * e] = bf_lo(a[e]); v[2 * e + 1] = bf_hi(a[e]); }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
    }
    if (p.mode == 0) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[e];
      s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
      const float mean = s * (1.0f / 64.0f);
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[e] - mean; ss += d * d; }
      ss += __shfl_xor(ss, 1, 64); ss += __shfl_xor(ss, 2, 64); ss += __shfl_xor(ss, 4, 64);
      const float rstd = rsqrtf(ss * (1.0f / 64.0f) + p.eps);
      const bf16_t* w = which ? p.kw : p.qw;
      const bf16_t* bb = which ? p.kb : p.qb;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (v[e] - mean) * rstd * bf2f(w[sub * 8 + e]) + bf2f(bb[sub * 8 + e]);
    } else if (p.mode == 1 && valid) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float c = p.cos_t[(long)n * 32 + sub * 4 + e], s = p.sin_t[(long)n * 32 + sub * 4 + e];
        const float a0 = v[2 * e], a1 = v[2 * e + 1];
        v[2 * e] = a0 * c - a1 * s;
        v[2 * e + 1] = a0 * s + a1 * c;
      }
    }
    if (!valid) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;     // zero rows in the padding region
    }
    bf16_t* dst = (which ? p.K : p.Q) + (((long)b * p.H + h) * p.Npad + n) * 64 + sub * 8;
    u32x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
    if (n < p.Npad) *(u32x4_t*)dst = o;
  }
  // ---- v: stage [64 tokens][64 d] in LDS, write transposed rows [d][64 tokens] ----
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int task = it * 256 + tid;        // 512 = 64 tokens x 8 chunks
    const int sub = task & 7, tok = task >> 3;
    const int n = n0 + tok;
    u32x4_t a = {0u, 0u, 0u, 0u};
    if (n < p.N) a = *(const u32x4_t*)(p.qkv + ((long)b * p.N + n) * row_stride + 2L * p.H * 64 + h * 64 + sub * 8);
    *(u32x4_t*)(&vt[tok][sub * 8]) = a;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int task = it * 256 + tid;        // 512 = 64 d x 8 token-chunks
    const int tc = task & 7, d = task >> 3;
    bf16_t tmp[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) tmp[e] = vt[tc * 8 + e][d];
    u32x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (uint32_t)tmp[2 * e] | ((uint32_t)tmp[2 * e + 1] << 16);
    if (n0 + tc * 8 < p.Npad)
      *(u32x4_t*)(p.Vt + (((long)b * p.H + h) * 64 + d) * p.Npad + n0 + tc * 8) = o;
  }
}

}  // namespace

LD_API int ld_qkv_split(const void* qkv, void* Q, void* K, void* Vt, int64_t B, int64_t N, int64_t H, int64_t Npad,
                        int32_t mode, const void* q_w, const void* q_b, const void* k_w, const void* k_b, float eps,
                        const float* cos_t, const float* sin_t, void* stream) {
  LD_REQUIRE(qkv && Q && K && Vt, "ld_qkv_split: null pointer");
  LD_REQUIRE(Npad % 64 == 0 && Npad >= N, "ld_qkv_split: Npad must be a multiple of 64 and >= N");
  LD_REQUIRE(mode >= 0 && mode <= 2, "ld_qkv_split: mode must be 0, 1 or 2");
  LD_REQUIRE(mode == 0 ? (q_w && q_b && k_w && k_b) : mode == 1 ? (cos_t && sin_t) : true,
             "ld_qkv_split: missing LN weights / RoPE table");
  SplitParams p{};
  p.qkv = (const bf16_t*)qkv; p.Q = (bf16_t*)Q; p.K = (bf16_t*)K; p.Vt = (bf16_t*)Vt;
  p.qw = (const bf16_t*)q_w; p.qb = (const bf16_t*)q_b; p.kw = (const bf16_t*)k_w; p.kb = (const bf16_t*)k_b;
  p.cos_t = cos_t; p.sin_t = sin_t; p.B = (int)B; p.N = (int)N; p.H = (int)H; p.Npad = (int)Npad; p.mode = mode; p.eps = eps;
  dim3 grid((unsigned)(Npad / 64), (unsigned)H, (unsigned)B), block(256);
  hipLaunchKernelGGL(ld_qkv_split_kernel, grid, block, 0, (hipStream_t)stream, p);
  return ld_check_launch("ld_qkv_split");
}
