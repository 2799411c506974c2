// Theia feature extractor (DeiT backbone, a Hugging Face ViTModel): the kernels that are not the transformer's shared building
// blocks.  The q/k/v, output and MLP linears are ld_gemm_bf16, the per-layer LayerNorms ld_layernorm, the head split
// ld_qkv_split mode 2 and the attention ld_attn_fwd_bf16 (landiff_amd/theia.py).
//   ld_vit_patch_rows  uint8 frames -> (x - 127.5) / 127.5 -> bf16 im2col rows of the 16x16/16 patch Conv2d
//   ld_vit_embed       bf16 patch embeddings + CLS + interpolated position table -> the fp32 residual stream
//   ld_vit_tail        final LayerNorm -> drop CLS -> TheiaExtractor's crop / zero pad -> fp32 [T][C][gh][gw] and bf16 rows
#include "ld_common.h"
#include "../../include/landiff_hip.h"

namespace {

inline dim3 grid_for(long total, int block = 256) {
  long b = (total + block - 1) / block;
  return dim3((unsigned)(b < 16384 ? (b > 0 ? b : 1) : 16384));
}

// out [T*P][768] bf16, P = (S/16)^2 (floor: the stride-16 Conv2d drops a remainder), column (c, kh, kw) = c*256 + kh*16 + kw
// (the Conv2d weight's order).  One thread per 8 columns (kw 0-7 or 8-15 of one (c, kh)).  nhwc: frames [T][H][W][3] with H, W <= S, read as if padded right and bottom
// with 127 to S x S; else frames [T][3][S][S].
__global__ void ld_vit_patch_rows_kernel(const uint8_t* in, int nhwc, bf16_t* out, int T, int H, int W, int S) {
  const int g = S / 16;
  const long P = (long)g * g;
  const long total = (long)T * P * 96;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int k = (int)(i % 96);
    const long row = i / 96;
    const int t = (int)(row / P);
    const int p = (int)(row % P);
    const int c = k >> 5, kh = (k >> 1) & 15, kw0 = (k & 1) * 8;
    const int y = (p / g) * 16 + kh, x0 = (p % g) * 16 + kw0;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int x = x0 + e;
      int u = 127;
      if (nhwc) {
        if (y < H && x < W) u = in[(((long)t * H + y) * W + x) * 3 + c];
      } else {
        u = in[(((long)t * 3 + c) * S + y) * S + x];
      }
      v[e] = ((float)u - 127.5f) / 127.5f;
    }
    u32x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
    *(u32x4_t*)(out + i * 8) = o;
  }
}

// x [T][1+P][C] f32: row 0 of every frame = pos[0] (the CLS token already added to it), row 1+p = float(patch[t*P+p]) + pos[1+p].
// One thread per 4 channels.
__global__ void ld_vit_embed_kernel(const bf16_t* patch, const float* pos, float* x, int T, int P, int C) {
  const int cq = C >> 2;
  const long N = (long)P + 1;
  const long total = (long)T * N * cq;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % cq) * 4;
    const long r = i / cq;
    const int n = (int)(r % N);
    const int t = (int)(r / N);
    f32x4_t o = *(const f32x4_t*)(pos + (long)n * C + c);
    if (n > 0) {
      const u32x2_t a = *(const u32x2_t*)(patch + ((long)t * P + n - 1) * C + c);
      o[0] = bf_lo(a[0]) + o[0]; o[1] = bf_hi(a[0]) + o[1];
      o[2] = bf_lo(a[1]) + o[2]; o[3] = bf_hi(a[1]) + o[3];
    }
    *(f32x4_t*)(x + r * C + c) = o;
  }
}

constexpr int TAIL_TOK = 32;      // output positions per workgroup (one frame)
constexpr int TAIL_CH = 256;      // channels per LDS pass

// Output position p = (i, j) of the (gh, gw) grid reads token 1 + i*s + j of its frame when i < s and j < s, else it is 0:
// TheiaExtractor's crop, or zero pad then crop, of the square s x s token grid.  y = LayerNorm(x) with fp32 weights (the
// reference's final layernorm runs in fp32 under autocast); feat [T][C][gh*gw] f32 <- y, cl [T*gh*gw][C] bf16 <-
// bf16((y - mean[c]) / (std[c] + 1e-8)), the arithmetic of ld_feature_norm_cl on feat.
__global__ __launch_bounds__(256) void ld_vit_tail_kernel(const float* x, const float* lw, const float* lb, float eps, int N, int s,
                                                         int gh, int gw, int C, float* feat, bf16_t* cl, const float* mean,
                                                         const float* stdv) {
  __shared__ float tile[TAIL_TOK][TAIL_CH + 1];
  __shared__ float st_mean[TAIL_TOK], st_rstd[TAIL_TOK];
  __shared__ long st_src[TAIL_TOK];
  const int t = blockIdx.y, p0 = blockIdx.x * TAIL_TOK;
  const int PP = gh * gw;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int k = 0; k < TAIL_TOK / 4; ++k) {
    const int tok = wv * (TAIL_TOK / 4) + k;
    const int p = p0 + tok;
    const int i = p / gw, j = p % gw;
    const bool valid = p < PP && i < s && j < s;
    float m = 0.f, r = 0.f;
    long src = -1;
    if (valid) {
      src = (long)t * N + 1 + (long)i * s + j;
      const float* xr = x + src * C;
      float sum = 0.f;
      for (int c = lane; c < C; c += 64) sum += xr[c];
      m = wave_sum(sum) / (float)C;
      float ss = 0.f;
      for (int c = lane; c < C; c += 64) { const float d = xr[c] - m; ss += d * d; }
      r = rsqrtf(wave_sum(ss) / (float)C + eps);
    }
    if (lane == 0) { st_mean[tok] = m; st_rstd[tok] = r; st_src[tok] = src; }
  }
  __syncthreads();
  for (int c0 = 0; c0 < C; c0 += TAIL_CH) {
    const int c = c0 + tid;
    if (c < C) {
      const float w = lw[c], b = lb[c];
      float mc = 0.f, sc = 1.f;
      if (cl) { mc = mean[c]; sc = stdv[c] + 1e-8f; }
      for (int tok = 0; tok < TAIL_TOK; ++tok) {
        const int p = p0 + tok;
        if (p >= PP) break;
        const long src = st_src[tok];
        const float y = src >= 0 ? (x[src * C + c] - st_mean[tok]) * st_rstd[tok] * w + b : 0.f;
        tile[tok][tid] = y;
        if (cl) cl[((long)t * PP + p) * C + c] = f2bf((y - mc) / sc);
      }
    }
    __syncthreads();
    if (feat) {
      const int tok = tid & (TAIL_TOK - 1), p = p0 + tok;
      for (int k = tid / TAIL_TOK; k < TAIL_CH; k += 256 / TAIL_TOK)
        if (c0 + k < C && p < PP) feat[((long)t * C + c0 + k) * PP + p] = tile[tok][k];
    }
    __syncthreads();
  }
}

}  // namespace

LD_API int ld_vit_patch_rows(const void* frames, int32_t nhwc, void* out, int64_t T, int64_t H, int64_t W, int64_t S, void* stream) {
  LD_REQUIRE(frames && out && T > 0 && S >= 16, "ld_vit_patch_rows: bad args (S >= 16)");
  LD_REQUIRE(nhwc ? (H > 0 && W > 0 && H <= S && W <= S) : (H == S && W == S), "ld_vit_patch_rows: frames must fit the S x S square");
  const long total = T * (S / 16) * (S / 16) * 96;
  hipLaunchKernelGGL(ld_vit_patch_rows_kernel, grid_for(total), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)frames,
                     (int)nhwc, (bf16_t*)out, (int)T, (int)H, (int)W, (int)S);
  return ld_check_launch("ld_vit_patch_rows");
}

LD_API int ld_vit_embed(const void* patch, const float* pos, float* x, int64_t T, int64_t P, int64_t C, void* stream) {
  LD_REQUIRE(patch && pos && x && T > 0 && P > 0 && C > 0 && C % 4 == 0, "ld_vit_embed: bad args (C %% 4 == 0)");
  hipLaunchKernelGGL(ld_vit_embed_kernel, grid_for(T * (P + 1) * (C / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)patch,
                     pos, x, (int)T, (int)P, (int)C);
  return ld_check_launch("ld_vit_embed");
}

LD_API int ld_vit_tail(const float* x, const float* ln_w, const float* ln_b, float eps, int64_t T, int64_t N, int64_t s,
                       int64_t gh, int64_t gw, int64_t C, float* feat, void* cl, const float* mean, const float* stdv,
                       void* stream) {
  LD_REQUIRE(x && ln_w && ln_b && T > 0 && C > 0 && gh > 0 && gw > 0, "ld_vit_tail: bad args");
  LD_REQUIRE(s > 0 && N == 1 + s * s, "ld_vit_tail: N must be 1 + s*s (CLS + the square token grid)");
  LD_REQUIRE(feat || cl, "ld_vit_tail: no output");
  LD_REQUIRE(!cl || (mean && stdv), "ld_vit_tail: the bf16 rows need mean and std");
  dim3 grid((unsigned)((gh * gw + TAIL_TOK - 1) / TAIL_TOK), (unsigned)T);
  hipLaunchKernelGGL(ld_vit_tail_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, ln_w, ln_b, eps, (int)N, (int)s, (int)gh,
                     (int)gw, (int)C, feat, (bf16_t*)cl, mean, stdv);
  return ld_check_launch("ld_vit_tail");
}
