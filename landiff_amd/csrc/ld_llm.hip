// The AR model's decode step as launches queued from native code (embedding -> all blocks -> final LayerNorm -> fp32 head), and
// the RMSNorm / LayerNorm kernels over short rows.  The kernels of the step live with their families: ld_llm_gemv.hip,
// ld_llm_attn.hip, ld_llm_sample.hip, ld_llm_wide.hip, ld_llm_score.hip.
//
// Replaces: LlamaTransformerBlock / TransformerBlock.local_kvcache_inference
// (landiff/llm/modules/transformer_blocks.py:22-40,67-88,128-236) and GPT.sample (landiff/llm/models/transformer.py:91-119).
#include "ld_llm.h"
#include "../../include/landiff_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------
// RMSNorm / LayerNorm over short rows (fp32 math), one wave per row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ld_rmsnorm_kernel(const bf16_t* x, const float* w, bf16_t* out,
                                                         int rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const bf16_t* xr = x + (long)r * D;
  float ss = 0.f;
  for (int c = lane; c < (D >> 3); c += 64) {
    const u32x4_t a = *(const u32x4_t*)(xr + c * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float lo = bf_lo(a[e]), hi = bf_hi(a[e]); ss += lo * lo + hi * hi; }
  }
  ss = wave_sum(ss);
  const float rs = rsqrtf(ss / (float)D + eps);
  for (int c = lane; c < (D >> 3); c += 64) {
    const u32x4_t a = *(const u32x4_t*)(xr + c * 8);
    const f32x4_t w0 = *(const f32x4_t*)(w + c * 8), w1 = *(const f32x4_t*)(w + c * 8 + 4);
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = bf_lo(a[e]) * rs; v[2 * e + 1] = bf_hi(a[e]) * rs; }
    u32x4_t o;
    o[0] = pack_bf16x2(v[0] * w0[0], v[1] * w0[1]); o[1] = pack_bf16x2(v[2] * w0[2], v[3] * w0[3]);
    o[2] = pack_bf16x2(v[4] * w1[0], v[5] * w1[1]); o[3] = pack_bf16x2(v[6] * w1[2], v[7] * w1[3]);
    *(u32x4_t*)(out + (long)r * D + c * 8) = o;
  }
}

// final LayerNorm of GPT.sample: bf16 rows (row stride ldx) -> fp32, fp32 affine
__global__ __launch_bounds__(256) void ld_ln_f32out_kernel(const bf16_t* x, long ldx, const float* w, const float* b,
                                                           float* out, int rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const bf16_t* xr = x + (long)r * ldx;
  float s = 0.f, ss = 0.f;
  for (int i = lane; i < D; i += 64) { const float v = bf2f(xr[i]); s += v; }
  s = wave_sum(s);
  const float mean = s / (float)D;
  for (int i = lane; i < D; i += 64) { const float d = bf2f(xr[i]) - mean; ss += d * d; }
  ss = wave_sum(ss);
  const float rs = rsqrtf(ss / (float)D + eps);
  for (int i = lane; i < D; i += 64) out[(long)r * D + i] = (bf2f(xr[i]) - mean) * rs * w[i] + b[i];
}

// Same, for rows of at most 4096 elements (D % 8 == 0): the row is read once with 16-byte loads and stays in registers
// for the mean, the centred second moment and the affine output (the three-pass kernel above spent 22 us on the two
// rows of a decode step, all of it dependent 2-byte loads).
__global__ __launch_bounds__(256) void ld_ln_f32out_reg_kernel(const bf16_t* x, long ldx, const float* w, const float* b,
                                                               float* out, int rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const bf16_t* xr = x + (long)r * ldx;
  const int nchunk = D >> 3;
  float v[8][8];
  float s = 0.f, ss = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = lane + 64 * k;
    u32x4_t a = (u32x4_t){0u, 0u, 0u, 0u};
    if (c < nchunk) a = *(const u32x4_t*)(xr + c * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[k][2 * e] = bf_lo(a[e]); v[k][2 * e + 1] = bf_hi(a[e]); s += v[k][2 * e] + v[k][2 * e + 1]; }
  }
  s = wave_sum(s);
  const float mean = s / (float)D;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (lane + 64 * k < nchunk) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[k][e] - mean; ss += d * d; }
    }
  }
  ss = wave_sum(ss);
  const float rs = rsqrtf(ss / (float)D + eps);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = lane + 64 * k;
    if (c < nchunk) {
      const f32x4_t w0 = *(const f32x4_t*)(w + c * 8), w1 = *(const f32x4_t*)(w + c * 8 + 4);
      const f32x4_t b0 = *(const f32x4_t*)(b + c * 8), b1 = *(const f32x4_t*)(b + c * 8 + 4);
      f32x4_t o0, o1;
#pragma unroll
      for (int e = 0; e < 4; ++e) { o0[e] = (v[k][e] - mean) * rs * w0[e] + b0[e]; o1[e] = (v[k][4 + e] - mean) * rs * w1[e] + b1[e]; }
      *(f32x4_t*)(out + (long)r * D + c * 8) = o0;
      *(f32x4_t*)(out + (long)r * D + c * 8 + 4) = o1;
    }
  }
}

}  // namespace

LD_API int ld_rmsnorm_bf16(const void* x, const float* w, void* out, int64_t rows, int64_t D, float eps, void* stream) {
  LD_REQUIRE(x && w && out && D % 8 == 0, "ld_rmsnorm_bf16: bad args");
  hipLaunchKernelGGL(ld_rmsnorm_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, w, (bf16_t*)out, (int)rows, (int)D, eps);
  return ld_check_launch("ld_rmsnorm_bf16");
}

LD_API int ld_layernorm_bf16_to_f32(const void* x, int64_t ldx, const float* w, const float* b, float* out,
                                    int64_t rows, int64_t D, float eps, void* stream) {
  LD_REQUIRE(x && w && b && out, "ld_layernorm_bf16_to_f32: null pointer");
  if (D % 8 == 0 && D <= 4096 && ldx % 8 == 0)
    hipLaunchKernelGGL(ld_ln_f32out_reg_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, (long)ldx, w, b, out, (int)rows, (int)D, eps);
  else
    hipLaunchKernelGGL(ld_ln_f32out_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, (long)ldx, w, b, out, (int)rows, (int)D, eps);
  return ld_check_launch("ld_layernorm_bf16_to_f32");
}

namespace {

typedef int (*GemvFn)(const void*, int64_t, int32_t, const void*, const void*, int32_t, const void*, const void*, int64_t, void*, int64_t,
                      int32_t, int64_t, int64_t, int64_t, int32_t, int32_t, const float*, float, void*);

// what tells the three forms of the decode step apart
struct StepEngine {
  const char* name;        // the entry point, for error texts
  GemvFn gemv;             // the Linear layers of the blocks
  GemvFn head;             // the fp32 head; null: ld_llm_head_f32
  int max_samples;         // 0: B = 1..MAXB rows of one sample; else B = 2 P rows, P <= max_samples (cond, uncond) pairs with token[P]
  int mlp_multiple;        // mlp must be a multiple of it ...
  int mlp_error;           // ... or this is returned
};

// One decode step: embedding -> 5 launches per block -> final LayerNorm -> fp32 head.  Everything is validated before the first launch.
// emb_table == null: x already holds the embedding rows.  pos_value >= 0 (the position is known on the host) goes to the attention
// launcher, which then leaves the splits this step does not use unlaunched.
int decode_step(const StepEngine& e, const ld_llm_layer* layers, int64_t n_layers, const float* emb_table, const int64_t* token,
                const int32_t* pos, int32_t pos_value, void* x, void* qkv, void* att, void* gate, float* attn_ws, const float* cos_t,
                const float* sin_t, const float* lnf_w, const float* lnf_b, float* lnf_out, const float* head_w, float* logits,
                int64_t B, int64_t hidden, int64_t heads, int64_t mlp, int64_t vocab, int64_t Lmax, int64_t nsplit, float rms_eps,
                float ln_eps, void* stream) {
  LD_REQUIRE(layers && n_layers > 0 && (emb_table == nullptr || token) && pos && x && qkv && att && gate && attn_ws && cos_t && sin_t &&
             lnf_w && lnf_b && lnf_out && head_w && logits, "%s: null pointer", e.name);
  if (e.max_samples) {
    LD_REQUIRE(B >= 2 && B % 2 == 0, "%s: %ld rows are not (cond, uncond) pairs", e.name, (long)B);
    if (B > 2 * e.max_samples)
      return ld_set_error(LD_ERR_UNSUPPORTED, "%s: %ld samples, at most %d", e.name, (long)(B / 2), e.max_samples);
  } else {
    LD_REQUIRE(B >= 1 && B <= MAXB, "%s: batch %ld not in [1,%d]", e.name, (long)B, MAXB);
  }
  LD_REQUIRE(hidden == heads * 128, "%s: head_dim must be 128 (hidden=%ld heads=%ld)", e.name, (long)hidden, (long)heads);
  LD_REQUIRE(mlp >= e.mlp_multiple && vocab >= 1, "%s: mlp=%ld vocab=%ld", e.name, (long)mlp, (long)vocab);
  if (mlp % e.mlp_multiple != 0) return ld_set_error(e.mlp_error, "%s: mlp=%ld is not a multiple of %d", e.name, (long)mlp, e.mlp_multiple);
  LD_REQUIRE(nsplit > 1 && (Lmax + nsplit - 1) / nsplit <= 16 * KV_MAXIT,
             "%s: the decode path is the key-split attention (nsplit > 1, <= 256 keys per split)", e.name);
  LD_REQUIRE(pos_value < Lmax, "%s: pos_value %d outside [0, Lmax)", e.name, (int)pos_value);
  for (int64_t i = 0; i < n_layers; ++i) {
    const ld_llm_layer& w = layers[i];
    LD_REQUIRE(w.wqkv && w.wo && w.w1 && w.w3 && w.w2 && w.n0 && w.n1 && w.k_cache && w.v_cache,
               "%s: layer %ld has a null pointer", e.name, (long)i);
  }
  int rc = emb_table ? ld_embed_launch(e.name, e.max_samples != 0, emb_table, token, x, B, hidden, stream) : 0;
  for (int64_t i = 0; i < n_layers && rc == 0; ++i) {
    const ld_llm_layer& w = layers[i];
    rc = e.gemv(x, hidden, 0, w.wqkv, nullptr, 0, nullptr, nullptr, 0, qkv, 3 * hidden, 0, B, 3 * hidden, hidden, 0, 0, w.n0, rms_eps, stream);
    if (rc) break;
    rc = ld_kv_attn_launch(nullptr, w.k_cache, w.v_cache, pos, pos_value, att, B, 1, heads, Lmax, attn_ws, nsplit, qkv, cos_t, sin_t, stream);
    if (rc) break;
    rc = e.gemv(att, hidden, 0, w.wo, nullptr, 0, nullptr, x, hidden, x, hidden, 0, B, hidden, hidden, 0, 0, nullptr, 0.f, stream);
    if (rc) break;
    rc = e.gemv(x, hidden, 0, w.w1, w.w3, 0, nullptr, nullptr, 0, gate, mlp, 0, B, mlp, hidden, 0, LD_ACT_GELU_TANH, w.n1, rms_eps, stream);
    if (rc) break;
    rc = e.gemv(gate, mlp, 0, w.w2, nullptr, 0, nullptr, x, hidden, x, hidden, 0, B, hidden, mlp, 0, 0, nullptr, 0.f, stream);
  }
  if (rc) return rc;
  rc = ld_layernorm_bf16_to_f32(x, hidden, lnf_w, lnf_b, lnf_out, B, hidden, ln_eps, stream);
  if (rc) return rc;
  if (!e.head) return ld_llm_head_f32(lnf_out, hidden, head_w, hidden, logits, vocab, B, vocab, hidden, stream);
  return e.head(lnf_out, hidden, 1, head_w, nullptr, 1, nullptr, nullptr, 0, logits, vocab, 1, B, vocab, hidden, 0, 0, nullptr, 0.f, stream);
}

}  // namespace

LD_API int ld_llm_decode_forward(const ld_llm_layer* layers, int64_t n_layers, const float* emb_table, const int64_t* token,
                                 const int32_t* pos, int32_t pos_value, void* x, void* qkv, void* att, void* gate, float* attn_ws,
                                 const float* cos_t, const float* sin_t, const float* lnf_w, const float* lnf_b,
                                 float* lnf_out, const float* head_w, float* logits, int64_t B, int64_t hidden,
                                 int64_t heads, int64_t mlp, int64_t vocab, int64_t Lmax, int64_t nsplit, float rms_eps,
                                 float ln_eps, void* stream) {
  static const StepEngine eng{"ld_llm_decode_forward", ld_gemv, ld_gemv, 0, 8, LD_ERR_INVALID};
  return decode_step(eng, layers, n_layers, emb_table, token, pos, pos_value, x, qkv, att, gate, attn_ws, cos_t, sin_t, lnf_w, lnf_b,
                     lnf_out, head_w, logits, B, hidden, heads, mlp, vocab, Lmax, nsplit, rms_eps, ln_eps, stream);
}

// P = B / 2 samples of one prompt (lm_model.py:417-508 once per sample): ld_gemv_pairs streams every weight matrix once for all pairs,
// the attention is a grid over (B * heads, split) at the one shared position.  Pair p gets the bits of a B = 2 ld_llm_decode_forward.
LD_API int ld_llm_decode_forward_pairs(const ld_llm_layer* layers, int64_t n_layers, const float* emb_table, const int64_t* token,
                                       const int32_t* pos, int32_t pos_value, void* x, void* qkv, void* att, void* gate, float* attn_ws,
                                       const float* cos_t, const float* sin_t, const float* lnf_w, const float* lnf_b,
                                       float* lnf_out, const float* head_w, float* logits, int64_t B, int64_t hidden,
                                       int64_t heads, int64_t mlp, int64_t vocab, int64_t Lmax, int64_t nsplit, float rms_eps,
                                       float ln_eps, void* stream) {
  static const StepEngine eng{"ld_llm_decode_forward_pairs", ld_gemv_pairs, ld_gemv_pairs, LD_LLM_MAX_PAIRS, 8, LD_ERR_INVALID};
  return decode_step(eng, layers, n_layers, emb_table, token, pos, pos_value, x, qkv, att, gate, attn_ws, cos_t, sin_t, lnf_w, lnf_b,
                     lnf_out, head_w, logits, B, hidden, heads, mlp, vocab, Lmax, nsplit, rms_eps, ln_eps, stream);
}

// The _pairs form on the second engine: ld_gemv_wide (ld_llm_wide.hip: the 2P rows are the columns of an MFMA) and ld_llm_head_f32 (a
// sequential fp32 dot per element, whatever M is).  What pair p gets depends on its own rows alone: not on P, not on the pair's index.
LD_API int ld_llm_decode_forward_wide(const ld_llm_layer* layers, int64_t n_layers, const float* emb_table, const int64_t* token,
                                      const int32_t* pos, int32_t pos_value, void* x, void* qkv, void* att, void* gate, float* attn_ws,
                                      const float* cos_t, const float* sin_t, const float* lnf_w, const float* lnf_b,
                                      float* lnf_out, const float* head_w, float* logits, int64_t B, int64_t hidden,
                                      int64_t heads, int64_t mlp, int64_t vocab, int64_t Lmax, int64_t nsplit, float rms_eps,
                                      float ln_eps, void* stream) {
  static const StepEngine eng{"ld_llm_decode_forward_wide", ld_gemv_wide, nullptr, LD_LLM_MAX_WIDE, 16, LD_ERR_UNSUPPORTED};
  return decode_step(eng, layers, n_layers, emb_table, token, pos, pos_value, x, qkv, att, gate, attn_ws, cos_t, sin_t, lnf_w, lnf_b,
                     lnf_out, head_w, logits, B, hidden, heads, mlp, vocab, Lmax, nsplit, rms_eps, ln_eps, stream);
}

#ifdef LD_VARIANTS   // the dependent-launch form of a decode step: measured slower, only in the variants build
LD_API int ld_llm_decode_blocks_chained(const ld_llm_layer* layers, int64_t n_layers, int32_t pos_value, void* x, void* qkv, void* att,
                                        void* gate, float* attn_ws, const float* cos_t, const float* sin_t, int64_t B, int64_t hidden,
                                        int64_t heads, int64_t mlp, int64_t Lmax, int64_t nsplit, float rms_eps, uint32_t* ctl,
                                        uint32_t epoch, void* stream0, void* stream1) {
  LD_REQUIRE(layers && n_layers > 0 && x && qkv && att && gate && attn_ws && cos_t && sin_t && ctl, "ld_llm_decode_blocks_chained: null pointer");
  LD_REQUIRE(pos_value >= 0 && pos_value < Lmax, "ld_llm_decode_blocks_chained: position %d outside [0, Lmax)", (int)pos_value);
  LD_REQUIRE(stream0 != stream1, "ld_llm_decode_blocks_chained: needs two different streams");
  if (B != 2 || hidden != heads * 128 || hidden % 8 || hidden > 4096 || mlp % 8 || mlp > 12288 || nsplit < 2 ||
      (Lmax + nsplit - 1) / nsplit > 16 * KV_MAXIT || 5 * n_layers > LD_LLM_CHAIN_MAX_OPS)
    return ld_set_error(LD_ERR_UNSUPPORTED, "ld_llm_decode_blocks_chained: B=%ld hidden=%ld heads=%ld mlp=%ld Lmax=%ld nsplit=%ld layers=%ld "
                        "outside the chained form", (long)B, (long)hidden, (long)heads, (long)mlp, (long)Lmax, (long)nsplit, (long)n_layers);
  hipStream_t st[2] = {(hipStream_t)stream0, (hipStream_t)stream1};
  int slot = 0, prev_grid = 0, rc = 0;
  auto sync = [&]() { return ChainSync{(unsigned*)ctl, slot, prev_grid, epoch + 1u}; };
  auto gemv = [&](const void* xin, int64_t ldx, const void* W, const void* W2, const void* resid, void* out, int64_t ldo, int64_t N, int64_t K,
                  int act, const float* norm_w) {
    int grid = 0;
    const int r = ld_gemv_chain_launch(xin, ldx, W, W2, resid, out, ldo, N, K, act, norm_w, rms_eps, sync(), st[slot & 1], &grid);
    prev_grid = grid; ++slot;
    return r;
  };
  for (int64_t i = 0; i < n_layers && rc == 0; ++i) {
    const ld_llm_layer& w = layers[i];
    LD_REQUIRE(w.wqkv && w.wo && w.w1 && w.w3 && w.w2 && w.n0 && w.n1 && w.k_cache && w.v_cache,
               "ld_llm_decode_blocks_chained: layer %ld has a null pointer", (long)i);
    rc = gemv(x, hidden, w.wqkv, nullptr, nullptr, qkv, 3 * hidden, 3 * hidden, hidden, 0, w.n0);
    if (rc) break;
    rc = ld_kv_attn_chain_launch(qkv, cos_t, sin_t, w.k_cache, w.v_cache, pos_value, attn_ws, att, B, heads, Lmax, nsplit, sync(), st[slot & 1]);
    if (rc) break;
    prev_grid = (int)(B * heads * nsplit); ++slot;
    rc = gemv(att, hidden, w.wo, nullptr, x, x, hidden, hidden, hidden, 0, nullptr);
    if (rc) break;
    rc = gemv(x, hidden, w.w1, w.w3, nullptr, gate, mlp, mlp, hidden, LD_ACT_GELU_TANH, w.n1);
    if (rc) break;
    rc = gemv(gate, mlp, w.w2, nullptr, x, x, hidden, hidden, mlp, 0, nullptr);
  }
  return rc;
}
#endif  // LD_VARIANTS
