// The small kernels around a decode step of the AR model: token embedding, logits -> probabilities -> draw -> advance.
//
// Replaces GPT.sample's embedding (landiff/llm/models/transformer.py:91-119) and the per-step logits math of Semantic1DLM.sample
// (landiff/llm/models/lm_model.py:417-454).  All per-step scalars (position, token) live in device memory so the whole step is
// graph-capturable.
#include "ld_llm.h"
#include "ld_llm_sample_dev.h"

namespace {

// token embedding rows (fp32 table) -> bf16 features, same token for every batch row
__global__ void ld_embed_kernel(const float* table, const long* token, bf16_t* out, int B, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * D) return;
  const long t = *token;
  out[i] = f2bf(table[t * D + (i % D)]);
}

// the same for P samples decoded side by side: rows (2p, 2p+1) take the embedding of token[p]
__global__ void ld_embed_pairs_kernel(const float* table, const long* token, bf16_t* out, int B, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * D) return;
  const long t = token[(i / D) >> 1];
  out[i] = f2bf(table[t * D + (i % D)]);
}

// logits [2][V] (cond, uncond) or [1][V] -> probs [V]: the distribution of ld_llm_sample_dev.h.  Single block; V <= LD_SAMPLE_MAXV.
// SAMPLE: the rest of the step in the same launch -- the draw that torch.multinomial makes for one sample,
// argmax_i(probs[i] / q[i]) with q ~ Exp(1) from the caller's generator (`noise`; ATen's multinomial is exactly
// empty_like(p).exponential_(1, gen), div, argmax: ties -> lowest index), the forced-token schedule / token record /
// position advance of ld_decode_advance_kernel, and the embedding rows of the token the next step starts from.
struct SampleArgs {
  const float* noise;      // [V] Exp(1) draws
  const int* forced; int* pos; long* token; long* out_tokens; int* out_count; long* sampled;
  const float* emb; bf16_t* x; int B, D;
  long out_stride;         // ld_llm_sample_advance_pairs: out_tokens row stride of workgroup (= sample) blockIdx.x
};
template <bool SAMPLE>
__global__ __launch_bounds__(1024) void ld_logits_to_probs_kernel(const float* logits, float* probs, float* cfg_logits,
                                                                  int V, int guided, float scale, float temperature,
                                                                  const int* pos_ptr, const int* allowed, int n_allowed_stride,
                                                                  int top_k, float top_p, SampleArgs sa) {
  __shared__ float red[32];
  __shared__ int redi[32];
  __shared__ float sv[LD_SAMPLE_MAXV];     // value per vocabulary id
  __shared__ float ss[LD_SAMPLE_MAXV];     // values in descending order (top-p)
  __shared__ float thr_s;
  const int tid = threadIdx.x, nt = blockDim.x;
  if constexpr (SAMPLE) {
    // ld_llm_sample_advance_pairs: workgroup p is sample p -- logits rows (2p, 2p+1), its own noise / probs row, position word,
    // token, out_tokens row, out_count, sampled slot and x rows (2p, 2p+1); forced / allowed are the shared schedule.  Every
    // workgroup reads and advances only ITS position word (all hold the same value), so no workgroup's ++ races another's read.
    if (const long wg = blockIdx.x) {
      logits += wg * 2 * V; pos_ptr += wg;
      if (probs) probs += wg * V;
      if (cfg_logits) cfg_logits += wg * V;
      sa.noise += wg * V; sa.pos += wg; sa.token += wg; sa.out_tokens += wg * sa.out_stride; sa.out_count += wg;
      if (sa.sampled) sa.sampled += wg;
      sa.x += wg * sa.B * sa.D;
    }
  }
  const int nal = dist_fill(sv, logits, logits + V, guided, scale, temperature, cfg_logits,
                            allowed ? allowed + (long)(*pos_ptr + 1) * n_allowed_stride : nullptr,   // row of the position being generated
                            V, tid, nt);
  dist_top_k(sv, &thr_s, top_k, nal, V, tid, nt);
  const float m2 = dist_max(sv, red, V, tid, nt);
  dist_divide(sv, dist_exp_sum(sv, red, m2, V, tid, nt), V, tid, nt);
  if (dist_top_p_applies(top_p, nal))
    dist_divide(sv, dist_top_p(sv, ss, red, top_p, V, tid, nt, [&](int i) { sv[i] = 0.f; }), V, tid, nt);
  for (int i = tid; i < V; i += nt) if (probs) probs[i] = sv[i];
  if constexpr (SAMPLE) {
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int i = tid; i < V; i += nt) {
      const float r = sv[i] / sa.noise[i];                   // IEEE division, as at::div
      if (r > best || (r == best && i < bi) || bi == 0x7fffffff) { best = r; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    __syncthreads();
    if ((tid & 63) == 0) { red[tid >> 6] = best; redi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < (nt >> 6); ++w)
        if (red[w] > best || (red[w] == best && redi[w] < bi)) { best = red[w]; bi = redi[w]; }
      // ld_decode_advance_kernel: the token generated now sits at position pos + 1
      const int pos = *sa.pos;
      const int f = sa.forced[pos + 1];
      long t = bi;
      if (sa.sampled) *sa.sampled = t;
      if (f >= 0) t = f;
      else { sa.out_tokens[*sa.out_count] = t; *sa.out_count = *sa.out_count + 1; }
      *sa.token = t;
      *sa.pos = pos + 1;
      redi[0] = (int)t;
    }
    __syncthreads();
    const long t = redi[0];
    for (int i = tid; i < sa.B * sa.D; i += nt) sa.x[i] = f2bf(sa.emb[t * sa.D + (i % sa.D)]);      // ld_embed_kernel
  }
}

// after torch.multinomial: apply the forced-token schedule, record the sampled token, advance position
__global__ void ld_decode_advance_kernel(const long* sampled, const int* forced, int* pos_ptr, long* token,
                                         long* out_tokens, int* out_count) {
  const int pos = *pos_ptr;
  const int f = forced[pos + 1];   // token generated now sits at position pos + 1
  long t = *sampled;
  if (f >= 0) t = f;
  else { out_tokens[*out_count] = t; *out_count = *out_count + 1; }
  *token = t;
  *pos_ptr = pos + 1;
}

}  // namespace

int ld_embed_launch(const char* what, bool pairs, const float* table, const int64_t* token, void* out, int64_t B, int64_t D,
                    void* stream) {
  hipLaunchKernelGGL(pairs ? ld_embed_pairs_kernel : ld_embed_kernel, dim3((B * D + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     table, (const long*)token, (bf16_t*)out, (int)B, (int)D);
  return ld_check_launch(what);
}

LD_API int ld_llm_embed(const float* table, const int64_t* token, void* out, int64_t B, int64_t D, void* stream) {
  LD_REQUIRE(table && token && out, "ld_llm_embed: null pointer");
  return ld_embed_launch("ld_llm_embed", false, table, token, out, B, D, stream);
}

LD_API int ld_llm_logits_to_probs(const float* logits, float* probs, float* cfg_logits, int64_t V, int32_t guided,
                                  float scale, float temperature, const int32_t* pos, const int32_t* allowed,
                                  int64_t allowed_stride, int32_t top_k, float top_p, void* stream) {
  LD_REQUIRE(logits && probs && V > 0 && V <= LD_SAMPLE_MAXV, "ld_llm_logits_to_probs: bad args (V=%ld, max %d)", (long)V, LD_SAMPLE_MAXV);
  LD_REQUIRE(!allowed || pos, "ld_llm_logits_to_probs: allowed table needs pos");
  hipLaunchKernelGGL(ld_logits_to_probs_kernel<false>, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits, probs, cfg_logits,
                     (int)V, guided, scale, temperature, (const int*)pos, (const int*)allowed, (int)allowed_stride,
                     (int)top_k, top_p, SampleArgs{});
  return ld_check_launch("ld_llm_logits_to_probs");
}

// One launch of P workgroups: workgroup p works on logits rows (2p, 2p+1), noise / probs / cfg_logits row p, pos[p], token[p],
// out_tokens[p][..], out_count[p], sampled[p] and rows_per_wg rows of x.  cap = 0: the one-sample form (no P / out_stride checks).
static int sample_advance(const char* name, int cap, int64_t P, int64_t rows_per_wg, int64_t out_stride, const float* logits,
                          float* probs, float* cfg_logits, int64_t V, int32_t guided, float scale, float temperature, int32_t* pos,
                          const int32_t* allowed, int64_t allowed_stride, int32_t top_k, float top_p, const float* noise,
                          const int32_t* forced, int64_t* token, int64_t* out_tokens, int32_t* out_count, int64_t* sampled,
                          const float* emb_table, void* x, int64_t D, void* stream) {
  LD_REQUIRE(logits && V > 0 && V <= LD_SAMPLE_MAXV, "%s: bad args (V=%ld, max %d)", name, (long)V, LD_SAMPLE_MAXV);
  LD_REQUIRE(pos && noise && forced && token && out_tokens && out_count && emb_table && x, "%s: null pointer", name);
  if (cap) {
    LD_REQUIRE(P >= 1 && D >= 1 && out_stride >= 0, "%s: P=%ld D=%ld out_stride=%ld", name, (long)P, (long)D, (long)out_stride);
    if (P > cap) return ld_set_error(LD_ERR_UNSUPPORTED, "%s: %ld samples, at most %d", name, (long)P, cap);
  }
  SampleArgs sa{noise, (const int*)forced, (int*)pos, (long*)token, (long*)out_tokens, (int*)out_count, (long*)sampled,
                emb_table, (bf16_t*)x, (int)rows_per_wg, (int)D, (long)out_stride};
  hipLaunchKernelGGL(ld_logits_to_probs_kernel<true>, dim3((unsigned)P), dim3(1024), 0, (hipStream_t)stream, logits, probs, cfg_logits,
                     (int)V, guided, scale, temperature, (const int*)pos, (const int*)allowed, (int)allowed_stride,
                     (int)top_k, top_p, sa);
  return ld_check_launch(name);
}

LD_API int ld_llm_sample_advance(const float* logits, float* probs, float* cfg_logits, int64_t V, int32_t guided, float scale,
                                 float temperature, int32_t* pos, const int32_t* allowed, int64_t allowed_stride,
                                 int32_t top_k, float top_p, const float* noise, const int32_t* forced, int64_t* token,
                                 int64_t* out_tokens, int32_t* out_count, int64_t* sampled, const float* emb_table, void* x,
                                 int64_t B, int64_t D, void* stream) {
  return sample_advance("ld_llm_sample_advance", 0, 1, B, 0, logits, probs, cfg_logits, V, guided, scale, temperature, pos, allowed,
                        allowed_stride, top_k, top_p, noise, forced, token, out_tokens, out_count, sampled, emb_table, x, D, stream);
}

// ld_llm_sample_advance for P samples (lm_model.py:417-508 per sample), x rows (2p, 2p+1) for sample p
LD_API int ld_llm_sample_advance_pairs(const float* logits, float* probs, float* cfg_logits, int64_t V, int32_t guided, float scale,
                                       float temperature, int32_t* pos, const int32_t* allowed, int64_t allowed_stride,
                                       int32_t top_k, float top_p, const float* noise, const int32_t* forced, int64_t* token,
                                       int64_t* out_tokens, int64_t out_stride, int32_t* out_count, int64_t* sampled,
                                       const float* emb_table, void* x, int64_t P, int64_t D, void* stream) {
  return sample_advance("ld_llm_sample_advance_pairs", LD_LLM_MAX_PAIRS, P, 2, out_stride, logits, probs, cfg_logits, V, guided, scale,
                        temperature, pos, allowed, allowed_stride, top_k, top_p, noise, forced, token, out_tokens, out_count, sampled,
                        emb_table, x, D, stream);
}

// ld_llm_sample_advance_pairs with the cap of the second engine (LD_LLM_MAX_WIDE samples): the same kernel, P workgroups.
LD_API int ld_llm_sample_advance_wide(const float* logits, float* probs, float* cfg_logits, int64_t V, int32_t guided, float scale,
                                      float temperature, int32_t* pos, const int32_t* allowed, int64_t allowed_stride,
                                      int32_t top_k, float top_p, const float* noise, const int32_t* forced, int64_t* token,
                                      int64_t* out_tokens, int64_t out_stride, int32_t* out_count, int64_t* sampled,
                                      const float* emb_table, void* x, int64_t P, int64_t D, void* stream) {
  return sample_advance("ld_llm_sample_advance_wide", LD_LLM_MAX_WIDE, P, 2, out_stride, logits, probs, cfg_logits, V, guided, scale,
                        temperature, pos, allowed, allowed_stride, top_k, top_p, noise, forced, token, out_tokens, out_count, sampled,
                        emb_table, x, D, stream);
}

LD_API int ld_llm_decode_advance(const int64_t* sampled, const int32_t* forced, int32_t* pos, int64_t* token,
                                 int64_t* out_tokens, int32_t* out_count, void* stream) {
  LD_REQUIRE(sampled && forced && pos && token && out_tokens && out_count, "ld_llm_decode_advance: null pointer");
  hipLaunchKernelGGL(ld_decode_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (const long*)sampled,
                     (const int*)forced, (int*)pos, (long*)token, (long*)out_tokens, (int*)out_count);
  return ld_check_launch("ld_llm_decode_advance");
}
