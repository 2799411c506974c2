// Host-side declarations that cross the files of the ld_llm family (ld_llm_gemv.hip, ld_llm_attn.hip, ld_llm_sample.hip and the
// decode-step drivers of ld_llm.hip).  Internal: none of these is exported.  Device-side helpers are in ld_llm_dev.h.
#pragma once
#include "ld_common.h"
#include "ld_llm_dev.h"

constexpr int MAXB = 4;      // activation rows ld_gemv takes

// ld_llm_attn.hip: ld_llm_kv_attn with the position known on the host (pos_value >= 0: the split launch does not wait for a load
// of *pos, and the splits this step leaves unused are not launched); pos_value < 0: read *pos on the device
int ld_kv_attn_launch(const void* q, const void* k_cache, const void* v_cache, const int32_t* pos, int32_t pos_value, void* out,
                      int64_t B, int64_t m, int64_t H, int64_t Lmax, float* workspace, int64_t nsplit, const void* qkv_fused,
                      const float* cos_t, const float* sin_t, void* stream);

// ld_llm_sample.hip: bf16 embedding rows of *token for all B rows, or (pairs) of token[b / 2] for row b; `what` names the caller
int ld_embed_launch(const char* what, bool pairs, const float* table, const int64_t* token, void* out, int64_t B, int64_t D,
                    void* stream);

#ifdef LD_VARIANTS   // the dependent-launch (ChainSync) forms of ld_llm_decode_blocks_chained, B = 2
// ld_llm_gemv.hip: out = epi(W . norm(x)) in the register GEMV's chained form; *grid_out = workgroups launched
int ld_gemv_chain_launch(const void* x, int64_t ldx, const void* W, const void* W2, const void* resid, void* out, int64_t ldo,
                         int64_t N, int64_t K, int act, const float* norm_w, float norm_eps, ChainSync cs, hipStream_t st,
                         int* grid_out);
// ld_llm_attn.hip: the key-split attention with fused RoPE / append in its chained form, B * H * nsplit workgroups
int ld_kv_attn_chain_launch(const void* qkv, const float* cos_t, const float* sin_t, void* k_cache, void* v_cache, int32_t pos_value,
                            float* workspace, void* out, int64_t B, int64_t H, int64_t Lmax, int64_t nsplit, ChainSync cs,
                            hipStream_t st);
#endif
