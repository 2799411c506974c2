// KV-cache attention of the AR model, head_dim 128: RoPE + KV append, the prefill kernel and the key-split decode kernel.
//
// Replaces apply_rope (landiff/modules/pos_emb.py:16-46) and the attention of LlamaTransformerBlock.local_kvcache_inference
// (landiff/llm/modules/transformer_blocks.py:128-236).  The position lives in device memory so the whole step is graph-capturable.
#include "ld_llm.h"
#include <stdio.h>
#include <stdlib.h>
#include "../../include/landiff_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------
// RoPE on q,k + KV append.  qkv [B][m][3][H][128] bf16; cache K/V [B][Lmax][H][128];
// position of token j = *pos + j.  q_out [B][m][H][128].
// ---------------------------------------------------------------------------------------------
__global__ void ld_rope_append_kernel(const bf16_t* qkv, const float* cos_t, const float* sin_t, const int* pos_ptr,
                                      bf16_t* q_out, bf16_t* kc, bf16_t* vc, int B, int m, int H, int Lmax) {
  const int D = 128;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (b, j, h, pair)
  const int total = B * m * H * (D / 2);
  if (idx >= total) return;
  const int pr = idx % (D / 2);
  const int h = (idx / (D / 2)) % H;
  const int j = (idx / (D / 2) / H) % m;
  const int b = idx / (D / 2) / H / m;
  const int pos = *pos_ptr + j;
  const float c = cos_t[pos * (D / 2) + pr], s = sin_t[pos * (D / 2) + pr];
  const long base = (((long)(b * m + j) * 3) * H + h) * D + 2 * pr;
  const long hd = (long)H * D;
  const float qa = bf2f(qkv[base]), qb = bf2f(qkv[base + 1]);
  const float ka = bf2f(qkv[base + hd]), kb = bf2f(qkv[base + hd + 1]);
  const long qo = ((long)(b * m + j) * H + h) * D + 2 * pr;
  q_out[qo] = f2bf(qa * c - qb * s);
  q_out[qo + 1] = f2bf(qa * s + qb * c);
  const long co = (((long)b * Lmax + pos) * H + h) * D + 2 * pr;
  kc[co] = f2bf(ka * c - kb * s);
  kc[co + 1] = f2bf(ka * s + kb * c);
  vc[co] = qkv[base + 2 * hd];
  vc[co + 1] = qkv[base + 2 * hd + 1];
}

// ---------------------------------------------------------------------------------------------
// KV attention, head_dim 128: query j (position *pos + j) attends keys [0, *pos + j].
// Mirrors the reference's dtype flow: bf16 scores, bf16 (score / sqrt(d)), fp32 softmax -> bf16 p, bf16 out.
// grid (B*H, m), 256 threads; scores staged in LDS (fp32, up to Lmax entries).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ld_kv_attn_kernel(const bf16_t* q, const bf16_t* kc, const bf16_t* vc,
                                                         const int* pos_ptr, bf16_t* out, int B, int m, int H, int Lmax) {
  extern __shared__ float sc[];       // [Lmax] scores, then [2][128] partial outputs + 8 reduction slots
  const int D = 128;
  const int bh = blockIdx.x, j = blockIdx.y;
  const int b = bh / H, h = bh - b * H;
  const int L = *pos_ptr + j + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16_t* qv = q + ((long)(b * m + j) * H + h) * D;
  // 16 lanes x 8 dims per key, 4 keys per wave iteration
  const int sub = lane & 15, kq = lane >> 4;
  float qreg[8];
  {
    const u32x4_t a = *(const u32x4_t*)(qv + sub * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) { qreg[2 * e] = bf_lo(a[e]); qreg[2 * e + 1] = bf_hi(a[e]); }
  }
  const float inv_sqrt_d = 0.08838834764831845f;   // 1/sqrt(128)
  float lmax = -3.0e38f;
  for (int k0 = wave * 4; k0 < L; k0 += 16) {
    const int key = k0 + kq;
    float d = 0.f;
    if (key < L) {
      const u32x4_t a = *(const u32x4_t*)(kc + (((long)b * Lmax + key) * H + h) * D + sub * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) { d = fmaf(qreg[2 * e], bf_lo(a[e]), d); d = fmaf(qreg[2 * e + 1], bf_hi(a[e]), d); }
    }
    d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64); d += __shfl_xor(d, 8, 64);
    if (key < L) {
      const float s = rbf(rbf(d) * inv_sqrt_d);    // einsum -> bf16, then "/ sqrt(d)" -> bf16
      if (sub == 0) sc[key] = s;
      lmax = fmaxf(lmax, s);
    }
  }
  float* red = sc + Lmax;
  lmax = wave_max(lmax);
  if (lane == 0) red[wave] = lmax;
  __syncthreads();
  const float mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float lsum = 0.f;
  for (int k = tid; k < L; k += 256) { const float e = __expf(sc[k] - mx); sc[k] = e; lsum += e; }
  lsum = wave_sum(lsum);
  __syncthreads();
  if (lane == 0) red[4 + wave] = lsum;
  __syncthreads();
  const float inv = 1.0f / (red[4] + red[5] + red[6] + red[7]);
  // out[d] = sum_k bf16(p_k) * v[k][d]; thread -> (d = tid & 127, key parity = tid >> 7)
  const int d = tid & 127, par = tid >> 7;
  float acc = 0.f;
  for (int k = par; k < L; k += 2) {
    const float pk = rbf(sc[k] * inv);
    acc = fmaf(pk, bf2f(vc[(((long)b * Lmax + k) * H + h) * D + d]), acc);
  }
  float* part = red + 8;
  part[par * 128 + d] = acc;
  __syncthreads();
  if (tid < 128) out[((long)(b * m + j) * H + h) * D + tid] = f2bf(part[tid] + part[128 + tid]);
}

// ---------------------------------------------------------------------------------------------
// Decode-step (m = 1) KV attention split over the key axis ("flash decoding"): grid (B*H, nsplit) so that the
// 2 x 16 (batch, head) pairs still fill 256 CUs.  Each workgroup writes (max, sum, unnormalised out[128]) for its
// key range; ld_kv_attn_combine_kernel merges them.  16 lanes x 8 dims per key, 16 keys per workgroup iteration,
// every K/V row is read once with 16-byte loads.  (p stays fp32 here; the reference rounds the normalised p to
// bf16 before the PV product -- a <= 2^-9 relative, zero-mean difference per term.)
// ---------------------------------------------------------------------------------------------
// If qkv != nullptr the kernel also does apply_rope + the KV append of the current token itself (q is then ignored):
// every workgroup rotates q on the fly; the workgroup whose key range holds position *pos rotates/stores the new k
// and v into the cache before using them.
__device__ __forceinline__ float ld_agent(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The merge of the splits rides in the same launch: every workgroup writes its partial result device-coherently (sc1), drains
// the stores and arrives on the (batch row, head)'s counter; the LAST one to arrive reads all partial results (sc1 loads),
// writes the attention output and leaves the counter at zero for the next launch.  Nobody waits for anybody (no co-residency
// requirement); one launch and one ~5 us dependent kernel per block less than split + combine.
// CHAIN: dependent-launch form (ChainSync): the K / V rows (earlier steps' data) are requested before the wait for the qkv
// operation, the new token's q / k / v come through sc1 loads, the merged output is written sc1, every workgroup arrives at the
// end; pos_value >= 0 replaces the device-side position (no dependence on the previous step's sampling launch).
template <bool CHAIN>
__global__ __launch_bounds__(256, CHAIN ? 2 : 1) void ld_kv_attn_split_kernel(const bf16_t* q, const bf16_t* qkv, const float* cos_t,
                                                               const float* sin_t, bf16_t* kc, bf16_t* vc,
                                                               const int* pos_ptr, int pos_value, float* ws, unsigned* counters,
                                                               bf16_t* out, int B, int H, int Lmax, int nsplit, KvSplitRule rule,
                                                               ChainSync cs) {
  __shared__ float red[8 + 4 * 128];
  __shared__ int is_last;
  const int D = 128;
  const int bh = blockIdx.x, sp = blockIdx.y;
  const int b = bh / H, h = bh - b * H;
  const int L = (pos_value >= 0 ? pos_value : *pos_ptr) + 1;
  const int ns = kv_eff_splits(L, nsplit, rule);       // splits in use at this context length; partial results keep the [bh][nsplit] layout
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (sp >= ns) {                                      // a split this step does not use
    if (CHAIN) { chain_wait(cs, tid); chain_arrive(cs, tid, blockIdx.y * gridDim.x + blockIdx.x); }
    return;
  }
  const int chunk = (L + ns - 1) / ns;
  const int k_begin = sp * chunk, k_end = min(L, k_begin + chunk);
  const int n = max(0, k_end - k_begin);
  const int sub = lane & 15, kq = lane >> 4;
  float* out_ws = ws + ((long)bh * nsplit + sp) * (D + 2);
  bf16_t* direct = (ns == 1 && !CHAIN) ? out + (long)bh * D : nullptr;
  KvRows rows;
  if (CHAIN) {
    if (n > 0) kv_rows_request(rows, kc, vc, (long)b * Lmax + k_begin, H, h, n, wave, kq, sub);
    chain_wait(cs, tid);
  }
  if (n == 0) {
    if (tid < D) st_agent(out_ws + 2 + tid, 0.f);
    if (tid == 0) { st_agent(out_ws, -3.0e38f); st_agent(out_ws + 1, 0.f); }
  } else {
    // Request order = dependency order: the new token's q/k/v + rotation factors first (short, L2), then this wave's K
    // rows AND V rows (4 keys per trip, <= KV_MAXIT trips) all at once -- one exposed HBM latency per launch, and the RoPE
    // arithmetic runs underneath it.  The key being appended this step is taken from qkv directly (its cache slot is
    // written for later steps but not read back here), so the prologue needs no barrier.
    u32x4_t a_q = (u32x4_t){0u, 0u, 0u, 0u}, a_k = a_q, a_v = a_q;
    float cs_[4] = {0.f, 0.f, 0.f, 0.f}, sn[4] = {0.f, 0.f, 0.f, 0.f};
    const int pos = L - 1;
    if (qkv) {
      const bf16_t* src = qkv + ((long)b * 3 * H + h) * D;      // [B][3][H][128]: q at +0, k at +H*D, v at +2*H*D
      if (CHAIN) {
        const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (2 * H + 1) * D * 2, 0x00020000);
        a_q = __builtin_amdgcn_raw_buffer_load_b128(rq, sub * 16, 0, 16);
        a_k = __builtin_amdgcn_raw_buffer_load_b128(rq, (H * D + sub * 8) * 2, 0, 16);
        a_v = __builtin_amdgcn_raw_buffer_load_b128(rq, (2 * H * D + sub * 8) * 2, 0, 16);
      } else {
        a_q = *(const u32x4_t*)(src + sub * 8);
        a_k = *(const u32x4_t*)(src + (long)H * D + sub * 8);
        a_v = *(const u32x4_t*)(src + 2L * H * D + sub * 8);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) { cs_[e] = cos_t[pos * 64 + sub * 4 + e]; sn[e] = sin_t[pos * 64 + sub * 4 + e]; }
    } else {
      a_q = *(const u32x4_t*)(q + ((long)b * H + h) * D + sub * 8);
    }
    if (!CHAIN) kv_rows_request(rows, kc, vc, (long)b * Lmax + k_begin, H, h, n, wave, kq, sub);
    kv_attn_split_core(rows, a_q, a_k, a_v, cs_, sn, qkv != nullptr, kc, vc, (long)b * Lmax + pos, H, h, pos - k_begin, n, true,
                       out_ws, red, red + 8, tid, lane, wave, [](float* p, float v) { st_agent(p, v); }, direct);
  }
  if (direct) return;                                  // one split: the output row is written, nothing to merge, no counter traffic
  // Hand-off in the write-through form (cdna_hip_programming.md section 6 Guideline 16, recipe R1; the second valid form of
  // MI355X_MICROARCH.md "Valid forms besides R1/R2": {sc1 stores and loads both sides}): the partial results were stored sc1
  // (st_agent: they leave this XCD's L2), EVERY storing wave drains vmcnt, the workgroup meets, ONE lane arrives with a relaxed
  // agent-scope add; the last arriver reads the partials with sc1 loads (ld_agent: L1 bypassed), which stand in for the acquire
  // because the producers stored sc1.  This relies on the ISA-level behaviour of sc1 accesses on gfx950 that the guide documents,
  // not on the HIP memory model (a relaxed counter orders nothing there); tests/test_gpu_llm_longctx.py and the bit-identity tests
  // of the decode forms are its check.  A release/acquire pair on the counter instead would put a buffer_wbl2 + buffer_inv
  // (~3.5 us, MI355X_MICROARCH.md) into each of the 24 x 1244 launches of a decode.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this thread's part of the partial result is at the coherence point
  __syncthreads();
  if (tid == 0)
    is_last = __hip_atomic_fetch_add(counters + bh, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(ns - 1);
  __syncthreads();
  if (is_last) {
    if (tid < D) {
      const float r = kv_attn_combine_core(ws + (long)bh * nsplit * (D + 2), ns, tid, [](const float* p) { return ld_agent(p); });
      if (CHAIN) __hip_atomic_store(out + (long)bh * D + tid, f2bf(r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else out[(long)bh * D + tid] = f2bf(r);
    }
    if (tid == 0) __hip_atomic_store(counters + bh, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (CHAIN) chain_arrive(cs, tid, blockIdx.y * gridDim.x + blockIdx.x);
}

}  // namespace

KvSplitRule ld_kv_split_rule() {
  static const KvSplitRule rule = [] {
    KvSplitRule r{KV_SPLIT_T1, KV_SPLIT_T2, KV_SPLIT_T4};
    if (const char* e = getenv("LD_KV_SPLIT_T")) {
      int a = 0, b = 0, c = 0;
      if (sscanf(e, "%d,%d,%d", &a, &b, &c) == 3) r = KvSplitRule{a, b, c};
    }
    return r;
  }();
  return rule;
}

LD_API int ld_llm_rope_append(const void* qkv, const float* cos_t, const float* sin_t, const int32_t* pos,
                              void* q_out, void* k_cache, void* v_cache, int64_t B, int64_t m, int64_t H,
                              int64_t Lmax, void* stream) {
  LD_REQUIRE(qkv && cos_t && sin_t && pos && q_out && k_cache && v_cache, "ld_llm_rope_append: null pointer");
  const long total = B * m * H * 64;
  hipLaunchKernelGGL(ld_rope_append_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)qkv, cos_t, sin_t, (const int*)pos, (bf16_t*)q_out, (bf16_t*)k_cache,
                     (bf16_t*)v_cache, (int)B, (int)m, (int)H, (int)Lmax);
  return ld_check_launch("ld_llm_rope_append");
}

int ld_kv_attn_launch(const void* q, const void* k_cache, const void* v_cache, const int32_t* pos, int32_t pos_value, void* out,
                      int64_t B, int64_t m, int64_t H, int64_t Lmax, float* workspace, int64_t nsplit,
                      const void* qkv_fused, const float* cos_t, const float* sin_t, void* stream) {
  LD_REQUIRE(k_cache && v_cache && pos && out, "ld_llm_kv_attn: null pointer");
  LD_REQUIRE(q || qkv_fused, "ld_llm_kv_attn: need q or qkv_fused");
  hipStream_t st = (hipStream_t)stream;
  if (m == 1 && nsplit > 1) {
    LD_REQUIRE(workspace, "ld_llm_kv_attn: split path needs a workspace of B*H*(nsplit*130 + 1) floats, the last B*H words zero");
    LD_REQUIRE(!qkv_fused || (cos_t && sin_t), "ld_llm_kv_attn: fused RoPE needs the cos/sin tables");
    LD_REQUIRE((Lmax + nsplit - 1) / nsplit <= 16 * KV_MAXIT, "ld_llm_kv_attn: Lmax=%ld needs nsplit >= %ld (<= 256 keys per split)",
               (long)Lmax, (long)((Lmax + 255) / 256));
    // the position is known on the host: do not even launch the splits this step leaves unused
    const int ny = pos_value >= 0 ? kv_eff_splits(pos_value + 1, (int)nsplit, ld_kv_split_rule()) : (int)nsplit;
    hipLaunchKernelGGL(ld_kv_attn_split_kernel<false>, dim3((unsigned)(B * H), (unsigned)ny), dim3(256), 0, st,
                       (const bf16_t*)q, (const bf16_t*)qkv_fused, cos_t, sin_t, (bf16_t*)k_cache, (bf16_t*)v_cache,
                       (const int*)pos, (int)pos_value, workspace, (unsigned*)(workspace + B * H * nsplit * 130), (bf16_t*)out, (int)B,
                       (int)H, (int)Lmax, (int)nsplit, ld_kv_split_rule(), ChainSync{});
    return ld_check_launch("ld_llm_kv_attn(split)");
  }
  LD_REQUIRE(q && !qkv_fused, "ld_llm_kv_attn: the fused RoPE/append form exists only for the decode split path");
  const size_t smem = (size_t)(Lmax + 8 + 256) * sizeof(float);
  LD_REQUIRE(smem <= 160 * 1024, "ld_llm_kv_attn: Lmax=%ld too long for the LDS score buffer", (long)Lmax);
  static thread_local LdSmemCache cache{};
  if (int rc = ld_ensure_dyn_smem((const void*)ld_kv_attn_kernel, smem, &cache)) return rc;
  hipLaunchKernelGGL(ld_kv_attn_kernel, dim3((unsigned)(B * H), (unsigned)m), dim3(256), smem, st,
                     (const bf16_t*)q, (const bf16_t*)k_cache, (const bf16_t*)v_cache, (const int*)pos,
                     (bf16_t*)out, (int)B, (int)m, (int)H, (int)Lmax);
  return ld_check_launch("ld_llm_kv_attn");
}

LD_API int ld_llm_kv_attn(const void* q, const void* k_cache, const void* v_cache, const int32_t* pos, void* out,
                          int64_t B, int64_t m, int64_t H, int64_t Lmax, float* workspace, int64_t nsplit,
                          const void* qkv_fused, const float* cos_t, const float* sin_t, void* stream) {
  return ld_kv_attn_launch(q, k_cache, v_cache, pos, -1, out, B, m, H, Lmax, workspace, nsplit, qkv_fused, cos_t, sin_t, stream);
}

#ifdef LD_VARIANTS
int ld_kv_attn_chain_launch(const void* qkv, const float* cos_t, const float* sin_t, void* k_cache, void* v_cache, int32_t pos_value,
                            float* workspace, void* out, int64_t B, int64_t H, int64_t Lmax, int64_t nsplit, ChainSync cs,
                            hipStream_t st) {
  hipLaunchKernelGGL(ld_kv_attn_split_kernel<true>, dim3((unsigned)(B * H), (unsigned)nsplit), dim3(256), 0, st,
                     (const bf16_t*)nullptr, (const bf16_t*)qkv, cos_t, sin_t, (bf16_t*)k_cache, (bf16_t*)v_cache, (const int*)nullptr,
                     (int)pos_value, workspace, (unsigned*)(workspace + B * H * nsplit * 130), (bf16_t*)out, (int)B, (int)H,
                     (int)Lmax, (int)nsplit, ld_kv_split_rule(), cs);
  return ld_check_launch("ld_llm_kv_attn(chained)");
}
#endif
