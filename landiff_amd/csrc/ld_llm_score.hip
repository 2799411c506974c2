// Scoring of AR token sequences: the log-probability of given tokens under the distribution the sampler draws from
// (ld_llm_token_logprobs), and the all-positions fp32 head of the teacher-forced pass (ld_llm_head_f32).
#include "ld_common.h"
#include "ld_llm_sample_dev.h"

namespace {

struct ScoreArgs {
  const float* cond; long cond_stride;       // conditional logits, row r at cond + r * cond_stride
  const float* uncond; long uncond_stride;   // unconditional logits (read when guided)
  int V, guided; float scale, temperature;
  const int* pos_ptr; long pos_stride; int pos_bias;   // pos_ptr: position of row r = pos_ptr[r * pos_stride] + pos_bias; else pos_bias + r
  const int* allowed; int allowed_stride; const int* forced; int n_pos;    // the schedule tables, n_pos rows each
  int top_k; float top_p;
  const long* target; float* logprob; int* valid;
  float* cfg_out; long cfg_stride;           // optional: the guided logits of the rows that are draws
};

// One workgroup per row.  The distribution is the sampler's (ld_llm_sample_dev.h); only the result is taken in the log domain:
// (l_t - max) - log(sum exp(l - max)) [- log(kept)], which stays finite where the sampler's fp32 probability
// exp(l_t - max) / sum has long underflowed to 0.
__global__ __launch_bounds__(1024) void ld_token_logprobs_kernel(ScoreArgs a) {
  __shared__ float red[32];
  __shared__ float sv[LD_SAMPLE_MAXV];     // filtered logit per vocabulary id, later its probability
  __shared__ float ss[LD_SAMPLE_MAXV];     // probabilities in descending order -> their running sum (top-p)
  __shared__ float thr_s;
  __shared__ int removed_s;
  const int tid = threadIdx.x, nt = blockDim.x, V = a.V;
  const long r = blockIdx.x;
  const int pos = a.pos_ptr ? a.pos_ptr[r * a.pos_stride] + a.pos_bias : a.pos_bias + (int)r;
  const long t = a.target[r];
  const bool in_tables = pos + 1 >= 0 && pos + 1 < a.n_pos;
  if ((a.allowed || a.forced) && !in_tables) {              // a position the schedule does not cover: no table row is read
    if (tid == 0) { a.logprob[r] = __builtin_nanf(""); if (a.valid) a.valid[r] = 0; }
    return;
  }
  if (a.forced && a.forced[pos + 1] >= 0) {                 // the schedule writes this token: not a draw
    if (tid == 0) { a.logprob[r] = 0.f; if (a.valid) a.valid[r] = 0; }
    return;
  }
  if (t < 0 || t >= V) {                                    // not a vocabulary id: outside every support
    if (tid == 0) { a.logprob[r] = -INFINITY; if (a.valid) a.valid[r] = 1; }
    return;
  }
  if (tid == 0) removed_s = 0;                              // (published by the barrier that ends dist_fill)
  const int nal = dist_fill(sv, a.cond + r * a.cond_stride, a.uncond + r * a.uncond_stride, a.guided, a.scale, a.temperature,
                            a.cfg_out ? a.cfg_out + r * a.cfg_stride : nullptr,
                            a.allowed ? a.allowed + (long)(pos + 1) * a.allowed_stride : nullptr, V, tid, nt);
  dist_top_k(sv, &thr_s, a.top_k, nal, V, tid, nt);
  const float m2 = dist_max(sv, red, V, tid, nt);
  const float lt = sv[t] - m2;                                // the target's shifted logit (-inf: removed), before sv is overwritten
  __syncthreads();
  const float tot = dist_exp_sum(sv, red, m2, V, tid, nt);
  float lp = lt - logf(tot);
  if (dist_top_p_applies(a.top_p, nal)) {
    dist_divide(sv, tot, V, tid, nt);
    const float kept = dist_top_p(sv, ss, red, a.top_p, V, tid, nt, [&](int i) { if (i == t) removed_s = 1; });
    lp = removed_s ? -INFINITY : lp - logf(kept);              // (the barriers of the last block sum publish removed_s)
  }
  if (tid == 0) {
    a.logprob[r] = lt == -INFINITY ? -INFINITY : lp;
    if (a.valid) a.valid[r] = 1;
  }
}

// C[M][N] = A[M][K] . W[N][K]^T in fp32 on v_mfma_f32_32x32x2_f32: a 64 x 64 output tile per workgroup of four waves (one 32 x 32
// accumulator each), K in steps of 16 through the LDS.  Every product is rounded once and added in k order (the instruction is an
// fp32 fmaf chain), so an element is a plain sequential fp32 dot product.  Rows / columns past M / N and k past K are loaded as
// zeros and never stored.
#define HEAD_BM 64
#define HEAD_BN 64
#define HEAD_BK 16
#define HEAD_LD (HEAD_BK + 1)     // LDS row stride in words: lanes 0..31 of a fragment read 32 different rows at one k
__global__ __launch_bounds__(256) void ld_head_f32_kernel(const float* A, long lda, const float* W, long ldw, float* C, long ldc,
                                                          int M, int N, int K) {
  __shared__ float As[HEAD_BM * HEAD_LD];
  __shared__ float Ws[HEAD_BN * HEAD_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * HEAD_BM, n0 = blockIdx.x * HEAD_BN;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int lr = tid >> 2, lc = (tid & 3) * 4;              // this thread's row and first k of a staged 64 x 16 tile
  f32x16_t acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const bool a_row = m0 + lr < M, w_row = n0 + lr < N;
  const float* ap = A + (long)(m0 + lr) * lda + lc;
  const float* wp = W + (long)(n0 + lr) * ldw + lc;
  for (int k0 = 0; k0 < K; k0 += HEAD_BK) {
    f32x4_t av = {0.f, 0.f, 0.f, 0.f}, wv = av;
    const bool k_in = k0 + lc < K;                            // K % 4 == 0: a group of four is inside or outside as a whole
    if (a_row && k_in) av = *(const f32x4_t*)(ap + k0);
    if (w_row && k_in) wv = *(const f32x4_t*)(wp + k0);
    __syncthreads();                                          // the previous step's fragments have been read
#pragma unroll
    for (int e = 0; e < 4; ++e) { As[lr * HEAD_LD + lc + e] = av[e]; Ws[lr * HEAD_LD + lc + e] = wv[e]; }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < HEAD_BK; kk += 2) {
      const float fa = As[(wm + (lane & 31)) * HEAD_LD + kk + (lane >> 5)];      // A[i = lane & 31][k = lane >> 5]
      const float fb = Ws[(wn + (lane & 31)) * HEAD_LD + kk + (lane >> 5)];      // B[k = lane >> 5][j = lane & 31] = W[j][k]
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc, 0, 0, 0);
    }
  }
  const int col = n0 + wn + (lane & 31);
  if (col < N) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = m0 + wm + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
      if (row < M) C[(long)row * ldc + col] = acc[e];
    }
  }
}

}  // namespace

LD_API int ld_llm_token_logprobs(const float* cond, int64_t cond_stride, const float* uncond, int64_t uncond_stride, int64_t n,
                                 int64_t V, int32_t guided, float scale, float temperature, const int32_t* pos, int64_t pos_stride,
                                 int32_t pos_bias, const int32_t* allowed, int64_t allowed_stride, const int32_t* forced,
                                 int64_t n_pos, int32_t top_k, float top_p, const int64_t* target, float* logprob, int32_t* valid,
                                 float* cfg_logits, int64_t cfg_stride, void* stream) {
  // sizes first: a refused shape is refused whatever the pointers are
  LD_REQUIRE(V > 0 && V <= LD_SAMPLE_MAXV, "ld_llm_token_logprobs: bad args (V=%ld, max %d)", (long)V, LD_SAMPLE_MAXV);
  LD_REQUIRE(cond && target && logprob, "ld_llm_token_logprobs: null pointer");
  LD_REQUIRE(n >= 1 && n <= 0x7fffffff, "ld_llm_token_logprobs: n=%ld rows", (long)n);
  LD_REQUIRE(!guided || uncond, "ld_llm_token_logprobs: guided needs the unconditional rows");
  LD_REQUIRE(cond_stride >= 0 && uncond_stride >= 0 && pos_stride >= 0, "ld_llm_token_logprobs: negative stride");
  LD_REQUIRE(!(allowed || forced) || n_pos > 0, "ld_llm_token_logprobs: the schedule tables need their row count n_pos");
  LD_REQUIRE(!allowed || allowed_stride >= 1, "ld_llm_token_logprobs: allowed_stride=%ld", (long)allowed_stride);
  LD_REQUIRE(temperature > 0.f, "ld_llm_token_logprobs: temperature must be positive");
  LD_REQUIRE(!cfg_logits || cfg_stride >= V, "ld_llm_token_logprobs: cfg_stride=%ld shorter than a row", (long)cfg_stride);
  ScoreArgs a{cond, (long)cond_stride, uncond ? uncond : cond, (long)uncond_stride, (int)V, guided, scale, temperature,
              (const int*)pos, (long)pos_stride, (int)pos_bias, (const int*)allowed, (int)allowed_stride, (const int*)forced,
              (int)(n_pos > 0x7fffffff ? 0x7fffffff : n_pos), (int)top_k, top_p, (const long*)target, logprob, (int*)valid, cfg_logits, (long)cfg_stride};
  hipLaunchKernelGGL(ld_token_logprobs_kernel, dim3((unsigned)n), dim3(1024), 0, (hipStream_t)stream, a);
  return ld_check_launch("ld_llm_token_logprobs");
}

LD_API int ld_llm_head_f32(const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc, int64_t M, int64_t N,
                           int64_t K, void* stream) {
  // sizes first: a refused shape is refused whatever the pointers are
  LD_REQUIRE(M >= 1 && N >= 1 && K >= 4 && M <= 0x7fffffff && N <= 0x7fffffff && K <= 0x7fffffff,
             "ld_llm_head_f32: M=%ld N=%ld K=%ld", (long)M, (long)N, (long)K);
  LD_REQUIRE(K % 4 == 0 && lda % 4 == 0 && ldw % 4 == 0, "ld_llm_head_f32: K, lda and ldw must be multiples of 4 (16-byte loads)");
  LD_REQUIRE(A && W && C, "ld_llm_head_f32: null pointer");
  LD_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0, "ld_llm_head_f32: A and W must be 16-byte aligned");
  LD_REQUIRE(lda >= K && ldw >= K && ldc >= N, "ld_llm_head_f32: a row stride shorter than its row");
  const long gx = (N + HEAD_BN - 1) / HEAD_BN, gy = (M + HEAD_BM - 1) / HEAD_BM;
  LD_REQUIRE(gy <= 65535, "ld_llm_head_f32: M=%ld too large", (long)M);
  hipLaunchKernelGGL(ld_head_f32_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, A, (long)lda, W,
                     (long)ldw, C, (long)ldc, (int)M, (int)N, (int)K);
  return ld_check_launch("ld_llm_head_f32");
}
