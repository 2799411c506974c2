// The distribution the AR sampler draws from, stated once: guided logit, / temperature, optional restriction to the allowed
// ids, optional top-k, softmax, optional top-p (lm_model.py:417-454, utils.py:345-359).  ld_logits_to_probs_kernel
// (ld_llm_sample.hip) turns it into probabilities and draws; ld_token_logprobs_kernel (ld_llm_score.hip) takes one id's
// log-probability under it.  A target on the edge of the nucleus is scored right only if both see the same bits, so both call
// these steps, in this order, from files built with -ffp-contract=off.
// Every function is called by all threads of one workgroup (nt <= 1024 of them, a multiple of 64) on LDS rows of
// LD_SAMPLE_MAXV floats: sv = one value per vocabulary id, ss = the values in descending order, red = 32 words.
#pragma once
#include "ld_common.h"
#include "../../include/landiff_hip.h"

__device__ __forceinline__ float block_sum_1024(float v, float* red, int tid, int nthreads) {
  v = wave_sum(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float tot = 0.f;
  for (int w = 0; w < (nthreads >> 6); ++w) tot += red[w];
  return tot;
}

// (a) sv[i] = filtered logit of id i.  lc / lu: the conditional / unconditional rows (lu is read when guided); cfg_out
// (optional) receives the guided logits; al (optional) = the allowed-ids row of the position being generated: {n, id_0 ..}.
// Returns n, the number of allowed ids (0: unrestricted).  Ends with a barrier.
__device__ __forceinline__ int dist_fill(float* sv, const float* lc, const float* lu, int guided, float scale, float temperature,
                                         float* cfg_out, const int* al, int V, int tid, int nt) {
  const int nal = al ? al[0] : 0;
  for (int i = tid; i < V; i += nt) {
    float l = lc[i];
    if (guided) { const float u = lu[i]; l = u + scale * (l - u); }
    if (cfg_out) cfg_out[i] = l;
    l = l / temperature;
    if (nal > 0) {
      bool ok = false;
      for (int a = 0; a < nal; ++a) ok |= (al[1 + a] == i);
      if (!ok) l = -INFINITY;
    }
    sv[i] = l;
  }
  __syncthreads();
  return nal;
}

// (b) top-k (unrestricted positions only): everything below the k-th largest logit -> -inf; ties at the threshold stay
__device__ __forceinline__ void dist_top_k(float* sv, float* thr_s, int top_k, int nal, int V, int tid, int nt) {
  if (top_k > 0 && top_k < V && nal == 0) {
    for (int i = tid; i < V; i += nt) {
      const float v = sv[i];
      int gt = 0, ge = 0;
      for (int j = 0; j < V; ++j) { const float o = sv[j]; gt += (o > v); ge += (o >= v); }
      if (gt < top_k && top_k <= ge) *thr_s = v;              // every writer holds the same value
    }
    __syncthreads();
    const float thr = *thr_s;
    for (int i = tid; i < V; i += nt) if (sv[i] < thr) sv[i] = -INFINITY;
    __syncthreads();
  }
}

// (c) the largest filtered logit.  No barrier after the read of red: (d) has one before it writes there.
__device__ __forceinline__ float dist_max(const float* sv, float* red, int V, int tid, int nt) {
  float mx = -3.0e38f;
  for (int i = tid; i < V; i += nt) mx = fmaxf(mx, sv[i]);
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  float m2 = red[0];
  for (int w = 1; w < (nt >> 6); ++w) m2 = fmaxf(m2, red[w]);
  return m2;
}

// (d) sv[i] = exp(sv[i] - m2); returns their sum
__device__ __forceinline__ float dist_exp_sum(float* sv, float* red, float m2, int V, int tid, int nt) {
  float s = 0.f;
  for (int i = tid; i < V; i += nt) { const float e = expf(sv[i] - m2); sv[i] = e; s += e; }
  return block_sum_1024(s, red, tid, nt);
}

__device__ __forceinline__ void dist_divide(float* sv, float by, int V, int tid, int nt) {
  for (int i = tid; i < V; i += nt) sv[i] = sv[i] / by;
  __syncthreads();
}

// (e) top-p over the probabilities sv (unrestricted positions only): sorted position j >= 1 is dropped when cumsum[j-1] >= top_p.
// dropped(i) is called for every dropped id i; returns the mass that is kept (the caller renormalises by it).
__device__ __forceinline__ bool dist_top_p_applies(float top_p, int nal) { return top_p >= 0.f && nal == 0; }
template <class Dropped>
__device__ __forceinline__ float dist_top_p(const float* sv, float* ss, float* red, float top_p, int V, int tid, int nt,
                                            Dropped dropped) {
  int rk[(LD_SAMPLE_MAXV + 1023) / 1024];
  int c = 0;
  for (int i = tid; i < V; i += nt, ++c) {
    const float v = sv[i];
    int r = 0;
    for (int j = 0; j < V; ++j) { const float o = sv[j]; r += (o > v) || (o == v && j < i); }   // stable descending rank
    rk[c] = r;
    ss[r] = v;
  }
  __syncthreads();
  if (tid == 0) {                                            // sequential fp32 cumsum (torch.cumsum's CPU order)
    float acc = 0.f;
    for (int j = 0; j < V; ++j) { acc += ss[j]; ss[j] = acc; }
  }
  __syncthreads();
  float ks = 0.f;
  c = 0;
  for (int i = tid; i < V; i += nt, ++c) {
    const int r = rk[c];
    float p = sv[i];
    if (r >= 1 && ss[r - 1] >= top_p) { p = 0.f; dropped(i); }
    ks += p;
  }
  return block_sum_1024(ks, red, tid, nt);
}
