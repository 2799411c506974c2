// HBM-bound LayerNorm kernels: LayerNorm (+AdaLN modulate, text/image regions), bf16 / fp32 or MXFP8 output.
//
// Replaces: layer.input_layernorm/post_attention_layernorm + modulate
// (landiff/diffusion/dit_video_concat.py:388,577-586,601-611); nn.LayerNorm of TiTok (landiff/tokenizer/modules/blocks.py:292-304).
//
// Pure streaming passes: 16-byte coalesced loads, one wave64 per row or row pair (no LDS, no barriers), fp32 statistics, bf16
// outputs rounded at the same points the reference's bf16 ops round.  The kernels are assembled from the pieces of ld_norm_dev.h.
#include "ld_norm_dev.h"
#include <type_traits>
#include "../../include/landiff_hip.h"

namespace {

// The general kernel: one row per wave, every input / output form.
template <int NC>   // chunks (of 8 elements) per lane
__global__ __launch_bounds__(256) void ld_layernorm_kernel(LnParams p) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= p.rows) return;
  const int nchunk = p.D >> 3;
  float v[NC][8], mean, rstd;
  ln_row_front<NC, true>(p, r, lane, nchunk, v, mean, rstd);
  const bf16_t* shift = nullptr; const bf16_t* scale = nullptr;
  if (p.mod) ln_mod_vectors(p, r, shift, scale);
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    if (c >= nchunk) continue;
    float y[8];
    ln_row_chunk(p, v[i], mean, rstd, shift, scale, c, p.out_f32 != 0, y);
    if (p.out_f32) {
      float* o = (float*)p.out + (long)r * p.ldo + c * 8;
      *(f32x4_t*)o = (f32x4_t){y[0], y[1], y[2], y[3]};
      *(f32x4_t*)(o + 4) = (f32x4_t){y[4], y[5], y[6], y[7]};
    } else {
      u32x4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(y[2 * e], y[2 * e + 1]);
      *(u32x4_t*)((bf16_t*)p.out + (long)r * p.ldo + c * 8) = o;
    }
  }
}

// The DiT's hot form (bf16 in / out, affine weights, AdaLN modulation): two rows per wave, packed math (ld_norm_dev.h).
template <int NC>
__global__ __launch_bounds__(256) void ld_layernorm_mod_kernel(LnParams p) { ln_pair_rows<NC, false>(p); }

// MXFP8 output: the bf16 value the kernels above store, quantised where it is produced -- the activation of the next MXFP8 GEMM.
// In the two-rows-per-wave form (round 6: the one-row kernel below spends ~20 scalar VALU operations per element on bf16 roundings
// and ran at 2.7 TB/s; same bits) ...
template <int NC>
__global__ __launch_bounds__(256) void ld_layernorm_mx2_kernel(LnParams p, unsigned char* mxs, long lds) { ln_pair_rows<NC, true>(p, mxs, lds); }

// ... and one row per wave: every other form (no modulation, no weights)
template <int NC>
__global__ __launch_bounds__(256) void ld_layernorm_mx_kernel(LnParams p, unsigned char* mxs, long lds) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= p.rows) return;
  const int nchunk = p.D >> 3;
  float v[NC][8], mean, rstd;
  ln_row_front<NC, false>(p, r, lane, nchunk, v, mean, rstd);
  const bf16_t* shift = nullptr; const bf16_t* scale = nullptr;
  if (p.mod) ln_mod_vectors(p, r, shift, scale);
  float yv[NC][8], amaxv[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    amaxv[i] = 0.f;
    if (c >= nchunk) continue;
    ln_row_chunk(p, v[i], mean, rstd, shift, scale, c, false, yv[i]);
#pragma unroll
    for (int e = 0; e < 8; ++e) { yv[i][e] = rbf(yv[i][e]); amaxv[i] = fmaxf(amaxv[i], fabsf(yv[i][e])); }      // the bf16 value, quantised below
  }
  // (second pass: the shuffles must be executed by all 64 lanes, including those past the row's last chunk)
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    const float amax = mx_block_amax(c < nchunk ? amaxv[i] : 0.f);
    if (c < nchunk) ln_store_mx(p, mxs, lds, r, c, yv[i], amax);
  }
}

// the instantiation for a row of D: 1, 2, 3 or 4 chunks per lane, or (MAXNC 8) 8 for anything above 4
template <int MAXNC, typename Pick>
auto ln_kernel_for(int64_t D, Pick&& pick) {
  const int nc = (int)((D / 8 + 63) / 64);
  switch (nc) {
    case 1: return pick(std::integral_constant<int, 1>{});
    case 2: return pick(std::integral_constant<int, 2>{});
    case 3: return pick(std::integral_constant<int, 3>{});
    default: return MAXNC > 4 && nc > 4 ? pick(std::integral_constant<int, MAXNC>{}) : pick(std::integral_constant<int, 4>{});
  }
}

// LD_LN_FAST=0: no two-rows-per-wave kernels (one knob for both entry points)
int k_ln_fast = LD_KNOB_UNSET;

// what ld_layernorm and ld_layernorm_mxfp8 have in common
struct LnCall {
  const char* who;
  const void *x, *w, *b, *mod;
  void* out;
  int64_t ldx, ldo, rows, D, mod_bstride, shift_img, scale_img, shift_txt, scale_txt, rows_per_batch, text_len;
  float eps;
  void* stream;
};

int ln_params(const LnCall& a, LnParams& p) {
  LD_REQUIRE((a.w == nullptr) == (a.b == nullptr), "%s: weight and bias go together", a.who);
  p.x = a.x; p.out = a.out; p.w = (const bf16_t*)a.w; p.b = (const bf16_t*)a.b; p.mod = (const bf16_t*)a.mod;
  p.ldx = a.ldx; p.ldo = a.ldo; p.rows = (int)a.rows; p.D = (int)a.D; p.eps = a.eps;
  p.rows_per_batch = a.rows_per_batch > 0 ? (int)a.rows_per_batch : (1 << 30); p.text_len = (int)a.text_len;
  p.mod_bstride = a.mod_bstride; p.shift_img = a.shift_img; p.scale_img = a.scale_img; p.shift_txt = a.shift_txt; p.scale_txt = a.scale_txt;
  return LD_OK;
}

// one wave per row: 4 rows per workgroup; per row pair: 8
template <typename... Mx>      // (the MXFP8 kernels: scale bytes, their row stride)
int ln_launch(const LnCall& a, const LnParams& p, void (*kernel)(LnParams, Mx...), int rows_per_wave, Mx... mx) {
  const int per_wg = 4 * rows_per_wave;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((a.rows + per_wg - 1) / per_wg)), dim3(256), 0, (hipStream_t)a.stream, p, mx...);
  return ld_check_launch(a.who);
}

}  // namespace

LD_API int ld_layernorm(const void* x, int64_t ldx, int32_t x_f32, const void* w, const void* b, void* out, int64_t ldo,
                        int32_t out_f32, int64_t rows, int64_t D, float eps, const void* mod, int64_t mod_bstride,
                        int64_t shift_img, int64_t scale_img, int64_t shift_txt, int64_t scale_txt,
                        int64_t rows_per_batch, int64_t text_len, void* stream) {
  LD_REQUIRE(x && out, "ld_layernorm: null pointer");
  LD_REQUIRE(D % 8 == 0 && D <= 4096 && D > 0, "ld_layernorm: D=%ld must be a multiple of 8 and <= 4096", (long)D);
  const LnCall a{"ld_layernorm", x, w, b, mod, out, ldx, ldo, rows, D, mod_bstride, shift_img, scale_img, shift_txt, scale_txt,
                 rows_per_batch, text_len, eps, stream};
  LnParams p{};
  if (const int rc = ln_params(a, p)) return rc;
  p.x_f32 = x_f32; p.out_f32 = out_f32;
  if (ld_knob("LD_LN_FAST", 1, &k_ln_fast) != 0 && mod && w && !x_f32 && !out_f32 && D <= 2048)        // the DiT's block LayerNorms
    return ln_launch(a, p, ln_kernel_for<4>(D, [](auto nc) { return &ld_layernorm_mod_kernel<decltype(nc)::value>; }), 2);
  return ln_launch(a, p, ln_kernel_for<8>(D, [](auto nc) { return &ld_layernorm_kernel<decltype(nc)::value>; }), 1);
}

LD_API int ld_layernorm_mxfp8(const void* x, int64_t ldx, const void* w, const void* b, void* q, int64_t ldq, void* scales,
                              int64_t lds, int64_t rows, int64_t D, float eps, const void* mod, int64_t mod_bstride,
                              int64_t shift_img, int64_t scale_img, int64_t shift_txt, int64_t scale_txt,
                              int64_t rows_per_batch, int64_t text_len, void* stream) {
  LD_REQUIRE(x && q && scales, "ld_layernorm_mxfp8: null pointer");
  LD_REQUIRE(D % 128 == 0 && D <= 2048 && D > 0 && ldq % 8 == 0 && lds >= rows, "ld_layernorm_mxfp8: D=%ld must be a multiple of 128 and <= 2048, lds >= rows", (long)D);
  const LnCall a{"ld_layernorm_mxfp8", x, w, b, mod, q, ldx, ldq, rows, D, mod_bstride, shift_img, scale_img, shift_txt, scale_txt,
                 rows_per_batch, text_len, eps, stream};
  LnParams p{};                                          // (x_f32 stays 0: bf16 in)
  if (const int rc = ln_params(a, p)) return rc;
  unsigned char* const mxs = (unsigned char*)scales;
  if (ld_knob("LD_LN_FAST", 1, &k_ln_fast) != 0 && mod && w)          // the DiT's block LayerNorms
    return ln_launch(a, p, ln_kernel_for<4>(D, [](auto nc) { return &ld_layernorm_mx2_kernel<decltype(nc)::value>; }), 2, mxs, (long)lds);
  return ln_launch(a, p, ln_kernel_for<4>(D, [](auto nc) { return &ld_layernorm_mx_kernel<decltype(nc)::value>; }), 1, mxs, (long)lds);
}
