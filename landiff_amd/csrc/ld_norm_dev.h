// Device pieces of the LayerNorm kernels (ld_norm_layer.hip): each of them written once and shared by the one-row / two-row and the
// bf16-output / MXFP8-output kernels, which therefore take the same statistics and round at the same points by construction.
// One wave64 per row (or row pair), no LDS, no barriers; lane l holds the 8-element chunks l, l + 64, ... of the row.
#pragma once
#include "ld_common.h"
#include "ld_mx.h"

// LayerNorm over D (D % 8 == 0, D <= 4096), optional AdaLN modulation selected per row region.
struct LnParams {
  const void* x; void* out;
  const bf16_t* w; const bf16_t* b;
  const bf16_t* mod;            // modulation vectors, or null
  long ldx, ldo;
  int rows, D;
  float eps;
  int x_f32, out_f32;
  int rows_per_batch, text_len;
  long mod_bstride, shift_img, scale_img, shift_txt, scale_txt;
};

typedef ld_f32x2_t f32x2_t;

// row -> its modulation vectors: batch = row / rows_per_batch, the text vectors for the batch's first text_len rows
__device__ __forceinline__ void ln_mod_vectors(const LnParams& p, int r, const bf16_t*& shift, const bf16_t*& scale) {
  const int bb = r / p.rows_per_batch;
  const bool txt = (r - bb * p.rows_per_batch) < p.text_len;
  shift = p.mod + bb * p.mod_bstride + (txt ? p.shift_txt : p.shift_img);
  scale = p.mod + bb * p.mod_bstride + (txt ? p.scale_txt : p.scale_img);
}

// ---- one row per wave ----
// Loads row r (bf16, or fp32 where the kernel allows it: X_F32_OK) and takes its statistics.
template <int NC, bool X_F32_OK>   // NC: chunks (of 8 elements) per lane
__device__ __forceinline__ void ln_row_front(const LnParams& p, int r, int lane, int nchunk, float (&v)[NC][8], float& mean, float& rstd) {
  float s = 0.f, s_odd = 0.f;       // even / odd elements summed apart: the order of ln_pair_front's packed sums
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    if (c < nchunk) {
      if (X_F32_OK && p.x_f32) {
        const float* xr = (const float*)p.x + (long)r * p.ldx + c * 8;
        const f32x4_t a = *(const f32x4_t*)xr, b4 = *(const f32x4_t*)(xr + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[i][e] = a[e]; v[i][4 + e] = b4[e]; }
      } else {
        const u32x4_t a = *(const u32x4_t*)((const bf16_t*)p.x + (long)r * p.ldx + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[i][2 * e] = bf_lo(a[e]); v[i][2 * e + 1] = bf_hi(a[e]); }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) { s += v[i][2 * e]; s_odd += v[i][2 * e + 1]; }
    }
  }
  mean = wave_sum(s + s_odd) / (float)p.D;
  float ss = 0.f, ss_odd = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    if (lane + 64 * i < nchunk) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d0 = v[i][2 * e] - mean, d1 = v[i][2 * e + 1] - mean;
        ss += d0 * d0; ss_odd += d1 * d1;
      }
    }
  }
  rstd = rsqrtf(wave_sum(ss + ss_odd) / (float)p.D + p.eps);
}

// Chunk c of a row: normalise, affine (with weights), modulate (shift non-null).  The rounding rule of the one-row kernels: a
// modulated value is bf16 -- modulate() is x * (1 + scale) + shift with every op in bf16, as in the reference -- so it is rounded
// before it is stored or quantised; an unmodulated value is fp32 and rounded by the store.  The last rounding of modulate(), that
// of the sum, is therefore left to a bf16 store or the quantiser's bf16 rounding, and done here (round_sum) for an fp32 store.
__device__ __forceinline__ void ln_row_chunk(const LnParams& p, const float (&v)[8], float mean, float rstd, const bf16_t* shift,
                                             const bf16_t* scale, int c, bool round_sum, float (&y)[8]) {
  float wv[8], bv[8];
  if (p.w) {
    const u32x4_t ww = *(const u32x4_t*)(p.w + c * 8), bw = *(const u32x4_t*)(p.b + c * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) { wv[2 * e] = bf_lo(ww[e]); wv[2 * e + 1] = bf_hi(ww[e]); bv[2 * e] = bf_lo(bw[e]); bv[2 * e + 1] = bf_hi(bw[e]); }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float t = (v[e] - mean) * rstd;
    if (p.w) t = t * wv[e] + bv[e];
    y[e] = t;
  }
  if (shift) {
    const u32x4_t sh = *(const u32x4_t*)(shift + c * 8), sc = *(const u32x4_t*)(scale + c * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float s0 = rbf(1.0f + bf_lo(sc[e])), s1 = rbf(1.0f + bf_hi(sc[e]));
      y[2 * e] = rbf(rbf(y[2 * e]) * s0) + bf_lo(sh[e]);
      y[2 * e + 1] = rbf(rbf(y[2 * e + 1]) * s1) + bf_hi(sh[e]);
    }
    if (round_sum) {
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = rbf(y[e]);
    }
  }
}

// ---- two rows per wave: the DiT's hot form (bf16 in, affine weights, AdaLN modulation) ----
// The same operations at the same roundings as the one-row pieces, arranged for VALU issue count -- those spend ~25 VALU operations
// per element, more issue time than the row's HBM time; these ~11:
//  * element PAIRS: one v_cvt_pk_bf16_f32 per bf16 rounding of two elements, v_pk_{add,mul,fma}_f32 for the arithmetic (a
//    bf16 pair unpacks into an adjacent register pair);
//  * TWO rows per wave: the four per-column vectors (weight, bias, shift, scale) are loaded and unpacked once for both.
// The statistics are summed per pair lane (even / odd elements) and combined at the end.
//
// Rows r0 and r0 + 1 (has1; an odd row count: the last wave does its row twice): v = x - mean, rstd and the modulation vectors of both.
template <int NC>
__device__ __forceinline__ void ln_pair_front(const LnParams& p, int r0, bool has1, int lane, int nchunk, f32x2_t (&v)[2][NC][4],
                                              float (&rstd)[2], const bf16_t* (&shift)[2], const bf16_t* (&scale)[2]) {
  u32x4_t raw[2][NC];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const bf16_t* xr = (const bf16_t*)p.x + (long)(r0 + (has1 ? j : 0)) * p.ldx;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + 64 * i;
      raw[j][i] = (u32x4_t){0u, 0u, 0u, 0u};
      if (c < nchunk) raw[j][i] = *(const u32x4_t*)(xr + c * 8);
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) ln_mod_vectors(p, r0 + (has1 ? j : 0), shift[j], scale[j]);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    f32x2_t s2 = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NC; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[j][i][e] = unpack_bf16x2(raw[j][i][e]); s2 += v[j][i][e]; }      // chunks past the row are zeros
    const float mean = wave_sum(s2[0] + s2[1]) / (float)p.D;
    const f32x2_t mean2 = {mean, mean};
    f32x2_t ss2 = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      if (lane + 64 * i < nchunk) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[j][i][e] -= mean2; ss2 += v[j][i][e] * v[j][i][e]; }
      }
    }
    rstd[j] = rsqrtf(wave_sum(ss2[0] + ss2[1]) / (float)p.D + p.eps);
  }
}

// MXFP8 output of chunk c of row r (codes to p.out, the block's scale byte to mxs [D/128][lds rows][4]): y holds the bf16 values
// the bf16-output kernels store, block_amax their block's maximum.  A 32-element MX block is the chunks of four adjacent lanes
// (c = lane + 64 i), so every lane of the wave takes part in a chunk index's mx_block_amax, also past the row's last chunk; only
// lanes with a chunk get here.
__device__ __forceinline__ void ln_store_mx(const LnParams& p, unsigned char* mxs, long lds, long r, int c, const float (&y)[8], float block_amax) {
  float inv;
  const int sb = mx_scale_byte(block_amax, inv);
  *(u32x2_t*)((unsigned char*)p.out + r * p.ldo + c * 8) = mx_pack8(y, inv);
  if ((c & 3) == 0) mxs[mx_scale_index(r, c * 8, lds)] = (unsigned char)sb;
}

// LayerNorm + modulate of both rows, chunk by chunk.  SAME: both rows take the same modulation vectors.  The output step is all that
// MX changes: a bf16 store, or the same bf16 values quantised to MXFP8 -- then lanes past the row's last chunk come along for the
// block maxima (live false: they read chunk 0 and store nothing).
template <int NC, bool SAME, bool MX>
__device__ __forceinline__ void ln_pair_apply(const LnParams& p, f32x2_t (&v)[2][NC][4], const float (&rstd)[2], const bf16_t* const (&shift)[2],
                                              const bf16_t* const (&scale)[2], int r0, bool has1, int lane, int nchunk, unsigned char* mxs, long lds) {
  const f32x2_t one2 = {1.0f, 1.0f};
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    const bool live = c < nchunk;
    if (!MX && !live) continue;
    const int cc = live ? c : 0;
    const u32x4_t ww = *(const u32x4_t*)(p.w + cc * 8), bw = *(const u32x4_t*)(p.b + cc * 8);
    u32x4_t sh[2], sc[2];
    sh[0] = *(const u32x4_t*)(shift[0] + cc * 8); sc[0] = *(const u32x4_t*)(scale[0] + cc * 8);
    if (!SAME) { sh[1] = *(const u32x4_t*)(shift[1] + cc * 8); sc[1] = *(const u32x4_t*)(scale[1] + cc * 8); }
    f32x2_t y[2][4];
    float amax[2] = {0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const f32x2_t w2 = unpack_bf16x2(ww[e]), b2 = unpack_bf16x2(bw[e]);
      f32x2_t sp[2], st[2];
#pragma unroll
      for (int j = 0; j < (SAME ? 1 : 2); ++j) {
        sp[j] = rbf2(unpack_bf16x2(sc[j][e]) + one2);
        st[j] = unpack_bf16x2(sh[j][e]);
      }
      if (SAME) { sp[1] = sp[0]; st[1] = st[0]; }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const f32x2_t rs = {rstd[j], rstd[j]};
        f32x2_t t = rbf2(v[j][i][e] * rs * w2 + b2);              // LayerNorm output in bf16
        // modulate(): x * (1 + scale) + shift, every op in bf16 as in the reference (dit_video_concat.py:388); the last rounding, of
        // the sum, is the bf16 store's own, or made here before the value is quantised
        t = rbf2(t * sp[j]) + st[j];
        if (MX) { t = rbf2(t); amax[j] = fmaxf(amax[j], fmaxf(fabsf(t[0]), fabsf(t[1]))); }
        y[j][e] = t;
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float am = 0.f;
      if (MX) am = mx_block_amax(live ? amax[j] : 0.f);
      if (!live || (j == 1 && !has1)) continue;
      if (MX) {
        const float f[8] = {y[j][0][0], y[j][0][1], y[j][1][0], y[j][1][1], y[j][2][0], y[j][2][1], y[j][3][0], y[j][3][1]};
        ln_store_mx(p, mxs, lds, r0 + j, c, f, am);
      } else {
        u32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(y[j][e]);
        *(u32x4_t*)((bf16_t*)p.out + (long)(r0 + j) * p.ldo + c * 8) = o;
      }
    }
  }
}

// A row pair per wave, start to end: the body of the two two-rows-per-wave kernels.
template <int NC, bool MX>
__device__ __forceinline__ void ln_pair_rows(const LnParams& p, unsigned char* mxs = nullptr, long lds = 0) {
  const int lane = threadIdx.x & 63;
  const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2;
  if (r0 >= p.rows) return;
  const bool has1 = r0 + 1 < p.rows;
  const int nchunk = p.D >> 3;
  f32x2_t v[2][NC][4];
  float rstd[2];
  const bf16_t* shift[2]; const bf16_t* scale[2];
  ln_pair_front<NC>(p, r0, has1, lane, nchunk, v, rstd, shift, scale);
  if (shift[0] == shift[1] && scale[0] == scale[1]) ln_pair_apply<NC, true, MX>(p, v, rstd, shift, scale, r0, has1, lane, nchunk, mxs, lds);
  else ln_pair_apply<NC, false, MX>(p, v, rstd, shift, scale, r0, has1, lane, nchunk, mxs, lds);
}
