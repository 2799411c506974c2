// Shared by the bf16 / fp8 GEMM and implicit-GEMM convolution files (ld_gemm*.hip): the kernel parameter block, the fused
// epilogues (device code), the LDS-DMA staging helpers and the host-side launch helpers.  ld_gemm.hip plans a call (which kernel
// family, which tiles); ld_gemm_2stage.hip, ld_gemm_8p.hip, ld_gemm_fp8.hip and ld_gemm_variants.hip hold the kernels and their launchers;
// ld_gemm_8p_dev.h holds what the kernels share around the main loop (raster, tile source, addresses, counted waits, tile walk).
#pragma once
#include "ld_common.h"
#include "ld_mx.h"
#include <type_traits>

namespace ldgemm {

constexpr int BK = 64;
typedef int i32x8_t __attribute__((ext_vector_type(8)));      // operand of the f8f6f4 MFMAs
constexpr int CW_STRIDE = 68;                    // fp32 row stride of the epilogue staging tile (64 cols + pad)

struct GemmParams {
  const bf16_t* A;
  const bf16_t* W;
  void* out;
  const bf16_t* bias;
  const bf16_t* mul;
  const void* resid;
  const bf16_t* gate;
  const bf16_t* add2;
  int M, N, K;
  long lda, ldo, ldr, ldmul, ldadd;
  int act;
  int out_f32, resid_f32;
  int rows_per_batch, text_len;
  long gate_bstride, gate_off_img, gate_off_txt;
  // conv (channels-last, zero-bordered input)
  int H, W_, Hp, Wp, Cin, kH, kW;   // output H,W; padded input Hp,Wp
  int group_m;                      // tile-raster group height (L2 locality)
  int m_begin;                      // first output row of this launch (rows stay absolute: M is the end row)
  // fp8 (e4m3) operands: A and W are byte matrices (lda in bytes), dequantised by per-row / per-output-channel scales
  const float* scale_a;             // [M]
  const float* scale_w;             // [N]
  // MXFP8 form: one E8M0 scale byte per 32 consecutive K elements, stored K-tile-major [K / 128][rows][4] so that the 256
  // rows of a tile and K-tile are 1 KB contiguous (a [rows][K / 32] strip cost one cache line per row and K-tile)
  const unsigned char* mx_a;
  const unsigned char* mx_w;
  unsigned char* mx_out;            // non-null: the output itself is MXFP8 (out = e4m3 bytes, ldo in bytes; scales here)
  long ld_mx_out;
  // fused qkv head split (EPI_QKV): N = 3 * heads * 64 columns [q | k | v]; out is unused
  bf16_t* q_out; bf16_t* k_out; bf16_t* vt_out;       // Q, K [B][heads][Npad][64], V^T [B][heads][64][Npad]
  const bf16_t* qn_w; const bf16_t* qn_b; const bf16_t* kn_w; const bf16_t* kn_b;   // QK-LayerNorm(64) weights
  int heads, Ntok, Npad;
  float qk_eps;
  // 8-phase kernels: the launch covers tiles [tile_begin, tile_end) of the 256 x 256 raster (tile_end == 0: all of them);
  // walk_tiles (ld_gemm_8p_dev.h) is the one reader.  The whole rounds of the chip go to ld_gemm8p_kernel, the partial last round
  // to ld_gemm8p_n128_kernel as 256 x 128 half tiles.
  int tile_begin, tile_end;
  // convolutions only: GroupNorm partial statistics of the bf16 output, [ceil(M / 64)][N / 4][2] fp32 = (sum, sum of squares) of
  // every 64-row x 4-channel patch, written by the epilogue that holds the values anyway (ld_conv_cl_bf16_gn); null: none
  float* gn_part;
};

__device__ __forceinline__ void glds16(const bf16_t* g, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)g,
      (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// epilogue on 8 consecutive columns of one output row
__device__ __forceinline__ void epilogue_store8(const GemmParams& p, float (&v)[8], int gm, int gn0, bool vec_ok) {
  const int nvalid = (p.N - gn0) < 8 ? (p.N - gn0) : 8;
  const bf16_t* gate_row = nullptr;
  if (p.gate) {
    const int b = gm / p.rows_per_batch;
    const int rin = gm - b * p.rows_per_batch;
    gate_row = p.gate + b * p.gate_bstride + (rin < p.text_len ? p.gate_off_txt : p.gate_off_img);
  }
  if (vec_ok) {
    float bias[8], mulv[8], gt[8], rs[8], ad[8];
    if (p.bias) {
      const u32x4_t bw = *(const u32x4_t*)(p.bias + gn0);
#pragma unroll
      for (int e = 0; e < 4; ++e) { bias[2 * e] = bf_lo(bw[e]); bias[2 * e + 1] = bf_hi(bw[e]); }
    }
    if (p.mul) {
      const u32x4_t mw = *(const u32x4_t*)(p.mul + (long)gm * p.ldmul + gn0);
#pragma unroll
      for (int e = 0; e < 4; ++e) { mulv[2 * e] = bf_lo(mw[e]); mulv[2 * e + 1] = bf_hi(mw[e]); }
    }
    if (gate_row) {
      const u32x4_t gw = *(const u32x4_t*)(gate_row + gn0);
#pragma unroll
      for (int e = 0; e < 4; ++e) { gt[2 * e] = bf_lo(gw[e]); gt[2 * e + 1] = bf_hi(gw[e]); }
    }
    if (p.resid) {
      if (p.resid_f32) {
        const f32x4_t r0 = *(const f32x4_t*)((const float*)p.resid + (long)gm * p.ldr + gn0);
        const f32x4_t r1 = *(const f32x4_t*)((const float*)p.resid + (long)gm * p.ldr + gn0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { rs[e] = r0[e]; rs[4 + e] = r1[e]; }
      } else {
        const u32x4_t rw = *(const u32x4_t*)((const bf16_t*)p.resid + (long)gm * p.ldr + gn0);
#pragma unroll
        for (int e = 0; e < 4; ++e) { rs[2 * e] = bf_lo(rw[e]); rs[2 * e + 1] = bf_hi(rw[e]); }
      }
    }
    if (p.add2) {
      const u32x4_t aw = *(const u32x4_t*)(p.add2 + (long)gm * p.ldadd + gn0);
#pragma unroll
      for (int e = 0; e < 4; ++e) { ad[2 * e] = bf_lo(aw[e]); ad[2 * e + 1] = bf_hi(aw[e]); }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float x = v[e];
      if (p.bias) x += bias[e];
      x = rbf(x);                                   // bf16 Linear/conv output
      if (p.act) x = rbf(apply_act(p.act, x));
      if (p.mul) x = rbf(x * mulv[e]);
      if (gate_row) x = rbf(x * gt[e]);
      if (p.resid) { x = rs[e] + x; if (!p.out_f32) x = rbf(x); }
      if (p.add2) { x = x + ad[e]; if (!p.out_f32) x = rbf(x); }
      v[e] = x;
    }
    if (p.out_f32) {
      float* o = (float*)p.out + (long)gm * p.ldo + gn0;
      *(f32x4_t*)o = (f32x4_t){v[0], v[1], v[2], v[3]};
      *(f32x4_t*)(o + 4) = (f32x4_t){v[4], v[5], v[6], v[7]};
    } else {
      u32x4_t ow;
#pragma unroll
      for (int e = 0; e < 4; ++e) ow[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
      *(u32x4_t*)((bf16_t*)p.out + (long)gm * p.ldo + gn0) = ow;
    }
  } else {
    for (int e = 0; e < nvalid; ++e) {
      const int gn = gn0 + e;
      float x = v[e];
      if (p.bias) x += bf2f(p.bias[gn]);
      x = rbf(x);
      if (p.act) x = rbf(apply_act(p.act, x));
      if (p.mul) x = rbf(x * bf2f(p.mul[(long)gm * p.ldmul + gn]));
      if (gate_row) x = rbf(x * bf2f(gate_row[gn]));
      if (p.resid) {
        const float r = p.resid_f32 ? ((const float*)p.resid)[(long)gm * p.ldr + gn]
                                    : bf2f(((const bf16_t*)p.resid)[(long)gm * p.ldr + gn]);
        x = r + x; if (!p.out_f32) x = rbf(x);
      }
      if (p.add2) { x = x + bf2f(p.add2[(long)gm * p.ldadd + gn]); if (!p.out_f32) x = rbf(x); }
      if (p.out_f32) ((float*)p.out)[(long)gm * p.ldo + gn] = x;
      else ((bf16_t*)p.out)[(long)gm * p.ldo + gn] = f2bf(x);
    }
  }
}

// Epilogue shared by both main loops: per MFMA row-block, accumulators -> wave-private LDS (fp32) -> row-contiguous
// 16-byte stores (wave tile = MI x NI MFMA 32x32 tiles, NI * 32 == 64 columns).  Must be entered with all main-loop
// LDS traffic of the whole workgroup retired (a barrier); inside, every wave works on its own staging tile, so the only
// ordering needed is the in-order execution of one wave's own DS instructions -- no workgroup barriers.
//
// Code size is the constraint here: the epilogue is straight-line code that every wave walks once per tile, and a
// body that carries every runtime feature (four activations inlined per element) grew the kernel past 160 KB -- more
// than the instruction cache, so each tile paid tens of microseconds of instruction fetch.  The three epilogues of
// the DiT layer are therefore compile-time specialisations (a few KB each, fully unrolled, operands of a row-block
// requested before its accumulators are staged); everything else takes the compact generic path.
enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_GATE = 2, EPI_GENERIC = 3, EPI_GELU_MX = 4, EPI_QKV = 5 };   // 4: bias + GELU, MXFP8 output; 5: qkv head split

// stage_block(ic) writes the 32 x 64 fp32 values of 32-row block ic of the wave tile into cw[32][CW_STRIDE] -- the only part
// that depends on the MFMA shape the accumulators came from (gemm_epilogue: 32x32x16, gemm_epilogue16: 16x16x32).
// hook(): called once, right after the epilogue's FIRST global loads have been issued (bias; gate / residual / control add of
// the first row block) and before anything waits on them.  The persistent 8-phase kernel issues the next tile's first K-tile
// there: LDS-DMA and loads retire in order, so anything the epilogue loads after that would wait for the DMA to land.
struct NoHook { __device__ __forceinline__ void operator()() const {} };
//
// GN (the convolution kernels): with p.gn_part set, every lane also sums the FINAL bf16 values it stores -- 8 consecutive channels
// of 4 rows per 32-row block -- as two 4-channel quads (sum, sum of squares), and after every second row block the 8 lanes that
// hold the same columns meet in a fixed butterfly and lane 0..7 store the 64-row patch's four numbers.  Each (64-row unit, quad)
// is written exactly once per launch, by a fixed sequence of fp32 additions: deterministic; ld_gn_stats_from_partials_kernel
// (ld_norm_group.hip) sums the units in double in index order.  Replaces the separate read of the whole activation by
// ld_gn_stats_kernel for the VAE's GroupNorms, all of which normalise a convolution's output (cp_enc_dec.py:546-569, 745-782).
template <int MI, int EPI, typename StageFn, typename Hook = NoHook, bool GN = false>
__device__ __forceinline__ void gemm_epilogue_core(const GemmParams& p, StageFn&& stage_block, float* cw, int lane,
                                                   int row0, int col0w, Hook&& hook = Hook{}) {
  const int col0 = (lane & 7) * 8;
  const int gn0 = col0w + col0;
  static_assert(!GN || (MI % 2 == 0 && (EPI == EPI_BIAS || EPI == EPI_GENERIC)), "GroupNorm partials: 64-row units, conv epilogues");
  float gq[4] = {0.f, 0.f, 0.f, 0.f};                       // quad 0 (sum, sumsq), quad 1 (sum, sumsq)
  auto gn_add = [&](const float (&v)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { gq[0] += v[e]; gq[1] += v[e] * v[e]; }
#pragma unroll
    for (int e = 4; e < 8; ++e) { gq[2] += v[e]; gq[3] += v[e] * v[e]; }
  };
  auto gn_flush = [&](int unit_row0) {                       // all 64 lanes get here together
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float a = gq[q];
      a += __shfl_xor(a, 8, 64); a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
      gq[q] = a;
    }
    if (lane < 8 && gn0 < p.N && unit_row0 < p.M)
      *(f32x4_t*)(p.gn_part + ((long)(unit_row0 >> 6) * (p.N >> 2) + (gn0 >> 2)) * 2) = (f32x4_t){gq[0], gq[1], gq[2], gq[3]};
    gq[0] = gq[1] = gq[2] = gq[3] = 0.f;
  };
  if constexpr (EPI == EPI_GENERIC) {
    hook();
    const bool vec_ok = ((p.N & 7) == 0) && ((p.ldo & 7) == 0) &&
                        (p.resid == nullptr || (p.ldr & 7) == 0) &&
                        (p.mul == nullptr || (p.ldmul & 7) == 0) &&
                        (p.add2 == nullptr || (p.ldadd & 7) == 0);
    auto row_block = [&](auto ic) {
      constexpr int i = decltype(ic)::value;
      stage_block(ic);
#pragma unroll 1
      for (int ps = 0; ps < 4; ++ps) {
        const int row = ps * 8 + (lane >> 3);
        const int gm = row0 + i * 32 + row;
        if (gm < p.M && gn0 < p.N) {
          float v[8];
          const f32x4_t lo = *(const f32x4_t*)(cw + row * CW_STRIDE + col0);
          const f32x4_t hi = *(const f32x4_t*)(cw + row * CW_STRIDE + col0 + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
          epilogue_store8(p, v, gm, gn0, vec_ok);
          if constexpr (GN) if (p.gn_part) gn_add(v);       // vec_ok (the launcher checks): v holds the stored, rounded values
        }
      }
      if constexpr (GN && (i & 1)) if (p.gn_part) gn_flush(row0 + (i - 1) * 32);
    };
    row_block(std::integral_constant<int, 0>{});
    if constexpr (MI > 1) row_block(std::integral_constant<int, 1>{});
    if constexpr (MI > 2) row_block(std::integral_constant<int, 2>{});
    if constexpr (MI > 3) row_block(std::integral_constant<int, 3>{});
  } else {
    // specialised: N % 8 == 0, all leading dimensions % 8 == 0, bf16 output (checked by the launcher)
    const bool col_ok = gn0 < p.N;
    float bias[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bias[e] = 0.f;
    if (p.bias && col_ok) {
      const u32x4_t bw = *(const u32x4_t*)(p.bias + gn0);
#pragma unroll
      for (int e = 0; e < 4; ++e) { bias[2 * e] = bf_lo(bw[e]); bias[2 * e + 1] = bf_hi(bw[e]); }
    }
    // gate row selection without a division per row: the tile's first batch and the next batch boundary
    int bnd = 0, b0 = 0;
    if constexpr (EPI == EPI_GATE) {
      b0 = row0 / p.rows_per_batch;
      bnd = (b0 + 1) * p.rows_per_batch;
    }
    const int rsub = lane >> 3;
    auto row_block = [&](auto ic) {
      constexpr int i = decltype(ic)::value;
      u32x4_t g[4], rs[4], ad[4];
      if constexpr (EPI == EPI_GATE) {
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
          const int gm = row0 + i * 32 + ps * 8 + rsub;
          g[ps] = rs[ps] = ad[ps] = (u32x4_t){0u, 0u, 0u, 0u};
          if (gm < p.M && col_ok) {
            const int b = gm >= bnd ? b0 + 1 : b0;
            const int rin = gm - b * p.rows_per_batch;
            g[ps] = *(const u32x4_t*)(p.gate + b * p.gate_bstride + (rin < p.text_len ? p.gate_off_txt : p.gate_off_img) + gn0);
            rs[ps] = *(const u32x4_t*)((const bf16_t*)p.resid + (long)gm * p.ldr + gn0);
            if (p.add2) ad[ps] = *(const u32x4_t*)(p.add2 + (long)gm * p.ldadd + gn0);
          }
        }
      }
      if constexpr (i == 0) hook();
      stage_block(ic);
#pragma unroll
      for (int ps = 0; ps < 4; ++ps) {
        const int row = ps * 8 + rsub;
        const int gm = row0 + i * 32 + row;
        const f32x4_t lo = *(const f32x4_t*)(cw + row * CW_STRIDE + col0);
        const f32x4_t hi = *(const f32x4_t*)(cw + row * CW_STRIDE + col0 + 4);
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
#pragma unroll
        for (int e = 0; e < 4; ++e) {                       // element pairs: one cvt_pk per bf16 rounding of two values
          ld_f32x2_t x = rbf2((ld_f32x2_t){v[2 * e], v[2 * e + 1]} + (ld_f32x2_t){bias[2 * e], bias[2 * e + 1]});      // bf16 Linear output
          if constexpr (EPI == EPI_GELU || EPI == EPI_GELU_MX) x = act_gelu_tanh2(x);
          if constexpr (EPI == EPI_GATE) {
            x = rbf2(x * unpack_bf16x2(g[ps][e]));
            x = unpack_bf16x2(rs[ps][e]) + x;               // rounded by the pack below (or here, when another term follows)
            if (p.add2) x = rbf2(x) + unpack_bf16x2(ad[ps][e]);
          }
          v[2 * e] = x[0]; v[2 * e + 1] = x[1];
        }
        if constexpr (EPI == EPI_GELU_MX) {
          // the bf16 activation, quantised where it is produced: a 32-column MX block is the 8 columns of four adjacent
          // lanes of the same row (lane bits 0-1)
          float amax = 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) {       // round to bf16 pairwise (one cvt_pk + two unpacks per pair)
            const uint32_t pk = pack_bf16x2(v[2 * e], v[2 * e + 1]);
            v[2 * e] = bf_lo(pk); v[2 * e + 1] = bf_hi(pk);
            amax = fmaxf(amax, fmaxf(fabsf(v[2 * e]), fabsf(v[2 * e + 1])));
          }
          float inv;
          const int sb = mx_scale_byte(mx_block_amax(amax), inv);
          if (gm < p.M && col_ok) {
            *(u32x2_t*)((unsigned char*)p.out + (long)gm * p.ldo + gn0) = mx_pack8(v, inv);
            if ((lane & 3) == 0) p.mx_out[mx_scale_index(gm, gn0, p.ld_mx_out)] = (unsigned char)sb;
          }
        } else if (gm < p.M && col_ok) {
          u32x4_t ow;
#pragma unroll
          for (int e = 0; e < 4; ++e) ow[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
          __builtin_nontemporal_store(ow, (u32x4_t*)((bf16_t*)p.out + (long)gm * p.ldo + gn0));
          if constexpr (GN) if (p.gn_part) gn_add(v);       // EPI_BIAS: v = rbf2(acc + bias), already the stored values
        }
      }
      if constexpr (GN && (i & 1)) if (p.gn_part) gn_flush(row0 + (i - 1) * 32);
    };
    // explicit expansion: a `#pragma unroll` over a body this large is silently dropped and acc[] lands in scratch
    row_block(std::integral_constant<int, 0>{});
    if constexpr (MI > 1) row_block(std::integral_constant<int, 1>{});
    if constexpr (MI > 2) row_block(std::integral_constant<int, 2>{});
    if constexpr (MI > 3) row_block(std::integral_constant<int, 3>{});
  }
  static_assert(MI <= 4, "extend the expansion");
}

template <int MI, int NI, int EPI, bool GN = false>
__device__ __forceinline__ void gemm_epilogue(const GemmParams& p, f32x16_t (&acc)[MI][NI], char* smem, int wave, int lane,
                                              int row0, int col0w) {
  float* cw = (float*)smem + wave * (32 * CW_STRIDE);
  auto stage_block = [&](auto ic) {
    constexpr int i = decltype(ic)::value;
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        cw[row * CW_STRIDE + j * 32 + (lane & 31)] = acc[i][j][r];
      }
  };
  gemm_epilogue_core<MI, EPI, decltype(stage_block)&, NoHook, GN>(p, stage_block, cw, lane, row0, col0w);
}

// Accumulators of v_mfma_f32_16x16x32_bf16: acc[i][j][r] = C[i * 16 + (lane >> 4) * 4 + r][j * 16 + (lane & 15)], a wave tile of
// (MI * 32) rows x 64 columns = [2 * MI][4] blocks starting at column block j0.
// SWAP: the accumulators came from MFMAs with the operands exchanged (W fragment first), i.e. blocks of C^T:
//   acc[i][j][r] = C[i * 16 + (lane & 15)][j * 16 + (lane >> 4) * 4 + r]
// -- a lane's four registers are four consecutive COLUMNS of one row, so staging a block is ONE ds_write_b128 per lane instead of
// four ds_write_b32 (128 -> 32 LDS store instructions per wave tile; conflict-free: the 8 lanes of a store group are 8 rows,
// 68 dwords apart).  Same dot products, same results.
template <int MI, int EPI, int NJ, bool SWAP = false, typename Hook = NoHook, bool GN = false>
__device__ __forceinline__ void gemm_epilogue16(const GemmParams& p, f32x4_t (&acc)[2 * MI][NJ], int j0, char* smem, int wave,
                                                int lane, int row0, int col0w, Hook&& hook = Hook{}) {
  float* cw = (float*)smem + wave * (32 * CW_STRIDE);
  auto stage_block = [&](auto ic) {
    constexpr int i = decltype(ic)::value;
#pragma unroll
    for (int di = 0; di < 2; ++di)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (SWAP) {
          *(f32x4_t*)(cw + (di * 16 + (lane & 15)) * CW_STRIDE + j * 16 + (lane >> 4) * 4) = acc[2 * i + di][j0 + j];
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            cw[(di * 16 + (lane >> 4) * 4 + r) * CW_STRIDE + j * 16 + (lane & 15)] = acc[2 * i + di][j0 + j][r];
        }
      }
  };
  gemm_epilogue_core<MI, EPI, decltype(stage_block)&, Hook, GN>(p, stage_block, cw, lane, row0, col0w, static_cast<Hook&&>(hook));
}

// ------------------------------------------------------------------------------------------------
// EPI_QKV: the DiT's qkv Linear with the head split fused into its epilogue (16x16x32 accumulators only).  Replaces the
// Linear output + sat's _transpose_for_scores + query/key_layernorm of AdaLNMixin.attention_fn
// (landiff/diffusion/dit_video_concat.py:636-653) -- i.e. ld_gemm_bf16 followed by ld_qkv_split mode 0 -- without the
// [M][3*heads*64] round trip through HBM.  A wave's 64 output columns are exactly one head of q, k or v:
//   q / k:  32-row blocks through the fp32 staging tile; the 8 lanes that hold a row's 64 columns do LayerNorm(64) on the
//           bf16-rounded Linear output (same operation order as ld_qkv_split_kernel) and store the 128-byte row of
//           Q / K [B][heads][Npad][64];
//   v:      the accumulators go (bias added, rounded) straight into a TRANSPOSED bf16 tile [64 d][rows] in LDS -- a lane's four
//           accumulator registers are four consecutive rows of one column, one ds_write_b64 -- and leave as 16-byte chunks
//           of V^T [B][heads][64][Npad] rows, 8 tokens each (batch boundary and M are multiples of 8 rows).
// Rows [Ntok, Npad) of Q / K / V^T are never written: the caller zero-fills those workspaces once.
// LDS: QKV_REGION bytes per wave (wave-private: only the in-order execution of a wave's own DS instructions orders it).
constexpr int QKV_REGION = 9216;       // >= 32 * CW_STRIDE * 4 (q/k staging) and 64 * (64 * 2 + 16) (v tile: 64 rows of a wave tile at a time)
template <int MI, typename Hook = NoHook>
__device__ __forceinline__ void qkv_epilogue16(const GemmParams& p, f32x4_t (&acc)[2 * MI][4], char* smem, int wave, int lane,
                                               int row0, int col0w, Hook&& hook = Hook{}) {
  if (col0w >= p.N) { hook(); return; }
  const int head = col0w >> 6;
  const int which = head / p.heads, h = head - which * p.heads;       // 0 = q, 1 = k, 2 = v
  char* reg = smem + wave * QKV_REGION;
  const int b0 = row0 / p.Ntok;
  const int bnd = (b0 + 1) * p.Ntok;           // a wave tile (<= 128 rows, Ntok >= 256) crosses at most one batch boundary
  if (which < 2) {
    float* cw = (float*)reg;
    const int sub = lane & 7, rsub = lane >> 3;
    const bf16_t* nw = which ? p.kn_w : p.qn_w;
    const bf16_t* nb = which ? p.kn_b : p.qn_b;
    bf16_t* dst = which ? p.k_out : p.q_out;
    float bias[8], wv[8], bv[8];
    {
      const u32x4_t bw = *(const u32x4_t*)(p.bias + col0w + sub * 8), ww = *(const u32x4_t*)(nw + sub * 8), nbw = *(const u32x4_t*)(nb + sub * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bias[2 * e] = bf_lo(bw[e]); bias[2 * e + 1] = bf_hi(bw[e]);
        wv[2 * e] = bf_lo(ww[e]); wv[2 * e + 1] = bf_hi(ww[e]);
        bv[2 * e] = bf_lo(nbw[e]); bv[2 * e + 1] = bf_hi(nbw[e]);
      }
    }
    hook();
    auto row_block = [&](auto ic) {
      constexpr int i = decltype(ic)::value;
#pragma unroll
      for (int di = 0; di < 2; ++di)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            cw[(di * 16 + (lane >> 4) * 4 + r) * CW_STRIDE + j * 16 + (lane & 15)] = acc[2 * i + di][j][r];
#pragma unroll
      for (int ps = 0; ps < 4; ++ps) {
        const int row = ps * 8 + rsub;
        const int gm = row0 + i * 32 + row;
        const f32x4_t lo = *(const f32x4_t*)(cw + row * CW_STRIDE + sub * 8);
        const f32x4_t hi = *(const f32x4_t*)(cw + row * CW_STRIDE + sub * 8 + 4);
        float v[8];
#pragma unroll
        for (int e = 0; e < 2; ++e) {                    // the bf16 Linear output, rounded pairwise
          const ld_f32x2_t a = rbf2((ld_f32x2_t){lo[2 * e], lo[2 * e + 1]} + (ld_f32x2_t){bias[2 * e], bias[2 * e + 1]});
          const ld_f32x2_t c = rbf2((ld_f32x2_t){hi[2 * e], hi[2 * e + 1]} + (ld_f32x2_t){bias[4 + 2 * e], bias[5 + 2 * e]});
          v[2 * e] = a[0]; v[2 * e + 1] = a[1]; v[4 + 2 * e] = c[0]; v[5 + 2 * e] = c[1];
        }
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[e];
        s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
        const float mean = s * (1.0f / 64.0f);
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[e] - mean; ss += d * d; }
        ss += __shfl_xor(ss, 1, 64); ss += __shfl_xor(ss, 2, 64); ss += __shfl_xor(ss, 4, 64);
        const float rstd = rsqrtf(ss * (1.0f / 64.0f) + p.qk_eps);
        u32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const ld_f32x2_t m2 = {mean, mean}, r2 = {rstd, rstd};
          o[e] = pack_bf16x2(((ld_f32x2_t){v[2 * e], v[2 * e + 1]} - m2) * r2 * (ld_f32x2_t){wv[2 * e], wv[2 * e + 1]} + (ld_f32x2_t){bv[2 * e], bv[2 * e + 1]});
        }
        if (gm < p.M) {
          const int b = gm >= bnd ? b0 + 1 : b0;
          const int n = gm - b * p.Ntok;
          __builtin_nontemporal_store(o, (u32x4_t*)(dst + (((long)b * p.heads + h) * p.Npad + n) * 64 + sub * 8));
        }
      }
    };
    row_block(std::integral_constant<int, 0>{});
    if constexpr (MI > 1) row_block(std::integral_constant<int, 1>{});
    if constexpr (MI > 2) row_block(std::integral_constant<int, 2>{});
    if constexpr (MI > 3) row_block(std::integral_constant<int, 3>{});
  } else {
    // (round 6) a 128-row wave tile goes through the transposed tile in two 64-row halves: 9 KB instead of 17 KB per wave, so that
    // the whole epilogue staging (8 x QKV_REGION) stays clear of K-tile buffer 0 and the persistent kernel can request the next
    // tile's first K-tile from inside this epilogue too (PREFETCH in ld_gemm8p_kernel).  Wave-private LDS: the second half's
    // stores follow the first half's loads in the wave's own DS queue, which executes in order.
    constexpr int VH = MI >= 4 ? 2 : 1;          // halves
    constexpr int MH = MI / VH;                  // 32-row blocks per half
    constexpr int ROWB = MH * 64 + 16;           // bytes per d row of the transposed tile (MH * 32 rows + pad, 16-byte aligned)
    static_assert(MI % VH == 0 && 64 * ROWB <= QKV_REGION, "v tile does not fit its LDS region");
    float bj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bj[j] = bf2f(p.bias[col0w + j * 16 + (lane & 15)]);
    hook();
#pragma unroll
    for (int vh = 0; vh < VH; ++vh) {
#pragma unroll
      for (int i = 0; i < 2 * MH; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          u32x2_t w2;
          w2[0] = pack_bf16x2(acc[vh * 2 * MH + i][j][0] + bj[j], acc[vh * 2 * MH + i][j][1] + bj[j]);
          w2[1] = pack_bf16x2(acc[vh * 2 * MH + i][j][2] + bj[j], acc[vh * 2 * MH + i][j][3] + bj[j]);
          *(u32x2_t*)(reg + (j * 16 + (lane & 15)) * ROWB + (i * 16 + (lane >> 4) * 4) * 2) = w2;
        }
      constexpr int CPR = MH * 4;                // 16-byte chunks (8 rows) per d row
#pragma unroll
      for (int it = 0; it < CPR; ++it) {         // 64 * CPR chunks, 64 per trip
        const int id = it * 64 + lane;
        const int d = id / CPR, c = id - d * CPR;
        const int gm = row0 + vh * MH * 32 + c * 8;
        const u32x4_t val = *(const u32x4_t*)(reg + d * ROWB + c * 16);
        if (gm < p.M) {
          const int b = gm >= bnd ? b0 + 1 : b0;
          const int n = gm - b * p.Ntok;
          __builtin_nontemporal_store(val, (u32x4_t*)(p.vt_out + (((long)b * p.heads + h) * 64 + d) * p.Npad + n));
        }
      }
    }
  }
}

// which specialisation a problem may use (the generic path handles everything)
inline int pick_epilogue(const GemmParams& p) {
  if (p.q_out) return EPI_QKV;
  if (p.mx_out) return EPI_GELU_MX;      // (the launcher checked: bias + GELU-tanh only, N % 32 == 0)
  const bool aligned = ((p.N & 7) == 0) && ((p.ldo & 7) == 0) && !p.out_f32 && !p.mul;
  if (!aligned) return EPI_GENERIC;
  if (p.gate && p.resid && !p.resid_f32 && p.act == 0 && (p.ldr & 7) == 0 && (!p.add2 || (p.ldadd & 7) == 0) &&
      p.rows_per_batch >= 512)
    return EPI_GATE;
  if (p.gate || p.resid || p.add2) return EPI_GENERIC;
  if (p.act == LD_ACT_GELU_TANH) return EPI_GELU;
  if (p.act == 0) return EPI_BIAS;
  return EPI_GENERIC;
}

// Two 1 KB LDS-DMA pieces of a half-tile through a raw buffer descriptor (rebuilt from its scalars at every use: loop-invariant
// SGPR values for the compiler): per-lane byte offsets o0 / o1, wave-uniform K offset `ko` in an SGPR -- no vector ALU per piece.
#ifndef LD_GEMM_ABL   // timing-only builds (WRONG results): bit 0 = no LDS-DMA in the main loop, bit 1 = fragments read once per tile,
#define LD_GEMM_ABL 0 // bit 2 = every K-tile re-reads K-tiles 0 / 1 (L2 hits), bit 3 = no vmcnt waits, bit 4 = every second LDS-DMA piece only
#endif
template <int OFF>
__device__ __forceinline__ void stage_pieces(const bf16_t* base, int bytes, char* lds, uint32_t o0, uint32_t o1, int ko) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(lds + OFF), 16, o0, ko, 0, 0);
  if (!(LD_GEMM_ABL & 16)) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(lds + OFF + 1024), 16, o1, ko, 0, 0);
}

template <int OFF>
__device__ __forceinline__ void stage_piece1(const bf16_t* base, int bytes, char* lds, uint32_t o0, int ko) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(lds + OFF), 16, o0, ko, 0, 0);
}

constexpr int LD_LDS_TOTAL = 160 * 1024;

template <auto Kernel>
int launch_kernel(const char* what, dim3 grid, dim3 block, int smem, hipStream_t stream, const GemmParams& p) {
  static thread_local LdSmemCache cache{};      // per kernel instantiation (and per host thread, per device inside)
  if (int rc = ld_ensure_dyn_smem((const void*)Kernel, (size_t)smem, &cache)) return rc;
  hipLaunchKernelGGL(Kernel, grid, block, smem, stream, p);
  return ld_check_launch(what);
}

// The runtime epilogue kind as a compile-time constant: f(std::integral_constant<int, E>{}) for E = epi when epi is one of
// ALLOWED..., for E = EPI_GENERIC otherwise.  ALLOWED is the list of specialisations a kernel family is built with -- every entry
// is a kernel instantiation (a few KB to tens of KB of code each), so the lists are per family and no longer than they need to be.
template <int... ALLOWED, typename F>
int with_epilogue(int epi, F&& f) {
  int rc = 0;
  const bool hit = ((epi == ALLOWED ? (rc = f(std::integral_constant<int, ALLOWED>{}), true) : false) || ...);
  return hit ? rc : f(std::integral_constant<int, EPI_GENERIC>{});
}

// CUs of the current device (cached per device ordinal and host thread); 256 where the runtime gives no multiple of 8
int cu_count();
// grid of a persistent launch: one workgroup per CU walking the tiles, or one per tile when there are no more tiles than CUs
inline unsigned persistent_grid(long ntiles) { const int ncu = cu_count(); return (unsigned)(ntiles > ncu ? ncu : ntiles); }

// The per-family launchers the planner (ld_gemm.hip) chooses from.  `conv`: the A operand is a zero-bordered channels-last tensor.
typedef int (*GemmLauncher)(const GemmParams& p, bool conv, hipStream_t stream);
int launch_2stage_128(const GemmParams& p, bool conv, hipStream_t stream);     // ld_gemm_2stage.hip: 128 x 128 tile, 4 waves
int launch_2stage_256(const GemmParams& p, bool conv, hipStream_t stream);     //                     256 x 256 tile, 8 waves
int launch_2stage_f8(const GemmParams& p, bool conv, hipStream_t stream);      //                     fp8 operands, 256 x 256 tile
int launch_8p(const GemmParams& p, bool conv, hipStream_t stream);             // ld_gemm_8p.hip: tiles [tile_begin, tile_end)
int launch_8p_n128(const GemmParams& p, bool conv, hipStream_t stream);        //                 the same range as 256 x 128 half tiles
#ifdef LD_VARIANTS
int launch_w4r(const GemmParams& p, bool conv, hipStream_t stream);            // ld_gemm_2stage.hip
int launch_sp(const GemmParams& p, bool conv, hipStream_t stream);             // ld_gemm_variants.hip
int launch_8p_m512(const GemmParams& p, bool conv, hipStream_t stream);
#endif
// raster group height of the persistent 256 x 256 loops for an N-column output (the planner's rule; LD_GEMM_GROUP_M overrides it)
int raster_group_m(int N);

}  // namespace ldgemm
