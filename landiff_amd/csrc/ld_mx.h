// The MXFP8 block rule (OCP Microscaling v1.0 container: e4m3 elements + one E8M0 scale byte per 32 consecutive elements of a row,
// byte = exponent + 127), stated once for every producer: ld_quant_mxfp8_kernel, the two MXFP8-output LayerNorm kernels and the GEMM
// epilogue with MXFP8 output.  The producers promise each other equal bits (tests/test_gpu_fp8.py), and they keep it by calling this.
// In all of them a lane holds 8 consecutive elements and a block is the elements of four adjacent lanes.
#pragma once
#include "ld_common.h"

// the block's maximum from the four lanes' own; every lane of the wave executes it
__device__ __forceinline__ float mx_block_amax(float amax) {
  amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
  return fmaxf(amax, __shfl_xor(amax, 2, 64));
}

// E8M0 byte sb of a block: the smallest power of two 2^(sb - 127) >= amax / 448, clamped to [1, 254]; 0 for an all-zero block.  So no
// element saturates (the floor rule of the MX paper, 2^(floor(log2 amax) - 8), clips block maxima in [448, 512) x scale and measured
// 20-45 % more error).  inv = 2^(127 - sb), an exact power of two: |v| * inv <= 448 by construction, no clamp before the cast.
__device__ __forceinline__ int mx_scale_byte(float amax, float& inv) {
  const uint32_t tb = __float_as_uint(amax * (1.0f / 448.0f));
  int sb = (int)((tb >> 23) & 0xffu) + ((tb & 0x7fffffu) != 0u ? 1 : 0);
  sb = amax > 0.f ? (sb < 1 ? 1 : (sb > 254 ? 254 : sb)) : 0;
  inv = __uint_as_float((uint32_t)(254 - sb) << 23);
  return sb;
}

// 8 consecutive elements, scaled -> 8 e4m3 bytes
__device__ __forceinline__ u32x2_t mx_pack8(const float (&v)[8], float inv) {
  u32x2_t o;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    unsigned w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * h] * inv, v[4 * h + 1] * inv, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * h + 2] * inv, v[4 * h + 3] * inv, w, true);
    o[h] = w;
  }
  return o;
}

// where the scale byte of the block at (row, col), col % 32 == 0, lives: K-tile-major [cols / 128][lds rows][4]
__device__ __forceinline__ long mx_scale_index(long row, int col, long lds) {
  return ((long)(col >> 7) * lds + row) * 4 + ((col >> 5) & 3);
}
