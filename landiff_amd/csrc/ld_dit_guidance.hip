// Final passes of the DiT's CFG branch skipping (landiff_amd/dit_guidance.py; DESIGN.md "CFG branch skipping"): unpatchify + denoiser
// scaling + CFG combine like ld_unpatchify_cfg_kernel (ld_elem.hip), in the three forms a sampler step can take.  fp32, every product
// and sum rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn), with e_u, e_c the bf16 rows of `lin`:
//   xs = x*c_skip,  d_u = e_u*c_out + xs,  d_c = e_c*c_out + xs
//   full  (ld_unpatchify_cfg_keep): D = d_c - d_u, out = fma(scale, D, d_u) -- the bits of ld_unpatchify_cfg -- and D is kept (fp32);
//                                   the same pass reduces  Sum e_u*e_c, Sum e_u^2, Sum e_c^2, Sum|D - D_old|, Sum|D_old|
//   cond  (ld_unpatchify_cond, delta null):  out = d_c
//   reuse (ld_unpatchify_cond, delta given): out = d_c + (scale - 1)*D_kept
//
// This file is built with -ffp-contract=off (build.sh): under hipcc's default contraction __fmul_rn / __fadd_rn are a plain `*` / `+`
// that the compiler may fuse, and which ones it fuses depends on the code around them.  ld_unpatchify_cfg_kernel as shipped rounds
// xs, d_u, d_c and D separately and fuses exactly its last step, out = fma(scale, D, d_u) (one v_fmac_f32); the full form below
// states that fma, so that a step with the feature on and an all-full plan is the featureless step bit for bit
// (tests/test_gpu_dit_guidance.py compares the two entry points' outputs).  Everything else here is unfused.
//
// HBM-bound passes over T*C*H*W elements (1.1 M at full size): one element per lane and trip, 256 lanes per workgroup, at most
// LD_DG_MAX_BLOCKS workgroups with a grid-stride loop, 64-bit element indices.
//
// The sums follow ld_dit_cache.hip's scheme and are reproducible bit for bit: the grid is a function of n alone, a lane adds its trips
// in ascending order, wave_sum's butterfly and the per-workgroup fold have a fixed shape, the per-workgroup partials go to `workspace`
// with plain stores, and a second launch of ONE workgroup adds them -- lane t takes partials t, t + 256, ... in ascending order, then
// the same fixed fold.  No float atomics.  Depth of the fp32 sum tree at full size: 5 trips + 6 (wave) + 2 (workgroup) + 4 + 6 + 2.
#include "ld_common.h"
#include "../../include/landiff_hip.h"

namespace {

constexpr int LD_DG_BLOCK = 256;
constexpr int LD_DG_MAX_BLOCKS = 1024;
constexpr int LD_DG_TRIPS = 4;          // elements per lane the grid is sized for, below the cap
constexpr int LD_DG_SUMS = 5;

inline int dg_blocks(int64_t n) {
  const int64_t per = (int64_t)LD_DG_BLOCK * LD_DG_TRIPS;
  const int64_t b = (n + per - 1) / per;
  return (int)(b < 1 ? 1 : (b > LD_DG_MAX_BLOCKS ? LD_DG_MAX_BLOCKS : b));
}

// Folds every lane's five sums into the workgroup's: lane 0 returns with the totals (waves added in index order).
__device__ __forceinline__ void block_fold5(float (&s)[LD_DG_SUMS]) {
  __shared__ float red[LD_DG_SUMS][LD_DG_BLOCK / 64];
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < LD_DG_SUMS; ++j) {
    s[j] = wave_sum(s[j]);
    if ((threadIdx.x & 63) == 0) red[j][wave] = s[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < LD_DG_SUMS; ++j) {
      s[j] = red[j][0];
#pragma unroll
      for (int w = 1; w < LD_DG_BLOCK / 64; ++w) s[j] = __fadd_rn(s[j], red[j][w]);
    }
  }
}

// element i of [T][C][H][W] -> its index in one batch row of lin [T*hp*wp][C*p*p]
__device__ __forceinline__ int64_t lin_index(int64_t i, int C, int H, int W, int p, int hp, int wp, int K) {
  const int ww = (int)(i % W);
  int64_t r = i / W;
  const int hh = (int)(r % H); r /= H;
  const int c = (int)(r % C);
  const int64_t t = r / C;
  const int64_t row = (t * hp + hh / p) * wp + ww / p;
  return row * K + c * p * p + (hh % p) * p + (ww % p);
}

// lin [2][T*hp*wp][C*p*p] bf16 (rows 0: uncond, 1: cond), x / out / delta / delta_old [T][C][H][W] f32.  delta_old may be delta
// (an element is read by the lane that then writes it) or null (sums 3 and 4 are then 0).
// workspace[5 * block + j] = this workgroup's sum j.
__global__ __launch_bounds__(LD_DG_BLOCK) void ld_unpatchify_cfg_keep_kernel(const bf16_t* lin, const float* x, float* out, float* delta,
                                                                            const float* delta_old, float* workspace, int T, int C,
                                                                            int H, int W, int p, float c_out, float c_skip,
                                                                            float scale) {
  const int hp = H / p, wp = W / p, K = C * p * p;
  const int64_t n_img = (int64_t)T * hp * wp;
  const int64_t total = (int64_t)T * C * H * W;
  const int64_t stride = (int64_t)gridDim.x * LD_DG_BLOCK;
  float s[LD_DG_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * LD_DG_BLOCK + threadIdx.x; i < total; i += stride) {
    const int64_t li = lin_index(i, C, H, W, p, hp, wp, K);
    const float eu = bf2f(lin[li]), ec = bf2f(lin[n_img * K + li]);
    const float xs = __fmul_rn(x[i], c_skip);
    const float du = __fadd_rn(__fmul_rn(eu, c_out), xs);
    const float dc = __fadd_rn(__fmul_rn(ec, c_out), xs);
    const float dl = __fsub_rn(dc, du);
    s[0] = __fadd_rn(s[0], __fmul_rn(eu, ec));
    s[1] = __fadd_rn(s[1], __fmul_rn(eu, eu));
    s[2] = __fadd_rn(s[2], __fmul_rn(ec, ec));
    if (delta_old) {
      const float o = delta_old[i];
      s[3] = __fadd_rn(s[3], fabsf(__fsub_rn(dl, o)));
      s[4] = __fadd_rn(s[4], fabsf(o));
    }
    delta[i] = dl;
    out[i] = __fmaf_rn(scale, dl, du);                     // (ld_unpatchify_cfg_kernel's one fused step, see the head of the file)
  }
  block_fold5(s);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < LD_DG_SUMS; ++j) workspace[LD_DG_SUMS * (int64_t)blockIdx.x + j] = s[j];
  }
}

// out[0..4] = the sums of `nparts` (workgroup) quintuples in workspace.  One workgroup.
__global__ __launch_bounds__(LD_DG_BLOCK) void ld_sum_partials5_kernel(const float* workspace, int nparts, float* out) {
  float s[LD_DG_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < nparts; i += LD_DG_BLOCK) {
#pragma unroll
    for (int j = 0; j < LD_DG_SUMS; ++j) s[j] = __fadd_rn(s[j], workspace[LD_DG_SUMS * i + j]);
  }
  block_fold5(s);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < LD_DG_SUMS; ++j) out[j] = s[j];
  }
}

// lin_cond [T*hp*wp][C*p*p] bf16 (the cond row alone).  delta null: out = d_c; else out = d_c + g * delta, g = scale - 1 from the host.
__global__ __launch_bounds__(LD_DG_BLOCK) void ld_unpatchify_cond_kernel(const bf16_t* lin, const float* x, float* out, const float* delta,
                                                                        int T, int C, int H, int W, int p, float c_out, float c_skip,
                                                                        float g) {
  const int hp = H / p, wp = W / p, K = C * p * p;
  const int64_t total = (int64_t)T * C * H * W;
  const int64_t stride = (int64_t)gridDim.x * LD_DG_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * LD_DG_BLOCK + threadIdx.x; i < total; i += stride) {
    const float ec = bf2f(lin[lin_index(i, C, H, W, p, hp, wp, K)]);
    float dc = __fadd_rn(__fmul_rn(ec, c_out), __fmul_rn(x[i], c_skip));
    if (delta) dc = __fadd_rn(dc, __fmul_rn(g, delta[i]));
    out[i] = dc;
  }
}

inline bool dg_shape_ok(int64_t T, int64_t C, int64_t H, int64_t W, int64_t p) {
  const int64_t lim = (int64_t)1 << 15;      // (the products below stay far inside 64 bits, and C*p*p inside an int)
  return T >= 1 && C >= 1 && H >= 1 && W >= 1 && p >= 1 && T < lim && C < lim && H < lim && W < lim && p < lim && H % p == 0 &&
         W % p == 0 && C * p * p < lim;
}

}  // namespace

static_assert(LD_DG_SUMS * LD_DG_MAX_BLOCKS == LD_DIT_GUIDANCE_WS_FLOATS, "workspace size of include/landiff_hip.h");

LD_API int ld_unpatchify_cfg_keep(const void* lin, const float* x, float* out, float* delta, const float* delta_old, float* sums5,
                                  float* workspace, int64_t T, int64_t C, int64_t H, int64_t W, int64_t p, float c_out, float c_skip,
                                  float scale, void* stream) {
  LD_REQUIRE(lin && x && out && delta && sums5 && workspace, "ld_unpatchify_cfg_keep: null pointer");
  LD_REQUIRE(dg_shape_ok(T, C, H, W, p), "ld_unpatchify_cfg_keep: T, C, H, W, p must be positive, with H and W multiples of p");
  const int blocks = dg_blocks(T * C * H * W);
  hipLaunchKernelGGL(ld_unpatchify_cfg_keep_kernel, dim3(blocks), dim3(LD_DG_BLOCK), 0, (hipStream_t)stream, (const bf16_t*)lin, x, out,
                     delta, delta_old, workspace, (int)T, (int)C, (int)H, (int)W, (int)p, c_out, c_skip, scale);
  int rc = ld_check_launch("ld_unpatchify_cfg_keep");
  if (rc) return rc;
  hipLaunchKernelGGL(ld_sum_partials5_kernel, dim3(1), dim3(LD_DG_BLOCK), 0, (hipStream_t)stream, workspace, blocks, sums5);
  return ld_check_launch("ld_unpatchify_cfg_keep (fold)");
}

LD_API int ld_unpatchify_cond(const void* lin_cond, const float* x, float* out, const float* delta, int64_t T, int64_t C, int64_t H,
                              int64_t W, int64_t p, float c_out, float c_skip, float scale, void* stream) {
  LD_REQUIRE(lin_cond && x && out, "ld_unpatchify_cond: null pointer");
  LD_REQUIRE(dg_shape_ok(T, C, H, W, p), "ld_unpatchify_cond: T, C, H, W, p must be positive, with H and W multiples of p");
  const float g = scale - 1.0f;          // one fp32 subtraction (exact for scale in [0.5, 2])
  hipLaunchKernelGGL(ld_unpatchify_cond_kernel, dim3(dg_blocks(T * C * H * W)), dim3(LD_DG_BLOCK), 0, (hipStream_t)stream,
                     (const bf16_t*)lin_cond, x, out, delta, (int)T, (int)C, (int)H, (int)W, (int)p, c_out, c_skip, g);
  return ld_check_launch("ld_unpatchify_cond");
}
