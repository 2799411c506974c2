// GroupNorm for the channels-last VAE / upsampler activations: deterministic statistics, fused GroupNorm/SpatialNorm + swish.
//
// Replaces: Normalize/GroupNorm + nonlinearity (vq_gan_blocks.py:29-38), SpatialNorm3D.forward + nonlinearity
// (landiff/diffusion/vae_modules/cp_enc_dec.py:67-69,546-569).
//
// Pure streaming passes: 16-byte coalesced loads, fp32 / double statistics, bf16 outputs rounded at the same points the
// reference's bf16 ops round.
#include "ld_common.h"
#include "../../include/landiff_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------
// GroupNorm statistics over a channels-last tensor x [F][P][C]: per (frame-group f, group g) sum and sum of
// squares in double.  No floating-point atomics anywhere: every workgroup writes its partial pair to
// partials [F][nblk][G][2] and ld_gn_stats_reduce_kernel sums them in a fixed order, so the statistics -- and with them the
// whole VAE / upsampler decode -- are bit-identical from run to run.  Channels per group: a multiple of 8 (whole chunks per group),
// or 2 or 4 (4 or 2 groups inside a thread's 8-channel chunk, one slot each of its four); anything else is refused.
// ---------------------------------------------------------------------------------------------
constexpr int GN_ROWS_PER_BLOCK = 512;
constexpr int LD_GN_FOLD_BLOCKS = 256;          // ld_groupnorm_stats_from_conv: workgroups of the fold = double pairs per group in `partials`

__global__ __launch_bounds__(256) void ld_gn_stats_kernel(const bf16_t* x, double* partials, long P, int C, int G, int rows_per_block) {
  // Per-thread partials are combined in a FIXED order: the fp32 LDS atomics this replaced made the statistics differ by
  // ~6e-7 from run to run, which a 30-layer decoder amplifies into visible last-bit noise.
  __shared__ float part[2][256][4];   // [sum | sumsq][thread][sub-group of the thread's 8 channels]
  const int f = blockIdx.y;
  const long p0 = (long)blockIdx.x * rows_per_block;
  const int cpg = C / G;
  const int chunks_per_row = C >> 3;
  const int tid = threadIdx.x;
  // a thread owns one 8-channel chunk column and strides over rows
  const int chunk = tid % chunks_per_row;
  const int rlane = tid / chunks_per_row;
  const int rstep = 256 / chunks_per_row;
  const int nsub = cpg >= 8 ? 1 : 8 / cpg;       // groups inside one 8-channel chunk (cpg in {2,4} -> 4, 2; cpg 1 would need 8 slots: refused)
  float gs[4] = {0.f, 0.f, 0.f, 0.f}, gss[4] = {0.f, 0.f, 0.f, 0.f};
  if (rlane < rstep) {
    // Round 5: GN_U rows are requested before the first is consumed (the loop used to hold ONE 16-byte load in flight per thread:
    // 2.4 TB/s); the rows are still accumulated one after the other in row order -- the same sums, bit for bit.
    constexpr int GN_U = 8;
    const long pend = min(p0 + rows_per_block, P);
    const bf16_t* base = x + (long)f * P * C + chunk * 8;
    auto accumulate = [&](const u32x4_t a) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[2 * e] = bf_lo(a[e]); v[2 * e + 1] = bf_hi(a[e]); }
      if (cpg >= 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { gs[0] += v[e]; gss[0] += v[e] * v[e]; }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { gs[e / cpg % 4] += v[e]; gss[e / cpg % 4] += v[e] * v[e]; }
      }
    };
    long r = p0 + rlane;
    for (; r + (long)(GN_U - 1) * rstep < pend; r += (long)GN_U * rstep) {
      u32x4_t a[GN_U];
#pragma unroll
      for (int u = 0; u < GN_U; ++u) a[u] = __builtin_nontemporal_load((const u32x4_t*)(base + (r + (long)u * rstep) * C));
#pragma unroll
      for (int u = 0; u < GN_U; ++u) accumulate(a[u]);
    }
    for (; r < pend; r += rstep) accumulate(*(const u32x4_t*)(base + r * C));
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) { part[0][tid][q] = gs[q]; part[1][tid][q] = gss[q]; }
  __syncthreads();
  if (tid < G) {
    // group tid <- chunks [c0, c1), sub-slot q, all row lanes, in index order
    double s = 0.0, ss = 0.0;
    int c0, c1, q;
    if (cpg >= 8) { c0 = tid * (cpg >> 3); c1 = c0 + (cpg >> 3); q = 0; }
    else { c0 = tid / nsub; c1 = c0 + 1; q = tid % nsub; }
    for (int rl = 0; rl < rstep; ++rl)
      for (int c = c0; c < c1; ++c) {
        const int t = rl * chunks_per_row + c;
        s += (double)part[0][t][q]; ss += (double)part[1][t][q];
      }
    double* o = partials + (((long)f * gridDim.x + blockIdx.x) * G + tid) * 2;
    o[0] = s; o[1] = ss;
  }
}

// One wave per (f, g): lane l sums blocks l, l + 64, ... in index order, then a fixed butterfly.
__global__ __launch_bounds__(64) void ld_gn_stats_reduce_kernel(const double* partials, double* stats, int nblk, int G) {
  const int fg = blockIdx.x, f = fg / G, g = fg - f * G, lane = threadIdx.x;
  double s = 0.0, ss = 0.0;
  for (int b = lane; b < nblk; b += 64) {
    const double* q = partials + (((long)f * nblk + b) * G + g) * 2;
    s += q[0]; ss += q[1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); ss += __shfl_xor(ss, o, 64); }
  if (lane == 0) { stats[(long)fg * 2] = s; stats[(long)fg * 2 + 1] = ss; }
}

// The same statistics from what the producing convolution's epilogue left behind (ld_conv_cl_bf16_gn, ld_gemm.hip; the sums: gemm_epilogue_core in ld_gemm.h): fp32
// (sum, sum of squares) of every 64-row x 4-channel patch, part [U][C / 4][2].  Workgroup b folds units [b * upb, (b + 1) * upb)
// into double partials [nblk][G][2] -- thread = (row lane, quad), coalesced rows of C / 4 pairs, row lanes and quads summed in
// index order -- and ld_gn_stats_reduce_kernel finishes as above.  11 MB instead of the 708 MB activation at 8 x 480 x 720 x 128.
__global__ __launch_bounds__(256) void ld_gn_fold_partials_kernel(const float* part, double* partials, int U, int C4, int G, int upb) {
  __shared__ double sh[2][256];
  const int tid = threadIdx.x;
  const int quad = tid % C4, ul = tid / C4, ustep = 256 / C4;
  const int u1 = min((int)(blockIdx.x + 1) * upb, U);
  double s = 0.0, ss = 0.0;
  for (int u = blockIdx.x * upb + ul; u < u1; u += ustep) {
    const ld_f32x2_t v = *(const ld_f32x2_t*)(part + ((long)u * C4 + quad) * 2);
    s += (double)v[0]; ss += (double)v[1];
  }
  sh[0][tid] = s; sh[1][tid] = ss;
  __syncthreads();
  if (tid < G) {
    const int qpg = C4 / G;                                 // quads per group
    double a = 0.0, b = 0.0;
    for (int l = 0; l < ustep; ++l)
      for (int q = tid * qpg; q < (tid + 1) * qpg; ++q) { a += sh[0][l * C4 + q]; b += sh[1][l * C4 + q]; }
    double* o = partials + ((long)blockIdx.x * G + tid) * 2;
    o[0] = a; o[1] = b;
  }
}

// ---------------------------------------------------------------------------------------------
// Apply GroupNorm (+ optional SpatialNorm scale/shift from low-res zq convs) + optional swish and write the
// result into the interior of a zero-bordered channels-last buffer (the conv kernel's input layout).
//   x [F*T][H][W][C]  ->  out [F][T + tpad][H + 2*hpad][W + 2*wpad][Cout_stride]  at (t + tpad, h + hpad, w + wpad)
// ---------------------------------------------------------------------------------------------
struct GnApplyParams {
  const bf16_t* x; bf16_t* out;
  const double* stats; const bf16_t* gamma; const bf16_t* beta;
  const bf16_t* zy; const bf16_t* zb;     // [Tz][Hz][Wz][C] or null
  int F, T, H, W, C, G;
  int Tz, Hz, Wz;
  int tpad, hpad, wpad;
  int swish;
  float eps;
  double inv_count;
  int fast_rcp;          // sigmoid's reciprocal as v_rcp_f32 (1 ulp, before the bf16 rounding) instead of the IEEE division sequence
  int wshift;            // W == Wz << wshift: the nearest-neighbour zq column is a shift (-1: the general rule, a division per position)
};

// (sum, sum of squares) of (frame-group, group) pair i -> mean and rstd: the moments in double, the variance clamped at zero in fp32
__device__ __forceinline__ void gn_mean_rstd(const GnApplyParams& p, int i, float& mean_out, float& rstd_out) {
  const double mean = p.stats[2 * i] * p.inv_count;
  const double var = p.stats[2 * i + 1] * p.inv_count - mean * mean;
  mean_out = (float)mean;
  rstd_out = rsqrtf(fmaxf((float)var, 0.f) + p.eps);
}

// SpatialNorm3D's nearest frame of zq for frame t: an odd T > 1 takes the first frame alone, then (t - 1)(Tz - 1) / (T - 1)
__device__ __forceinline__ int gn_zq_frame(const GnApplyParams& p, int t) {
  if (p.T > 1 && (p.T & 1)) return (t == 0) ? 0 : 1 + (int)(((long)(t - 1) * (p.Tz - 1)) / (p.T - 1));
  return (int)(((long)t * p.Tz) / p.T);
}

__global__ __launch_bounds__(256) void ld_gn_apply_kernel(GnApplyParams p) {
  __shared__ float s_mean[512], s_rstd[512];      // per (frame-group, group)
  for (int i = threadIdx.x; i < p.F * p.G; i += 256) gn_mean_rstd(p, i, s_mean[i], s_rstd[i]);
  __syncthreads();
  const int chunks = p.C >> 3;
  const long total = (long)p.F * p.T * p.H * p.W * chunks;
  const int cpg = p.C / p.G;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int chunk = (int)(i % chunks);
    long pos = i / chunks;
    const int w = (int)(pos % p.W); pos /= p.W;
    const int h = (int)(pos % p.H); pos /= p.H;
    const int t = (int)(pos % p.T);
    const int f = (int)(pos / p.T);
    const u32x4_t a = *(const u32x4_t*)(p.x + (i / chunks) * p.C + chunk * 8);
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = bf_lo(a[e]); v[2 * e + 1] = bf_hi(a[e]); }
    const u32x4_t gw = *(const u32x4_t*)(p.gamma + chunk * 8), bw = *(const u32x4_t*)(p.beta + chunk * 8);
    float sy[8], sb[8];
    if (p.zy) {
      const int tz = gn_zq_frame(p, t);
      const int hz = (int)(((long)h * p.Hz) / p.H), wz = (int)(((long)w * p.Wz) / p.W);
      const long zo = (((long)tz * p.Hz + hz) * p.Wz + wz) * p.C + chunk * 8;
      const u32x4_t yw = *(const u32x4_t*)(p.zy + zo), zw = *(const u32x4_t*)(p.zb + zo);
#pragma unroll
      for (int e = 0; e < 4; ++e) { sy[2 * e] = bf_lo(yw[e]); sy[2 * e + 1] = bf_hi(yw[e]); sb[2 * e] = bf_lo(zw[e]); sb[2 * e + 1] = bf_hi(zw[e]); }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int g = (chunk * 8 + e) / cpg;
      const float mean = s_mean[f * p.G + g], rstd = s_rstd[f * p.G + g];
      const float gm = (e & 1) ? bf_hi(gw[e >> 1]) : bf_lo(gw[e >> 1]);
      const float bt = (e & 1) ? bf_hi(bw[e >> 1]) : bf_lo(bw[e >> 1]);
      float y = rbf((v[e] - mean) * rstd * gm + bt);      // GroupNorm output (bf16)
      if (p.zy) y = rbf(rbf(y * sy[e]) + sb[e]);                  // norm_f * conv_y(zq) + conv_b(zq)
      if (p.swish) y = rbf(y * rbf(p.fast_rcp ? __builtin_amdgcn_rcpf(1.0f + __expf(-y)) : 1.0f / (1.0f + __expf(-y))));  // x * sigmoid(x)
      v[e] = y;
    }
    const long Tp = p.T + p.tpad, Hp = p.H + 2 * p.hpad, Wp = p.W + 2 * p.wpad;
    const long o = ((((long)f * Tp + t + p.tpad) * Hp + h + p.hpad) * Wp + w + p.wpad) * p.C + chunk * 8;
    u32x4_t ow;
#pragma unroll
    for (int e = 0; e < 4; ++e) ow[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
    *(u32x4_t*)(p.out + o) = ow;
  }
}

// The same operation for channel counts whose 16-byte chunks divide the workgroup (C / 8 | 256: every VAE / upsampler
// width): one (frame-group, t, h) row of W positions per workgroup, thread -> fixed chunk, so the per-channel operands
// (gamma, beta, the group's mean / rstd) are unpacked once per thread and no index needs a division except the nearest-
// neighbour column of zq; element pairs for the bf16 roundings.  (The flat kernel above decomposes a 64-bit linear index
// per chunk and divides by the group width per element: several times the arithmetic of the normalisation itself.)
__global__ __launch_bounds__(256) void ld_gn_apply_rows_kernel(GnApplyParams p) {
  const int chunks = p.C >> 3;
  const int tid = threadIdx.x;
  const int chunk = tid % chunks, wstep = 256 / chunks;
  const int row = blockIdx.x;                         // (f, t, h)
  const int h = row % p.H, ft = row / p.H;
  const int t = ft % p.T, f = ft / p.T;
  const int cpg = p.C / p.G;
  ld_f32x2_t mean2[4], rstd2[4], gm2[4], bt2[4];
  {
    const u32x4_t gw = *(const u32x4_t*)(p.gamma + chunk * 8), bw = *(const u32x4_t*)(p.beta + chunk * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      gm2[e] = unpack_bf16x2(gw[e]); bt2[e] = unpack_bf16x2(bw[e]);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        float mean, rstd;
        gn_mean_rstd(p, f * p.G + (chunk * 8 + 2 * e + k) / cpg, mean, rstd);
        mean2[e][k] = mean; rstd2[e][k] = rstd;
      }
    }
  }
  int tz = 0, hz = 0;
  if (p.zy) {
    tz = gn_zq_frame(p, t);
    hz = (int)(((long)h * p.Hz) / p.H);
  }
  const bf16_t* xrow = p.x + (long)row * p.W * p.C + chunk * 8;
  const long Tp = p.T + p.tpad, Hp = p.H + 2 * p.hpad, Wp = p.W + 2 * p.wpad;
  bf16_t* orow = p.out + ((((long)f * Tp + t + p.tpad) * Hp + h + p.hpad) * Wp + p.wpad) * p.C + chunk * 8;
  const bf16_t* zyrow = p.zy ? p.zy + ((long)tz * p.Hz + hz) * p.Wz * p.C + chunk * 8 : nullptr;
  const bf16_t* zbrow = p.zy ? p.zb + ((long)tz * p.Hz + hz) * p.Wz * p.C + chunk * 8 : nullptr;
  // Round 5: GA_U positions per trip, all of their loads (x from HBM, the two zq rows from L2) requested before the first is
  // normalised -- the loop used to wait for one 16-byte load at a time.  Element-wise work: the same bits.
  constexpr int GA_U = 4;
  auto finish = [&](const u32x4_t a, const u32x4_t yw, const u32x4_t zw, int w) {
    u32x4_t ow;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ld_f32x2_t y = rbf2((unpack_bf16x2(a[e]) - mean2[e]) * rstd2[e] * gm2[e] + bt2[e]);      // GroupNorm output (bf16)
      if (p.zy) y = rbf2(rbf2(y * unpack_bf16x2(yw[e])) + unpack_bf16x2(zw[e]));              // norm_f * conv_y(zq) + conv_b(zq)
      if (p.swish) {                                                                                     // x * sigmoid(x)
        const ld_f32x2_t den = {1.0f + __expf(-y[0]), 1.0f + __expf(-y[1])};
        // Round 5: 1 / den as v_rcp_f32.  The IEEE division the compiler emits for `1.0f / x` is ten VALU instructions, eight times
        // per 16-byte chunk: together more than the rest of the normalisation, and enough to make this kernel VALU-bound
        // (3.8 TB/s of read + write at 480 x 720).  The quotient is rounded to bf16 right away; LD_GN_FAST_RCP=0: the division.
        const ld_f32x2_t sg = p.fast_rcp ? (ld_f32x2_t){__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])}
                                         : (ld_f32x2_t){1.0f / den[0], 1.0f / den[1]};
        y = y * rbf2(sg);
      }
      ow[e] = pack_bf16x2(y);
    }
    *(u32x4_t*)(orow + (long)w * p.C) = ow;
  };
  int w = tid / chunks;
  for (; w + (GA_U - 1) * wstep < p.W; w += GA_U * wstep) {
    u32x4_t a[GA_U], yw[GA_U], zw[GA_U];
#pragma unroll
    for (int u = 0; u < GA_U; ++u) {
      const int wu = w + u * wstep;
      a[u] = __builtin_nontemporal_load((const u32x4_t*)(xrow + (long)wu * p.C));
      yw[u] = zw[u] = (u32x4_t){0u, 0u, 0u, 0u};
      if (p.zy) {
        const int wz = p.wshift >= 0 ? (wu >> p.wshift) : (int)(((long)wu * p.Wz) / p.W);
        yw[u] = *(const u32x4_t*)(zyrow + (long)wz * p.C); zw[u] = *(const u32x4_t*)(zbrow + (long)wz * p.C);
      }
    }
#pragma unroll
    for (int u = 0; u < GA_U; ++u) finish(a[u], yw[u], zw[u], w + u * wstep);
  }
  for (; w < p.W; w += wstep) {
    const u32x4_t a = *(const u32x4_t*)(xrow + (long)w * p.C);
    u32x4_t yw = (u32x4_t){0u, 0u, 0u, 0u}, zw = yw;
    if (p.zy) {
      const int wz = p.wshift >= 0 ? (w >> p.wshift) : (int)(((long)w * p.Wz) / p.W);
      yw = *(const u32x4_t*)(zyrow + (long)wz * p.C); zw = *(const u32x4_t*)(zbrow + (long)wz * p.C);
    }
    finish(a, yw, zw, w);
  }
}

}  // namespace

LD_API int64_t ld_groupnorm_stats_blocks(int64_t P) { return (P + GN_ROWS_PER_BLOCK - 1) / GN_ROWS_PER_BLOCK; }

LD_API int ld_groupnorm_stats(const void* x, double* stats, double* partials, int64_t F, int64_t P, int64_t C, int64_t G, void* stream) {
  LD_REQUIRE(x && stats && partials, "ld_groupnorm_stats: null pointer");
  LD_REQUIRE(C % 8 == 0 && C / 8 <= 256 && G <= 64 && C % G == 0, "ld_groupnorm_stats: unsupported C=%ld G=%ld", (long)C, (long)G);
  const int cpg = (int)(C / G);
  // (cpg == 1 is 8 groups per 16-byte chunk, and a thread keeps four sub-group slots: `8 % cpg == 0` used to let it through to aliased sums)
  LD_REQUIRE(cpg % 8 == 0 || cpg == 2 || cpg == 4, "ld_groupnorm_stats: channels per group %d unsupported (a multiple of 8, or 2 or 4)", cpg);
  const int rows_per_block = GN_ROWS_PER_BLOCK;
  const int nblk = (int)ld_groupnorm_stats_blocks(P);
  dim3 grid((unsigned)nblk, (unsigned)F), block(256);
  hipLaunchKernelGGL(ld_gn_stats_kernel, grid, block, 0, (hipStream_t)stream, (const bf16_t*)x, partials, (long)P, (int)C, (int)G, rows_per_block);
  hipLaunchKernelGGL(ld_gn_stats_reduce_kernel, dim3((unsigned)(F * G)), dim3(64), 0, (hipStream_t)stream, (const double*)partials, stats, nblk, (int)G);
  return ld_check_launch("ld_groupnorm_stats");
}

LD_API int ld_groupnorm_stats_from_conv(const float* gn_partials, double* stats, double* partials, int64_t P, int64_t C, int64_t G,
                                        void* stream) {
  LD_REQUIRE(gn_partials && stats && partials, "ld_groupnorm_stats_from_conv: null pointer");
  LD_REQUIRE(P > 0 && P < (1LL << 31) && C % 4 == 0 && C / 4 <= 256 && 256 % (C / 4) == 0 && G > 0 && G <= 64 && (C / 4) % G == 0,
             "ld_groupnorm_stats_from_conv: unsupported P=%ld C=%ld G=%ld (C / 4 a power of two <= 256, whole quads per group)", (long)P,
             (long)C, (long)G);
  const int U = (int)((P + 63) / 64), C4 = (int)(C / 4);
  const int rows_at_once = 256 / C4;
  int upb = (U + LD_GN_FOLD_BLOCKS - 1) / LD_GN_FOLD_BLOCKS;                          // at most LD_GN_FOLD_BLOCKS workgroups ...
  upb = ((upb + rows_at_once - 1) / rows_at_once) * rows_at_once;                      // ... of whole trips
  const int nblk = (U + upb - 1) / upb;
  hipLaunchKernelGGL(ld_gn_fold_partials_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, gn_partials, partials, U, C4, (int)G, upb);
  hipLaunchKernelGGL(ld_gn_stats_reduce_kernel, dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream, (const double*)partials, stats, nblk, (int)G);
  return ld_check_launch("ld_groupnorm_stats_from_conv");
}

LD_API int ld_groupnorm_apply(const void* x, void* out_padded, const double* stats, const void* gamma, const void* beta,
                              const void* zy, const void* zb, int64_t F, int64_t T, int64_t H, int64_t W, int64_t C,
                              int64_t G, int64_t Tz, int64_t Hz, int64_t Wz, int64_t tpad, int64_t hpad, int64_t wpad,
                              int32_t swish, float eps, void* stream) {
  LD_REQUIRE(x && out_padded && stats && gamma && beta, "ld_groupnorm_apply: null pointer");
  LD_REQUIRE((zy == nullptr) == (zb == nullptr), "ld_groupnorm_apply: zy and zb go together");
  LD_REQUIRE(C % 8 == 0 && C % G == 0, "ld_groupnorm_apply: bad channel count");
  LD_REQUIRE(F * G <= 512, "ld_groupnorm_apply: F*G=%ld exceeds 512", (long)(F * G));
  GnApplyParams p{};
  p.x = (const bf16_t*)x; p.out = (bf16_t*)out_padded; p.stats = stats; p.gamma = (const bf16_t*)gamma; p.beta = (const bf16_t*)beta;
  p.zy = (const bf16_t*)zy; p.zb = (const bf16_t*)zb;
  p.F = (int)F; p.T = (int)T; p.H = (int)H; p.W = (int)W; p.C = (int)C; p.G = (int)G;
  p.Tz = (int)Tz; p.Hz = (int)Hz; p.Wz = (int)Wz; p.tpad = (int)tpad; p.hpad = (int)hpad; p.wpad = (int)wpad;
  p.swish = swish; p.eps = eps;
  static int k_rcp = LD_KNOB_UNSET;
  p.fast_rcp = ld_knob("LD_GN_FAST_RCP", 1, &k_rcp) != 0;
  p.wshift = -1;
  if (zy && Wz > 0 && W % Wz == 0) {
    const long r = W / Wz;
    if ((r & (r - 1)) == 0) { p.wshift = 0; while ((1L << p.wshift) < r) ++p.wshift; }
  }
  p.inv_count = 1.0 / ((double)T * H * W * (C / G));
  const long total = F * T * H * W * (C / 8);
  const long blocks = (total + 255) / 256;
  dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192)), block(256);
  static int k_rows = LD_KNOB_UNSET;       // LD_GN_ROWS=0: the flat kernel for every channel count
  if (ld_knob("LD_GN_ROWS", 1, &k_rows) != 0 && 256 % (C / 8) == 0 && F * T * H < (1l << 30))
    hipLaunchKernelGGL(ld_gn_apply_rows_kernel, dim3((unsigned)(F * T * H)), block, 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(ld_gn_apply_kernel, grid, block, 0, (hipStream_t)stream, p);
  return ld_check_launch("ld_groupnorm_apply");
}
