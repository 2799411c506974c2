// Streaming passes of the DiT step cache (landiff_amd/dit_cache.py; DESIGN.md "DiT step cache"): the change indicator
//   Sum|cur - prev|, Sum|prev|   (+ prev <- cur in the same pass)
// and the residual bookkeeping around the transformer stack
//   out = bf16(a - b)  (+ Sum|out - old|, Sum|old| in the same pass),   out = bf16(a + r).
//
// All HBM-bound: 16-byte loads / stores (8 bf16 per lane and trip), 256 lanes per workgroup, at most LD_DC_MAX_BLOCKS
// workgroups with a grid-stride loop, 64-bit element indices, any n >= 1 (the < 8 trailing elements take a scalar loop; pointers
// that are not 16-byte aligned send every element through that loop).
//
// Sums are reproducible bit for bit, from run to run and from machine to machine: the grid is a function of n alone, a lane adds
// its trips in ascending order (the 8 elements of a trip pairwise), wave_sum's butterfly and the per-workgroup fold have a fixed
// shape, the per-workgroup partials go to `workspace` with plain stores, and a second launch of ONE workgroup adds them -- lane t
// takes partials t, t + 256, ... in ascending order, then the same fixed fold.  No float atomics anywhere.  Depth of the fp32 sum
// tree at the DiT's 68 M elements: 16 trips + 3 (pairwise) + 6 (wave) + 2 (workgroup) + 8 + 6 + 2 = 43 additions.
#include "ld_common.h"
#include "../../include/landiff_hip.h"

namespace {

constexpr int LD_DC_BLOCK = 256;
constexpr int LD_DC_MAX_BLOCKS = 2048;

inline int dc_blocks(int64_t n) {
  const int64_t per = (int64_t)LD_DC_BLOCK * 8;
  const int64_t b = (n + per - 1) / per;
  return (int)(b < 1 ? 1 : (b > LD_DC_MAX_BLOCKS ? LD_DC_MAX_BLOCKS : b));
}

inline bool dc_aligned16(const void* p) { return p == nullptr || ((uintptr_t)p & 15u) == 0; }

// pairwise sum of 8 values (depth 3)
__device__ __forceinline__ float sum8(const float* v) {
  return __fadd_rn(__fadd_rn(__fadd_rn(v[0], v[1]), __fadd_rn(v[2], v[3])), __fadd_rn(__fadd_rn(v[4], v[5]), __fadd_rn(v[6], v[7])));
}

// Folds every lane's (s0, s1) into the workgroup's pair: lane 0 returns with the totals (waves added in index order).
__device__ __forceinline__ void block_fold2(float& s0, float& s1) {
  __shared__ float red[2][LD_DC_BLOCK / 64];
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wave] = s0; red[1][wave] = s1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    s0 = red[0][0]; s1 = red[1][0];
#pragma unroll
    for (int w = 1; w < LD_DC_BLOCK / 64; ++w) { s0 = __fadd_rn(s0, red[0][w]); s1 = __fadd_rn(s1, red[1][w]); }
  }
}

// cur, prev: n bf16.  workspace[2 * block + {0, 1}] = this workgroup's Sum|cur - prev|, Sum|prev|.  update: prev <- cur.
__global__ __launch_bounds__(LD_DC_BLOCK) void ld_absdiff_partials_kernel(const bf16_t* cur, bf16_t* prev, int64_t n, int64_t nvec,
                                                                         float* workspace, int update) {
  const int64_t tid = (int64_t)blockIdx.x * LD_DC_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * LD_DC_BLOCK;
  float s0 = 0.f, s1 = 0.f;
  for (int64_t v = tid; v < nvec; v += stride) {
    const u32x4_t c = *(const u32x4_t*)(cur + v * 8);
    const u32x4_t p = *(const u32x4_t*)(prev + v * 8);
    float d[8], a[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float pl = bf_lo(p[e]), ph = bf_hi(p[e]);
      d[2 * e] = fabsf(__fsub_rn(bf_lo(c[e]), pl));
      d[2 * e + 1] = fabsf(__fsub_rn(bf_hi(c[e]), ph));
      a[2 * e] = fabsf(pl);
      a[2 * e + 1] = fabsf(ph);
    }
    s0 = __fadd_rn(s0, sum8(d));
    s1 = __fadd_rn(s1, sum8(a));
    if (update) *(u32x4_t*)(prev + v * 8) = c;
  }
  for (int64_t i = nvec * 8 + tid; i < n; i += stride) {
    const bf16_t cb = cur[i];
    const float p = bf2f(prev[i]);
    s0 = __fadd_rn(s0, fabsf(__fsub_rn(bf2f(cb), p)));
    s1 = __fadd_rn(s1, fabsf(p));
    if (update) prev[i] = cb;
  }
  block_fold2(s0, s1);
  if (threadIdx.x == 0) { workspace[2 * (int64_t)blockIdx.x] = s0; workspace[2 * (int64_t)blockIdx.x + 1] = s1; }
}

// out[0..1] = the sums of `nparts` (workgroup) pairs in workspace.  One workgroup.
__global__ __launch_bounds__(LD_DC_BLOCK) void ld_sum_partials_kernel(const float* workspace, int nparts, float* out) {
  float s0 = 0.f, s1 = 0.f;
  for (int i = threadIdx.x; i < nparts; i += LD_DC_BLOCK) {
    s0 = __fadd_rn(s0, workspace[2 * i]);
    s1 = __fadd_rn(s1, workspace[2 * i + 1]);
  }
  block_fold2(s0, s1);
  if (threadIdx.x == 0) { out[0] = s0; out[1] = s1; }
}

// out = bf16(a - b) (SUB) or bf16(a + b): one fp32 operation, one rounding.  SUMS (with SUB): old may be the buffer `out`
// replaces (each element is read by the lane that then writes it); workspace pairs = Sum|out - old|, Sum|old|, `out` as rounded.
template <bool SUB, bool SUMS>
__global__ __launch_bounds__(LD_DC_BLOCK) void ld_residual_kernel(const bf16_t* a, const bf16_t* b, bf16_t* out, int64_t n, int64_t nvec,
                                                                 const bf16_t* old, float* workspace) {
  const int64_t tid = (int64_t)blockIdx.x * LD_DC_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * LD_DC_BLOCK;
  float s0 = 0.f, s1 = 0.f;
  for (int64_t v = tid; v < nvec; v += stride) {
    const u32x4_t x = *(const u32x4_t*)(a + v * 8);
    const u32x4_t y = *(const u32x4_t*)(b + v * 8);
    u32x4_t o, r;
    if (SUMS) o = *(const u32x4_t*)(old + v * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = SUB ? __fsub_rn(bf_lo(x[e]), bf_lo(y[e])) : __fadd_rn(bf_lo(x[e]), bf_lo(y[e]));
      const float hi = SUB ? __fsub_rn(bf_hi(x[e]), bf_hi(y[e])) : __fadd_rn(bf_hi(x[e]), bf_hi(y[e]));
      r[e] = pack_bf16x2(lo, hi);
    }
    if (SUMS) {
      float d[8], m[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ol = bf_lo(o[e]), oh = bf_hi(o[e]);
        d[2 * e] = fabsf(__fsub_rn(bf_lo(r[e]), ol));
        d[2 * e + 1] = fabsf(__fsub_rn(bf_hi(r[e]), oh));
        m[2 * e] = fabsf(ol);
        m[2 * e + 1] = fabsf(oh);
      }
      s0 = __fadd_rn(s0, sum8(d));
      s1 = __fadd_rn(s1, sum8(m));
    }
    *(u32x4_t*)(out + v * 8) = r;
  }
  for (int64_t i = nvec * 8 + tid; i < n; i += stride) {
    const float x = bf2f(a[i]), y = bf2f(b[i]);
    const bf16_t r = f2bf(SUB ? __fsub_rn(x, y) : __fadd_rn(x, y));
    if (SUMS) {
      const float o = bf2f(old[i]);
      s0 = __fadd_rn(s0, fabsf(__fsub_rn(bf2f(r), o)));
      s1 = __fadd_rn(s1, fabsf(o));
    }
    out[i] = r;
  }
  if (SUMS) {
    block_fold2(s0, s1);
    if (threadIdx.x == 0) { workspace[2 * (int64_t)blockIdx.x] = s0; workspace[2 * (int64_t)blockIdx.x + 1] = s1; }
  }
}

}  // namespace

static_assert(2 * LD_DC_MAX_BLOCKS == LD_DIT_CACHE_WS_FLOATS, "workspace size of include/landiff_hip.h");

LD_API int ld_absdiff_sums(const void* cur, void* prev, int64_t n, float* out, float* workspace, int32_t update_prev, void* stream) {
  LD_REQUIRE(cur && prev && out && workspace, "ld_absdiff_sums: null pointer");
  LD_REQUIRE(n >= 1, "ld_absdiff_sums: n must be at least 1");
  LD_REQUIRE(cur != prev, "ld_absdiff_sums: cur and prev are the same buffer");
  const int64_t nvec = (dc_aligned16(cur) && dc_aligned16(prev)) ? n / 8 : 0;
  const int blocks = dc_blocks(n);
  hipLaunchKernelGGL(ld_absdiff_partials_kernel, dim3(blocks), dim3(LD_DC_BLOCK), 0, (hipStream_t)stream, (const bf16_t*)cur,
                     (bf16_t*)prev, n, nvec, workspace, (int)update_prev);
  int rc = ld_check_launch("ld_absdiff_sums");
  if (rc) return rc;
  hipLaunchKernelGGL(ld_sum_partials_kernel, dim3(1), dim3(LD_DC_BLOCK), 0, (hipStream_t)stream, workspace, blocks, out);
  return ld_check_launch("ld_absdiff_sums (fold)");
}

LD_API int ld_residual_sub(const void* a, const void* b, void* out, int64_t n, const void* old, float* out2, float* workspace,
                           void* stream) {
  LD_REQUIRE(a && b && out, "ld_residual_sub: null pointer");
  LD_REQUIRE(n >= 1, "ld_residual_sub: n must be at least 1");
  LD_REQUIRE(!old || (out2 && workspace), "ld_residual_sub: old needs out2 and workspace");
  const int64_t nvec = (dc_aligned16(a) && dc_aligned16(b) && dc_aligned16(out) && dc_aligned16(old)) ? n / 8 : 0;
  const int blocks = dc_blocks(n);
  if (!old) {
    hipLaunchKernelGGL((ld_residual_kernel<true, false>), dim3(blocks), dim3(LD_DC_BLOCK), 0, (hipStream_t)stream, (const bf16_t*)a,
                       (const bf16_t*)b, (bf16_t*)out, n, nvec, (const bf16_t*)nullptr, (float*)nullptr);
    return ld_check_launch("ld_residual_sub");
  }
  hipLaunchKernelGGL((ld_residual_kernel<true, true>), dim3(blocks), dim3(LD_DC_BLOCK), 0, (hipStream_t)stream, (const bf16_t*)a,
                     (const bf16_t*)b, (bf16_t*)out, n, nvec, (const bf16_t*)old, workspace);
  int rc = ld_check_launch("ld_residual_sub");
  if (rc) return rc;
  hipLaunchKernelGGL(ld_sum_partials_kernel, dim3(1), dim3(LD_DC_BLOCK), 0, (hipStream_t)stream, workspace, blocks, out2);
  return ld_check_launch("ld_residual_sub (fold)");
}

LD_API int ld_residual_add(const void* a, const void* r, void* out, int64_t n, void* stream) {
  LD_REQUIRE(a && r && out, "ld_residual_add: null pointer");
  LD_REQUIRE(n >= 1, "ld_residual_add: n must be at least 1");
  const int64_t nvec = (dc_aligned16(a) && dc_aligned16(r) && dc_aligned16(out)) ? n / 8 : 0;
  hipLaunchKernelGGL((ld_residual_kernel<false, false>), dim3(dc_blocks(n)), dim3(LD_DC_BLOCK), 0, (hipStream_t)stream,
                     (const bf16_t*)a, (const bf16_t*)r, (bf16_t*)out, n, nvec, (const bf16_t*)nullptr, (float*)nullptr);
  return ld_check_launch("ld_residual_add");
}
