// What the GEMM kernels around the 8-phase main loop state once (device code): the XCD-grouped tile raster, the LDS-DMA tile
// source, the swizzle / fragment / convolution addresses, the phase barrier and the MFMA section, the staging plan with its counted
// vmcnt waits, the two-phase K-tile, the main loop of one tile and the persistent tile walk.  ld_gemm_8p.hip (full and half
// tiles) and ld_gemm_variants.hip (512 x 128 tile, software-pipelined loop) build their kernels from it; ld_gemm_fp8.hip (MXFP8)
// takes the raster, the addresses, the MFMA section and the waits and says why it stops there; the two-stage kernels of
// ld_gemm_2stage.hip take the raster and the addresses.
#pragma once
#include "ld_gemm.h"

namespace ldgemm {

using I0 = std::integral_constant<int, 0>;
using I1 = std::integral_constant<int, 1>;
using I2 = std::integral_constant<int, 2>;
using I3 = std::integral_constant<int, 3>;

// ---- raster ----
// Virtual tile id v -> tile origin: XCD-contiguous logical id (each XCD has a private 4 MB L2) -> grouped raster: the ~64 tiles
// resident on one XCD form a group_m x (64 / group_m) patch, so an A panel and a W panel are each re-read from L2 ~8 times instead
// of W being re-streamed from MALL / HBM for every row of tiles.  The grid of a persistent launch is a multiple of 8 whenever a
// workgroup owns more than one tile, so v % 8 == blockIdx.x % 8: a workgroup's tiles stay on its XCD.
template <int BM, int BN>
__device__ __forceinline__ void tile_origin(int v, int nbm, int nbn, int group_m, int m_begin, int& m0, int& n0) {
  const int bid = xcd_remap(v, nbm * nbn);
  const int per_group = group_m * nbn;
  const int group = bid / per_group, in_group = bid - group * per_group;
  const int first_m = group * group_m;
  const int rows_here = (nbm - first_m) < group_m ? (nbm - first_m) : group_m;
  m0 = m_begin + (first_m + in_group % rows_here) * BM;
  n0 = (in_group / rows_here) * BN;
}

// ---- tile source ----
// Raw buffer descriptors of a tile's operands (A: based at the tile's first row, rows past M read as zeros; convolution: the whole
// padded input, rows clamped by the offsets; W: based at the tile's first column, nothing past N).  The descriptors are rebuilt
// from these scalars at every use -- loop-invariant SGPR values for the compiler; a __amdgpu_buffer_rsrc_t object captured by
// nested generic lambdas does not get through the host pass.
__device__ __forceinline__ int clip(long v) { return (int)(v < 0x7fffffffL ? v : 0x7fffffffL); }
struct TileSrc { const bf16_t* a; const bf16_t* w; int a_bytes, w_bytes; };
template <int ES, bool CONV>          // ES: bytes per element (lda in elements; W rows are K elements)
__device__ __forceinline__ TileSrc tile_src(const GemmParams& p, int m0, int n0) {
  TileSrc s;
  s.a = (const bf16_t*)((const char*)p.A + (CONV ? 0 : (long)m0 * p.lda * ES));
  s.w = (const bf16_t*)((const char*)p.W + (long)n0 * p.K * ES);
  s.a_bytes = CONV ? 0x7fffffff : clip(((long)(p.M - m0) * p.lda) * ES);
  s.w_bytes = n0 < p.N ? clip(((long)(p.N - n0) * p.K) * ES) : 0;      // (the second half of a half-wide last column: nothing)
  return s;
}

// ---- addresses ----
// 16-byte chunk of a staged 128-byte row that lane (lane & 7) of an 8-lane row group fetches for local row lr: the source-side
// swizzle (the fragment read applies the same key)
__device__ __forceinline__ int swz_chunk(int lane, int lr) { return (lane & 7) ^ ((lr >> 1) & 7); }
// Fragment read of a 16x16x32 operand: row (lane & 15) of the block that starts at local row row0 (a multiple of 16), 16-byte chunk
// ks * 4 + (lane >> 4) of the 128-byte K row.  The swizzle key ((row >> 1) & 7) depends on lane & 15 only, so the further blocks
// of a wave are immediate offsets (+2048 B) of this one address per k-step.
__device__ __forceinline__ int frag_addr(int row0, int lane, int ks) {
  const int c = (ks * 4 + (lane >> 4)) ^ (((lane & 15) >> 1) & 7);
  return (row0 + (lane & 15)) * 128 + (c << 4);
}
// Convolution A operand (channels-last, zero-bordered input), in elements: where output row gm = (t, h, w) starts in the padded
// input, and what K-tile kt (filter tap kt / cpt, channels (kt % cpt) * BK ..) adds to it
__device__ __forceinline__ long conv_row_elems(const GemmParams& p, int gm) {
  const int hw = p.H * p.W_;
  const int t = gm / hw, rem = gm - t * hw;
  const int hh = rem / p.W_, w = rem - hh * p.W_;
  return (((long)t * p.Hp + hh) * p.Wp + w) * p.Cin;
}
__device__ __forceinline__ long conv_tap_elems(const GemmParams& p, int kt, int cpt) {
  const int tap = kt / cpt, c0 = (kt - tap * cpt) * BK;
  const int khw = p.kH * p.kW;
  const int dt = tap / khw, r2 = tap - dt * khw;
  const int dh = r2 / p.kW, dw = r2 - dh * p.kW;
  return (((long)dt * p.Hp + dh) * p.Wp + dw) * p.Cin + c0;
}

// ---- phase barrier and MFMA section ----
// Raw s_barrier throughout the main loops: __syncthreads() would drain vmcnt to zero.
__device__ __forceinline__ void bar() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}
// The matrix segment of a phase: the fragments requested before the barrier are waited for, then the MFMAs run at raised priority
// (a wave whose 64 columns lie past N issues none).
// lgkmcnt(0) as the BUILTIN (simm16 0xC07F = vmcnt 63, expcnt 7, lgkmcnt 0): hipcc's own wait-count bookkeeping sees it.  As
// inline asm it is invisible to that pass, which then re-waits before the next phase's fragment reads on the path that
// skips the MFMAs (a pending ds_read into a register it is about to reuse) -- serialising the B and A reads of the next phase.
template <typename F>
__device__ __forceinline__ void mfma_section(bool live, F&& mfmas) {
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_sched_barrier(0);
  if (live) {
    __builtin_amdgcn_s_setprio(1);
    mfmas();
    __builtin_amdgcn_s_setprio(0);
  }
  __builtin_amdgcn_sched_barrier(0);
}

// ---- staging plan and counted waits ----
// LDS-DMA instructions per wave for one A half-tile, one W half-tile and one scale strip of a K-tile.  A K-tile is staged as its
// FIRST part A_0 / W_0 (/ S) and, one phase later, its SECOND part W_1 / A_1 -- in that order, and LDS-DMA retires in order.  Every
// wait below is the number of the newest instructions that may stay in flight:
//   prologue      issued: K-tile 0, FIRST(1)                                      K-tile 0 must have landed
//   P0(kt)        in flight on entry (oldest first): A_1(kt), FIRST(kt + 1); issued: SECOND(kt + 1)
//                                                                                 A_1(kt) must have landed: it is read in P1
//   P1(kt)        in flight: FIRST(kt + 1), W_1 / A_1(kt + 1); issued: FIRST(kt + 2)
//                                                     FIRST(kt + 1) and W_1(kt + 1) must have landed: read in P0(kt + 1)
//   P1, last but one K-tile: nothing new was issued; only A_1(kt + 1) may stay in flight
// A reader is one barrier behind the wait (RAW: own vmcnt + a barrier that every wave has passed).
template <int A, int W, int S = 0>
struct StagePlan {
  static constexpr int FIRST = A + W + S, SECOND = W + A;
  static constexpr int PROLOGUE = FIRST, P0 = FIRST + SECOND, P1 = A + FIRST, P1_TAIL = A;
};
template <typename PLAN>
constexpr bool plan_waits_are(int prologue, int p0, int p1, int p1_tail) {
  return PLAN::PROLOGUE == prologue && PLAN::P0 == p0 && PLAN::P1 == p1 && PLAN::P1_TAIL == p1_tail;
}
// the literals the three shipped kernels carried before the waits were derived: a compile proves that none moved
static_assert(plan_waits_are<StagePlan<2, 2>>(4, 8, 6, 2), "256 x 256 bf16 tile: a counted wait moved");
static_assert(plan_waits_are<StagePlan<2, 1>>(3, 6, 5, 2), "256 x 128 bf16 half tile: a counted wait moved");
static_assert(plan_waits_are<StagePlan<2, 2, 1>>(5, 9, 7, 2), "256 x 256 MXFP8 tile: a counted wait moved");

template <int N, bool LGKM0 = false>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  if constexpr (LGKM0) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
  else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- the two-phase K-tile (round 6) ----
// TWO phases of 32 MFMAs per K-tile instead of the four phases of 16 of rounds 3-5 (in git history; ld_gemm8p_m512_kernel still
// runs those): half the barriers and half the role switches between the two waves of a SIMD per K-tile; the same MFMAs on the same
// accumulators in the same order -> the same bits.  Measured -2.6 % on the four DiT GEMMs (profiles/r06_gemm_two_phase_ab.txt).
//   P0: read B_g0, B_g1, A_h0 (/ the scales);  stage SECOND = W_1 / A_1 of K-tile kt + 1;      MFMA (h0, g0), (h0, g1)
//   P1: read A_h1;                             stage FIRST = A_0 / W_0 (/ S) of K-tile kt + 2;  MFMA (h1, g1), (h1, g0)
// A slot is re-staged as early as ONE phase after its last read, so every wave retires its fragment reads (lgkmcnt 0) BEFORE
// the first barrier of the reading phase: a wave that has passed the barrier ending that phase knows that every wave of both
// rows holds its fragments in registers.
// The kernel supplies read_p0 / read_p1 (bufc), stage_first / stage_second (bufc, kt) and mma_p0 / mma_p1 (each an mfma_section).
template <typename PLAN, int B, typename R0, typename R1, typename SF, typename SS, typename M0, typename M1>
__device__ __forceinline__ void ktile_2phase(std::integral_constant<int, B>, int kt, int nk, R0&& read_p0, R1&& read_p1,
                                             SF&& stage_first, SS&& stage_second, M0&& mma_p0, M1&& mma_p1) {
  using Bc = std::integral_constant<int, B>;
  using Nc = std::integral_constant<int, B ^ 1>;
  if (!(LD_GEMM_ABL & 2) || kt == 0) read_p0(Bc{});
  if (kt + 1 < nk) {
    if (!(LD_GEMM_ABL & 1)) stage_second(Nc{}, kt + 1);
    if (LD_GEMM_ABL & 8) wait_vm<63, true>(); else wait_vm<PLAN::P0, true>();
  } else {
    wait_vm<0, true>();
  }
  bar(); mma_p0(); bar();
  if (!(LD_GEMM_ABL & 2)) read_p1(Bc{});
  if (kt + 2 < nk) {
    if (!(LD_GEMM_ABL & 1)) stage_first(Bc{}, kt + 2);
    if (LD_GEMM_ABL & 8) wait_vm<63, true>(); else wait_vm<PLAN::P1, true>();
  } else if (kt + 1 < nk) {
    wait_vm<PLAN::P1_TAIL, true>();
  } else {
    wait_vm<0, true>();
  }
  bar(); mma_p1(); bar();
}

// ---- the main loop of one tile ----
// Prologue (K-tile 0 complete -- requested here unless the previous tile's epilogue did --, FIRST of K-tile 1 in flight), the
// K-tiles in buffer pairs (compile-time buffer indices, odd tail peeled) and the closing barriers.  The two waves that share a SIMD
// (wave w and w + 4) run ONE barrier apart -- the late one takes an extra barrier up front, the early one at the end -- so that they
// alternate between the matrix segment and the LDS / DMA segment and the matrix pipe always has a wave whose operands are in
// registers.
template <typename PLAN, typename S0, typename S1, typename KT>
__device__ __forceinline__ void tile_main_loop(int nk, bool k0_staged, int wave, S0&& stage_ktile0, S1&& stage_ktile1_first, KT&& ktile) {
  const bool late = wave >= 4;
  if (!k0_staged) stage_ktile0();
  if (nk > 1) {
    stage_ktile1_first();
    wait_vm<PLAN::PROLOGUE>();
  } else {
    wait_vm<0>();
  }
  bar();
  if (late) bar();
  // (nk goes to the K-tile from here, the one value the loop tests: the K-tile's own `kt + 1 < nk` folds into the loop's)
  int kt = 0;
  for (; kt + 1 < nk; kt += 2) {
    ktile(I0{}, kt, nk);
    ktile(I1{}, kt + 1, nk);
  }
  if (kt < nk) ktile(I0{}, kt, nk);
  if (!late) bar();
  __syncthreads();                                        // every fragment read of this tile has been waited for
}

// ---- the persistent tile walk ----
// A workgroup walks the work items blockIdx.x, + gridDim.x, ... of the launch's range [p.tile_begin, p.tile_end) of the BM x BN
// raster (tile_end == 0: to the end); HALVES = 2 cuts every tile of the range in two along N, one work item each, and an empty half
// (a half-wide last column) is skipped and never prefetched for.  Per item: src = tile_src_of(m0, n0), begin_tile(m0, n0), acc = 0,
// main_loop(k0_staged), epilogue(m0, n0, hook).
// PREFETCH (the epilogue's LDS staging stays clear of K-tile buffer 0): the first K-tile of the NEXT item is requested from inside
// the epilogue by hook() -- right after the epilogue's own first loads have been issued: loads and LDS-DMA retire in order -- and
// lands under it: a tile no longer pays workgroup launch, argument loads and the first DMA round trip.
// trace(point, v): 0 = the tile starts, 1 = its main loop has ended, 2 = its epilogue has (timing builds).
struct NoTrace { __device__ __forceinline__ void operator()(int, int) const {} };
template <int BM, int BN, int HALVES, bool PREFETCH, int NI, int NJ, typename SRC, typename TS, typename BT, typename S0, typename ML,
          typename EP, typename TR = NoTrace>
__device__ __forceinline__ void walk_tiles(const GemmParams& p, f32x4_t (&acc)[NI][NJ], SRC& src, TS&& tile_src_of, BT&& begin_tile,
                                           S0&& stage_ktile0, ML&& main_loop, EP&& epilogue, TR&& trace = TR{}) {
  const int nbm = (p.M - p.m_begin + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  const int u_end = HALVES * (p.tile_end > 0 ? p.tile_end : nbm * nbn);
  auto item_origin = [&](int u, int& m0, int& n0) {       // work item u = half u % HALVES of tile u / HALVES
    tile_origin<BM, BN>(u / HALVES, nbm, nbn, p.group_m, p.m_begin, m0, n0);
    if constexpr (HALVES > 1) n0 += (u % HALVES) * (BN / HALVES);
  };
  bool k0_staged = false;                                 // K-tile 0 of the item about to start is already on its way
  for (int u = HALVES * p.tile_begin + blockIdx.x; u < u_end; u += gridDim.x) {
    int m0, n0;
    item_origin(u, m0, n0);
    if constexpr (HALVES > 1) if (n0 >= p.N) continue;
    trace(0, u / HALVES);
    src = tile_src_of(m0, n0);
    begin_tile(m0, n0);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
    main_loop(k0_staged);
    trace(1, u / HALVES);

    // ---- epilogue, with the next item's first K-tile requested from inside it ----
    const int un = u + gridDim.x;
    bool hooked = false;
    SRC nsrc = src;
    k0_staged = false;
    if (PREFETCH && un < u_end) {
      int m1, n1;
      item_origin(un, m1, n1);
      if (HALVES == 1 || n1 < p.N) { nsrc = tile_src_of(m1, n1); k0_staged = true; }
    }
    auto hook = [&]() {
      if (!hooked && k0_staged) stage_ktile0(nsrc);
      hooked = true;
    };
    epilogue(m0, n0, hook);
    hook();
    trace(2, u / HALVES);
    if (un < u_end) __syncthreads();                     // the epilogue's staging region is free again before it is re-staged
  }
}

}  // namespace ldgemm
