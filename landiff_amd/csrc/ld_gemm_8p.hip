// The 8-phase main loop on 256 x 256 tiles, persistent (ld_gemm8p_kernel), and on 256 x 128 half tiles for the partial last round
// of a launch (ld_gemm8p_n128_kernel).  ld_gemm.h: what the GEMM files share; ld_gemm.hip: which problems come here.
#include "ld_gemm.h"

namespace ldgemm {
namespace {

// ------------------------------------------------------------------------------------------------
// 8-phase main loop (round 3 default for the 256 x 256 tile; LD_GEMM_8P=0 selects the two-stage loop of ld_gemm_kernel): the
// 256x256x64 tile / 8 waves (2 x 4, 128 x 64 per wave) / 16x16x32 MFMAs of ld_gemm_kernel<256,256,2,4,...,M16> with the
// staging PIPELINED through the K loop instead of issued tile by tile:
//   * LDS = 2 K-tile buffers x 4 half-tile slots of 16 KB: A_h (h = 0, 1) holds, for BOTH wave rows wr, the 64 tile rows
//     wr * 128 + h * 64 .. + 64 (local row wr * 64 + r); B_g (g = 0, 1) holds, for ALL FOUR wave columns wc, the 32 tile
//     columns wc * 64 + g * 32 .. + 32 (local row wc * 32 + r).  Which tile row lands in which slot is free -- the LDS-DMA
//     source address is per lane -- and this choice makes every one of a K-tile's four phases read ONE half-tile of A and ONE
//     of W for the whole workgroup, so a slot is dead long before its K-tile is finished and can be re-staged early, while
//     a wave's output stays 128 contiguous rows x 64 contiguous columns (the epilogues, incl. the fused qkv head split, are
//     those of ld_gemm_kernel).
//   * a K-tile = 4 phases of 16 MFMAs (one 64 x 32 quadrant of the wave tile x K = 64):
//       ph0: read B_g0 (4 ds_read_b128) + A_h0 (8)   stage B_1(t+1)   MFMA (h0, g0)
//       ph1: read B_g1 (4)                           stage A_1(t+1)   MFMA (h0, g1)
//       ph2: read A_h1 (8)                           stage A_0(t+2)   MFMA (h1, g1)
//       ph3: --  (B_g0 fragments kept in registers)  stage B_0(t+2)   MFMA (h1, g0)   + the K-tile's only vmcnt wait
//     every slot is re-staged >= 2 phases after its last read (WAR) and its DMA has 1.5-2 K-tiles (~3000 cycles) to land;
//     the counted wait of ph3 leaves the two newest half-tiles (4 LDS-DMA instructions per wave) in flight and retires
//     K-tile t+1, which is read from the next phase on, one barrier later (RAW: own vmcnt + a barrier every wave has
//     passed).  Raw s_barrier throughout: __syncthreads() would drain vmcnt to zero.
//   * each phase is [fragment reads, stage] barrier [lgkmcnt(0), 16 MFMAs] barrier, and the two wave rows run ONE barrier
//     apart (wr = 1 takes an extra barrier up front, wr = 0 one at the end): the two waves that share a SIMD (wave w and
//     w + 4) alternate between the matrix segment and the LDS / DMA segment, so the matrix pipe always has a wave whose
//     operands are already in registers.
//   * staging goes through raw buffer descriptors: per-lane byte offsets fixed for the kernel, the K-tile / filter-tap offset
//     in an SGPR -- two buffer_load ... lds per half-tile and no vector ALU (the flat form cost two 64-bit adds per piece).
//   * PERSISTENT tiles: the grid is at most one workgroup per CU and a workgroup walks tiles blockIdx.x, + gridDim.x, ... of the
//     XCD-grouped raster.  The epilogue's LDS staging lives at the END of the 160 KB, clear of K-tile buffer 0, so the first
//     K-tile of the NEXT tile is requested before the epilogue starts (right after the epilogue's own first loads have been
//     issued: loads and LDS-DMA retire in order) and lands under it: a tile no longer pays workgroup launch, argument loads and
//     the first DMA round trip.  (Round 6: the fused-qkv epilogue too -- its V^T tile goes through LDS in two halves, 72 KB of staging.)
// Measured (tools/gemm_ab.py, profiles/r03_gemm_*): bit-identical outputs; see DESIGN.md section 4.
// ------------------------------------------------------------------------------------------------

#ifdef LD_GEMM_TRACE   // timing builds (tools/gemm_tile_trace.py): per tile of ld_gemm8p_kernel start / end of main loop / end, XCC_ID, HW_ID
__device__ unsigned long long* g_gemm_trace = nullptr;     // [0]: record counter, then 4 words per record
__device__ int g_gemm_trace_cap = 0;
#endif

template <bool CONV, int EPI>
__global__ __launch_bounds__(512, 2) void ld_gemm8p_kernel(GemmParams p) {
  constexpr int BM = 256, BN = 256;
  constexpr int SLOT = 128 * 128, KBUF = 4 * SLOT;        // 16 KB half-tile slot (128 rows x 128 B); A0 A1 B0 B1 per K-tile
  constexpr int EPI_BYTES = (EPI == EPI_QKV) ? 8 * QKV_REGION : 8 * 32 * CW_STRIDE * 4;
  constexpr int EPI_OFF = (LD_LDS_TOTAL - EPI_BYTES) & ~15;      // epilogue staging at the end of the LDS
  // K-tile buffer 0 is free while the epilogue runs.  Not for the fused-qkv epilogue, although its staging has left buffer 0 alone
  // since round 6: measured 0.745 ms with, 0.734 ms without the early request (profiles/r06_gemm_two_phase_ab.txt)
  constexpr bool PREFETCH = EPI_OFF >= KBUF && EPI != EPI_QKV;
  constexpr bool SWAPACC = EPI != EPI_QKV;                // C^T accumulator blocks: 16-byte epilogue staging stores (gemm_epilogue16<SWAP>)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  const int nbm = (p.M - p.m_begin + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  const int ntiles = nbm * nbn;
  const int gm_sz = p.group_m;
  // virtual block id v -> tile origin (XCD-contiguous logical id -> grouped raster, as ld_gemm_kernel).  gridDim.x is a
  // multiple of 8 whenever a workgroup owns more than one tile, so v % 8 == blockIdx.x % 8: a workgroup's tiles stay on its XCD.
  auto tile_origin = [&](int v, int& m0, int& n0) {
    const int bid = xcd_remap(v, ntiles);
    const int per_group = gm_sz * nbn;
    const int group = bid / per_group, in_group = bid - group * per_group;
    const int first_m = group * gm_sz;
    const int rows_here = (nbm - first_m) < gm_sz ? (nbm - first_m) : gm_sz;
    m0 = p.m_begin + (first_m + in_group % rows_here) * BM;
    n0 = (in_group / rows_here) * BN;
  };

  // ---- LDS-DMA sources: this wave stages pieces 2 * wave + {0, 1} (8 local rows x 128 B each) of every half-tile ----
  // Raw buffer descriptors (A: based at the tile's first row, rows past M read as zeros; convolution: the whole padded input,
  // rows clamped), one 32-bit byte offset per [half][piece] in VGPRs, the K-tile (or filter tap) offset in an SGPR.
  // (The descriptors are rebuilt from their scalars at every use -- loop-invariant SGPR values for the compiler; a
  //  __amdgpu_buffer_rsrc_t object captured by nested generic lambdas does not get through the host pass.)
  const auto clip = [](long v) { return (int)(v < 0x7fffffffL ? v : 0x7fffffffL); };
  struct Src { const bf16_t* a; const bf16_t* w; int a_bytes, w_bytes; };
  auto tile_src = [&](int m0, int n0) {
    Src s;
    s.a = p.A + (CONV ? 0 : (long)m0 * p.lda);
    s.w = p.W + (long)n0 * p.K;
    s.a_bytes = CONV ? 0x7fffffff : clip(((long)(p.M - m0) * p.lda) * 2);
    s.w_bytes = clip(((long)(p.N - n0) * p.K) * 2);
    return s;
  };
  uint32_t offA[2][2], offW[2][2];                        // [half][piece] byte offsets
  auto set_offsets = [&](int m0, bool weights) {          // (A offsets depend on the tile only for a convolution)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int lr = wave * 16 + i * 8 + (lane >> 3);     // local row of the slot, 0 .. 127
      const int chunk = (lane & 7) ^ ((lr >> 1) & 7);     // source-side swizzle (the read applies the same key)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int tm = (lr >> 6) * 128 + h * 64 + (lr & 63);
        if (CONV) {
          int gm = m0 + tm; gm = gm < p.M ? gm : p.M - 1;
          const int hw = p.H * p.W_;
          const int t = gm / hw, rem = gm - t * hw;
          const int hh = rem / p.W_, w = rem - hh * p.W_;
          offA[h][i] = (uint32_t)(((((long)t * p.Hp + hh) * p.Wp + w) * p.Cin + chunk * 8) * 2);
        } else {
          offA[h][i] = (uint32_t)(((long)tm * p.lda + chunk * 8) * 2);
        }
        if (weights) {
          const int tn = (lr >> 5) * 64 + h * 32 + (lr & 31);
          offW[h][i] = (uint32_t)(((long)tn * p.K + chunk * 8) * 2);
        }
      }
    }
  };
  const int nk = p.K / BK;
  const int cpt = CONV ? p.Cin / BK : 1;
  auto koff_a = [&](int kt) -> int {                      // byte offset of K-tile kt within an A row
    if (LD_GEMM_ABL & 4) kt &= 1;                         // (timing build: every K-tile re-reads K-tiles 0 / 1 -- L2 hits only)
    if (CONV) {
      const int tap = kt / cpt, c0 = (kt - tap * cpt) * BK;
      const int khw = p.kH * p.kW;
      const int dt = tap / khw, r2 = tap - dt * khw;
      const int dh = r2 / p.kW, dw = r2 - dh * p.kW;
      return (int)(((((long)dt * p.Hp + dh) * p.Wp + dw) * p.Cin + c0) * 2);
    }
    return kt * (BK * 2);
  };
  char* const my_piece = smem + wave * 2048;              // + buffer * KBUF + slot * SLOT (+ 1024 for the second piece)
  Src src;                                                // the tile being computed
  auto stage_a = [&](const Src& s, auto bufc, auto hc, int kt) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(hc)::value * SLOT;
    stage_pieces<OFF>(s.a, s.a_bytes, my_piece, offA[decltype(hc)::value][0], offA[decltype(hc)::value][1], koff_a(kt));
  };
  auto stage_w = [&](const Src& s, auto bufc, auto gc, int kt) {
    constexpr int OFF = decltype(bufc)::value * KBUF + (2 + decltype(gc)::value) * SLOT;
    stage_pieces<OFF>(s.w, s.w_bytes, my_piece, offW[decltype(gc)::value][0], offW[decltype(gc)::value][1], ((LD_GEMM_ABL & 4) ? (kt & 1) : kt) * (BK * 2));
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  auto stage_ktile0 = [&](const Src& s) {
    stage_a(s, I0{}, I0{}, 0); stage_w(s, I0{}, I0{}, 0); stage_w(s, I0{}, I1{}, 0); stage_a(s, I0{}, I1{}, 0);
  };

  // fragment reads: 16x16x32 operand = row (lane & 15), 16-byte chunk ks * 4 + (lane >> 4) of the 128-byte K row; the swizzle
  // key ((row >> 1) & 7) depends on lane & 15 only (block and wave offsets are multiples of 16 rows), so the blocks of a
  // subtile are immediate offsets (+2048 B) of one address per k-step
  int rdA[2], rdB[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int c = (ks * 4 + (lane >> 4)) ^ (((lane & 15) >> 1) & 7);
    rdA[ks] = (wr * 64 + (lane & 15)) * 128 + (c << 4);
    rdB[ks] = (wc * 32 + (lane & 15)) * 128 + (c << 4);
  }
  f32x4_t acc[8][4];
  bf16x8_t a[4][2], b0[2][2], b1[2][2];
  auto read_a = [&](auto bufc, auto hc) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(hc)::value * SLOT;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) a[i][ks] = *(const bf16x8_t*)(smem + rdA[ks] + OFF + i * 2048);
  };
  auto read_b = [&](auto bufc, auto gc, bf16x8_t (&b)[2][2]) {
    constexpr int OFF = decltype(bufc)::value * KBUF + (2 + decltype(gc)::value) * SLOT;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) b[j][ks] = *(const bf16x8_t*)(smem + rdB[ks] + OFF + j * 2048);
  };
  bool wave_live = true;                                  // (a wave whose 64 columns lie past N issues no MFMAs)
  auto bar = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  // Round 6: TWO phases of 32 MFMAs per K-tile instead of the four phases of 16 of rounds 3-5 (in git history).
  // Half the barriers and half the role switches between the two waves of a SIMD per K-tile; the same MFMAs on the same accumulators
  // in the same order -> the same bits.  Measured -2.6 % on the four DiT GEMMs (profiles/r06_gemm_two_phase_ab.txt).
  auto mma2 = [&](auto hc, auto g0c, bf16x8_t (&bA)[2][2], auto g1c, bf16x8_t (&bB)[2][2]) {
    constexpr int H = decltype(hc)::value, G0 = decltype(g0c)::value, G1 = decltype(g1c)::value;
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    if (wave_live) {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[H * 4 + i][G0 * 2 + j] = SWAPACC ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(bA[j][ks], a[i][ks], acc[H * 4 + i][G0 * 2 + j], 0, 0, 0)
                                                 : __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][ks], bA[j][ks], acc[H * 4 + i][G0 * 2 + j], 0, 0, 0);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[H * 4 + i][G1 * 2 + j] = SWAPACC ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(bB[j][ks], a[i][ks], acc[H * 4 + i][G1 * 2 + j], 0, 0, 0)
                                                 : __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][ks], bB[j][ks], acc[H * 4 + i][G1 * 2 + j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  // P0: read B_g0, B_g1, A_h0 (16 fragments); stage B_1 / A_1 of K-tile kt + 1; MFMA (h0, g0), (h0, g1)
  // P1: read A_h1 (8);                        stage A_0 / B_0 of K-tile kt + 2; MFMA (h1, g1), (h1, g0)
  // A slot is re-staged as early as ONE phase after its last read, so every wave retires its fragment reads (lgkmcnt 0) BEFORE
  // the first barrier of the reading phase: a wave that has passed the barrier ending that phase knows that every wave of both
  // rows holds its fragments in registers.
  auto ktile = [&](auto bufc, int kt) {
    constexpr int B = decltype(bufc)::value;
    using Bc = std::integral_constant<int, B>;
    using Nc = std::integral_constant<int, B ^ 1>;
    // P0.  LDS-DMA in flight on entry (oldest first): A_1(kt) [2], A_0 / B_0(kt + 1) [4]
    if (!(LD_GEMM_ABL & 2) || kt == 0) {
      read_b(Bc{}, I0{}, b0);
      read_b(Bc{}, I1{}, b1);
      __builtin_amdgcn_sched_barrier(0);
      read_a(Bc{}, I0{});
    }
    if (kt + 1 < nk) {
      if (!(LD_GEMM_ABL & 1)) { stage_w(src, Nc{}, I1{}, kt + 1); stage_a(src, Nc{}, I1{}, kt + 1); }
      if (LD_GEMM_ABL & 8) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");   // A_1(kt) has landed: read in P1, one barrier later
    } else {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    bar(); mma2(I0{}, I0{}, b0, I1{}, b1); bar();
    // P1.  In flight: A_0 / B_0(kt + 1) [4], B_1 / A_1(kt + 1) [4]
    if (!(LD_GEMM_ABL & 2)) read_a(Bc{}, I1{});
    if (kt + 2 < nk) {
      if (!(LD_GEMM_ABL & 1)) { stage_a(src, Bc{}, I0{}, kt + 2); stage_w(src, Bc{}, I0{}, kt + 2); }
      if (LD_GEMM_ABL & 8) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");   // A_0 / B_0 / B_1 of K-tile kt + 1 have landed
    } else if (kt + 1 < nk) {
      asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");   // nothing new was issued: only A_1(kt + 1) may stay in flight
    } else {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    bar(); mma2(I1{}, I1{}, b1, I0{}, b0); bar();
  };

  set_offsets(0, true);
  bool k0_staged = false;                                 // K-tile 0 of the tile about to start is already on its way
  const int v_end = p.tile_end > 0 ? p.tile_end : ntiles; // (the tiles behind it: ld_gemm8p_n128_kernel)
  for (int v = p.tile_begin + blockIdx.x; v < v_end; v += gridDim.x) {
    int m0, n0;
    tile_origin(v, m0, n0);
#ifdef LD_GEMM_TRACE
    const unsigned long long tr0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long tr1 = 0;
#endif
    src = tile_src(m0, n0);
    wave_live = n0 + wc * 64 < p.N;
    if (CONV) set_offsets(m0, false);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

    // ---- prologue: K-tile 0 complete, A_0 / B_0 of K-tile 1 in flight ----
    if (!k0_staged) stage_ktile0(src);
    if (nk > 1) {
      stage_a(src, I1{}, I0{}, 1); stage_w(src, I1{}, I0{}, 1);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    bar();
    if (wr == 1) bar();                                   // the second wave row runs one barrier behind the first

    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
      ktile(I0{}, kt);
      ktile(I1{}, kt + 1);
    }
    if (kt < nk) ktile(I0{}, kt);
    if (wr == 0) bar();
    __syncthreads();                                      // every fragment read of this tile has been waited for
#ifdef LD_GEMM_TRACE
    tr1 = __builtin_amdgcn_s_memrealtime();
#endif

    // ---- epilogue, with the next tile's first K-tile requested from inside it ----
    const int vn = v + gridDim.x;
    bool hooked = false;
    Src nsrc = src;
    k0_staged = false;
    if (PREFETCH && !CONV && vn < v_end) {                // (a convolution's next-tile A offsets would need a second register set)
      int m1, n1;
      tile_origin(vn, m1, n1);
      nsrc = tile_src(m1, n1);
      k0_staged = true;
    }
    auto hook = [&]() {
      if (!hooked && k0_staged) stage_ktile0(nsrc);
      hooked = true;
    };
    if constexpr (EPI == EPI_QKV) qkv_epilogue16<4>(p, acc, smem + EPI_OFF, wave, lane, m0 + wr * 128, n0 + wc * 64, hook);
    else gemm_epilogue16<4, EPI, 4, SWAPACC, decltype(hook)&, CONV>(p, acc, 0, smem + EPI_OFF, wave, lane, m0 + wr * 128, n0 + wc * 64, hook);
    hook();
#ifdef LD_GEMM_TRACE
    if (tid == 0 && g_gemm_trace) {
      unsigned hw, xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      const unsigned long long slot = __hip_atomic_fetch_add(g_gemm_trace, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((long long)slot < g_gemm_trace_cap) {
        unsigned long long* rec = g_gemm_trace + 1 + slot * 4;
        rec[0] = tr0; rec[1] = tr1; rec[2] = __builtin_amdgcn_s_memrealtime();
        rec[3] = ((unsigned long long)(xcc & 0xf) << 48) | ((unsigned long long)(hw & 0xffff) << 32) | (unsigned)v;
      }
    }
#endif
    if (vn < v_end) __syncthreads();                      // the staging region is free again before buffer-1 slots are re-staged
  }
}

// ------------------------------------------------------------------------------------------------
// The same 8-phase loop on 256 x 128 HALF tiles (round 5): the partial last round of a launch.  A GEMM whose 256 x 256 tiles
// do not fill whole rounds of the chip used to send its last tile ROWS to a second launch of 128 x 128 two-stage tiles: two
// workgroups per CU that share the matrix pipe, 1.4 quarter tiles per CU on average and two on the CUs that set the time -- 9 % of
// a DiT layer-call's GEMM time for 4 % of its tiles (profiles/r04_gemm_tile_trace.txt).  Here the r < 128 tiles behind the whole
// rounds (the tiles [tile_begin, ntiles) of the SAME raster, so the main launch is exactly `rounds` tiles per CU) are cut in two
// along N and run one per CU: 2 r <= 256 workgroups, one round, each half the work of a full tile.
//   * 8 waves as 4 x 2, wave tile 64 x 64 = [4][4] accumulators; per K-tile and wave 8 A + 8 W fragment reads for 32 MFMAs (the
//     2 x 4 layout of the full tile on 128 columns would need 16 + 4) -- 128 KB of LDS reads per K-tile against 1088 MFMA cycles;
//   * LDS: 2 K-tile buffers x (A_0, A_1: 16 KB = for all four wave rows wr the 32 tile rows wr * 64 + h * 32 ..; W_0, W_1: 8 KB =
//     for both wave columns wc the 32 tile columns wc * 64 + g * 32 ..) = 96 KB; a wave stages two 1 KB pieces of every A half
//     and one of every W half: 6 LDS-DMA instructions per K-tile;
//   * phases, staging order, counted vmcnt (3 = A_0 + W_0 of K-tile t + 2), the one-barrier skew between waves 0-3 and 4-7 (the
//     two waves of a SIMD), persistent loop and epilogues: those of ld_gemm8p_kernel; same dot products in the same order ->
//     the same bits as any other tiling of the GEMM.
// ------------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512, 2) void ld_gemm8p_n128_kernel(GemmParams p) {
  constexpr int BM = 256, BNF = 256;                      // the raster is the full tiles'
  constexpr int SLOT_A = 128 * 128, SLOT_B = 64 * 128, KBUF = 2 * SLOT_A + 2 * SLOT_B;     // 48 KB per K-tile: A0 A1 B0 B1
  constexpr int EPI_BYTES = (EPI == EPI_QKV) ? 8 * QKV_REGION : 8 * 32 * CW_STRIDE * 4;
  constexpr int EPI_OFF = (LD_LDS_TOTAL - EPI_BYTES) & ~15;
  constexpr bool PREFETCH = EPI_OFF >= KBUF;
  constexpr bool SWAPACC = EPI != EPI_QKV;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const bool late = wave >= 4;                            // the second wave of each SIMD runs one barrier behind the first

  const int nbm = (p.M - p.m_begin + BM - 1) / BM, nbn = (p.N + BNF - 1) / BNF;
  const int ntiles = nbm * nbn;
  const int gm_sz = p.group_m;
  auto tile_origin = [&](int v, int& m0, int& n0) {       // (ld_gemm8p_kernel's)
    const int bid = xcd_remap(v, ntiles);
    const int per_group = gm_sz * nbn;
    const int group = bid / per_group, in_group = bid - group * per_group;
    const int first_m = group * gm_sz;
    const int rows_here = (nbm - first_m) < gm_sz ? (nbm - first_m) : gm_sz;
    m0 = p.m_begin + (first_m + in_group % rows_here) * BM;
    n0 = (in_group / rows_here) * BNF;
  };
  const int v_end = p.tile_end > 0 ? p.tile_end : ntiles;
  const int nhalf = 2 * (v_end - p.tile_begin);           // work items: half u of tile tile_begin + (u >> 1)
  auto half_origin = [&](int u, int& m0, int& n0) {
    tile_origin(p.tile_begin + (u >> 1), m0, n0);
    n0 += (u & 1) * 128;
  };

  const auto clip = [](long v) { return (int)(v < 0x7fffffffL ? v : 0x7fffffffL); };
  struct Src { const bf16_t* a; const bf16_t* w; int a_bytes, w_bytes; };
  auto tile_src = [&](int m0, int n0) {
    Src s;
    s.a = p.A + (long)m0 * p.lda;
    s.w = p.W + (long)n0 * p.K;
    s.a_bytes = clip(((long)(p.M - m0) * p.lda) * 2);
    s.w_bytes = n0 < p.N ? clip(((long)(p.N - n0) * p.K) * 2) : 0;
    return s;
  };
  uint32_t offA[2][2], offW[2];                           // A: [half][piece], W: [half]
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int lr = wave * 16 + i * 8 + (lane >> 3);       // local row of an A slot, 0 .. 127
    const int chunk = (lane & 7) ^ ((lr >> 1) & 7);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int tm = (lr >> 5) * 64 + h * 32 + (lr & 31);
      offA[h][i] = (uint32_t)(((long)tm * p.lda + chunk * 8) * 2);
    }
  }
  {
    const int lr = wave * 8 + (lane >> 3);                // local row of a W slot, 0 .. 63
    const int chunk = (lane & 7) ^ ((lr >> 1) & 7);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int tn = (lr >> 5) * 64 + g * 32 + (lr & 31);
      offW[g] = (uint32_t)(((long)tn * p.K + chunk * 8) * 2);
    }
  }
  const int nk = p.K / BK;
  char* const a_piece = smem + wave * 2048;               // + buffer * KBUF + h * SLOT_A (+ 1024 for the second piece)
  char* const w_piece = smem + 2 * SLOT_A + wave * 1024;  // + buffer * KBUF + g * SLOT_B
  Src src;
  auto stage_a = [&](const Src& s, auto bufc, auto hc, int kt) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(hc)::value * SLOT_A;
    stage_pieces<OFF>(s.a, s.a_bytes, a_piece, offA[decltype(hc)::value][0], offA[decltype(hc)::value][1], kt * (BK * 2));
  };
  auto stage_w = [&](const Src& s, auto bufc, auto gc, int kt) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(gc)::value * SLOT_B;
    stage_piece1<OFF>(s.w, s.w_bytes, w_piece, offW[decltype(gc)::value], kt * (BK * 2));
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  auto stage_ktile0 = [&](const Src& s) {
    stage_a(s, I0{}, I0{}, 0); stage_w(s, I0{}, I0{}, 0); stage_w(s, I0{}, I1{}, 0); stage_a(s, I0{}, I1{}, 0);
  };

  int rdA[2], rdB[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int c = (ks * 4 + (lane >> 4)) ^ (((lane & 15) >> 1) & 7);
    rdA[ks] = (wr * 32 + (lane & 15)) * 128 + (c << 4);
    rdB[ks] = 2 * SLOT_A + (wc * 32 + (lane & 15)) * 128 + (c << 4);
  }
  f32x4_t acc[4][4];
  bf16x8_t a[2][2], b0[2][2], b1[2][2];
  auto read_a = [&](auto bufc, auto hc) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(hc)::value * SLOT_A;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) a[i][ks] = *(const bf16x8_t*)(smem + rdA[ks] + OFF + i * 2048);
  };
  auto read_b = [&](auto bufc, auto gc, bf16x8_t (&b)[2][2]) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(gc)::value * SLOT_B;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) b[j][ks] = *(const bf16x8_t*)(smem + rdB[ks] + OFF + j * 2048);
  };
  bool wave_live = true;
  auto bar = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  // two phases of 16 MFMAs per K-tile (ld_gemm8p_kernel's round-6 loop on the half tile)
  auto mma2 = [&](auto hc, auto g0c, bf16x8_t (&bA)[2][2], auto g1c, bf16x8_t (&bB)[2][2]) {
    constexpr int H = decltype(hc)::value, G0 = decltype(g0c)::value, G1 = decltype(g1c)::value;
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    if (wave_live) {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[H * 2 + i][G0 * 2 + j] = SWAPACC ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(bA[j][ks], a[i][ks], acc[H * 2 + i][G0 * 2 + j], 0, 0, 0)
                                                 : __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][ks], bA[j][ks], acc[H * 2 + i][G0 * 2 + j], 0, 0, 0);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[H * 2 + i][G1 * 2 + j] = SWAPACC ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(bB[j][ks], a[i][ks], acc[H * 2 + i][G1 * 2 + j], 0, 0, 0)
                                                 : __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][ks], bB[j][ks], acc[H * 2 + i][G1 * 2 + j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto ktile = [&](auto bufc, int kt) {      // (LDS-DMA instructions per wave: an A half = 2, a W half = 1)
    constexpr int B = decltype(bufc)::value;
    using Bc = std::integral_constant<int, B>;
    using Nc = std::integral_constant<int, B ^ 1>;
    // P0.  In flight on entry (oldest first): A_1(kt) [2], A_0 / W_0(kt + 1) [3]
    read_b(Bc{}, I0{}, b0);
    read_b(Bc{}, I1{}, b1);
    __builtin_amdgcn_sched_barrier(0);
    read_a(Bc{}, I0{});
    if (kt + 1 < nk) {
      stage_w(src, Nc{}, I1{}, kt + 1); stage_a(src, Nc{}, I1{}, kt + 1);
      asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");   // A_1(kt) has landed
    } else {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    bar(); mma2(I0{}, I0{}, b0, I1{}, b1); bar();
    // P1.  In flight: A_0 / W_0(kt + 1) [3], W_1 / A_1(kt + 1) [3]
    read_a(Bc{}, I1{});
    if (kt + 2 < nk) {
      stage_a(src, Bc{}, I0{}, kt + 2); stage_w(src, Bc{}, I0{}, kt + 2);
      asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)" ::: "memory");   // A_0 / W_0 / W_1 of K-tile kt + 1 have landed
    } else if (kt + 1 < nk) {
      asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    bar(); mma2(I1{}, I1{}, b1, I0{}, b0); bar();
  };

  bool k0_staged = false;
  for (int u = blockIdx.x; u < nhalf; u += gridDim.x) {
    int m0, n0;
    half_origin(u, m0, n0);
    const int un = u + gridDim.x;
    if (n0 >= p.N) continue;                              // the empty half of a tile in a half-wide last column (never prefetched for)
    src = tile_src(m0, n0);
    wave_live = n0 + wc * 64 < p.N;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

    if (!k0_staged) stage_ktile0(src);
    if (nk > 1) {
      stage_a(src, I1{}, I0{}, 1); stage_w(src, I1{}, I0{}, 1);
      asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    bar();
    if (late) bar();

    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
      ktile(I0{}, kt);
      ktile(I1{}, kt + 1);
    }
    if (kt < nk) ktile(I0{}, kt);
    if (!late) bar();
    __syncthreads();

    bool hooked = false;
    Src nsrc = src;
    k0_staged = false;
    if (PREFETCH && un < nhalf) {
      int m1, n1;
      half_origin(un, m1, n1);
      if (n1 < p.N) { nsrc = tile_src(m1, n1); k0_staged = true; }
    }
    auto hook = [&]() {
      if (!hooked && k0_staged) stage_ktile0(nsrc);
      hooked = true;
    };
    if constexpr (EPI == EPI_QKV) qkv_epilogue16<2>(p, acc, smem + EPI_OFF, wave, lane, m0 + wr * 64, n0 + wc * 64, hook);
    else gemm_epilogue16<2, EPI, 4, SWAPACC>(p, acc, 0, smem + EPI_OFF, wave, lane, m0 + wr * 64, n0 + wc * 64, hook);
    hook();
    if (un < nhalf) __syncthreads();
  }
}

}  // namespace

int launch_8p(const GemmParams& p, bool conv, hipStream_t stream) {
  constexpr int SMEM = LD_LDS_TOTAL;                       // 2 x 64 KB K-tile buffers; epilogue staging at the end of the 160 KB
  const int nbm = (p.M - p.m_begin + 255) / 256, nbn = (p.N + 255) / 256;
  const long ntiles = (p.tile_end > 0 ? p.tile_end : (long)nbm * nbn) - p.tile_begin;     // tiles of THIS launch
  // persistent tiles: one workgroup per CU (LD_GEMM_PERSIST=0: one workgroup per tile)
  static int k_persist = LD_KNOB_UNSET;
  dim3 grid(ld_knob("LD_GEMM_PERSIST", 1, &k_persist) ? persistent_grid(ntiles) : (unsigned)ntiles), block(512);
  auto go = [&](auto conv_c, auto e) {
    constexpr int E = decltype(e)::value;
    return launch_kernel<ld_gemm8p_kernel<decltype(conv_c)::value, E>>(E == EPI_QKV ? "ld_gemm_qkv_heads" : "ld_gemm8p", grid, block, SMEM, stream, p);
  };
  if (conv) return with_epilogue<EPI_BIAS>(pick_epilogue(p), [&](auto e) { return go(std::true_type{}, e); });
  return with_epilogue<EPI_QKV, EPI_BIAS, EPI_GELU, EPI_GATE>(pick_epilogue(p), [&](auto e) { return go(std::false_type{}, e); });
}

// the partial last round of a launch as 256 x 128 half tiles, one per workgroup (ld_gemm8p_n128_kernel)
int launch_8p_n128(const GemmParams& p, bool, hipStream_t stream) {
  const int nbm = (p.M - p.m_begin + 255) / 256, nbn = (p.N + 255) / 256;
  const int v_end = p.tile_end > 0 ? p.tile_end : nbm * nbn;
  dim3 grid((unsigned)(2 * (v_end - p.tile_begin))), block(512);
  return with_epilogue<EPI_QKV, EPI_BIAS, EPI_GELU, EPI_GATE>(pick_epilogue(p), [&](auto e) {
    constexpr int E = decltype(e)::value;
    return launch_kernel<ld_gemm8p_n128_kernel<E>>(E == EPI_QKV ? "ld_gemm_qkv_heads(half tiles)" : "ld_gemm8p_n128", grid, block, LD_LDS_TOTAL, stream, p);
  });
}

}  // namespace ldgemm

#ifdef LD_GEMM_TRACE
LD_API int ld_gemm_trace_set(void* buf, int64_t capacity_records) {
  unsigned long long* b = (unsigned long long*)buf; int cap = (int)capacity_records;
  if (hipMemcpyToSymbol(HIP_SYMBOL(ldgemm::g_gemm_trace), &b, sizeof(b)) != hipSuccess) return 1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(ldgemm::g_gemm_trace_cap), &cap, sizeof(cap)) != hipSuccess) return 1;
  return 0;
}
#endif
