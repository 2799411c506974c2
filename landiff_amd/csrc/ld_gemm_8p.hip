// The 8-phase main loop on 256 x 256 tiles, persistent (ld_gemm8p_kernel), and on 256 x 128 half tiles for the partial last round
// of a launch (ld_gemm8p_n128_kernel): two instantiations of one body (gemm8p_body) on two geometries.  ld_gemm_8p_dev.h: the raster,
// tile source, addresses, counted waits, two-phase K-tile and tile walk it is built from; ld_gemm.h: what all GEMM files share;
// ld_gemm.hip: which problems come here.
#include "ld_gemm_8p_dev.h"

namespace ldgemm {
namespace {

// ------------------------------------------------------------------------------------------------
// 8-phase main loop (round 3 default for the 256 x 256 tile; LD_GEMM_8P=0 selects the two-stage loop of ld_gemm_kernel): the
// 256x256x64 tile / 8 waves (2 x 4, 128 x 64 per wave) / 16x16x32 MFMAs of ld_gemm_kernel<256,256,2,4,...,M16> with the
// staging PIPELINED through the K loop instead of issued tile by tile:
//   * LDS = 2 K-tile buffers x 4 half-tile slots of 16 KB: A_h (h = 0, 1) holds, for BOTH wave rows wr, the 64 tile rows
//     wr * 128 + h * 64 .. + 64 (local row wr * 64 + r); B_g (g = 0, 1) holds, for ALL FOUR wave columns wc, the 32 tile
//     columns wc * 64 + g * 32 .. + 32 (local row wc * 32 + r).  Which tile row lands in which slot is free -- the LDS-DMA
//     source address is per lane -- and this choice makes every phase of a K-tile read whole half-tiles of A and W for the whole
//     workgroup, so a slot is dead long before its K-tile is finished and can be re-staged early, while
//     a wave's output stays 128 contiguous rows x 64 contiguous columns (the epilogues, incl. the fused qkv head split, are
//     those of ld_gemm_kernel).
//   * a K-tile = 2 phases of 32 MFMAs (ktile_2phase; rounds 3-5: 4 phases of 16, one 64 x 32 quadrant of the wave tile each):
//     every slot is re-staged >= 1 phase after its last read (WAR) and its DMA has 1.5-2 K-tiles (~3000 cycles) to land; the counted
//     waits (StagePlan) retire what the next phase reads, one barrier before it is read.
//   * each phase is [fragment reads, stage] barrier [lgkmcnt(0), 32 MFMAs] barrier, and the two waves that share a SIMD run ONE
//     barrier apart (tile_main_loop).
//   * staging goes through raw buffer descriptors: per-lane byte offsets fixed for the kernel, the K-tile / filter-tap offset
//     in an SGPR -- two buffer_load ... lds per half-tile and no vector ALU (the flat form cost two 64-bit adds per piece).
//   * PERSISTENT tiles (walk_tiles): the grid is at most one workgroup per CU.  The epilogue's LDS staging lives at the END of the
//     160 KB, clear of K-tile buffer 0, so the first K-tile of the NEXT tile is requested from inside the epilogue.  (Round 6: the
//     fused-qkv epilogue's V^T tile goes through LDS in two halves, 72 KB of staging.)
// Measured (tools/gemm_ab.py, profiles/r03_gemm_*): bit-identical outputs; see DESIGN.md section 4.
//
// The same loop on 256 x 128 HALF tiles (round 5): the partial last round of a launch.  A GEMM whose 256 x 256 tiles
// do not fill whole rounds of the chip used to send its last tile ROWS to a second launch of 128 x 128 two-stage tiles: two
// workgroups per CU that share the matrix pipe, 1.4 quarter tiles per CU on average and two on the CUs that set the time -- 9 % of
// a DiT layer-call's GEMM time for 4 % of its tiles (profiles/r04_gemm_tile_trace.txt).  Here the r < 128 tiles behind the whole
// rounds (the tiles [tile_begin, tile_end) of the SAME raster, so the main launch is exactly `rounds` tiles per CU) are cut in two
// along N and run one per CU: 2 r <= 256 workgroups, one round, each half the work of a full tile.
//   * 8 waves as 4 x 2, wave tile 64 x 64 = [4][4] accumulators; per K-tile and wave 8 A + 8 W fragment reads for 32 MFMAs (the
//     2 x 4 layout of the full tile on 128 columns would need 16 + 4) -- 128 KB of LDS reads per K-tile against 1088 MFMA cycles;
//   * LDS: 2 K-tile buffers x (A_0, A_1: 16 KB = for all four wave rows wr the 32 tile rows wr * 64 + h * 32 ..; W_0, W_1: 8 KB =
//     for both wave columns wc the 32 tile columns wc * 64 + g * 32 ..) = 96 KB; a wave stages two 1 KB pieces of every A half
//     and one of every W half: 6 LDS-DMA instructions per K-tile;
//   * everything else is the full tile's; same dot products in the same order -> the same bits as any other tiling of the GEMM.
// ------------------------------------------------------------------------------------------------

// WN wave columns of 64 output columns each: 4 = the 256 x 256 tile (waves 2 x 4), 2 = the 256 x 128 half tile (waves 4 x 2)
template <int WN_>
struct Geo8p {
  static constexpr int WN = WN_, WM = 8 / WN;
  static constexpr int MI = 256 / WM / 32;                // 32-row blocks of a wave tile (4 / 2); a wave reads MI 16-row blocks per A half
  static constexpr int RH = MI * 16;                      // rows of one wave row in an A half-tile
  static constexpr int HALVES = 256 / (WN * 64);          // work items per tile of the 256 x 256 raster
  static constexpr int SLOT_A = WM * RH * 128, SLOT_B = WN * 32 * 128;     // 16 KB; 16 / 8 KB
  static constexpr int KBUF = 2 * SLOT_A + 2 * SLOT_B;    // A0 A1 B0 B1 per K-tile
  static constexpr int WP = SLOT_B / 8192;                // 1 KB LDS-DMA pieces per wave and W half (an A half: always 2)
  using Plan = StagePlan<2, WP>;
};

#ifdef LD_GEMM_TRACE   // timing builds (tools/gemm_tile_trace.py): per tile of ld_gemm8p_kernel start / end of main loop / end, XCC_ID, HW_ID
__device__ unsigned long long* g_gemm_trace = nullptr;     // [0]: record counter, then 4 words per record
__device__ int g_gemm_trace_cap = 0;
struct TileTrace {
  unsigned long long tr0 = 0, tr1 = 0;
  __device__ __forceinline__ void operator()(int point, int v) {
    if (point == 0) tr0 = __builtin_amdgcn_s_memrealtime();
    else if (point == 1) tr1 = __builtin_amdgcn_s_memrealtime();
    else if (threadIdx.x == 0 && g_gemm_trace) {
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
  }
};
#else
using TileTrace = NoTrace;
#endif

template <typename G, bool CONV, int EPI>
__device__ __forceinline__ void gemm8p_body(const GemmParams& p) {
  constexpr int MI = G::MI, SLOT_A = G::SLOT_A, SLOT_B = G::SLOT_B, KBUF = G::KBUF, WP = G::WP;
  using Plan = typename G::Plan;
  static_assert(!CONV || G::HALVES == 1, "convolutions run on full tiles");
  constexpr int EPI_BYTES = (EPI == EPI_QKV) ? 8 * QKV_REGION : 8 * 32 * CW_STRIDE * 4;
  constexpr int EPI_OFF = (LD_LDS_TOTAL - EPI_BYTES) & ~15;      // epilogue staging at the end of the LDS
  // K-tile buffer 0 is free while the epilogue runs.  On the full tile not for the fused-qkv epilogue, although its staging has left
  // buffer 0 alone since round 6: measured 0.745 ms with, 0.734 ms without the early request (profiles/r06_gemm_two_phase_ab.txt).
  // (A convolution's next-tile A offsets would need a second register set.)
  constexpr bool PREFETCH = EPI_OFF >= KBUF && (EPI != EPI_QKV || G::HALVES == 2) && !CONV;
  constexpr bool SWAPACC = EPI != EPI_QKV;                // C^T accumulator blocks: 16-byte epilogue staging stores (gemm_epilogue16<SWAP>)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / G::WN, wc = wave % G::WN;

  // ---- LDS-DMA sources: this wave stages 8-row pieces 2 * wave + {0, 1} of every A half-tile and WP * wave + .. of every W half-tile ----
  // one 32-bit byte offset per [half][piece] in VGPRs, the K-tile (or filter tap) offset in an SGPR
  uint32_t offA[2][2], offW[2][WP];
  auto set_offsets = [&](int m0, bool weights) {          // (A offsets depend on the tile only for a convolution)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int lr = wave * 16 + i * 8 + (lane >> 3);     // local row of the A slot, 0 .. 127
      const int chunk = swz_chunk(lane, lr);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int tm = (lr / G::RH) * (2 * G::RH) + h * G::RH + (lr % G::RH);
        if (CONV) {
          int gm = m0 + tm; gm = gm < p.M ? gm : p.M - 1;
          offA[h][i] = (uint32_t)((conv_row_elems(p, gm) + chunk * 8) * 2);
        } else {
          offA[h][i] = (uint32_t)(((long)tm * p.lda + chunk * 8) * 2);
        }
      }
    }
    if (weights) {
#pragma unroll
      for (int i = 0; i < WP; ++i) {
        const int lr = wave * (8 * WP) + i * 8 + (lane >> 3);     // local row of the W slot
        const int chunk = swz_chunk(lane, lr);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const int tn = (lr >> 5) * 64 + g * 32 + (lr & 31);
          offW[g][i] = (uint32_t)(((long)tn * p.K + chunk * 8) * 2);
        }
      }
    }
  };
  const int nk = p.K / BK;
  const int cpt = CONV ? p.Cin / BK : 1;
  auto koff_w = [&](int kt) -> int {                      // byte offset of K-tile kt within a W row
    if (LD_GEMM_ABL & 4) kt &= 1;                         // (timing build: every K-tile re-reads K-tiles 0 / 1 -- L2 hits only)
    return kt * (BK * 2);
  };
  auto koff_a = [&](int kt) -> int {                      // ... within an A row
    if (LD_GEMM_ABL & 4) kt &= 1;
    return CONV ? (int)(conv_tap_elems(p, kt, cpt) * 2) : kt * (BK * 2);
  };
  char* const a_piece = smem + wave * 2048;                           // + buffer * KBUF + h * SLOT_A (+ 1024 for the second piece)
  char* const w_piece = smem + 2 * SLOT_A + wave * (WP * 1024);       // + buffer * KBUF + g * SLOT_B
  TileSrc src;                                            // the tile being computed
  auto stage_a = [&](const TileSrc& s, auto bufc, auto hc, int kt) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(hc)::value * SLOT_A;
    stage_pieces<OFF>(s.a, s.a_bytes, a_piece, offA[decltype(hc)::value][0], offA[decltype(hc)::value][1], koff_a(kt));
  };
  auto stage_w = [&](const TileSrc& s, auto bufc, auto gc, int kt) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(gc)::value * SLOT_B;
    if constexpr (WP == 2) stage_pieces<OFF>(s.w, s.w_bytes, w_piece, offW[decltype(gc)::value][0], offW[decltype(gc)::value][1], koff_w(kt));
    else stage_piece1<OFF>(s.w, s.w_bytes, w_piece, offW[decltype(gc)::value][0], koff_w(kt));
  };
  auto stage_first = [&](const TileSrc& s, auto bufc, int kt) { stage_a(s, bufc, I0{}, kt); stage_w(s, bufc, I0{}, kt); };
  auto stage_second = [&](const TileSrc& s, auto bufc, int kt) { stage_w(s, bufc, I1{}, kt); stage_a(s, bufc, I1{}, kt); };
  auto stage_ktile0 = [&](const TileSrc& s) { stage_first(s, I0{}, 0); stage_second(s, I0{}, 0); };

  int rdA[2], rdB[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    rdA[ks] = frag_addr(wr * G::RH, lane, ks);
    rdB[ks] = 2 * SLOT_A + frag_addr(wc * 32, lane, ks);
  }
  f32x4_t acc[2 * MI][4];
  bf16x8_t a[MI][2], b0[2][2], b1[2][2];
  auto read_a = [&](auto bufc, auto hc) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(hc)::value * SLOT_A;
#pragma unroll
    for (int i = 0; i < MI; ++i)
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
  bool wave_live = true;                                  // (a wave whose 64 columns lie past N issues no MFMAs)
  auto mma1 = [&](auto hc, auto gc, bf16x8_t (&b)[2][2]) {        // the MI * 16 x 32 quadrant (h, g) of the wave tile
    constexpr int H = decltype(hc)::value, Gq = decltype(gc)::value;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[H * MI + i][Gq * 2 + j] = SWAPACC ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][ks], a[i][ks], acc[H * MI + i][Gq * 2 + j], 0, 0, 0)
                                                : __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][ks], b[j][ks], acc[H * MI + i][Gq * 2 + j], 0, 0, 0);
  };
  auto read_p0 = [&](auto bufc) {
    read_b(bufc, I0{}, b0);
    read_b(bufc, I1{}, b1);
    __builtin_amdgcn_sched_barrier(0);
    read_a(bufc, I0{});
  };
  auto read_p1 = [&](auto bufc) { read_a(bufc, I1{}); };
  auto mma_p0 = [&]() { mfma_section(wave_live, [&]() { mma1(I0{}, I0{}, b0); mma1(I0{}, I1{}, b1); }); };
  auto mma_p1 = [&]() { mfma_section(wave_live, [&]() { mma1(I1{}, I1{}, b1); mma1(I1{}, I0{}, b0); }); };
  auto ktile = [&](auto bufc, int kt, int nk) {
    ktile_2phase<Plan>(bufc, kt, nk, read_p0, read_p1, [&](auto b, int k) { stage_first(src, b, k); },
                       [&](auto b, int k) { stage_second(src, b, k); }, mma_p0, mma_p1);
  };

  set_offsets(0, true);
  walk_tiles<256, 256, G::HALVES, PREFETCH>(
      p, acc, src, [&](int m0, int n0) { return tile_src<2, CONV>(p, m0, n0); },
      [&](int m0, int n0) {
        wave_live = n0 + wc * 64 < p.N;
        if (CONV) set_offsets(m0, false);
      },
      stage_ktile0,
      [&](bool k0_staged) {
        tile_main_loop<Plan>(nk, k0_staged, wave, [&]() { stage_ktile0(src); }, [&]() { stage_first(src, I1{}, 1); }, ktile);
      },
      [&](int m0, int n0, auto& hook) {
        if constexpr (EPI == EPI_QKV) qkv_epilogue16<MI>(p, acc, smem + EPI_OFF, wave, lane, m0 + wr * (MI * 32), n0 + wc * 64, hook);
        else gemm_epilogue16<MI, EPI, 4, SWAPACC, decltype(hook), CONV>(p, acc, 0, smem + EPI_OFF, wave, lane, m0 + wr * (MI * 32), n0 + wc * 64, hook);
      },
      std::conditional_t<G::HALVES == 1, TileTrace, NoTrace>{});
}

template <bool CONV, int EPI>
__global__ __launch_bounds__(512, 2) void ld_gemm8p_kernel(GemmParams p) { gemm8p_body<Geo8p<4>, CONV, EPI>(p); }

template <int EPI>
__global__ __launch_bounds__(512, 2) void ld_gemm8p_n128_kernel(GemmParams p) { gemm8p_body<Geo8p<2>, false, EPI>(p); }

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
