// Measured alternatives to the shipped GEMM main loops, built into the variants library only (build.sh: VARIANT_ONLY): the 8-phase
// loop on 512 x 128 tiles (LD_GEMM_M512=1) and the software-pipelined loop (LD_GEMM_SP=1); the register-staged round-1 loop
// (LD_GEMM_TILE=11) sits beside the two-stage kernels in ld_gemm_2stage.hip.  Bit-identical to the shipped routes and measured slower
// or no faster; tests/test_gpu_variants.py runs them.  Both keep their own K-tile inside the shared tile walk of ld_gemm_8p_dev.h, which
// gives them the raster, the tile source, the addresses and the launch's tile range.
#include "ld_gemm_8p_dev.h"

namespace ldgemm {
namespace {

// ------------------------------------------------------------------------------------------------
// The 8-phase loop on a 512 x 128 tile (round 5): outputs 128 columns wide (the VAE's Cout = 128 level at 480 x 720: 40 % of its
// convolution time).  On the 256 x 256 tile such an output leaves the wave columns 2 and 3 -- two of the four SIMDs -- without
// work; the 128 x 128 two-stage kernel they ran on instead reaches ~1085 TFLOP/s where the 8-phase loop reaches ~1250.  Here the
// eight waves form 4 wave ROWS x 2 wave columns with the SAME wave tile as ld_gemm8p_kernel (128 x 64, [8][4] accumulators, 16
// MFMAs per phase) and the same phase schedule, barriers and one-barrier skew between the two waves of a SIMD; what changes is the
// LDS plan: an A half-tile is 4 x 64 rows (32 KB, four 1 KB LDS-DMA pieces per wave), a W half-tile 2 x 32 columns (8 KB, one
// piece per wave), a K-tile 80 KB, two of them the whole 160 KB -- so the epilogue staging reuses K-tile buffer 0 behind the
// barrier that ends the main loop, and a persistent workgroup does not prefetch its next tile's first K-tile (the convolution
// form of ld_gemm8p_kernel does not either).  The K-tile keeps the FOUR phases of 16 MFMAs of rounds 3-5 (the numbers below were
// measured on that schedule):
//       ph0: read B_g0 + A_h0   stage B_1(t+1)   MFMA (h0, g0)        ph2: read A_h1   stage A_0(t+2)   MFMA (h1, g1)
//       ph1: read B_g1          stage A_1(t+1)   MFMA (h0, g1)        ph3: --          stage B_0(t+2)   MFMA (h1, g0) + the only vmcnt wait
// The counted wait of ph3 leaves the FIRST part of K-tile t + 2 (4 + 1 pieces) in flight.  Same dot products in the
// same order as the other two conv routes: bit-identical outputs.
// MEASURED (profiles/r05_vae_conv_route_ab.txt): alone in a loop 2.37 -> 2.16 ms per 8-frame launch (1135 vs 1031 TFLOP/s); inside
// the VAE decode, same box, arms alternated: 337.4 / 336.7 ms per video against 337.4 / 335.7 -- no gain (in context the 128 x 128
// tiles already run at ~1085) -- so it is a measured alternative of the VARIANTS build (LD_GEMM_M512=1 there), not a shipped route.
// (For the DiT GEMMs' half-empty last tile column it would not pay at the headline shape: DESIGN.md section 9.)
// ------------------------------------------------------------------------------------------------
template <bool CONV, int EPI>
__global__ __launch_bounds__(512, 2) void ld_gemm8p_m512_kernel(GemmParams p) {
  static_assert(EPI != EPI_QKV, "the fused qkv split is not built for the 512 x 128 tile");
  constexpr int BM = 512, BN = 128;
  constexpr int ASLOT = 256 * 128, BSLOT = 64 * 128;      // A half-tile: 4 wave rows x 64 rows (32 KB); W half-tile: 2 wave columns x 32 (8 KB)
  constexpr int KBUF = 2 * ASLOT + 2 * BSLOT;             // A0 A1 B0 B1 per K-tile = 80 KB; two buffers = all 160 KB
  static_assert(2 * KBUF == LD_LDS_TOTAL && 8 * 32 * CW_STRIDE * 4 <= KBUF, "LDS plan");
  constexpr int EPI_OFF = 0;                              // the epilogue staging reuses K-tile buffer 0 (entered behind a workgroup barrier)
  constexpr bool SWAPACC = true;                          // C^T accumulator blocks: 16-byte epilogue staging stores (gemm_epilogue16<SWAP>)
  using Plan = StagePlan<4, 1>;                           // LDS-DMA instructions per wave: an A half = 4, a W half = 1
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wq = wave & 3;                // waves w and w + 4 share a SIMD: they differ in wr only
  const int wrow = (wq >> 1) * 2 + wr, wc = wq & 1;       // wave row 0..3 (128 tile rows each), wave column 0..1 (64 columns each)

  // ---- LDS-DMA sources: this wave stages pieces 4 * wave + {0 .. 3} (8 local rows x 128 B each) of every A half-tile and piece
  // `wave` of every W half-tile ----
  uint32_t offA[2][4], offW[2];                           // [half][piece] byte offsets: four A pieces and one W piece per half-tile and wave
  auto set_offsets = [&](int m0, bool weights) {          // (A offsets depend on the tile only for a convolution)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lr = wave * 32 + i * 8 + (lane >> 3);     // local row of the A slot, 0 .. 255
      const int chunk = swz_chunk(lane, lr);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int tm = (lr >> 6) * 128 + h * 64 + (lr & 63);
        if (CONV) {
          int gm = m0 + tm; gm = gm < p.M ? gm : p.M - 1;
          offA[h][i] = (uint32_t)((conv_row_elems(p, gm) + chunk * 8) * 2);
        } else {
          offA[h][i] = (uint32_t)(((long)tm * p.lda + chunk * 8) * 2);
        }
      }
    }
    if (weights) {
      const int lr = wave * 8 + (lane >> 3);              // local row of the W slot, 0 .. 63
      const int chunk = swz_chunk(lane, lr);
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int tn = (lr >> 5) * 64 + g * 32 + (lr & 31);
        offW[g] = (uint32_t)(((long)tn * p.K + chunk * 8) * 2);
      }
    }
  };
  const int nk = p.K / BK;
  const int cpt = CONV ? p.Cin / BK : 1;
  auto koff_a = [&](int kt) -> int {                      // byte offset of K-tile kt within an A row
    return CONV ? (int)(conv_tap_elems(p, kt, cpt) * 2) : kt * (BK * 2);
  };
  char* const my_a = smem + wave * 4096;                  // + buffer * KBUF + half * ASLOT (+ 1024 per further piece)
  char* const my_w = smem + 2 * ASLOT + wave * 1024;      // + buffer * KBUF + half * BSLOT
  TileSrc src;                                            // the tile being computed
  auto stage_a = [&](const TileSrc& s, auto bufc, auto hc, int kt) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(hc)::value * ASLOT;
    const int ko = koff_a(kt);
    stage_pieces<OFF>(s.a, s.a_bytes, my_a, offA[decltype(hc)::value][0], offA[decltype(hc)::value][1], ko);
    stage_pieces<OFF + 2048>(s.a, s.a_bytes, my_a, offA[decltype(hc)::value][2], offA[decltype(hc)::value][3], ko);
  };
  auto stage_w = [&](const TileSrc& s, auto bufc, auto gc, int kt) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(gc)::value * BSLOT;
    stage_piece1<OFF>(s.w, s.w_bytes, my_w, offW[decltype(gc)::value], kt * (BK * 2));
  };
  auto stage_ktile0 = [&](const TileSrc& s) {
    stage_a(s, I0{}, I0{}, 0); stage_w(s, I0{}, I0{}, 0); stage_w(s, I0{}, I1{}, 0); stage_a(s, I0{}, I1{}, 0);
  };

  int rdA[2], rdB[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    rdA[ks] = frag_addr(wrow * 64, lane, ks);
    rdB[ks] = 2 * ASLOT + frag_addr(wc * 32, lane, ks);
  }
  f32x4_t acc[8][4];
  bf16x8_t a[4][2], b0[2][2], b1[2][2];
  auto read_a = [&](auto bufc, auto hc) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(hc)::value * ASLOT;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) a[i][ks] = *(const bf16x8_t*)(smem + rdA[ks] + OFF + i * 2048);
  };
  auto read_b = [&](auto bufc, auto gc, bf16x8_t (&b)[2][2]) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(gc)::value * BSLOT;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) b[j][ks] = *(const bf16x8_t*)(smem + rdB[ks] + OFF + j * 2048);
  };
  bool wave_live = true;                                  // (a wave whose 64 columns lie past N issues no MFMAs)
  auto mma = [&](auto hc, auto gc, bf16x8_t (&b)[2][2]) {
    constexpr int H = decltype(hc)::value, G = decltype(gc)::value;
    mfma_section(wave_live, [&]() {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[H * 4 + i][G * 2 + j] = SWAPACC ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][ks], a[i][ks], acc[H * 4 + i][G * 2 + j], 0, 0, 0)
                                                : __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][ks], b[j][ks], acc[H * 4 + i][G * 2 + j], 0, 0, 0);
    });
  };
  auto ktile = [&](auto bufc, int kt, int nk) {
    constexpr int B = decltype(bufc)::value;
    using Bc = std::integral_constant<int, B>;
    using Nc = std::integral_constant<int, B ^ 1>;
    // ph0
    read_b(Bc{}, I0{}, b0);
    __builtin_amdgcn_sched_barrier(0);
    read_a(Bc{}, I0{});
    if (kt + 1 < nk) stage_w(src, Nc{}, I1{}, kt + 1);
    bar(); mma(I0{}, I0{}, b0); bar();
    // ph1
    read_b(Bc{}, I1{}, b1);
    if (kt + 1 < nk) stage_a(src, Nc{}, I1{}, kt + 1);
    bar(); mma(I0{}, I1{}, b1); bar();
    // ph2
    read_a(Bc{}, I1{});
    if (kt + 2 < nk) stage_a(src, Bc{}, I0{}, kt + 2);
    bar(); mma(I1{}, I1{}, b1); bar();
    // ph3
    if (kt + 2 < nk) {
      stage_w(src, Bc{}, I0{}, kt + 2);
      wait_vm<Plan::FIRST>();                             // K-tile kt + 1 has landed; A_0 (4 pieces) / B_0 (1) of kt + 2 stay in flight
    } else {
      wait_vm<0>();
    }
    bar(); mma(I1{}, I0{}, b0); bar();
  };

  set_offsets(0, true);
  // (no prefetch of the next tile's first K-tile: the epilogue staging lives in buffer 0)
  walk_tiles<BM, BN, 1, false>(
      p, acc, src, [&](int m0, int n0) { return tile_src<2, CONV>(p, m0, n0); },
      [&](int m0, int n0) {
        wave_live = n0 + wc * 64 < p.N;
        if (CONV) set_offsets(m0, false);
      },
      stage_ktile0,
      [&](bool k0_staged) {
        tile_main_loop<Plan>(nk, k0_staged, wave, [&]() { stage_ktile0(src); },
                             [&]() { stage_a(src, I1{}, I0{}, 1); stage_w(src, I1{}, I0{}, 1); }, ktile);
      },
      [&](int m0, int n0, auto& hook) {
        gemm_epilogue16<4, EPI, 4, SWAPACC, decltype(hook), CONV>(p, acc, 0, smem + EPI_OFF, wave, lane, m0 + wrow * 128, n0 + wc * 64, hook);
      });
}

// ------------------------------------------------------------------------------------------------
// Software-pipelined main loop (round 4; LD_GEMM_SP=1): the 256 x 256 x 64 tile / 8 waves (2 x 4, 128 x 64 per wave) /
// 16x16x32 MFMAs of ld_gemm8p_kernel, but every wave pipelines ITS OWN fragment reads under its own MFMAs and the workgroup
// meets ONCE per K-tile instead of eight times:
//   * a K-tile = 4 stages of 16 MFMAs (k-step ks x row half of the wave tile); while a stage's MFMAs issue, the wave's
//     ds_read_b128 for the NEXT stage go out in between them into a second fragment register set (two A sets + two W sets of
//     4 fragments = 64 registers next to the 128 accumulators);
//       S0 (ks 0, rows 0-63):   reads A rows 64-127 ks 0
//       S1 (ks 0, rows 64-127): reads A rows 0-63 ks 1 and W ks 1
//       S2 (ks 1, rows 0-63):   reads A rows 64-127 ks 1               -- the wave's last reads of this K-tile
//       [lgkmcnt(0), vmcnt(0): K-tile t+1 has landed; s_barrier: every wave is done reading K-tile t]
//       S3 (ks 1, rows 64-127): issues the 8 LDS-DMA pieces of K-tile t+2 into the buffer just freed and reads A rows 0-63 / W
//                               ks 0 of K-tile t+1 from the other buffer
//   * LDS: two K-tile buffers of 64 KB (A tile 256 rows x 128 B | W tile 256 rows x 128 B, chunk index XOR ((row >> 1) & 7) on
//     the DMA source and on the read); a wave stages pieces 4 w .. 4 w + 3 (8 rows each) of both tiles: one per-lane byte
//     offset per piece parity, the rest of the address in the SGPR offset.
//   * persistent tiles, epilogues and the next tile's first K-tile requested from inside the epilogue: as ld_gemm8p_kernel.
// The matrix pipe no longer waits for a partner wave to get through a load segment and seven of the eight barriers per K-tile
// are gone; what a DMA has to land in is one K-tile (~2300 cycles) instead of 1.5-2.
// ------------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512, 2) void ld_gemm_sp_kernel(GemmParams p) {
  constexpr int BM = 256, BN = 256;
  constexpr int TILE = 256 * 128, KBUF = 2 * TILE;        // A tile | W tile per K-tile buffer
  constexpr int EPI_BYTES = (EPI == EPI_QKV) ? 8 * QKV_REGION : 8 * 32 * CW_STRIDE * 4;
  constexpr int EPI_OFF = (LD_LDS_TOTAL - EPI_BYTES) & ~15;
  constexpr bool PREFETCH = EPI_OFF >= KBUF;
  constexpr bool SWAPACC = EPI != EPI_QKV;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  // staging: piece 4 * wave + i (i = 0..3) of each tile = local rows 32 * wave + 8 * i + (lane >> 3); the swizzle key
  // ((row >> 1) & 7) = (4 * i + (lane >> 4)) & 7 depends on the parity of i only, the 16-row step of i >> 1 goes into the SGPR offset
  uint32_t offA[2], offW[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int lr = wave * 32 + par * 8 + (lane >> 3);
    const int chunk = swz_chunk(lane, lr);
    offA[par] = (uint32_t)(((long)lr * p.lda + chunk * 8) * 2);
    offW[par] = (uint32_t)(((long)lr * p.K + chunk * 8) * 2);
  }
  const int stepA = (int)(16 * p.lda * 2), stepW = 16 * p.K * 2;       // bytes per 16 rows
  const int nk = p.K / BK;
  char* const my_piece = smem + wave * 4096;
  auto stage_piece = [&](const TileSrc& s, auto bufc, auto ic, int kt, bool weights) {
    constexpr int B = decltype(bufc)::value, i = decltype(ic)::value;
    constexpr int OFF = B * KBUF + i * 1024;
    if (!weights) {
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)s.a, 0, s.a_bytes, 0x00020000);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(my_piece + OFF), 16, offA[i & 1],
                                               kt * (BK * 2) + (i >> 1) * stepA, 0, 0);
    } else {
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)s.w, 0, s.w_bytes, 0x00020000);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(my_piece + TILE + OFF), 16, offW[i & 1],
                                               kt * (BK * 2) + (i >> 1) * stepW, 0, 0);
    }
  };
  auto stage_ktile = [&](const TileSrc& s, auto bufc, int kt) {
    stage_piece(s, bufc, I0{}, kt, false); stage_piece(s, bufc, I0{}, kt, true);
    stage_piece(s, bufc, I1{}, kt, false); stage_piece(s, bufc, I1{}, kt, true);
    stage_piece(s, bufc, I2{}, kt, false); stage_piece(s, bufc, I2{}, kt, true);
    stage_piece(s, bufc, I3{}, kt, false); stage_piece(s, bufc, I3{}, kt, true);
  };
  // fragment reads
  int rdA[2], rdW[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    rdA[ks] = frag_addr(wr * 128, lane, ks);
    rdW[ks] = TILE + frag_addr(wc * 64, lane, ks);
  }
  f32x4_t acc[8][4];
  bf16x8_t aP[4], aR[4], wQ[4], wS[4];
  auto ld_a = [&](bf16x8_t& d, auto bufc, int ks, int blk) { d = *(const bf16x8_t*)(smem + rdA[ks] + decltype(bufc)::value * KBUF + blk * 2048); };
  auto ld_w = [&](bf16x8_t& d, auto bufc, int ks, int blk) { d = *(const bf16x8_t*)(smem + rdW[ks] + decltype(bufc)::value * KBUF + blk * 2048); };
  bool wave_live = true;
  auto mm = [&](int ib, int j, const bf16x8_t& a, const bf16x8_t& w) {
    acc[ib][j] = SWAPACC ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, acc[ib][j], 0, 0, 0)
                         : __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, w, acc[ib][j], 0, 0, 0);
  };
#define SPF() __builtin_amdgcn_sched_barrier(0)
  // one stage: 16 MFMAs on (a[0..3] -> row blocks r0 .. r0 + 3) x (w[0..3]); `side(g)` issues the stage's loads / DMA in gap g
  // (LIVE = false: a wave whose 64 columns lie past N takes part in the staging and the barriers but issues no MFMAs)
  auto stage16 = [&](auto livec, int r0, const bf16x8_t (&a)[4], const bf16x8_t (&w)[4], auto&& side) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      if constexpr (decltype(livec)::value) mm(r0 + (g >> 2), g & 3, a[g >> 2], w[g & 3]);
      side(g);
      SPF();
    }
  };
  // stage2c / morec (compile time): K-tile kt + 2 / kt + 1 exists -- the steady-state loop carries no tests
  auto ktile = [&](auto bufc, const TileSrc& src, int kt, auto livec, auto stage2c, auto morec) {
    constexpr int B = decltype(bufc)::value;
    using Bc = std::integral_constant<int, B>;
    using Nc = std::integral_constant<int, B ^ 1>;
    stage16(livec, 0, aP, wQ, [&](int g) { if ((g & 3) == 1) ld_a(aR[g >> 2], Bc{}, 0, 4 + (g >> 2)); });
    stage16(livec, 4, aR, wQ, [&](int g) {
      if ((g & 3) == 0) ld_a(aP[g >> 2], Bc{}, 1, g >> 2);
      if ((g & 3) == 2) ld_w(wS[g >> 2], Bc{}, 1, g >> 2);
    });
    stage16(livec, 0, aP, wS, [&](int g) { if ((g & 3) == 1) ld_a(aR[g >> 2], Bc{}, 1, 4 + (g >> 2)); });
    __builtin_amdgcn_s_waitcnt(0xC07F);                              // lgkmcnt(0): this wave's last reads of K-tile kt are in registers
    wait_vm<0>();                                                    // its pieces of K-tile kt + 1 have landed
    bar();
    constexpr bool more = decltype(morec)::value, stage2 = decltype(stage2c)::value;
    stage16(livec, 4, aR, wS, [&](int g) {
      if constexpr (stage2) {
        if (g == 0) stage_piece(src, Bc{}, I0{}, kt + 2, false);
        if (g == 2) stage_piece(src, Bc{}, I0{}, kt + 2, true);
        if (g == 4) stage_piece(src, Bc{}, I1{}, kt + 2, false);
        if (g == 6) stage_piece(src, Bc{}, I1{}, kt + 2, true);
        if (g == 8) stage_piece(src, Bc{}, I2{}, kt + 2, false);
        if (g == 10) stage_piece(src, Bc{}, I2{}, kt + 2, true);
        if (g == 12) stage_piece(src, Bc{}, I3{}, kt + 2, false);
        if (g == 14) stage_piece(src, Bc{}, I3{}, kt + 2, true);
      }
      if constexpr (more) {
        if ((g & 3) == 1) ld_a(aP[g >> 2], Nc{}, 0, g >> 2);
        if ((g & 3) == 3) ld_w(wQ[g >> 2], Nc{}, 0, g >> 2);
      }
    });
  };

  // the persistent walk, epilogues and next-tile request of ld_gemm8p_kernel around this kernel's own main loop
  TileSrc src;
  walk_tiles<BM, BN, 1, PREFETCH>(
      p, acc, src, [&](int m0, int n0) { return tile_src<2, false>(p, m0, n0); }, [&](int, int n0) { wave_live = n0 + wc * 64 < p.N; },
      [&](const TileSrc& s) { stage_ktile(s, I0{}, 0); },
      [&](bool k0_staged) {
        // ---- prologue: K-tile 0 landed, K-tile 1 in flight; first fragments in registers ----
        if (!k0_staged) stage_ktile(src, I0{}, 0);
        if (nk > 1) {
          stage_ktile(src, I1{}, 1);
          wait_vm<8>();                                   // the 8 pieces of K-tile 1
        } else {
          wait_vm<0>();
        }
        bar();
#pragma unroll
        for (int b = 0; b < 4; ++b) { ld_a(aP[b], I0{}, 0, b); ld_w(wQ[b], I0{}, 0, b); }
        using T = std::true_type; using F = std::false_type;
        auto kloop = [&](auto livec) {                                  // nk is even and >= 4 (launcher)
          int kt = 0;
          for (; kt + 2 < nk; kt += 2) {
            ktile(I0{}, src, kt, livec, T{}, T{});
            ktile(I1{}, src, kt + 1, livec, T{}, T{});
          }
          ktile(I0{}, src, kt, livec, F{}, T{});
          ktile(I1{}, src, kt + 1, livec, F{}, F{});
        };
        if (wave_live) kloop(T{}); else kloop(F{});
        // (every LDS read of this tile completed before its last barrier: the epilogue may overwrite the buffers)
      },
      [&](int m0, int n0, auto& hook) {
        if constexpr (EPI == EPI_QKV) qkv_epilogue16<4>(p, acc, smem + EPI_OFF, wave, lane, m0 + wr * 128, n0 + wc * 64, hook);
        else gemm_epilogue16<4, EPI, 4, SWAPACC>(p, acc, 0, smem + EPI_OFF, wave, lane, m0 + wr * 128, n0 + wc * 64, hook);
      });
#undef SPF
}

}  // namespace

// 512 x 128 tiles for convolutions with a 128-column output (ld_gemm8p_m512_kernel), persistent like launch_8p
int launch_8p_m512(const GemmParams& p, bool, hipStream_t stream) {
  dim3 grid(persistent_grid((long)((p.M + 511) / 512) * ((p.N + 127) / 128))), block(512);
  return with_epilogue<EPI_BIAS>(pick_epilogue(p), [&](auto e) {
    return launch_kernel<ld_gemm8p_m512_kernel<true, decltype(e)::value>>("ld_gemm8p_m512", grid, block, LD_LDS_TOTAL, stream, p);
  });
}

// the software-pipelined loop on launch_8p's grid: tiles [tile_begin, tile_end), one workgroup per CU unless LD_GEMM_PERSIST=0
int launch_sp(const GemmParams& p, bool, hipStream_t stream) {
  const int nbm = (p.M - p.m_begin + 255) / 256, nbn = (p.N + 255) / 256;
  const long ntiles = (p.tile_end > 0 ? p.tile_end : (long)nbm * nbn) - p.tile_begin;
  static int k_persist = LD_KNOB_UNSET;
  dim3 grid(ld_knob("LD_GEMM_PERSIST", 1, &k_persist) ? persistent_grid(ntiles) : (unsigned)ntiles), block(512);
  return with_epilogue<EPI_QKV, EPI_BIAS, EPI_GELU, EPI_GATE>(pick_epilogue(p), [&](auto e) {
    constexpr int E = decltype(e)::value;
    return launch_kernel<ld_gemm_sp_kernel<E>>(E == EPI_QKV ? "ld_gemm_qkv_heads(sp)" : "ld_gemm_sp", grid, block, LD_LDS_TOTAL, stream, p);
  });
}

}  // namespace ldgemm
