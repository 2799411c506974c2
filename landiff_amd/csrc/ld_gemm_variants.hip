// Measured alternatives to the shipped GEMM main loops, built into the variants library only (build.sh: VARIANT_ONLY): the 8-phase
// loop on 512 x 128 tiles (LD_GEMM_M512=1) and the software-pipelined loop (LD_GEMM_SP=1); the register-staged round-1 loop
// (LD_GEMM_TILE=11) sits beside the two-stage kernels in ld_gemm_2stage.hip.  Bit-identical to the shipped routes and measured slower
// or no faster; tests/test_gpu_variants.py runs them.
#include "ld_gemm.h"

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
// form of ld_gemm8p_kernel does not either).  The counted wait of ph3 leaves 4 + 1 pieces in flight.  Same dot products in the
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
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wq = wave & 3;                // waves w and w + 4 share a SIMD: they differ in wr only
  const int wrow = (wq >> 1) * 2 + wr, wc = wq & 1;       // wave row 0..3 (128 tile rows each), wave column 0..1 (64 columns each)

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
  uint32_t offA[2][4], offW[2];                           // [half][piece] byte offsets: four A pieces and one W piece per half-tile and wave
  auto set_offsets = [&](int m0, bool weights) {          // (A offsets depend on the tile only for a convolution)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lr = wave * 32 + i * 8 + (lane >> 3);     // local row of the A slot, 0 .. 255
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
      }
    }
    if (weights) {
      const int lr = wave * 8 + (lane >> 3);              // local row of the W slot, 0 .. 63
      const int chunk = (lane & 7) ^ ((lr >> 1) & 7);
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
    if (CONV) {
      const int tap = kt / cpt, c0 = (kt - tap * cpt) * BK;
      const int khw = p.kH * p.kW;
      const int dt = tap / khw, r2 = tap - dt * khw;
      const int dh = r2 / p.kW, dw = r2 - dh * p.kW;
      return (int)(((((long)dt * p.Hp + dh) * p.Wp + dw) * p.Cin + c0) * 2);
    }
    return kt * (BK * 2);
  };
  char* const my_a = smem + wave * 4096;                  // + buffer * KBUF + half * ASLOT (+ 1024 per further piece)
  char* const my_w = smem + 2 * ASLOT + wave * 1024;      // + buffer * KBUF + half * BSLOT
  Src src;                                                // the tile being computed
  auto stage_a = [&](const Src& s, auto bufc, auto hc, int kt) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(hc)::value * ASLOT;
    const int ko = koff_a(kt);
    stage_pieces<OFF>(s.a, s.a_bytes, my_a, offA[decltype(hc)::value][0], offA[decltype(hc)::value][1], ko);
    stage_pieces<OFF + 2048>(s.a, s.a_bytes, my_a, offA[decltype(hc)::value][2], offA[decltype(hc)::value][3], ko);
  };
  auto stage_w = [&](const Src& s, auto bufc, auto gc, int kt) {
    constexpr int OFF = decltype(bufc)::value * KBUF + decltype(gc)::value * BSLOT;
    stage_piece1<OFF>(s.w, s.w_bytes, my_w, offW[decltype(gc)::value], kt * (BK * 2));
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
    rdA[ks] = (wrow * 64 + (lane & 15)) * 128 + (c << 4);
    rdB[ks] = 2 * ASLOT + (wc * 32 + (lane & 15)) * 128 + (c << 4);
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
    // lgkmcnt(0) as the BUILTIN (simm16 0xC07F = vmcnt 63, expcnt 7, lgkmcnt 0): hipcc's own wait-count bookkeeping sees it.  As
    // inline asm it is invisible to that pass, which then re-waits before the next phase's fragment reads on the path that
    // skips the MFMAs (a pending ds_read into a register it is about to reuse) -- serialising the B and A reads of ph0.
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
            acc[H * 4 + i][G * 2 + j] = SWAPACC ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][ks], a[i][ks], acc[H * 4 + i][G * 2 + j], 0, 0, 0)
                                                : __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][ks], b[j][ks], acc[H * 4 + i][G * 2 + j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto bar = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  auto ktile = [&](auto bufc, int kt) {
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
      asm volatile("s_waitcnt vmcnt(5)" ::: "memory");    // K-tile kt + 1 has landed; A_0 (4 pieces) / B_0 (1) of kt + 2 stay in flight
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    bar(); mma(I1{}, I0{}, b0); bar();
  };

  set_offsets(0, true);
  bool k0_staged = false;                                 // K-tile 0 of the tile about to start is already on its way
  const int v_end = p.tile_end > 0 ? p.tile_end : ntiles; // (the tiles behind it: ld_gemm8p_n128_kernel)
  for (int v = p.tile_begin + blockIdx.x; v < v_end; v += gridDim.x) {
    int m0, n0;
    tile_origin(v, m0, n0);
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
      asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
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

    // ---- epilogue, with the next tile's first K-tile requested from inside it ----
    const int vn = v + gridDim.x;
    bool hooked = false;
    Src nsrc = src;
    k0_staged = false;
    // (no prefetch of the next tile's first K-tile: the epilogue staging lives in buffer 0)
    auto hook = [&]() {
      if (!hooked && k0_staged) stage_ktile0(nsrc);
      hooked = true;
    };
    gemm_epilogue16<4, EPI, 4, SWAPACC, decltype(hook)&, CONV>(p, acc, 0, smem + EPI_OFF, wave, lane, m0 + wrow * 128, n0 + wc * 64, hook);
    hook();
    if (vn < v_end) __syncthreads();                      // the staging region (K-tile buffer 0) is free again before it is re-staged
  }
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
  const int nbm = (p.M - p.m_begin + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  const int ntiles = nbm * nbn;
  const int gm_sz = p.group_m;
  auto tile_origin = [&](int v, int& m0, int& n0) {
    const int bid = xcd_remap(v, ntiles);
    const int per_group = gm_sz * nbn;
    const int group = bid / per_group, in_group = bid - group * per_group;
    const int first_m = group * gm_sz;
    const int rows_here = (nbm - first_m) < gm_sz ? (nbm - first_m) : gm_sz;
    m0 = p.m_begin + (first_m + in_group % rows_here) * BM;
    n0 = (in_group / rows_here) * BN;
  };
  const auto clip = [](long v) { return (int)(v < 0x7fffffffL ? v : 0x7fffffffL); };
  struct Src { const bf16_t* a; const bf16_t* w; int a_bytes, w_bytes; };
  auto tile_src = [&](int m0, int n0) {
    Src s;
    s.a = p.A + (long)m0 * p.lda;
    s.w = p.W + (long)n0 * p.K;
    s.a_bytes = clip(((long)(p.M - m0) * p.lda) * 2);
    s.w_bytes = clip(((long)(p.N - n0) * p.K) * 2);
    return s;
  };
  // staging: piece 4 * wave + i (i = 0..3) of each tile = local rows 32 * wave + 8 * i + (lane >> 3); the swizzle key
  // ((row >> 1) & 7) = (4 * i + (lane >> 4)) & 7 depends on the parity of i only, the 16-row step of i >> 1 goes into the SGPR offset
  uint32_t offA[2], offW[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int lr = wave * 32 + par * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((lr >> 1) & 7);
    offA[par] = (uint32_t)(((long)lr * p.lda + chunk * 8) * 2);
    offW[par] = (uint32_t)(((long)lr * p.K + chunk * 8) * 2);
  }
  const int stepA = (int)(16 * p.lda * 2), stepW = 16 * p.K * 2;       // bytes per 16 rows
  const int nk = p.K / BK;
  char* const my_piece = smem + wave * 4096;
  auto stage_piece = [&](const Src& s, auto bufc, auto ic, int kt, bool weights) {
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
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
  auto stage_ktile = [&](const Src& s, auto bufc, int kt) {
    stage_piece(s, bufc, I0{}, kt, false); stage_piece(s, bufc, I0{}, kt, true);
    stage_piece(s, bufc, I1{}, kt, false); stage_piece(s, bufc, I1{}, kt, true);
    stage_piece(s, bufc, I2{}, kt, false); stage_piece(s, bufc, I2{}, kt, true);
    stage_piece(s, bufc, I3{}, kt, false); stage_piece(s, bufc, I3{}, kt, true);
  };
  // fragment reads
  int rdA[2], rdW[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int c = (ks * 4 + (lane >> 4)) ^ (((lane & 15) >> 1) & 7);
    rdA[ks] = (wr * 128 + (lane & 15)) * 128 + (c << 4);
    rdW[ks] = TILE + (wc * 64 + (lane & 15)) * 128 + (c << 4);
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
  auto ktile = [&](auto bufc, const Src& src, int kt, auto livec, auto stage2c, auto morec) {
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
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // its pieces of K-tile kt + 1 have landed
    SPF(); __builtin_amdgcn_s_barrier(); SPF();
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

  bool k0_staged = false;
  for (int v = blockIdx.x; v < ntiles; v += gridDim.x) {
    int m0, n0;
    tile_origin(v, m0, n0);
    const Src src = tile_src(m0, n0);
    wave_live = n0 + wc * 64 < p.N;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    // ---- prologue: K-tile 0 landed, K-tile 1 in flight; first fragments in registers ----
    if (!k0_staged) stage_ktile(src, I0{}, 0);
    if (nk > 1) {
      stage_ktile(src, I1{}, 1);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    SPF(); __builtin_amdgcn_s_barrier(); SPF();
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
    const int vn = v + gridDim.x;
    bool hooked = false;
    Src nsrc = src;
    k0_staged = false;
    if (PREFETCH && vn < ntiles) {
      int m1, n1;
      tile_origin(vn, m1, n1);
      nsrc = tile_src(m1, n1);
      k0_staged = true;
    }
    auto hook = [&]() {
      if (!hooked && k0_staged) stage_ktile(nsrc, I0{}, 0);
      hooked = true;
    };
    if constexpr (EPI == EPI_QKV) qkv_epilogue16<4>(p, acc, smem + EPI_OFF, wave, lane, m0 + wr * 128, n0 + wc * 64, hook);
    else gemm_epilogue16<4, EPI, 4, SWAPACC>(p, acc, 0, smem + EPI_OFF, wave, lane, m0 + wr * 128, n0 + wc * 64, hook);
    hook();
    if (vn < ntiles) __syncthreads();
  }
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
