// Two-stage, barrier-drained main loops (ld_gemm.h: what the GEMM files share; ld_gemm.hip: which problems come here): the 128 x 128
// tile of small problems, the bottom rows of a row-split launch and the 256 x 256 tile with LD_GEMM_8P=0 (ld_gemm_kernel), the same
// loop on fp8 operands (ld_gemm_f8_kernel) and, in the variants build, the register-staged round-1 loop (ld_gemm_w4r_kernel).
// These three share one file on purpose: the compiler's register allocation for the 32x32x16 forms of ld_gemm_kernel and for
// ld_gemm_w4r_kernel depends on ld_gemm_f8_kernel being in the same module (compared per function against the one-file build).
#include "ld_gemm_8p_dev.h"     // the raster and the addresses (the 8-phase family's header states them once)

namespace ldgemm {
namespace {

// Block tile BM x BN, WM x WN waves, each wave (BM/WM) x (BN/WN) = MI x NI MFMA 32x32 tiles.
// M16: the same tiles on v_mfma_f32_16x16x32_bf16 (32-deep k-steps, [2 * MI][4] accumulators of 4 registers): equal FLOPs per
// register and per LDS byte, but the 16x16x32 form draws less power per FLOP on random operands -- under the chip's power
// governor an MFMA-only loop sustains 2105 TFLOP/s on it against 1837 on 32x32x16 (tools/probe/mfma_power.hip,
// profiles/r02_mfma_power_probe.txt) -- and power, not issue slots, is what bounds these kernels.
template <int BM, int BN, int WM, int WN, int NSTAGE, bool CONV, int EPI, bool M16 = false>
__global__ __launch_bounds__(WM * WN * 64, (WM * WN >= 16) ? 4 : 2) void ld_gemm_kernel(GemmParams p) {
  constexpr int NW = WM * WN;
  constexpr int NT = NW * 64;
  constexpr int MI = BM / WM / 32, NI = BN / WN / 32;
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int A_LOADS = BM / 8 / NW, B_LOADS = BN / 8 / NW;     // 1 KB LDS-DMA pieces per wave
  static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "tile/wave mismatch");
  static_assert(BN / WN == 64, "epilogue staging assumes 64-column wave tiles");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WN, wc = wave % WN;

  const int nbm = (p.M - p.m_begin + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  int m0, n0;
  tile_origin<BM, BN>(blockIdx.x, nbm, nbn, p.group_m, p.m_begin, m0, n0);      // one tile per workgroup, in the grouped raster's order

  // ---- per-thread source row offsets ----
  // element offsets, zero-extended where they are added to the pointers: < 2^32 for a convolution, whose padded input
  // conv_cl keeps below CONV_MAX_BYTES = 8 GiB (a 49-frame 480 x 720 VAE-encoder level reaches 2.27e9)
  uint32_t offA[A_LOADS], offW[B_LOADS];
#pragma unroll
  for (int i = 0; i < A_LOADS; ++i) {
    const int r = (wave * A_LOADS + i) * 8 + (lane >> 3);
    const int chunk = swz_chunk(lane, r);
    int gm = m0 + r; gm = gm < p.M ? gm : p.M - 1;
    if (CONV) {
      offA[i] = (uint32_t)(conv_row_elems(p, gm) + chunk * 8);
    } else {
      offA[i] = (uint32_t)((long)gm * p.lda + chunk * 8);
    }
  }
#pragma unroll
  for (int i = 0; i < B_LOADS; ++i) {
    const int r = (wave * B_LOADS + i) * 8 + (lane >> 3);
    const int chunk = swz_chunk(lane, r);
    int gn = n0 + r; gn = gn < p.N ? gn : p.N - 1;
    offW[i] = (uint32_t)((long)gn * p.K + chunk * 8);
  }

  const int nk = p.K / BK;
  const int cpt = CONV ? p.Cin / BK : 1;   // K-tiles per tap

  auto stage = [&](int buf, int kt) {
    const long koffA = CONV ? conv_tap_elems(p, kt, cpt) : (long)kt * BK;
    const long koffW = (long)kt * BK;
    char* base = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) glds16(p.A + offA[i] + koffA, base + (wave * A_LOADS + i) * 1024);
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) glds16(p.W + offW[i] + koffW, base + A_BYTES + (wave * B_LOADS + i) * 1024);
  };

  f32x16_t acc[M16 ? 1 : MI][M16 ? 1 : NI];
  f32x4_t acc16[M16 ? 2 * MI : 1][M16 ? 4 : 1];
  if constexpr (M16) {
#pragma unroll
    for (int i = 0; i < 2 * MI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc16[i][j][r] = 0.f;
  } else {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  }

  // fragment read offsets: row * 128 B plus the swizzled 16-B chunk of k-step kk (rows of later MFMA tiles are
  // +32 rows = +4096 B (16x16x32: +16 rows = +2048 B) with the same swizzle key, so they fold into the ds_read immediate
  // offset).  16x16x32 operand: lane l holds row l & 15, k = (l >> 4) * 8 .. + 8 of the 32-deep step: the 16-byte chunk
  // ks * 4 + (l >> 4); with the (row >> 1) & 7 XOR the four 16-lane groups of a ds_read_b128 each cover all 64 banks.
  int rdA[4], rdB[4];
  if constexpr (M16) {
    const int ra = wr * (BM / WM) + (lane & 15), rb = wc * (BN / WN) + (lane & 15);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = ks * 4 + (lane >> 4);
      rdA[ks] = ra * 128 + ((c ^ ((ra >> 1) & 7)) << 4);
      rdB[ks] = A_BYTES + rb * 128 + ((c ^ ((rb >> 1) & 7)) << 4);
    }
    rdA[2] = rdA[3] = rdB[2] = rdB[3] = 0;
  } else {
    const int ra = wr * (BM / WM) + (lane & 31), rb = wc * (BN / WN) + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int c = kk * 2 + (lane >> 5);
      rdA[kk] = ra * 128 + ((c ^ ((ra >> 1) & 7)) << 4);
      rdB[kk] = A_BYTES + rb * 128 + ((c ^ ((rb >> 1) & 7)) << 4);
    }
  }

  // One K-tile of MFMAs.  Fragments are software pipelined by hand (k-step kk+1 is requested before the MFMAs of kk)
  // and a scheduling barrier after every k-step keeps hipcc from hoisting all 4 k-steps' loads at once, which spills
  // the 128-register accumulator tile of the 256x256 configuration.
  // a wave whose 64 output columns lie entirely past N (the half-empty last tile column of the N = 1920 shapes) issues no
  // MFMAs: its accumulators stay zero and are never stored; the tile takes as long, at half the energy
  const bool wave_live = n0 + wc * (BN / WN) < p.N;
  auto compute = [&](auto bufc) {
    constexpr int OFF = decltype(bufc)::value * STAGE;
    if (!wave_live) return;
    if constexpr (M16) {
      // B fragments of both k-steps up front; A fragments single-buffered: block i's k-step-1 fragment is requested right
      // after its four k-step-0 MFMAs (2 * MI - 1 blocks of MFMAs of cover), which keeps the fragment registers at
      // (2 * MI + 8) x 4 next to the accumulators
      bf16x8_t a[2 * MI], b[2][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[0][j] = *(const bf16x8_t*)(smem + rdB[0] + OFF + j * 2048);
#pragma unroll
      for (int i = 0; i < 2 * MI; ++i) a[i] = *(const bf16x8_t*)(smem + rdA[0] + OFF + i * 2048);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[1][j] = *(const bf16x8_t*)(smem + rdB[1] + OFF + j * 2048);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int i = 0; i < 2 * MI; ++i) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[ks][j], acc16[i][j], 0, 0, 0);
          if (ks == 0) {
            __builtin_amdgcn_sched_barrier(0);
            a[i] = *(const bf16x8_t*)(smem + rdA[1] + OFF + i * 2048);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      bf16x8_t a[2][MI], b[2][NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) a[0][i] = *(const bf16x8_t*)(smem + rdA[0] + OFF + i * 4096);
#pragma unroll
      for (int j = 0; j < NI; ++j) b[0][j] = *(const bf16x8_t*)(smem + rdB[0] + OFF + j * 4096);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int cur = kk & 1, nxt = cur ^ 1;
        if (kk < 3) {
#pragma unroll
          for (int i = 0; i < MI; ++i) a[nxt][i] = *(const bf16x8_t*)(smem + rdA[kk + 1] + OFF + i * 4096);
#pragma unroll
          for (int j = 0; j < NI; ++j) b[nxt][j] = *(const bf16x8_t*)(smem + rdB[kk + 1] + OFF + j * 4096);
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[cur][i], b[cur][j], acc[i][j], 0, 0, 0);
        if (MI * NI > 4) __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  if (NSTAGE == 2) {
    // two K-tiles per trip with compile-time buffer indices; no mid-loop exit (a `break` between the two halves makes
    // hipcc keep two copies of the 64 accumulator registers and shuffle them every trip), odd tail peeled
    stage(0, 0);
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
      __syncthreads();   // drains this wave's LDS-DMA (vmcnt(0)) and releases the other buffer
      stage(1, kt + 1);
      compute(std::integral_constant<int, 0>{});
      __syncthreads();
      if (kt + 2 < nk) stage(0, kt + 2);
      compute(std::integral_constant<int, 1>{});
    }
    if (kt < nk) {
      __syncthreads();
      compute(std::integral_constant<int, 0>{});
    }
  } else {
    // 3-deep LDS ring: the K-tile two steps ahead is requested while tile kt is consumed, and the barrier only
    // waits for tile kt (counted vmcnt: the newest tile's DMA stays in flight across the barrier; a raw s_barrier is
    // used because __syncthreads would drain vmcnt to 0).  RAW: own vmcnt + barrier; WAR: buffer (kt+2)%3 was last
    // read by compute(kt-1), which every wave has finished before passing barrier kt.
    constexpr int LPS = A_LOADS + B_LOADS;       // LDS-DMA instructions per wave per stage
    stage(0, 0);
    if (nk > 1) stage(1, 1);
    auto step = [&](auto bufc, int kt) {
      constexpr int B = decltype(bufc)::value;
      if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + 2 < nk) stage((B + 2) % 3, kt + 2);
      compute(bufc);
    };
    int kt = 0;
    for (; kt + 2 < nk; kt += 3) {
      step(std::integral_constant<int, 0>{}, kt);
      step(std::integral_constant<int, 1>{}, kt + 1);
      step(std::integral_constant<int, 2>{}, kt + 2);
    }
    if (kt < nk) step(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < nk) step(std::integral_constant<int, 1>{}, kt + 1);
  }
  __syncthreads();

  if constexpr (EPI == EPI_QKV) {
    static_assert(M16 || EPI != EPI_QKV, "the fused qkv split exists for the 16x16x32 accumulator layout only");
    if constexpr (M16) qkv_epilogue16<MI>(p, acc16, smem, wave, lane, m0 + wr * (BM / WM), n0 + wc * 64);
  } else if constexpr (M16) gemm_epilogue16<MI, EPI, 4, false, NoHook, CONV && MI % 2 == 0>(p, acc16, 0, smem, wave, lane, m0 + wr * (BM / WM), n0 + wc * 64);
  else gemm_epilogue<MI, NI, EPI, CONV && MI % 2 == 0>(p, acc, smem, wave, lane, m0 + wr * (BM / WM), n0 + wc * 64);
}

// ------------------------------------------------------------------------------------------------
// fp8 (OCP e4m3) x fp8 -> fp32 GEMM for the DiT's four large linear layers (BASELINE config 5; never the headline
// metric, which is bf16).  Same 256x256 tile / 8 waves (2 x 4, 128x64 per wave) / two-stage LDS-DMA structure as
// ld_gemm_kernel: a K-tile is again 128 BYTES per row -- now 128 elements -- so the DMA pieces, the XOR swizzle and the
// LDS footprint are unchanged while every tile carries twice the K.  v_mfma_scale_f32_32x32x64_f8f6f4 (unit scales)
// takes 32 bytes per lane per operand: row = lane % 32; lanes 0-31 hold k 0-15 and 32-47 of the 64-deep step, lanes 32-63
// hold k 16-31 and 48-63 (tools/probe/fp8_mfma_layout.hip, fp8_mfma_scale.hip), i.e. two 16-byte chunks of the tile row.
// The accumulator is dequantised in registers -- acc * scale_a[row] * scale_w[col] -- and then takes the ordinary
// epilogues (bias / GELU / gated residual).
// ------------------------------------------------------------------------------------------------

// MX = true: MXFP8 operands -- the per-32-element E8M0 scales go into the MFMA itself (one byte per lane and operand: the
// lane's row and its 32-deep half of the 64-deep step), fetched as one dword per row and 128-deep K-tile straight into
// registers one tile ahead; no dequantisation in the epilogue.
template <int EPI, bool MX>
__global__ __launch_bounds__(512, 2) void ld_gemm_f8_kernel(GemmParams p) {
  constexpr int BM = 256, BN = 256, WN = 4, NW = 8, MI = 4, NI = 2;
  constexpr int KB = 128;                                    // bytes (= elements) of K per tile
  constexpr int A_BYTES = BM * KB, B_BYTES = BN * KB, STAGE = A_BYTES + B_BYTES;
  constexpr int A_LOADS = BM / 8 / NW, B_LOADS = BN / 8 / NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WN, wc = wave % WN;
  const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  int m0, n0;
  tile_origin<BM, BN>(blockIdx.x, nbm, nbn, p.group_m, 0, m0, n0);
  // LDS-DMA through raw buffer descriptors based at the tile origin (rows past M / N read as zeros, no clamping): the
  // wave-uniform part of every address -- K-tile, 16-row step between a wave's pieces -- is the scalar offset, the per-lane
  // part is ONE 32-bit offset per piece parity (the source-side swizzle key (row >> 1) & 7 repeats every 16 rows).
  const long ldab = p.lda, ldwb = p.K;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.A + (long)m0 * ldab), 0, clip((long)(p.M - m0) * ldab), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.W + (long)n0 * ldwb), 0, clip((long)(p.N - n0) * ldwb), 0x00020000);
  uint32_t voA[2], voW[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int ra = (wave * A_LOADS + par) * 8 + (lane >> 3), rb = (wave * B_LOADS + par) * 8 + (lane >> 3);
    voA[par] = (uint32_t)(ra * ldab + (swz_chunk(lane, ra) << 4));
    voW[par] = (uint32_t)(rb * ldwb + (swz_chunk(lane, rb) << 4));
  }
  const int sa16 = (int)(16 * ldab), sw16 = (int)(16 * ldwb);
  const int nk = p.K / KB;
  // MX scales: one dword (4 blocks = one K-tile) per tile row, staged through LDS next to the operands -- waves 0-3 fetch
  // the 256 A rows' dwords, waves 4-7 the 256 W rows' (one 4-byte LDS-DMA each) -- and read back at use (no registers held)
  constexpr int SC_OFF = 2 * STAGE;                          // [2 stages][A 1 KB | W 1 KB]
  const long srows = wave < 4 ? p.M : p.N;                    // rows per K-tile slab of the scale array
  const long sorig = wave < 4 ? m0 : n0;
  const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(MX ? (wave < 4 ? p.mx_a : p.mx_w) + sorig * 4 : (const unsigned char*)p.A), 0,
      MX ? clip(((long)(p.K >> 7) * srows - sorig) * 4) : 0, 0x00020000);
  const uint32_t soff = (uint32_t)(((wave & 3) * 64 + lane) * 4);
  const int sslab = (int)(srows * 4);                         // bytes between consecutive K-tiles' slabs
  auto stage = [&](auto bufc, int kt) {
    constexpr int buf = decltype(bufc)::value;
    if (MX) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsS, (__attribute__((address_space(3))) void*)(smem + SC_OFF + buf * 2048 + wave * 256),
                                               4, soff, kt * sslab, 0, 0);
    }
    char* base = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(base + (wave * A_LOADS + i) * 1024), 16,
                                               voA[i & 1], kt * KB + (i >> 1) * sa16, 0, 0);
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (__attribute__((address_space(3))) void*)(base + A_BYTES + (wave * B_LOADS + i) * 1024), 16,
                                               voW[i & 1], kt * KB + (i >> 1) * sw16, 0, 0);
  };

  f32x16_t acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  int rdA[2][2], rdB[2][2];                                  // [64-deep step][16-byte half]
  {
    const int ra = wr * 128 + (lane & 31), rb = wc * 64 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // register half h of lane-half g holds k = 64 kk + 32 h + 16 g .. +16: that is the hardware's K order (it matters
        // once the two 32-element blocks of a step carry different scales; tools/probe/fp8_mfma_scale.hip)
        const int c = kk * 4 + h * 2 + (lane >> 5);
        rdA[kk][h] = ra * 128 + ((c ^ ((ra >> 1) & 7)) << 4);
        rdB[kk][h] = A_BYTES + rb * 128 + ((c ^ ((rb >> 1) & 7)) << 4);
      }
  }
  auto ldfrag = [&](int off) {
    const u32x4_t lo = *(const u32x4_t*)(smem + off);
    return lo;
  };
  auto frag32 = [&](int off0, int off1) {
    const u32x4_t lo = ldfrag(off0), hi = ldfrag(off1);
    return (i32x8_t){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  };
  // One K-tile: per 64-deep step the two W fragments stay live, the A fragments stream through a two-deep register
  // pipeline (fragment i+1 is requested before the MFMAs of fragment i) -- 32 fragment registers instead of 48.
  auto compute = [&](auto bufc) {
    constexpr int OFF = decltype(bufc)::value * STAGE;
    uint32_t sb[NI];
    const char* sc = smem + SC_OFF + decltype(bufc)::value * 2048;
    if (MX) {
#pragma unroll
      for (int j = 0; j < NI; ++j) sb[j] = *(const uint32_t*)(sc + 1024 + (wc * 64 + j * 32 + (lane & 31)) * 4) >> ((lane >> 5) * 8);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      i32x8_t b[NI], a[2];
#pragma unroll
      for (int j = 0; j < NI; ++j) b[j] = frag32(rdB[kk][0] + OFF + j * 4096, rdB[kk][1] + OFF + j * 4096);
      a[0] = frag32(rdA[kk][0] + OFF, rdA[kk][1] + OFF);
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        if (i + 1 < MI) a[(i + 1) & 1] = frag32(rdA[kk][0] + OFF + (i + 1) * 4096, rdA[kk][1] + OFF + (i + 1) * 4096);
        uint32_t sa = 0;
        if (MX) sa = *(const uint32_t*)(sc + (wr * 128 + i * 32 + (lane & 31)) * 4) >> ((lane >> 5) * 8);
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          if constexpr (MX) {
            // after the >> (8 * half), byte 0 / byte 2 of the register is this lane's block of step 0 / step 1
            if (kk == 0) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[i & 1], b[j], acc[i][j], 0, 0, 0, sa, 0, sb[j]);
            else acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[i & 1], b[j], acc[i][j], 0, 0, 2, sa, 2, sb[j]);
          } else {
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[i & 1], b[j], acc[i][j], 0, 0, 0, 127, 0, 127);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;
  stage(B0{}, 0);
  int kt = 0;
  for (; kt + 1 < nk; kt += 2) {
    __syncthreads();
    stage(B1{}, kt + 1);
    compute(std::integral_constant<int, 0>{});
    __syncthreads();
    if (kt + 2 < nk) stage(B0{}, kt + 2);
    compute(std::integral_constant<int, 1>{});
  }
  if (kt < nk) {
    __syncthreads();
    compute(std::integral_constant<int, 0>{});
  }
  __syncthreads();

  // dequantise: acc[i][j][r] is C[row0 + 32 i + 8 (r / 4) + 4 (lane / 32) + r % 4][col0 + 32 j + lane % 32]
  const int row0 = m0 + wr * 128, col0 = n0 + wc * 64;
  if constexpr (!MX) {
    float sw[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) { const int gn = col0 + j * 32 + (lane & 31); sw[j] = p.scale_w[gn < p.N ? gn : p.N - 1]; }
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gm = row0 + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        const float sa = p.scale_a[gm < p.M ? gm : p.M - 1];
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j][r] *= sa * sw[j];
      }
  }
  gemm_epilogue<MI, NI, EPI>(p, acc, smem, wave, lane, row0, col0);
}

#ifdef LD_VARIANTS   // measured alternative, not in the shipped library
// ------------------------------------------------------------------------------------------------
// One-wave-per-SIMD, register-staged main loop on v_mfma_f32_32x32x16_bf16 (the round-1 default, LD_GEMM_TILE=11; see
// profiles/r01d_gemm_vs_vendor_library.txt for the measurements that shaped it): 256x256 tile, 4 waves x 128x128 = 4x4
// accumulators of 16 registers (256 of the wave's 512 registers), K-tiles 64 deep on full 128-byte lines.  Global memory -> VGPRs by buffer_load_dwordx4 (row offsets in SGPRs, out-of-range rows read as zero
// through the buffer descriptor's bounds check), two register sets = prefetch three K-tiles ahead; VGPRs -> LDS by
// ds_write_b128 one tile ahead into a two-slot ring (2 x 64 KB, XOR-swizzled 16-byte chunks as in ld_gemm_kernel).
//   tile t:  k-steps 0,1: 16 MFMA each + ds_write of K-tile t+1 (8 per k-step)     [its slot was last read in tile t-1]
//            k-step  2  : 16 MFMA + first half of the loads of K-tile t+3
//            lgkmcnt(0) + barrier: K-tile t+1 visible everywhere, and nobody reads slot t&1 past k-step 3's registers
//            k-step  3  : 16 MFMA + second half of the loads; fragment prefetch of (t+1, 0)
template <int EPI>
__global__ __launch_bounds__(256, 1) void ld_gemm_w4r_kernel(GemmParams p) {
  constexpr int BM = 256, BN = 256, KT = 64;
  constexpr int A_BYTES = BM * KT * 2;              // 32 KB
  constexpr int SLOT = (BM + BN) * KT * 2;          // 64 KB
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;

  const int nbm = (p.M - p.m_begin + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  int m0, n0;
  tile_origin<BM, BN>(blockIdx.x, nbm, nbn, p.group_m, p.m_begin, m0, n0);

  // this wave stages rows [wave*64, wave*64+64) of the A tile and of the W tile: 8 + 8 loads of 8 rows x 128 B per K-tile
  const long ldab = p.lda * 2, ldwb = (long)p.K * 2;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.A + (long)m0 * ldab), 0, clip((long)(p.M - m0) * ldab), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.W + (long)n0 * ldwb), 0, clip((long)(p.N - n0) * ldwb), 0x00020000);
  const int rl = lane >> 3, cl = lane & 7;                         // row within the 8-row group, 16-byte chunk
  const uint32_t voA = (uint32_t)((wave * 64 + rl) * ldab + cl * 16);
  const uint32_t voW = (uint32_t)((wave * 64 + rl) * ldwb + cl * 16);
  const int sa8 = (int)(8 * ldab), sw8 = (int)(8 * ldwb);          // SGPR step between a wave's 8-row groups
  // LDS write addresses: row = wave*64 + i*8 + rl, chunk cl ^ ((row >> 1) & 7); (row>>1)&7 alternates with i's parity
  int wrofs[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int row = wave * 64 + par * 8 + rl;
    wrofs[par] = row * 128 + ((cl ^ ((row >> 1) & 7)) << 4);
  }
  const int nk = p.K / KT;

  u32x4_t st[2][16];           // two staging sets: K-tile tau lives in set tau & 1 (loads 0-7: A groups, 8-15: W groups)
  auto LOAD = [&](auto setc, int q, int kt) {
    constexpr int U = decltype(setc)::value;
    if (q < 8) st[U][q] = __builtin_amdgcn_raw_buffer_load_b128(rsA, voA, kt * (KT * 2) + q * sa8, 0);
    else st[U][q] = __builtin_amdgcn_raw_buffer_load_b128(rsW, voW, kt * (KT * 2) + (q - 8) * sw8, 0);
  };
  auto WRITE = [&](auto setc, int slot, int q) {
    constexpr int U = decltype(setc)::value;
    const int i = q & 7;
    char* dst = smem + slot * SLOT + (q < 8 ? 0 : A_BYTES) + wrofs[i & 1] + (i >> 1) * 2048;
    *(u32x4_t*)dst = st[U][q];
  };

  f32x16_t acc[2][4][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[h][i][j][r] = 0.f;

  int rdA[4], rdB[4];          // fragment read offsets inside a slot for the four k-steps (+4096 B per further 32 rows)
  {
    const int ra = wr * 128 + (lane & 31), rb = wc * 128 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int c = kk * 2 + (lane >> 5);
      rdA[kk] = ra * 128 + ((c ^ ((ra >> 1) & 7)) << 4);
      rdB[kk] = A_BYTES + rb * 128 + ((c ^ ((rb >> 1) & 7)) << 4);
    }
  }
  bf16x8_t fa[2][4], fb[2][4];
  auto FRAG = [&](auto bufc, int slot, int kk, int g) {
    constexpr int B = decltype(bufc)::value;
    if (g < 4) fa[B][g] = *(const bf16x8_t*)(smem + rdA[kk] + slot * SLOT + g * 4096);
    else fb[B][g - 4] = *(const bf16x8_t*)(smem + rdB[kk] + slot * SLOT + (g - 4) * 4096);
  };
#define FENCE() __builtin_amdgcn_sched_barrier(0)
  // one k-step: 16 MFMAs on fragment set B, the 8 fragment reads of the next k-step behind the first four pairs, and one
  // staging operation per pair: MODE 1 = ds_write of set U pieces q0..q0+7, MODE 2 = loads of K-tile lkt into set U
  auto kstep = [&](auto bufc, int nslot, int nkk, auto modec, auto setc, int q0, int wslot, int lkt) {
    constexpr int B = decltype(bufc)::value;
    constexpr int MODE = decltype(modec)::value;
    using NB = std::integral_constant<int, 1 - B>;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const int i = g >> 1, j0 = (g & 1) * 2;
      acc[j0 >> 1][i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[B][i], fb[B][j0], acc[j0 >> 1][i][0], 0, 0, 0);
      if (g < 4) FRAG(NB{}, nslot, nkk, 2 * g);
      acc[j0 >> 1][i][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[B][i], fb[B][j0 + 1], acc[j0 >> 1][i][1], 0, 0, 0);
      if (g < 4) FRAG(NB{}, nslot, nkk, 2 * g + 1);
      if (MODE == 1) WRITE(setc, wslot, q0 + g);
      if (MODE == 2) LOAD(setc, q0 + g, lkt);
      FENCE();
    }
  };
  using B0 = std::integral_constant<int, 0>; using B1 = std::integral_constant<int, 1>;
  using M0 = std::integral_constant<int, 0>; using M1 = std::integral_constant<int, 1>; using M2 = std::integral_constant<int, 2>;

  // ---- prologue: K-tiles 0, 1, 2 requested; K-tile 0 -> slot 0; fragments of (0,0) ----
#pragma unroll
  for (int q = 0; q < 16; ++q) LOAD(B0{}, q, 0);
#pragma unroll
  for (int q = 0; q < 16; ++q) LOAD(B1{}, q, 1 < nk ? 1 : 0);
#pragma unroll
  for (int q = 0; q < 16; ++q) WRITE(B0{}, 0, q);
#pragma unroll
  for (int q = 0; q < 16; ++q) LOAD(B0{}, q, 2 < nk ? 2 : 0);
  __builtin_amdgcn_s_waitcnt(0xc07f);         // lgkmcnt(0) only (vmcnt / expcnt fields at "no wait")
  __builtin_amdgcn_s_barrier();
  FENCE();
#pragma unroll
  for (int g = 0; g < 8; ++g) FRAG(B0{}, 0, 0, g);

  // tile t in slot S = t & 1; set U = (t + 1) & 1 holds K-tile t+1 on entry and receives K-tile t+3
  auto tile = [&](auto slotc, int t) {
    constexpr int S = decltype(slotc)::value;
    using U = std::integral_constant<int, 1 - S>;
    const int lkt = t + 3 < nk ? t + 3 : nk - 1;      // past the end: a re-fetch that is never multiplied
    kstep(B0{}, S, 1, M1{}, U{}, 0, 1 - S, 0);        // k-step 0: fragments of (t,1); ds_write pieces 0-7 of K-tile t+1
    kstep(B1{}, S, 2, M1{}, U{}, 8, 1 - S, 0);        // k-step 1: fragments of (t,2); ds_write pieces 8-15
    kstep(B0{}, S, 3, M2{}, U{}, 0, 0, lkt);          // k-step 2: fragments of (t,3); loads 0-7 of K-tile t+3
    __builtin_amdgcn_s_waitcnt(0xc07f);               // lgkmcnt(0): this wave's ds_writes and fragment reads retired
    __builtin_amdgcn_s_barrier();
    FENCE();
    kstep(B1{}, 1 - S, 0, M2{}, U{}, 8, 0, lkt);      // k-step 3: fragments of (t+1,0); loads 8-15
  };
  for (int t = 0; t < nk; t += 2) {
    tile(std::integral_constant<int, 0>{}, t);
    tile(std::integral_constant<int, 1>{}, t + 1);
  }
#undef FENCE
  __syncthreads();

  gemm_epilogue<4, 2, EPI>(p, acc[0], smem, wave, lane, m0 + wr * 128, n0 + wc * 128);
  gemm_epilogue<4, 2, EPI>(p, acc[1], smem, wave, lane, m0 + wr * 128, n0 + wc * 128 + 64);
}
#endif  // LD_VARIANTS

template <int BM, int BN, int WM, int WN, int NSTAGE>
int launch_cfg(const GemmParams& p, bool conv, hipStream_t stream) {
  constexpr int NW = WM * WN;
  constexpr int STAGE = (BM + BN) * BK * 2;
  constexpr int EPIB = NW * 32 * CW_STRIDE * 4;
  constexpr int SMEM = (NSTAGE * STAGE > EPIB) ? NSTAGE * STAGE : EPIB;
  constexpr int SMEM_QKV = (SMEM > NW * QKV_REGION) ? SMEM : NW * QKV_REGION;
  // GroupNorm partials are summed per 64-row unit = two 32-row blocks of a wave tile (gemm_epilogue_core<GN>): a tile whose wave
  // rows are an odd number of blocks would compile the sums out and leave the caller's buffer unwritten
  static_assert((BM / WM / 32) % 2 == 0, "this tile cannot write GroupNorm partials");
  const int nbm = (p.M - p.m_begin + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  dim3 grid(nbm * nbn), block(NW * 64);
  const int epi = pick_epilogue(p);
  if (epi == EPI_QKV)     // (the fused head split lives in the 16x16x32 kernels only; the planner refuses it on a convolution)
    return launch_kernel<ld_gemm_kernel<BM, BN, WM, WN, NSTAGE, false, EPI_QKV, true>>("ld_gemm_qkv_heads", grid, block, SMEM_QKV, stream, p);
  // 16x16x32 MFMAs by default (LD_GEMM_M16=0: the 32x32x16 form, kept for A/B measurements): +7...11 % on the DiT shapes
  static int k_m16 = LD_KNOB_UNSET;
  auto go = [&](auto m16, auto conv_c, auto e) {
    return launch_kernel<ld_gemm_kernel<BM, BN, WM, WN, NSTAGE, decltype(conv_c)::value, decltype(e)::value, decltype(m16)::value>>(
        decltype(m16)::value ? "ld_gemm16" : "ld_gemm", grid, block, SMEM, stream, p);
  };
  auto by_epilogue = [&](auto m16) {
    if (conv) return with_epilogue<EPI_BIAS>(epi, [&](auto e) { return go(m16, std::true_type{}, e); });
    return with_epilogue<EPI_BIAS, EPI_GELU, EPI_GATE>(epi, [&](auto e) { return go(m16, std::false_type{}, e); });
  };
  return ld_knob("LD_GEMM_M16", 1, &k_m16) ? by_epilogue(std::true_type{}) : by_epilogue(std::false_type{});
}

}  // namespace

int launch_2stage_128(const GemmParams& p, bool conv, hipStream_t stream) { return launch_cfg<128, 128, 2, 2, 2>(p, conv, stream); }
int launch_2stage_256(const GemmParams& p, bool conv, hipStream_t stream) { return launch_cfg<256, 256, 2, 4, 2>(p, conv, stream); }

// fp8 operands (per-row scales, or MXFP8 when p.mx_a is set) on 256 x 256 tiles: ld_gemm_f8_kernel
int launch_2stage_f8(const GemmParams& p, bool, hipStream_t stream) {
  constexpr int STAGE = (256 + 256) * 128;
  constexpr int EPIB = 8 * 32 * CW_STRIDE * 4;
  constexpr int SMEM = ((2 * STAGE > EPIB) ? 2 * STAGE : EPIB) + 4096;      // + the MX scale strips of both stages
  const int nbm = (p.M + 255) / 256, nbn = (p.N + 255) / 256;
  dim3 grid(nbm * nbn), block(512);
  if (p.mx_a)
    return with_epilogue<EPI_BIAS, EPI_GELU, EPI_GATE, EPI_GELU_MX>(pick_epilogue(p), [&](auto e) {
      return launch_kernel<ld_gemm_f8_kernel<decltype(e)::value, true>>("ld_gemm_mxfp8", grid, block, SMEM, stream, p);
    });
  return with_epilogue<EPI_BIAS, EPI_GELU, EPI_GATE>(pick_epilogue(p), [&](auto e) {
    return launch_kernel<ld_gemm_f8_kernel<decltype(e)::value, false>>("ld_gemm_fp8", grid, block, SMEM, stream, p);
  });
}

#ifdef LD_VARIANTS
int launch_w4r(const GemmParams& p, bool, hipStream_t stream) {
  constexpr int SMEM = 2 * (256 + 256) * 64 * 2;   // two 64 KB K-tile slots (the epilogue staging reuses them)
  const int nbm = (p.M - p.m_begin + 255) / 256, nbn = (p.N + 255) / 256;
  dim3 grid(nbm * nbn), block(256);
  return with_epilogue<EPI_BIAS, EPI_GELU, EPI_GATE>(pick_epilogue(p), [&](auto e) {
    return launch_kernel<ld_gemm_w4r_kernel<decltype(e)::value>>("ld_gemm_w4r", grid, block, SMEM, stream, p);
  });
}
#endif

}  // namespace ldgemm
