// Software-pipelined attention main loop for the unmasked DiT shape (joint text+video attention, head_dim 64).
// Replaces the same reference op as ld_attn.hip (sat attention_fn_default -> F.scaled_dot_product_attention,
// landiff/diffusion/dit_video_concat.py:636-664).  Own translation unit: built with -fno-slp-vectorize (hipcc otherwise
// packs scalar fp32 adds into v_pk_add_f32, which measured slower next to MFMAs).
//
// What bounds this kernel on MI355X is the SIMD's VALU issue port, not the matrix pipe: per 64-key tile a wave issues 16
// MFMAs (32 cycles of pipe each, ~16 cycles of port each) and, in the textbook online-softmax form, ~110 VALU
// instructions (32 v_exp_f32 at ~8 cycles, the rest at 4): ~820 port cycles against 512 pipe cycles
// (profiles/r01_attn_pmc_*.txt).  Two things follow:
//
//  1. Pipelining.  Every MFMA of the loop has VALU / LDS work of a *different* tile issued behind it in program order, so
//     one in-order wave keeps the matrix pipe and the VALU port busy at the same time (2 waves/SIMD):
//
//       iteration j:  first 8 MFMAs   S_{j+1} = K_{j+1} Q^T   ||  exp2 of S_j[keys 0:32], V_j fragments <- LDS,
//                                                                  LDS-DMA of K_{j+5} / V_{j+3}
//                     next 8-12 MFMAs O += V_j P_j (+ row sums) ||  exp2 of S_j[keys 32:64], bf16 packing of P_j,
//                                                                  K_{j+2} fragments <- LDS  [safe form: max(S_{j+1})]
//
//     The order inside an iteration is pinned gap by gap with sched_barrier(0).
//
//  2. Less VALU work per score (FAST form).  softmax(s) = exp2(s) / sum exp2(s) needs no running maximum as long as
//     nothing overflows or underflows, so the fast pass starts the QK^T accumulators at the inline constant 0, never
//     computes a maximum, and takes the row sums from the matrix pipe (an all-ones A fragment times P: 4 more MFMAs
//     instead of 32 VALU adds per tile).  When it ends, each row's denominator l = sum_k exp2(s_k) is checked against
//     [2^-80, 2^110]: inside that window no term that matters (down to 2^-46 of the row maximum) was flushed and nothing
//     overflowed, so the result is the exact softmax up to rounding.  A workgroup in which any row fails the test
//     (|q.k| * scale * log2(e) beyond ~+-100 -- not seen with LayerNormed q, k) recomputes with the SAFE pass: the same
//     pipeline with the running maximum, the deferred rescale and VALU row sums.
//
// LDS: four K slots and four V^T slots of 8 KB (tile t in slot t & 3; 64 KB per workgroup, 2 workgroups per CU).
// Iterations come in pairs ("periods") with ONE workgroup barrier per pair: period m = iterations 2m, 2m+1 reads V_2m,
// V_2m+1, K_2m+2, K_2m+3 and, in its first iteration, issues the LDS-DMA of V_2m+2, V_2m+3, K_2m+4, K_2m+5 into the four
// slots that period m-1 finished reading.  RAW: every wave drains its own DMA pieces (vmcnt(0)) before the barrier that
// ends the period; the next period reads them.  WAR: lgkmcnt(0) before the same barrier retires the period's ds_reads
// before any wave refills those slots.  The DMA itself is buffer_load ... lds with the tile offset in an SGPR (soffset)
// and a loop-invariant per-lane voffset: no VALU address arithmetic in the loop.
#include "ld_attn.h"
#include "ld_attn_dev.h"

namespace {

#define FENCE() __builtin_amdgcn_sched_barrier(0)

template <int NW>     // waves per workgroup (32 query rows each): 4 (two workgroups per CU) or 8 (one)
__device__ __forceinline__ void attn_pipe2_body(const AttnParams& p, int force_safe, char* smem) {   // smem: K slots 0..3 | V^T slots 0..3 | NW flag words
  constexpr int VBASE = ATTN_VBASE;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;
  const int n = (p.Nk + KT - 1) / KT;             // >= 6 and (n - 2) % 4 == 0 (launcher)

  const AttnBlock blk = attn_block(p, xcd_remap(blockIdx.x, gridDim.x), NW * 32, 32, wave);
  const int q = blk.q0 + (lane & 31);
  if (blk.past) return;

  bf16x8_t qf[4];
  {
    const bf16_t* qrow = blk.Qb + (long)(q < p.Npad ? q : p.Npad - 1) * D + hi * 8;   // rows past Npad (NW = 8) are never stored
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const u32x4_t raw = *(const u32x4_t*)(qrow + kk * 16);
      u32x4_t sc;
#pragma unroll
      for (int e = 0; e < 4; ++e) sc[e] = pack_bf16x2(bf_lo(raw[e]) * p.c, bf_hi(raw[e]) * p.c);
      qf[kk] = __builtin_bit_cast(bf16x8_t, sc);
    }
  }

  // LDS-DMA: the first half of the waves brings K tiles, the second half V^T tiles (the K rows are read in order here: AttnSwzK32)
  const bool kwave = wave < NW / 2;
  const AttnDma<NW, AttnSwzK32> ring(blk.Kb, blk.Vb, p.Npad, wave, lane);
  constexpr int NPW = decltype(ring)::NPW;
  auto dma_piece = [&](int i, int slot, int t) { ring.piece(smem, i, slot, t); };
  auto dma = [&](int slot, int t) { ring.tile(smem, slot, t); };

  int kofs[4], vofs[4];
  {
    const int key = swap23(lane & 31);
    const int d = lane & 31;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int c = kk * 2 + hi;
      kofs[kk] = key * 128 + ((c ^ ((key >> 1) & 7)) << 4);
      vofs[kk] = VBASE + d * 128 + ((c ^ ((d >> 1) & 7)) << 4);
    }
  }

  f32x16_t o[2];
  using T = std::true_type; using F = std::false_type;
  using S0 = std::integral_constant<int, 0>; using S1 = std::integral_constant<int, 1>;
  using S2 = std::integral_constant<int, 2>; using S3 = std::integral_constant<int, 3>;

  // One whole pass over the keys; returns this lane's softmax denominator (FAST: complete; SAFE: the lane's half).
  auto pass = [&](auto fast_c) -> float {
    constexpr bool FAST = decltype(fast_c)::value;
    constexpr bool MSUM = false;   // FAST row sums on the matrix pipe: measured 6 % slower than the 32 VALU adds (4.80 vs 4.51 ms)
    constexpr float THR = 8.0f;
    const f32x16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bf16x8_t ones = {0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80};
    f32x16_t acc0 = zero16;      // FAST: row sums from the matrix pipe;  SAFE: -(running max), the C operand of QK^T
    float ls0 = 0.f, ls1 = 0.f;  // SAFE: two partial row sums
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
    f32x16_t sA[2], sB[2];
    bf16x8_t kf[2][4], vf[2][4];

    auto load_kf = [&](int slot) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int i = 0; i < 2; ++i) kf[i][kk] = *(const bf16x8_t*)(smem + kofs[kk] + slot * KTILE_BYTES + i * 4096);
    };
    // SAFE: running-max bookkeeping on a finished score tile (the branch is rare after the first tiles)
    auto rebase_if = [&](f32x16_t (&s)[2], float mx, bool first) {
      mx = lane32_max(mx);
      if (!__all(!(first || mx > THR))) {
        const float d = first ? mx : fmaxf(mx, 0.0f);
        const float alpha = __builtin_amdgcn_exp2f(-d);
        ls0 *= alpha; ls1 *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] -= d;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) { o[i][r] *= alpha; s[i][r] -= d; }
      }
    };
    auto mask_tail = [&](f32x16_t (&s)[2], int t) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const int key0 = t * KT + i * 32 + g * 16 + hi * 8;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (key0 + e >= p.Nk) s[i][g * 8 + e] = NEG_BIG;
        }
    };
    auto tile_max = [&](const f32x16_t (&s)[2]) {
      float m0 = fmaxf(s[0][0], s[0][1]), m1 = fmaxf(s[1][0], s[1][1]);
#pragma unroll
      for (int r = 2; r < 16; r += 2) { m0 = fmaxf(fmaxf(m0, s[0][r]), s[0][r + 1]); m1 = fmaxf(fmaxf(m1, s[1][r]), s[1][r + 1]); }
      return fmaxf(m0, m1);
    };

    // One pipelined iteration.  sc = S_j, sn receives S_{j+1}.  HAS_QK: tile j+1 exists; HAS_K2: tile j+2 exists (a main-loop
    // iteration); MASK: tile j+1 is the ragged one.  Even main-loop iterations issue the period's eight DMA pieces (past the
    // end the tile index is clamped, which re-fetches tile n-1 into a slot nobody reads); odd iterations end the period.
    auto iter = [&](f32x16_t (&sc)[2], f32x16_t (&sn)[2], int j, auto vslot_c, auto has_qk_c, auto has_k2_c, auto mask_c) {
      constexpr int vslot = decltype(vslot_c)::value;            // slot of V_j; the others follow from it
      constexpr int k2slot = (vslot + 2) & 3;
      constexpr bool HAS_QK = decltype(has_qk_c)::value, HAS_K2 = decltype(has_k2_c)::value, MASK = decltype(mask_c)::value;
      constexpr bool EVEN = (vslot & 1) == 0;
      constexpr bool do_dma = HAS_K2 && EVEN;
      // even iteration j = 2m: V_j+2, V_j+3 go to V slots (j + 2) & 3, (j + 3) & 3; K_j+4, K_j+5 to K slots j & 3, (j + 1) & 3
      int dt0 = kwave ? j + 4 : j + 2, dt1 = dt0 + 1;
      dt0 = dt0 < n ? dt0 : n - 1; dt1 = dt1 < n ? dt1 : n - 1;
      const int dslot0 = kwave ? vslot : (vslot + 2) & 3, dslot1 = kwave ? (vslot + 1) & 3 : (vslot + 3) & 3;
      u32x4_t pw[4];
      float m0 = NEG_BIG, m1 = NEG_BIG;
      auto EXP2 = [&](int i, int r) {        // two scores -> probabilities (SAFE: + row sums)
        sc[i][r] = __builtin_amdgcn_exp2f(sc[i][r]);
        sc[i][r + 1] = __builtin_amdgcn_exp2f(sc[i][r + 1]);
        if (!(FAST && MSUM)) { ls0 += sc[i][r]; ls1 += sc[i][r + 1]; }
      };
      auto EXP1 = [&](int i, int r) { sc[i][r] = __builtin_amdgcn_exp2f(sc[i][r]); if (!(FAST && MSUM)) ls0 += sc[i][r]; };
      auto CVT2 = [&](int ks, int e) {       // two of the four packed words of P fragment ks
        pw[ks][e] = pack_bf16x2(sc[ks >> 1][(ks & 1) * 8 + 2 * e], sc[ks >> 1][(ks & 1) * 8 + 2 * e + 1]);
        pw[ks][e + 1] = pack_bf16x2(sc[ks >> 1][(ks & 1) * 8 + 2 * e + 2], sc[ks >> 1][(ks & 1) * 8 + 2 * e + 3]);
      };
      auto MAX4 = [&](float& m, int i, int r) {
        if (FAST || !HAS_QK) return;
        m = fmaxf(fmaxf(m, sn[i][r]), sn[i][r + 1]); m = fmaxf(fmaxf(m, sn[i][r + 2]), sn[i][r + 3]);
      };
      auto VF = [&](int g) { vf[g & 1][g >> 1] = *(const bf16x8_t*)(smem + vofs[g >> 1] + vslot * KTILE_BYTES + (g & 1) * 4096); };
      auto KF = [&](int g) { if (HAS_K2) kf[g & 1][g >> 1] = *(const bf16x8_t*)(smem + kofs[g >> 1] + k2slot * KTILE_BYTES + (g & 1) * 4096); };
      auto QK = [&](int g) {                 // g = kk * 2 + i
        if (HAS_QK) sn[g & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[g & 1][g >> 1], qf[g >> 1],
                                                                       (g >> 1) == 0 ? (FAST ? zero16 : acc0) : sn[g & 1], 0, 0, 0);
      };
      auto PV = [&](int g) {                 // g = ks * 2 + i
        o[g & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[g & 1][g >> 1], __builtin_bit_cast(bf16x8_t, pw[g >> 1]), o[g & 1], 0, 0, 0);
      };
      auto SUM = [&](int ks) {               // FAST: row sums of P fragment ks on the matrix pipe
        if (FAST && MSUM) acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, __builtin_bit_cast(bf16x8_t, pw[ks]), acc0, 0, 0, 0);
      };
      // ---- QK^T of tile j+1 over exp2 of the first 32 keys of tile j ----
      auto DMA = [&](int g) {                 // gap g of an even main-loop iteration: piece g of the period's 2 * NPW
        if (do_dma && g < 2 * NPW) dma_piece(g % NPW, g < NPW ? dslot0 : dslot1, g < NPW ? dt0 : dt1);
      };
      QK(0); EXP2(0, 0);  VF(0); DMA(0); FENCE();
      QK(1); EXP2(0, 2);  VF(1); DMA(1); FENCE();
      QK(2); EXP2(0, 4);  VF(2); DMA(2); FENCE();
      QK(3); EXP2(0, 6);  VF(3); DMA(3); FENCE();
      QK(4); EXP2(0, 8);  VF(4); DMA(4); FENCE();
      QK(5); EXP2(0, 10); VF(5); DMA(5); FENCE();
      QK(6); EXP2(0, 12); VF(6); CVT2(0, 0); DMA(6); FENCE();
      QK(7); EXP2(0, 14); VF(7); CVT2(0, 2); DMA(7); FENCE();
      if (MASK) mask_tail(sn, j + 1);
      if (FAST && MSUM) {
        // ---- PV + row sums (12 MFMAs) over exp2 of the last 32 keys ----
        PV(0);  EXP2(1, 0);  CVT2(1, 0); FENCE();
        PV(1);  EXP2(1, 2);  CVT2(1, 2); FENCE();
        SUM(0); EXP2(1, 4);  FENCE();
        PV(2);  EXP2(1, 6);  FENCE();
        PV(3);  EXP2(1, 8);  CVT2(2, 0); KF(0); FENCE();
        SUM(1); EXP2(1, 10); CVT2(2, 2); KF(1); FENCE();
        PV(4);  EXP2(1, 12); KF(2); FENCE();
        PV(5);  EXP2(1, 14); KF(3); FENCE();
        SUM(2); CVT2(3, 0);  CVT2(3, 2); KF(4); FENCE();
        PV(6);  KF(5); FENCE();
        PV(7);  KF(6); FENCE();
        SUM(3); KF(7); FENCE();
      } else {
        // ---- PV (8 MFMAs) over exp2 of the last 32 keys and the maximum of tile j+1 ----
        PV(0); EXP2(1, 0);  EXP1(1, 2);  CVT2(1, 0); KF(0); FENCE();
        PV(1); EXP2(1, 3);  EXP1(1, 5);  CVT2(1, 2); KF(1); MAX4(m0, 0, 0); FENCE();
        PV(2); EXP2(1, 6);  EXP1(1, 8);  CVT2(2, 0); KF(2); MAX4(m0, 0, 4); FENCE();
        PV(3); EXP2(1, 9);  EXP1(1, 11); CVT2(2, 2); KF(3); MAX4(m0, 0, 8); FENCE();
        PV(4); EXP2(1, 12); CVT2(3, 0);  KF(4); MAX4(m0, 0, 12); FENCE();
        PV(5); EXP2(1, 14); CVT2(3, 2);  KF(5); MAX4(m1, 1, 0); FENCE();
        PV(6); KF(6); MAX4(m1, 1, 4); MAX4(m1, 1, 8); FENCE();
        PV(7); KF(7); MAX4(m1, 1, 12); FENCE();
        if constexpr (!FAST && HAS_QK) rebase_if(sn, fmaxf(m0, m1), false);   // (FAST: no maximum exists -- keep the dead test out of the loop)
      }
      // ---- end of a period (odd iteration): retire this wave's LDS reads and DMA pieces, then the barrier.
      //      (the builtin, unlike inline asm, is visible to hipcc's own wait-count bookkeeping: no redundant waits follow)
      if (!EVEN) {
        __builtin_amdgcn_s_waitcnt(0x0070);          // vmcnt(0) lgkmcnt(0)
        __builtin_amdgcn_s_barrier();
      }
      FENCE();
    };

    // ---- prologue: K0..K3, V0, V1 land; S_0 from K0; K_1 fragments ----
    if (kwave) { dma(0, 0); dma(1, 1); dma(2, 2); dma(3, 3); }
    else { dma(0, 0); dma(1, 1); }
    __builtin_amdgcn_s_waitcnt(0x0070);
    __builtin_amdgcn_s_barrier();
    FENCE();
    load_kf(0);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int i = 0; i < 2; ++i)
        sA[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[i][kk], qf[kk], kk == 0 ? zero16 : sA[i], 0, 0, 0);
    FENCE();
    load_kf(1);
    if (!FAST) rebase_if(sA, tile_max(sA), true);
    __builtin_amdgcn_s_waitcnt(0x0070);
    __builtin_amdgcn_s_barrier();        // every wave has K0 / K1 in registers: period 0 may refill their slots
    FENCE();

    // ---- main loop: iterations j = 0 .. n-3 (tiles j+1 and j+2 exist, tile j+1 is never the ragged one) ----
    int j = 0;
    for (; j + 4 <= n - 2; j += 4) {
      iter(sA, sB, j,     S0{}, T{}, T{}, F{});
      iter(sB, sA, j + 1, S1{}, T{}, T{}, F{});
      iter(sA, sB, j + 2, S2{}, T{}, T{}, F{});
      iter(sB, sA, j + 3, S3{}, T{}, T{}, F{});
    }
    // the two final iterations (j = n-2: masks tile n-1 if ragged, no K fragments to fetch; j = n-1: only finishes tile n-1)
    if (n * KT > p.Nk) iter(sA, sB, j, S0{}, T{}, F{}, T{});
    else iter(sA, sB, j, S0{}, T{}, F{}, F{});
    iter(sB, sA, j + 1, S1{}, F{}, F{}, F{});
    return (FAST && MSUM) ? acc0[0] : lane32_sum(ls0 + ls1);
  };

  float ltot = 0.f;
  bool redo = force_safe != 0;
  if (!redo) {
    ltot = pass(T{});
    // 2^-80 <= l <= 2^110 (ATTN_L_MIN / ATTN_L_MAX; NaN fails): see the header comment
    const float l1[1] = {ltot};
    redo = attn_window_vote<NW, 1>(smem, l1, q, p.Nq, lane, wave);
  }
  if (redo) ltot = pass(F{});
  attn_dma_drain();

  const float inv = ltot > 0.f ? 1.0f / ltot : 0.f;
  if (q < p.Nq) {
    bf16_t* orow = p.O + (long)blk.b * p.o_bs + (long)q * p.o_rs + blk.h * D;   // (the 32x32 layout: its own epilogue)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = i * 32 + 8 * g + 4 * hi;
        u32x2_t w2;
        w2[0] = pack_bf16x2(o[i][4 * g + 0] * inv, o[i][4 * g + 1] * inv);
        w2[1] = pack_bf16x2(o[i][4 * g + 2] * inv, o[i][4 * g + 3] * inv);
        *(u32x2_t*)(orow + d0) = w2;
      }
  }
}
#undef FENCE

// (non-template entry points: hipcc emitted no host stub for the kernel when it was itself the template)
__global__ __launch_bounds__(256, 2) void ld_attn_pipe2_w4_kernel(AttnParams p, int force_safe) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  attn_pipe2_body<4>(p, force_safe, smem);
}
__global__ __launch_bounds__(512, 2) void ld_attn_pipe2_w8_kernel(AttnParams p, int force_safe) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  attn_pipe2_body<8>(p, force_safe, smem);
}

}  // namespace

// nw = 4 | 8: the workgroup size in waves
int ld_attn_pipe2_launch(const AttnParams& p, hipStream_t st, int safe, int nw, AttnRan* ran) {
  static thread_local LdSmemCache c4{}, c8{};
  const int qbw = nw * 32;
  dim3 grid((unsigned)((long)p.B * p.H * ((p.Npad + qbw - 1) / qbw)));
  if (nw == 4) return attn_launch(ld_attn_pipe2_w4_kernel, &c4, ATTN_SMEM_BYTES, grid, dim3(256), st, ran,
                                  attn_ran_static(ATTN_KNAMES(ld_attn_pipe2_w4_kernel), safe), "ld_attn_fwd_bf16(pipe2)", p, safe);
  return attn_launch(ld_attn_pipe2_w8_kernel, &c8, ATTN_SMEM_BYTES, grid, dim3(512), st, ran,
                     attn_ran_static(ATTN_KNAMES(ld_attn_pipe2_w8_kernel), safe), "ld_attn_fwd_bf16(pipe2)", p, safe);
}
