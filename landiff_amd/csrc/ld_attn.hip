// Flash-style fused attention for gfx950, head_dim 64, bf16 in / fp32 accumulate / bf16 out.
//
// Replaces:
//   sat attention_fn_default -> F.scaled_dot_product_attention on the joint text+video sequence
//   (landiff/diffusion/dit_video_concat.py:636-664; called from :587,:1308), and
//   flex_attention(block_mask=VideoDecoderMask) in the TiTok decoder
//   (landiff/tokenizer/modules/blocks.py:172-212; mask landiff/tokenizer/modules/flex_attention_mask.py:193-335,
//   whose closed form is  allowed(q,kv) <=> fid[kv] <= fid[q]  -- SURVEY.md Appendix B).
//
// MI355X-first structure:
//   * one workgroup = 4 wave64 = 128 query rows (32 per wave); K and V^T tiles of 64 keys are
//     brought HBM->LDS by LDS-DMA (global_load_lds_dwordx4), double buffered, one barrier/tile.
//   * S^T = K Q^T with v_mfma_f32_32x32x16_bf16 ("swapped" product): a lane then owns ONE query
//     column (lane&31) and 32 of the 64 keys, so the softmax row reductions are lane-local
//     plus a single exchange with lane^32 (v_permlane32_swap).
//   * the K rows fed to the MFMA are permuted (bits 2<->3 of the row index swapped in the LDS
//     read address -- free), which makes the 8 accumulator registers [8*ks .. 8*ks+7] exactly
//     the 8 consecutive keys the PV MFMA wants as its B fragment: no cross-lane traffic, no
//     P round trip through LDS.
//   * V is consumed as V^T [d][key] (written in that layout by the qkv-split kernel), so the
//     PV A-fragment is a plain ds_read_b128; O^T accumulates per (d-row, q-column) and the
//     online-softmax rescale is a per-lane scalar multiply.
//   * LDS tiles are lane-linear (DMA) with the 16-B chunk XOR-swizzled by ((row>>1)&7) on the
//     source address and on the read: conflict-free ds_read_b128.
//   * frame-block mask: per-KV-tile [min,max] frame ids let a workgroup skip fully masked
//     tiles (no load, no MFMA) and apply the element mask only on the few straddling tiles.
#include "ld_attn.h"

#ifndef LD_ATTN_PLAIN_WPS
#define LD_ATTN_PLAIN_WPS 3      // register budget (waves per SIMD) of the default instantiation
#endif
#define LD_STR_(x) #x
#define LD_STR(x) LD_STR_(x)

namespace {

__device__ __forceinline__ void glds16(const bf16_t* g, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)g,
      (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// v_max3_f32 by hand: plain fmaxf on MFMA outputs makes hipcc insert a canonicalising v_max per operand.  CAUTION: an asm statement
// gets no hazard padding -- when the operands are MFMA results the caller provides the MFMA -> VALU wait states (below)
__device__ __forceinline__ float max3f(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

template <bool MFMASUM, int WPS>   // WPS = waves/SIMD of the register budget
__global__ __launch_bounds__(256, WPS) void ld_attn_kernel(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 stages of one key tile (K 8 KB + V^T 8 KB) + 64 B
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;
  const int nqb = p.Npad / QB;
  const int nkt_all = (p.Nk + KT - 1) / KT;

  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = bid / nqb, qb = bid - bh * nqb;
  const int b = bh / p.H, h = bh - b * p.H;

  const bf16_t* Qb = p.Q + (long)bh * p.Npad * D;
  const bf16_t* Kb = p.K + (long)bh * p.Npad * D;
  const bf16_t* Vb = p.Vt + (long)bh * D * p.Npad;

  const int q = qb * QB + wave * 32 + (lane & 31);   // this lane's query row
  if (qb * QB >= p.Nq) return;                        // whole block past the end (uniform)

  // ---- frame ids of the queries; block/wave ranges ----
  const bool masked = p.fid_k != nullptr;
  int qfid = 0, wqmin = 0, wqmax = 0, bqmax = 0;
  if (masked) {
    const int qc = q < p.Nq ? q : p.Nq - 1;
    qfid = p.fid_q[qc];
    int mn = qfid, mx = qfid;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn = min(mn, __shfl_xor(mn, o, 64));
      mx = max(mx, __shfl_xor(mx, o, 64));
    }
    wqmin = mn; wqmax = mx;
    int* red = (int*)(smem + 2 * STAGE_BYTES);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    bqmax = max(max(red[0], red[1]), max(red[2], red[3]));
  }

  // ---- Q fragments (B operand of K Q^T): lane = query column, 8 consecutive d per k-step ----
  // Q is pre-multiplied by softmax_scale*log2(e) (one extra bf16 rounding of q, 2^-9 relative) so that the MFMA
  // accumulator is directly the exp2 argument: started at -m (running max, log2 units) it needs no per-element FMA.
  bf16x8_t qf[4];
  {
    const bf16_t* qrow = Qb + (long)q * D + hi * 8;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const u32x4_t raw = *(const u32x4_t*)(qrow + kk * 16);
      u32x4_t sc;
#pragma unroll
      for (int e = 0; e < 4; ++e) sc[e] = pack_bf16x2(bf_lo(raw[e]) * p.c, bf_hi(raw[e]) * p.c);
      qf[kk] = __builtin_bit_cast(bf16x8_t, sc);
    }
  }

  // ---- LDS-DMA source offsets: waves 0,1 stage K (rows = keys), waves 2,3 stage V^T (rows = d) ----
  long goff[4];
  int ldsoff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = wave * 4 + i;            // 0..15 (1 KB pieces of one 64-key tile)
    const int r = (idx & 7) * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((r >> 1) & 7);
    if (idx < 8) goff[i] = (long)r * D + chunk * 8;          // + kv0 * D
    else goff[i] = (long)r * p.Npad + chunk * 8;             // + kv0
    ldsoff[i] = (idx < 8 ? 0 : KTILE_BYTES) + (idx & 7) * 1024;
  }
  auto stage = [&](int buf, int t) {            // a stage is one key tile
    char* base = smem + buf * STAGE_BYTES;
    const long kv0 = (long)t * KT;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = wave * 4 + i;
      const bf16_t* src = (idx < 8) ? (Kb + kv0 * D + goff[i]) : (Vb + kv0 + goff[i]);
      glds16(src, base + ldsoff[i]);
    }
  };
  auto tile_needed = [&](int t) {               // can some query of the workgroup see a key of tile t?
    if (!masked) return true;
    return t < nkt_all && p.kt_min[t] <= bqmax;   // (the bound is the caller's too: stated twice, as the instruction stream was tuned)
  };
  auto next_tile = [&](int t) {
    ++t;
    while (t < nkt_all && !tile_needed(t)) ++t;
    return t;
  };

  // fragment read byte offsets within a 64-key tile, one per (row block i, k-step): loop invariant, so the
  // per-tile LDS addressing is just "register + immediate" (the stage/buffer offsets are compile-time constants)
  int kofs[4], vofs[4];       // row block i = 1 is +32 rows = +4096 B with the same swizzle key: an immediate offset
  {
    const int key = swap23(lane & 31);
    const int d = lane & 31;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int c = kk * 2 + hi;
      kofs[kk] = key * 128 + ((c ^ ((key >> 1) & 7)) << 4);
      vofs[kk] = KTILE_BYTES + d * 128 + ((c ^ ((d >> 1) & 7)) << 4);
    }
  }

  f32x16_t o[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
  // running max m (log2 units) lives negated in a 16-register block that is the C operand of the first QK^T MFMA;
  // it only changes in the rare rescale branch (deferred: P may grow to 2^THR before we rescale)
  f32x16_t negm;
#pragma unroll
  for (int r = 0; r < 16; ++r) negm[r] = 0.f;
  float negm0 = 0.f;                 // scalar copy used by the lean-register (WPS >= 4) form
  float lsum = 0.f;
  // MFMASUM: the softmax denominator comes out of the matrix pipe (an all-ones A fragment times P), not from 32 VALU adds
  f32x16_t lacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) lacc[r] = 0.f;
  const bf16x8_t ones = {0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80};
  bool unset = true;                 // no valid key seen yet for this query
  constexpr float THR = 8.0f;        // deferred rescale: P may grow to 2^THR before the running max is rebased

  auto tile = [&](auto bufc, int t) {
    constexpr int OFF = decltype(bufc)::value * STAGE_BYTES;
    bool skip = false, need_mask = false;
    if (masked) {
      const int tmin = p.kt_min[t], tmax = p.kt_max[t];
      skip = tmin > wqmax;
      need_mask = tmax > wqmin;
    } else {
      need_mask = (t + 1) * KT > p.Nk;
    }
    if (skip) return;
    // ---- S^T = K Q^T: all 8 K fragments are requested up front (one exposed LDS latency per tile, not four);
    //      the first k-step uses the inline-constant 0 as C, so the accumulators are never zeroed by VALU moves ----
    f32x16_t sacc[2];
    if (WPS >= 4) {
      // lean-register form (<= 128 VGPRs, 4 waves/SIMD): C starts at the inline constant 0, K fragments in two halves
      const f32x16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        bf16x8_t kh[2][2];
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
          for (int i = 0; i < 2; ++i) kh[i][k2] = *(const bf16x8_t*)(smem + kofs[half * 2 + k2] + OFF + i * 4096);
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            sacc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh[i][k2], qf[half * 2 + k2],
                                                              (half == 0 && k2 == 0) ? zero16 : sacc[i], 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[i][r] += negm0;        // S' - m_old
    } else {
    bf16x8_t kf[2][4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int i = 0; i < 2; ++i) kf[i][kk] = *(const bf16x8_t*)(smem + kofs[kk] + OFF + i * 4096);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
        sacc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[i][kk], qf[kk], kk == 0 ? negm : sacc[i], 0, 0, 0);
    }
    }
    // V^T fragments for the PV product: requested now so their LDS latency hides under the softmax VALU work
    bf16x8_t vf[2][4];
    if (WPS < 4) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i) vf[i][ks] = *(const bf16x8_t*)(smem + vofs[ks] + OFF + i * 4096);
    }
    // register r of sacc[i] holds key  t*64 + i*32 + (r>>3)*16 + hi*8 + (r&7)
    auto apply_mask = [&]() {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const int key0 = t * KT + i * 32 + g * 16 + hi * 8;
          if (masked) {
            const int4 f0 = *(const int4*)(p.fid_k + key0);
            const int4 f1 = *(const int4*)(p.fid_k + key0 + 4);
            const int f[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (f[e] > qfid) sacc[i][g * 8 + e] = NEG_BIG;
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (key0 + e >= p.Nk) sacc[i][g * 8 + e] = NEG_BIG;
          }
        }
    };
    if (need_mask) apply_mask();
    // ---- online softmax (per query column; lane and lane^32 share the row) ----
    // max3f is an asm statement and its operands are MFMA results: hipcc pads the MFMA -> VALU read hazard only for instructions it
    // knows, so the wait states go here, in a statement that names the accumulators (round 6: the same helper right behind its
    // MFMAs in ld_attn_q64.hip's row-maximum pass read OLD accumulator values now and then -- run-to-run differences of one ulp)
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(sacc[0]), "+v"(sacc[1]));
    float mx = max3f(sacc[0][0], sacc[1][0], sacc[0][1]);
    mx = max3f(mx, sacc[1][1], sacc[0][2]);
#pragma unroll
    for (int r = 2; r < 15; ++r) mx = max3f(mx, sacc[1][r], sacc[0][r + 1]);
    mx = fmaxf(mx, sacc[1][15]);
    mx = lane32_max(mx);            // = max_k(S') - m_old for this query (S' in log2 units)
    const bool valid = mx > -1.0e29f;                       // at least one unmasked key in this tile
    if (!__all(!(valid && (unset || mx > THR)))) {
      // rare: (re)base the running max.  d = how much m grows for this lane; everything held at the old max scales by 2^-d
      const float d = valid ? (unset ? mx : fmaxf(mx, 0.0f)) : 0.0f;
      unset = unset && !valid;
      const float alpha = __builtin_amdgcn_exp2f(-d);
      lsum *= alpha;
      if (MFMASUM) lacc[0] *= alpha;                       // only row 0 of the ones-product is ever read
      if (WPS >= 4) negm0 -= d;
      else {
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[r] -= d;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { o[i][r] *= alpha; sacc[i][r] -= d; }
    }
    float psum = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(sacc[i][r]);
        sacc[i][r] = pv;
        if (!MFMASUM) psum += pv;
      }
    lsum += psum;
    // ---- O^T += V^T P^T ----
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      u32x4_t pw;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        pw[e] = pack_bf16x2(sacc[ks >> 1][(ks & 1) * 8 + 2 * e], sacc[ks >> 1][(ks & 1) * 8 + 2 * e + 1]);
      const bf16x8_t pb = __builtin_bit_cast(bf16x8_t, pw);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bf16x8_t va = (WPS >= 4) ? *(const bf16x8_t*)(smem + vofs[ks] + OFF + i * 4096) : vf[i][ks];
        o[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pb, o[i], 0, 0, 0);
      }
      if (MFMASUM) lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, pb, lacc, 0, 0, 0);
    }
  };
  // (a forwarding level kept on purpose: with tile() called from the loop directly hipcc allocates the registers of all three
  //  instantiations differently, and this kernel's instruction stream is what was measured)
  auto stage_tile = [&](auto bufc, int t) { tile(bufc, t); };

  // two tiles per trip with compile-time buffer indices; the second half sits under an `if`, not behind a `break`
  // (a mid-loop exit makes hipcc keep two copies of the O accumulators and shuffle them every trip)
  int t = next_tile(-1);
  if (t < nkt_all) stage(0, t);
  while (t < nkt_all) {
    int tn = next_tile(t);
    __syncthreads();
    if (tn < nkt_all) stage(1, tn);
    stage_tile(std::integral_constant<int, 0>{}, t);
    t = tn;
    if (t < nkt_all) {
      tn = next_tile(t);
      __syncthreads();
      if (tn < nkt_all) stage(0, tn);
      stage_tile(std::integral_constant<int, 1>{}, t);
      t = tn;
    }
  }

  // ---- finalize: O = O^T / l, write bf16 rows ----
  const float ltot = MFMASUM ? lacc[0] : lane32_sum(lsum);
  const float inv = ltot > 0.f ? 1.0f / ltot : 0.f;
  if (q < p.Nq) {
    bf16_t* orow = p.O + (long)b * p.o_bs + (long)q * p.o_rs + h * D;
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

}  // namespace

// ---- what the calling thread's last launch ran: written by attn_run alone ----
static thread_local AttnRan g_attn_ran = {"", nullptr, 0};

// name of the kernel the calling thread's last ld_attn_fwd_bf16 launched (bench.py labels its roofline object with it)
LD_API const char* ld_attn_last_kernel(void) { return g_attn_ran.name; }

LD_API int ld_attn_last_fallbacks(int32_t* out, void* stream) {
  LD_REQUIRE(out, "ld_attn_last_fallbacks: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  if (g_attn_ran.fb_kind == 1) e = hipMemcpyAsync(out, g_attn_ran.fb_src, 4, hipMemcpyDeviceToDevice, st);
  else e = hipMemsetAsync(out, g_attn_ran.fb_kind == 2 ? 0xFF : 0, 4, st);
  if (e != hipSuccess) return ld_set_error(LD_ERR_LAUNCH, "ld_attn_last_fallbacks: %s", hipGetErrorString(e));
  return LD_OK;
}

// ---- the plan: which kernel a problem gets.  Shapes and knobs only, never the HIP runtime (ld_attn_route runs it dry). ----
enum { ATTN_PLAIN = 0, ATTN_Q64 = 1, ATTN_Q64_EXACT = 2, ATTN_Q64_WIN = 3, ATTN_P16 = 4, ATTN_Q128 = 5, ATTN_PIPE2 = 6 };   // (ld_attn_route, landiff_hip.h)
enum AttnForm { FORM_DEFAULT = 0, FORM_EXACT = 1, FORM_WINDOW = 2 };       // ld_attn_fwd_bf16 / _exact / _window

struct AttnPlan {
  int route = ATTN_PLAIN;               // < 0: an error code, message set, nothing to launch
  int safe = 0, msum = 1, nw = 4, npre = 44, variant = 0;
  bool want_dyn = false;
  int win[3] = {0, 0, 0};               // ATTN_Q64_WIN: {prefix, group, frames}
};

static int attn_window_too_short(int64_t nkt) {
  return ld_set_error(LD_ERR_UNSUPPORTED, "ld_attn_fwd_bf16_window: %ld key tiles; the pipelined kernel needs at least %d", (long)nkt,
                      ATTN_PIPELINED_MIN_TILES);
}

// The LD_ATTN_* knobs, all read here and through ld_knob (once per process, or per call under LD_TUNING=1: ld_common.h):
//   LD_ATTN_VARIANT  0  0 = the pipelined 16x16x32 kernels below for every unmasked problem of >= ATTN_PIPELINED_MIN_TILES key tiles,
//                       else the plain kernel; 9 = the plain kernel everywhere; 1 / 4 = the plain kernel with row sums on the matrix
//                       pipe / in its lean-register 4-waves form; 8 = the round-1 pipelined 32x32x16 kernel of ld_attn_pipe.hip for
//                       tile counts 4 m + 2 (variants build only: the shipped library runs the plain kernel)
//   LD_ATTN_Q64      1  0 = the 32-query-row wave tile of ld_attn_p16.hip instead of the 64-row one of ld_attn_q64.hip
//   LD_ATTN_Q128     0  (variants build only) 1 = the 128-row, one-wave-per-SIMD tile of ld_attn_q128.hip for problems with enough
//                       query rows to fill the chip with its 512-row workgroups; 2 = for every pipelined problem
//   LD_ATTN_SAFE     0  1 = the pipelined kernels run their running-max pass (testing, A/B timing)
//   LD_ATTN_DYN      1  0 = q64: the hardware's round-robin dispatch of one workgroup per query block, not the dynamic form (which
//                       the launcher takes for grids of at least four rounds of the chip's slots when the stream allows it)
//   LD_ATTN_MSUM     1  0 = p16: the row sums by v_add_f32, not on the matrix pipe (A/B timing)
//   LD_ATTN_NW       4  8 = p16 / pipe2: 8-wave workgroups (halve the K/V traffic per CU, measure the same: 4.44 vs 4.46 ms)
//   LD_ATTN_NPRE    44  q128: 36 | 52 the other exp2 splits, 1036 | 1040 with the packs under the PV phase (A/B timing)
// The exact form is decided before LD_ATTN_VARIANT / LD_ATTN_Q64, and the window form goes to the q64 window kernels whatever
// they say: there is no other kernel for either.
static AttnPlan attn_plan(const AttnParams& p, AttnForm form, const int* win) {
  static int k_var = LD_KNOB_UNSET, k_q64 = LD_KNOB_UNSET, k_safe = LD_KNOB_UNSET, k_dyn = LD_KNOB_UNSET, k_msum = LD_KNOB_UNSET,
             k_nw = LD_KNOB_UNSET;
  AttnPlan pl;
  pl.variant = ld_knob("LD_ATTN_VARIANT", 0, &k_var);
  pl.safe = ld_knob("LD_ATTN_SAFE", 0, &k_safe);
  pl.want_dyn = ld_knob("LD_ATTN_DYN", 1, &k_dyn) > 0 && !pl.safe;
  pl.msum = ld_knob("LD_ATTN_MSUM", 1, &k_msum);
  pl.nw = ld_knob("LD_ATTN_NW", 4, &k_nw) == 8 ? 8 : 4;      // (anything but 8 is 4)
  const bool q64 = ld_knob("LD_ATTN_Q64", 1, &k_q64) != 0;
  const int64_t nkt = ((int64_t)p.Nk + KT - 1) / KT;
  const bool pipelined = !p.fid_k && nkt >= ATTN_PIPELINED_MIN_TILES;
  auto to = [&](int route) { pl.route = route; return pl; };
  if (form == FORM_WINDOW) {
    for (int i = 0; i < 3; ++i) pl.win[i] = win ? win[i] : 0;
    return to(nkt < ATTN_PIPELINED_MIN_TILES ? attn_window_too_short(nkt) : ATTN_Q64_WIN);
  }
  const bool exact = form == FORM_EXACT;
#ifdef LD_VARIANTS
  static int k_q128 = LD_KNOB_UNSET, k_npre = LD_KNOB_UNSET;
  const int q128 = ld_knob("LD_ATTN_Q128", 0, &k_q128);
  pl.npre = ld_knob("LD_ATTN_NPRE", 44, &k_npre);
  if (pl.variant == 0 && !exact && pipelined && (q128 == 2 || (q128 == 1 && (int64_t)p.B * p.H * ((p.Npad + 511) / 512) >= 512)))
    return to(ATTN_Q128);
#endif
  // exact form: the two-pass kernel where the pipelined tile applies; every other shape takes the plain kernel, whose online
  // softmax is exact for any logit range already
  if (exact && pipelined) return to(ATTN_Q64_EXACT);
  if (pl.variant == 0 && pipelined && q64 && !exact) return to(ATTN_Q64);
  if (pl.variant == 0 && pipelined && !exact) return to(ATTN_P16);        // any tile count
#ifdef LD_VARIANTS
  if (pl.variant == 8 && !exact && pipelined && (nkt - 2) % 4 == 0) return to(ATTN_PIPE2);   // (the round-1 kernel: tile counts 4 m + 2)
#endif
  return to(ATTN_PLAIN);       // by pl.variant: ld_attn_kernel<false,3> | <true,2> (1) | <false,4> (4)
}

static int attn_plain_launch(const AttnParams& p, hipStream_t st, int variant, AttnRan* ran) {
  auto launch = [&](void (*kernel)(AttnParams), const char* name) {
    *ran = {name, nullptr, 0};                   // a running-max kernel: no window to leave
    hipLaunchKernelGGL(kernel, dim3((unsigned)((int64_t)p.B * p.H * (p.Npad / QB))), dim3(256), 2 * STAGE_BYTES + 64, st, p);
    return ld_check_launch("ld_attn_fwd_bf16");
  };
  if (variant == 1) return launch(ld_attn_kernel<true, 2>, "ld_attn_kernel<true,2>");
  if (variant == 4) return launch(ld_attn_kernel<false, 4>, "ld_attn_kernel<false,4>");
  return launch(ld_attn_kernel<false, LD_ATTN_PLAIN_WPS>, "ld_attn_kernel<false," LD_STR(LD_ATTN_PLAIN_WPS) ">");
}

// Executes a plan: one launcher call, and the one place that records what ran (a launcher that fails before its launch reports
// nothing, and the record stays what it was).
static int attn_run(const AttnPlan& pl, const AttnParams& p, hipStream_t st) {
  if (pl.route < 0) return pl.route;
  AttnRan ran = {nullptr, nullptr, 0};
  int rc;
  switch (pl.route) {
    case ATTN_Q64: rc = ld_attn_q64_launch(p, st, nullptr, pl.safe, pl.want_dyn, &ran); break;
    case ATTN_Q64_WIN: rc = ld_attn_q64_launch(p, st, pl.win, pl.safe, pl.want_dyn, &ran); break;
    case ATTN_Q64_EXACT: rc = ld_attn_q64_exact_launch(p, st, &ran); break;
    case ATTN_P16: rc = ld_attn_p16_launch(p, st, pl.safe, pl.msum, pl.nw, &ran); break;
#ifdef LD_VARIANTS
    case ATTN_Q128: rc = ld_attn_q128_launch(p, st, pl.safe, pl.npre, &ran); break;
    case ATTN_PIPE2: rc = ld_attn_pipe2_launch(p, st, pl.safe, pl.nw, &ran); break;
#endif
    default: rc = attn_plain_launch(p, st, pl.variant, &ran); break;
  }
  if (ran.name) g_attn_ran = ran;
  return rc;
}

// the shape rules (`who` names the entry point in the messages): pure, so that ld_attn_route answers with the launch's own messages
static int attn_check_shape(const char* who, AttnForm form, int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t Npad) {
  LD_REQUIRE(B > 0 && H > 0 && Nq > 0 && Nk > 0, "%s: empty problem", who);
  LD_REQUIRE(Npad % QB == 0 && Npad >= Nq && Npad >= Nk, "%s: Npad=%ld must be a multiple of %d and >= %s", who, (long)Npad, QB,
             form == FORM_WINDOW ? "N" : "Nq,Nk");
  if (form == FORM_WINDOW) LD_REQUIRE(B * H * ((Npad + 255) / 256) < (1LL << 31), "%s: grid too large", who);
  return LD_OK;
}

// What the three entry points share: pointers, shapes, mask tables and alignment checked (in this order: the first failure names
// itself), the parameter block filled, the plan made and run.
static int attn_fwd(const char* who, AttnForm form, const int* win, const void* Q, const void* K, const void* Vt, void* O,
                    int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t Npad, int64_t o_batch_stride, int64_t o_row_stride,
                    float softmax_scale, const int32_t* fid_q, const int32_t* fid_k, const int32_t* kt_min, const int32_t* kt_max, void* stream) {
  LD_REQUIRE(Q && K && Vt && O, "%s: null pointer", who);
  if (int rc = attn_check_shape(who, form, B, H, Nq, Nk, Npad)) return rc;
  LD_REQUIRE((fid_q == nullptr) == (fid_k == nullptr), "%s: fid_q and fid_k go together", who);
  LD_REQUIRE(!fid_k || (kt_min && kt_max), "%s: masked attention needs kt_min/kt_max", who);
  LD_REQUIRE(o_row_stride % 4 == 0 && ((uintptr_t)O & 7) == 0, "%s: output alignment", who);
  AttnParams p{};
  p.Q = (const bf16_t*)Q; p.K = (const bf16_t*)K; p.Vt = (const bf16_t*)Vt; p.O = (bf16_t*)O;
  p.B = (int)B; p.H = (int)H; p.Nq = (int)Nq; p.Nk = (int)Nk; p.Npad = (int)Npad;
  p.o_bs = o_batch_stride; p.o_rs = o_row_stride;
  p.c = softmax_scale * 1.4426950408889634f;
  p.fid_q = fid_q; p.fid_k = fid_k; p.kt_min = kt_min; p.kt_max = kt_max;
  return attn_run(attn_plan(p, form, win), p, (hipStream_t)stream);
}

LD_API int ld_attn_fwd_bf16(const void* Q, const void* K, const void* Vt, void* O,
                            int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t Npad,
                            int64_t o_batch_stride, int64_t o_row_stride, float softmax_scale,
                            const int32_t* fid_q, const int32_t* fid_k,
                            const int32_t* kt_min, const int32_t* kt_max, void* stream) {
  return attn_fwd("ld_attn_fwd_bf16", FORM_DEFAULT, nullptr, Q, K, Vt, O, B, H, Nq, Nk, Npad, o_batch_stride, o_row_stride, softmax_scale, fid_q, fid_k, kt_min, kt_max, stream);
}

LD_API int ld_attn_fwd_bf16_exact(const void* Q, const void* K, const void* Vt, void* O,
                                  int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t Npad,
                                  int64_t o_batch_stride, int64_t o_row_stride, float softmax_scale,
                                  const int32_t* fid_q, const int32_t* fid_k,
                                  const int32_t* kt_min, const int32_t* kt_max, void* stream) {      // (one operation with ld_attn_fwd_bf16: its messages carry that name)
  return attn_fwd("ld_attn_fwd_bf16", FORM_EXACT, nullptr, Q, K, Vt, O, B, H, Nq, Nk, Npad, o_batch_stride, o_row_stride, softmax_scale, fid_q, fid_k, kt_min, kt_max, stream);
}

// ---- frame-window attention: every 256-row query block walks the prefix tiles and the tiles of the frames within `window` of its
// own (attn_window_block, ld_attn.h).  Host side: arguments, the plan, the refusals. ----

// The arguments of a window problem, checked and clamped (G to N, w to the frame count: the same plan, no overflow).  Pure.
static int attn_window_args(const char* who, int64_t N, int64_t P, int64_t* G, int64_t* w) {
  LD_REQUIRE(N > 0 && N < (1 << 28), "%s: N=%ld outside (0, 2^28)", who, (long)N);
  LD_REQUIRE(P >= 0 && P <= N, "%s: prefix=%ld outside [0, N=%ld]", who, (long)P, (long)N);
  LD_REQUIRE(*G >= 1, "%s: group=%ld (tokens per frame) must be >= 1", who, (long)*G);
  LD_REQUIRE(*w >= 0, "%s: window=%ld (frames each side) must be >= 0", who, (long)*w);
  attn_window_clamp(N, P, G, w);
  return LD_OK;
}

LD_API int ld_attn_window_plan(int64_t N, int64_t prefix, int64_t group, int64_t window, int64_t block,
                               int32_t* t_lo, int32_t* t_hi, int32_t* n_eff) {
  LD_REQUIRE(t_lo && t_hi && n_eff, "ld_attn_window_plan: null pointer");
  if (int rc = attn_window_args("ld_attn_window_plan", N, prefix, &group, &window)) return rc;
  LD_REQUIRE(block >= 0 && block < (N + 255) / 256, "ld_attn_window_plan: block %ld of %ld", (long)block, (long)((N + 255) / 256));
  int lo, hi, ne;
  attn_window_block((int)N, (int)prefix, (int)group, (int)window, (int)block, &lo, &hi, &ne);
  *t_lo = lo; *t_hi = hi; *n_eff = ne;
  return LD_OK;
}

LD_API int ld_attn_fwd_bf16_window(const void* Q, const void* K, const void* Vt, void* O,
                                   int64_t B, int64_t H, int64_t N, int64_t Npad,
                                   int64_t o_batch_stride, int64_t o_row_stride, float softmax_scale,
                                   int64_t prefix, int64_t group, int64_t window, void* stream) {
  // the window's own rules first (pure host arithmetic: a caller may probe a shape without a device)
  if (int rc = attn_window_args("ld_attn_fwd_bf16_window", N, prefix, &group, &window)) return rc;
  const int64_t n = (N + KT - 1) / KT, pt = (prefix + KT - 1) / KT;
  if (n < ATTN_PIPELINED_MIN_TILES) return attn_window_too_short(n);
  for (int64_t b = 0; b < (N + 255) / 256; ++b) {
    int lo, hi, ne;
    attn_window_block((int)N, (int)prefix, (int)group, (int)window, (int)b, &lo, &hi, &ne);
    if (ne < ATTN_PIPELINED_MIN_TILES)
      return ld_set_error(LD_ERR_UNSUPPORTED, "ld_attn_fwd_bf16_window: query block %ld would walk %d key tiles (prefix %ld, group %ld, window %ld); "
                          "the pipelined kernel needs at least %d", (long)b, ne, (long)prefix, (long)group, (long)window, ATTN_PIPELINED_MIN_TILES);
    if (!(lo >= pt && lo <= hi && hi <= n))     // (cannot happen: the rule keeps every list inside [0, n))
      return ld_set_error(LD_ERR_INVALID, "ld_attn_fwd_bf16_window: block %ld: tile range [%d, %d) outside [%ld, %ld]", (long)b, lo, hi, (long)pt, (long)n);
  }
  const int win[3] = {(int)prefix, (int)group, (int)window};
  return attn_fwd("ld_attn_fwd_bf16_window", FORM_WINDOW, win, Q, K, Vt, O, B, H, N, N, Npad, o_batch_stride, o_row_stride, softmax_scale,
                  nullptr, nullptr, nullptr, nullptr, stream);
}

// The plan run dry: the route code of the kernel family a launch of these shapes would take (landiff_hip.h), or the launch's own
// refusal.  No HIP call.
LD_API int ld_attn_route(int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t Npad, int32_t masked, int32_t form) {
  LD_REQUIRE(form >= FORM_DEFAULT && form <= FORM_WINDOW, "ld_attn_route: form %d is not 0 (default), 1 (exact) or 2 (window)", (int)form);
  const char* who = form == FORM_WINDOW ? "ld_attn_fwd_bf16_window" : "ld_attn_fwd_bf16";
  if (form == FORM_WINDOW) {
    LD_REQUIRE(!masked && Nq == Nk, "ld_attn_route: there is no masked or rectangular (Nq=%ld, Nk=%ld) window form", (long)Nq, (long)Nk);
    int64_t one_frame = Nk > 0 ? Nk : 1, every = 0;         // (the sequence alone: the window's own numbers are ld_attn_window_plan's)
    if (int rc = attn_window_args(who, Nk, 0, &one_frame, &every)) return rc;
  }
  if (int rc = attn_check_shape(who, (AttnForm)form, B, H, Nq, Nk, Npad)) return rc;
  static const int32_t some_mask = 0;       // (the plan only asks whether there is a mask)
  AttnParams p{};
  p.B = (int)B; p.H = (int)H; p.Nq = (int)Nq; p.Nk = (int)Nk; p.Npad = (int)Npad;
  if (masked) p.fid_q = p.fid_k = &some_mask;
  return attn_plan(p, (AttnForm)form, nullptr).route;
}
