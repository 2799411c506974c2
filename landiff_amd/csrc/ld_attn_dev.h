// Device pieces that the pipelined attention kernels are assembled from (ld_attn_q64_body.h, ld_attn_p16.hip and, in the variants
// build, ld_attn_q128.hip and ld_attn_pipe.hip): the layout of the workgroup's LDS, the K/V ring's LDS-DMA plan, the fragment read
// offsets and key indices of the 16x16x32 layout, the fast pass's window test with the workgroup vote, the DMA drain and the O
// epilogue.  Each rule is stated here once; a kernel body keeps its own pipeline.  Include after ld_attn.h.
//
// These kernels have no register to spare, so every piece is a forceinline function of VALUES: what a piece needs per lane is
// passed in, and nothing here keeps a per-lane value alive that its caller did not already hold.  The shapes below are the ones
// that left every kernel's VGPR / scratch / occupancy where it was (tools/kernel_resources.sh; the notes at attn_load_qt and
// attn_store_o say what did not).  What stays in the kernel files on purpose: ld_attn_p16.hip restates AttnDma's setup in place (set
// up by a function, its 4-wave kernel spills 52 more bytes); the running-max step of the safe pass is written per kernel (the score
// tile is [b][qb] in q64, [kb][qb] in p16, and q128 pins its order with asm statements and wait states: one text would be mostly
// adaptor); ld_attn_pipe.hip keeps the fragment load, offsets, masks and epilogue of its 32x32x16 layout.
#pragma once
#include "ld_attn.h"

namespace {

// ---- LDS of a workgroup: K slots 0..3 | V^T slots 0..3 (8 KB each) | per-wave flag words | the dynamic form's broadcast word ----
constexpr int ATTN_VBASE = 4 * KTILE_BYTES;                 // the V^T slots
constexpr int ATTN_FLAGS_OFF = 8 * KTILE_BYTES;             // NW (<= 8) words: "a row of this wave left the fast pass's window"
constexpr int ATTN_BCAST_OFF = ATTN_FLAGS_OFF + 32;         // dynamic q64 form: the block index thread 0 pulled
constexpr int ATTN_SMEM_BYTES = ATTN_FLAGS_OFF + 64;        // what every launcher asks for

// The fast pass's window: a row's denominator l = sum_k exp2(s_k) must lie in [2^-80, 2^110] (the argument is in the header
// comment of ld_attn_pipe.hip).
constexpr float ATTN_L_MIN = 8.2718061e-25f;                // 2^-80
constexpr float ATTN_L_MAX = 1.2980742e33f;                 // 2^110

template <int I> using IC = std::integral_constant<int, I>;
template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) { f(IC<I>{}); static_for<N, I + 1>(f); }
}

// 16-byte chunk c of row r of a tile image lives at chunk c ^ f(r).  V^T rows (and the K rows of the 32x32x16 kernel, whose K
// fragments read rows in order): f = bits 3:1.  The K rows of the 16x16x32 kernels are read permuted (ld_attn_p16.hip), for which
// bit 1 | bits 4:3 << 1 is the conflict-free key.
__device__ __forceinline__ int attn_swz_v(int r) { return (r >> 1) & 7; }
__device__ __forceinline__ int attn_swz_k(int r) { return ((r >> 1) & 1) | (((r >> 3) & 3) << 1); }
struct AttnSwzK16 { static __device__ __forceinline__ int f(int r) { return attn_swz_k(r); } };   // 16x16x32 kernels
struct AttnSwzK32 { static __device__ __forceinline__ int f(int r) { return attn_swz_v(r); } };   // ld_attn_pipe.hip

// Where workgroup `bid` (remapped block index) works: head bh = (b, h), its Q / K / V^T, and the first query row q0 of wave `wave`.
// past: the whole block lies past Nq (the caller returns).
struct AttnBlock {
  int b, h, q0;
  const bf16_t *Qb, *Kb, *Vb;
  bool past;
};
__device__ __forceinline__ AttnBlock attn_block(const AttnParams& p, int bid, int rows_wg, int rows_wave, int wave) {
  const int nqb = (p.Npad + rows_wg - 1) / rows_wg;
  const int bh = bid / nqb, qblk = bid - bh * nqb;
  AttnBlock k;
  k.b = bh / p.H; k.h = bh - k.b * p.H;
  k.Qb = p.Q + (long)bh * p.Npad * D;
  k.Kb = p.K + (long)bh * p.Npad * D;
  k.Vb = p.Vt + (long)bh * D * p.Npad;
  k.q0 = qblk * rows_wg + wave * rows_wave;
  k.past = qblk * rows_wg >= p.Nq;
  return k;
}

// One Q^T fragment (B operand of the 16x16x32 QK^T): row q (clamped to Npad - 1: such rows are never stored), d = ks*32 + h4*8 ..
// + 8, pre-multiplied by scale * log2(e) and RNE-packed.
__device__ __forceinline__ u32x4_t attn_qt_frag(const AttnParams& p, const bf16_t* Qb, int q, int h4, int ks) {
  const u32x4_t raw = *(const u32x4_t*)(Qb + (long)(q < p.Npad ? q : p.Npad - 1) * D + h4 * 8 + ks * 32);
  u32x4_t sc;
#pragma unroll
  for (int e = 0; e < 4; ++e) sc[e] = pack_bf16x2(bf_lo(raw[e]) * p.c, bf_hi(raw[e]) * p.c);
  return sc;
}
// The wave's fragments, rows q0 + qb*16 + l16: sink(qb, ks, words) takes each.  (Plain unrolled loops, not static_for: with the
// compile-time form ld_attn_q64_dyn_kernel spilled 8 more bytes.  A sink that needs qb / ks as constants -- ld_attn_q128.hip --
// walks attn_qt_frag itself.)
template <int NQB, class Sink>
__device__ __forceinline__ void attn_load_qt(const AttnParams& p, const bf16_t* Qb, int q0, int l16, int h4, Sink&& sink) {
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) sink(qb, ks, attn_qt_frag(p, Qb, q0 + qb * 16 + l16, h4, ks));
}

// The ring's LDS-DMA plan of one wave.  The first half of the NW waves brings K tiles (rows = keys), the second half V^T tiles
// (rows = d): a tile is sixteen 1 KB pieces of eight 128-byte rows, NPW of them per wave; a piece is one buffer_load ... lds with the
// tile offset in an SGPR and a loop-invariant per-lane offset (no VALU address arithmetic in the loops).  The LDS image is
// lane-linear; the swizzle is applied to the source address.  SWZK: the K rows' swizzle key (AttnSwzK16 / AttnSwzK32).
template <int NW, class SWZK>
struct AttnDma {
  static constexpr int NPW = 16 / NW;             // pieces per wave and tile
  __amdgpu_buffer_rsrc_t rsrc;                    // K or V^T of this head: raw buffer, wave-uniform
  int tstride;                                    // bytes per tile step in the source
  uint32_t goff[NPW];                             // per lane: byte offset of its 16 bytes of piece i inside a tile
  int ldsoff[NPW];                                // wave-uniform: piece i inside a slot (V^T: + ATTN_VBASE)

  __device__ __forceinline__ AttnDma(const bf16_t* Kb, const bf16_t* Vb, int Npad, int wave, int lane) {
    const bool kwave = wave < NW / 2;
    rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(kwave ? Kb : Vb), 0, 0x7fffffff, 0x00020000);
    tstride = kwave ? KT * D * 2 : KT * 2;
    const int rstride = kwave ? D : Npad;
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
      const int piece = (wave % (NW / 2)) * NPW + i;
      const int r = piece * 8 + (lane >> 3);
      const int chunk = (lane & 7) ^ (kwave ? SWZK::f(r) : attn_swz_v(r));
      goff[i] = (uint32_t)(r * rstride + chunk * 8) * 2u;
      ldsoff[i] = (kwave ? 0 : ATTN_VBASE) + piece * 1024;
    }
  }
  __device__ __forceinline__ void piece(char* smem, int i, int slot, int t) const {      // piece i of source tile t -> slot
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(smem + slot * KTILE_BYTES + ldsoff[i]),
                                             16, goff[i], t * tstride, 0, 0);
  }
  __device__ __forceinline__ void tile(char* smem, int slot, int t) const {
#pragma unroll
    for (int i = 0; i < NPW; ++i) piece(smem, i, slot, t);
  }
};

// Fragment read offsets of the 16x16x32 layout.  K block 2*kg + b, k-step ks: kofs[ks] + slot*8K + kg*4096 + b*512 (lane l16 reads
// the permuted key row 8*(l16 >> 2) + (l16 & 3)); V^T block db, key group kg: vofs[kg] + slot*8K + db*2048.  kbase / vbase: what
// the caller's addresses start from (byte offsets into smem: 0 and ATTN_VBASE).
template <class T>
__device__ __forceinline__ void attn_frag_offsets(int l16, int h4, T kbase, T vbase, T (&kofs)[2], T (&vofs)[2]) {
  const int key = 8 * (l16 >> 2) + (l16 & 3);
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int c = ks * 4 + h4;
    kofs[ks] = kbase + key * 128 + ((c ^ attn_swz_k(key)) << 4);
    vofs[ks] = vbase + l16 * 128 + ((c ^ attn_swz_v(l16)) << 4);
  }
}

// Which key a score register holds (the K-row permutation of ld_attn_p16.hip): register r of S^T block bb of half hh (tile
// hh >> 1, key group hh & 1) in a lane of 16-lane group h4 is key attn_key0(hh, bb, h4) + r.  Every ragged-tail mask derives from it.
__device__ __forceinline__ int attn_key0(int hh, int bb, int h4) { return (hh >> 1) * KT + (hh & 1) * 32 + h4 * 8 + bb * 4; }

// keys of half hh at or past nk -> -inf-like scores (s[bb][qb]: the [2][NQB] score tile of a half)
template <int NQB>
__device__ __forceinline__ void attn_mask_half(f32x4_t (&s)[2][NQB], int hh, int h4, int nk) {
#pragma unroll
  for (int bb = 0; bb < 2; ++bb) {
    const int key0 = attn_key0(hh, bb, h4);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (key0 + r >= nk) {
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) s[bb][qb][r] = NEG_BIG;
      }
  }
}

// After a fast pass: did any stored row of the WORKGROUP leave the window (NaN fails too)?  l[qb]: the denominator of row
// qrow + qb*16 of this lane.  Each wave leaves its answer in its flag word (the dynamic q64 form counts them: ld_attn_q64.hip),
// every wave reads all NW: the whole workgroup takes the safe pass together, whose loop has workgroup barriers.
template <int NW, int NQB>
__device__ __forceinline__ bool attn_window_vote(char* smem, const float (&l)[NQB], int qrow, int Nq, int lane, int wave) {
  bool bad = false;
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb)
    bad = bad || (!(l[qb] >= ATTN_L_MIN && l[qb] <= ATTN_L_MAX) && (qrow + qb * 16 < Nq));
  int* flags = (int*)(smem + ATTN_FLAGS_OFF);
  const bool wbad = __any(bad);
  if (lane == 0) flags[wave] = wbad ? 1 : 0;
  __syncthreads();
  bool redo = false;
#pragma unroll
  for (int w = 0; w < NW; ++w) redo = redo || flags[w] != 0;
  __syncthreads();
  return redo;
}

// Every LDS-DMA of this workgroup has LANDED before the workgroup ends: the loops run ahead of the tiles they consume (and, where
// they have no peeled tail, request tiles nobody reads); a wave that ended with buffer_load ... lds in flight would let the data
// arrive in LDS that may by then belong to the next workgroup on this CU.  (Round 5: added while hunting the co-residency bug
// that turned out to be the packed-fp32 one -- csrc/build.sh -- and kept: it measures at 0 us of a 3.6 ms launch.)
__device__ __forceinline__ void attn_dma_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// O epilogue of the O^T [db][qb] accumulator layout (16 d x 16 q blocks), one 16-row query block: row q of this lane gets
// d = db*16 + h4*4 .. + 4 as 1/l times o<db>, RNE-packed into one 8-byte store each.  A row whose denominator is not positive is
// stored as zeros; rows at or past Nq are not stored.  (Per block and by value, not a loop over a source: as one function over the
// whole [4][NQB] tile, by array or by accessor, ld_attn_q64_exact_kernel spilled 20 to 56 more bytes.)
__device__ __forceinline__ void attn_store_o(const AttnParams& p, int b, int h, int q, int h4, float l,
                                             const f32x4_t& o0, const f32x4_t& o1, const f32x4_t& o2, const f32x4_t& o3) {
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  if (q < p.Nq) {
    bf16_t* orow = p.O + (long)b * p.o_bs + (long)q * p.o_rs + h * D + h4 * 4;
    auto put = [&](int db, const f32x4_t& o4) {
      u32x2_t w2;
      w2[0] = pack_bf16x2(o4[0] * inv, o4[1] * inv);
      w2[1] = pack_bf16x2(o4[2] * inv, o4[3] * inv);
      *(u32x2_t*)(orow + db * 16) = w2;
    };
    put(0, o0); put(1, o1); put(2, o2); put(3, o3);
  }
}

}  // namespace
