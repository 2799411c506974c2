// fp8 (OCP e4m3) GEMMs for the DiT's large linear layers: MXFP8 operands on the persistent 8-phase loop (ld_gemm8p_mx_kernel), the
// two quantisers, and the fp8 / MXFP8 entry points.  (Per-row scaled and MXFP8 operands on the two-stage loop: ld_gemm_f8_kernel,
// ld_gemm_2stage.hip.)
// ld_gemm.h: what the GEMM files share; ld_gemm_8p_dev.h: the raster, addresses, MFMA section and derived counted waits that
// ld_gemm8p_mx_kernel takes from the bf16 8-phase kernels.
#include "ld_gemm_8p_dev.h"
#include "../../include/landiff_hip.h"

namespace ldgemm {
int fill_epilogue(GemmParams& p, const ld_epilogue_t* e);     // ld_gemm.hip
namespace {

// ------------------------------------------------------------------------------------------------
// MXFP8 operands on the persistent loop of ld_gemm8p_kernel (round 6; BASELINE configs[4]).  A K-tile of 128 e4m3 elements is a
// 128-byte row, exactly the bf16 kernel's 64-element row: the same eight 16 KB half-tile slots, the same per-lane LDS-DMA offsets
// (in bytes), the same XOR swizzle, the same two phases of the K-tile with the two wave rows one barrier apart, the same persistent
// tile walk, next-tile request from inside the epilogue and the same epilogues (incl. the fused qkv head split and the MXFP8-writing
// GELU epilogue), because v_mfma_scale_f32_16x16x128_f8f6f4 leaves its 16 x 16 block in the registers of v_mfma_f32_16x16x32_bf16.
// What changes:
//   * one MFMA per accumulator block and K-tile (32 per wave, ~32 cycles each) instead of two; its 32-byte operand is the PAIR of
//     16-byte fragments the bf16 loop reads for its two k-steps -- lane (r, g) holds k = 16 g .. + 16 and 64 + 16 g .. + 16 of row r
//     (tools/probe/fp8_mfma16_layout.hip: layout D1) -- so the fragment reads are the bf16 kernel's, address for address;
//   * block scales: one E8M0 byte per row and 32 K elements, [K / 128][rows][4] in memory (ld_quantize_mxfp8).  A K-tile's 256 + 256
//     row dwords travel by 4-byte LDS-DMA next to A_0 / B_0 (waves 0-3: A rows, 4-7: W rows) into a 2 KB strip per K-tile buffer; in
//     P0 a lane reads the dwords of its 8 + 4 block rows and keeps byte g (the hardware takes block g's scale from lane group g:
//     scale layout S0) of each, packed four to a register -- the MFMA's op_sel picks the byte.
// LDS: [K-tile buffer 0: 64 KB][scale strips: 2 x 2 KB][K-tile buffer 1: 64 KB]; the epilogue staging at the end of the 160 KB stays
// clear of buffer 0 and the strips.
// From ld_gemm_8p_dev.h: the raster, the swizzle and fragment addresses, bar(), mfma_section and the waits of StagePlan<2, 2, 1>.
// The tile source (with its scale strip), the K-tile and the tile walk below stay this kernel's own text, although they restate
// ktile_2phase / tile_main_loop / walk_tiles: built from those, with equal barrier, MFMA and counted-wait counts and no scratch, the
// K = 1920 GEMMs of this kernel measured 2-3 % slower than the parent build (143 -> 148..150 us at 35552 x 1920 x 1920, outside the
// spread of two files of the parent build), the only arms of profiles/gemm_refactor.txt to do so.
// ------------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512, 2) void ld_gemm8p_mx_kernel(GemmParams p) {
  constexpr int BM = 256, BN = 256, KB = 128;             // KB: bytes (= e4m3 elements) of K per tile
  constexpr int SLOT = 128 * 128, KBUF = 4 * SLOT;
  constexpr int SC_OFF = KBUF, SC_BYTES = 4096;           // [buffer][A rows 1 KB | W rows 1 KB]
  constexpr int BUF1 = KBUF + SC_BYTES;                   // byte offset of K-tile buffer 1
  constexpr int EPI_BYTES = (EPI == EPI_QKV) ? 8 * QKV_REGION : 8 * 32 * CW_STRIDE * 4;
  constexpr int EPI_OFF = (LD_LDS_TOTAL - EPI_BYTES) & ~15;
  constexpr bool PREFETCH = EPI_OFF >= BUF1 && EPI != EPI_QKV;
  constexpr bool SWAPACC = EPI != EPI_QKV;
  using Plan = StagePlan<2, 2, 1>;                        // LDS-DMA instructions per wave: a half-tile = 2, a scale strip = 1
  static_assert(BUF1 + KBUF <= LD_LDS_TOTAL, "LDS layout");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  const int ntiles = nbm * nbn;
  auto origin = [&](int v, int& m0, int& n0) { tile_origin<BM, BN>(v, nbm, nbn, p.group_m, 0, m0, n0); };
  const long ldab = p.lda, ldwb = p.K;                    // row strides in bytes
  struct Src { const unsigned char* a; const unsigned char* w; const unsigned char* s; int a_bytes, w_bytes, s_bytes; };
  const bool a_wave = wave < 4;                           // which operand's scale dwords this wave fetches
  const long srows = a_wave ? p.M : p.N;
  auto tile_src = [&](int m0, int n0) {
    Src s;
    s.a = (const unsigned char*)p.A + (long)m0 * ldab;
    s.w = (const unsigned char*)p.W + (long)n0 * ldwb;
    s.a_bytes = clip((long)(p.M - m0) * ldab);
    s.w_bytes = clip((long)(p.N - n0) * ldwb);
    const long so = a_wave ? m0 : n0;
    s.s = (a_wave ? p.mx_a : p.mx_w) + so * 4;            // rows past M / N read as zero scale bytes (their products are never stored)
    s.s_bytes = clip(((long)(p.K >> 7) * srows - so) * 4);
    return s;
  };
  // [piece] byte offsets of half 0 (the bf16 kernel's rows and swizzle); half 1 = + 64 rows of A / + 32 rows of W, added per use by
  // an asm statement the compiler cannot hoist: with four more offset registers live through the K loop the gated-residual and
  // GELU instantiations spilled one of them, and the reload's s_waitcnt vmcnt(0) drained the LDS-DMA queue once per K-tile
  uint32_t offA[2], offW[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int lr = wave * 16 + i * 8 + (lane >> 3);
    const int chunk = swz_chunk(lane, lr);
    const int tm = (lr >> 6) * 128 + (lr & 63);
    const int tn = (lr >> 5) * 64 + (lr & 31);
    offA[i] = (uint32_t)((long)tm * ldab + chunk * 16);
    offW[i] = (uint32_t)((long)tn * ldwb + chunk * 16);
  }
  const int dA1 = (int)(64 * ldab), dW1 = (int)(32 * ldwb);
  auto half_off = [](uint32_t o, int d, auto hc) -> uint32_t {
    if constexpr (decltype(hc)::value == 0) return o;
    uint32_t r;
    asm volatile("v_add_u32 %0, %1, %2" : "=v"(r) : "v"(o), "s"(d));
    return r;
  };
  const uint32_t offS = (uint32_t)(((wave & 3) * 64 + lane) * 4);     // this lane's row dword of the strip
  const int sslab = (int)(srows * 4);                     // bytes between consecutive K-tiles' scale slabs
  const int nk = p.K / KB;
  char* const my_piece = smem + wave * 2048;
  Src src;
  auto stage_a = [&](const Src& s, auto bufc, auto hc, int kt) {
    constexpr int OFF = (decltype(bufc)::value ? BUF1 : 0) + decltype(hc)::value * SLOT;
    stage_pieces<OFF>((const bf16_t*)s.a, s.a_bytes, my_piece, half_off(offA[0], dA1, hc), half_off(offA[1], dA1, hc), kt * KB);
  };
  auto stage_w = [&](const Src& s, auto bufc, auto gc, int kt) {
    constexpr int OFF = (decltype(bufc)::value ? BUF1 : 0) + (2 + decltype(gc)::value) * SLOT;
    stage_pieces<OFF>((const bf16_t*)s.w, s.w_bytes, my_piece, half_off(offW[0], dW1, gc), half_off(offW[1], dW1, gc), kt * KB);
  };
  auto stage_s = [&](const Src& s, auto bufc, int kt) {     // 256 B per wave: the 64 row dwords (waves 0-3: A rows, 4-7: W rows)
    constexpr int OFF = SC_OFF + decltype(bufc)::value * 2048;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)s.s, 0, s.s_bytes, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(smem + OFF + wave * 256), 4, offS, kt * sslab, 0, 0);
  };
  auto stage_ktile0 = [&](const Src& s) {                 // 9 LDS-DMA instructions per wave
    stage_a(s, I0{}, I0{}, 0); stage_w(s, I0{}, I0{}, 0); stage_s(s, I0{}, 0); stage_w(s, I0{}, I1{}, 0); stage_a(s, I0{}, I1{}, 0);
  };

  int rdA[2], rdB[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {                        // 16-byte chunk g and chunk 4 + g of the row: the operand's two halves
    rdA[ks] = frag_addr(wr * 64, lane, ks);
    rdB[ks] = frag_addr(wc * 32, lane, ks);
  }
  f32x4_t acc[8][4];
  u32x4_t a[4][2], b0[2][2], b1[2][2];
  uint32_t sA[2] = {0u, 0u}, sB = 0u;                     // packed scale bytes: sA[h] byte i = block row i of half h; sB byte 2 g + j
  auto read_a = [&](auto bufc, auto hc) {
    constexpr int OFF = (decltype(bufc)::value ? BUF1 : 0) + decltype(hc)::value * SLOT;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) a[i][ks] = *(const u32x4_t*)(smem + rdA[ks] + OFF + i * 2048);
  };
  auto read_b = [&](auto bufc, auto gc, u32x4_t (&b)[2][2]) {
    constexpr int OFF = (decltype(bufc)::value ? BUF1 : 0) + (2 + decltype(gc)::value) * SLOT;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) b[j][ks] = *(const u32x4_t*)(smem + rdB[ks] + OFF + j * 2048);
  };
  // the lane group's byte of a row dword by a byte load: 12 ds_read_u8 + 9 shift-ors per K-tile (dword loads + extract measured
  // slower: profiles/r06_gemm_mx_scale_byte_loads_ab.txt)
  const int sbyteA = (wr * 128 + (lane & 15)) * 4 + (lane >> 4);       // byte g of this lane's row dword, block row 0 of half 0
  const int sbyteB = 1024 + (wc * 64 + (lane & 15)) * 4 + (lane >> 4);
  auto read_scales = [&](auto bufc) {
    const char* sc = smem + SC_OFF + decltype(bufc)::value * 2048;
    const unsigned char* sa = (const unsigned char*)sc + sbyteA;
    const unsigned char* sb = (const unsigned char*)sc + sbyteB;
    sA[0] = (uint32_t)sa[0] | ((uint32_t)sa[64] << 8) | ((uint32_t)sa[128] << 16) | ((uint32_t)sa[192] << 24);
    sB = (uint32_t)sb[0] | ((uint32_t)sb[64] << 8) | ((uint32_t)sb[128] << 16) | ((uint32_t)sb[192] << 24);     // byte 2 g + j: row g * 32 + j * 16
    // (all three in P0: the strip is restaged for K-tile kt + 2 by the OTHER wave row's P1, which runs while this row is in P1 too --
    //  reading the second half's scales only where they are first used, in P1, raced with that DMA and bought nothing)
    sA[1] = (uint32_t)sa[256] | ((uint32_t)sa[320] << 8) | ((uint32_t)sa[384] << 16) | ((uint32_t)sa[448] << 24);
  };
  bool wave_live = true;
  auto frag = [](const u32x4_t (&f)[2]) {
    return (i32x8_t){(int)f[0][0], (int)f[0][1], (int)f[0][2], (int)f[0][3], (int)f[1][0], (int)f[1][1], (int)f[1][2], (int)f[1][3]};
  };
  auto mma1 = [&](auto hc, auto gc, u32x4_t (&b)[2][2]) {   // 8 MFMAs: the 64 x 32 quadrant (h, g)
    constexpr int H = decltype(hc)::value, G = decltype(gc)::value;
    auto one = [&](auto ic, auto jc) {                      // (op_sel is an immediate: block indices as types)
      constexpr int i = decltype(ic)::value, j = decltype(jc)::value;
      if constexpr (SWAPACC)
        acc[H * 4 + i][G * 2 + j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(frag(b[j]), frag(a[i]), acc[H * 4 + i][G * 2 + j], 0, 0, 2 * G + j, sB, i, sA[H]);
      else
        acc[H * 4 + i][G * 2 + j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(frag(a[i]), frag(b[j]), acc[H * 4 + i][G * 2 + j], 0, 0, i, sA[H], 2 * G + j, sB);
    };
    one(I0{}, I0{}); one(I0{}, I1{}); one(I1{}, I0{}); one(I1{}, I1{});
    one(I2{}, I0{}); one(I2{}, I1{}); one(I3{}, I0{}); one(I3{}, I1{});
  };
  auto mma2 = [&](auto hc, auto g0c, u32x4_t (&bA)[2][2], auto g1c, u32x4_t (&bB)[2][2]) {
    mfma_section(wave_live, [&]() { mma1(hc, g0c, bA); mma1(hc, g1c, bB); });
  };
  // LDS-DMA instructions per wave: a half-tile = 2, a scale strip = 1.  In flight on entry of P0(kt), oldest first:
  // A_1(kt) [2], then A_0 / B_0 / S(kt + 1) [5]
  auto ktile = [&](auto bufc, int kt) {
    constexpr int B = decltype(bufc)::value;
    using Bc = std::integral_constant<int, B>;
    using Nc = std::integral_constant<int, B ^ 1>;
    // P0
    read_b(Bc{}, I0{}, b0);
    read_b(Bc{}, I1{}, b1);
    __builtin_amdgcn_sched_barrier(0);
    read_a(Bc{}, I0{});
    read_scales(Bc{});
    if (kt + 1 < nk) {
      stage_w(src, Nc{}, I1{}, kt + 1); stage_a(src, Nc{}, I1{}, kt + 1);
      wait_vm<Plan::P0, true>();   // A_1(kt) has landed
    } else {
      wait_vm<0, true>();
    }
    bar(); mma2(I0{}, I0{}, b0, I1{}, b1); bar();
    // P1.  In flight: A_0 / B_0 / S(kt + 1) [5], B_1 / A_1(kt + 1) [4]
    read_a(Bc{}, I1{});
    if (kt + 2 < nk) {
      stage_a(src, Bc{}, I0{}, kt + 2); stage_w(src, Bc{}, I0{}, kt + 2); stage_s(src, Bc{}, kt + 2);
      wait_vm<Plan::P1, true>();   // A_0 / B_0 / S / B_1 of K-tile kt + 1 have landed
    } else if (kt + 1 < nk) {
      wait_vm<Plan::P1_TAIL, true>();
    } else {
      wait_vm<0, true>();
    }
    bar(); mma2(I1{}, I1{}, b1, I0{}, b0); bar();
  };

  bool k0_staged = false;
  for (int v = blockIdx.x; v < ntiles; v += gridDim.x) {
    int m0, n0;
    origin(v, m0, n0);
    src = tile_src(m0, n0);
    wave_live = n0 + wc * 64 < p.N;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
    if (!k0_staged) stage_ktile0(src);
    if (nk > 1) {
      stage_a(src, I1{}, I0{}, 1); stage_w(src, I1{}, I0{}, 1); stage_s(src, I1{}, 1);
      wait_vm<Plan::PROLOGUE>();
    } else {
      wait_vm<0>();
    }
    bar();
    if (wr == 1) bar();
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
      ktile(I0{}, kt);
      ktile(I1{}, kt + 1);
    }
    if (kt < nk) ktile(I0{}, kt);
    if (wr == 0) bar();
    __syncthreads();

    const int vn = v + gridDim.x;
    bool hooked = false;
    Src nsrc = src;
    k0_staged = false;
    if (PREFETCH && vn < ntiles) {
      int m1, n1;
      origin(vn, m1, n1);
      nsrc = tile_src(m1, n1);
      k0_staged = true;
    }
    auto hook = [&]() {
      if (!hooked && k0_staged) stage_ktile0(nsrc);
      hooked = true;
    };
    if constexpr (EPI == EPI_QKV) qkv_epilogue16<4>(p, acc, smem + EPI_OFF, wave, lane, m0 + wr * 128, n0 + wc * 64, hook);
    else gemm_epilogue16<4, EPI, 4, SWAPACC, decltype(hook)&>(p, acc, 0, smem + EPI_OFF, wave, lane, m0 + wr * 128, n0 + wc * 64, hook);
    hook();
    if (vn < ntiles) __syncthreads();
  }
}

// MXFP8 on the persistent two-phase loop (ld_gemm8p_mx_kernel): every tile of the raster, one workgroup per CU walking it
int launch_8p_mx(GemmParams p, hipStream_t stream) {
  p.group_m = raster_group_m(p.N);
  dim3 grid(persistent_grid((long)((p.M + 255) / 256) * ((p.N + 255) / 256))), block(512);
  return with_epilogue<EPI_QKV, EPI_BIAS, EPI_GELU, EPI_GATE, EPI_GELU_MX>(pick_epilogue(p), [&](auto e) {
    constexpr int E = decltype(e)::value;
    return launch_kernel<ld_gemm8p_mx_kernel<E>>(E == EPI_QKV ? "ld_gemm_qkv_heads_mxfp8" : "ld_gemm_mxfp8(8p)", grid, block, LD_LDS_TOTAL, stream, p);
  });
}

int launch_f8(GemmParams p, hipStream_t stream) {
  // LD_GEMM_MX8P=0: the round-1 two-stage MXFP8 kernel (A/B timing; the fused qkv form exists in the persistent kernel only)
  static int k_mx8p = LD_KNOB_UNSET;
  if (p.mx_a && (p.q_out || ld_knob("LD_GEMM_MX8P", 1, &k_mx8p) != 0)) return launch_8p_mx(p, stream);
  p.group_m = 8;
  return launch_2stage_f8(p, false, stream);
}

// MXFP8 quantiser: elements = e4m3 cast of x / scale, one scale per 32 consecutive K elements by the block rule of ld_mx.h.
// One wave per row; a block is the four 8-element chunks of four adjacent lanes.
__global__ __launch_bounds__(256) void ld_quant_mxfp8_kernel(const bf16_t* x, long ldx, unsigned char* q, long ldq,
                                                             unsigned char* sc, long lds, int rows, int K) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int nchunk = K >> 3;
  for (int c = lane; c < ((nchunk + 63) & ~63); c += 64) {
    u32x4_t v = (u32x4_t){0u, 0u, 0u, 0u};
    if (c < nchunk) v = *(const u32x4_t*)(x + (long)r * ldx + c * 8);
    float f[8];
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[2 * e] = bf_lo(v[e]); f[2 * e + 1] = bf_hi(v[e]); amax = fmaxf(amax, fmaxf(fabsf(f[2 * e]), fabsf(f[2 * e + 1]))); }
    float inv;
    const int sb = mx_scale_byte(mx_block_amax(amax), inv);
    if (c < nchunk) {
      *(u32x2_t*)(q + (long)r * ldq + c * 8) = mx_pack8(f, inv);
      if ((c & 3) == 0) sc[mx_scale_index(r, c * 8, lds)] = (unsigned char)sb;
    }
  }
}

// Row-wise dynamic quantisation to OCP e4m3: scale[r] = amax(row) / 448 (1 for an all-zero row), q = cvt(x / scale).
// One wave per row, the row stays in registers between the two passes (K <= 8192: 16 chunks of 8 per lane).
__global__ __launch_bounds__(256) void ld_quant_fp8_kernel(const bf16_t* x, long ldx, unsigned char* q, long ldq, float* scale,
                                                           int rows, int K) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int nchunk = K >> 3;
  u32x4_t v[16];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = lane + 64 * i;
    v[i] = (u32x4_t){0u, 0u, 0u, 0u};
    if (c < nchunk) v[i] = *(const u32x4_t*)(x + (long)r * ldx + c * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fmaxf(fabsf(bf_lo(v[i][e])), fabsf(bf_hi(v[i][e]))));
  }
  amax = wave_max(amax);
  const float sc = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;
  const float inv = 1.0f / sc;
  if (lane == 0) scale[r] = sc;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = lane + 64 * i;
    if (c >= nchunk) continue;
    u32x2_t o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float f0 = fminf(fmaxf(bf_lo(v[i][2 * h]) * inv, -448.f), 448.f), f1 = fminf(fmaxf(bf_hi(v[i][2 * h]) * inv, -448.f), 448.f);
      const float f2 = fminf(fmaxf(bf_lo(v[i][2 * h + 1]) * inv, -448.f), 448.f), f3 = fminf(fmaxf(bf_hi(v[i][2 * h + 1]) * inv, -448.f), 448.f);
      unsigned w = 0;
      w = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, w, false);
      w = __builtin_amdgcn_cvt_pk_fp8_f32(f2, f3, w, true);
      o[h] = w;
    }
    *(u32x2_t*)(q + (long)r * ldq + c * 8) = o;
  }
}

}  // namespace
}  // namespace ldgemm

using namespace ldgemm;

LD_API int ld_quantize_fp8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int64_t rows, int64_t K,
                           void* stream) {
  LD_REQUIRE(x && q && scale && rows > 0, "ld_quantize_fp8: bad args");
  LD_REQUIRE(K % 8 == 0 && K <= 8192 && ldx % 8 == 0 && ldq % 8 == 0, "ld_quantize_fp8: K=%ld must be a multiple of 8 and <= 8192", (long)K);
  hipLaunchKernelGGL(ld_quant_fp8_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, (long)ldx, (unsigned char*)q, (long)ldq, scale, (int)rows, (int)K);
  return ld_check_launch("ld_quantize_fp8");
}

LD_API int ld_gemm_fp8(const void* A8, int64_t lda, const float* scale_a, const void* W8, const float* scale_w, void* out,
                       int64_t ldo, int64_t M, int64_t N, int64_t K, const ld_epilogue_t* epi, void* stream) {
  LD_REQUIRE(A8 && W8 && out && scale_a && scale_w, "ld_gemm_fp8: null pointer");
  LD_REQUIRE(M > 0 && N > 0 && K > 0 && K % 128 == 0, "ld_gemm_fp8: K=%ld must be a positive multiple of 128", (long)K);
  LD_REQUIRE(lda % 16 == 0 && ((uintptr_t)A8 & 15) == 0 && ((uintptr_t)W8 & 15) == 0 && ((uintptr_t)out & 15) == 0,
             "ld_gemm_fp8: lda and pointers must be 16-byte aligned");
  LD_REQUIRE(M * lda < (1LL << 32) && N * K < (1LL << 32), "ld_gemm_fp8: operand larger than 4 GiB");
  GemmParams p{};
  p.A = (const bf16_t*)A8; p.W = (const bf16_t*)W8; p.out = out;
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.lda = lda; p.ldo = ldo;
  p.scale_a = scale_a; p.scale_w = scale_w;
  int rc = fill_epilogue(p, epi);
  if (rc) return rc;
  return launch_f8(p, (hipStream_t)stream);
}

LD_API int ld_quantize_mxfp8(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds, int64_t rows,
                             int64_t K, void* stream) {
  LD_REQUIRE(x && q && scales && rows > 0, "ld_quantize_mxfp8: bad args");
  LD_REQUIRE(K % 128 == 0 && ldx % 8 == 0 && ldq % 8 == 0 && lds >= rows, "ld_quantize_mxfp8: K=%ld must be a multiple of 128, lds >= rows", (long)K);
  hipLaunchKernelGGL(ld_quant_mxfp8_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, (long)ldx, (unsigned char*)q, (long)ldq, (unsigned char*)scales, (long)lds, (int)rows, (int)K);
  return ld_check_launch("ld_quantize_mxfp8");
}

LD_API int ld_gemm_mxfp8(const void* A8, int64_t lda, const void* scales_a, const void* W8, const void* scales_w, void* out,
                         int64_t ldo, void* out_scales, int64_t ldos, int64_t M, int64_t N, int64_t K,
                         const ld_epilogue_t* epi, void* stream) {
  LD_REQUIRE(A8 && W8 && out && scales_a && scales_w, "ld_gemm_mxfp8: null pointer");
  LD_REQUIRE(M > 0 && N > 0 && K > 0 && K % 128 == 0, "ld_gemm_mxfp8: K=%ld must be a positive multiple of 128", (long)K);
  LD_REQUIRE(lda % 16 == 0 && ((uintptr_t)A8 & 15) == 0 && ((uintptr_t)W8 & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
             ((uintptr_t)scales_a & 3) == 0 && ((uintptr_t)scales_w & 3) == 0, "ld_gemm_mxfp8: alignment (operands 16 B, scales 4 B)");
  LD_REQUIRE(M * lda < (1LL << 32) && N * K < (1LL << 32), "ld_gemm_mxfp8: operand larger than 4 GiB");
  GemmParams p{};
  p.A = (const bf16_t*)A8; p.W = (const bf16_t*)W8; p.out = out;
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.lda = lda; p.ldo = ldo;
  p.mx_a = (const unsigned char*)scales_a; p.mx_w = (const unsigned char*)scales_w;      // [K/128][M][4], [K/128][N][4] contiguous
  int rc = fill_epilogue(p, epi);
  if (rc) return rc;
  if (out_scales) {     // MXFP8 output (the 4h activation handed to the next MXFP8 GEMM): bias + GELU-tanh only
    LD_REQUIRE(N % 128 == 0 && ldo % 8 == 0 && ldos >= M, "ld_gemm_mxfp8: MXFP8 output needs N %% 128 == 0, ldo %% 8 == 0, ldos >= M");
    LD_REQUIRE(p.act == LD_ACT_GELU_TANH && !p.resid && !p.gate && !p.add2 && !p.mul && !p.out_f32,
               "ld_gemm_mxfp8: MXFP8 output is the bias + GELU-tanh epilogue only");
    p.mx_out = (unsigned char*)out_scales; p.ld_mx_out = ldos;
  }
  return launch_f8(p, (hipStream_t)stream);
}

/* The fused qkv head split on MXFP8 operands (BASELINE configs[4]): ld_gemm_qkv_heads with A / W as e4m3 codes + block scales. */
LD_API int ld_gemm_qkv_heads_mxfp8(const void* A8, int64_t lda, const void* scales_a, const void* W8, const void* scales_w,
                                   const void* bias, int64_t M, int64_t K, void* Q, void* Kh, void* Vt, int64_t B, int64_t Ntok,
                                   int64_t heads, int64_t Npad, const void* q_w, const void* q_b, const void* k_w, const void* k_b,
                                   float eps, void* stream) {
  LD_REQUIRE(A8 && W8 && scales_a && scales_w && bias && Q && Kh && Vt && q_w && q_b && k_w && k_b, "ld_gemm_qkv_heads_mxfp8: null pointer");
  LD_REQUIRE(M == B * Ntok && B > 0 && heads > 0 && K > 0 && K % 128 == 0, "ld_gemm_qkv_heads_mxfp8: M=%ld must be B*Ntok=%ld, K=%ld a multiple of 128",
             (long)M, (long)(B * Ntok), (long)K);
  LD_REQUIRE(Ntok % 8 == 0 && Ntok >= 256 && Npad % 8 == 0 && Npad >= Ntok, "ld_gemm_qkv_heads_mxfp8: Ntok=%ld (multiple of 8, >= 256), Npad=%ld", (long)Ntok, (long)Npad);
  LD_REQUIRE(lda % 16 == 0 && ((uintptr_t)A8 & 15) == 0 && ((uintptr_t)W8 & 15) == 0 && ((uintptr_t)scales_a & 3) == 0 && ((uintptr_t)scales_w & 3) == 0 &&
             ((uintptr_t)bias & 15) == 0 && ((uintptr_t)Q & 15) == 0 && ((uintptr_t)Kh & 15) == 0 && ((uintptr_t)Vt & 15) == 0 &&
             ((uintptr_t)q_w & 15) == 0 && ((uintptr_t)q_b & 15) == 0 && ((uintptr_t)k_w & 15) == 0 && ((uintptr_t)k_b & 15) == 0,
             "ld_gemm_qkv_heads_mxfp8: alignment (operands 16 B, scales 4 B)");
  LD_REQUIRE(M * lda < (1LL << 32) && 3 * heads * 64 * K < (1LL << 32) && M < (1LL << 31), "ld_gemm_qkv_heads_mxfp8: operand larger than 4 GiB");
  GemmParams p{};
  p.A = (const bf16_t*)A8; p.W = (const bf16_t*)W8; p.out = nullptr;
  p.M = (int)M; p.N = (int)(3 * heads * 64); p.K = (int)K; p.lda = lda; p.ldo = 0;
  p.mx_a = (const unsigned char*)scales_a; p.mx_w = (const unsigned char*)scales_w;
  int rc = fill_epilogue(p, nullptr);
  if (rc) return rc;
  p.bias = (const bf16_t*)bias;
  p.q_out = (bf16_t*)Q; p.k_out = (bf16_t*)Kh; p.vt_out = (bf16_t*)Vt;
  p.qn_w = (const bf16_t*)q_w; p.qn_b = (const bf16_t*)q_b; p.kn_w = (const bf16_t*)k_w; p.kn_b = (const bf16_t*)k_b;
  p.heads = (int)heads; p.Ntok = (int)Ntok; p.Npad = (int)Npad; p.qk_eps = eps;
  return launch_8p_mx(p, (hipStream_t)stream);
}
