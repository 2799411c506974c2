// bf16 MFMA GEMM / implicit-GEMM convolution for gfx950 with fused epilogues.
//
//   out[m][n] = epilogue( sum_k A[m][k] * W[n][k] )        (W in nn.Linear layout, K contiguous)
//
// Replaces (reference op sites):
//   sat ColumnParallelLinear/RowParallelLinear + bias + GELU-tanh + gated residual
//   (landiff/diffusion/dit_video_concat.py:568-629,1234-1237,1357-1370),
//   nn.Linear in the TiTok decoder (landiff/tokenizer/modules/blocks.py:164-219,253-261),
//   ContextParallelCausalConv3d / Conv2d (landiff/diffusion/vae_modules/cp_enc_dec.py:416-473,
//   590-633; landiff/diffusion/semantic_models/modules/vq_gan_blocks.py:90-148).
//
// Structure (MI355X-first, not a translation of a warp-32 tiling):
//   * 128x128 output tile per 256-thread workgroup, 4 wave64 as 2x2, each wave 64x64 =
//     2x2 v_mfma_f32_32x32x16_bf16 accumulators (64 acc VGPRs), BK = 64.
//   * A and W tiles go HBM -> LDS by LDS-DMA (global_load_lds_dwordx4, 16 B/lane, no VGPR
//     round trip), double buffered (2 x 32 KB), one barrier per K-tile.
//   * LDS image is lane-linear (DMA constraint); bank conflicts on the ds_read_b128 fragment
//     reads are removed by XOR-swizzling the 16-B chunk index with ((row>>1)&7) on the
//     *source* address and on the read (both-sides rule).
//   * Convolution is the same kernel with a different A-row address generator: the input is a
//     zero-bordered channels-last tensor [T+kT-1][H+kH-1][W+kW-1][Cin], so every tap is a plain
//     128-byte row read: no bounds checks, coalesced (B,T,H,W,C) loads.
//   * Epilogue goes through wave-private LDS so that global stores / residual loads are
//     16-byte, row-contiguous.
//   * blockIdx is remapped so that consecutive tiles of one A panel sit on one XCD (private L2).
//
// This file: the planner (which kernel family and which tiles a problem gets) and the bf16 / convolution / route entry points.
// ld_gemm.h: parameters, epilogues and helpers shared by the kernel files ld_gemm_2stage.hip (two-stage loop), ld_gemm_8p.hip
// (8-phase loop), ld_gemm_fp8.hip (fp8 / MXFP8) and ld_gemm_variants.hip (measured alternatives, variants library only).
#include "ld_gemm.h"
#include "../../include/landiff_hip.h"

// ld_conv_narrow.hip: 3x3x3 convolutions with <= 4 output channels; 1 = not its shape, 0 = launched (query_only: would be)
int ld_conv_narrow_try(const void* in_padded, const void* w, const void* bias, void* out, long ldo, long T, long H, long W, long Cin,
                       long Cout, long kT, long kH, long kW, bool plain_bias_epilogue, hipStream_t stream, bool query_only);

namespace ldgemm {
namespace {

// Bytes of the zero-bordered channels-last input a convolution's A-address generator walks: [(T + kT - 1)][Hp][Wp][Cin] bf16.
long conv_input_bytes(const GemmParams& p) {
  const long kT = p.K / ((long)p.kH * p.kW * p.Cin);
  const long T = p.M / ((long)p.H * p.W_);
  return (T + kT - 1) * p.Hp * p.Wp * p.Cin * 2;
}
// The 8-phase kernel addresses a convolution input through ONE raw buffer descriptor based at the tensor (num_records 2^31 - 1,
// 32-bit per-lane BYTE offsets): inputs of 2 GiB or more are out of its range and take the two-stage kernel, whose 32-bit
// ELEMENT offsets + 64-bit tap offsets reach 8 GiB (ld_conv_cl_bf16 refuses anything larger).
constexpr long CONV_8P_MAX_BYTES = 0x7fffffffL;
constexpr long CONV_MAX_BYTES = 1L << 33;

enum { ROUTE_128_2STAGE = 0, ROUTE_256_2STAGE = 1, ROUTE_256_8PHASE = 2, ROUTE_256_W4R = 3, ROUTE_512_8PHASE = 4, ROUTE_NARROW = 5,
       ROUTE_8P_HALF_TAIL = 6, ROUTE_8P_ROW_TAIL = 7 };   // (documented at ld_conv_route and ld_gemm_route in landiff_hip.h)

// What a call will do: the route number that ld_gemm_route / ld_conv_route report, and one or two launches, each with its own
// parameter block (raster group height, tile range or row range filled in).  route < 0: an error code, message set, no launches.
struct GemmPlan {
  int route = 0, n = 0;
  bool conv = false;
  struct { GemmLauncher fn; GemmParams p; } launch[2];
  GemmPlan() = default;
  GemmPlan(int error) : route(error) {}      // (what LD_REQUIRE returns)
  void add(GemmLauncher fn, const GemmParams& p) { launch[n].fn = fn; launch[n].p = p; ++n; }
};

// The round arithmetic below counts tiles against the MI355X's 256 CUs, a constant and not the device's own count: plan() reads
// knobs and shapes only, never the HIP runtime, so that the route queries answer in a process that has no GPU -- and answer what
// the tests pin.  (The launchers size their grids by the device: cu_count().)
constexpr int PLAN_CUS = 256;

GemmPlan plan(const GemmParams& p0, bool conv) {
  GemmParams p = p0;
  // LD_GEMM_TILE (tuning knob): 1 = 128x128 / 4 waves, 3 = 256x256 / 8 waves (both 2-stage, barrier-drained, 16x16x32 MFMAs
  // unless LD_GEMM_M16=0; 3 is the default for large problems when the knob is unset), 11 = 4 waves x 128x128 register-staged
  // on 32x32x16 MFMAs (the round-1 default, kept as the measured alternative; its two siblings -- an 8-wave load/compute
  // ping-pong and a 4-wave LDS-DMA pipeline, within 2 % of it -- were removed in round 2)
  static int k_tile = LD_KNOB_UNSET, k_8p = LD_KNOB_UNSET, k_split = LD_KNOB_UNSET;
  const int forced = ld_knob("LD_GEMM_TILE", 0, &k_tile);
  p.group_m = raster_group_m(p.N);
  const int epi = pick_epilogue(p);
  LD_REQUIRE(epi != EPI_QKV || !conv, "ld_gemm_qkv_heads: not a convolution epilogue");
  // (every conv route's epilogue is EPI_BIAS or EPI_GENERIC with 64-row units: the forms that sum partials)
  LD_REQUIRE(!p.gn_part || (conv && (epi == EPI_BIAS || epi == EPI_GENERIC)), "ld_conv_cl_bf16_gn: epilogue %d does not sum GroupNorm partials", epi);
  GemmPlan out;
  out.conv = conv;
  // measured on MI355X (tools/gemm_dit_shapes.py): the 256x256 tile wins once the grid fills the chip twice over
  // (L2->LDS traffic halves); the 128x128 tile (2 workgroups/CU) is for small problems.  A 128x256-tile, two-workgroups-
  // per-CU form of the pipelined loop (epilogue of one workgroup under the main loop of the other) measured 10 % slower
  // than the 256x256 tile on all four DiT shapes and was dropped.
  int cfg = forced;
  if (cfg == 0) {
    const long tiles256 = (long)((p.M + 255) / 256) * ((p.N + 255) / 256);
    // (the DiT's 1920x1920 GEMMs: 256x256 tiles 0.26 ms vs 0.29 ms on 128x128; the VAE's narrow convolutions, Cout <= 512,
    //  stay on 128x128 tiles unless K is long: 0.50 vs 0.58 s per video.  Round 5, per shape (tools/conv_shape_time.py,
    //  profiles/r05_vae_conv_route_ab.txt): the 256-wide tile must be at least 3/4 used -- Cin 256 -> Cout 128 at 480 x 720 ran
    //  with half of its waves dead, 5.82 ms against 4.41 on 128 x 128 tiles -- and K >= 2048 is long enough: the 1 x 3 x 3
    //  upsampler convs, K = 2304, 3.15 -> 2.69 ms)
    const bool wide_enough = 4L * p.N >= 3L * 256 * ((p.N + 255) / 256);
    cfg = (tiles256 >= 2 * PLAN_CUS && (conv ? (wide_enough && p.K >= 2048) : p.K >= 1024)) ? 3 : 1;
  }
#ifdef LD_VARIANTS
  // LD_GEMM_M512=1 (variants build): a convolution with one 128-wide column of output and 2048 <= K <= 4096 (the VAE's 480 x 720
  // level) on 512 x 128 tiles of the 8-phase loop, when they fill the chip at least once.  Bit-identical; faster alone (2.37 ->
  // 2.16 ms), no gain inside the VAE decode: see ld_gemm8p_m512_kernel.  At K = 6912 (Cin 256) it measured slower: 4.49 -> 4.92 ms.
  static int k_m512 = LD_KNOB_UNSET;
  if (conv && forced == 0 && p.N > 64 && p.N <= 128 && p.K >= 2048 && p.K <= 4096 && p.K % BK == 0 && (p.M + 511) / 512 >= PLAN_CUS &&
      conv_input_bytes(p) < CONV_8P_MAX_BYTES && ld_knob("LD_GEMM_M512", 0, &k_m512) != 0) {
    out.route = ROUTE_512_8PHASE;
    out.add(launch_8p_m512, p);
    return out;
  }
#endif
  if (cfg != 3 && cfg != 11 && cfg != 8) {
    out.route = ROUTE_128_2STAGE;
    out.add(launch_2stage_128, p);
    return out;
  }
  // The main loop of the 256 x 256 tile.
  // (round 1 default for the large linear layers: the register-staged 4-wave loop on 32x32x16 MFMAs, LD_GEMM_TILE=11, now only
  //  in the variants build; the 8-wave LDS-DMA kernel on 16x16x32 MFMAs is 3-8 % faster than it on all four DiT shapes: both are
  //  bound by the power governor, and the 16x16x32 form costs less energy per FLOP)
  const bool main_is_8p = (cfg == 8 || ld_knob("LD_GEMM_8P", 1, &k_8p)) && cfg != 11;
  GemmLauncher big = launch_2stage_256;      // (also the fused qkv split with LD_GEMM_8P=0: it lives in the 16x16x32 kernels only)
  out.route = ROUTE_256_2STAGE;
  if (main_is_8p && (!conv || conv_input_bytes(p) < CONV_8P_MAX_BYTES)) {
    big = launch_8p;
    out.route = ROUTE_256_8PHASE;
  }
#ifdef LD_VARIANTS
  // LD_GEMM_SP=1: the software-pipelined loop (with LD_TUNING=1 re-read per call: tools/gemm_ab.py times both loops alternately)
  static int k_sp = LD_KNOB_UNSET;
  if (big == launch_8p) {
    if (!conv && ld_knob("LD_GEMM_SP", 0, &k_sp) == 1 && (p.K / BK) % 2 == 0 && p.K / BK >= 4) big = launch_sp;
  } else if (!p.q_out && cfg == 11 && p.K % 128 == 0 && !conv) {
    big = launch_w4r;
    out.route = ROUTE_256_W4R;
  }
#endif
  // Wave quantisation: one 256x256 tile per CU at a time, so a grid of 4.3 "rounds" of 256 tiles costs 5.  When the last
  // round would be less than ~60 % full, the bottom rows are cut off and run as 128x128 tiles (two per CU, four times as
  // many) in a second launch: DiT proj / 4h->h GEMMs (N = 1920: 1112 tiles = 4.34 rounds) gain ~12 %.
  const int split = ld_knob("LD_GEMM_MSPLIT", 1, &k_split);
  const int nbm = (p.M + 255) / 256, nbn = (p.N + 255) / 256;
  const long tiles = (long)nbm * nbn;
  const long full = tiles / PLAN_CUS, rem = tiles % PLAN_CUS;
  const bool tail = !conv && p.m_begin == 0 && full >= 2 && rem > 0;
  // Round 5: at most half a round left over and a short K -> the whole rounds (tiles [0, full * 256) of the raster, exactly `full`
  // per CU) on the 8-phase kernel, the rest cut in two along N: 2 * rem <= 256 half tiles, one per CU (ld_gemm8p_n128_kernel).
  // Measured (profiles/r05_gemm_half_tile_tail_ab.txt): a half tile takes 0.86 of a full tile's time -- its phases hold 8 MFMAs
  // between two barriers instead of 16 and the loop's fixed cost per phase no longer hides behind the partner wave -- so the form
  // only wins where the tail launch's own fixed costs matter: K <= 2048 (DiT qkv -12 us of 765, dense / 4h +-3 us); at K = 7680
  // (4h->h) it loses 24 us of 831 to the two-per-CU 128 x 128 tiles and is not used.  LD_GEMM_MSPLIT=2: the round-1..4 form below
  // for every shape, =3: half tiles for every K (A/B timing).
  if ((split == 1 || split == 3) && tail && main_is_8p && 2 * rem <= PLAN_CUS && p.K % BK == 0 && (p.K <= 2048 || split == 3)) {
    GemmParams a = p, b = p;
    a.tile_begin = 0; a.tile_end = (int)(full * PLAN_CUS);
    b.tile_begin = (int)(full * PLAN_CUS); b.tile_end = 0;
    out.route = ROUTE_8P_HALF_TAIL;        // (main_is_8p and !conv: `big` is the 8-phase kernel)
    out.add(big, a);
    out.add(launch_8p_n128, b);
    return out;
  }
  // (rounds 1-4, and today for remainders between 50 and 60 % of a round) the bottom tile ROWS cut off and run as 128 x 128 tiles
  const int rows_main = (int)((full * PLAN_CUS) / nbn);        // whole tile rows that fit in `full` rounds
  if (split && tail && rem * 100 <= 60 * PLAN_CUS && rows_main > 0 && rows_main < nbm) {
    GemmParams a = p, b = p;
    a.M = rows_main * 256;
    b.m_begin = rows_main * 256;
    if (out.route == ROUTE_256_8PHASE) out.route = ROUTE_8P_ROW_TAIL;     // (LD_GEMM_8P=0: stays 1, the two-stage main part)
    out.add(big, a);
    out.add(launch_2stage_128, b);
    return out;
  }
  out.add(big, p);
  return out;
}

// executes a plan's launches in order; stops at the first error
int run(const GemmPlan& gp, hipStream_t stream) {
  if (gp.route < 0) return gp.route;
  for (int i = 0; i < gp.n; ++i)
    if (int rc = gp.launch[i].fn(gp.launch[i].p, gp.conv, stream)) return rc;
  return LD_OK;
}

}  // namespace

// raster group height: 8 x 4 tile patches per XCD (32 resident tiles) for wide outputs; narrow ones (the DiT's N = 1920 GEMMs:
// 8 tile columns) do better with 4 rows x all 8 columns -- the whole W panel set stays in the XCD's L2 (ff2 1311 -> 1344 TFLOP/s).
// LD_GEMM_GROUP_M > 0 fixes the height for every shape.
int raster_group_m(int N) {
  static int k_group_m = LD_KNOB_UNSET;
  const int forced = ld_knob("LD_GEMM_GROUP_M", 0, &k_group_m);
  return forced > 0 ? forced : ((N + 255) / 256 <= 8 ? 4 : 8);
}

int cu_count() {
  static thread_local int cache[16];           // by device ordinal, like LdSmemCache; 0 = not asked yet
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (dev >= 0 && dev < 16 && cache[dev]) return cache[dev];
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0 || (ncu & 7)) ncu = 256;
  if (dev >= 0 && dev < 16) cache[dev] = ncu;
  return ncu;
}

int fill_epilogue(GemmParams& p, const ld_epilogue_t* e) {
  p.bias = nullptr; p.mul = nullptr; p.resid = nullptr; p.gate = nullptr; p.add2 = nullptr;
  p.act = 0; p.out_f32 = 0; p.resid_f32 = 0; p.rows_per_batch = 1 << 30; p.text_len = 0;
  p.gate_bstride = 0; p.gate_off_img = 0; p.gate_off_txt = 0;
  p.ldr = p.ldmul = p.ldadd = 0;
  if (!e) return LD_OK;
  LD_REQUIRE(e->act >= 0 && e->act <= LD_ACT_TANH, "ld_gemm: bad activation %d", e->act);
  p.bias = (const bf16_t*)e->bias; p.act = e->act;
  p.mul = (const bf16_t*)e->mul; p.ldmul = e->ldmul;
  p.resid = e->resid; p.ldr = e->ldr; p.resid_f32 = e->resid_f32;
  p.gate = (const bf16_t*)e->gate;
  p.add2 = (const bf16_t*)e->add2; p.ldadd = e->ldadd;
  p.out_f32 = e->out_f32;
  if (e->rows_per_batch > 0) p.rows_per_batch = e->rows_per_batch;
  p.text_len = e->text_len;
  p.gate_bstride = e->gate_bstride; p.gate_off_img = e->gate_off_img; p.gate_off_txt = e->gate_off_txt;
  return LD_OK;
}

}  // namespace ldgemm

using namespace ldgemm;

LD_API int ld_gemm_bf16(const void* A, int64_t lda, const void* W, void* out, int64_t ldo,
                        int64_t M, int64_t N, int64_t K, const ld_epilogue_t* epi, void* stream) {
  LD_REQUIRE(A && W && out, "ld_gemm_bf16: null pointer");
  LD_REQUIRE(M > 0 && N > 0 && K > 0, "ld_gemm_bf16: empty problem M=%ld N=%ld K=%ld", (long)M, (long)N, (long)K);
  LD_REQUIRE(K % BK == 0, "ld_gemm_bf16: K=%ld must be a multiple of %d", (long)K, BK);
  LD_REQUIRE(lda % 8 == 0, "ld_gemm_bf16: lda=%ld must be a multiple of 8 elements", (long)lda);
  LD_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)out & 15) == 0,
             "ld_gemm_bf16: pointers must be 16-byte aligned");
  LD_REQUIRE(M * (int64_t)N < (1LL << 40) && M < (1LL << 31) && N < (1LL << 31), "ld_gemm_bf16: problem too large");
  GemmParams p{};
  p.A = (const bf16_t*)A; p.W = (const bf16_t*)W; p.out = out;
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.lda = lda; p.ldo = ldo;
  int rc = fill_epilogue(p, epi);
  if (rc) return rc;
  return run(plan(p, false), (hipStream_t)stream);
}

LD_API int ld_gemm_qkv_heads(const void* A, int64_t lda, const void* W, const void* bias, int64_t M, int64_t K,
                             void* Q, void* Kh, void* Vt, int64_t B, int64_t Ntok, int64_t heads, int64_t Npad,
                             const void* q_w, const void* q_b, const void* k_w, const void* k_b, float eps, void* stream) {
  LD_REQUIRE(A && W && bias && Q && Kh && Vt && q_w && q_b && k_w && k_b, "ld_gemm_qkv_heads: null pointer");
  LD_REQUIRE(M == B * Ntok && B > 0 && heads > 0 && K > 0, "ld_gemm_qkv_heads: M=%ld must be B*Ntok=%ld", (long)M, (long)(B * Ntok));
  LD_REQUIRE(K % BK == 0 && lda % 8 == 0, "ld_gemm_qkv_heads: K=%ld must be a multiple of %d, lda of 8", (long)K, BK);
  LD_REQUIRE(Ntok % 8 == 0 && Ntok >= 256 && Npad % 8 == 0 && Npad >= Ntok, "ld_gemm_qkv_heads: Ntok=%ld (multiple of 8, >= 256), Npad=%ld", (long)Ntok, (long)Npad);
  LD_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)bias & 15) == 0 && ((uintptr_t)Q & 15) == 0 &&
             ((uintptr_t)Kh & 15) == 0 && ((uintptr_t)Vt & 15) == 0 && ((uintptr_t)q_w & 15) == 0 && ((uintptr_t)q_b & 15) == 0 &&
             ((uintptr_t)k_w & 15) == 0 && ((uintptr_t)k_b & 15) == 0, "ld_gemm_qkv_heads: pointers must be 16-byte aligned");
  LD_REQUIRE(M < (1LL << 31), "ld_gemm_qkv_heads: problem too large");
  GemmParams p{};
  p.A = (const bf16_t*)A; p.W = (const bf16_t*)W; p.out = nullptr;
  p.M = (int)M; p.N = (int)(3 * heads * 64); p.K = (int)K; p.lda = lda; p.ldo = 0;
  int rc = fill_epilogue(p, nullptr);
  if (rc) return rc;
  p.bias = (const bf16_t*)bias;
  p.q_out = (bf16_t*)Q; p.k_out = (bf16_t*)Kh; p.vt_out = (bf16_t*)Vt;
  p.qn_w = (const bf16_t*)q_w; p.qn_b = (const bf16_t*)q_b; p.kn_w = (const bf16_t*)k_w; p.kn_b = (const bf16_t*)k_b;
  p.heads = (int)heads; p.Ntok = (int)Ntok; p.Npad = (int)Npad; p.qk_eps = eps;
  return run(plan(p, false), (hipStream_t)stream);
}

static int conv_cl(const void* in_padded, const void* Wt, void* out, int64_t ldo, int64_t T, int64_t H, int64_t W, int64_t Cin,
                   int64_t Cout, int64_t kT, int64_t kH, int64_t kW, const ld_epilogue_t* epi, float* gn_partials, void* stream) {
  LD_REQUIRE(in_padded && Wt && out, "ld_conv_cl_bf16: null pointer");
  LD_REQUIRE(T > 0 && H > 0 && W > 0 && Cout > 0, "ld_conv_cl_bf16: empty problem");
  LD_REQUIRE(Cin % BK == 0, "ld_conv_cl_bf16: Cin=%ld must be a multiple of %d (zero-pad channels)", (long)Cin, BK);
  LD_REQUIRE(kT >= 1 && kH >= 1 && kW >= 1 && (kH & 1) && (kW & 1), "ld_conv_cl_bf16: bad kernel size");
  LD_REQUIRE(T * H * W < (1LL << 31), "ld_conv_cl_bf16: too many output positions");
  GemmParams p{};
  p.A = (const bf16_t*)in_padded; p.W = (const bf16_t*)Wt; p.out = out;
  p.M = (int)(T * H * W); p.N = (int)Cout; p.K = (int)(kT * kH * kW * Cin); p.lda = 0; p.ldo = ldo;
  p.H = (int)H; p.W_ = (int)W; p.Hp = (int)(H + kH - 1); p.Wp = (int)(W + kW - 1);
  p.Cin = (int)Cin; p.kH = (int)kH; p.kW = (int)kW;
  LD_REQUIRE(conv_input_bytes(p) < CONV_MAX_BYTES, "ld_conv_cl_bf16: padded input of %ld bytes is beyond the 8 GiB the kernels address "
             "(split the chunk in time)", conv_input_bytes(p));
  int rc = fill_epilogue(p, epi);
  if (rc) return rc;
  // a handful of output channels (the VAE's conv_out): not a GEMM worth a 128-wide tile -- ld_conv_narrow.hip reads the input once
  const bool plain = !p.act && !p.mul && !p.resid && !p.gate && !p.add2 && !p.out_f32;
  if (gn_partials) {
    // the epilogue sums the values it stores: 16-byte rows of 8 channels only (the vector path of both conv epilogues)
    LD_REQUIRE(Cout % 8 == 0 && ldo % 8 == 0 && !p.out_f32 && (!p.resid || p.ldr % 8 == 0) && (!p.mul || p.ldmul % 8 == 0) &&
               (!p.add2 || p.ldadd % 8 == 0), "ld_conv_cl_bf16_gn: Cout, ldo and the epilogue operands' leading dimensions must be multiples of 8, bf16 output");
    LD_REQUIRE(((uintptr_t)gn_partials & 15) == 0, "ld_conv_cl_bf16_gn: gn_partials must be 16-byte aligned");
    p.gn_part = gn_partials;
  } else {
    rc = ld_conv_narrow_try(in_padded, Wt, p.bias, out, ldo, T, H, W, Cin, Cout, kT, kH, kW, plain, (hipStream_t)stream, false);
    if (rc <= 0) return rc;
  }
  return run(plan(p, true), (hipStream_t)stream);
}

LD_API int ld_conv_cl_bf16(const void* in_padded, const void* Wt, void* out, int64_t ldo,
                           int64_t T, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                           int64_t kT, int64_t kH, int64_t kW, const ld_epilogue_t* epi, void* stream) {
  return conv_cl(in_padded, Wt, out, ldo, T, H, W, Cin, Cout, kT, kH, kW, epi, nullptr, stream);
}

LD_API int64_t ld_conv_gn_partials_size(int64_t M, int64_t Cout) { return ((M + 63) / 64) * (Cout / 4) * 2; }

LD_API int ld_conv_cl_bf16_gn(const void* in_padded, const void* Wt, void* out, int64_t ldo,
                              int64_t T, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                              int64_t kT, int64_t kH, int64_t kW, const ld_epilogue_t* epi, float* gn_partials, void* stream) {
  LD_REQUIRE(gn_partials, "ld_conv_cl_bf16_gn: null gn_partials");
  return conv_cl(in_padded, Wt, out, ldo, T, H, W, Cin, Cout, kT, kH, kW, epi, gn_partials, stream);
}

LD_API int ld_conv_route(int64_t T, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t kT, int64_t kH, int64_t kW) {
  if (T <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Cin <= 0 || Cin % BK || kT < 1 || kH < 1 || kW < 1 || T * H * W >= (1LL << 31))
    return ld_set_error(LD_ERR_INVALID, "ld_conv_route: bad shape");
  GemmParams p{};
  p.M = (int)(T * H * W); p.N = (int)Cout; p.K = (int)(kT * kH * kW * Cin);
  p.H = (int)H; p.W_ = (int)W; p.Hp = (int)(H + kH - 1); p.Wp = (int)(W + kW - 1);
  p.Cin = (int)Cin; p.kH = (int)kH; p.kW = (int)kW;
  if (conv_input_bytes(p) >= CONV_MAX_BYTES) return ld_set_error(LD_ERR_INVALID, "ld_conv_route: padded input beyond 8 GiB");
  if (ld_conv_narrow_try(nullptr, nullptr, nullptr, nullptr, Cout, T, H, W, Cin, Cout, kT, kH, kW, true, nullptr, true) == 0) return ROUTE_NARROW;
  return plan(p, true).route;
}

LD_API int ld_gemm_route(int64_t M, int64_t N, int64_t K, int64_t ldo, const ld_epilogue_t* epi, int32_t* epilogue_kind) {
  if (M <= 0 || N <= 0 || K <= 0 || K % BK || M >= (1LL << 31) || N >= (1LL << 31) || M * N >= (1LL << 40))
    return ld_set_error(LD_ERR_INVALID, "ld_gemm_route: bad shape M=%ld N=%ld K=%ld", (long)M, (long)N, (long)K);
  GemmParams p{};
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.ldo = ldo;
  int rc = fill_epilogue(p, epi);
  if (rc) return rc;
  if (epilogue_kind) *epilogue_kind = pick_epilogue(p);
  return plan(p, false).route;
}
