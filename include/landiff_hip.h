/* liblandiff_hip.so -- C ABI of the MI355X (gfx950) LanDiff inference kernels.
 *
 * The reference (LanDiff/LanDiff) has no FFI: its operator seams are Python methods that take
 * torch tensors.  Each entry point below names the reference op site it
 * replaces (paths relative to the reference repo root).  Conventions:
 *   - raw device pointers (tensor.data_ptr()), shapes/strides as int64_t in ELEMENTS,
 *   - the caller owns every buffer including workspaces; the library never allocates,
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); all work is
 *     asynchronous on it, no internal synchronisation, re-entrant per stream,
 *   - the library keeps ONE piece of state: the work-queue counters of the dynamic attention launch (64 sets of
 *     64 bytes in static device memory, one copy per device; see ld_attn_fwd_bf16 and ld_reset).  A set belongs to one
 *     (device, stream) pair and is zeroed on the launch stream before every use, so launches on different streams never
 *     share one and a failed launch leaves nothing behind; everything else is stateless,
 *   - return 0 on success, negative on error; ld_last_error() gives the thread-local message,
 *   - bf16 tensors are raw uint16 bit patterns; "f32" means IEEE float.
 */
#ifndef LANDIFF_HIP_H
#define LANDIFF_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a signature changes or an entry point is added / removed (2: ld_groupnorm_stats took its `partials`
 * argument, ld_gemm_qkv_heads / ld_llm_sample_advance / ld_groupnorm_stats_blocks / ld_attn_last_kernel were added).  A caller
 * compares ld_version() with the LD_ABI_VERSION it was built against before anything else (landiff_amd/_lib.py does).
 * 6: ld_reset and ld_attn_queue_poke were added.  7: ld_conv_cl_bf16_gn, ld_conv_gn_partials_size and
 * ld_groupnorm_stats_from_conv were added.  8: ld_gemm_qkv_heads_mxfp8 was added.
 * 9: ld_attn_fwd_bf16_exact was added.  10: ld_attn_last_fallbacks was added.  11: ld_vae_enc_place_input,
 * ld_vae_enc_downsample and ld_vae_posterior were added.  12: ld_vit_patch_rows, ld_vit_embed and ld_vit_tail were added,
 * ld_qkv_split gained mode 2.  13: ld_gemm_route was added.  14: ld_gemv_pairs, ld_llm_decode_forward_pairs and
 * ld_llm_sample_advance_pairs were added.  15: ld_llm_token_logprobs and ld_llm_head_f32 were added;
 * ld_gemv_wide, ld_llm_decode_forward_wide and ld_llm_sample_advance_wide joined later, and so did ld_absdiff_sums,
 * ld_residual_sub, ld_residual_add, ld_attn_fwd_bf16_window, ld_attn_window_plan, ld_unpatchify_cfg_keep, ld_unpatchify_cond, ld_latent_pin and ld_mask_to_latent (additions do not change
 * the number: no existing signature moved).  16: ld_attn_route was added; ld_resize_u8 and ld_resize_mask_u8 joined later
 * (additions again).  17: ld_clip_diff_u8 and ld_clip_ssim_u8 were added; ld_retime_u8 joined later (an addition), and so did
 * ld_jpeg_size, ld_jpeg_coefs_u8, ld_jpeg_entropy_i16 and ld_jpeg_encode_u8 (additions again), then ld_jpeg_dec_size,
 * ld_jpeg_find_segments, ld_jpeg_decode_entropy and ld_jpeg_decode_rgb (additions), then ld_gemv_route (an addition), then
 * ld_jpeg_dec_sync_size and ld_jpeg_decode_entropy_sync (additions).  18: ld_jpeg_rate_size, ld_jpeg_c8_u8, ld_jpeg_quant_i16 and
 * ld_jpeg_encode_rate_u8 were added. */
#define LD_ABI_VERSION 18

int ld_version(void);
const char* ld_last_error(void);

/* activation codes for ld_epilogue_t.act */
#define LD_ACT_NONE_ 0
#define LD_ACT_GELU_TANH_ 1
#define LD_ACT_GELU_ERF_ 2
#define LD_ACT_SILU_ 3
#define LD_ACT_TANH_ 4

/* Fused GEMM/conv epilogue, applied in this order on the fp32 accumulator x of out[m][n]:
 *   x += bias[n]; x = bf16(x); x = bf16(act(x)); x = bf16(x * mul[m][n]);
 *   x = bf16(x * gate[b(m)][region(m)][n]); x = resid[m][n] + x; x = x + add2[m][n]
 * (null pointers skip a step; the last two round to bf16 unless out_f32).
 * b(m) = m / rows_per_batch, region = text if (m % rows_per_batch) < text_len else image,
 * gate row = gate + b*gate_bstride + (gate_off_txt | gate_off_img).
 * Mirrors: bias+GELU-tanh of sat's MLP, `h + gate * y` of AdaLNMixin.layer_forward
 * (landiff/diffusion/dit_video_concat.py:593-598,619-624), the control add (:1357-1370),
 * `x + attn` / `x + mlp` of ResidualAttentionBlock (landiff/tokenizer/modules/blocks.py:292-304),
 * `x + h` of the VAE/upsampler ResnetBlocks (cp_enc_dec.py:782, vq_gan_blocks.py:148). */
typedef struct ld_epilogue_t {
  const void* bias;    /* bf16 [N] */
  int32_t act;
  const void* mul;     /* bf16 [M][ldmul] */
  int64_t ldmul;
  const void* resid;   /* bf16 or f32 [M][ldr] */
  int64_t ldr;
  int32_t resid_f32;
  const void* gate;    /* bf16 */
  int64_t gate_bstride, gate_off_img, gate_off_txt;
  int32_t rows_per_batch, text_len;
  const void* add2;    /* bf16 [M][ldadd] */
  int64_t ldadd;
  int32_t out_f32;
} ld_epilogue_t;

/* out[M][N] = epi(A[M][K] @ W[N][K]^T), bf16 operands, fp32 MFMA accumulation.
 * K % 64 == 0, lda % 8 == 0, 16-byte aligned pointers.
 * Replaces sat ColumnParallelLinear/RowParallelLinear (DiT qkv/dense/mlp), nn.Linear in the
 * TiTok decoder, the control zero-linears (dit_video_concat.py:1234-1237), 1x1x1 convs. */
int ld_gemm_bf16(const void* A, int64_t lda, const void* W, void* out, int64_t ldo,
                 int64_t M, int64_t N, int64_t K, const ld_epilogue_t* epi, void* stream);

/* The DiT's qkv Linear with the head split fused into its epilogue: ld_gemm_bf16 (bias) followed by ld_qkv_split mode 0,
 * without the [M][3*heads*64] round trip through HBM.  Replaces attention.query_key_value + sat's _transpose_for_scores +
 * query/key_layernorm of AdaLNMixin.attention_fn (landiff/diffusion/dit_video_concat.py:636-653).
 * A [M = B*Ntok][K] bf16 (row stride lda), W [3*heads*64][K] (thirds q | k | v), bias [3*heads*64];
 * Q, Kh [B][heads][Npad][64] = LayerNorm(64, eps) of the bf16 Linear output per head; Vt [B][heads][64][Npad] = V transposed.
 * Rows [Ntok, Npad) of the three outputs are NOT written: zero-fill them once.  K % 64 == 0, Ntok % 8 == 0, Ntok >= 256. */
int ld_gemm_qkv_heads(const void* A, int64_t lda, const void* W, const void* bias, int64_t M, int64_t K,
                      void* Q, void* Kh, void* Vt, int64_t B, int64_t Ntok, int64_t heads, int64_t Npad,
                      const void* q_w, const void* q_b, const void* k_w, const void* k_b, float eps, void* stream);

/* Which kernel ld_gemm_bf16 runs for a shape and epilogue, without launching anything (no GPU needed; the pointers of `epi` are
 * only tested for null).  Returns the route code of ld_conv_route below -- 0 = 128x128 two-stage, 1 = 256x256 two-stage,
 * 2 = 256x256 8-phase on every tile -- or one of the two split forms (the last, partial round of 256x256 tiles on 256 CUs run by a
 * second launch):
 *   6 = 8-phase on the whole rounds, the remaining tiles as 256x128 half tiles (remainder at most half a round, K <= 2048),
 *   7 = 8-phase on the top tile rows, the rows below as 128x128 tiles (remainder at most 60 % of a round, not the case above);
 * negative = the shape is refused.  *epilogue_kind (may be null) = the epilogue the kernels are specialised for:
 * 0 = bias (act none), 1 = bias + GELU-tanh, 2 = gate + bf16 residual (+ add2; rows_per_batch >= 512), 3 = generic (everything
 * else: other activations, mul, fp32 residual or output, N or a leading dimension not a multiple of 8).  The fused qkv split
 * (ld_gemm_qkv_heads, epilogue 5) takes the route of ld_gemm_route(M, 3 * heads * 64, K, ...).  As for convolutions, the routes
 * give bit-identical outputs: the 8-phase rounds, the half-tile tail and the row tail equal 256-row slices of the same GEMM run on
 * the 128x128 route, bit for bit (measured at the DiT's shapes, tests/test_gpu_gemm_routes.py).  Host logic only.  (The same
 * query for attention: ld_attn_route, with the attention entry points below.) */
int ld_gemm_route(int64_t M, int64_t N, int64_t K, int64_t ldo, const ld_epilogue_t* epi, int32_t* epilogue_kind);

/* Channels-last implicit-GEMM convolution, stride 1.
 * in_padded: bf16 [T+kT-1][H+kH-1][W+kW-1][Cin] with the zero spatial border and the causal time
 * halo already in place (the producer kernels write that layout); Wt: bf16 [Cout][kT][kH][kW][Cin];
 * out: [T*H*W][ldo].  Cin % 64 == 0.
 * Replaces ContextParallelCausalConv3d.forward (landiff/diffusion/vae_modules/cp_enc_dec.py:416-473)
 * and the Conv2d sites of Upsample3D (:605-633) and vq_gan_blocks (ResnetBlock :90-148). */
int ld_conv_cl_bf16(const void* in_padded, const void* Wt, void* out, int64_t ldo,
                    int64_t T, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                    int64_t kT, int64_t kH, int64_t kW, const ld_epilogue_t* epi, void* stream);

/* ld_conv_cl_bf16 whose epilogue also leaves GroupNorm partial sums of the bf16 OUTPUT it stores: gn_partials, caller-owned,
 * ld_conv_gn_partials_size(T*H*W, Cout) floats = [ceil(T*H*W / 64)][Cout / 4][2] (sum, sum of squares of every 64-row x
 * 4-channel patch), every entry written exactly once by a fixed sequence of fp32 additions (deterministic; no atomics).
 * ld_groupnorm_stats_from_conv turns them into the statistics ld_groupnorm_stats would compute from a second read of the
 * activation -- every GroupNorm of the VAE decoder normalises a convolution's output (SpatialNorm3D, cp_enc_dec.py:546-569,
 * inside the resblock :745-782).  Needs Cout % 8 == 0, ldo % 8 == 0, bf16 output, epilogue operands with leading dimensions
 * % 8 == 0 (LD_ERR_INVALID otherwise); always the GEMM routes 0-2. */
int64_t ld_conv_gn_partials_size(int64_t M, int64_t Cout);
int ld_conv_cl_bf16_gn(const void* in_padded, const void* Wt, void* out, int64_t ldo,
                       int64_t T, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                       int64_t kT, int64_t kH, int64_t kW, const ld_epilogue_t* epi, float* gn_partials, void* stream);

/* Which kernel ld_conv_cl_bf16 runs for a shape, without launching anything (no GPU needed): 0 = 128x128 two-stage,
 * 1 = 256x256 two-stage (32-bit element offsets: padded inputs up to 8 GiB), 2 = 256x256 8-phase (one raw buffer descriptor
 * over the padded input: inputs below 2 GiB only -- larger ones are routed to 1), negative = the shape is refused
 * (e.g. a padded input of 8 GiB or more), 3 = never returned for a convolution (the register-staged 4-wave GEMM loop of the
 * variants build), 5 = the narrow-output kernel (3x3x3, Cin 128, <= 4 output channels, H % 4 == 0,
 * W % 16 == 0 and a bias-only epilogue -- the VAE's conv_out: ld_conv_narrow.hip reads the input once instead of once per tap),
 * 4 = 512x128 8-phase (VARIANTS build with LD_GEMM_M512=1 only: 64 < Cout <= 128, 2048 <= K <= 4096, at least 256 such tiles,
 * padded input below 2 GiB -- a measured alternative for the VAE's 480x720 level).  All GEMM routes (0, 1, 2, 4) give bit-identical
 * outputs.  Host logic only; lets the size guard be tested on CPU. */
int ld_conv_route(int64_t T, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t kT, int64_t kH, int64_t kW);

/* ---- calibration loops for bench.py (not on the product path; ld_calib.hip) ----
 * ld_calib_mfma_bf16: n_workgroups x 256 threads (one wave per SIMD), `iters` trips of 128 v_mfma_f32_16x16x32_bf16 per wave on
 * operands taken once from `operands` (random bf16: the matrix pipe's power depends on the operand bits); *flops_out = FLOP of
 * the launch.  ld_calib_stream_read: one pass of 16-byte non-temporal loads over `bytes`. */
int ld_calib_mfma_bf16(const void* operands, int64_t operand_bytes, float* sink, int64_t n_workgroups, int64_t iters,
                       double* flops_out, void* stream);
int ld_calib_stream_read(const void* buf, int64_t bytes, uint32_t* sink, void* stream);

/* ---- optional fp8 (OCP e4m3) form of the DiT's large linear layers (BASELINE.json configs[4]; the headline metric and
 * every parity claim of the bf16 path stay on ld_gemm_bf16) ---- */

/* Row-wise dynamic quantisation of the activations in front of a Linear: x bf16 [rows][K] (row stride ldx) ->
 * q e4m3 [rows][K] (row stride ldq bytes) and scale[r] = amax(row r) / 448 (1 for an all-zero row); q = rne(x / scale). */
int ld_quantize_fp8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int64_t rows, int64_t K, void* stream);

/* out[M][N] = epilogue(scale_a[m] * scale_w[n] * sum_k A8[m][k] * W8[n][k]): the same nn.Linear sites and the same
 * epilogues as ld_gemm_bf16 (dit_video_concat.py:540-629), operands e4m3 (A8 row stride lda bytes, W8 [N][K] contiguous),
 * fp32 accumulation on v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales.  K % 128 == 0. */
int ld_gemm_fp8(const void* A8, int64_t lda, const float* scale_a, const void* W8, const float* scale_w, void* out,
                int64_t ldo, int64_t M, int64_t N, int64_t K, const ld_epilogue_t* epi, void* stream);

/* MXFP8 form of the same (OCP Microscaling v1.0 container: blocks of 32 consecutive K elements share one E8M0 scale;
 * here the smallest power of two >= amax / 448, so nothing saturates; elements are e4m3 casts of x / scale).
 * scales: uint8, K-tile-major [K/128][lds >= rows][4] (byte = exponent + 127; 0 for an all-zero block): the 256 rows of
 * a GEMM tile and K-tile are 1 KB contiguous for the LDS-DMA.  K % 128 == 0. */
int ld_quantize_mxfp8(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds, int64_t rows,
                      int64_t K, void* stream);

/* out = epilogue(sum over blocks of 2^(sa-127) 2^(sw-127) sum_{k in block} A8[m][k] W8[n][k]): the block scales are
 * applied by the MFMA itself (v_mfma_scale_f32_16x16x128_f8f6f4 on the persistent two-phase loop since round 6).  scales_a [K/128][M][4], scales_w [K/128][N][4] contiguous. */
int ld_gemm_mxfp8(const void* A8, int64_t lda, const void* scales_a, const void* W8, const void* scales_w, void* out,
                  int64_t ldo, void* out_scales, int64_t ldos, int64_t M, int64_t N, int64_t K,
                  const ld_epilogue_t* epi, void* stream);
/* (out_scales != NULL: the output is itself MXFP8 -- out = e4m3 [M][ldo bytes], out_scales [N/128][ldos >= M][4] -- for the
 * bias + GELU-tanh epilogue of dense_h_to_4h, whose result only feeds the next MXFP8 GEMM.) */

/* ld_gemm_qkv_heads on MXFP8 operands (BASELINE configs[4]; round 6): the DiT's qkv Linear with QK-LayerNorm, head split and V
 * transpose in its epilogue, A8 [M][lda bytes] / W8 [3*heads*64][K] e4m3 codes with scales_a [K/128][M][4], scales_w
 * [K/128][3*heads*64][4].  Same outputs and shape rules as ld_gemm_qkv_heads; K % 128 == 0.  Reference sites: as ld_gemm_qkv_heads. */
int ld_gemm_qkv_heads_mxfp8(const void* A8, int64_t lda, const void* scales_a, const void* W8, const void* scales_w,
                            const void* bias, int64_t M, int64_t K, void* Q, void* Kh, void* Vt, int64_t B, int64_t Ntok,
                            int64_t heads, int64_t Npad, const void* q_w, const void* q_b, const void* k_w, const void* k_b,
                            float eps, void* stream);

/* ld_layernorm (+ AdaLN modulate) with MXFP8 output: exactly ld_layernorm's bf16 result, quantised where it is produced
 * (q e4m3 [rows][ldq bytes], scales [D/128][lds >= rows][4]) for the MXFP8 GEMM that consumes it.  bf16 input, D % 128 == 0. */
int ld_layernorm_mxfp8(const void* x, int64_t ldx, const void* w, const void* b, void* q, int64_t ldq, void* scales,
                       int64_t lds, int64_t rows, int64_t D, float eps, const void* mod, int64_t mod_bstride,
                       int64_t shift_img, int64_t scale_img, int64_t shift_txt, int64_t scale_txt,
                       int64_t rows_per_batch, int64_t text_len, void* stream);

/* Fused attention, head_dim 64: O = softmax(scale * Q K^T [+ frame mask]) V.
 * Q, K: bf16 [B*H][Npad][64]; Vt: bf16 [B*H][64][Npad] (V transposed, keys contiguous);
 * O: bf16, element (b, n, h*64 + d) at O + b*o_batch_stride + n*o_row_stride + h*64 + d.
 * Npad % 128 == 0; rows/keys in [N, Npad) must be zero-filled.  fid_q/fid_k (int32 [Npad], or
 * both NULL) select the frame-block mask allowed(q,kv) <=> fid_k[kv] <= fid_q[q]; padding keys
 * carry INT32_MAX; kt_min/kt_max are the per-64-key-tile min/max of fid_k.
 * Masked problems, pinned element by element in tests/test_gpu_attn_masked.py: Nq != Nk is supported (Nq query rows against
 * Nk keys; the TiTok encoder launches its visual and its latent rows separately, the second from offset Q / fid_q / O
 * pointers); the K and V^T padding in [Nk, Npad) must be zero, Q rows past Nq need NOT be (they are read up to Nq rounded up
 * to 128, computed and never stored; their label is taken as fid_q[Nq - 1]); rows of O outside [0, Nq) are not touched; a
 * query row with no visible key yields zeros, not NaN (as flex_attention does).  Masked problems and problems of fewer than
 * 6 key tiles run the plain online-softmax kernel (ld_attn_kernel, ld_attn.hip) in this entry point and in
 * ld_attn_fwd_bf16_exact alike.  The pipelined kernels of the other problems read Q in 256-row blocks up to row Npad - 1:
 * do not call those with a Q pointer offset into a head (landiff_amd/ops.py: attn_fwd refuses it).
 * Replaces sat attention_fn_default/F.scaled_dot_product_attention behind AdaLNMixin.attention_fn
 * (landiff/diffusion/dit_video_concat.py:636-664) and flex_attention with VideoDecoderMask
 * (landiff/tokenizer/modules/blocks.py:172-212, flex_attention_mask.py:193-335).
 * Large unmasked problems (>= 4 rounds of 2 workgroups per CU) run as a dynamic launch whose workgroups pull query blocks
 * through per-XCD counters.  The counter set is chosen by (current device, stream): the first 64 streams of a device that
 * launch attention own one each, further streams -- and any stream that is being captured into a graph -- take the static
 * launch of the same kernel body (bit-identical output).  The set is zeroed on `stream` right before the kernel. */
int ld_attn_fwd_bf16(const void* Q, const void* K, const void* Vt, void* O,
                     int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t Npad,
                     int64_t o_batch_stride, int64_t o_row_stride, float softmax_scale,
                     const int32_t* fid_q, const int32_t* fid_k,
                     const int32_t* kt_min, const int32_t* kt_max, void* stream);

/* The same operation with an exact safe softmax for ANY logit range at a fixed cost (~1.55 x ld_attn_fwd_bf16's launch at the DiT
 * shape): for checkpoints whose q.k * softmax_scale row maxima leave the window of the default launch's max-free fast pass (beyond ~76
 * in natural-log units, i.e. denominators beyond 2^110; profiles/r06_attn_logit_sweep.txt), where the default launch stays correct
 * but re-runs every affected 256-row block (up to 2.6 x).  Unmasked problems of >= 6 key tiles: two passes over the keys (row maxima
 * from QK^T only, then the pipelined loop with -max as the score accumulators' initial value; ld_attn_q64_exact.hip); every other
 * shape: the plain online-softmax kernel ld_attn_fwd_bf16 itself uses there.  No data-dependent branch; run to run identical. */
int ld_attn_fwd_bf16_exact(const void* Q, const void* K, const void* Vt, void* O,
                           int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t Npad,
                           int64_t o_batch_stride, int64_t o_row_stride, float softmax_scale,
                           const int32_t* fid_q, const int32_t* fid_k,
                           const int32_t* kt_min, const int32_t* kt_max, void* stream);

/* Opt-in frame-window attention for sequences laid out [prefix | frame 0 | frame 1 | ...] (N = Nq = Nk tokens, `prefix` text
 * tokens, `group` tokens per frame, `window` frames each side): the pipelined kernel of ld_attn_fwd_bf16 walking fewer key tiles.
 * Same layouts, padding rules and dispatch (static / dynamic, counter sets, graph capture) as ld_attn_fwd_bf16; sets
 * ld_attn_last_kernel (ld_attn_q64_win_kernel / ld_attn_q64_win_dyn_kernel) and the source of ld_attn_last_fallbacks.
 * The rule, per 256-row query block b with rows r0 = 256 b .. r1 = min(r0 + 256, N) - 1, n = ceil(N / 64), pt = ceil(prefix / 64):
 *   r0 < prefix: the block holds a text row and walks every tile [0, n);
 *   else f_lo = (r0 - prefix) / group, f_hi = (r1 - prefix) / group, k_lo = prefix + max(0, f_lo - window) * group,
 *        k_hi = min(N, prefix + (f_hi + window + 1) * group), t_lo = max(pt, k_lo / 64), t_hi = ceil(k_hi / 64):
 *        the block walks tiles 0 .. pt-1, t_lo .. t_hi-1 (n_eff = pt + t_hi - t_lo of them).
 * Every row of the block sees exactly the keys k < N of the listed tiles: all text, at least every token within `window` frames
 * of its own, plus up to one tile and one block of ragged extra at the window's edges -- a deliberate superset (no element mask).
 * Refused before anything is launched: LD_ERR_INVALID for window < 0, group < 1, prefix outside [0, N]; LD_ERR_UNSUPPORTED for
 * fewer than 6 key tiles or a block with n_eff < 6.  There is no masked, rectangular (Nq != Nk) or exact two-pass window form.
 * What the window does to a trained checkpoint's output is unmeasured. */
int ld_attn_fwd_bf16_window(const void* Q, const void* K, const void* Vt, void* O,
                            int64_t B, int64_t H, int64_t N, int64_t Npad,
                            int64_t o_batch_stride, int64_t o_row_stride, float softmax_scale,
                            int64_t prefix, int64_t group, int64_t window, void* stream);

/* The tile range of query block `block` under the rule above, from the function the launcher validates with and the kernels
 * walk by: *t_lo, *t_hi, *n_eff (a text block reports t_lo = pt, t_hi = n).  Host logic only, no GPU needed.  LD_ERR_INVALID for
 * bad arguments or a block outside [0, ceil(N / 256)); shapes ld_attn_fwd_bf16_window would refuse as unsupported still plan. */
int ld_attn_window_plan(int64_t N, int64_t prefix, int64_t group, int64_t window, int64_t block,
                        int32_t* t_lo, int32_t* t_hi, int32_t* n_eff);

/* Which kernel family an attention launch of these shapes runs, without launching anything (no GPU needed, no HIP call): the
 * launch's own plan run dry, under the same LD_ATTN_* knobs.  form: 0 = ld_attn_fwd_bf16, 1 = ld_attn_fwd_bf16_exact,
 * 2 = ld_attn_fwd_bf16_window (Nq = Nk = N, masked = 0); masked != 0: a label mask is given.  Returns
 *   0 = the plain online-softmax kernel (ld_attn_kernel: masked problems and problems of fewer than 6 key tiles, in both of the
 *       first two forms; every problem under LD_ATTN_VARIANT=9, 1 or 4),
 *   1 = the 64-row wave tile (ld_attn_q64_kernel, or ld_attn_q64_dyn_kernel where the launcher can go dynamic: that depends on the
 *       device, the stream and graph capture, which this query does not see),
 *   2 = its two-pass exact form (ld_attn_q64_exact_kernel),  3 = its frame-window form (ld_attn_q64_win_kernel / _win_dyn_kernel),
 *   4 = the 32-row wave tile (ld_attn_p16_*_kernel: LD_ATTN_Q64=0),
 *   5 = the 128-row tile (ld_attn_q128_*kernel) and 6 = the round-1 pipeline (ld_attn_pipe2_*_kernel): VARIANTS build only, under
 *       LD_ATTN_Q128 / LD_ATTN_VARIANT=8,
 * negative = refused, with the message the launch would give for the shape (empty problem, Npad not a multiple of 128 or below
 * Nq / Nk; form 2: fewer than 6 key tiles, a mask or Nq != Nk).  For form 2 it answers from the sequence alone: whether every query
 * block's own tile list is long enough is ld_attn_window_plan's business.  After a launch, ld_attn_last_kernel names a kernel of the
 * family reported here (tests/test_gpu_attn.py). */
int ld_attn_route(int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t Npad, int32_t masked, int32_t form);

/* Forgets the stream -> counter-set assignments of the current device and zeroes its sets (asynchronously on `stream`).
 * Only for a process that keeps creating streams, or after a device error: the caller guarantees that no ld_attn_fwd_bf16
 * launch of this device is enqueued or running on any other stream. */
int ld_reset(void* stream);

/* Test hook: fills counter set `set` (all 64 when set < 0) of the current device with `value`, as a launch that died
 * mid-flight could leave it.  Later launches must be unaffected (tests/test_gpu_attn.py). */
int ld_attn_queue_poke(int32_t set, uint32_t value, void* stream);

/* Name of the kernel the calling thread's last ld_attn_fwd_bf16 launched ("" before the first call): the launcher picks
 * by shape and tuning environment, and measurement code must label what actually ran. */
const char* ld_attn_last_kernel(void);

/* How many 256-row query blocks of the calling thread's most recent ld_attn_fwd_bf16 launch had a row whose softmax denominator
 * left the window of the max-free fast pass (2^-80 .. 2^110) and were recomputed by the running-max pass: a 4-byte value written to
 * `out` (DEVICE memory) by a copy enqueued on `stream`, which must be the stream of that launch and must not have seen another
 * attention launch since.  0 for launches by kernels without such a window (short or masked problems, the exact form); -1 when
 * the launch has a window but kept no count (the static dispatch used under graph capture or beyond 64 streams per device).
 * A caller that runs the same layers again and again (a sampler loop) reads it to switch a layer whose checkpoint leaves the
 * window to ld_attn_fwd_bf16_exact (landiff_amd/dit.py: attn_exact="auto"; profiles/r06_attn_logit_sweep.txt for the prices). */
int ld_attn_last_fallbacks(int32_t* out, void* stream);

/* ---- tokenizer encoder side (ld_tokenize.hip) ---- */

/* VideoVQ.norm_features + the "b t c h w -> b (t h w) c" rearrange in front of TiTokEncoder.patch_embed
 * (landiff/tokenizer/models/video_titok_vq.py:226-231, landiff/tokenizer/modules/blocks.py:598-600):
 * features [T][C][P] (fp32 if in_f32 else bf16, P = h*w) -> out [T*P][C] bf16 = bf16((x - mean[c]) / (std[c] + 1e-8)). */
int ld_feature_norm_cl(const void* features, int32_t in_f32, const float* mean, const float* stdv, void* out,
                       int64_t T, int64_t C, int64_t P, void* stream);

/* VideoVQ.denorm_features (video_titok_vq.py:228-233; active only when the config names a mean_std_path) on the
 * channels-last decoder output, then the cast back to the module dtype (condition.py:103-104):
 * x bf16 [rows][C] -> out bf16 = bf16(float(x) * (std[c] + 1e-8) + mean[c]).  out may alias x. */
int ld_feature_denorm(const void* x, const float* mean, const float* stdv, void* out, int64_t rows, int64_t C, void* stream);

/* Nearest code of vector-quantize-pytorch's EuclideanCodebook.forward in eval (argmax of -cdist, fp32), called by
 * VideoVQ.encode_to_index (video_titok_vq.py:196-200): x bf16 [rows][ldx] (first dim columns), codebook fp32 [V][dim]
 * -> idx int64 [rows] = the first code minimising |x|^2 + |e|^2 - 2 x.e. */
int ld_vq_nearest(const void* x, int64_t ldx, const float* codebook, int64_t* idx, int64_t rows, int64_t V,
                  int64_t dim, void* stream);

/* ---- HBM-bound small-batch kernels (ld_llm_gemv.hip, ld_llm_attn.hip, ld_llm_sample.hip, ld_llm.hip) ---- */

/* y[b][n] = epi(sum_k in_act(x[b][k]) * W[n][k]), 1 <= B <= 4, weights streamed once (one wave per row).
 * bf16 weights: result rounds to bf16 (Linear output), then act, then `* bf16(W2 x)` (gated MLP,
 * LlamaMLP2: landiff/llm/modules/transformer_blocks.py:67-88), then `resid + y`.  w_f32: fp32 weights,
 * x and out fp32 (GPT head, landiff/llm/models/transformer.py:115-118).  in_act is applied to x (bf16-rounded),
 * e.g. the SiLU in front of adaLN_modulation (landiff/diffusion/dit_video_concat.py:499-503).  norm_w (fp32 [K], optional)
 * fuses the block's RMSNorm in front of the projection: x -> bf16(x * rsqrt(mean(x^2) + norm_eps) * norm_w).
 * bias is bf16 [N]; resid has out's type (bf16, or fp32 when out_f32: the sum is then not rounded).
 * in_act together with norm_w is NOT a form: no caller has one, and "normalise the activated x" and "activate the normalised x"
 * are both plausible -- ld_gemv and ld_gemv_pairs refuse it (ld_gemv_wide refuses in_act altogether).
 * LD_ERR_INVALID, nothing launched: null x / W / out, B outside [1, 4], N < 1, K or ldx no multiple of 8, B * K beyond the LDS
 * (160 KB of bf16, or fp32 with fp32 weights), fp32 weights with W2 or without fp32 x and out, norm_w with fp32 x or weights,
 * in_act with norm_w. */
int ld_gemv(const void* x, int64_t ldx, int32_t x_f32, const void* W, const void* W2, int32_t w_f32,
            const void* bias, const void* resid, int64_t ldr, void* out, int64_t ldo, int32_t out_f32,
            int64_t B, int64_t N, int64_t K, int32_t in_act, int32_t act, const float* norm_w, float norm_eps,
            void* stream);

/* The kernel ld_gemv takes for a call, without launching anything (the GEMV's ld_gemm_route): the launcher's own plan, run dry.
 * gated: W2 given; normed: norm_w given.  Returns
 *   0  the LDS-staged streaming kernel (ld_gemv_kernel): a wave takes *R weight rows at a time and keeps *U 16-byte loads per row
 *      and lane in flight per trip over K (a trip covers 64 * U chunks of 8 elements); *J = 0.  fp32 weights: R = 1, U = 4.
 *   1  the register-resident kernel (ld_gemv_reg_kernel; bf16 x and weights, no in_act, K <= 4096, or K <= 12288 for B <= 2 and no
 *      W2): thread t of a workgroup owns chunks t, t + 256, ..., *J of them (1, 2 or 6), a workgroup takes *R rows at a time; *U = 0.
 *   a negative code with ld_gemv's message for a shape or form ld_gemv refuses (see there; pointers and ldx are not part of the query).
 * J, R, U may be null.  Honours LD_GEMV_MODE and LD_GEMV_R like the launch (read once per process).  Host logic only: it answers in
 * a process without a GPU. */
int ld_gemv_route(int64_t B, int64_t N, int64_t K, int32_t x_f32, int32_t w_f32, int32_t out_f32, int32_t gated, int32_t normed,
                  int32_t in_act, int32_t* J, int32_t* R, int32_t* U);

/* ld_gemv for P = B / 2 pairs of activation rows, 1 <= P <= LD_LLM_MAX_PAIRS: the P (cond, uncond) pairs of P samples of one
 * prompt decoded side by side (Semantic1DLM.sample once per seed, lm_model.py:417-508, through the cached blocks of
 * transformer_blocks.py:128-236).  Same arguments as ld_gemv.  Rows (2p, 2p+1) of the output are BIT-IDENTICAL to ld_gemv with
 * B = 2 on those two rows, in every form (fused RMSNorm, gated GELU, residual -- also in place, out == resid --, fp32 head).
 * The bf16 forms the decode uses (K <= 4096, or K <= 12288 without W2) are one launch that reads every weight row from HBM once:
 * the register-resident kernel of the B = 2 route with the same chunk ownership per K and all 2P activation rows in registers.
 * Other forms (fp32 weights: the 17 MB head; fp32 x; in_act; longer K) run the B = 2 route once per pair.
 * LD_ERR_INVALID: odd B, null pointers, K % 8, in_act with norm_w (see ld_gemv); LD_ERR_UNSUPPORTED: P > LD_LLM_MAX_PAIRS --
 * nothing is launched. */
#define LD_LLM_MAX_PAIRS 4
int ld_gemv_pairs(const void* x, int64_t ldx, int32_t x_f32, const void* W, const void* W2, int32_t w_f32,
                  const void* bias, const void* resid, int64_t ldr, void* out, int64_t ldo, int32_t out_f32,
                  int64_t B, int64_t N, int64_t K, int32_t in_act, int32_t act, const float* norm_w, float norm_eps,
                  void* stream);

/* The second engine of the batched decode: out[b][n] = epi(sum_k xn[b][k] * W[n][k]) for B = 2P rows, 1 <= P <= LD_LLM_MAX_WIDE,
 * as a weight-streaming skinny GEMM on v_mfma_f32_32x32x16_bf16 (32 weight rows x the B activation rows as the 32 columns; every
 * weight byte read once).  Arguments of ld_gemv_pairs; bf16 x / W / out only, with the forms the decode uses: fused RMSNorm of x
 * (norm_w), the gated form act(W x) * (W2 x), bias, residual add (out == resid allowed).  Rounding points are ld_gemv's (bf16
 * normalised activations, fp32 accumulation and epilogue, one rounding to bf16 per Linear output); the ORDER of the fp32 sum is
 * another, so the result is not ld_gemv's bit for bit.  What it guarantees instead: row b's bits depend on row b alone -- not on
 * B, on b, or on the other rows (the order of summation is a function of K only).
 * LD_ERR_INVALID: odd B, null pointers, misaligned x / W; LD_ERR_UNSUPPORTED: B > 32, K % 16 != 0, fp32 x / weights / output,
 * in_act -- nothing is launched. */
#define LD_LLM_MAX_WIDE 16
int ld_gemv_wide(const void* x, int64_t ldx, int32_t x_f32, const void* W, const void* W2, int32_t w_f32,
                 const void* bias, const void* resid, int64_t ldr, void* out, int64_t ldo, int32_t out_f32,
                 int64_t B, int64_t N, int64_t K, int32_t in_act, int32_t act, const float* norm_w, float norm_eps,
                 void* stream);

/* RMSNorm (transformer_blocks.py:22-40): bf16 rows [rows][D], fp32 weight, fp32 math, bf16 out. */
int ld_rmsnorm_bf16(const void* x, const float* w, void* out, int64_t rows, int64_t D, float eps, void* stream);

/* Final LayerNorm of GPT.sample (transformer.py:112-114): bf16 rows (stride ldx) -> fp32, fp32 affine. */
int ld_layernorm_bf16_to_f32(const void* x, int64_t ldx, const float* w, const float* b, float* out,
                             int64_t rows, int64_t D, float eps, void* stream);

/* apply_rope (landiff/modules/pos_emb.py:16-46) on q,k of qkv [B][m][3][H][128] at positions *pos + j, and KV append
 * into k_cache/v_cache [B][Lmax][H][128] (replaces the torch.cat growth of transformer_blocks.py:153-164). */
int ld_llm_rope_append(const void* qkv, const float* cos_t, const float* sin_t, const int32_t* pos,
                       void* q_out, void* k_cache, void* v_cache, int64_t B, int64_t m, int64_t H,
                       int64_t Lmax, void* stream);

/* Attention of query j (position *pos + j) over keys [0, *pos + j] (transformer_blocks.py:166-186):
 * bf16 scores, bf16(score / sqrt(128)), fp32 softmax -> bf16 p, bf16 output [B][m][H][128].
 * m == 1 with nsplit > 1 uses the key-split path (workspace: B*H*(nsplit*130 + 1) 4-byte words, caller-owned; the last B*H
 * words are arrival counters that must be ZERO before the first call -- the launch leaves them zero: the last split of a
 * (batch row, head) to arrive merges the partial results, no second launch; p kept fp32); there
 * qkv_fused ([B][3][H][128], q may be NULL) makes the kernel do apply_rope and the KV append of the new token itself.
 * nsplit is the MAXIMUM number of key splits (it sizes the workspace and must keep Lmax / nsplit <= 256): a step at context length
 * L = *pos + 1 uses 1 / 2 / 4 / nsplit of them by a fixed rule of L alone (short contexts are not worth a merge; one split writes
 * the output directly), evaluated on the device, so every way of issuing the step gives the same bits. */
int ld_llm_kv_attn(const void* q, const void* k_cache, const void* v_cache, const int32_t* pos, void* out,
                   int64_t B, int64_t m, int64_t H, int64_t Lmax, float* workspace, int64_t nsplit,
                   const void* qkv_fused, const float* cos_t, const float* sin_t, void* stream);

/* One decode step of GPT.sample (landiff/llm/models/transformer.py:91-119 with the cached blocks of
 * transformer_blocks.py:128-236) for B = 2 (the CFG pair): embedding of *token, n_layers x [RMSNorm+qkv GEMV, RoPE +
 * KV append + key-split attention at position *pos, wo GEMV + residual, RMSNorm + gated-GELU MLP GEMVs + residual],
 * final LayerNorm (fp32) and the fp32 head -> logits [B][vocab].  Exactly the launches a caller would issue through
 * ld_llm_embed / ld_gemv / ld_llm_kv_attn / ld_layernorm_bf16_to_f32, queued from native code in one call: the
 * ~150 launches of a step are then bound by the GPU (~1.2 ms) and not by the host language's per-call overhead.
 * emb_table == NULL: x already holds the embedding rows of the token (written by ld_llm_sample_advance).
 * All step state (*token, *pos) is read on the device; pos_value >= 0 tells the launches the value *pos holds (a decode loop
 * knows it: one more per step) so that the attention launches do not start with a dependent load of *pos, -1: read *pos (graph
 * capture); buffers are caller-owned: x/att [B][hidden], qkv [B][3*hidden],
 * gate [B][mlp] bf16, attn_ws B*heads*(nsplit*130 + 1) words (see ld_llm_kv_attn: the last B*heads zero), lnf_out [B][hidden] fp32,
 * logits [B][vocab] fp32. */
typedef struct ld_llm_layer {
  const void* wqkv; const void* wo; const void* w1; const void* w3; const void* w2;   /* bf16 [3h][h] [h][h] [mlp][h] [mlp][h] [h][mlp] */
  const float* n0; const float* n1;                                                    /* RMSNorm gains, fp32 [h] */
  void* k_cache; void* v_cache;                                                        /* bf16 [B][Lmax][heads][128] */
} ld_llm_layer;
int ld_llm_decode_forward(const ld_llm_layer* layers, int64_t n_layers, const float* emb_table, const int64_t* token,
                          const int32_t* pos, int32_t pos_value, void* x, void* qkv, void* att, void* gate, float* attn_ws,
                          const float* cos_t, const float* sin_t, const float* lnf_w, const float* lnf_b, float* lnf_out,
                          const float* head_w, float* logits, int64_t B, int64_t hidden, int64_t heads, int64_t mlp,
                          int64_t vocab, int64_t Lmax, int64_t nsplit, float rms_eps, float ln_eps, void* stream);

/* ld_llm_decode_forward for P = B / 2 samples of ONE prompt decoded side by side (same text, same prefix, so one shared position
 * and forced-token schedule; lm_model.py:417-508 per sample over transformer_blocks.py:128-236): B = 2P rows, pair p = rows
 * (2p, 2p+1) of x / qkv / att / gate / lnf_out / logits and of every layer's k_cache / v_cache [B][Lmax][heads][128]; token [P]
 * (emb_table == NULL: x already holds the rows, written by ld_llm_sample_advance_pairs); pos: the position word (word 0 of the
 * per-sample position array).  The GEMVs go through ld_gemv_pairs (each weight matrix streamed once for all pairs), attention
 * through the key-split kernel over (B * heads, split): pair p gets exactly the bits ld_llm_decode_forward gives a B = 2 caller
 * with the same Lmax and nsplit -- nsplit MUST be the B = 2 caller's value (the split rule is part of the bits); attn_ws:
 * B*heads*(nsplit*130 + 1) words, the last B*heads zero.  LD_ERR_INVALID: odd B, null pointers, head_dim != 128;
 * LD_ERR_UNSUPPORTED: P > LD_LLM_MAX_PAIRS -- checked before anything is launched. */
int ld_llm_decode_forward_pairs(const ld_llm_layer* layers, int64_t n_layers, const float* emb_table, const int64_t* token,
                                const int32_t* pos, int32_t pos_value, void* x, void* qkv, void* att, void* gate, float* attn_ws,
                                const float* cos_t, const float* sin_t, const float* lnf_w, const float* lnf_b, float* lnf_out,
                                const float* head_w, float* logits, int64_t B, int64_t hidden, int64_t heads, int64_t mlp,
                                int64_t vocab, int64_t Lmax, int64_t nsplit, float rms_eps, float ln_eps, void* stream);

/* ld_llm_decode_forward_pairs on the second engine, B = 2P rows, P <= LD_LLM_MAX_WIDE: every block GEMV is ld_gemv_wide, the head
 * is ld_llm_head_f32; embedding of token[P], key-split attention (nsplit of the two-row runner) and final LayerNorm as in the
 * _pairs form.  Pair p's logits depend on pair p's token and cache rows alone (not on P or p); they agree with
 * ld_llm_decode_forward's to bf16 rounding noise, not bit for bit.  LD_ERR_INVALID: odd B, null pointers, head_dim != 128;
 * LD_ERR_UNSUPPORTED: P > LD_LLM_MAX_WIDE, mlp % 16 != 0 -- checked before anything is launched. */
int ld_llm_decode_forward_wide(const ld_llm_layer* layers, int64_t n_layers, const float* emb_table, const int64_t* token,
                               const int32_t* pos, int32_t pos_value, void* x, void* qkv, void* att, void* gate, float* attn_ws,
                               const float* cos_t, const float* sin_t, const float* lnf_w, const float* lnf_b, float* lnf_out,
                               const float* head_w, float* logits, int64_t B, int64_t hidden, int64_t heads, int64_t mlp,
                               int64_t vocab, int64_t Lmax, int64_t nsplit, float rms_eps, float ln_eps, void* stream);

/* ---- Entry points of the VARIANTS build only (landiff_amd/variants/liblandiff_hip_variants.so, built by
 * `LD_BUILD_VARIANTS=1 landiff_amd/csrc/build.sh` with -DLD_VARIANTS): two other forms of the decode step that were built, are
 * bit-identical to ld_llm_decode_forward, measured slower and are kept under test as measured alternatives.  The shipped
 * library does not export them. ---- */
#ifdef LD_VARIANTS
/* The same step with all blocks in ONE persistent launch (ld_llm_fused.hip): identical bits, ~one launch instead of 144.
 * layers_dev: the ld_llm_layer table in DEVICE memory.  ctl: LD_LLM_FUSED_CTL_WORDS 32-bit words of device memory owned by
 * the caller, zeroed before the first step of a decode (word 0: steps done, word 1: error flag -- non-zero after a grid
 * barrier timed out; every later launch then returns without touching anything; words 32..: arrival counters).  The launch
 * needs the GPU's CUs to itself (its workgroups wait for each other): do not run it concurrently with other streams' kernels.
 * LD_ERR_UNSUPPORTED (nothing launched) unless B == 2, head_dim 128, hidden <= 2048, mlp <= 12288, nsplit >= 2 and at most
 * 256 keys per split -- use ld_llm_decode_forward then.  Replaces transformer_blocks.py:128-236 / transformer.py:91-119. */
#define LD_LLM_FUSED_CTL_WORDS 512
int ld_llm_decode_blocks_fused(const ld_llm_layer* layers_dev, int64_t n_layers, const int32_t* pos, void* x, void* qkv, void* att,
                               void* gate, float* attn_ws, const float* cos_t, const float* sin_t, int64_t B, int64_t hidden,
                               int64_t heads, int64_t mlp, int64_t Lmax, int64_t nsplit, float rms_eps, uint32_t* ctl, void* stream);
/* embedding (optional) -> ld_llm_decode_blocks_fused -> final LayerNorm -> fp32 head: the drop-in form of ld_llm_decode_forward */
int ld_llm_decode_forward_fused(const ld_llm_layer* layers_dev, int64_t n_layers, const float* emb_table, const int64_t* token,
                                const int32_t* pos, void* x, void* qkv, void* att, void* gate, float* attn_ws,
                                const float* cos_t, const float* sin_t, const float* lnf_w, const float* lnf_b, float* lnf_out,
                                const float* head_w, float* logits, int64_t B, int64_t hidden, int64_t heads, int64_t mlp,
                                int64_t vocab, int64_t Lmax, int64_t nsplit, float rms_eps, float ln_eps, uint32_t* ctl,
                                void* stream);

/* The blocks of the same step as DEPENDENT LAUNCHES ON TWO STREAMS: operation k (5 per block: qkv, attention, wo, w1.w3, w2) goes
 * to stream k & 1 with no stream dependency on operation k - 1; its workgroups request their first weight rows (the attention: its
 * K / V rows), then wait until every workgroup of operation k - 1 has arrived on that operation's counters, and arrive on their own
 * when their outputs are written (sc1) and drained -- a launch is dispatched and streaming weights while its predecessor runs.
 * Identical bits.  layers: HOST table (as ld_llm_decode_forward).  pos_value: the position *pos holds (the host knows it: one
 * more per step) -- the launches do not read *pos, so they do not depend on the previous step's sampling launch.  ctl:
 * LD_LLM_CHAIN_CTL_WORDS words of device memory, zeroed before the first step of a decode (word 0: error flag, set when a wait
 * timed out after ~1 s -- later waits then fall through); epoch: steps done since the zeroing.  Caller's duties: stream1 must
 * be ordered after whatever wrote the KV cache / x before the first step (e.g. the prefill), and whatever reads x after the call
 * must be ordered after BOTH streams.  Every launch fits twice on the chip (<= 128 registers, <= 512 workgroups; the attention
 * half the chip), so the waiting launch can never keep its predecessor from becoming resident -- provided nothing else occupies
 * the GPU for long.  LD_ERR_UNSUPPORTED outside B == 2, head_dim 128, hidden <= 4096, mlp <= 12288, <= 256 keys per split,
 * 5 * n_layers <= LD_LLM_CHAIN_MAX_OPS. */
#define LD_LLM_CHAIN_MAX_OPS 256
#define LD_LLM_CHAIN_CTL_WORDS (64 + LD_LLM_CHAIN_MAX_OPS * 8 * 16)
int ld_llm_decode_blocks_chained(const ld_llm_layer* layers, int64_t n_layers, int32_t pos_value, void* x, void* qkv, void* att,
                                 void* gate, float* attn_ws, const float* cos_t, const float* sin_t, int64_t B, int64_t hidden,
                                 int64_t heads, int64_t mlp, int64_t Lmax, int64_t nsplit, float rms_eps, uint32_t* ctl,
                                 uint32_t epoch, void* stream0, void* stream1);
#endif /* LD_VARIANTS */

/* nn.Embedding lookup of *token (fp32 table [V][D]) -> bf16 features [B][D] (landiff/llm/modules/tokenizer.py:10-55). */
int ld_llm_embed(const float* table, const int64_t* token, void* out, int64_t B, int64_t D, void* stream);

/* lm_model.py:417-454: logits [2][V] = (cond, uncond) -> CFG `u + s*(c-u)` (guided), / temperature, optional
 * restriction to allowed[*pos + 1][1 .. 1+allowed[..][0]], softmax -> probs [V] (V <= 4096).  cfg_logits (optional) gets
 * the CFG logits.  At unrestricted positions: top_k > 0 keeps logits >= the k-th largest (lm_model.py:441-443), and
 * top_p >= 0 is top_p_probability (landiff/utils.py:345-359: descending sort, sequential cumsum, drop sorted position
 * j >= 1 when cumsum[j-1] >= top_p, renormalise).  top_k <= 0 / top_p < 0 switch the filters off (the CLI default). */
int ld_llm_logits_to_probs(const float* logits, float* probs, float* cfg_logits, int64_t V, int32_t guided,
                           float scale, float temperature, const int32_t* pos, const int32_t* allowed,
                           int64_t allowed_stride, int32_t top_k, float top_p, void* stream);

/* ld_llm_logits_to_probs, the draw, ld_llm_decode_advance and ld_llm_embed of the next token in one launch (the tail of a
 * decode step: lm_model.py:417-508).  `noise` [V]: Exp(1) draws from the caller's generator -- torch.multinomial(p, 1, gen)
 * IS argmax(p / empty_like(p).exponential_(1, gen)) (lowest index on ties), so the token equals the reference's draw from
 * the same generator state.  probs / cfg_logits / sampled (the raw draw, before the forced-token override) are optional
 * outputs; x [B][D] bf16 receives the embedding rows of *token (ld_llm_decode_forward then takes emb_table = NULL). */
int ld_llm_sample_advance(const float* logits, float* probs, float* cfg_logits, int64_t V, int32_t guided, float scale,
                          float temperature, int32_t* pos, const int32_t* allowed, int64_t allowed_stride,
                          int32_t top_k, float top_p, const float* noise, const int32_t* forced, int64_t* token,
                          int64_t* out_tokens, int32_t* out_count, int64_t* sampled, const float* emb_table, void* x,
                          int64_t B, int64_t D, void* stream);

/* ld_llm_sample_advance for P samples (1 <= P <= LD_LLM_MAX_PAIRS) in one launch of P workgroups (lm_model.py:417-508 per
 * sample): workgroup p does what ld_llm_sample_advance does on logits rows (2p, 2p+1) of [2P][V] with noise / probs / cfg_logits
 * row p of [P][V], pos[p], token[p], out_tokens[p * out_stride ..], out_count[p], sampled[p] and x rows (2p, 2p+1) of [2P][D].
 * forced / allowed are the one shared schedule.  pos holds one word per sample, all equal: each workgroup reads and advances
 * its own, so no workgroup's increment races another's read (the forward pass reads word 0). */
int ld_llm_sample_advance_pairs(const float* logits, float* probs, float* cfg_logits, int64_t V, int32_t guided, float scale,
                                float temperature, int32_t* pos, const int32_t* allowed, int64_t allowed_stride,
                                int32_t top_k, float top_p, const float* noise, const int32_t* forced, int64_t* token,
                                int64_t* out_tokens, int64_t out_stride, int32_t* out_count, int64_t* sampled,
                                const float* emb_table, void* x, int64_t P, int64_t D, void* stream);

/* ld_llm_sample_advance_pairs for the second engine: the same kernel and arguments, 1 <= P <= LD_LLM_MAX_WIDE
 * (LD_ERR_UNSUPPORTED beyond). */
int ld_llm_sample_advance_wide(const float* logits, float* probs, float* cfg_logits, int64_t V, int32_t guided, float scale,
                               float temperature, int32_t* pos, const int32_t* allowed, int64_t allowed_stride,
                               int32_t top_k, float top_p, const float* noise, const int32_t* forced, int64_t* token,
                               int64_t* out_tokens, int64_t out_stride, int32_t* out_count, int64_t* sampled,
                               const float* emb_table, void* x, int64_t P, int64_t D, void* stream);

/* After torch.multinomial: forced-token override (forced[*pos + 1] >= 0), record sampled visual tokens, ++*pos
 * (the elif chain of lm_model.py:455-508). */
int ld_llm_decode_advance(const int64_t* sampled, const int32_t* forced, int32_t* pos, int64_t* token,
                          int64_t* out_tokens, int32_t* out_count, void* stream);

/* ---- scoring of token sequences (ld_llm_score.hip) ---- */

/* Largest vocabulary of the single-workgroup sampling / scoring kernels (ld_llm_logits_to_probs, ld_llm_sample_advance*,
 * ld_llm_token_logprobs). */
#define LD_SAMPLE_MAXV 4096

/* Log-probability of target[r] under the distribution ld_llm_logits_to_probs builds from logits row r (lm_model.py:417-454:
 * CFG `u + s*(c-u)` when guided, / temperature, restriction to allowed[pos + 1], top-k and top-p at unrestricted positions with
 * the same tie, stable-rank and sequential-cumsum rules), n rows, one workgroup each.  Row r's conditional logits are
 * cond + r * cond_stride and its unconditional ones uncond + r * uncond_stride (fp32, V <= LD_SAMPLE_MAXV each; uncond may be NULL
 * when not guided): [2][n][V] is (base, base + n * ld, stride ld), the decode's [2P][V] pairs are (base, base + V, stride 2V).
 * Position of row r: pos[r * pos_stride] + pos_bias when pos != NULL (a device word; after a sampling launch has advanced it,
 * pos_bias = -1 names the position that launch sampled at), else pos_bias + r.  allowed ([n_pos][allowed_stride], as
 * ld_llm_logits_to_probs) and forced ([n_pos], as ld_llm_decode_advance) are the shared schedule, either may be NULL; a row whose
 * pos + 1 is outside [0, n_pos) gets NaN and valid 0 without a table read.
 * logprob[r] = (l_t - max) - log(sum exp(l - max)) [- log(kept mass) under top-p], taken in the log domain: finite wherever the
 * target is in the support, however small its probability; -inf exactly when the restriction, top-k or top-p removes the target
 * (or target is no id of [0, V)).  forced[pos + 1] >= 0: the schedule writes that token, the row is not a draw: logprob 0,
 * valid 0.  valid (optional) is 1 for every other row.  cfg_logits (optional, row r at cfg_logits + r * cfg_stride) receives the
 * guided logits of the rows that are draws with a target in [0, V): the bits ld_llm_logits_to_probs writes to its cfg_logits. */
int ld_llm_token_logprobs(const float* cond, int64_t cond_stride, const float* uncond, int64_t uncond_stride, int64_t n,
                          int64_t V, int32_t guided, float scale, float temperature, const int32_t* pos, int64_t pos_stride,
                          int32_t pos_bias, const int32_t* allowed, int64_t allowed_stride, const int32_t* forced,
                          int64_t n_pos, int32_t top_k, float top_p, const int64_t* target, float* logprob, int32_t* valid,
                          float* cfg_logits, int64_t cfg_stride, void* stream);

/* C[M][N] = A[M][K] . W[N][K]^T, fp32 operands and fp32 accumulation (v_mfma_f32_32x32x2_f32: each element a k-ordered fmaf
 * chain), row strides lda / ldw / ldc in elements: the head of transformer.py:112-118 on every row of a teacher-forced pass (the
 * decode's two rows go through ld_gemv).  Any M, N; K, lda, ldw multiples of 4 and A, W 16-byte aligned (LD_ERR_INVALID
 * otherwise).  Nothing outside [M] x [N] of C is written. */
int ld_llm_head_f32(const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc, int64_t M, int64_t N,
                    int64_t K, void* stream);

/* ---- normalisation kernels (ld_norm_layer.hip, ld_norm_qkv.hip, ld_norm_group.hip) ---- */

/* LayerNorm over D (fp32 statistics) with optional AdaLN modulate `x*(1+scale)+shift` (bf16 ops) whose vectors are
 * picked per row: batch = row / rows_per_batch, region = text if (row % rows_per_batch) < text_len else image;
 * vector = mod + batch*mod_bstride + {shift,scale}_{img,txt}.  (dit_video_concat.py:388,577-586,601-611;
 * also nn.LayerNorm in TiTok blocks.py:292-304 with fp32 in / bf16 out.)
 * x is bf16, or f32 when x_f32; out likewise (out_f32); w, b, mod are bf16, w and b both given or both null.
 * D % 8 == 0 and 0 < D <= 4096 (LD_ERR_INVALID otherwise).  NOT checked -- the rows are read and written in 16-byte pieces: x, out,
 * w, b and every modulation vector 16-byte aligned, hence ldx, ldo multiples of 8 elements for bf16 and 4 for f32, and mod_bstride and
 * the four offsets multiples of 8.  Columns [D, ldo) of out and rows >= `rows` are not written.
 * With mod, bf16 x and out, affine weights and D <= 2048 a two-rows-per-wave kernel runs (LD_LN_FAST=0, a knob like every other -- read once per process, per call under LD_TUNING=1: never);
 * it stores the same bf16 values as the general kernel. */
int ld_layernorm(const void* x, int64_t ldx, int32_t x_f32, const void* w, const void* b, void* out, int64_t ldo,
                 int32_t out_f32, int64_t rows, int64_t D, float eps, const void* mod, int64_t mod_bstride,
                 int64_t shift_img, int64_t scale_img, int64_t shift_txt, int64_t scale_txt,
                 int64_t rows_per_batch, int64_t text_len, void* stream);

/* qkv [B*N][3*H*64] (thirds q|k|v, sat SelfAttention layout) -> Q,K [B][H][Npad][64] (zero padded) and
 * V^T [B][H][64][Npad].  mode 0: LayerNorm(64, eps) on q,k heads (dit_video_concat.py:649-653);
 * mode 1: interleaved-pair RoPE with cos/sin [N][32] (blocks.py:172-180, pos_emb.py:16-46);
 * mode 2: the plain split, no normalisation or rotation (HF ViTSelfAttention of the Theia backbone; no weights needed).
 * Npad % 64 == 0 and Npad >= N; mode 0 needs the four bf16 [64] weight vectors, mode 1 the two f32 tables (LD_ERR_INVALID
 * otherwise).  Rows [N, Npad) of Q and K and columns [N, Npad) of V^T are written as zeros; nothing behind the three tensors is
 * touched.  NOT checked: qkv, Q, K and Vt 16-byte aligned (the qkv row is 3*H*64 elements, so every row is). */
int ld_qkv_split(const void* qkv, void* Q, void* K, void* Vt, int64_t B, int64_t N, int64_t H, int64_t Npad,
                 int32_t mode, const void* q_w, const void* q_b, const void* k_w, const void* k_b, float eps,
                 const float* cos_t, const float* sin_t, void* stream);

/* GroupNorm statistics of channels-last x [F][P][C] (torch.nn.GroupNorm inside Normalize, vq_gan_blocks.py:35-38, and
 * SpatialNorm3D, cp_enc_dec.py:546-569): stats[f][g] = (sum, sum of squares) in double.  No floating-point atomics:
 * partials is a caller-owned workspace of F * ld_groupnorm_stats_blocks(P) * G * 2 doubles, reduced in a fixed order, so
 * the result is bit-identical from run to run.  stats need not be zeroed.
 * C % 8 == 0, C <= 2048, G <= 64, C % G == 0 and C / G either a multiple of 8 or one of 2, 4 (LD_ERR_INVALID otherwise: a thread
 * keeps four sub-group sums of its 8 channels, so one channel per group is not supported).  x 16-byte aligned (not checked). */
int64_t ld_groupnorm_stats_blocks(int64_t P);
int ld_groupnorm_stats(const void* x, double* stats, double* partials, int64_t F, int64_t P, int64_t C, int64_t G, void* stream);

/* The same stats[g] (F = 1) from the partial sums ld_conv_cl_bf16_gn left for an output of P rows x C channels: a fold of the
 * 64-row units into at most 256 double pairs per group (partials: caller-owned workspace of 256 * G * 2 doubles), then the same
 * fixed-order reduce.  The sums are those of the same bf16 values, added in another order (fp32 within a 64 x 4 patch, double
 * above): statistics agree with ld_groupnorm_stats to ~1e-7 relative, not bit for bit.  C / 4 a power of two <= 256, G <= 64,
 * whole quads per group. */
int ld_groupnorm_stats_from_conv(const float* gn_partials, double* stats, double* partials, int64_t P, int64_t C, int64_t G,
                                 void* stream);

/* y = swish?( GN(x) [* zy + zb] ) written into the interior of a zero-bordered channels-last buffer
 * [F][T+tpad][H+2*hpad][W+2*wpad][C]; zy/zb [Tz][Hz][Wz][C] are conv_y(zq)/conv_b(zq) at latent resolution, gathered
 * with SpatialNorm3D's nearest rule incl. the first-frame split for odd T (cp_enc_dec.py:546-569); GroupNorm(32,
 * eps 1e-6) + swish of vq_gan_blocks.py:29-38,90-148 when zy is NULL. */
int ld_groupnorm_apply(const void* x, void* out_padded, const double* stats, const void* gamma, const void* beta,
                       const void* zy, const void* zb, int64_t F, int64_t T, int64_t H, int64_t W, int64_t C,
                       int64_t G, int64_t Tz, int64_t Hz, int64_t Wz, int64_t tpad, int64_t hpad, int64_t wpad,
                       int32_t swish, float eps, void* stream);

/* ---- layout / elementwise kernels (ld_elem.hip) ---- */

/* x [B][T][C][H][W] f32 (-> bf16, + sem [T][C][H][W] bf16 for the control net, dit_video_concat.py:991)
 * -> patch rows [B*T*(H/p)*(W/p)][C*p*p] bf16 for the patch-embed GEMM (:47-62). */
int ld_patchify(const float* x, const void* sem, void* out, int64_t B, int64_t T, int64_t C, int64_t H, int64_t W,
                int64_t p, void* stream);

/* unpatchify (:392-410) + Denoiser.forward `net*c_out + x*c_skip` (denoiser.py:25-41) + CFG `u + s*(c-u)`
 * (guiders.py:75-79): lin [2][T*hp*wp][C*p*p] bf16 (uncond, cond), x/out [T][C][H][W] f32.  fp32; xs = x*c_skip, u = e_u*c_out + xs,
 * c = e_c*c_out + xs and D = c - u are rounded operation by operation as eager torch rounds them; out = fma(s, D, u), one rounding
 * (eager torch rounds s*D first: that rounding, 2^-24 |s*D| at most, is all the two differ by before the last rounding). */
int ld_unpatchify_cfg(const void* lin, const float* x, float* out, int64_t T, int64_t C, int64_t H, int64_t W,
                      int64_t p, float c_out, float c_skip, float scale, void* stream);

/* out = a*x + b*y + c*z (y, z optional) of sampling.py:613-644,771-781, left to right as fma(c, z, fma(b, y, a*x)): a*x is rounded,
 * b*y and c*z enter through one fused multiply-add each (eager torch rounds the products first: a rounding or two of the partial sums
 * apart, bit-equal with x alone).  out may be x, y or z (an element is read before it is written, by the thread that writes it). */
int ld_axpbypcz(float* out, const float* x, float a, const float* y, float b, const float* z, float c, int64_t n, void* stream);

/* ---- clip editing (ld_edit.hip; LanDiffPipeline.edit_video) ----
 * The sampler's re-noise / pin of known latents, the `sdedit` branch of VPSDEDPMPP2MSampler.__call__ (sampling.py:800-835) over any
 * set of latent cells: x [T][C][H][W] f32 in place, mask [T][H][W] u8 broadcast over C (null: every element).  Where the mask is
 * non-zero x = alpha*known + sigma*noise, the two products and the sum rounded separately; with noise null x = known (a copy).
 * Elsewhere x is not written.  noise may alias x; known may not. */
int ld_latent_pin(float* x, const float* known, const float* noise, const uint8_t* mask, float alpha, float sigma, int64_t T,
                  int64_t C, int64_t H, int64_t W, void* stream);

/* Pixel keep-mask [F][Hp][Wp] u8 (non-zero = keep) -> latent keep-mask [(F + 3) / 4][Hp / 8][Wp / 8] u8 (1 / 0): cell (t, i, j)
 * is kept only if every pixel of its block is -- frames {0} for t = 0 and {4t-3 .. 4t} for t >= 1 (the VAE's causal 1 + 4k frame
 * mapping), rows 8i .. 8i+7, columns 8j .. 8j+7.  LD_ERR_INVALID unless F % 4 == 1, Hp % 8 == 0, Wp % 8 == 0 and mask_px is
 * 8-byte aligned. */
int ld_mask_to_latent(const uint8_t* mask_px, uint8_t* out, int64_t F, int64_t Hp, int64_t Wp, void* stream);

/* ---- the conform stage (ld_conform.hip; landiff_amd/conform.py) ----
 * Antialiased separable resampling of uint8 channels-last frames, with a crop box and a frame gather fused in (what torchvision's
 * resize does for the reference, theia_extractor.py:88-90).  src [Fs][Hs][Ws][C], C 1 or 3; dst [n_out][Ho][Wo][C]; output frame k
 * is made from source frame frame_idx[k] (int32 on the device; repeats and any order allowed; null: frame k, n_out <= Fs) -- the
 * caller checks its range, an index outside [0, Fs) is clamped.  Only the box rows y0 .. y0+hc-1, columns x0 .. x0+wc-1 are read.
 * The filter arrives as tables, built by the caller in float64 and rounded to fp32 (landiff_amd/conform.py axis_table), per axis
 * over the box, n_in the box's size along it:  scale = n_in / n_out; half = 1 (filter 0, bilinear: f(x) = 1 - |x|, |x| < 1) or 2
 * (filter 1, bicubic, Keys a = -0.5: f(x) = ((a+2)|x| - (a+3))x^2 + 1, |x| < 1; a(((|x| - 5)|x| + 8)|x| - 4), 1 <= |x| < 2);
 * support = half * scale and inv = 1 / scale when scale >= 1, else half and 1;  c = scale (i + 0.5), lo = max(0, int(c - support
 * + 0.5)), hi = min(n_in, int(c + support + 0.5));  tap j in [lo, hi) weighs f((j - c + 0.5) inv), divided by the taps' sum
 * (PyTorch's antialias weights).  win [n_out][2] int32 = (lo, hi - lo), w [n_out][tmax] f32 = the weights of output i in
 * w[i][0 .. cnt), tmax >= every cnt: any tap count.  A window is clamped into the box and to tmax taps whatever the table holds.
 * value = sum_y w_y (sum_x w_x src): fp32 fma chains, nothing rounded in between, then clamp(round-half-even(v), 0, 255) once.
 * `filter` must be the tables' filter: it sizes the tiles.  LD_ERR_INVALID: null pointer, C not 1 or 3, empty shape, a box that
 * leaves the source, n_out > Fs without frame_idx, unknown filter. */
int ld_resize_u8(const uint8_t* src, uint8_t* dst, const int32_t* frame_idx, const int32_t* win_y, const float* w_y,
                 int64_t tmax_y, const int32_t* win_x, const float* w_x, int64_t tmax_x, int64_t Fs, int64_t Hs, int64_t Ws,
                 int64_t C, int64_t n_out, int64_t Ho, int64_t Wo, int64_t y0, int64_t x0, int64_t hc, int64_t wc,
                 int32_t filter, void* stream);

/* The same geometry over a keep-mask, C = 1, no arithmetic: dst = 1 if every source byte in the window [lo_y, hi_y) x [lo_x, hi_x)
 * of the filter's tables is non-zero, else 0 -- decided by the window's bounds, not by whether a weight happens to be 0; the rule
 * of ld_mask_to_latent one level up (a pixel is kept only if everything it was made from is kept). */
int ld_resize_mask_u8(const uint8_t* src, uint8_t* dst, const int32_t* frame_idx, const int32_t* win_y, const int32_t* win_x,
                      int64_t Fs, int64_t Hs, int64_t Ws, int64_t n_out, int64_t Ho, int64_t Wo, int64_t y0, int64_t x0,
                      int64_t hc, int64_t wc, int32_t filter, void* stream);

/* ---- the retime stage (ld_retime.hip; landiff_amd/retime.py) ----
 * src u8 [F][H][W][C] -> dst u8 [n_out][H][W][C], C 1 or 3: output frame k lies at source position src_idx[k] + phase_p[k] / q
 * (device int32 tables of n_out entries, 0 <= phase_p < q, src_idx + (phase_p > 0) <= F - 1: the caller checks them).  Phase 0
 * copies src[src_idx[k]].  Otherwise, between A = src[i] and B = src[i + 1], every 8 x 8 output block is matched over the
 * 16 x 16 luma window centred on it (Y = (77 R + 150 G + 29 B + 128) >> 8, or the channel itself; every coordinate clamped to the
 * frame): for d = (dy, dx) in [-search, search]^2, per component a = -rhu(p d, q), b = d + a with rhu(n, m) =
 * floor((2 n + m) / (2 m)); SAD(d) = sum |Y_A[y + a] - Y_B[y + b]|; the chosen d minimises (SAD + penalty (|dy| + |dx|),
 * |dy| + |dx|, dy, dx); a chosen SAD above max_sad * 256 makes the block use d = (0, 0); then out = rhu((q - p) A[y + a] +
 * p B[y + b], q) per pixel and channel.  Integer arithmetic only; two runs give the same bits.  mv (may be null): int16
 * [n_out][ceil(H/8)][ceil(W/8)][2] = (dy, dx) after the fallback; sad (may be null): int32 [n_out][ceil(H/8)][ceil(W/8)] = the
 * chosen candidate's SAD; both zero for phase-0 frames.  One launch; all element offsets are 64-bit.  LD_ERR_INVALID: null src,
 * dst, src_idx or phase_p, C not 1 or 3, a size < 1, search outside 0..32, penalty or max_sad outside 0..255, q outside 1..65535. */
int ld_retime_u8(const uint8_t* src, uint8_t* dst, const int32_t* src_idx, const int32_t* phase_p, int32_t q, int16_t* mv,
                 int32_t* sad, int64_t F, int64_t n_out, int64_t H, int64_t W, int64_t C, int32_t search, int32_t penalty,
                 int32_t max_sad, void* stream);

/* ---- the encode stage (ld_jpeg.hip, the rules it shares in ld_jpeg_dev.h; landiff_amd/encode.py) ----
 * Baseline sequential JPEG of uint8 RGB frames, integer arithmetic only, the restart interval one MCU row: every MCU row of every
 * frame is an independent byte-aligned segment (DC predictors reset, the last byte padded with 1-bits, every 0xFF followed by 0x00).
 * subsampling: 420 (MCU 16 x 16, six blocks Y00 Y01 Y10 Y11 Cb Cr) or 444 (MCU 8 x 8, three blocks).  Frames whose size is no
 * multiple of the MCU are extended by edge replication.  The arithmetic (DESIGN 8.12 states every rounding; tests/jpeg_ref.py
 * restates it): Y, Cb, Cr by the JFIF matrix in 16-bit fixed point, (.. + 32768) >> 16, clamped to 0..255; 4:2:0 chroma = the rounded
 * mean of the 2 x 2 cell's converted values; - 128; a separable 8 x 8 DCT, each pass sqrt(8) x the 1-D transform with 13-bit constants, t = (sum + 256)
 * >> 9 after the rows, c8 = (sum + 65536) >> 17 after the columns (8 x the coefficient); q = sign(c8) (|c8| + 4 t) / (8 t) with the quantiser t =
 * clamp((base s + 50) / 100, 1, 255), s = 5000 / quality below 50, else 200 - 2 quality; AC clamped to +-1023; zigzag order; Annex
 * F.1.2 entropy coding with the given Huffman tables.
 * `tables`: LD_JPEG_TABLE_WORDS int32 on the device, built by the caller (landiff_amd/encode.py device_tables: the one place the
 * tables are stated): [0, 64) the DCT matrix K[u][x]; [64, 192) the base quantisation tables, luma then chroma, in zigzag order;
 * [192, 256) the zigzag position of coefficient [v][u]; [256, 272) and [272, 288) the DC codes of luma and chroma by category;
 * [288, 544) and [544, 800) the AC codes of luma and chroma by (run << 4 | size); a code word is code | length << 16.
 * frames [F][H][W][3] with byte strides: row_stride >= 3 W between rows, frame_stride between frames.  All offsets are 64-bit; two
 * runs give the same bits.  LD_ERR_INVALID: a null or misaligned pointer (tables 4, coefficients 16, int64 arrays 8 bytes), quality
 * outside 1..100, an empty shape, strides that do not hold a frame, a capacity below ld_jpeg_size's.  LD_ERR_UNSUPPORTED: another
 * subsampling, W > 8192 or H > 65535 (more than 3072 blocks in a segment).  Both before any launch.
 *
 * ld_jpeg_size: the sizes a caller allocates by, for F frames of H x W (negative: the refusal's code).  FRAME_BLOCKS: 8 x 8 blocks
 * per frame; SEGMENTS: segments (MCU rows) per frame; SEGMENT_BLOCKS: blocks per segment; SEGMENT_BYTES: the most bytes a segment
 * can take = 2 ceil(SEGMENT_BLOCKS * 1658 / 8) (the longest block is 20 + 63 * 26 bits, stuffing at most doubles the bytes);
 * STREAM_BYTES: F (header_bytes + SEGMENTS (SEGMENT_BYTES + 2)), what ld_jpeg_encode_u8's `out` must hold.  The kernels never cut
 * anything to fit: a capacity below the bound is refused. */
#define LD_JPEG_TABLE_WORDS 800
#define LD_JPEG_SIZE_FRAME_BLOCKS 0
#define LD_JPEG_SIZE_SEGMENTS 1
#define LD_JPEG_SIZE_SEGMENT_BLOCKS 2
#define LD_JPEG_SIZE_SEGMENT_BYTES 3
#define LD_JPEG_SIZE_STREAM_BYTES 4
int64_t ld_jpeg_size(int32_t what, int64_t F, int64_t H, int64_t W, int32_t subsampling, int64_t header_bytes);

/* pixels -> quantised coefficients int16 [F][FRAME_BLOCKS][64]: blocks in scan order (MCUs row by row, an MCU's blocks in the order
 * above), a block's coefficients in zigzag order. */
int ld_jpeg_coefs_u8(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables, int16_t* coefs,
                     int64_t F, int64_t H, int64_t W, int32_t subsampling, int32_t quality, void* stream);

/* coefficients int16 [n_seg][mcus_per_row * (6 or 3)][64] -> the entropy-coded, stuffed bytes of every segment, without a marker:
 * segs [n_seg][seg_capacity] (seg_capacity >= SEGMENT_BYTES of the row), seg_len int64 [n_seg].  Any int16 values: AC within
 * +-1023 and DC differences within +-2047 are the caller's to keep (larger ones have no code). */
int ld_jpeg_entropy_i16(const int16_t* coefs, const int32_t* tables, uint8_t* segs, int64_t seg_capacity, int64_t* seg_len,
                        int64_t n_seg, int64_t mcus_per_row, int32_t subsampling, void* stream);

/* pixels -> one contiguous stream per frame in `out`: frame f's bytes are out[offsets[f] .. offsets[f] + lengths[f]), the frames
 * back to back from 0 (offsets, lengths: int64 [F] on the device).  A stream is `header` (header_bytes bytes on the device: SOI ..
 * SOS, equal for every frame of the call; the caller builds it, DRI = MCUs per row), then per MCU row its segment and RST(row mod 8),
 * EOI after the last.  Workspaces: coefs_ws int16 [F][FRAME_BLOCKS][64]; seg_ws int64 [2][F * SEGMENTS].  Four launches: the
 * coefficients, a counting pass of the entropy coder (every segment's stuffed length), the layout (a scan), the writing pass. */
int ld_jpeg_encode_u8(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables,
                      const uint8_t* header, int64_t header_bytes, int16_t* coefs_ws, int64_t* seg_ws, uint8_t* out,
                      int64_t out_capacity, int64_t* offsets, int64_t* lengths, int64_t F, int64_t H, int64_t W,
                      int32_t subsampling, int32_t quality, void* stream);

/* ---- rate control for the encode stage (ld_jpeg_rate.hip; ld_jpeg_c8_u8 in ld_jpeg.hip; landiff_amd/encode.py JpegRateConfig) ----
 * The encode above with the quality found on the device, so that the streams fit a byte budget.  Sizes are exact: a trial's size is
 * counted by the counting pass that lays out the final stream (header, every stuffed segment and its marker); nothing is estimated.
 * Two modes, exactly one a call (the other budget 0): frame_bytes = N, every stream <= N, each frame searching its own quality;
 * clip_bytes = N, the streams together <= N at one quality for all frames.  The search is a stated bisection between the floor q_min
 * and the ceiling q_max: lo = q_min - 1, hi = q_max + 1, the first trial is q_max; a trial that fits sets lo = q, another hi = q;
 * the next trial is (lo + hi) / 2 while hi - lo > 1; the result is max(lo, q_min) with over_budget = (lo == q_min - 1) -- such a
 * frame is still encoded, at q_min; nothing is cut.  Stream size is not monotone in quality, so the result fits and is this
 * bisection's, not necessarily the largest quality that fits.  ROUNDS = 1 + ceil(log2(q_max - q_min + 1)) rounds are queued whatever
 * the data; a frame (clip) that has finished skips the rest, and its trial rows there read (0, 0).
 * The colour conversion and the DCT run once (c8, 8 x the coefficient before the quantiser: |c8| <= 8192, an int16); a round is
 * three launches (quantise c8 at every frame's trial quality, the counting pass, the step that applies the rule), the final encode
 * four (quantise at the chosen qualities, count, layout, write): LAUNCHES = 1 + 3 ROUNDS + 4, no synchronisation, no kernel waits on
 * another's flag.  Integer arithmetic only, 64-bit offsets; two runs give the same bits.
 *
 * ld_jpeg_rate_size: ROUNDS; LAUNCHES; STATE_WORDS = 3 F int32 (state_ws); TRIAL_WORDS = 2 ROUNDS F int64 (trials).  Negative: the
 * refusal's code (q_min <= q_max outside 1..100, an empty shape, an unsupported geometry). */
#define LD_JPEG_RATE_SIZE_ROUNDS 0
#define LD_JPEG_RATE_SIZE_LAUNCHES 1
#define LD_JPEG_RATE_SIZE_STATE_WORDS 2
#define LD_JPEG_RATE_SIZE_TRIAL_WORDS 3
int64_t ld_jpeg_rate_size(int32_t what, int64_t F, int64_t H, int64_t W, int32_t subsampling, int32_t q_min, int32_t q_max);

/* pixels -> c8 int16 [F][FRAME_BLOCKS][64]: ld_jpeg_coefs_u8 up to the quantiser, in its layout (blocks in scan order, zigzag order). */
int ld_jpeg_c8_u8(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables, int16_t* c8, int64_t F,
                  int64_t H, int64_t W, int32_t subsampling, void* stream);

/* c8 [F][frame_blocks][64] and quality int32 [F] on the device (1..100 each, the caller's to keep; 0: the frame is left untouched)
 * -> coefs [F][frame_blocks][64], exactly ld_jpeg_coefs_u8's of frame f at quality[f].  One launch. */
int ld_jpeg_quant_i16(const int16_t* c8, const int32_t* tables, const int32_t* quality, int16_t* coefs, int64_t F,
                      int64_t frame_blocks, int32_t subsampling, void* stream);

/* ld_jpeg_encode_u8 under a budget.  `header`: one template for the call (any quality's); the writing pass stores frame f's two
 * 64-byte DQT bodies at dqt_luma and dqt_chroma of its copy (encode.jpeg_dqt_offsets), so that stream f is byte for byte what
 * ld_jpeg_encode_u8 writes at quality[f].  Workspaces: c8_ws and coefs_ws int16 [F][FRAME_BLOCKS][64]; seg_ws int64 [2][F * SEGMENTS];
 * state_ws int32 [STATE_WORDS].  Outputs, int64 on the device: offsets, lengths, quality, over_budget [F]; trials [ROUNDS][F][2] =
 * (quality, that frame's size) of every trial (trials_capacity: its int64 words).  LD_ERR_INVALID, before any launch: a null or
 * misaligned pointer, q_min or q_max outside 1..100, q_min > q_max, a negative budget, both budgets or neither, DQT offsets outside
 * the header, out_capacity below ld_jpeg_size's STREAM_BYTES, trials_capacity below TRIAL_WORDS. */
int ld_jpeg_encode_rate_u8(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables,
                           const uint8_t* header, int64_t header_bytes, int64_t dqt_luma, int64_t dqt_chroma, int16_t* c8_ws,
                           int16_t* coefs_ws, int64_t* seg_ws, int32_t* state_ws, uint8_t* out, int64_t out_capacity,
                           int64_t* offsets, int64_t* lengths, int64_t* quality, int64_t* over_budget, int64_t* trials,
                           int64_t trials_capacity, int64_t F, int64_t H, int64_t W, int32_t subsampling, int32_t q_min,
                           int32_t q_max, int64_t frame_bytes, int64_t clip_bytes, void* stream);

/* ---- the decode stage (ld_jpeg_dec.hip; landiff_amd/decode.py) ----
 * Baseline JPEG streams on the device -> uint8 RGB frames, integer arithmetic only, equal to libjpeg's (PIL's) decode byte for
 * byte: c = coefficient x quantiser; jidctint's "islow" inverse DCT with 13-bit constants, columns then rows, (x + (1 << (s - 1)))
 * >> s with s = 11 and 18, in 64-bit (any int16 coefficient times any quantiser fits: there is no range refusal); the sample
 * is v + 128 saturated to 0..255; at 4:2:0 the triangle chroma filter (3/4, 1/4 in both axes, roundings 8 and 7, clamped to the real chroma size
 * ceil(H / 2) x ceil(W / 2); plain replication when that is 2 samples wide or fewer); Y, Cb, Cr -> R, G, B with 16-bit constants.
 * DESIGN 8.13 states every formula; tests/jpeg_dec_ref.py restates it.  The host parses the headers (landiff_amd/decode.py
 * parse_jpeg) and refuses what is not SOF0 / 8 bit / three components 4:2:0 or 4:4:4 / one interleaved scan before any launch.
 * All frames of a call have one size and subsampling; W <= 8192, H <= 65535, F <= 65535.
 *
 * `tables`: n_sets table sets of LD_JPEG_DEC_TABLE_WORDS int32 each (decode.decode_tables); frame f uses set tset[f] (clamped to
 * the sets there are).  A set: [0, 192) the quantisers of components 0, 1, 2 in zigzag order; then six Huffman tables of 544 words,
 * DC and AC of component 0, 1, 2: [0, 16) limit[l - 1] = (the last code of length l + 1) << (16 - l), the running value where a
 * length has no code; [16, 32) offset[l - 1] = the index of the first value of length l minus its first code; [32, 288) HUFFVAL;
 * [288, 544) for every 8-bit prefix length << 8 | value of the code it starts with, 0 where that code is longer than 8 bits.
 * `scan` int64 [F][2]: where frame f's entropy-coded data starts in `data` and how many bytes may be searched (to the stream's end);
 * `ri` int32 [F]: its restart interval in MCUs, 0 = none.  Both are clamped into the buffer by the kernels.
 *
 * Segment table int64 [F][S][5] = (frame, start in `data`, length, first MCU, MCU count): row s < ceil(MCUs / ri) (1 without
 * restarts) is the data between restart markers s - 1 and s; rows from that count on are (frame, 0, 0, 0, 0); rows whose marker
 * was not found have start = length = 0.  frame_info int64 [F][3] = (restart markers found, 1 if they are numbered 0..7 in order,
 * the length of the entropy-coded data: up to the first 0xFF that is followed by neither 0x00 nor 0xD0..0xD7).
 * Coefficients int16 [F][FRAME_BLOCKS][64], zigzag order, blocks in scan order: ld_jpeg_coefs_u8's layout.
 * status int32 [F][S], one word per segment (0 for rows past the frame's count): LD_JPEG_DEC_*.  BAD_CODE: no code of <= 16 bits
 * matches, a DC size above 11 or an AC size above 10.  OVERFLOW: a run steps past coefficient 63.  OVERRUN: bits wanted past the
 * segment's end.  MARKERS: the frame's restart markers are not exactly its segment count - 1, numbered in order (every segment of
 * the frame reports it, nothing of the frame is decoded).  RANGE is never reported (the 64-bit passes).  A segment's blocks are
 * all written whatever its status (zeros after the error).
 * Every read of `data` is bounded by the segment's clamped end and every coefficient store by its block, whatever the tables and
 * the stream hold.  LD_ERR_INVALID: a null or misaligned pointer (coefficients 16, int64 arrays and planes 8, int32 arrays 4
 * bytes), an empty shape, strides that do not hold a frame.  LD_ERR_UNSUPPORTED: another subsampling, W > 8192 or H > 65535. */
#define LD_JPEG_DEC_TABLE_WORDS 3456
#define LD_JPEG_DEC_SIZE_FRAME_BLOCKS 0
#define LD_JPEG_DEC_SIZE_MCUS 1
#define LD_JPEG_DEC_SIZE_PLANE_BYTES 2
#define LD_JPEG_DEC_SIZE_TABLE_WORDS 3
#define LD_JPEG_DEC_OK 0
#define LD_JPEG_DEC_BAD_CODE 1
#define LD_JPEG_DEC_OVERFLOW 2
#define LD_JPEG_DEC_OVERRUN 3
#define LD_JPEG_DEC_RANGE 4
#define LD_JPEG_DEC_MARKERS 5
/* the sizes a caller allocates by (negative: the refusal's code): blocks per frame, MCUs per frame (the most segments a frame can
 * have), the bytes of ld_jpeg_decode_rgb's plane workspace per frame, the words of a table set */
int64_t ld_jpeg_dec_size(int32_t what, int64_t H, int64_t W, int32_t subsampling);

/* One workgroup per frame finds every RSTn and the end of the entropy-coded data: seg_table and frame_info as above.  No atomics on
 * global memory; the order is deterministic. */
int ld_jpeg_find_segments(const uint8_t* data, int64_t data_bytes, const int64_t* scan, const int32_t* ri, int64_t* seg_table,
                          int64_t* frame_info, int64_t F, int64_t S, int64_t H, int64_t W, int32_t subsampling, void* stream);

/* Annex F.2.2, one lane per segment: seg_table -> coefs and status.  A stream without restart markers is one lane per frame. */
int ld_jpeg_decode_entropy(const uint8_t* data, int64_t data_bytes, const int64_t* seg_table, const int64_t* frame_info,
                           const int32_t* ri, const int32_t* tables, const int32_t* tset, int64_t n_sets, int16_t* coefs,
                           int32_t* status, int64_t F, int64_t S, int64_t H, int64_t W, int32_t subsampling, void* stream);

/* coefs -> out uint8 [F][H][W][3] with byte strides (row_stride >= 3 W).  Two launches: dequantise + inverse DCT + range limit into
 * planes_ws (F x PLANE_BYTES, 8-byte aligned), then chroma upsampling + colour conversion, stored as whole rows. */
int ld_jpeg_decode_rgb(const int16_t* coefs, const int32_t* tables, const int32_t* tset, int64_t n_sets, uint8_t* planes_ws,
                       uint8_t* out, int64_t frame_stride, int64_t row_stride, int64_t F, int64_t H, int64_t W,
                       int32_t subsampling, void* stream);

/* ---- the decode stage's second entropy route (ld_jpeg_dec_sync.hip; DESIGN 8.14, restated in tests/jpeg_sync_ref.py) ----
 * One lane per subsequence of sub_bytes raw bytes of a restart segment (a power of two in 64 .. 1024) instead of one lane per
 * segment: for streams without restart markers.  coefs and status are exactly ld_jpeg_decode_entropy's, whatever max_rounds is
 * (1 .. 4096): a segment whose subsequences have not agreed after max_rounds rounds, and a segment with an error, is decoded once
 * more by the lane-per-segment kernel in the same call, without a host round trip.  Two runs give the same bits.
 * scan_bytes: an upper bound the host knows of the summed lengths of all segments (the frames' scan bytes; <= data_bytes); it
 * sizes the flat list of subsequences, SUBSEQUENCES = scan_bytes / sub_bytes + F S + 64 F rounded up to 64, and with it the
 * workspace (16-byte aligned) and every grid.  A frame that does not fit the list (a table that ld_jpeg_find_segments did not
 * write) falls back whole.
 * sync_info int32 [F][S][2]: the rounds that changed an exit of the segment (its rounds to the fixed point, at most max_rounds),
 * and 1 if the segment fell back.  exits (optional, with exits_index; for tests) int64 [SUBSEQUENCES][4]: per subsequence the exit
 * state p = 8 x raw byte + bit, j the block within the MCU, k the next zigzag index, and the blocks it completed; exits_index int32
 * [F][S][2]: the segment's first row of `exits` and its rows (0 for rows the frame does not use and for frames with MARKERS).
 * Every refusal answers before a launch. */
#define LD_JPEG_DEC_SYNC_SIZE_WORKSPACE 0
#define LD_JPEG_DEC_SYNC_SIZE_SUBSEQUENCES 1
/* bytes of the workspace / rows of `exits` (negative: the refusal's code; sub_bytes and max_rounds are checked before anything else) */
int64_t ld_jpeg_dec_sync_size(int32_t what, int64_t scan_bytes, int64_t F, int64_t S, int32_t sub_bytes, int32_t max_rounds);

int ld_jpeg_decode_entropy_sync(const uint8_t* data, int64_t data_bytes, const int64_t* seg_table, const int64_t* frame_info,
                                const int32_t* ri, const int32_t* tables, const int32_t* tset, int64_t n_sets, int16_t* coefs,
                                int32_t* status, int64_t F, int64_t S, int64_t H, int64_t W, int32_t subsampling, int64_t scan_bytes,
                                int32_t sub_bytes, int32_t max_rounds, void* workspace, int64_t workspace_bytes, int32_t* sync_info,
                                int64_t* exits, int32_t* exits_index, void* stream);

/* ---- clip comparison (ld_metrics.hip; landiff_amd/metrics.py) ----
 * Two uint8 channels-last clips a, b [F][H][W][C], C 1 or 3 (the pipeline's output layout), and an optional keep-mask [F][H][W] u8
 * (non-zero = counted; null: every pixel).  a and b may alias and need no alignment.  A frame holds fewer than 2^31 bytes.
 *
 * ld_clip_diff_u8: out int64 [F][C][5] = the number of counted pixels n, sum (a-b)^2, sum |a-b|, max |a-b| (0 when n is 0) and
 * the number of counted pixels with a != b, per frame and channel: exact (64-bit sums; integer atomics).  Any H, W >= 1. */
int ld_clip_diff_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, int64_t* out, int64_t F, int64_t H, int64_t W,
                    int64_t C, void* stream);

/* ld_clip_ssim_u8: out double [F][C][2] = (sum of the SSIM map's counted values, their count) per frame and channel; the mean
 * is the caller's division.  Pixel values are floats in [0, 255], L = 255, C1 = (0.01 L)^2, C2 = (0.03 L)^2.  `window`
 * [LD_SSIM_TAPS] f32: the separable window's weights, an 11-tap Gaussian of sigma 1.5 normalised to sum 1, built by the caller in
 * float64 and rounded once.  Valid region only: the map is (H-10) x (W-10), position (y, x) weighs pixels y .. y+10, x .. x+10;
 * H or W < 11 is LD_ERR_INVALID.  With E the windowed mean: mu_x = E[x], var_x = E[x^2] - mu_x^2, cov = E[xy] - mu_x mu_y (biased),
 * ssim = (2 mu_x mu_y + C1)(2 cov + C2) / ((mu_x^2 + mu_y^2 + C1)(var_x + var_y + C2)).  With a mask a position counts when its
 * centre pixel (y+5, x+5) is kept; the window still reads every pixel under it.
 * Arithmetic: fp32, every product and sum rounded on its own (no fma), taps added in ascending order, rows first then columns; the
 * moments are taken of x - 128 and y - 128 (exact, and the variances do not change).  Symmetric in (a, b); exactly 1 where a == b.
 * Map values are added in double: a tile of LD_SSIM_TILE_H x (LD_SSIM_TILE_ELEMS / C) positions by a fixed tree, a frame's tiles
 * in a fixed order, through `workspace` (>= F * tiles_y * tiles_x * C * 2 doubles, checked against workspace_doubles) -- no
 * floating-point atomics: the result is bit-repeatable and a frame's figures do not depend on the other frames of the call. */
#define LD_SSIM_TAPS 11
#define LD_SSIM_TILE_H 32
#define LD_SSIM_TILE_ELEMS 48
int ld_clip_ssim_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, const float* window, double* out, double* workspace,
                    int64_t workspace_doubles, int64_t F, int64_t H, int64_t W, int64_t C, void* stream);

/* timestep_embedding (sgm/modules/diffusionmodules/util.py:207-233): t [B] f32 -> [B][dim] bf16 (cos || sin). */
int ld_timestep_embedding(const float* t, void* out, int64_t B, int64_t dim, float max_period, void* stream);

/* Place a channels-last tensor in [F][Ti][Hi][Wi][Cin] into the interior of a zero-bordered buffer
 * [F][To+tpad][Ho+2*hpad][Wo+2*wpad][Cout].  mode 0 copy (+channel zero pad); mode 1 nearest x2 (time too when
 * time_up, first frame single for odd Ti: Upsample3D, cp_enc_dec.py:605-627); mode 2 PixelShuffle(2).
 * Only the interior is written (To x Ho x Wo positions, all Cout channels, behind tpad leading frames): the caller zeroes the
 * border once.  Cout % 8 == 0; mode 0 Cin <= Cout (any Cin: channels [Cin, Cout) are written as zeros), mode 1 Cin == Cout,
 * mode 2 Cin == 4*Cout (LD_ERR_INVALID otherwise).  NOT checked: out_padded 16-byte aligned; `in` 16-byte aligned with
 * Cin % 8 == 0 in modes 0 (when Cin >= 8) and 1 -- whole 8-channel chunks are moved as one 16-byte word; a mode-0 tail chunk and
 * mode 2 read element by element. */
int ld_place_cl(const void* in, void* out_padded, int64_t F, int64_t Ti, int64_t Hi, int64_t Wi, int64_t Cin,
                int64_t Cout, int32_t mode, int32_t time_up, int64_t tpad, int64_t hpad, int64_t wpad, void* stream);

/* dif_infer.py:37-49 + landiff/utils.py:327-331: x [P][ldx] bf16 (3 channels) -> uint8 [P][3] (truncation) and,
 * optionally, the fp32 video [3][P] in [0,1]. */
int ld_to_uint8(const void* x, int64_t ldx, uint8_t* out, float* video, int64_t P, void* stream);

/* f32 latent ([T][C][H][W] if src_tchw else [C][T][H][W]) -> bf16 channels-last [T][H][W][Cpad], value bf16(bf16(x)*mul)
 * (dif_infer.py:251 `1/scale_factor * latent` on the bf16 samples). */
int ld_latent_to_cl(const float* x, void* out, int64_t T, int64_t C, int64_t H, int64_t W, int64_t Cpad, float mul,
                    int32_t src_tchw, void* stream);

/* ---- DiT step cache (ld_dit_cache.hip; landiff_amd/dit_cache.py).  No reference op site: the reference evaluates every
 * sampler step.  n >= 1 elements of bf16, any n; pointers that are 16-byte aligned take the 16-byte path.  The sums are fp32,
 * reproducible bit for bit (fixed grid = f(n), fixed-order two-stage reduction through `workspace`, no atomics);
 * workspace: LD_DIT_CACHE_WS_FLOATS floats of device memory, free for reuse once the call's launches have run. ---- */
#define LD_DIT_CACHE_WS_FLOATS 4096

/* out[0] = Sum|cur - prev|, out[1] = Sum|prev| (device memory); update_prev != 0: the same pass writes prev <- cur (the sums
 * are those against the OLD prev). */
int ld_absdiff_sums(const void* cur, void* prev, int64_t n, float* out, float* workspace, int32_t update_prev, void* stream);

/* out = bf16(float(a) - float(b)).  old (optional, may be the buffer `out` overwrites): out2[0] = Sum|out - old|,
 * out2[1] = Sum|old| with `out` as rounded; out2 and workspace are needed only with old. */
int ld_residual_sub(const void* a, const void* b, void* out, int64_t n, const void* old, float* out2, float* workspace,
                    void* stream);

/* out = bf16(float(a) + float(r)); out == a is allowed. */
int ld_residual_add(const void* a, const void* r, void* out, int64_t n, void* stream);

/* ---- DiT CFG branch skipping (ld_dit_guidance.hip; landiff_amd/dit_guidance.py).  No reference op site: the reference evaluates
 * both branches on every step.  The final pass of a step in its three forms; fp32, every product and sum rounded on its own:
 *   xs = x*c_skip, d_u = e_u*c_out + xs, d_c = e_c*c_out + xs   (e_u, e_c: the bf16 rows of lin)
 * H and W must be multiples of p.  The sums are reproducible bit for bit (ld_dit_cache.hip's scheme);
 * workspace: LD_DIT_GUIDANCE_WS_FLOATS floats of device memory, free for reuse once the call's launches have run. ---- */
#define LD_DIT_GUIDANCE_WS_FLOATS 5120

/* A full step: lin [2][T*hp*wp][C*p*p] bf16 (uncond, cond), x / out / delta [T][C][H][W] f32.  delta = d_c - d_u,
 * out = fma(scale, delta, d_u) (the bits of ld_unpatchify_cfg as built: its last multiply-add is one fused operation).  sums5 (device memory) = Sum e_u*e_c, Sum e_u^2, Sum e_c^2,
 * Sum|delta - delta_old|, Sum|delta_old|; delta_old may be null (the last two are 0) or the buffer delta overwrites. */
int ld_unpatchify_cfg_keep(const void* lin, const float* x, float* out, float* delta, const float* delta_old, float* sums5,
                           float* workspace, int64_t T, int64_t C, int64_t H, int64_t W, int64_t p, float c_out, float c_skip,
                           float scale, void* stream);

/* A cond-only step: lin_cond [T*hp*wp][C*p*p] bf16.  delta null: out = d_c (scale is not read); else out = d_c + (scale - 1)*delta,
 * scale - 1 formed in fp32. */
int ld_unpatchify_cond(const void* lin_cond, const float* x, float* out, const float* delta, int64_t T, int64_t C, int64_t H,
                       int64_t W, int64_t p, float c_out, float c_skip, float scale, void* stream);

/* ---- 3D-VAE encoder (ld_vae_enc.hip; ContextParallelEncoder3D, cp_enc_dec.py:785-911, + DiagonalGaussianRegularizer,
 * regularizers.py:10-28,96-114).  Its convolutions, GroupNorms and residual adds are ld_conv_cl_bf16[_gn] / ld_groupnorm_*. ---- */

/* Frames [F][H][W][3] (uint8 when frames_u8: x / 127.5 - 1, else f32 in [-1, 1]) -> conv_in's input: bf16
 * [F+2][H+2][W+2][Cpad], EVERY element written -- zero spatial border, channels 3.. zero, time frames 0 and 1 copies of
 * frame 0 (the causal halo without a cache, _fake_cp_pass_from_previous_rank, cp_enc_dec.py:249-300).  Cpad % 8 == 0. */
int ld_vae_enc_place_input(const void* frames, int32_t frames_u8, void* out_padded, int64_t F, int64_t H, int64_t W,
                           int64_t Cpad, void* stream);

/* DownSample3D (cp_enc_dec.py:634-681) up to its conv: x bf16 [T][H][W][C] -> bf16 [To][H/2+2][W/2+2][4C] (every element
 * written), out[t][a][b][(2p+q)*C + c] = x'[t][2a+p][2b+q][c], zero where 2a+p >= H or 2b+q >= W (the (0,1,0,1) pad and one
 * more zero row / column, for ld_conv_cl_bf16's odd kernel sizes).  x' = x,
 * or with compress_time and T > 1 the time pool: frame 0 kept and pairs averaged for odd T, pairs for even T (To = (T+1)/2 or
 * T/2), the mean of two bf16 values in fp32 rounded once.  The 3x3 stride-2 conv is then ld_conv_cl_bf16 as a stride-1 1x3x3
 * conv over 4C channels whose weights are rearranged once, with zeros for the taps that do not exist (2x2 of the 3x3 taps
 * carry weights; landiff_amd/vae_encoder.py: s2d_conv_weight).  C % 8 == 0, H and W even. */
int ld_vae_enc_downsample(const void* x, void* out, int64_t T, int64_t H, int64_t W, int64_t C, int32_t compress_time,
                          void* stream);

/* The posterior of conv_out's f32 output x [T*H*W][ldx] (mean = channels [0, Z), logvar = [Z, 2Z), clamped to [-30, 20]):
 * z [T][Z][H][W] f32 = scale * (mean + exp(0.5 * logvar) * eps) with eps f32 [Z][T][H][W] (randn_like of the reference's
 * [1, Z, T, H, W] mean), or scale * mean when eps is null.  mean / logvar (optional, [T][Z][H][W] f32) get the unscaled values. */
int ld_vae_posterior(const float* x, int64_t ldx, const float* eps, float* z, float* mean, float* logvar, int64_t T,
                     int64_t Z, int64_t H, int64_t W, float scale, void* stream);

/* ---- Theia feature extractor (ld_theia.hip; DeiT-base = HF ViTModel, theia_model.py:441-451 + theia_extractor.py:88-139,
 * run with interpolate=True under bf16 autocast).  Its linears are ld_gemm_bf16, its LayerNorms ld_layernorm, its head split
 * ld_qkv_split mode 2 and its attention ld_attn_fwd_bf16 (B = frames in one launch). ---- */

/* The patch Conv2d's im2col rows: out bf16 [T*P][768], P = (S/16)^2 (integer division), row t*P + py*(S/16) + px, column c*256 + kh*16 + kw
 * (the Conv2d weight's (c, kh, kw) order) = bf16((u - 127.5f) / 127.5f) of pixel (16py + kh, 16px + kw) of channel c
 * (DeiT.yax_processor, theia_model.py:446-451).  nhwc = 0: frames uint8 [T][3][S][S] (H = W = S); nhwc = 1: frames uint8
 * [T][H][W][3] with H, W <= S, padded right and bottom with 127 to S x S as pad_to_square does (condition.py:15-27) without
 * materialising the square.  S >= 16; the last S % 16 rows / columns are dropped, as by the stride-16 Conv2d. */
int ld_vit_patch_rows(const void* frames, int32_t nhwc, void* out, int64_t T, int64_t H, int64_t W, int64_t S, void* stream);

/* ViTEmbeddings after the patch Conv2d: x f32 [T][1+P][C] <- row 0 of each frame pos[0] (CLS + its position, added once on the
 * host), row 1+p float(patch[t*P + p]) + pos[1+p]; patch bf16 [T*P][C] (the Conv2d's bf16 output), pos f32 [1+P][C] the
 * interpolated position table.  C % 4 == 0. */
int ld_vit_embed(const void* patch, const float* pos, float* x, int64_t T, int64_t P, int64_t C, void* stream);

/* The extractor's end: final LayerNorm (fp32 weights, eps) of x f32 [T][N = 1 + s*s][C], CLS dropped, then
 * TheiaExtractor's output_shape rule on the s x s grid: position (i, j) of the (gh, gw) output = token 1 + i*s + j when
 * i < s and j < s, else 0 (the crop branch and the zero-pad-then-crop branch agree on a square grid).  Outputs (either may be
 * null): feat f32 [T][C][gh][gw] (the feature_extractor contract) and cl bf16 [T*gh*gw][C] = bf16((y - mean[c]) / (std[c] +
 * 1e-8)), exactly ld_feature_norm_cl of feat, the TiTok encoder's input rows. */
int ld_vit_tail(const float* x, const float* ln_w, const float* ln_b, float eps, int64_t T, int64_t N, int64_t s,
                int64_t gh, int64_t gw, int64_t C, float* feat, void* cl, const float* mean, const float* stdv, void* stream);

/* ---- T5 text encoders (HF transformers T5EncoderModel called from
 * landiff/llm/modules/text_encoder.py:36-42,82-112 and landiff/diffusion/sgm/modules/encoders/modules.py:249-292) ---- */

/* T5LayerNorm (transformers modeling_t5.py): fp32 variance, bf16(x*rsqrt) then bf16(weight * that); bf16 weight.
 * x and out are dense [rows][D] (row stride D, no leading dimension), D % 8 == 0, rows > 0 (LD_ERR_INVALID otherwise);
 * x, w and out 16-byte aligned (not checked). */
int ld_t5_rmsnorm(const void* x, const void* w, void* out, int64_t rows, int64_t D, float eps, void* stream);

/* T5 self-attention, head_dim 64, N <= 512: q/k/v/out [N][ld] bf16 (head h at columns 64h..64h+63), no score scaling,
 * additive relative-position bias bias_table[bucket[j - i + N - 1]][h] (bf16 [num_buckets][H]), softmax in fp32.
 * bf16 rounding points: q.k, q.k + bias, the probabilities, the output; bucket is int32 [2N - 1].  0 < N <= 512, H > 0,
 * ld >= 64*H and ld % 8 == 0 (LD_ERR_INVALID otherwise); q, k, v and out share ld (they may be column views of one fused
 * [N][3*H*64] buffer) and q, k 16-byte aligned (not checked).  Only columns [0, 64*H) of the N rows of out are written. */
int ld_t5_attn(const void* q, const void* k, const void* v, void* out, int64_t ld, const void* bias_table,
               const int32_t* bucket, int64_t N, int64_t H, void* stream);

#ifdef __cplusplus
}
#endif
#endif
