// Rate control of the encode stage (landiff_amd/encode.py JpegRateConfig; restated in tests/jpeg_rate_ref.py): clips
// encoded to a byte budget, the quality searched on the device.  Integer arithmetic only: no float anywhere in this file.
// ld_jpeg_encode_rate_u8 queues, all at once: ld_jpeg.hip's coefficient kernel up to the quantiser (c8); per round a trial =
// jpeg_quant_kernel (c8 at every frame's trial quality) + ld_jpeg.hip's counting pass + jpeg_rate_step_kernel (frame sizes, the
// stated bisection, the next trial); then jpeg_quant_kernel at the chosen qualities and ld_jpeg.hip's stream tail, whose writing
// pass stores each frame's DQT bodies into its copy of the header.  A finished frame's workgroups read a quality of 0 and return.
// The quantiser, a frame's size and the launchers of ld_jpeg.hip used here are ld_jpeg_dev.h's.
#include "ld_jpeg_dev.h"

using namespace ld_jpeg;

namespace {

constexpr int kThreads = 256;

// jpeg_quant_kernel: c8 [F][frame_blocks][64] (zigzag order) -> the quantised coefficients at frame f's quality: frame_q[f], or
//   `uniform` for every frame where frame_q is null; a frame of quality 0 (its search has finished) is skipped.  A workgroup
//   belongs to one frame and holds that frame's two tables in LDS; a thread owns eight coefficients (one 16-byte load and store).
__global__ __launch_bounds__(kThreads) void jpeg_quant_kernel(const int16_t* c8, const int32_t* tables, const int32_t* frame_q,
                                                              int16_t* coefs, long frame_blocks, long wg_per_frame, int bpm, int uniform) {
  __shared__ int tab[128];
  const int tid = threadIdx.x;
  const long f = blockIdx.x / wg_per_frame, wg = blockIdx.x - f * wg_per_frame;
  const int quality = frame_q ? frame_q[f] : uniform;
  if (quality == 0) return;
  if (tid < 128) tab[tid] = quantiser(tables[kTabQuant + tid], quality);
  __syncthreads();
  const long b = wg * (kThreads / 8) + (tid >> 3);                   // the block within the frame
  if (b >= frame_blocks) return;
  const int j = (int)(b % bpm), z0 = (tid & 7) * 8;
  const int* t = tab + (component_of(j, bpm) ? 64 : 0) + z0;
  const long at = ((f * frame_blocks + b) * 64 + z0) / 8;
  const int4 in = reinterpret_cast<const int4*>(c8)[at];
  const int w[4] = {in.x, in.y, in.z, in.w};
  int o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int q[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) q[h] = quantise((int)(short)((uint32_t)w[k] >> (16 * h)), t[2 * k + h], z0 + 2 * k + h);
    o[k] = (q[0] & 0xffff) | (int)((uint32_t)q[1] << 16);
  }
  reinterpret_cast<int4*>(coefs)[at] = make_int4(o[0], o[1], o[2], o[3]);
}

struct StepArgs {
  const int64_t* seg_len;                          // [F][rows] of this round's trial (stale for frames that have finished)
  int32_t* lo;                                     // [F] the search's state: the largest quality known to fit (q_min - 1: none yet)
  int32_t* hi;                                     // [F] the smallest quality known not to fit (q_max + 1: none yet)
  int32_t* frame_q;                                // [F] in: this round's trial (round 0: q_max, nothing is read); out: the next, 0 = finished
  int64_t* trial;                                  // [F][2] this round's (quality, size) rows
  int64_t* quality;                                // [F] written in the last round
  int64_t* over;                                   // [F]
  long F, budget;
  int rows, header_bytes, q_min, q_max, round, last, clip;
};

// jpeg_rate_step_kernel: one workgroup.  Frame sizes from the count pass's segment lengths (frame_bytes), in clip mode their
// total; then the stated bisection, per frame (clip mode: every frame holds the clip's state, so the rule is applied once per
// frame to the same numbers).  After the last round frame_q holds the chosen quality of every frame.
__global__ __launch_bounds__(kThreads) void jpeg_rate_step_kernel(StepArgs a) {
  __shared__ long part[kThreads];
  const int tid = threadIdx.x;
  const long chunk = (a.F + kThreads - 1) / kThreads;
  const long f0 = min(a.F, tid * chunk), f1 = min(a.F, f0 + chunk);
  auto size_of = [&](long f) { return frame_bytes(a.seg_len, f, a.rows, a.header_bytes); };
  auto active = [&](long f) { return a.round == 0 || a.frame_q[f] != 0; };
  long total = 0;
  if (a.clip) {                                    // (all frames are active or none)
    long mine = 0;
    for (long f = f0; f < f1; ++f) if (active(f)) mine += size_of(f);
    part[tid] = mine;
    __syncthreads();
    for (int t = 0; t < kThreads; ++t) total += part[t];
  }
  for (long f = f0; f < f1; ++f) {
    int lo = a.round == 0 ? a.q_min - 1 : a.lo[f], hi = a.round == 0 ? a.q_max + 1 : a.hi[f];
    int next = 0;
    if (active(f)) {
      const int q = a.round == 0 ? a.q_max : a.frame_q[f];
      const long n = size_of(f);
      if ((a.clip ? total : n) <= a.budget) lo = q; else hi = q;
      a.trial[2 * f] = q;
      a.trial[2 * f + 1] = n;
      if (hi - lo > 1) next = (lo + hi) / 2;       // (lo + hi >= 1: the quotient is the floor)
    } else {
      a.trial[2 * f] = 0;
      a.trial[2 * f + 1] = 0;
    }
    a.lo[f] = lo;
    a.hi[f] = hi;
    if (a.last) {
      next = max(lo, a.q_min);
      a.quality[f] = next;
      a.over[f] = lo == a.q_min - 1;
    }
    a.frame_q[f] = next;
  }
}

int rate_rounds(int q_min, int q_max) {            // 1 + ceil(log2(q_max - q_min + 1))
  int r = 1;
  for (int n = q_max - q_min + 1; n > 1; n = (n + 1) / 2) ++r;
  return r;
}

int launch_quant(const char* who, const int16_t* c8, const int32_t* tables, const int32_t* frame_q, int16_t* coefs, int64_t F,
                 long frame_blocks, int bpm, int uniform, hipStream_t stream) {
  const long wpf = (frame_blocks + kThreads / 8 - 1) / (kThreads / 8);
  LD_REQUIRE(F * wpf < (1L << 31), "%s: %lld frames of %ld blocks exceed one launch", who, (long long)F, frame_blocks);
  hipLaunchKernelGGL(jpeg_quant_kernel, dim3((unsigned)(F * wpf)), dim3(kThreads), 0, stream, c8, tables, frame_q, coefs, frame_blocks,
                     wpf, bpm, uniform);
  return ld_check_launch(who);
}

// what every round's step of one search takes (trial, round and last are set per round); state_ws: int32 [3][F] = lo, hi, frame_q
StepArgs step_args(const EntropyArgs& e, int64_t F, int32_t* state_ws, int64_t* quality, int64_t* over, int q_min, int q_max, int64_t budget,
                   bool clip) {
  StepArgs a;
  a.seg_len = e.seg_len, a.rows = e.rows, a.header_bytes = e.header_bytes, a.F = (long)F;
  a.lo = state_ws, a.hi = state_ws + F, a.frame_q = state_ws + 2 * F, a.quality = quality, a.over = over;
  a.q_min = q_min, a.q_max = q_max, a.budget = (long)budget, a.clip = clip;
  return a;
}

}  // namespace

LD_API int64_t ld_jpeg_rate_size(int32_t what, int64_t F, int64_t H, int64_t W, int32_t subsampling, int32_t q_min, int32_t q_max) {
  Geom g;
  if (F <= 0 || H <= 0 || W <= 0 || F >= (1 << 24))
    return ld_set_error(LD_ERR_INVALID, "ld_jpeg_rate_size: F, H, W must be positive (F < 2^24)");
  if (q_min < 1 || q_max > 100 || q_min > q_max)
    return ld_set_error(LD_ERR_INVALID, "ld_jpeg_rate_size: q_min <= q_max must lie in 1..100, got %d, %d", (int)q_min, (int)q_max);
  if (int rc = geometry("ld_jpeg_rate_size", H, W, subsampling, &g)) return rc;
  const int R = rate_rounds(q_min, q_max);
  switch (what) {
    case LD_JPEG_RATE_SIZE_ROUNDS: return R;
    case LD_JPEG_RATE_SIZE_LAUNCHES: return 1 + 3L * R + 4;
    case LD_JPEG_RATE_SIZE_STATE_WORDS: return 3 * F;
    case LD_JPEG_RATE_SIZE_TRIAL_WORDS: return 2L * R * F;
    default: return ld_set_error(LD_ERR_INVALID, "ld_jpeg_rate_size: unknown quantity %d", (int)what);
  }
}

LD_API int ld_jpeg_quant_i16(const int16_t* c8, const int32_t* tables, const int32_t* quality, int16_t* coefs, int64_t F,
                             int64_t frame_blocks, int32_t subsampling, void* stream) {
  LD_REQUIRE(c8 && tables && quality && coefs, "ld_jpeg_quant_i16: null pointer");
  LD_REQUIRE(aligned(tables, 4) && aligned(quality, 4) && aligned(c8, 16) && aligned(coefs, 16),
             "ld_jpeg_quant_i16: tables and quality must be 4-byte, c8 and coefs 16-byte aligned");
  LD_REQUIRE(F > 0 && F < (1 << 24) && frame_blocks > 0, "ld_jpeg_quant_i16: empty shape, or more than 2^24 - 1 frames");
  int bpm;
  if (int rc = blocks_per_mcu("ld_jpeg_quant_i16", subsampling, &bpm)) return rc;
  LD_REQUIRE(frame_blocks % bpm == 0, "ld_jpeg_quant_i16: frame_blocks %lld is no multiple of the %d blocks of an MCU",
             (long long)frame_blocks, bpm);
  return launch_quant("ld_jpeg_quant_i16", c8, tables, quality, coefs, F, (long)frame_blocks, bpm, 0, (hipStream_t)stream);
}

LD_API int ld_jpeg_encode_rate_u8(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables,
                                  const uint8_t* header, int64_t header_bytes, int64_t dqt_luma, int64_t dqt_chroma, int16_t* c8_ws,
                                  int16_t* coefs_ws, int64_t* seg_ws, int32_t* state_ws, uint8_t* out, int64_t out_capacity,
                                  int64_t* offsets, int64_t* lengths, int64_t* quality, int64_t* over_budget, int64_t* trials,
                                  int64_t trials_capacity, int64_t F, int64_t H, int64_t W, int32_t subsampling, int32_t q_min,
                                  int32_t q_max, int64_t frame_bytes, int64_t clip_bytes, void* stream) {
  const char* who = "ld_jpeg_encode_rate_u8";
  LD_REQUIRE(frames && tables && header && c8_ws && coefs_ws && seg_ws && state_ws && out && offsets && lengths && quality &&
                 over_budget && trials, "%s: null pointer", who);
  LD_REQUIRE(aligned(tables, 4) && aligned(state_ws, 4) && aligned(c8_ws, 16) && aligned(coefs_ws, 16) && aligned(seg_ws, 8) &&
                 aligned(offsets, 8) && aligned(lengths, 8) && aligned(quality, 8) && aligned(over_budget, 8) && aligned(trials, 8),
             "%s: tables / state_ws must be 4-byte, c8_ws / coefs_ws 16-byte, seg_ws / offsets / lengths / quality / over_budget / "
             "trials 8-byte aligned", who);
  LD_REQUIRE(q_min >= 1 && q_max <= 100, "%s: q_min and q_max must be in 1..100, got %d, %d", who, (int)q_min, (int)q_max);
  LD_REQUIRE(q_min <= q_max, "%s: q_min %d is above q_max %d", who, (int)q_min, (int)q_max);
  LD_REQUIRE(frame_bytes >= 0 && clip_bytes >= 0, "%s: a budget must be >= 1 (0: that mode is off), got frame_bytes %lld, clip_bytes %lld",
             who, (long long)frame_bytes, (long long)clip_bytes);
  LD_REQUIRE(!(frame_bytes && clip_bytes), "%s: frame_bytes and clip_bytes are both given: exactly one mode a call", who);
  LD_REQUIRE(frame_bytes || clip_bytes, "%s: neither frame_bytes nor clip_bytes is given: exactly one mode a call", who);
  LD_REQUIRE(header_bytes > 0 && header_bytes < (1 << 16), "%s: header_bytes must be in 1..65535, got %lld", who, (long long)header_bytes);
  LD_REQUIRE(dqt_luma >= 0 && dqt_luma + 64 <= dqt_chroma && dqt_chroma + 64 <= header_bytes,
             "%s: dqt_luma %lld / dqt_chroma %lld are no two 64-byte bodies within the header's %lld bytes", who, (long long)dqt_luma,
             (long long)dqt_chroma, (long long)header_bytes);
  Geom g;
  if (int rc = check_streams(who, F, H, W, subsampling, header_bytes, out_capacity, &g)) return rc;
  const int R = rate_rounds(q_min, q_max);
  LD_REQUIRE(trials_capacity >= 2L * R * F, "%s: trials_capacity %lld is below the %ld words of %d rounds (ld_jpeg_rate_size)", who,
             (long long)trials_capacity, 2L * R * F, R);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_coefs(who, frames, frame_stride, row_stride, tables, c8_ws, F, H, W, g, 0, true, s)) return rc;
  EntropyArgs a = stream_args(coefs_ws, tables, seg_ws, out, header, header_bytes, offsets, F, g);
  StepArgs st = step_args(a, F, state_ws, quality, over_budget, q_min, q_max, frame_bytes ? frame_bytes : clip_bytes, clip_bytes != 0);
  for (int r = 0; r < R; ++r) {                      // round 0 tries q_max, which the host knows: frame_q is first written by its step
    a.frame_q = r ? st.frame_q : nullptr;
    if (int rc = launch_quant(who, c8_ws, tables, a.frame_q, coefs_ws, F, g.frame_blocks, g.bpm, q_max, s)) return rc;
    launch_count(a, F, s);
    st.trial = trials + 2L * r * F, st.round = r, st.last = r == R - 1;
    hipLaunchKernelGGL(jpeg_rate_step_kernel, dim3(1), dim3(kThreads), 0, s, st);
  }
  a.frame_q = st.frame_q, a.dqt[0] = (int)dqt_luma, a.dqt[1] = (int)dqt_chroma;
  if (int rc = launch_quant(who, c8_ws, tables, a.frame_q, coefs_ws, F, g.frame_blocks, g.bpm, 0, s)) return rc;
  launch_tail(a, offsets, lengths, F, s);
  return ld_check_launch(who);
}
