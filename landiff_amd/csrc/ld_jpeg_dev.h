// What the JPEG stages share, each rule stated once: a frame's geometry and its refusals, the small helpers, the workgroup scan, the
// quantiser and a frame's byte size.  Users: the encode stage (ld_jpeg.hip, ld_jpeg_rate.hip) and, through ld_jpeg_dec_dev.h, the
// decode stage.  Its last part: what ld_jpeg.hip exports to the rate file.  Integer arithmetic only.
#pragma once
#include "ld_common.h"
#include "../../include/landiff_hip.h"

namespace ld_jpeg {

constexpr int kMaxWidth = 8192, kMaxHeight = 65535;          // 3072 blocks per segment at most (1024 MCUs x 3, or 512 x 6); SOF0 holds 16 bits

struct Geom {
  int mcu, bpm, mcux, mcuy, PH, PW;                // MCU edge, blocks per MCU, MCUs per row / column, the planes' padded size
  long mcus, seg_blocks, frame_blocks;             // per frame, per MCU row (a segment of the encoder), per frame
};

// The blocks of an MCU; non-zero: the refusal's code (the message is set).
inline int blocks_per_mcu(const char* who, int32_t subsampling, int* bpm) {
  if (subsampling != 420 && subsampling != 444)
    return ld_set_error(LD_ERR_UNSUPPORTED, "%s: subsampling must be 420 or 444, got %d", who, (int)subsampling);
  *bpm = subsampling == 420 ? 6 : 3;
  return LD_OK;
}

// The geometry of a frame; non-zero: the refusal's code (the message is set).
inline int geometry(const char* who, int64_t H, int64_t W, int32_t subsampling, Geom* g) {
  if (int rc = blocks_per_mcu(who, subsampling, &g->bpm)) return rc;
  LD_REQUIRE(H > 0 && W > 0, "%s: empty shape", who);
  if (W > kMaxWidth || H > kMaxHeight)
    return ld_set_error(LD_ERR_UNSUPPORTED, "%s: frames up to %d wide and %d high are supported, got %lld x %lld (H x W)", who,
                        kMaxWidth, kMaxHeight, (long long)H, (long long)W);
  g->mcu = g->bpm == 6 ? 16 : 8;
  g->mcux = (int)((W + g->mcu - 1) / g->mcu), g->mcuy = (int)((H + g->mcu - 1) / g->mcu);
  g->PW = g->mcux * g->mcu, g->PH = g->mcuy * g->mcu, g->mcus = (long)g->mcux * g->mcuy;
  g->seg_blocks = (long)g->mcux * g->bpm, g->frame_blocks = g->mcus * g->bpm;
  return LD_OK;
}

inline bool aligned(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }
__device__ __forceinline__ long clampl(long v, long lo, long hi) { return v < lo ? lo : v > hi ? hi : v; }
// the component of block j of an MCU of bpm blocks
__device__ __forceinline__ int component_of(int j, int bpm) { return bpm == 6 ? (j < 4 ? 0 : j - 3) : j; }

// exclusive scan of one value per thread over a workgroup of kN threads (tmp: kN values in LDS); the total is returned to every thread
template <int kN, typename V>
__device__ __forceinline__ V block_scan(V v, V* tmp, V* total) {
  const int tid = threadIdx.x;
  tmp[tid] = v;
  __syncthreads();
  for (int o = 1; o < kN; o <<= 1) {
    const V add = tid >= o ? tmp[tid - o] : 0;
    __syncthreads();
    tmp[tid] += add;
    __syncthreads();
  }
  const V incl = tmp[tid];
  *total = tmp[kN - 1];
  __syncthreads();
  return incl - v;
}

// IJG's quality rule on one entry of a base table
__device__ __forceinline__ int quantiser(int base, int quality) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  return min(max((base * s + 50) / 100, 1), 255);
}

// c8 (8 x the DCT coefficient) by the quantiser t, rounded half away from zero; z: the zigzag position (an AC is clamped to 10 bits)
__device__ __forceinline__ int quantise(int c8, int t, int z) {
  int q = (abs(c8) + 4 * t) / (8 * t);
  if (z) q = min(q, 1023);
  return c8 < 0 ? -q : q;
}

// the bytes of frame f's stream: its header, every segment (seg_len [F][rows]) and the segment's marker
__device__ __forceinline__ long frame_bytes(const int64_t* seg_len, long f, int rows, int header_bytes) {
  long n = header_bytes;
  for (int r = 0; r < rows; ++r) n += seg_len[f * rows + r] + 2;
  return n;
}

// ---- the encode stage: what ld_jpeg.hip shares with ld_jpeg_rate.hip.  Offsets into its `tables` (int32 words; LD_JPEG_TABLE_WORDS in all):
constexpr int kTabDct = 0, kTabQuant = 64, kTabZig = 192, kTabDc = 256, kTabAc = 288, kTabWords = LD_JPEG_TABLE_WORDS;
static_assert(kTabAc + 512 == kTabWords, "table layout");

// jpeg_entropy_kernel's arguments, set by name.  The defaults are the off-state: bare segments seg_stride apart, no markers, no headers.
struct EntropyArgs {
  const int16_t* coefs = nullptr;                  // [n_seg][seg_blocks][64]
  const int32_t* tables = nullptr;
  int64_t* seg_len = nullptr;                      // [n_seg]: stuffed bytes of the segment, without its marker
  const int64_t* seg_off = nullptr;                // kWrite: where every segment goes in out (null: seg * seg_stride)
  uint8_t* out = nullptr;
  const uint8_t* header = nullptr;                 // kWrite, with frame_off: copied to the start of every frame
  const int64_t* frame_off = nullptr;
  long seg_stride = 0;
  int seg_blocks = 0, bpm = 0, rows = 1, header_bytes = 0, markers = 0;
  // rate control (null: off).  frame_q [F]: the quality a frame's coefficients were quantised at; 0: the frame's search
  // has finished, its segments are skipped.  kWrite: the frame's two DQT bodies are stored at dqt[0], dqt[1] of its header.
  const int32_t* frame_q = nullptr;
  int dqt[2] = {0, 0};
};

// The streams of an encode call: a segment per MCU row with its marker, every frame behind a copy of the header at offsets[f].
// seg_ws: int64 [2][F mcuy], the segments' lengths, then their offsets.
EntropyArgs stream_args(const int16_t* coefs_ws, const int32_t* tables, int64_t* seg_ws, uint8_t* out, const uint8_t* header,
                        int64_t header_bytes, const int64_t* offsets, int64_t F, const Geom& g);
// What both encode calls check last: the shape, the geometry, the segment count, out_capacity against the bound.  Non-zero: the refusal's code.
int check_streams(const char* who, int64_t F, int64_t H, int64_t W, int32_t subsampling, int64_t header_bytes, int64_t out_capacity, Geom* g);
// jpeg_coefs_kernel into `coefs`; raw: up to the quantiser (c8, `quality` unused).  Checks the strides and the launch's size.
int launch_coefs(const char* who, const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables, int16_t* coefs,
                 int64_t F, int64_t H, int64_t W, const Geom& g, int32_t quality, bool raw, hipStream_t stream);
// The counting pass of stream_args' streams: every segment's stuffed length into seg_ws.
void launch_count(const EntropyArgs& a, int64_t F, hipStream_t stream);
// The stream tail: count -> layout (offsets, lengths) -> write.
void launch_tail(const EntropyArgs& a, int64_t* offsets, int64_t* lengths, int64_t F, hipStream_t stream);

}  // namespace ld_jpeg

