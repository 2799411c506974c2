// The encode stage (landiff_amd/encode.py): uint8 RGB frames on the device -> baseline JPEG streams, one restart
// interval per MCU row.  Integer arithmetic only: no float anywhere in this file.  The rule is restated in numpy in tests/jpeg_ref.py;
// every table (DCT matrix, base quantisation tables, zigzag, Huffman codes) arrives in `tables`, built by landiff_amd/encode.py.
//
// jpeg_coefs_kernel: one wave per 8 x 8 block of one component, four blocks per workgroup.  A lane owns one sample: it converts
//   its pixel (4:2:0 chroma: its 2 x 2 cell, the rounded mean of the four converted values) with the JFIF matrix in 16-bit fixed
//   point, level-shifts, and the two DCT passes go through the wave's 64-word slice of LDS (13-bit constants of sqrt(8) x the DCT; 4 fractional
//   bits between the passes, 8 x the coefficient into the quantiser); the quantised value is stored at its zigzag position.  Coordinates are clamped to
//   the frame: edge replication.
// jpeg_entropy_kernel<kWrite>: one workgroup per segment (an MCU row of a frame).  A thread owns whole blocks: it counts a block's
//   bits, a workgroup scan turns the counts into bit offsets, and the codes are OR-ed into a zeroed LDS window of 32 KiB with LDS
//   atomics (neighbouring blocks share words); a segment longer than the window is walked in pieces, every code clipped to the
//   window word by word -- nothing is cut.  Then a thread owns whole bytes: it counts the 0xFF bytes of its chunk of the window,
//   a second scan gives the stuffed offsets, and (kWrite) the bytes go out, each 0xFF followed by 0x00.  The kWrite = false pass
//   only leaves the stuffed length: the stream layout is known before a byte is written, so the streams are written once, in
//   place, with no bound-sized slot buffer in between.
// jpeg_layout_kernel: one workgroup: per-frame lengths, their exclusive scan, every segment's offset.  64-bit throughout.
// Rate control (ld_jpeg_encode_rate_u8): jpeg_coefs_kernel<raw> stops before the quantiser and keeps c8; a trial is
//   jpeg_quant_kernel (c8 at every frame's trial quality) + the counting pass + jpeg_rate_step_kernel (frame sizes, the stated
//   bisection, the next trial); the final encode is the three passes above on the chosen qualities, the writing pass storing each
//   frame's DQT bodies into its copy of the header.  All rounds are queued at once; a finished frame's workgroups read a 0 and return.
// Nothing depends on the order in which lanes or workgroups finish (ORs, and disjoint stores): two runs give the same bits.
#include "ld_common.h"
#include "../../include/landiff_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxWidth = 8192;                    // 3072 blocks per segment at most (1024 MCUs x 3, or 512 x 6)
constexpr int kMaxHeight = 65535;                  // SOF0 holds 16 bits
constexpr int kMaxSegBlocks = kMaxWidth / 8 * 3;
constexpr int kBlockBits = 20 + 63 * 26;           // the longest block: DC category 11, 63 x (16-bit code + 10 bits)
constexpr int kPieceWords = 8192;                  // the LDS window of the bitstream: 32 KiB
constexpr int kPieceBytes = kPieceWords * 4;
// offsets into `tables` (int32 words; LD_JPEG_TABLE_WORDS in all)
constexpr int kTabDct = 0, kTabQuant = 64, kTabZig = 192, kTabDc = 256, kTabAc = 288, kTabWords = LD_JPEG_TABLE_WORDS;
static_assert(kTabAc + 512 == kTabWords, "table layout");

struct Geom {
  int mcu, bpm, mcux, mcuy;                        // MCU edge in pixels, blocks per MCU, MCUs per row and column
  long seg_blocks, frame_blocks, seg_cap;
};

// The geometry of a frame; false: unsupported (the message is set).
bool geometry(const char* who, int64_t H, int64_t W, int32_t subsampling, Geom* g) {
  if (subsampling != 420 && subsampling != 444) {
    ld_set_error(LD_ERR_UNSUPPORTED, "%s: subsampling must be 420 or 444, got %d", who, (int)subsampling);
    return false;
  }
  if (W > kMaxWidth || H > kMaxHeight) {
    ld_set_error(LD_ERR_UNSUPPORTED, "%s: frames up to %d wide and %d high are supported, got %lld x %lld (H x W)", who, kMaxWidth,
                 kMaxHeight, (long long)H, (long long)W);
    return false;
  }
  g->mcu = subsampling == 420 ? 16 : 8;
  g->bpm = subsampling == 420 ? 6 : 3;
  g->mcux = (int)((W + g->mcu - 1) / g->mcu);
  g->mcuy = (int)((H + g->mcu - 1) / g->mcu);
  g->seg_blocks = (long)g->mcux * g->bpm;
  g->frame_blocks = g->seg_blocks * g->mcuy;
  g->seg_cap = 2 * ((g->seg_blocks * kBlockBits + 7) / 8);     // every byte stuffed: the bound nothing can exceed
  return true;
}

struct CoefArgs {
  const uint8_t* frames;
  const int32_t* tables;
  int16_t* coefs;
  long frame_stride, row_stride, total_blocks, frame_blocks;
  int H, W, mcu, bpm, mcux, quality;
};

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// IJG's quality rule on one entry of a base table (what jpeg_coefs_kernel<false> does while it loads its tables)
__device__ __forceinline__ int quantiser(int base, int quality) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  return min(max((base * s + 50) / 100, 1), 255);
}

// component c (0 Y, 1 Cb, 2 Cr) of one pixel: the JFIF matrix in 16-bit fixed point, rounded, clamped
__device__ __forceinline__ int ycc(const uint8_t* px, int c) {
  const int r = px[0], g = px[1], b = px[2];
  if (c == 0) return clamp255((19595 * r + 38470 * g + 7471 * b + 32768) >> 16);
  if (c == 1) return clamp255((-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32768) >> 16);
  return clamp255((32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32768) >> 16);
}

// kRaw: the same kernel up to the quantiser -- c8 itself is stored (|c8| <= 8192, DESIGN 8.15: an int16 holds it), for the rate search
template <bool kRaw>
__global__ __launch_bounds__(kThreads) void jpeg_coefs_kernel(CoefArgs a) {
  __shared__ int tab[256];                         // DCT matrix [u][x] | quantisers luma, chroma (zigzag order) | zigzag position of [v][u]
  __shared__ int work[4][2][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  {
    int v = a.tables[tid];
    if (!kRaw && tid >= kTabQuant && tid < kTabZig) {       // IJG's quality rule on the base table
      const int s = a.quality < 50 ? 5000 / a.quality : 200 - 2 * a.quality;
      v = min(max((v * s + 50) / 100, 1), 255);
    }
    tab[tid] = v;
  }
  const long gb = (long)blockIdx.x * 4 + wave;
  const bool active = gb < a.total_blocks;
  const int y = lane >> 3, x = lane & 7;
  int comp = 0;
  if (active) {
    const long f = gb / a.frame_blocks;
    const long fb = gb - f * a.frame_blocks;
    const int m = (int)(fb / a.bpm), j = (int)(fb - (long)m * a.bpm);
    const int my = m / a.mcux, mx = m - my * a.mcux;
    const uint8_t* fr = a.frames + f * a.frame_stride;
    int s;
    if (a.bpm == 3 || j < 4) {
      comp = a.bpm == 3 ? j : 0;
      const int py = my * a.mcu + (a.bpm == 3 ? 0 : (j >> 1) * 8) + y, px = mx * a.mcu + (a.bpm == 3 ? 0 : (j & 1) * 8) + x;
      s = ycc(fr + (long)min(py, a.H - 1) * a.row_stride + 3L * min(px, a.W - 1), comp);
    } else {
      comp = j - 3;
      const int py = my * 16 + 2 * y, px = mx * 16 + 2 * x;
      const long r0 = (long)min(py, a.H - 1) * a.row_stride, r1 = (long)min(py + 1, a.H - 1) * a.row_stride;
      const long c0 = 3L * min(px, a.W - 1), c1 = 3L * min(px + 1, a.W - 1);
      s = (ycc(fr + r0 + c0, comp) + ycc(fr + r0 + c1, comp) + ycc(fr + r1 + c0, comp) + ycc(fr + r1 + c1, comp) + 2) >> 2;
    }
    work[wave][0][lane] = s - 128;
  }
  __syncthreads();
  if (active) {                                    // rows: t[y][u], 13 -> 4 fractional bits
    int acc = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += tab[kTabDct + x * 8 + i] * work[wave][0][y * 8 + i];
    work[wave][1][lane] = (acc + 256) >> 9;
  }
  __syncthreads();
  if (active) {                                    // columns: c8[v][u] = 8 x the coefficient, 17 -> 0 fractional bits; lane = (v, u)
    int acc = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += tab[kTabDct + y * 8 + i] * work[wave][1][i * 8 + x];
    const int c8 = (acc + 65536) >> 17;
    const int z = tab[kTabZig + lane];
    if (kRaw) {
      a.coefs[gb * 64 + z] = (int16_t)c8;
      return;
    }
    const int t = tab[kTabQuant + (comp ? 64 : 0) + z];
    int q = (abs(c8) + 4 * t) / (8 * t);           // round half away from zero
    if (z) q = min(q, 1023);
    a.coefs[gb * 64 + z] = (int16_t)(c8 < 0 ? -q : q);
  }
}

// exclusive scan of one value per thread over the workgroup (tmp: kThreads ints); the total is returned to every thread
__device__ __forceinline__ int block_scan(int v, int* tmp, int* total) {
  const int tid = threadIdx.x;
  tmp[tid] = v;
  __syncthreads();
  for (int o = 1; o < kThreads; o <<= 1) {
    const int add = tid >= o ? tmp[tid - o] : 0;
    __syncthreads();
    tmp[tid] += add;
    __syncthreads();
  }
  const int incl = tmp[tid];
  *total = tmp[kThreads - 1];
  __syncthreads();
  return incl - v;
}

__device__ __forceinline__ int bit_size(int a) { return a ? 32 - __clz(a) : 0; }

// Annex F.1.2 for one block: emit(bits, n) once per symbol with its appended value bits, n <= 26.  A DC difference beyond +-2047 or
// an AC beyond +-1023 has no code: its category is clamped, so that whatever the values no block passes kBlockBits (the bits of
// such a value mean nothing).
template <class Emit>
__device__ __forceinline__ void code_block(const int16_t* c, int pred, const uint32_t* dc, const uint32_t* ac, Emit&& emit) {
  const int4* p = reinterpret_cast<const int4*>(c);
  int run = 0;
  for (int g = 0; g < 8; ++g) {
    const int4 q = p[g];
    const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int v = (int)(short)((uint32_t)w[j >> 1] >> (16 * (j & 1)));
      if (g == 0 && j == 0) {
        const int diff = v - pred, s = min(bit_size(abs(diff)), 11);
        const uint32_t h = dc[s];
        emit(((h & 0xffffu) << s) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u)), (int)(h >> 16) + s);
        continue;
      }
      if (v == 0) { ++run; continue; }
      while (run > 15) { const uint32_t h = ac[0xF0]; emit(h & 0xffffu, (int)(h >> 16)); run -= 16; }
      const int s = min(bit_size(abs(v)), 10);
      const uint32_t h = ac[run << 4 | s];
      emit(((h & 0xffffu) << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), (int)(h >> 16) + s);
      run = 0;
    }
  }
  if (run) { const uint32_t h = ac[0]; emit(h & 0xffffu, (int)(h >> 16)); }
}

struct EntropyArgs {
  const int16_t* coefs;                            // [n_seg][seg_blocks][64]
  const int32_t* tables;
  int64_t* seg_len;                                // [n_seg]: stuffed bytes of the segment, without its marker
  const int64_t* seg_off;                          // kWrite: where every segment goes in out (null: seg * seg_stride)
  uint8_t* out;
  const uint8_t* header;                           // kWrite, with frame_off: copied to the start of every frame
  const int64_t* frame_off;
  long seg_stride;
  int seg_blocks, bpm, rows, header_bytes, markers;
  // rate control (null: off).  frame_q [F]: the quality a frame's coefficients were quantised at; 0: the frame's search
  // has finished, its segments are skipped.  kWrite: the frame's two DQT bodies are stored at dqt[0], dqt[1] of its header.
  const int32_t* frame_q;
  int dqt[2];
};

template <bool kWrite>
__global__ __launch_bounds__(kThreads) void jpeg_entropy_kernel(EntropyArgs a) {
  __shared__ uint32_t huff[kTabWords - kTabDc];    // dc luma[16] | dc chroma[16] | ac luma[256] | ac chroma[256]: code | size << 16
  __shared__ int bits[kMaxSegBlocks];              // a block's bit count, then its bit offset in the segment
  __shared__ int tmp[kThreads];
  __shared__ uint32_t win[kPieceWords];            // bit k of the window is bit 31 - (k & 31) of word k >> 5
  const int tid = threadIdx.x;
  const long seg = blockIdx.x;
  const int nb = a.seg_blocks, bpm = a.bpm;
  if (a.frame_q && a.frame_q[seg / a.rows] == 0) return;             // (the whole workgroup: before any barrier)
  for (int i = tid; i < kTabWords - kTabDc; i += kThreads) huff[i] = (uint32_t)a.tables[kTabDc + i];
  __syncthreads();
  const int16_t* coefs = a.coefs + seg * nb * 64;
  // the block whose DC predicts block b's: the previous block of its component in the segment (-1: none, predictor 0)
  auto pred_of = [&](int b) {
    const int j = b % bpm;
    if (bpm == 6 && j > 0 && j < 4) return b - 1;
    if (b < bpm) return -1;
    return bpm == 6 && j == 0 ? b - 3 : b - bpm;
  };
  auto chroma_of = [&](int b) { const int j = b % bpm; return bpm == 6 ? j >= 4 : j > 0; };
  auto walk = [&](int b, auto&& emit) {
    const int pb = pred_of(b), ch = chroma_of(b);
    code_block(coefs + (long)b * 64, pb < 0 ? 0 : (int)coefs[(long)pb * 64], huff + 16 * ch, huff + 32 + 256 * ch, emit);
  };

  // ---- bit counts, then bit offsets: thread t scans the contiguous chunk of blocks [t chunk, (t + 1) chunk) ----
  for (int b = tid; b < nb; b += kThreads) {
    int n = 0;
    walk(b, [&](uint32_t, int k) { n += k; });
    bits[b] = n;
  }
  __syncthreads();
  const int chunk = (nb + kThreads - 1) / kThreads;
  int mine = 0;
  for (int b = tid * chunk; b < min(nb, (tid + 1) * chunk); ++b) mine += bits[b];
  int total_bits;
  int at = block_scan(mine, tmp, &total_bits);     // at most 3072 * 1658 bits: an int holds it
  for (int b = tid * chunk; b < min(nb, (tid + 1) * chunk); ++b) { const int n = bits[b]; bits[b] = at; at += n; }
  __syncthreads();
  const int nbytes = (total_bits + 7) >> 3;        // the last byte is padded with 1-bits

  uint8_t* dst = nullptr;
  if (kWrite) dst = a.out + (a.seg_off ? a.seg_off[seg] : seg * a.seg_stride);
  long written = 0;
  for (int p0 = 0; p0 < nbytes; p0 += kPieceBytes) {           // ---- the window over bytes [p0, p0 + pb) ----
    const int pb = min(kPieceBytes, nbytes - p0), pw = (pb + 3) >> 2;
    const uint32_t w0 = (uint32_t)p0 >> 2;
    const int bit0 = p0 * 8, bit1 = (p0 + pb) * 8;
    for (int i = tid; i < pw; i += kThreads) win[i] = 0;
    __syncthreads();
    // a code of n <= 26 bits at bit `pos` touches at most two words; each is kept only if the window holds it
    auto put = [&](int pos, uint32_t v, int n) {
      const uint32_t w = ((uint32_t)pos >> 5) - w0;              // (a word below the window wraps: only w + 1 == 0, the window's first word, can pass)
      const unsigned long long x = (unsigned long long)v << (64 - n - (pos & 31));
      const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
      if (hi && w < (uint32_t)pw) atomicOr(&win[w], hi);
      if (lo && w + 1 < (uint32_t)pw) atomicOr(&win[w + 1], lo);
    };
    for (int b = tid; b < nb; b += kThreads) {
      int pos = bits[b];
      const int end = b + 1 < nb ? bits[b + 1] : total_bits;
      if (end <= bit0 || pos >= bit1) continue;
      walk(b, [&](uint32_t v, int n) { put(pos, v, n); pos += n; });
    }
    if (tid == 0 && p0 + pb == nbytes && (total_bits & 7)) put(total_bits, (1u << (8 - (total_bits & 7))) - 1u, 8 - (total_bits & 7));
    __syncthreads();
    // ---- whole bytes: thread t owns bytes [t bchunk, (t + 1) bchunk) of the window ----
    const int bchunk = (pb + kThreads - 1) / kThreads;
    const int lo = min(pb, tid * bchunk), hi = min(pb, lo + bchunk);
    auto byte_at = [&](int i) { return (win[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu; };
    int ff = 0;
    for (int i = lo; i < hi; ++i) ff += byte_at(i) == 0xffu;
    int extra;
    const int before = block_scan(ff, tmp, &extra);              // (its first barrier is passed after every lane's last OR)
    if (kWrite) {
      uint8_t* o = dst + written + lo + before;
      for (int i = lo; i < hi; ++i) {
        const uint32_t v = byte_at(i);
        *o++ = (uint8_t)v;
        if (v == 0xffu) *o++ = 0;
      }
    }
    written += pb + extra;
    __syncthreads();                                             // everybody has read its bytes: the window may be zeroed again
  }
  if (!kWrite) {
    if (tid == 0) a.seg_len[seg] = written;
    return;
  }
  if (a.markers && tid == 0) {                      // RSTm after every row but the last, EOI after that
    const int r = (int)(seg % a.rows);
    dst[written] = 0xff;
    dst[written + 1] = r == a.rows - 1 ? 0xd9 : (uint8_t)(0xd0 + (r & 7));
  }
  if (a.frame_off && seg % a.rows == 0) {
    uint8_t* h = a.out + a.frame_off[seg / a.rows];
    const int fq = a.frame_q ? a.frame_q[seg / a.rows] : 0;
    for (int i = tid; i < a.header_bytes; i += kThreads) {
      int v = a.header[i];
      const int l = i - a.dqt[0], c = i - a.dqt[1];                    // the position in the luma / chroma body, if i lies in one
      if (fq && l >= 0 && l < 64) v = quantiser(a.tables[kTabQuant + l], fq);
      else if (fq && c >= 0 && c < 64) v = quantiser(a.tables[kTabQuant + 64 + c], fq);
      h[i] = (uint8_t)v;
    }
  }
}

// seg_len [F][rows] -> lengths [F] = header + sum (len + 2), offsets [F] = their exclusive scan, seg_off [F][rows]
__global__ __launch_bounds__(kThreads) void jpeg_layout_kernel(const int64_t* seg_len, int64_t* seg_off, int64_t* offsets,
                                                              int64_t* lengths, long F, int rows, int header_bytes) {
  __shared__ long part[kThreads];
  const int tid = threadIdx.x;
  const long chunk = (F + kThreads - 1) / kThreads;
  const long f0 = min(F, tid * chunk), f1 = min(F, f0 + chunk);
  long mine = 0;
  for (long f = f0; f < f1; ++f) {
    long n = header_bytes;
    for (int r = 0; r < rows; ++r) n += seg_len[f * rows + r] + 2;
    lengths[f] = n;
    mine += n;
  }
  part[tid] = mine;
  __syncthreads();
  long at = 0;
  for (int t = 0; t < tid; ++t) at += part[t];
  for (long f = f0; f < f1; ++f) {
    offsets[f] = at;
    long o = at + header_bytes;
    for (int r = 0; r < rows; ++r) { seg_off[f * rows + r] = o; o += seg_len[f * rows + r] + 2; }
    at = o;
  }
}

// ---- rate control ----
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
  const int* t = tab + ((bpm == 6 ? j >= 4 : j > 0) ? 64 : 0) + z0;
  const long at = ((f * frame_blocks + b) * 64 + z0) / 8;
  const int4 in = reinterpret_cast<const int4*>(c8)[at];
  const int w[4] = {in.x, in.y, in.z, in.w};
  int o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int q[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = (int)(short)((uint32_t)w[k] >> (16 * h)), d = t[2 * k + h];
      int m = (abs(c) + 4 * d) / (8 * d);            // round half away from zero
      if (z0 + 2 * k + h) m = min(m, 1023);
      q[h] = c < 0 ? -m : m;
    }
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

// jpeg_rate_step_kernel: one workgroup.  Frame sizes from the count pass's segment lengths (header + every segment and its
// marker), in clip mode their total; then the stated bisection, per frame (clip mode: every frame holds the clip's state, so the
// rule is applied once per frame to the same numbers).  After the last round frame_q holds the chosen quality of every frame.
__global__ __launch_bounds__(kThreads) void jpeg_rate_step_kernel(StepArgs a) {
  __shared__ long part[kThreads];
  const int tid = threadIdx.x;
  const long chunk = (a.F + kThreads - 1) / kThreads;
  const long f0 = min(a.F, tid * chunk), f1 = min(a.F, f0 + chunk);
  auto size_of = [&](long f) {
    long n = a.header_bytes;
    for (int r = 0; r < a.rows; ++r) n += a.seg_len[f * a.rows + r] + 2;
    return n;
  };
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

bool aligned(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

int check_shape(const char* who, int64_t F, int64_t H, int64_t W) {
  LD_REQUIRE(F > 0 && H > 0 && W > 0, "%s: empty shape", who);
  LD_REQUIRE(F < (1 << 24), "%s: at most 2^24 - 1 frames a call, got %lld", who, (long long)F);
  return LD_OK;
}

int launch_coefs(const char* who, const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables,
                 int16_t* coefs, int64_t F, int64_t H, int64_t W, const Geom& g, int32_t quality, hipStream_t stream, bool raw = false) {
  LD_REQUIRE(row_stride >= 3 * W && frame_stride >= (H - 1) * row_stride + 3 * W,
             "%s: row_stride %lld / frame_stride %lld do not hold %lld x %lld RGB pixels", who, (long long)row_stride,
             (long long)frame_stride, (long long)H, (long long)W);
  const long total = (long)F * g.frame_blocks;
  LD_REQUIRE((total + 3) / 4 < (1L << 31), "%s: %ld blocks exceed one launch", who, total);
  CoefArgs a{frames, tables, coefs, (long)frame_stride, (long)row_stride, total, g.frame_blocks, (int)H, (int)W, g.mcu, g.bpm, g.mcux,
             (int)quality};
  if (raw) hipLaunchKernelGGL(jpeg_coefs_kernel<true>, dim3((unsigned)((total + 3) / 4)), dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL(jpeg_coefs_kernel<false>, dim3((unsigned)((total + 3) / 4)), dim3(kThreads), 0, stream, a);
  return ld_check_launch(who);
}

}  // namespace

LD_API int64_t ld_jpeg_size(int32_t what, int64_t F, int64_t H, int64_t W, int32_t subsampling, int64_t header_bytes) {
  Geom g;
  if (F <= 0 || H <= 0 || W <= 0 || header_bytes < 0 || F >= (1 << 24))
    return ld_set_error(LD_ERR_INVALID, "ld_jpeg_size: F, H, W must be positive (F < 2^24) and header_bytes >= 0");
  if (!geometry("ld_jpeg_size", H, W, subsampling, &g)) return LD_ERR_UNSUPPORTED;
  switch (what) {
    case LD_JPEG_SIZE_FRAME_BLOCKS: return g.frame_blocks;
    case LD_JPEG_SIZE_SEGMENTS: return g.mcuy;
    case LD_JPEG_SIZE_SEGMENT_BLOCKS: return g.seg_blocks;
    case LD_JPEG_SIZE_SEGMENT_BYTES: return g.seg_cap;
    case LD_JPEG_SIZE_STREAM_BYTES: return F * (header_bytes + (long)g.mcuy * (g.seg_cap + 2));
    default: return ld_set_error(LD_ERR_INVALID, "ld_jpeg_size: unknown quantity %d", (int)what);
  }
}

LD_API int ld_jpeg_coefs_u8(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables, int16_t* coefs,
                            int64_t F, int64_t H, int64_t W, int32_t subsampling, int32_t quality, void* stream) {
  LD_REQUIRE(frames && tables && coefs, "ld_jpeg_coefs_u8: null pointer");
  LD_REQUIRE(aligned(tables, 4) && aligned(coefs, 16), "ld_jpeg_coefs_u8: tables must be 4-byte and coefs 16-byte aligned");
  LD_REQUIRE(quality >= 1 && quality <= 100, "ld_jpeg_coefs_u8: quality must be in 1..100, got %d", (int)quality);
  if (int rc = check_shape("ld_jpeg_coefs_u8", F, H, W)) return rc;
  Geom g;
  if (!geometry("ld_jpeg_coefs_u8", H, W, subsampling, &g)) return LD_ERR_UNSUPPORTED;
  return launch_coefs("ld_jpeg_coefs_u8", frames, frame_stride, row_stride, tables, coefs, F, H, W, g, quality, (hipStream_t)stream);
}

LD_API int ld_jpeg_entropy_i16(const int16_t* coefs, const int32_t* tables, uint8_t* segs, int64_t seg_capacity, int64_t* seg_len,
                               int64_t n_seg, int64_t mcus_per_row, int32_t subsampling, void* stream) {
  LD_REQUIRE(coefs && tables && segs && seg_len, "ld_jpeg_entropy_i16: null pointer");
  LD_REQUIRE(aligned(tables, 4) && aligned(coefs, 16) && aligned(seg_len, 8),
             "ld_jpeg_entropy_i16: tables must be 4-byte, coefs 16-byte and seg_len 8-byte aligned");
  LD_REQUIRE(n_seg > 0 && n_seg < (1L << 31) && mcus_per_row > 0, "ld_jpeg_entropy_i16: empty shape or more than 2^31 - 1 segments");
  if (subsampling != 420 && subsampling != 444)
    return ld_set_error(LD_ERR_UNSUPPORTED, "ld_jpeg_entropy_i16: subsampling must be 420 or 444, got %d", (int)subsampling);
  const int bpm = subsampling == 420 ? 6 : 3;
  if (mcus_per_row * bpm > kMaxSegBlocks)
    return ld_set_error(LD_ERR_UNSUPPORTED, "ld_jpeg_entropy_i16: a segment holds at most %d blocks, got %lld", kMaxSegBlocks,
                        (long long)(mcus_per_row * bpm));
  const long nb = mcus_per_row * bpm, cap = 2 * ((nb * kBlockBits + 7) / 8);
  LD_REQUIRE(seg_capacity >= cap, "ld_jpeg_entropy_i16: seg_capacity %lld is below the bound %ld (ld_jpeg_size)",
             (long long)seg_capacity, cap);
  EntropyArgs a{coefs, tables, seg_len, nullptr, segs, nullptr, nullptr, (long)seg_capacity, (int)nb, bpm, 1, 0, 0, nullptr, {0, 0}};
  hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)n_seg), dim3(kThreads), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3((unsigned)n_seg), dim3(kThreads), 0, (hipStream_t)stream, a);
  return ld_check_launch("ld_jpeg_entropy_i16");
}

LD_API int ld_jpeg_encode_u8(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables,
                             const uint8_t* header, int64_t header_bytes, int16_t* coefs_ws, int64_t* seg_ws, uint8_t* out,
                             int64_t out_capacity, int64_t* offsets, int64_t* lengths, int64_t F, int64_t H, int64_t W,
                             int32_t subsampling, int32_t quality, void* stream) {
  LD_REQUIRE(frames && tables && header && coefs_ws && seg_ws && out && offsets && lengths, "ld_jpeg_encode_u8: null pointer");
  LD_REQUIRE(aligned(tables, 4) && aligned(coefs_ws, 16) && aligned(seg_ws, 8) && aligned(offsets, 8) && aligned(lengths, 8),
             "ld_jpeg_encode_u8: tables must be 4-byte, coefs_ws 16-byte, seg_ws / offsets / lengths 8-byte aligned");
  LD_REQUIRE(quality >= 1 && quality <= 100, "ld_jpeg_encode_u8: quality must be in 1..100, got %d", (int)quality);
  LD_REQUIRE(header_bytes > 0 && header_bytes < (1 << 16), "ld_jpeg_encode_u8: header_bytes must be in 1..65535, got %lld",
             (long long)header_bytes);
  if (int rc = check_shape("ld_jpeg_encode_u8", F, H, W)) return rc;
  Geom g;
  if (!geometry("ld_jpeg_encode_u8", H, W, subsampling, &g)) return LD_ERR_UNSUPPORTED;
  const long n_seg = (long)F * g.mcuy, need = F * (header_bytes + (long)g.mcuy * (g.seg_cap + 2));
  LD_REQUIRE(n_seg < (1L << 31), "ld_jpeg_encode_u8: %ld segments exceed one launch", n_seg);
  LD_REQUIRE(out_capacity >= need, "ld_jpeg_encode_u8: out_capacity %lld is below the bound %ld (ld_jpeg_size)", (long long)out_capacity,
             need);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_coefs("ld_jpeg_encode_u8", frames, frame_stride, row_stride, tables, coefs_ws, F, H, W, g, quality, s)) return rc;
  int64_t* seg_len = seg_ws;
  int64_t* seg_off = seg_ws + n_seg;
  EntropyArgs a{coefs_ws, tables, seg_len, seg_off, out, header, offsets, 0, (int)g.seg_blocks, g.bpm, g.mcuy, (int)header_bytes, 1, nullptr, {0, 0}};
  hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)n_seg), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(jpeg_layout_kernel, dim3(1), dim3(kThreads), 0, s, seg_len, seg_off, offsets, lengths, (long)F, g.mcuy,
                     (int)header_bytes);
  hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3((unsigned)n_seg), dim3(kThreads), 0, s, a);
  return ld_check_launch("ld_jpeg_encode_u8");
}

// ---- rate control ----
LD_API int64_t ld_jpeg_rate_size(int32_t what, int64_t F, int64_t H, int64_t W, int32_t subsampling, int32_t q_min, int32_t q_max) {
  Geom g;
  if (F <= 0 || H <= 0 || W <= 0 || F >= (1 << 24))
    return ld_set_error(LD_ERR_INVALID, "ld_jpeg_rate_size: F, H, W must be positive (F < 2^24)");
  if (q_min < 1 || q_max > 100 || q_min > q_max)
    return ld_set_error(LD_ERR_INVALID, "ld_jpeg_rate_size: q_min <= q_max must lie in 1..100, got %d, %d", (int)q_min, (int)q_max);
  if (!geometry("ld_jpeg_rate_size", H, W, subsampling, &g)) return LD_ERR_UNSUPPORTED;
  const int R = rate_rounds(q_min, q_max);
  switch (what) {
    case LD_JPEG_RATE_SIZE_ROUNDS: return R;
    case LD_JPEG_RATE_SIZE_LAUNCHES: return 1 + 3L * R + 4;
    case LD_JPEG_RATE_SIZE_STATE_WORDS: return 3 * F;
    case LD_JPEG_RATE_SIZE_TRIAL_WORDS: return 2L * R * F;
    default: return ld_set_error(LD_ERR_INVALID, "ld_jpeg_rate_size: unknown quantity %d", (int)what);
  }
}

LD_API int ld_jpeg_c8_u8(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables, int16_t* c8,
                         int64_t F, int64_t H, int64_t W, int32_t subsampling, void* stream) {
  LD_REQUIRE(frames && tables && c8, "ld_jpeg_c8_u8: null pointer");
  LD_REQUIRE(aligned(tables, 4) && aligned(c8, 16), "ld_jpeg_c8_u8: tables must be 4-byte and c8 16-byte aligned");
  if (int rc = check_shape("ld_jpeg_c8_u8", F, H, W)) return rc;
  Geom g;
  if (!geometry("ld_jpeg_c8_u8", H, W, subsampling, &g)) return LD_ERR_UNSUPPORTED;
  return launch_coefs("ld_jpeg_c8_u8", frames, frame_stride, row_stride, tables, c8, F, H, W, g, 0, (hipStream_t)stream, true);
}

namespace {

int launch_quant(const char* who, const int16_t* c8, const int32_t* tables, const int32_t* frame_q, int16_t* coefs, int64_t F,
                 long frame_blocks, int bpm, int uniform, hipStream_t stream) {
  const long wpf = (frame_blocks + kThreads / 8 - 1) / (kThreads / 8);
  LD_REQUIRE(F * wpf < (1L << 31), "%s: %lld frames of %ld blocks exceed one launch", who, (long long)F, frame_blocks);
  hipLaunchKernelGGL(jpeg_quant_kernel, dim3((unsigned)(F * wpf)), dim3(kThreads), 0, stream, c8, tables, frame_q, coefs, frame_blocks,
                     wpf, bpm, uniform);
  return ld_check_launch(who);
}

}  // namespace

LD_API int ld_jpeg_quant_i16(const int16_t* c8, const int32_t* tables, const int32_t* quality, int16_t* coefs, int64_t F,
                             int64_t frame_blocks, int32_t subsampling, void* stream) {
  LD_REQUIRE(c8 && tables && quality && coefs, "ld_jpeg_quant_i16: null pointer");
  LD_REQUIRE(aligned(tables, 4) && aligned(quality, 4) && aligned(c8, 16) && aligned(coefs, 16),
             "ld_jpeg_quant_i16: tables and quality must be 4-byte, c8 and coefs 16-byte aligned");
  LD_REQUIRE(F > 0 && F < (1 << 24) && frame_blocks > 0, "ld_jpeg_quant_i16: empty shape, or more than 2^24 - 1 frames");
  if (subsampling != 420 && subsampling != 444)
    return ld_set_error(LD_ERR_UNSUPPORTED, "ld_jpeg_quant_i16: subsampling must be 420 or 444, got %d", (int)subsampling);
  const int bpm = subsampling == 420 ? 6 : 3;
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
  if (int rc = check_shape(who, F, H, W)) return rc;
  Geom g;
  if (!geometry(who, H, W, subsampling, &g)) return LD_ERR_UNSUPPORTED;
  const long n_seg = (long)F * g.mcuy, need = F * (header_bytes + (long)g.mcuy * (g.seg_cap + 2));
  const int R = rate_rounds(q_min, q_max);
  LD_REQUIRE(n_seg < (1L << 31), "%s: %ld segments exceed one launch", who, n_seg);
  LD_REQUIRE(out_capacity >= need, "%s: out_capacity %lld is below the bound %ld (ld_jpeg_size)", who, (long long)out_capacity, need);
  LD_REQUIRE(trials_capacity >= 2L * R * F, "%s: trials_capacity %lld is below the %ld words of %d rounds (ld_jpeg_rate_size)", who,
             (long long)trials_capacity, 2L * R * F, R);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_coefs(who, frames, frame_stride, row_stride, tables, c8_ws, F, H, W, g, 0, s, true)) return rc;
  int64_t* seg_len = seg_ws;
  int64_t* seg_off = seg_ws + n_seg;
  int32_t* frame_q = state_ws + 2 * F;
  EntropyArgs a{coefs_ws, tables, seg_len, seg_off, out, header, offsets, 0, (int)g.seg_blocks, g.bpm, g.mcuy, (int)header_bytes, 1,
                frame_q, {(int)dqt_luma, (int)dqt_chroma}};
  for (int r = 0; r < R; ++r) {                      // round 0 tries q_max, which the host knows: frame_q is first written by its step
    if (int rc = launch_quant(who, c8_ws, tables, r ? frame_q : nullptr, coefs_ws, F, g.frame_blocks, g.bpm, q_max, s)) return rc;
    EntropyArgs c = a;
    if (r == 0) c.frame_q = nullptr;
    hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)n_seg), dim3(kThreads), 0, s, c);
    StepArgs st{seg_len, state_ws, state_ws + F, frame_q, trials + 2L * r * F, quality, over_budget, (long)F,
                (long)(frame_bytes ? frame_bytes : clip_bytes), g.mcuy, (int)header_bytes, q_min, q_max, r, r == R - 1, clip_bytes != 0};
    hipLaunchKernelGGL(jpeg_rate_step_kernel, dim3(1), dim3(kThreads), 0, s, st);
  }
  if (int rc = launch_quant(who, c8_ws, tables, frame_q, coefs_ws, F, g.frame_blocks, g.bpm, 0, s)) return rc;
  hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)n_seg), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(jpeg_layout_kernel, dim3(1), dim3(kThreads), 0, s, seg_len, seg_off, offsets, lengths, (long)F, g.mcuy,
                     (int)header_bytes);
  hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3((unsigned)n_seg), dim3(kThreads), 0, s, a);
  return ld_check_launch(who);
}
