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
// The geometry, the quantiser and a frame's size are ld_jpeg_dev.h's; so are the launchers through which rate control (ld_jpeg_rate.hip)
// queues jpeg_coefs_kernel<raw>, which keeps c8, the counting pass and the stream tail (count -> layout -> write) with a quality per frame.
// Nothing depends on the order in which lanes or workgroups finish (ORs, and disjoint stores): two runs give the same bits.
#include "ld_jpeg_dev.h"

using namespace ld_jpeg;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSegBlocks = kMaxWidth / 8 * 3;
constexpr int kBlockBits = 20 + 63 * 26;           // the longest block: DC category 11, 63 x (16-bit code + 10 bits)
constexpr int kPieceWords = 8192;                  // the LDS window of the bitstream: 32 KiB
constexpr int kPieceBytes = kPieceWords * 4;

// the most bytes of a segment of seg_blocks blocks (every byte stuffed: the bound nothing can exceed), and of F streams
long seg_cap(long seg_blocks) { return 2 * ((seg_blocks * kBlockBits + 7) / 8); }
long stream_cap(int64_t F, int64_t header_bytes, const Geom& g) { return F * (header_bytes + (long)g.mcuy * (seg_cap(g.seg_blocks) + 2)); }

struct CoefArgs {
  const uint8_t* frames;
  const int32_t* tables;
  int16_t* coefs;
  long frame_stride, row_stride, total_blocks, frame_blocks;
  int H, W, mcu, bpm, mcux, quality;
};

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
  tab[tid] = !kRaw && tid >= kTabQuant && tid < kTabZig ? quantiser(a.tables[tid], a.quality) : a.tables[tid];
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
    a.coefs[gb * 64 + z] = (int16_t)quantise(c8, tab[kTabQuant + (comp ? 64 : 0) + z], z);
  }
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
  // the block whose DC predicts block b's: the previous block of its component in the segment (negative: none, predictor 0).
  // 4:2:0 (Y Y Y Y Cb Cr): j = 1..3 -> b - 1, j = 0 -> b - 3 (the last Y of the MCU before), j = 4, 5 -> b - 6; 4:4:4 (Y Cb Cr): b - 3.
  // In the segment's first MCU b - 3 and b - 6 are negative, b - 1 (j >= 1) is not.  Only `< 0` is tested.
  auto pred_of = [&](int b) { const int j = b % bpm; return b - (component_of(j, bpm) ? bpm : j ? 1 : 3); };
  auto chroma_of = [&](int b) { return component_of(b % bpm, bpm) != 0; };
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
  int at = block_scan<kThreads>(mine, tmp, &total_bits);    // at most 3072 * 1658 bits: an int holds it
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
    const int before = block_scan<kThreads>(ff, tmp, &extra);          // (its first barrier is passed after every lane's last OR)
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

// seg_len [F][rows] -> lengths [F] (frame_bytes), offsets [F] = their exclusive scan, seg_off [F][rows]
__global__ __launch_bounds__(kThreads) void jpeg_layout_kernel(const int64_t* seg_len, int64_t* seg_off, int64_t* offsets,
                                                              int64_t* lengths, long F, int rows, int header_bytes) {
  __shared__ long part[kThreads];
  const int tid = threadIdx.x;
  const long chunk = (F + kThreads - 1) / kThreads;
  const long f0 = min(F, tid * chunk), f1 = min(F, f0 + chunk);
  long mine = 0;
  for (long f = f0; f < f1; ++f) {
    const long n = frame_bytes(seg_len, f, rows, header_bytes);
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

int check_shape(const char* who, int64_t F, int64_t H, int64_t W) {
  LD_REQUIRE(F > 0 && H > 0 && W > 0, "%s: empty shape", who);
  LD_REQUIRE(F < (1 << 24), "%s: at most 2^24 - 1 frames a call, got %lld", who, (long long)F);
  return LD_OK;
}

}  // namespace

EntropyArgs ld_jpeg::stream_args(const int16_t* coefs_ws, const int32_t* tables, int64_t* seg_ws, uint8_t* out, const uint8_t* header,
                                 int64_t header_bytes, const int64_t* offsets, int64_t F, const Geom& g) {
  EntropyArgs a;
  a.coefs = coefs_ws, a.tables = tables, a.seg_blocks = (int)g.seg_blocks, a.bpm = g.bpm, a.rows = g.mcuy, a.markers = 1, a.out = out;
  a.seg_len = seg_ws, a.seg_off = seg_ws + F * g.mcuy, a.header = header, a.header_bytes = (int)header_bytes, a.frame_off = offsets;
  return a;
}

int ld_jpeg::check_streams(const char* who, int64_t F, int64_t H, int64_t W, int32_t subsampling, int64_t header_bytes, int64_t out_capacity, Geom* g) {
  if (int rc = check_shape(who, F, H, W)) return rc;
  if (int rc = geometry(who, H, W, subsampling, g)) return rc;
  const long n_seg = (long)F * g->mcuy, need = stream_cap(F, header_bytes, *g);
  LD_REQUIRE(n_seg < (1L << 31), "%s: %ld segments exceed one launch", who, n_seg);
  LD_REQUIRE(out_capacity >= need, "%s: out_capacity %lld is below the bound %ld (ld_jpeg_size)", who, (long long)out_capacity, need);
  return LD_OK;
}

int ld_jpeg::launch_coefs(const char* who, const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables,
                      int16_t* coefs, int64_t F, int64_t H, int64_t W, const Geom& g, int32_t quality, bool raw, hipStream_t stream) {
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

void ld_jpeg::launch_count(const EntropyArgs& a, int64_t F, hipStream_t stream) {
  hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)(F * a.rows)), dim3(kThreads), 0, stream, a);
}

void ld_jpeg::launch_tail(const EntropyArgs& a, int64_t* offsets, int64_t* lengths, int64_t F, hipStream_t stream) {
  launch_count(a, F, stream);
  hipLaunchKernelGGL(jpeg_layout_kernel, dim3(1), dim3(kThreads), 0, stream, a.seg_len, a.seg_len + F * a.rows, offsets, lengths, (long)F, a.rows,
                     a.header_bytes);
  hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3((unsigned)(F * a.rows)), dim3(kThreads), 0, stream, a);
}

LD_API int64_t ld_jpeg_size(int32_t what, int64_t F, int64_t H, int64_t W, int32_t subsampling, int64_t header_bytes) {
  Geom g;
  if (F <= 0 || H <= 0 || W <= 0 || header_bytes < 0 || F >= (1 << 24))
    return ld_set_error(LD_ERR_INVALID, "ld_jpeg_size: F, H, W must be positive (F < 2^24) and header_bytes >= 0");
  if (int rc = geometry("ld_jpeg_size", H, W, subsampling, &g)) return rc;
  switch (what) {
    case LD_JPEG_SIZE_FRAME_BLOCKS: return g.frame_blocks;
    case LD_JPEG_SIZE_SEGMENTS: return g.mcuy;
    case LD_JPEG_SIZE_SEGMENT_BLOCKS: return g.seg_blocks;
    case LD_JPEG_SIZE_SEGMENT_BYTES: return seg_cap(g.seg_blocks);
    case LD_JPEG_SIZE_STREAM_BYTES: return stream_cap(F, header_bytes, g);
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
  if (int rc = geometry("ld_jpeg_coefs_u8", H, W, subsampling, &g)) return rc;
  return launch_coefs("ld_jpeg_coefs_u8", frames, frame_stride, row_stride, tables, coefs, F, H, W, g, quality, false, (hipStream_t)stream);
}

LD_API int ld_jpeg_c8_u8(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables, int16_t* c8,
                         int64_t F, int64_t H, int64_t W, int32_t subsampling, void* stream) {
  LD_REQUIRE(frames && tables && c8, "ld_jpeg_c8_u8: null pointer");
  LD_REQUIRE(aligned(tables, 4) && aligned(c8, 16), "ld_jpeg_c8_u8: tables must be 4-byte and c8 16-byte aligned");
  if (int rc = check_shape("ld_jpeg_c8_u8", F, H, W)) return rc;
  Geom g;
  if (int rc = geometry("ld_jpeg_c8_u8", H, W, subsampling, &g)) return rc;
  return launch_coefs("ld_jpeg_c8_u8", frames, frame_stride, row_stride, tables, c8, F, H, W, g, 0, true, (hipStream_t)stream);
}

LD_API int ld_jpeg_entropy_i16(const int16_t* coefs, const int32_t* tables, uint8_t* segs, int64_t seg_capacity, int64_t* seg_len,
                               int64_t n_seg, int64_t mcus_per_row, int32_t subsampling, void* stream) {
  LD_REQUIRE(coefs && tables && segs && seg_len, "ld_jpeg_entropy_i16: null pointer");
  LD_REQUIRE(aligned(tables, 4) && aligned(coefs, 16) && aligned(seg_len, 8),
             "ld_jpeg_entropy_i16: tables must be 4-byte, coefs 16-byte and seg_len 8-byte aligned");
  LD_REQUIRE(n_seg > 0 && n_seg < (1L << 31) && mcus_per_row > 0, "ld_jpeg_entropy_i16: empty shape or more than 2^31 - 1 segments");
  int bpm;
  if (int rc = blocks_per_mcu("ld_jpeg_entropy_i16", subsampling, &bpm)) return rc;
  if (mcus_per_row * bpm > kMaxSegBlocks)
    return ld_set_error(LD_ERR_UNSUPPORTED, "ld_jpeg_entropy_i16: a segment holds at most %d blocks, got %lld", kMaxSegBlocks,
                        (long long)(mcus_per_row * bpm));
  const long nb = mcus_per_row * bpm, cap = seg_cap(nb);
  LD_REQUIRE(seg_capacity >= cap, "ld_jpeg_entropy_i16: seg_capacity %lld is below the bound %ld (ld_jpeg_size)",
             (long long)seg_capacity, cap);
  EntropyArgs a;
  a.coefs = coefs, a.tables = tables, a.seg_blocks = (int)nb, a.bpm = bpm, a.seg_len = seg_len, a.out = segs, a.seg_stride = (long)seg_capacity;
  hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)n_seg), dim3(kThreads), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3((unsigned)n_seg), dim3(kThreads), 0, (hipStream_t)stream, a);
  return ld_check_launch("ld_jpeg_entropy_i16");
}

LD_API int ld_jpeg_encode_u8(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, const int32_t* tables,
                             const uint8_t* header, int64_t header_bytes, int16_t* coefs_ws, int64_t* seg_ws, uint8_t* out,
                             int64_t out_capacity, int64_t* offsets, int64_t* lengths, int64_t F, int64_t H, int64_t W,
                             int32_t subsampling, int32_t quality, void* stream) {
  const char* who = "ld_jpeg_encode_u8";
  LD_REQUIRE(frames && tables && header && coefs_ws && seg_ws && out && offsets && lengths, "%s: null pointer", who);
  LD_REQUIRE(aligned(tables, 4) && aligned(coefs_ws, 16) && aligned(seg_ws, 8) && aligned(offsets, 8) && aligned(lengths, 8),
             "%s: tables must be 4-byte, coefs_ws 16-byte, seg_ws / offsets / lengths 8-byte aligned", who);
  LD_REQUIRE(quality >= 1 && quality <= 100, "%s: quality must be in 1..100, got %d", who, (int)quality);
  LD_REQUIRE(header_bytes > 0 && header_bytes < (1 << 16), "%s: header_bytes must be in 1..65535, got %lld", who, (long long)header_bytes);
  Geom g;
  if (int rc = check_streams(who, F, H, W, subsampling, header_bytes, out_capacity, &g)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_coefs(who, frames, frame_stride, row_stride, tables, coefs_ws, F, H, W, g, quality, false, s)) return rc;
  launch_tail(stream_args(coefs_ws, tables, seg_ws, out, header, header_bytes, offsets, F, g), offsets, lengths, F, s);
  return ld_check_launch(who);
}
