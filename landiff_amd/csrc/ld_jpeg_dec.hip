// The decode stage (landiff_amd/decode.py): baseline JPEG streams on the device -> uint8 RGB frames, the inverse of
// ld_jpeg.hip.  Integer arithmetic only: no float anywhere in this file.  The rule (libjpeg's "islow" inverse DCT, its triangle
// chroma upsampling and its 16-bit colour constants, which is what PIL decodes with) is restated in numpy in tests/jpeg_dec_ref.py.
// The host parses every header up to SOS (decode.parse_jpeg) and hands over, per frame, where its scan starts and how long it is,
// its restart interval and the index of its table set (decode.decode_tables: quantisers and the Huffman tables of its own DHT).
//
// jpeg_find_segments_kernel: one workgroup per frame walks the scan in chunks of 4 KiB with a running marker count.  Before the
//   end of the entropy-coded data every 0xFF starts a pair (0xFF 0x00 a data byte, 0xFF 0xD0..0xD7 a restart marker); the first
//   0xFF followed by anything else (or by nothing) ends the data.  So a chunk is searched in parallel: the first end (an LDS min),
//   the markers before it (a workgroup scan gives each its number), then marker k closes segment k and opens segment k + 1.
//   Bounds: the scan is clamped into the buffer; a byte i is read only if i < its length; a row k of the table is written only
//   if k < the frame's segment count, which comes from the frame's size and restart interval and is clamped to the table's rows.
// jpeg_decode_entropy_kernel: one lane per segment (Annex F.2.2), 64 lanes a workgroup, the workgroup's frame's Huffman tables in
//   LDS.  A lane keeps a 64-bit bit buffer filled byte by byte; after a 0xFF the next byte (the stuffed 0x00) is skipped.
//   Bounds: the segment (start, length) and its MCUs (first, count) are clamped into the buffer and the frame whatever the table
//   says; a byte is read only at pos < length; a Huffman value is read at an index masked to the table's 256 entries; a
//   coefficient is written at k only after k <= 63 was checked, into a block b < count * blocks per MCU.  Every block of the
//   segment is zeroed by this lane before its values are written, also after an error: no memset is relied on.
// jpeg_idct_kernel: eight lanes per block, 32 blocks per workgroup: a lane dequantises and transforms one column (64-bit: any
//   int16 coefficient times any quantiser fits), the columns' results cross through LDS, the lane transforms one row,
//   saturates it to 0..255 and stores its 8 samples as one 8-byte word into the component's plane (planes are padded to whole MCUs).
// jpeg_colour_kernel: one workgroup per 256 pixels of one output row: chroma upsampling (read clamped to the real chroma size),
//   colour conversion, the 768 bytes staged in LDS and stored as consecutive bytes.  All offsets are 64-bit.
// Nothing depends on the order in which lanes or workgroups finish: two runs give the same bits.
// The geometry, the small helpers and the workgroup scan are ld_jpeg_dev.h's, shared with the encode stage; the table layout and the
// bit reader are ld_jpeg_dec_dev.h's, shared with the second entropy route (ld_jpeg_dec_sync.hip), which also launches
// jpeg_decode_entropy_kernel under a mask for the segments it hands back.
#include "ld_jpeg_dec_dev.h"

using namespace ld_jpeg_dec;

namespace {

constexpr int kThreads = 256;
constexpr int kFindBytes = 16;                               // bytes a thread searches per chunk
constexpr int kChunk = kThreads * kFindBytes;

struct FindArgs {
  const uint8_t* data;
  const int64_t* scan;                             // [F][2]: start, length
  const int32_t* ri;                               // [F]
  int64_t* seg;                                    // [F][S][5]: frame, start, length, first MCU, MCU count
  int64_t* info;                                   // [F][3]: markers found, 1 if numbered 0..7 in order, length of the entropy-coded data
  long data_bytes, S, mcus;
};

__global__ __launch_bounds__(kThreads) void jpeg_find_segments_kernel(FindArgs a) {
  __shared__ int tmp[kThreads];
  __shared__ int first_end;
  const int tid = threadIdx.x;
  const long f = blockIdx.x;
  const long s0 = clampl(a.scan[2 * f], 0, a.data_bytes), n = clampl(a.scan[2 * f + 1], 0, a.data_bytes - s0);
  const uint8_t* p = a.data + s0;                  // p[i] is read only with i < n
  const long ri = max(a.ri[f], 0);
  const long nf = segments_of(a.mcus, ri, a.S);
  int64_t* rows = a.seg + f * a.S * 5;             // rows[k * 5 + ..] is written only with k < nf <= S
  // what follows the 0xFF at i: 0 a stuffed byte, 1 a restart marker, 2 the end of the data
  auto kind = [&](long i, int* m) {
    const int nx = i + 1 < n ? p[i + 1] : 0x100;
    *m = nx - 0xD0;
    return nx == 0 ? 0 : (nx >= 0xD0 && nx <= 0xD7) ? 1 : 2;
  };
  long count = 0, end = n;                         // markers so far, the data's length: the same in every thread
  int order = 1;
  bool ended = false;
  for (long c0 = 0; c0 < n && !ended; c0 += kChunk) {
    if (tid == 0) first_end = kChunk;
    __syncthreads();
    const long lo = min(n, c0 + (long)tid * kFindBytes), hi = min(n, lo + kFindBytes);
    int mine = 0, my_end = kChunk, m;
    for (long i = lo; i < hi; ++i) {
      if (p[i] != 0xFF) continue;
      const int k = kind(i, &m);
      if (k == 2) { my_end = (int)(i - c0); break; }
      mine += k;
    }
    if (my_end < kChunk) atomicMin(&first_end, my_end);
    __syncthreads();
    const int e = first_end;
    if (lo - c0 >= e) mine = 0;                    // markers after the end are no markers (the end's own thread stopped there)
    int total;
    long k = count + block_scan<kThreads>(mine, tmp, &total);
    for (long i = lo; i < hi && mine > 0; ++i) {
      if (p[i] != 0xFF || kind(i, &m) != 1) continue;
      if (m != (int)(k & 7)) order = 0;
      if (k < nf) rows[k * 5 + 2] = i;             // (relative to the scan; made a length below)
      if (k + 1 < nf) rows[(k + 1) * 5 + 1] = i + 2;
      ++k;
      --mine;
    }
    count += total;
    if (e < kChunk) { ended = true; end = c0 + e; }
  }
  order = __syncthreads_and(order);                // (and every row's store is visible to the workgroup)
  for (long s = tid; s < a.S; s += kThreads) {     // a row is read and rewritten by one thread
    long st = 0, len = 0, fm = 0, cnt = 0;
    if (s < nf) {
      fm = ri > 0 ? s * ri : 0;
      cnt = ri > 0 ? min(ri, a.mcus - fm) : a.mcus;
      if (s <= count) {
        const long rel = s ? rows[s * 5 + 1] : 0;
        len = (s < count ? rows[s * 5 + 2] : end) - rel;
        st = s0 + rel;
      }
    }
    rows[s * 5 + 0] = f; rows[s * 5 + 1] = st; rows[s * 5 + 2] = len; rows[s * 5 + 3] = fm; rows[s * 5 + 4] = cnt;
  }
  if (tid == 0) { a.info[3 * f] = count; a.info[3 * f + 1] = order; a.info[3 * f + 2] = end; }
}

struct EntropyArgs {
  const uint8_t* data;
  const int64_t* seg;
  const int64_t* info;
  const int32_t* ri;
  const int32_t* tables;                           // [n_sets][kTabWords]
  const int32_t* tset;                             // [F]
  int16_t* coefs;                                  // [F][frame_blocks][64]
  int32_t* status;                                 // [F][S]
  const int32_t* mask;                             // null, or [F][S]: only segments with a non-zero word are decoded
  long data_bytes, S, mcus, frame_blocks, n_sets;
  int bpm;
};

__global__ __launch_bounds__(64) void jpeg_decode_entropy_kernel(EntropyArgs a) {
  __shared__ int tab[6 * kHuffWords];              // per component: DC table, AC table; each limit[16] | offset[16] | values[256] | look-ahead[256]
  const long f = blockIdx.y;
  {
    const long set = clampl(a.tset[f], 0, a.n_sets - 1);
    const int32_t* src = a.tables + set * kTabWords + kTabHuff;
    for (int i = threadIdx.x; i < 6 * kHuffWords; i += 64) tab[i] = src[i];
  }
  __syncthreads();
  const long s = (long)blockIdx.x * 64 + threadIdx.x;
  if (s >= a.S) return;
  if (a.mask && !a.mask[f * a.S + s]) return;     // (the sync route's fallback: the other segments are left as they are)
  const long nf = segments_of(a.mcus, max(a.ri[f], 0), a.S);
  if (s >= nf) { a.status[f * a.S + s] = LD_JPEG_DEC_OK; return; }
  const int64_t* row = a.seg + (f * a.S + s) * 5;
  const long fm = clampl(row[3], 0, a.mcus), nblk = clampl(row[4], 0, a.mcus - fm) * a.bpm;      // blocks [fm bpm, fm bpm + nblk) of the frame
  const long st = clampl(row[1], 0, a.data_bytes), end = clampl(row[2], 0, a.data_bytes - st);
  const uint8_t* p = a.data + st;                  // p[pos] is read only with pos < end
  int16_t* out = a.coefs + (f * a.frame_blocks + fm * a.bpm) * 64;
  int status = (a.info[3 * f] == nf - 1 && a.info[3 * f + 1] == 1) ? LD_JPEG_DEC_OK : LD_JPEG_DEC_MARKERS;

  BitReader<false> rd;
  rd.open(p, end, 0, 0);
  auto symbol = [&](const int* T) { return rd.symbol(T); };
  auto receive = [&](int n, int* v) { return rd.receive(n, v); };

  int pred0 = 0, pred1 = 0, pred2 = 0;            // the DC predictors: 0 at the segment's start
  for (long b = 0; b < nblk; ++b) {
    int16_t* blk = out + b * 64;
    int4* z = reinterpret_cast<int4*>(blk);
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = make_int4(0, 0, 0, 0);
    if (status) continue;
    const int c = component_of((int)(b % a.bpm), a.bpm);
    const int* dc = tab + 2 * c * kHuffWords;
    const int* ac = dc + kHuffWords;
    int t = symbol(dc), v = 0;
    if (t < 0) { status = -t; continue; }
    if (t > 11) { status = LD_JPEG_DEC_BAD_CODE; continue; }
    if (t && !receive(t, &v)) { status = LD_JPEG_DEC_OVERRUN; continue; }
    const int dcv = (int16_t)((c == 0 ? pred0 : c == 1 ? pred1 : pred2) + v);
    if (c == 0) pred0 = dcv; else if (c == 1) pred1 = dcv; else pred2 = dcv;
    blk[0] = (int16_t)dcv;
    for (int k = 1; k < 64;) {
      const int rs = symbol(ac);
      if (rs < 0) { status = -rs; break; }
      const int r = rs >> 4, n = rs & 15;
      if (n == 0) {
        if (r != 15) break;                        // EOB
        k += 16;
        if (k > 64) status = LD_JPEG_DEC_OVERFLOW;
        continue;
      }
      if (n > 10) { status = LD_JPEG_DEC_BAD_CODE; break; }
      k += r;
      if (k > 63) { status = LD_JPEG_DEC_OVERFLOW; break; }
      if (!receive(n, &v)) { status = LD_JPEG_DEC_OVERRUN; break; }
      blk[k++] = (int16_t)v;
    }
  }
  a.status[f * a.S + s] = status;
}

// natural index 8 v + u -> zigzag position
__device__ const unsigned char kZigPos[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                              41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                              46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// jidctint's pass over eight values: o[i] = (x + (1 << (s - 1))) >> s.  64-bit: DESIGN 8.13 states why that always fits.
__device__ __forceinline__ void idct8(const long* i, long* o, int s) {
  long z1 = (i[2] + i[6]) * 4433;
  const long t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
  const long t0 = (i[0] + i[4]) * 8192, t1 = (i[0] - i[4]) * 8192;
  const long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  long a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
  z1 = a0 + a3;
  long z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const long z5 = (z3 + z4) * 9633;
  a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  const long r = 1L << (s - 1);
  o[0] = (t10 + a3 + r) >> s; o[7] = (t10 - a3 + r) >> s;
  o[1] = (t11 + a2 + r) >> s; o[6] = (t11 - a2 + r) >> s;
  o[2] = (t12 + a1 + r) >> s; o[5] = (t12 - a1 + r) >> s;
  o[3] = (t13 + a0 + r) >> s; o[4] = (t13 - a0 + r) >> s;
}

struct IdctArgs {
  const int16_t* coefs;
  const int32_t* tables;
  const int32_t* tset;
  uint8_t* planes;                                 // [F][3][PH][PW]
  long total_blocks, frame_blocks, n_sets;
  int bpm, mcux, PH, PW;
};

__global__ __launch_bounds__(kThreads) void jpeg_idct_kernel(IdctArgs a) {
  __shared__ long ws[kThreads / 8][64];
  const int tid = threadIdx.x, lb = tid >> 3, c = tid & 7;
  const long gb = (long)blockIdx.x * (kThreads / 8) + lb;
  const bool active = gb < a.total_blocks;
  long in[8], o[8];
  long f = 0;
  int comp = 0, py = 0, px = 0;
  if (active) {
    f = gb / a.frame_blocks;
    const long fb = gb - f * a.frame_blocks;
    const int m = (int)(fb / a.bpm), j = (int)(fb - (long)m * a.bpm);
    const int my = m / a.mcux, mx = m - my * a.mcux;                   // my < mcuy: gb < total_blocks
    if (a.bpm == 3) { comp = j; py = my * 8; px = mx * 8; }
    else if (j < 4) { py = my * 16 + (j >> 1) * 8; px = mx * 16 + (j & 1) * 8; }
    else { comp = j - 3; py = my * 8; px = mx * 8; }
    const int32_t* q = a.tables + clampl(a.tset[f], 0, a.n_sets - 1) * kTabWords + kTabQuant + comp * 64;
    const int16_t* cf = a.coefs + gb * 64;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int z = kZigPos[r * 8 + c];
      in[r] = (long)cf[z] * (long)q[z];
    }
    idct8(in, o, 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[lb][r * 8 + c] = o[r];
  }
  __syncthreads();
  if (active) {
#pragma unroll
    for (int i = 0; i < 8; ++i) in[i] = ws[lb][c * 8 + i];
    idct8(in, o, 18);
    unsigned long long w = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {                  // saturated: libjpeg's range-limit table wherever that table is no wrap
      const long x = o[i] + 128;
      w |= (unsigned long long)(x < 0 ? 0 : x > 255 ? 255 : x) << (8 * i);
    }
    // py + c < PH and px + 8 <= PW (whole MCUs), PW a multiple of 8 and the planes 8-byte aligned: one aligned 8-byte store
    uint8_t* dst = a.planes + ((f * 3 + comp) * a.PH + py + c) * a.PW + px;
    *reinterpret_cast<unsigned long long*>(dst) = w;
  }
}

struct ColourArgs {
  const uint8_t* planes;
  uint8_t* out;
  long frame_stride, row_stride;
  int H, W, tiles, PH, PW, sub420;
};

__global__ __launch_bounds__(kThreads) void jpeg_colour_kernel(ColourArgs a) {
  __shared__ uint8_t line[kThreads * 3];
  const int tid = threadIdx.x;
  const long g = blockIdx.x;
  const int tile = (int)(g % a.tiles);
  const int y = (int)((g / a.tiles) % a.H);
  const long f = g / ((long)a.tiles * a.H);
  const int x = tile * kThreads + tid;
  const uint8_t* Y = a.planes + f * 3 * a.PH * a.PW;
  if (x < a.W) {
    const int yy = Y[(long)y * a.PW + x];
    int cc[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint8_t* C = Y + (long)(k + 1) * a.PH * a.PW;
      if (!a.sub420) { cc[k] = C[(long)y * a.PW + x]; continue; }
      const int h = (a.H + 1) >> 1, w = (a.W + 1) >> 1;                // the real chroma size: nothing beyond it is read
      const int r = y >> 1, j = x >> 1;
      if (w <= 2) { cc[k] = C[(long)r * a.PW + j]; continue; }
      const int nb = min(max((y & 1) ? r + 1 : r - 1, 0), h - 1);
      const uint8_t* c0 = C + (long)r * a.PW;
      const uint8_t* c1 = C + (long)nb * a.PW;
      const int jn = (x & 1) ? min(j + 1, w - 1) : max(j - 1, 0);
      const int sj = 3 * c0[j] + c1[j], sn = 3 * c0[jn] + c1[jn];
      cc[k] = (3 * sj + sn + ((x & 1) ? 7 : 8)) >> 4;
    }
    const int cb = cc[0] - 128, cr = cc[1] - 128;
    line[3 * tid + 0] = (uint8_t)clamp255(yy + ((91881 * cr + 32768) >> 16));
    line[3 * tid + 1] = (uint8_t)clamp255(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    line[3 * tid + 2] = (uint8_t)clamp255(yy + ((116130 * cb + 32768) >> 16));
  }
  __syncthreads();
  const int nbytes = 3 * min(kThreads, a.W - tile * kThreads);        // this tile's share of the row: within 3 W
  uint8_t* dst = a.out + f * a.frame_stride + (long)y * a.row_stride + 3L * tile * kThreads;
  for (int i = tid; i < nbytes; i += kThreads) dst[i] = line[i];
}

}  // namespace

void ld_jpeg_dec::launch_entropy_segments(const uint8_t* data, long data_bytes, const int64_t* seg_table, const int64_t* frame_info,
                                          const int32_t* ri, const int32_t* tables, const int32_t* tset, long n_sets, int16_t* coefs,
                                          int32_t* status, const int32_t* mask, long F, long S, const Geom& g, hipStream_t stream) {
  EntropyArgs a{data, seg_table, frame_info, ri, tables, tset, coefs, status, mask, data_bytes, S, g.mcus, g.frame_blocks, n_sets, g.bpm};
  hipLaunchKernelGGL(jpeg_decode_entropy_kernel, dim3((unsigned)((S + 63) / 64), (unsigned)F), dim3(64), 0, stream, a);
}

LD_API int64_t ld_jpeg_dec_size(int32_t what, int64_t H, int64_t W, int32_t subsampling) {
  Geom g;
  if (int rc = geometry("ld_jpeg_dec_size", H, W, subsampling, &g)) return rc;
  switch (what) {
    case LD_JPEG_DEC_SIZE_FRAME_BLOCKS: return g.frame_blocks;
    case LD_JPEG_DEC_SIZE_MCUS: return g.mcus;
    case LD_JPEG_DEC_SIZE_PLANE_BYTES: return 3L * g.PH * g.PW;
    case LD_JPEG_DEC_SIZE_TABLE_WORDS: return kTabWords;
    default: return ld_set_error(LD_ERR_INVALID, "ld_jpeg_dec_size: unknown quantity %d", (int)what);
  }
}

LD_API int ld_jpeg_find_segments(const uint8_t* data, int64_t data_bytes, const int64_t* scan, const int32_t* ri, int64_t* seg_table,
                                 int64_t* frame_info, int64_t F, int64_t S, int64_t H, int64_t W, int32_t subsampling, void* stream) {
  LD_REQUIRE(data && scan && ri && seg_table && frame_info, "ld_jpeg_find_segments: null pointer");
  LD_REQUIRE(aligned(scan, 8) && aligned(ri, 4) && aligned(seg_table, 8) && aligned(frame_info, 8),
             "ld_jpeg_find_segments: scan, seg_table and frame_info must be 8-byte and ri 4-byte aligned");
  LD_REQUIRE(data_bytes > 0 && S > 0, "ld_jpeg_find_segments: data_bytes and S must be positive, got %lld and %lld",
             (long long)data_bytes, (long long)S);
  if (int rc = check_frames("ld_jpeg_find_segments", F)) return rc;
  Geom g;
  if (int rc = geometry("ld_jpeg_find_segments", H, W, subsampling, &g)) return rc;
  FindArgs a{data, scan, ri, seg_table, frame_info, (long)data_bytes, (long)S, g.mcus};
  hipLaunchKernelGGL(jpeg_find_segments_kernel, dim3((unsigned)F), dim3(kThreads), 0, (hipStream_t)stream, a);
  return ld_check_launch("ld_jpeg_find_segments");
}

LD_API int ld_jpeg_decode_entropy(const uint8_t* data, int64_t data_bytes, const int64_t* seg_table, const int64_t* frame_info,
                                  const int32_t* ri, const int32_t* tables, const int32_t* tset, int64_t n_sets, int16_t* coefs,
                                  int32_t* status, int64_t F, int64_t S, int64_t H, int64_t W, int32_t subsampling, void* stream) {
  LD_REQUIRE(data && seg_table && frame_info && ri && tables && tset && coefs && status, "ld_jpeg_decode_entropy: null pointer");
  LD_REQUIRE(aligned(seg_table, 8) && aligned(frame_info, 8) && aligned(ri, 4) && aligned(tables, 4) && aligned(tset, 4) &&
                 aligned(coefs, 16) && aligned(status, 4),
             "ld_jpeg_decode_entropy: seg_table and frame_info must be 8-byte, ri, tables, tset and status 4-byte and coefs 16-byte aligned");
  LD_REQUIRE(data_bytes > 0 && S > 0 && n_sets > 0, "ld_jpeg_decode_entropy: data_bytes, S and n_sets must be positive");
  if (int rc = check_frames("ld_jpeg_decode_entropy", F)) return rc;
  Geom g;
  if (int rc = geometry("ld_jpeg_decode_entropy", H, W, subsampling, &g)) return rc;
  LD_REQUIRE((S + 63) / 64 < (1L << 31), "ld_jpeg_decode_entropy: %lld segments a frame exceed one launch", (long long)S);
  launch_entropy_segments(data, (long)data_bytes, seg_table, frame_info, ri, tables, tset, (long)n_sets, coefs, status, nullptr, (long)F,
                          (long)S, g, (hipStream_t)stream);
  return ld_check_launch("ld_jpeg_decode_entropy");
}

LD_API int ld_jpeg_decode_rgb(const int16_t* coefs, const int32_t* tables, const int32_t* tset, int64_t n_sets, uint8_t* planes_ws,
                              uint8_t* out, int64_t frame_stride, int64_t row_stride, int64_t F, int64_t H, int64_t W,
                              int32_t subsampling, void* stream) {
  LD_REQUIRE(coefs && tables && tset && planes_ws && out, "ld_jpeg_decode_rgb: null pointer");
  LD_REQUIRE(aligned(coefs, 16) && aligned(tables, 4) && aligned(tset, 4) && aligned(planes_ws, 8),
             "ld_jpeg_decode_rgb: coefs must be 16-byte, planes_ws 8-byte, tables and tset 4-byte aligned");
  LD_REQUIRE(n_sets > 0, "ld_jpeg_decode_rgb: n_sets must be positive");
  if (int rc = check_frames("ld_jpeg_decode_rgb", F)) return rc;
  Geom g;
  if (int rc = geometry("ld_jpeg_decode_rgb", H, W, subsampling, &g)) return rc;
  LD_REQUIRE(row_stride >= 3 * W && frame_stride >= (H - 1) * row_stride + 3 * W,
             "ld_jpeg_decode_rgb: row_stride %lld / frame_stride %lld do not hold %lld x %lld RGB pixels", (long long)row_stride,
             (long long)frame_stride, (long long)H, (long long)W);
  const long total = (long)F * g.frame_blocks, per = kThreads / 8;
  const int tiles = (int)((W + kThreads - 1) / kThreads);
  const long groups = (long)F * H * tiles;
  LD_REQUIRE((total + per - 1) / per < (1L << 31) && groups < (1L << 31), "ld_jpeg_decode_rgb: %ld blocks / %ld row tiles exceed one launch",
             total, groups);
  hipStream_t s = (hipStream_t)stream;
  IdctArgs ia{coefs, tables, tset, planes_ws, total, g.frame_blocks, (long)n_sets, g.bpm, g.mcux, g.PH, g.PW};
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((total + per - 1) / per)), dim3(kThreads), 0, s, ia);
  ColourArgs ca{planes_ws, out, (long)frame_stride, (long)row_stride, (int)H, (int)W, tiles, g.PH, g.PW, subsampling == 420};
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)groups), dim3(kThreads), 0, s, ca);
  return ld_check_launch("ld_jpeg_decode_rgb");
}
