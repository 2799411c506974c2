// What the two entropy routes of the decode stage share (ld_jpeg_dec.hip: one lane per restart segment; ld_jpeg_dec_sync.hip: one
// lane per subsequence of a segment) beyond ld_jpeg_dev.h: the layout of a table set, the bit reader with its Huffman
// symbol and its EXTENDed value, and the launch of the lane-per-segment kernel under an optional mask.  Integer arithmetic only.
#pragma once
#include "ld_jpeg_dev.h"

namespace ld_jpeg_dec {

using ld_jpeg::Geom, ld_jpeg::geometry, ld_jpeg::aligned, ld_jpeg::clamp255, ld_jpeg::clampl, ld_jpeg::component_of, ld_jpeg::block_scan;

// offsets into one table set (int32 words; LD_JPEG_DEC_TABLE_WORDS in all)
constexpr int kTabQuant = 0, kTabHuff = 192, kHuffWords = 544, kTabWords = LD_JPEG_DEC_TABLE_WORDS;
constexpr int kHuffLimit = 0, kHuffOff = 16, kHuffVals = 32, kHuffLook = 288;      // within one Huffman table
static_assert(kTabHuff + 6 * kHuffWords == kTabWords, "table layout");

inline int check_frames(const char* who, int64_t F) {
  LD_REQUIRE(F > 0 && F < (1 << 16), "%s: 1 .. 65535 frames a call, got %lld", who, (long long)F);
  return LD_OK;
}

// the segments of a frame of `mcus` MCUs at restart interval ri, never more than the table's S rows
__device__ __forceinline__ long segments_of(long mcus, long ri, long S) { return min(ri > 0 ? (mcus + ri - 1) / ri : 1L, S); }

// The next bits of one segment, p[0 .. end): a 64-bit buffer filled byte by byte from bit 63 down, zeros past the segment's end;
// after a 0xFF the next byte (the stuffed 0x00) is skipped.  p[pos] is read only with pos < end.
// kTrack: `over` counts the buffered bits that come from bytes at or after `mark` (the sync route's end of a subsequence).
template <bool kTrack>
struct BitReader {
  const uint8_t* p;
  long end, pos, mark;
  unsigned long long buf;
  int nbits, over;

  __device__ __forceinline__ void open(const uint8_t* p_, long end_, long pos_, long mark_) {
    p = p_; end = end_; pos = pos_; mark = mark_;
    buf = 0; nbits = 0; over = 0;
  }
  __device__ __forceinline__ void fill() {
    while (nbits <= 56 && pos < end) {
      const unsigned long long b = p[pos];
      if (kTrack && pos >= mark) over += 8;
      pos += b == 0xFF ? 2 : 1;                    // the stuffed 0x00
      buf |= b << (56 - nbits);
      nbits += 8;
    }
  }
  __device__ __forceinline__ void drop(int n) {    // n <= nbits
    buf <<= n;
    nbits -= n;
  }
  // one Huffman symbol (>= 0) or minus a status: OVERRUN where the code would need bits past the end, BAD_CODE where sixteen
  // bits that are there start no code
  __device__ __forceinline__ int symbol(const int* T) {
    fill();
    const uint32_t c16 = (uint32_t)(buf >> 48);
    const int e = T[kHuffLook + (c16 >> 8)];
    int l = e >> 8, v = e & 255;
    if (!e) {                                      // no code of 8 bits or fewer
      l = 9;
      while (l <= 16 && c16 >= (uint32_t)T[kHuffLimit + l - 1]) ++l;
      if (l > 16) return nbits < 16 ? -LD_JPEG_DEC_OVERRUN : -LD_JPEG_DEC_BAD_CODE;
      v = T[kHuffVals + ((T[kHuffOff + l - 1] + (int)(c16 >> (16 - l))) & 255)] & 255;
    }
    if (l > nbits) return -LD_JPEG_DEC_OVERRUN;
    drop(l);
    return v;
  }
  // n in 1..15 bits, EXTENDed (F.2.2.1); false: past the segment's end (nothing is consumed)
  __device__ __forceinline__ bool receive(int n, int* v) {
    fill();
    if (n > nbits) return false;
    const int r = (int)(buf >> (64 - n));
    drop(n);
    *v = r < (1 << (n - 1)) ? r - (1 << n) + 1 : r;
    return true;
  }
};

// The lane-per-segment kernel of ld_jpeg_decode_entropy (ld_jpeg_dec.hip), arguments already checked.  mask: null, or int32 [F][S]:
// only the segments with a non-zero word are decoded, nothing of another segment (coefficients, status) is touched.
void launch_entropy_segments(const uint8_t* data, long data_bytes, const int64_t* seg_table, const int64_t* frame_info,
                             const int32_t* ri, const int32_t* tables, const int32_t* tset, long n_sets, int16_t* coefs,
                             int32_t* status, const int32_t* mask, long F, long S, const Geom& g, hipStream_t stream);

}  // namespace ld_jpeg_dec
