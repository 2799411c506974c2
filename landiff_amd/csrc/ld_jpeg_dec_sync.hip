// The decode stage's second entropy route (restated in tests/jpeg_sync_ref.py): a restart segment of any length is
// decoded by one lane per subsequence of B = sub_bytes raw bytes, so that a stream without restart markers (PIL, ffmpeg, cameras)
// is no longer one lane per frame.  Integer arithmetic only: no float anywhere in this file.  All offsets are 64-bit.
//
// A lane's state is (p, j, k): p = 8 x (raw byte within the segment) + bit, always a bit of a data byte or 8 len (a 0x00 after a
// 0xFF is stuffed and belongs to nobody); j the block within the MCU; k the next zigzag index, 0 = a DC is due.  exit(i, entry)
// decodes codewords (one Huffman symbol with its extra bits) from `entry` while p < 8 min((i + 1) B, len) and returns the state
// reached and the blocks completed.  Rounds (Jacobi, two buffers: nothing depends on scheduling): E0[i] = exit(i, start of
// subsequence i), Er[i] = exit(i, Er-1[i - 1]), Er[0] = E0[0]; by induction Er[0..r] are the serial decoder's states.
//
// The launches, in order (their number is fixed by max_rounds; no kernel waits for a flag):
//   jpeg_sync_count_kernel   one workgroup per frame: the subsequences of every segment and where they start within the frame
//   jpeg_sync_frames_kernel  one workgroup: where every frame's subsequences start in the flat list (frames padded to whole
//                            workgroups, so that a workgroup holds one frame's Huffman tables in LDS)
//   jpeg_sync_round_kernel   round 0, then max_rounds rounds; a segment whose last round changed nothing exits at once, and a
//                            workgroup of a frame with no such change before it loads the tables
//   jpeg_sync_prefix_kernel  one workgroup per segment: exclusive scan of the block counts = every subsequence's first block
//   (the coefficients are zeroed by a memset)
//   jpeg_sync_write_kernel   decode again from E[i - 1], now storing; the DC *difference* goes to blk[0]; every lane checks its
//                            exit against E[i]: a mismatch marks the segment not converged
//   jpeg_sync_finish_kernel  status (that of the lowest subsequence that reported one), sync_info, the fallback mask
//   jpeg_sync_dc_kernel      one workgroup per segment: inclusive scan modulo 2^16 of the differences per component
//   jpeg_decode_entropy_kernel (ld_jpeg_dec.hip) under the mask: segments not converged, or with an error, are decoded serially
// Bounds: a segment (start, length) and its MCUs are clamped into the buffer and the frame as the serial kernel clamps them; a byte
// is read only at pos < length (BitReader) or at an index checked against it; a coefficient is stored at k <= 63 of a block
// b < the segment's block count; a flat index t is used only below the list's capacity T, which the host sized the workspace by.
// A lane's loop is bounded by construction: every iteration consumes at least one bit of at most 8 B + 27, and is capped besides.
#include "ld_jpeg_dec_dev.h"

#include <limits.h>

using namespace ld_jpeg_dec;

namespace {

constexpr int kLanes = 64;                         // a workgroup of the lane kernels: one wave, one frame
constexpr int kThreads = 256;                      // the scans
constexpr int kMaxRounds = 4096;
constexpr int kNoError = INT_MAX;

struct State {
  long p;
  int j, k, n;                                     // n: blocks completed
};
// E as stored: 16 bytes a subsequence
__device__ __forceinline__ int4 pack(const State& s) {
  return make_int4((int)(s.p & 0xffffffffL), (int)(s.p >> 32), s.j | s.k << 8, s.n);
}
__device__ __forceinline__ State unpack(const int4& v) {
  State s;
  s.p = (long)(unsigned)v.x | (long)v.y << 32;
  s.j = v.z & 255;
  s.k = v.z >> 8;
  s.n = v.w;
  return s;
}
__device__ __forceinline__ bool same(const int4& a, const int4& b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// The workspace, carved by the host from the bounds it knows (ld_jpeg_dec_sync_size): NS = F S segments, T flat subsequences.
struct Work {
  int32_t* seg_rel;                                // [NS] where the segment's subsequences start within its frame's
  int32_t* seg_cnt;                                // [NS] its subsequences (0: a row the frame does not use, or a frame refused)
  int32_t* frame_total;                            // [F]
  int32_t* frame_base;                             // [F + 1] where the frame's subsequences start in the flat list; multiples of 64
  int32_t* frame_short;                            // [F] 1: the list's capacity did not hold the frame (its segments fall back)
  int32_t* sub_seg;                                // [T] the segment of flat subsequence t, -1 none
  int32_t* first_block;                            // [T] the block of the segment at which subsequence t starts
  int4* E;                                         // [2][T]
  int32_t* changed;                                // [max_rounds + 1][NS]: round r changed an exit of the segment
  int32_t* frame_changed;                          // [max_rounds + 1][F] (right behind `changed`: one memset): ... of the frame
  int32_t* err;                                    // [NS] min over the subsequences of (index << 3 | status), kNoError: none
  int32_t* bad;                                    // [NS] 1: the write pass disagreed with E
  int32_t* mask;                                   // [NS] 1: the segment falls back
  long T;
};

struct SyncArgs {
  const uint8_t* data;
  const int64_t* seg;
  const int64_t* info;
  const int32_t* ri;
  const int32_t* tables;
  const int32_t* tset;
  int16_t* coefs;
  int32_t* status;
  int32_t* sync_info;                              // [F][S][2]
  int64_t* exits;                                  // null, or [T][4]
  int32_t* exits_index;                            // null, or [F][S][2]: first row of `exits`, rows
  Work w;
  long data_bytes, S, F, mcus, frame_blocks, n_sets;
  int bpm, B, max_rounds, round;
};

// The clamped view of one segment, as the serial kernel takes it.
struct Segment {
  const uint8_t* p;
  long len, fm, nblk;
};
__device__ __forceinline__ Segment segment_of(const SyncArgs& a, long g) {
  const int64_t* row = a.seg + g * 5;
  Segment s;
  s.fm = clampl(row[3], 0, a.mcus);
  s.nblk = clampl(row[4], 0, a.mcus - s.fm) * a.bpm;
  const long st = clampl(row[1], 0, a.data_bytes);
  s.len = clampl(row[2], 0, a.data_bytes - st);
  s.p = a.data + st;
  return s;
}
__device__ __forceinline__ bool markers_ok(const SyncArgs& a, long f, long nf) { return a.info[3 * f] == nf - 1 && a.info[3 * f + 1] == 1; }

__global__ __launch_bounds__(kThreads) void jpeg_sync_count_kernel(SyncArgs a) {
  __shared__ long tmp[kThreads];
  const long f = blockIdx.x;
  const long nf = segments_of(a.mcus, max(a.ri[f], 0), a.S);
  const bool ok = markers_ok(a, f, nf);
  long run = 0;                                    // (long: a table whose segments overlap may claim more than the list holds)
  for (long s0 = 0; s0 < a.S; s0 += kThreads) {
    const long s = s0 + threadIdx.x;
    long n = 0;
    if (s < nf && ok) n = max(1L, (segment_of(a, f * a.S + s).len + a.B - 1) / a.B);
    long total;
    const long at = run + block_scan<kThreads>(n, tmp, &total);
    if (s < a.S) {
      const long g = f * a.S + s;
      const bool fits = at + n <= a.w.T;           // otherwise the frame does not fit either: frame_short
      a.w.seg_rel[g] = fits ? (int)at : 0;
      a.w.seg_cnt[g] = fits ? (int)n : 0;
      a.w.err[g] = kNoError;
      a.w.bad[g] = 0;
    }
    run += total;
  }
  if (threadIdx.x == 0) a.w.frame_total[f] = (int)min(run, (long)INT_MAX);
}

__global__ __launch_bounds__(kThreads) void jpeg_sync_frames_kernel(SyncArgs a) {
  __shared__ long tmp[kThreads];
  long run = 0;                                    // (long: the sum is checked against T before it is stored as an int)
  for (long f0 = 0; f0 < a.F; f0 += kThreads) {
    const long f = f0 + threadIdx.x;
    const long n = f < a.F ? ((long)a.w.frame_total[f] + kLanes - 1) / kLanes : 0;      // in workgroups
    long total;
    const long at = run + block_scan<kThreads>(n, tmp, &total);
    if (f < a.F) {
      const bool fits = (at + n) * kLanes <= a.w.T;
      a.w.frame_short[f] = !fits;
      a.w.frame_base[f] = (int)(min(at * kLanes, a.w.T));
      if (!fits) a.w.frame_total[f] = 0;
    }
    run += total;
  }
  if (threadIdx.x == 0) a.w.frame_base[a.F] = (int)min(run * kLanes, a.w.T);
}

// The walk of one lane: exit(i, entry), and with kWrite the write pass.
struct Walk {
  State out;
  bool capped;                                     // the iteration cap ended the loop (unreachable by the bound; the lane then counts as wrong)
  int status;                                      // kWrite: the error met (the lane stopped there), 0 none
  bool whole;                                      // the lane decoded up to its subsequence's end
};

template <bool kWrite>
__device__ __forceinline__ Walk walk(const Segment& sg, const int* tab, int bpm, int B, long i, State e, int16_t* blocks, long b) {
  Walk r;
  r.status = 0;
  r.whole = true;
  r.capped = false;
  e.n = 0;
  r.out = e;
  const long limit = min((i + 1) * (long)B, sg.len);
  if (e.p >= 8 * limit) return r;                  // nothing of this subsequence is left to the lane
  BitReader<true> rd;
  rd.open(sg.p, sg.len, e.p >> 3, limit);
  rd.fill();
  rd.drop((int)(e.p & 7));                         // p names a bit of a data byte below len: the fill loaded that byte
  int j = min(max(e.j, 0), bpm - 1), k = min(max(e.k, 0), 63), n = 0;      // (what the rounds stored is in range; nothing is assumed)
  bool at_end = false;
  // every iteration consumes at least one bit, and there are at most 8 B + 27 from the entry to where the loop stops
  for (int it = 0; !(rd.pos >= limit && rd.nbits <= rd.over); ++it) {
    if (it >= 8 * B + 32) { r.capped = true; break; }
    if (kWrite && b + n >= sg.nblk) { r.whole = false; break; }
    const BitReader<true> saved = rd;
    const int* dc = tab + 2 * component_of(j, bpm) * kHuffWords;
    const int sym = rd.symbol(k == 0 ? dc : dc + kHuffWords);
    if (sym == -LD_JPEG_DEC_OVERRUN) { at_end = true; break; }
    int v = 0, size = k == 0 ? sym : sym & 15;
    if (sym < 0 || size > (k == 0 ? 11 : 10)) {    // no code, or a size no baseline stream has: one bit on
      if (kWrite) { r.status = LD_JPEG_DEC_BAD_CODE; r.whole = false; break; }
      rd = saved;
      rd.fill();
      rd.drop(1);
      continue;
    }
    bool done = false;                             // the block ends here
    if (k == 0) {
      if (size && !rd.receive(size, &v)) { at_end = true; break; }
      if (kWrite) blocks[(b + n) * 64] = (int16_t)v;
      k = 1;
    } else if (size == 0) {
      if (sym >> 4 != 15) done = true;             // EOB
      else {
        k += 16;
        if (k > 64) {
          if (kWrite) { r.status = LD_JPEG_DEC_OVERFLOW; r.whole = false; break; }
          done = true;
        }
      }
    } else {
      const int run = sym >> 4;
      if (k + run > 63) {                          // a run past 63: the block's end, the symbol is consumed
        if (kWrite) { r.status = LD_JPEG_DEC_OVERFLOW; r.whole = false; break; }
        done = true;
      } else {
        if (!rd.receive(size, &v)) { at_end = true; break; }
        k += run;
        if (kWrite) blocks[(b + n) * 64 + k] = (int16_t)v;       // k <= 63 and b + n < nblk were checked
        ++k;
      }
    }
    if (done || k >= 64) {
      j = j + 1 == bpm ? 0 : j + 1;
      k = 0;
      ++n;
    }
  }
  r.out.j = j;
  r.out.k = k;
  r.out.n = n;
  if (r.capped) {                                  // well-defined whatever happened: the lane stops at the segment's end, not whole
    r.out.p = 8 * sg.len;
    r.whole = false;
    return r;
  }
  if (at_end) {                                    // a codeword that needs bits past the segment's end: j, k as before it
    r.out.p = 8 * sg.len;
    if (kWrite) { r.status = LD_JPEG_DEC_OVERRUN; r.whole = false; }
    return r;
  }
  if (!r.whole) return r;
  // the position: (over - nbits) data bits past the first data byte at or after the limit
  long q = limit;
  if (q < sg.len && q > 0 && sg.p[q - 1] == 0xFF) ++q;
  int d = rd.over - rd.nbits;
  for (; d >= 8 && q < sg.len; d -= 8) {
    ++q;
    if (q < sg.len && sg.p[q - 1] == 0xFF) ++q;
  }
  r.out.p = q >= sg.len ? 8 * sg.len : 8 * q + d;
  return r;
}

// What every lane kernel does first: the frame's tables into LDS, then the lane's segment and subsequence.  false: no work.
struct Lane {
  long g, i;                                       // segment (f S + s), subsequence within it
  int n;                                           // the segment's subsequences
};
__device__ __forceinline__ bool lane_of(const SyncArgs& a, long t, int seg, Lane* l) {
  if (seg < 0) return false;
  const long f = seg / a.S;
  l->g = seg;
  l->i = t - a.w.frame_base[f] - a.w.seg_rel[seg];
  l->n = a.w.seg_cnt[seg];
  return l->i >= 0 && l->i < l->n;
}
// the frame a workgroup of kLanes flat subsequences belongs to (frames start at multiples of kLanes), -1: past the last
__device__ __forceinline__ long frame_of(const SyncArgs& a, long t) {
  if (t >= a.w.frame_base[a.F]) return -1;
  long lo = 0, hi = a.F - 1;                       // the last frame whose base is <= t
  while (lo < hi) {
    const long mid = (lo + hi + 1) >> 1;
    if (a.w.frame_base[mid] <= t) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ void load_tables(const SyncArgs& a, long f, int* tab) {
  const long set = clampl(a.tset[f], 0, a.n_sets - 1);
  const int32_t* src = a.tables + set * kTabWords + kTabHuff;
  for (int i = threadIdx.x; i < 6 * kHuffWords; i += kLanes) tab[i] = src[i];
  __syncthreads();
}
// the state at which subsequence i starts when nothing is known: its first data bit, a DC of block 0 due
__device__ __forceinline__ State cold_start(const Segment& sg, long i, int B) {
  State e;
  long q = i * (long)B;
  if (q > 0 && q < sg.len && sg.p[q - 1] == 0xFF) ++q;           // a stuffed byte at the boundary belongs to nobody
  e.p = 8 * min(q, sg.len);
  e.j = e.k = e.n = 0;
  return e;
}

// round 0 (a.round == 0): also finds every flat subsequence's segment; rounds 1..: Er[i] = exit(i, Er-1[i - 1])
__global__ __launch_bounds__(kLanes) void jpeg_sync_round_kernel(SyncArgs a) {
  __shared__ int tab[6 * kHuffWords];
  const long t0 = (long)blockIdx.x * kLanes, t = t0 + threadIdx.x;             // t < T: the grid is T / kLanes
  const long f = frame_of(a, t0);                  // the same for the whole workgroup
  if (f < 0) {
    if (a.round == 0) a.w.sub_seg[t] = -1;
    return;
  }
  // a frame none of whose segments changed last round: the whole workgroup exits at once, before the tables are loaded
  if (a.round > 1 && !a.w.frame_changed[(long)(a.round - 1) * a.F + f]) return;
  load_tables(a, f, tab);
  int seg;
  if (a.round == 0) {
    const long rel = t - a.w.frame_base[f];
    seg = -1;
    if (rel < a.w.frame_total[f]) {                // the last segment of the frame whose first subsequence is <= rel
      long lo = 0, hi = a.S - 1;
      while (lo < hi) {
        const long mid = (lo + hi + 1) >> 1;
        if (a.w.seg_rel[f * a.S + mid] <= rel) lo = mid; else hi = mid - 1;
      }
      seg = (int)(f * a.S + lo);
    }
    a.w.sub_seg[t] = seg;
  } else {
    seg = a.w.sub_seg[t];
  }
  Lane l;
  if (!lane_of(a, t, seg, &l)) return;
  const Segment sg = segment_of(a, l.g);
  const long NS = a.F * a.S;
  if (a.round == 0) {
    a.w.E[t] = pack(walk<false>(sg, tab, a.bpm, a.B, l.i, cold_start(sg, l.i, a.B), nullptr, 0).out);
    return;
  }
  if (a.round > 1 && !a.w.changed[(long)(a.round - 1) * NS + l.g]) return;     // stable: both buffers hold the fixed point
  const int4* prev = a.w.E + (long)((a.round - 1) & 1) * a.w.T;
  int4* next = a.w.E + (long)(a.round & 1) * a.w.T;
  const int4 old = prev[t];
  int4 now = old;
  if (l.i > 0) now = pack(walk<false>(sg, tab, a.bpm, a.B, l.i, unpack(prev[t - 1]), nullptr, 0).out);
  next[t] = now;
  if (!same(now, old)) {                           // (every lane that stores, stores the same 1)
    a.w.changed[(long)a.round * NS + l.g] = 1;
    a.w.frame_changed[(long)a.round * a.F + f] = 1;
  }
}

__global__ __launch_bounds__(kThreads) void jpeg_sync_prefix_kernel(SyncArgs a) {
  __shared__ int tmp[kThreads];
  const long g = (long)blockIdx.y * a.S + blockIdx.x;
  const int n = a.w.seg_cnt[g];                    // the same in every thread
  if (n == 0 || a.w.frame_short[blockIdx.y]) return;
  const long base = (long)a.w.frame_base[blockIdx.y] + a.w.seg_rel[g];         // base + n <= T (jpeg_sync_frames_kernel)
  const int4* E = a.w.E + (long)(a.max_rounds & 1) * a.w.T;
  int run = 0;
  for (int i0 = 0; i0 < n; i0 += kThreads) {
    const int i = i0 + threadIdx.x;
    // counts are at most 8 B + 27 each; a sum that wraps (a segment of more than 2^31 blocks' worth of exits) only makes the
    // write pass disagree or stop at the segment's block count: every store stays bounded by that count
    const int c = i < n ? E[base + i].w : 0;
    int total;
    const int at = run + block_scan<kThreads>(c, tmp, &total);
    if (i < n) a.w.first_block[base + i] = at;
    run += total;
  }
}

__global__ __launch_bounds__(kLanes) void jpeg_sync_write_kernel(SyncArgs a) {
  __shared__ int tab[6 * kHuffWords];
  const long t0 = (long)blockIdx.x * kLanes, t = t0 + threadIdx.x;
  const long f = frame_of(a, t0);
  if (f < 0) return;
  load_tables(a, f, tab);
  Lane l;
  if (!lane_of(a, t, a.w.sub_seg[t], &l)) return;
  const Segment sg = segment_of(a, l.g);
  const int4* E = a.w.E + (long)(a.max_rounds & 1) * a.w.T;
  const int4 mine = E[t];
  if (a.exits) {
    const State s = unpack(mine);
    int64_t* row = a.exits + t * 4;
    row[0] = s.p; row[1] = s.j; row[2] = s.k; row[3] = s.n;
  }
  State e;
  e.p = 0;
  e.j = e.k = e.n = 0;
  if (l.i > 0) e = unpack(E[t - 1]);
  e.j = min(max(e.j, 0), a.bpm - 1);               // (what the rounds stored is in range; nothing is assumed of it)
  e.k = min(max(e.k, 0), 63);
  e.p = clampl(e.p, 0, 8 * sg.len);
  const long b = max(a.w.first_block[t], 0);
  int16_t* blocks = a.coefs + (f * a.frame_blocks + sg.fm * a.bpm) * 64;       // blocks [0, nblk) of the segment
  const Walk w = walk<true>(sg, tab, a.bpm, a.B, l.i, e, blocks, b);
  int status = w.status;
  bool bad = false;
  if (w.whole) {
    bad = !same(pack(w.out), mine);
    if (l.i == l.n - 1 && b + w.out.n < sg.nblk) status = LD_JPEG_DEC_OVERRUN;   // the bits ran out while blocks are owed
  } else if (!status) {
    bad = b + unpack(mine).n < sg.nblk;            // the lane stopped at the block count: every later lane must start there too
  }
  if (bad || w.capped) a.w.bad[l.g] = 1;
  if (status) atomicMin(&a.w.err[l.g], (int)(min(l.i, (long)(INT_MAX >> 3) - 1) << 3 | status));
}

__global__ __launch_bounds__(kThreads) void jpeg_sync_finish_kernel(SyncArgs a) {
  const long NS = a.F * a.S;
  const long g = (long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= NS) return;
  const long f = g / a.S, s = g - f * a.S;
  const long nf = segments_of(a.mcus, max(a.ri[f], 0), a.S);
  int status = LD_JPEG_DEC_OK, rounds = 0, fell = 0;
  if (s < nf) {
    if (!markers_ok(a, f, nf)) status = LD_JPEG_DEC_MARKERS;        // nothing of the frame is decoded: its blocks stay zero
    else {
      const int e = a.w.err[g];
      if (e != kNoError) status = e & 7;
      fell = a.w.frame_short[f] || a.w.bad[g] || status != LD_JPEG_DEC_OK;     // after an error the serial kernel's zeros are owed
      while (rounds < a.max_rounds && a.w.changed[(long)(rounds + 1) * NS + g]) ++rounds;
    }
  }
  a.status[g] = status;
  a.w.mask[g] = fell;
  a.sync_info[2 * g] = rounds;
  a.sync_info[2 * g + 1] = fell;
  if (a.exits_index) {
    a.exits_index[2 * g] = a.w.frame_base[f] + a.w.seg_rel[g];
    a.exits_index[2 * g + 1] = a.w.seg_cnt[g];
  }
}

// differences -> DC values: per component an inclusive scan modulo 2^16, equal to the serial (int16)(pred + v) chain
__global__ __launch_bounds__(kThreads) void jpeg_sync_dc_kernel(SyncArgs a) {
  __shared__ int tmp[kThreads];
  const long f = blockIdx.y, g = f * a.S + blockIdx.x;
  if (a.w.seg_cnt[g] == 0 || a.w.frame_short[f]) return;        // the same in every thread
  const Segment sg = segment_of(a, g);
  int16_t* blocks = a.coefs + (f * a.frame_blocks + sg.fm * a.bpm) * 64;
  const long per = (sg.nblk + kThreads - 1) / kThreads;
  const long lo = min(sg.nblk, threadIdx.x * per), hi = min(sg.nblk, lo + per);
  int sum[3] = {0, 0, 0}, before[3];
  for (long b = lo; b < hi; ++b) {
    int& v = sum[component_of((int)(b % a.bpm), a.bpm)];
    v = (v + (uint16_t)blocks[b * 64]) & 0xffff;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {                    // 256 terms below 2^16: no overflow
    int total;
    before[c] = block_scan<kThreads>(sum[c], tmp, &total);
  }
  for (long b = lo; b < hi; ++b) {
    const int c = component_of((int)(b % a.bpm), a.bpm);
    before[c] = (before[c] + (uint16_t)blocks[b * 64]) & 0xffff;
    blocks[b * 64] = (int16_t)(uint16_t)before[c];
  }
}

bool sub_bytes_ok(int32_t b) { return b >= 64 && b <= 1024 && (b & (b - 1)) == 0; }

// the flat list's capacity and the workspace's parts, from what the host knows; non-zero: the refusal's code
int layout(const char* who, int64_t scan_bytes, int64_t F, int64_t S, int32_t sub_bytes, int32_t max_rounds, char* base, Work* w,
           int64_t* bytes) {
  LD_REQUIRE(sub_bytes_ok(sub_bytes), "%s: sub_bytes must be a power of two in 64 .. 1024, got %d", who, (int)sub_bytes);
  LD_REQUIRE(max_rounds >= 1 && max_rounds <= kMaxRounds, "%s: max_rounds must be in 1 .. %d, got %d", who, kMaxRounds, (int)max_rounds);
  LD_REQUIRE(scan_bytes > 0 && S > 0, "%s: scan_bytes and S must be positive, got %lld and %lld", who, (long long)scan_bytes, (long long)S);
  if (int rc = check_frames(who, F)) return rc;
  const int64_t NS = F * S;
  // sum of ceil(len / B) <= scan_bytes / B + NS; every frame is padded to whole workgroups
  const int64_t T = (scan_bytes / sub_bytes + NS + (int64_t)kLanes * F + kLanes - 1) / kLanes * kLanes;
  LD_REQUIRE(S < (1L << 31) && NS < (1L << 30) && T < (1L << 31), "%s: %lld segments / %lld subsequences exceed one call", who, (long long)NS,
             (long long)T);
  int64_t at = 0;
  auto take = [&](int64_t n) { char* p = base ? base + at : nullptr; at += (n + 15) / 16 * 16; return p; };
  w->E = reinterpret_cast<int4*>(take(2 * T * 16));
  w->seg_rel = reinterpret_cast<int32_t*>(take(NS * 4));
  w->seg_cnt = reinterpret_cast<int32_t*>(take(NS * 4));
  w->err = reinterpret_cast<int32_t*>(take(NS * 4));
  w->bad = reinterpret_cast<int32_t*>(take(NS * 4));
  w->mask = reinterpret_cast<int32_t*>(take(NS * 4));
  w->frame_total = reinterpret_cast<int32_t*>(take(F * 4));
  w->frame_base = reinterpret_cast<int32_t*>(take((F + 1) * 4));
  w->frame_short = reinterpret_cast<int32_t*>(take(F * 4));
  w->sub_seg = reinterpret_cast<int32_t*>(take(T * 4));
  w->first_block = reinterpret_cast<int32_t*>(take(T * 4));
  w->changed = reinterpret_cast<int32_t*>(take((int64_t)(max_rounds + 1) * (NS + F) * 4));
  w->frame_changed = w->changed + (int64_t)(max_rounds + 1) * NS;
  w->T = T;
  *bytes = at;
  return LD_OK;
}

}  // namespace

LD_API int64_t ld_jpeg_dec_sync_size(int32_t what, int64_t scan_bytes, int64_t F, int64_t S, int32_t sub_bytes, int32_t max_rounds) {
  Work w;
  int64_t bytes;
  if (int rc = layout("ld_jpeg_dec_sync_size", scan_bytes, F, S, sub_bytes, max_rounds, nullptr, &w, &bytes)) return rc;
  switch (what) {
    case LD_JPEG_DEC_SYNC_SIZE_WORKSPACE: return bytes;
    case LD_JPEG_DEC_SYNC_SIZE_SUBSEQUENCES: return w.T;
    default: return ld_set_error(LD_ERR_INVALID, "ld_jpeg_dec_sync_size: unknown quantity %d", (int)what);
  }
}

LD_API int ld_jpeg_decode_entropy_sync(const uint8_t* data, int64_t data_bytes, const int64_t* seg_table, const int64_t* frame_info,
                                       const int32_t* ri, const int32_t* tables, const int32_t* tset, int64_t n_sets, int16_t* coefs,
                                       int32_t* status, int64_t F, int64_t S, int64_t H, int64_t W, int32_t subsampling,
                                       int64_t scan_bytes, int32_t sub_bytes, int32_t max_rounds, void* workspace,
                                       int64_t workspace_bytes, int32_t* sync_info, int64_t* exits, int32_t* exits_index, void* stream) {
  const char* who = "ld_jpeg_decode_entropy_sync";
  Work w;
  int64_t need;
  if (int rc = layout(who, scan_bytes, F, S, sub_bytes, max_rounds, static_cast<char*>(workspace), &w, &need)) return rc;
  LD_REQUIRE(data && seg_table && frame_info && ri && tables && tset && coefs && status && workspace && sync_info, "%s: null pointer", who);
  LD_REQUIRE((exits == nullptr) == (exits_index == nullptr), "%s: exits and exits_index go together", who);
  LD_REQUIRE(aligned(seg_table, 8) && aligned(frame_info, 8) && aligned(ri, 4) && aligned(tables, 4) && aligned(tset, 4) &&
                 aligned(coefs, 16) && aligned(status, 4) && aligned(workspace, 16) && aligned(sync_info, 4) && aligned(exits, 8) &&
                 aligned(exits_index, 4),
             "%s: seg_table, frame_info and exits must be 8-byte, ri, tables, tset, status, sync_info and exits_index 4-byte, coefs and "
             "the workspace 16-byte aligned", who);
  LD_REQUIRE(data_bytes > 0 && n_sets > 0, "%s: data_bytes and n_sets must be positive", who);
  LD_REQUIRE(scan_bytes <= data_bytes, "%s: scan_bytes %lld exceed data_bytes %lld", who, (long long)scan_bytes, (long long)data_bytes);
  LD_REQUIRE(workspace_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed (ld_jpeg_dec_sync_size)", who,
             (long long)workspace_bytes, (long long)need);
  Geom g;
  if (int rc = geometry(who, H, W, subsampling, &g)) return rc;
  LD_REQUIRE((S + 63) / 64 < (1L << 31) && S < 65536L * 32768, "%s: %lld segments a frame exceed one launch", who, (long long)S);
  hipStream_t s = (hipStream_t)stream;
  const long NS = (long)F * S;
  SyncArgs a{data, seg_table, frame_info, ri, tables, tset, coefs, status, sync_info, exits, exits_index, w, (long)data_bytes, (long)S,
             (long)F, g.mcus, g.frame_blocks, (long)n_sets, g.bpm, (int)sub_bytes, (int)max_rounds, 0};
  if (hipMemsetAsync(w.changed, 0, (size_t)(max_rounds + 1) * (NS + F) * 4, s) != hipSuccess ||
      hipMemsetAsync(coefs, 0, (size_t)F * g.frame_blocks * 64 * sizeof(int16_t), s) != hipSuccess)
    return ld_set_error(LD_ERR_LAUNCH, "%s: a memset was not accepted", who);
  // segment kernels: x = the segment within the frame; S may exceed 65535 only in x (y = the frame, F <= 65535)
  const dim3 per_segment((unsigned)S, (unsigned)F), lanes((unsigned)(w.T / kLanes));
  hipLaunchKernelGGL(jpeg_sync_count_kernel, dim3((unsigned)F), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(jpeg_sync_frames_kernel, dim3(1), dim3(kThreads), 0, s, a);
  for (int r = 0; r <= max_rounds; ++r) {
    a.round = r;
    hipLaunchKernelGGL(jpeg_sync_round_kernel, lanes, dim3(kLanes), 0, s, a);
  }
  hipLaunchKernelGGL(jpeg_sync_prefix_kernel, per_segment, dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(jpeg_sync_write_kernel, lanes, dim3(kLanes), 0, s, a);
  hipLaunchKernelGGL(jpeg_sync_finish_kernel, dim3((unsigned)((NS + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(jpeg_sync_dc_kernel, per_segment, dim3(kThreads), 0, s, a);
  launch_entropy_segments(data, (long)data_bytes, seg_table, frame_info, ri, tables, tset, (long)n_sets, coefs, status, w.mask, (long)F,
                          (long)S, g, s);
  return ld_check_launch(who);
}
