// The retime stage (landiff_amd/retime.py): uint8 channels-last frames at another frame rate, in-between frames made by
// bilateral block matching and motion-compensated blending.  Integer arithmetic only: no float anywhere in this file (the only
// float instructions in its ISA are the compiler's exact expansion of integer division).
//
// ld_retime_u8: one launch for the whole clip, one workgroup per group of 2 x 2 output blocks (16 x 16 pixels) of one output frame.
// Output frame k lies at source position src_idx[k] + phase_p[k] / q.  phase 0: the group is copied.  Otherwise, between
// A = src[i] and B = src[i + 1]:
//   * the luma of the group's two search windows ((24 + 2R)^2 texels each, the union of its blocks' (16 + 2R)^2 windows,
//     coordinates clamped to the frame) is computed once while they are staged in LDS as bytes -- not once per candidate;
//   * the blocks' (2R + 1)^2 candidates d = (dy, dx) are spread over the 256 lanes.  A candidate splits into the read offsets
//     a = -rhu(p d, q) into A (a table of 2R + 1 entries, made once per workgroup) and b = d + a into B; its 16 x 16 SAD runs on
//     packed bytes (v_sad_u8), sixteen at a time: the five aligned dwords that hold a row's sixteen bytes are read from LDS and
//     v_alignbyte shifts them into place;
//   * a block's arg-min of (cost, |dy| + |dx|, dy, dx) is one unsigned 64-bit min (an LDS atomic) over a key packed in that order;
//   * a chosen SAD above max_sad * 256 falls back to d = (0, 0); then every pixel and channel of the block is
//     rhu((q - p) A[y + a] + p B[y + b], q), read from global memory with clamped coordinates.
// Nothing depends on the order in which lanes or workgroups finish (a min, and disjoint stores): two runs give the same bits.
#include "ld_common.h"
#include "../../include/landiff_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBlock = 8;                          // output block edge
constexpr int kWin = 16;                           // matching window edge, centred on the block: rows 8 by - 4 .. 8 by + 11
constexpr int kLead = (kWin - kBlock) / 2;
constexpr int kGroup = 2;                          // blocks per workgroup and axis
constexpr int kMaxSearch = 32;
constexpr int kHeader = 160;                       // u64 best[4] | int fin[4][2] | signed char aoff[2 * 32 + 1], padded

struct RetimeArgs {
  const uint8_t* src;
  uint8_t* dst;
  const int32_t* src_idx;
  const int32_t* phase_p;
  int16_t* mv;
  int32_t* sad;
  int q, F, H, W, C, nby, nbx, ngy, ngx, R, penalty, max_sad;
};

// floor(n / m) for m > 0
__device__ __forceinline__ int floor_div(int n, int m) { return n >= 0 ? n / m : -((-n + m - 1) / m); }
// round half up with floor division
__device__ __forceinline__ int rhu(int n, int m) { return floor_div(2 * n + m, 2 * m); }

__host__ __device__ inline int win_edge(int R) { return kWin + kBlock * (kGroup - 1) + 2 * R; }     // texels per axis, a whole group
__host__ __device__ inline int win_pitch(int R) { return (win_edge(R) + 3) & ~3; }                  // bytes, a multiple of 4
// one window: rows of `pitch` bytes and one spare dword (the unaligned reads of the last row look one dword ahead)
__host__ __device__ inline int win_bytes(int R) { return (win_edge(R) * win_pitch(R) + 4 + 15) & ~15; }

// the sixteen bytes at byte offset `o` of a window (o + 20 <= its size), as four dwords.  The bytes of the fifth dword past the
// sixteenth are shifted out again: no result depends on them (they may be a row's spare bytes, which nobody writes).
__device__ __forceinline__ void row16(const uint32_t* w, int o, uint32_t v[4]) {
  const uint32_t* p = w + (o >> 2);
  const uint32_t sh = (uint32_t)o & 3u;
  const uint32_t d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3], d4 = p[4];
  v[0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
  v[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
  v[2] = __builtin_amdgcn_alignbyte(d3, d2, sh);
  v[3] = __builtin_amdgcn_alignbyte(d4, d3, sh);
}

__global__ __launch_bounds__(kThreads) void ld_retime_kernel(RetimeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int C = a.C, H = a.H, W = a.W, R = a.R;
  const long grp = blockIdx.x;
  const int gx = (int)(grp % a.ngx), gy = (int)((grp / a.ngx) % a.ngy);
  const long k = grp / ((long)a.ngx * a.ngy);
  const int y0 = gy * kGroup * kBlock, x0 = gx * kGroup * kBlock;                  // the group's first pixel
  const int gh = min(kGroup * kBlock, H - y0), gw = min(kGroup * kBlock, W - x0);  // its pixels ...
  const int nb_y = (gh + kBlock - 1) / kBlock, nb_x = (gw + kBlock - 1) / kBlock;  // ... and blocks inside the frame
  const int q = a.q;
  // the caller checks both tables; whatever they hold, no read leaves src
  int p = min(max(a.phase_p[k], 0), q - 1);
  const int i0 = min(max(a.src_idx[k], 0), a.F - 1);
  if (i0 >= a.F - 1) p = 0;
  const long frame = (long)H * W * C;
  const uint8_t* A = a.src + (long)i0 * frame;
  uint8_t* out = a.dst + k * frame;
  const int gwc = gw * C;

  if (p == 0) {                                     // (uniform over the workgroup)
    for (int e = tid; e < gh * gwc; e += kThreads) {
      const int row = e / gwc, j = e - row * gwc;
      const long o = ((long)(y0 + row) * W + x0) * C + j;
      out[o] = A[o];
    }
    if (tid < nb_y * nb_x) {
      const long cell = (k * a.nby + gy * kGroup + tid / nb_x) * a.nbx + gx * kGroup + tid % nb_x;
      if (a.mv) { a.mv[2 * cell] = 0; a.mv[2 * cell + 1] = 0; }
      if (a.sad) a.sad[cell] = 0;
    }
    return;
  }
  const uint8_t* B = A + frame;

  unsigned long long* best = reinterpret_cast<unsigned long long*>(smem);
  int* fin = reinterpret_cast<int*>(smem + 32);
  signed char* aoff = reinterpret_cast<signed char*>(smem + 64);                   // aoff[d + R] = -rhu(p d, q), |aoff| <= R
  const int pitch = win_pitch(R), wbytes = win_bytes(R);
  unsigned char* ya = smem + kHeader;
  unsigned char* yb = ya + wbytes;
  if (tid < kGroup * kGroup) best[tid] = ~0ull;
  if (tid <= 2 * R) aoff[tid] = (signed char)(-rhu(p * (tid - R), q));

  // ---- stage the luma of both windows: window texel (r, c) is frame texel (clamp(y0 - 4 - R + r), clamp(x0 - 4 - R + c)).
  // Rows 0 .. Sy - 1 are A's, Sy .. 2 Sy - 1 are B's; a thread walks (r, c) in steps of 256 texels without dividing again. ----
  const int Sy = kWin + kBlock * (nb_y - 1) + 2 * R, Sx = kWin + kBlock * (nb_x - 1) + 2 * R;
  {
    const int step_r = kThreads / Sx, step_c = kThreads - step_r * Sx;
    int r = tid / Sx, c = tid - r * Sx;
    while (r < 2 * Sy) {
      const int f = r >= Sy, rr = f ? r - Sy : r;
      const int y = min(max(y0 - kLead - R + rr, 0), H - 1), x = min(max(x0 - kLead - R + c, 0), W - 1);
      const uint8_t* px = (f ? B : A) + ((long)y * W + x) * C;
      uint32_t l = px[0];
      if (C == 3) l = (77u * l + 150u * px[1] + 29u * px[2] + 128u) >> 8;
      (f ? yb : ya)[rr * pitch + c] = (unsigned char)l;
      r += step_r; c += step_c;
      if (c >= Sx) { c -= Sx; ++r; }
    }
  }
  __syncthreads();

  // ---- candidates over the lanes.  key = cost << 24 | (|dy| + |dx|) << 16 | (dy + R) << 8 | (dx + R): cost < 2^17, the
  // other three fields <= 64, so the unsigned order of the key is the order of the tuple (cost, |dy| + |dx|, dy, dx). ----
  const uint32_t* wa = reinterpret_cast<const uint32_t*>(ya);
  const uint32_t* wb = reinterpret_cast<const uint32_t*>(yb);
  const int side = 2 * R + 1, ncand = side * side, nblk = nb_y * nb_x;
  for (int i = tid; i < nblk * ncand; i += kThreads) {
    const int blk = i / ncand, cnd = i - blk * ncand;
    const int jy = blk / nb_x, jx = blk - jy * nb_x;
    const int ry = cnd / side, rx = cnd - ry * side;                              // dy + R, dx + R
    const int dy = ry - R, dx = rx - R;
    const int ay = aoff[ry], ax = aoff[rx];
    // the block's window starts at (8 jy, 8 jx) of the group's; + R: displacement 0
    const int oa = (kBlock * jy + R + ay) * pitch + kBlock * jx + R + ax;
    const int ob = (kBlock * jy + R + dy + ay) * pitch + kBlock * jx + R + dx + ax;
    uint32_t s = 0;
#pragma unroll 4
    for (int r = 0; r < kWin; ++r) {
      uint32_t va[4], vb[4];
      row16(wa, oa + r * pitch, va);
      row16(wb, ob + r * pitch, vb);
#pragma unroll
      for (int u = 0; u < 4; ++u) s = __builtin_amdgcn_sad_u8(va[u], vb[u], s);
    }
    const uint32_t l1 = (uint32_t)(abs(dy) + abs(dx));
    const unsigned long long cost = s + (uint32_t)a.penalty * l1;
    atomicMin(&best[blk], cost << 24 | (unsigned long long)l1 << 16 | (uint32_t)ry << 8 | (uint32_t)rx);
  }
  __syncthreads();
  if (tid < nblk) {
    const unsigned long long key = best[tid];
    const int l1 = (int)(key >> 16 & 0xff);
    int dy = (int)(key >> 8 & 0xff) - R, dx = (int)(key & 0xff) - R;
    const int s = (int)(key >> 24) - a.penalty * l1;
    if (s > a.max_sad * 256) dy = dx = 0;            // the stored SAD stays the chosen candidate's
    fin[2 * tid] = dy; fin[2 * tid + 1] = dx;
    const long cell = (k * a.nby + gy * kGroup + tid / nb_x) * a.nbx + gx * kGroup + tid % nb_x;
    if (a.mv) { a.mv[2 * cell] = (int16_t)dy; a.mv[2 * cell + 1] = (int16_t)dx; }
    if (a.sad) a.sad[cell] = s;
  }
  __syncthreads();

  // ---- compensation: out = rhu((q - p) A[y + a] + p B[y + b], q), coordinates clamped ----
  for (int e = tid; e < gh * gwc; e += kThreads) {
    const int row = e / gwc, j = e - row * gwc, col = C == 3 ? j / 3 : j, c = j - col * C;
    const int blk = (row / kBlock) * nb_x + col / kBlock;
    const int dy = fin[2 * blk], dx = fin[2 * blk + 1];
    const int ay = aoff[dy + R], ax = aoff[dx + R];
    const int y = y0 + row, x = x0 + col;
    const int yA = min(max(y + ay, 0), H - 1), xA = min(max(x + ax, 0), W - 1);
    const int yB = min(max(y + dy + ay, 0), H - 1), xB = min(max(x + dx + ax, 0), W - 1);
    const uint32_t va = A[((long)yA * W + xA) * C + c], vb = B[((long)yB * W + xB) * C + c];
    const uint32_t n = (uint32_t)(q - p) * va + (uint32_t)p * vb;              // <= 65535 * 255
    out[((long)y * W + x) * C + c] = (uint8_t)((2u * n + (uint32_t)q) / (2u * (uint32_t)q));
  }
}

}  // namespace

LD_API int ld_retime_u8(const uint8_t* src, uint8_t* dst, const int32_t* src_idx, const int32_t* phase_p, int32_t q, int16_t* mv,
                        int32_t* sad, int64_t F, int64_t n_out, int64_t H, int64_t W, int64_t C, int32_t search, int32_t penalty,
                        int32_t max_sad, void* stream) {
  LD_REQUIRE(src && dst && src_idx && phase_p, "ld_retime_u8: null pointer");
  LD_REQUIRE(C == 1 || C == 3, "ld_retime_u8: C must be 1 or 3, got %lld", (long long)C);
  LD_REQUIRE(F > 0 && n_out > 0 && H > 0 && W > 0, "ld_retime_u8: empty shape");
  LD_REQUIRE(F < (1 << 30) && n_out < (1 << 30) && H < (1 << 24) && W < (1 << 24), "ld_retime_u8: shape too large");
  LD_REQUIRE(search >= 0 && search <= kMaxSearch, "ld_retime_u8: search must be in 0..%d, got %d", kMaxSearch, (int)search);
  LD_REQUIRE(penalty >= 0 && penalty <= 255, "ld_retime_u8: penalty must be in 0..255, got %d", (int)penalty);
  LD_REQUIRE(max_sad >= 0 && max_sad <= 255, "ld_retime_u8: max_sad must be in 0..255, got %d", (int)max_sad);
  LD_REQUIRE(q >= 1 && q <= 65535, "ld_retime_u8: q must be in 1..65535, got %d", (int)q);
  const int nby = (int)((H + kBlock - 1) / kBlock), nbx = (int)((W + kBlock - 1) / kBlock);
  RetimeArgs a{src, dst, src_idx, phase_p, mv, sad, (int)q, (int)F, (int)H, (int)W, (int)C, nby, nbx, (nby + kGroup - 1) / kGroup,
               (nbx + kGroup - 1) / kGroup, (int)search, (int)penalty, (int)max_sad};
  const long groups = (long)a.ngy * a.ngx * n_out;
  LD_REQUIRE(groups < (1L << 31), "ld_retime_u8: %ld block groups exceed one launch", groups);
  const size_t smem = kHeader + 2 * (size_t)win_bytes(a.R);                     // at most 160 + 2 * 7760 bytes
  hipLaunchKernelGGL(ld_retime_kernel, dim3((unsigned)groups), dim3(kThreads), smem, (hipStream_t)stream, a);
  return ld_check_launch("ld_retime_u8");
}
