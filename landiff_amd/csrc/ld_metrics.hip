// Clip comparison (landiff_amd/metrics.py): two uint8 channels-last clips a, b [F][H][W][C], C 1 or 3, and an optional per-pixel
// keep-mask [F][H][W] -> per (frame, channel) figures.  Nothing here is on the generation path.
//
// ld_clip_diff_u8: exact integer statistics (n, sum (a-b)^2, sum |a-b|, max |a-b|, number of a != b) as int64.  A thread adds the
// at most 16 bytes of one load in 32 bits (16 * 255^2 < 2^21) and everything beyond that in 64; blocks meet in integer atomics,
// which are exact in any order.
// ld_clip_ssim_u8: mean SSIM over the valid region of an 11-tap separable window (the definition: include/landiff_hip.h).  One
// workgroup per tile of the SSIM map: the footprint of both clips is staged in LDS as bytes (16-byte loads over the aligned
// middle of every row, byte loads over its ends, each clip at its own 16-byte phase: nothing outside the clip is read), the
// horizontal pass writes the five moment rows (x, y, x^2, y^2, xy, of x - 128 and y - 128: exact in fp32, the variances do not
// change and most of E[x^2] - mu^2's cancellation goes) as fp32 to LDS, the vertical pass, the formula and the tile's reduction
// follow.  A tile leaves one (sum, count) per channel in the workspace; a second kernel adds a frame's tiles in a fixed order.
//
// The arithmetic is written to be symmetric in (a, b) and to give exactly 1 for a == b: every product and sum below is rounded on
// its own, so no expression may be contracted into an fma (2 mx my + C1 and mx^2 + my^2 + C1 would stop being the same number).
#pragma clang fp contract(off)
#include "ld_common.h"
#include "../../include/landiff_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {     // a fixed tree: the same bits every time
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------------------------------------
// integer statistics
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int kDiffBlocksMax = 48;               // blocks per frame: a multiple of 3 (see below)

struct DiffAcc {                                  // one channel slot of one thread
  unsigned long long ssd, sad;
  unsigned n, ndiff, mx;                          // a frame has fewer than 2^31 bytes (checked by the launcher)
};

// a frame's bytes [0, n) as head bytes, 16-byte chunks and tail bytes: the chunks are 16-byte aligned in BOTH clips, which takes
// the two frame bases to share their phase -- otherwise (byte form) every byte is a tail byte
template <int C, bool MASK>
__global__ __launch_bounds__(kThreads) void ld_clip_diff_kernel(const uint8_t* a, const uint8_t* b, const uint8_t* mask,
                                                                unsigned long long* out, long n, int blocks_per_frame) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long f = blockIdx.x / blocks_per_frame;
  const int bi = blockIdx.x % blocks_per_frame;
  const uint8_t* fa = a + f * n;
  const uint8_t* fb = b + f * n;
  const uint8_t* fm = MASK ? mask + f * (n / C) : nullptr;
  const int pa = (int)((uintptr_t)fa & 15), pb = (int)((uintptr_t)fb & 15);
  const long head = pa == pb ? min(n, (long)((16 - pa) & 15)) : 0;
  const long nch = pa == pb ? (n - head) >> 4 : 0;
  const long tail0 = head + 16 * nch;             // first tail byte

  DiffAcc acc[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) acc[s] = DiffAcc{0, 0, 0, 0, 0};

  // ---- chunks.  Chunk k starts at byte head + 16 k, whose channel is (head + k) % 3 as 16 = 1 mod 3; a thread's chunks are
  // blocks_per_frame * kThreads apart, a multiple of 3, so they all start on one channel: byte i of any of them goes to slot i % C
  // and the slots are turned into channels once, below. ----
  const long g = (long)bi * kThreads + tid, stride = (long)blocks_per_frame * kThreads;
  for (long k = g; k < nch; k += stride) {
    const long o = head + 16 * k;
    const u32x4_t va = *reinterpret_cast<const u32x4_t*>(fa + o);
    const u32x4_t vb = *reinterpret_cast<const u32x4_t*>(fb + o);
    unsigned ssd[3] = {0, 0, 0}, sad[3] = {0, 0, 0};            // 16 bytes: at most 16 * 255^2, safe in 32 bits
    const long p0 = o / C;
    const int r0 = (int)(o - p0 * C);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int x = (va[i >> 2] >> (8 * (i & 3))) & 255, y = (vb[i >> 2] >> (8 * (i & 3))) & 255;
      const unsigned d = (unsigned)abs(x - y);
      const bool keep = MASK ? fm[p0 + (r0 + i) / C] != 0 : true;
      DiffAcc& s = acc[i % C];
      if (keep) {
        ssd[i % C] += d * d;
        sad[i % C] += d;
        s.n += 1;
        s.ndiff += d != 0;
        s.mx = max(s.mx, d);
      }
    }
#pragma unroll
    for (int s = 0; s < C; ++s) { acc[s].ssd += ssd[s]; acc[s].sad += sad[s]; }
  }
  if (C == 3) {                                   // slot s of this thread is channel (s + head + g) % 3
    const int rot = (int)((head + g) % 3);
    const DiffAcc t0 = acc[0], t1 = acc[1], t2 = acc[2];
    acc[0] = rot == 0 ? t0 : rot == 1 ? t2 : t1;
    acc[1] = rot == 0 ? t1 : rot == 1 ? t0 : t2;
    acc[2] = rot == 0 ? t2 : rot == 1 ? t1 : t0;
  }
  // ---- head and tail bytes, one per thread and round ----
  const long nedge = head + (n - tail0);
  for (long e = g; e < nedge; e += stride) {
    const long o = e < head ? e : tail0 + (e - head);
    const unsigned d = (unsigned)abs((int)fa[o] - (int)fb[o]);
    const long p = o / C;
    const int c = (int)(o - p * C);
    const bool keep = MASK ? fm[p] != 0 : true;
#pragma unroll
    for (int s = 0; s < C; ++s)
      if (keep && c == s) {
        acc[s].ssd += d * d;
        acc[s].sad += d;
        acc[s].n += 1;
        acc[s].ndiff += d != 0;
        acc[s].mx = max(acc[s].mx, d);
      }
  }
  // ---- the block's sums, then one atomic per figure ----
  __shared__ unsigned long long red[kWaves][3][5];
#pragma unroll
  for (int s = 0; s < C; ++s) {
    const unsigned long long v0 = wave_sum_u64(acc[s].n), v1 = wave_sum_u64(acc[s].ssd), v2 = wave_sum_u64(acc[s].sad);
    const unsigned long long v3 = wave_max_u32(acc[s].mx), v4 = wave_sum_u64(acc[s].ndiff);
    if (lane == 0) { red[wave][s][0] = v0; red[wave][s][1] = v1; red[wave][s][2] = v2; red[wave][s][3] = v3; red[wave][s][4] = v4; }
  }
  __syncthreads();
  if (tid < C * 5) {
    const int s = tid / 5, q = tid % 5;
    unsigned long long v = red[0][s][q];
    for (int w = 1; w < kWaves; ++w) v = q == 3 ? max(v, red[w][s][q]) : v + red[w][s][q];
    unsigned long long* dst = out + (f * C + s) * 5 + q;
    if (q == 3) atomicMax(dst, v); else if (v) atomicAdd(dst, v);
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// SSIM
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int kTaps = LD_SSIM_TAPS;               // 11
constexpr int kTileH = LD_SSIM_TILE_H;            // map rows of a tile
constexpr int kTileE = LD_SSIM_TILE_ELEMS;        // map elements (positions x channels) of a tile row: 48 / C positions
constexpr int kRows = kTileH + kTaps - 1;         // footprint rows
constexpr int kPitch = (kTileE + 3 * (kTaps - 1) + 15 + 15) & ~15;   // a staged row: up to 15 bytes of lead, then its bytes
constexpr int kMom = kRows * kTileE;              // floats of one moment plane
// LDS: 2 clips x 42 rows x 96 B + 5 planes x 42 x 48 x 4 B + the reduction = 49.3 KiB: three workgroups (12 waves) per CU.  A
// 16-row tile would fit five but its horizontal pass, the dearer one (it converts the bytes), covers 26 / 16 footprint rows per
// map row where this one covers 42 / 32.
static_assert(kTileE % 3 == 0, "a tile row holds whole pixels for C = 1 and C = 3");

struct SsimArgs {
  const uint8_t* a;
  const uint8_t* b;
  const uint8_t* mask;
  const float* win;
  double* ws;                                     // [F][tiles][C][2]
  int H, W, Hm, Wm, tiles_y, tiles_x;
};

// rows [0, rh) of n bytes each, gstep apart from g0, into LDS: row r's byte k lands at u8[r * kPitch + phase(r) + k], phase the
// low four bits of the row's global address, so that an aligned 16-byte chunk of the row moves as one load and one store
__device__ __forceinline__ void stage_rows(const uint8_t* g0, long gstep, int rh, int n, unsigned char* u8, int tid) {
  const uintptr_t gph = (uintptr_t)g0;
  constexpr int nch = kPitch >> 4;
  for (int i = tid; i < rh * nch; i += kThreads) {
    const int r = i / nch, c = i - r * nch;
    const int ph = (int)((gph + r * gstep) & 15);
    const int lo = 16 * c - ph;                   // the chunk's first byte, counted from the row's first
    if (lo >= 0 && lo + 16 <= n) *reinterpret_cast<u32x4_t*>(u8 + r * kPitch + 16 * c) = *reinterpret_cast<const u32x4_t*>(g0 + r * gstep + lo);
  }
  for (int i = tid; i < rh * 32; i += kThreads) { // per row 16 candidates for head bytes, 16 for tail bytes
    const int r = i >> 5, e = i & 15;
    const int ph = (int)((gph + r * gstep) & 15);
    const int head = min(n, (16 - ph) & 15), tail = (n - head) & 15;
    const int k = (i & 16) ? n - tail + e : e;
    if (e < ((i & 16) ? tail : head)) u8[r * kPitch + ph + k] = g0[r * gstep + k];
  }
}

template <int C, bool MASK>
__global__ __launch_bounds__(kThreads) void ld_clip_ssim_kernel(SsimArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char sa[kRows * kPitch];
  __shared__ __attribute__((aligned(16))) unsigned char sb[kRows * kPitch];
  __shared__ float mom[5 * kMom];
  __shared__ double red_s[kWaves][3];
  __shared__ int red_n[kWaves][3];
  constexpr int TW = kTileE / C;                  // map positions of a tile row
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long blk = blockIdx.x;
  const int tx = (int)(blk % p.tiles_x), ty = (int)((blk / p.tiles_x) % p.tiles_y);
  const long f = blk / ((long)p.tiles_x * p.tiles_y);
  const int oy0 = ty * kTileH, ox0 = tx * TW;
  const int th = min(kTileH, p.Hm - oy0), twe = min(TW, p.Wm - ox0) * C;
  const int rh = th + kTaps - 1, n = twe + (kTaps - 1) * C;     // footprint rows, bytes of a footprint row
  const long gstep = (long)p.W * C;
  const long goff = ((f * p.H + oy0) * p.W + ox0) * C;

  float w[kTaps];
#pragma unroll
  for (int t = 0; t < kTaps; ++t) w[t] = p.win[t];

  stage_rows(p.a + goff, gstep, rh, n, sa, tid);
  stage_rows(p.b + goff, gstep, rh, n, sb, tid);
  __syncthreads();

  // ---- horizontal pass: footprint row r, element j -> the five moments, taps added in ascending order ----
  const uintptr_t pha = (uintptr_t)(p.a + goff), phb = (uintptr_t)(p.b + goff);
  for (int i = tid; i < rh * twe; i += kThreads) {
    const int r = i / twe, j = i - r * twe;
    const unsigned char* ra = sa + r * kPitch + (int)((pha + r * gstep) & 15) + j;
    const unsigned char* rb = sb + r * kPitch + (int)((phb + r * gstep) & 15) + j;
    float hx = 0.0f, hy = 0.0f, hxx = 0.0f, hyy = 0.0f, hxy = 0.0f;
#pragma unroll
    for (int t = 0; t < kTaps; ++t) {
      const float x = (float)ra[t * C] - 128.0f, y = (float)rb[t * C] - 128.0f;
      hx = hx + w[t] * x;
      hy = hy + w[t] * y;
      hxx = hxx + w[t] * (x * x);
      hyy = hyy + w[t] * (y * y);
      hxy = hxy + w[t] * (x * y);
    }
    float* m = mom + r * kTileE + j;
    m[0] = hx; m[kMom] = hy; m[2 * kMom] = hxx; m[3 * kMom] = hyy; m[4 * kMom] = hxy;
  }
  __syncthreads();

  // ---- vertical pass, the formula, the thread's sums ----
  const float C1 = 6.5025f, C2 = 58.5225f;        // (0.01 * 255)^2, (0.03 * 255)^2
  double sum[3] = {0.0, 0.0, 0.0};
  int cnt[3] = {0, 0, 0};
  for (int i = tid; i < th * twe; i += kThreads) {
    const int oy = i / twe, j = i - oy * twe;
    const float* m = mom + oy * kTileE + j;
    float v[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      float s = 0.0f;
#pragma unroll
      for (int t = 0; t < kTaps; ++t) s = s + w[t] * m[q * kMom + t * kTileE];
      v[q] = s;
    }
    const float mx = v[0] + 128.0f, my = v[1] + 128.0f;
    const float vx = v[2] - v[0] * v[0], vy = v[3] - v[1] * v[1], vxy = v[4] - v[0] * v[1];
    const float num = (2.0f * (mx * my) + C1) * (2.0f * vxy + C2);
    const float den = ((mx * mx + my * my) + C1) * ((vx + vy) + C2);
    const float ssim = num / den;
    const int px = j / C, c = j - px * C;
    const bool keep = MASK ? p.mask[(f * p.H + oy0 + oy + kTaps / 2) * p.W + ox0 + px + kTaps / 2] != 0 : true;
#pragma unroll
    for (int s = 0; s < C; ++s)
      if (keep && c == s) { sum[s] += (double)ssim; cnt[s] += 1; }
  }
#pragma unroll
  for (int s = 0; s < C; ++s) {
    const double vs = wave_sum_f64(sum[s]);
    const int vn = (int)wave_sum_u64((unsigned long long)cnt[s]);
    if (lane == 0) { red_s[wave][s] = vs; red_n[wave][s] = vn; }
  }
  __syncthreads();
  if (tid < C) {
    double vs = red_s[0][tid];
    int vn = red_n[0][tid];
    for (int k = 1; k < kWaves; ++k) { vs += red_s[k][tid]; vn += red_n[k][tid]; }
    double* o = p.ws + (blk * C + tid) * 2;
    o[0] = vs;
    o[1] = (double)vn;
  }
}

// out[f][c] = the frame's tiles added in a fixed order: thread t adds tiles t, t + 256, ... in turn, then the block's fixed tree
__global__ __launch_bounds__(kThreads) void ld_clip_ssim_sum_kernel(const double* ws, double* out, int tiles, int C) {
  __shared__ double red[kWaves][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long f = blockIdx.x / C;
  const int c = blockIdx.x % C;
  double s = 0.0, n = 0.0;
  for (int t = tid; t < tiles; t += kThreads) {
    const double* v = ws + ((f * tiles + t) * C + c) * 2;
    s += v[0];
    n += v[1];
  }
  s = wave_sum_f64(s);
  n = wave_sum_f64(n);
  if (lane == 0) { red[wave][0] = s; red[wave][1] = n; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < kWaves; ++k) { s += red[k][0]; n += red[k][1]; }
    out[2 * (long)blockIdx.x] = s;
    out[2 * (long)blockIdx.x + 1] = n;
  }
}

int check_shape(const char* name, int64_t F, int64_t H, int64_t W, int64_t C) {
  LD_REQUIRE(C == 1 || C == 3, "%s: C must be 1 or 3, got %lld", name, (long long)C);
  LD_REQUIRE(F > 0 && H > 0 && W > 0, "%s: empty shape [%lld][%lld][%lld][%lld]", name, (long long)F, (long long)H, (long long)W, (long long)C);
  LD_REQUIRE(F < (1 << 20) && H < (1 << 20) && W < (1 << 20) && H * W * C < (1LL << 31),
             "%s: a frame must hold fewer than 2^31 bytes and a clip fewer than 2^20 frames, got [%lld][%lld][%lld][%lld]", name,
             (long long)F, (long long)H, (long long)W, (long long)C);
  return LD_OK;
}

}  // namespace

LD_API int ld_clip_diff_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, int64_t* out, int64_t F, int64_t H, int64_t W,
                           int64_t C, void* stream) {
  LD_REQUIRE(a && b && out, "ld_clip_diff_u8: null pointer");
  if (int rc = check_shape("ld_clip_diff_u8", F, H, W, C)) return rc;
  const long n = (long)(H * W * C);
  long bpf = (n / 16 + kThreads * 4 - 1) / (kThreads * 4);       // about four chunks per thread ...
  bpf = 3 * ((bpf + 2) / 3);                                     // ... in a multiple of 3 blocks (the kernel's channel rule)
  if (bpf < 3) bpf = 3;
  if (bpf > kDiffBlocksMax) bpf = kDiffBlocksMax;
  LD_REQUIRE(F * bpf < (1LL << 31), "ld_clip_diff_u8: %lld frames exceed one launch", (long long)F);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, (size_t)(F * C * 5) * sizeof(int64_t), st) != hipSuccess)
    return ld_set_error(LD_ERR_LAUNCH, "ld_clip_diff_u8: clearing the output failed");
  unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
  const dim3 grid((unsigned)(F * bpf)), block(kThreads);
  if (C == 3 && mask) hipLaunchKernelGGL((ld_clip_diff_kernel<3, true>), grid, block, 0, st, a, b, mask, o, n, (int)bpf);
  else if (C == 3) hipLaunchKernelGGL((ld_clip_diff_kernel<3, false>), grid, block, 0, st, a, b, mask, o, n, (int)bpf);
  else if (mask) hipLaunchKernelGGL((ld_clip_diff_kernel<1, true>), grid, block, 0, st, a, b, mask, o, n, (int)bpf);
  else hipLaunchKernelGGL((ld_clip_diff_kernel<1, false>), grid, block, 0, st, a, b, mask, o, n, (int)bpf);
  return ld_check_launch("ld_clip_diff_u8");
}

LD_API int ld_clip_ssim_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, const float* window, double* out,
                           double* workspace, int64_t workspace_doubles, int64_t F, int64_t H, int64_t W, int64_t C, void* stream) {
  LD_REQUIRE(a && b && window && out && workspace, "ld_clip_ssim_u8: null pointer");
  if (int rc = check_shape("ld_clip_ssim_u8", F, H, W, C)) return rc;
  LD_REQUIRE(H >= kTaps && W >= kTaps, "ld_clip_ssim_u8: the %d-tap window needs H, W >= %d, got %lld x %lld", kTaps, kTaps,
             (long long)H, (long long)W);
  const int Hm = (int)H - kTaps + 1, Wm = (int)W - kTaps + 1, TW = kTileE / (int)C;
  SsimArgs p{a, b, mask, window, workspace, (int)H, (int)W, Hm, Wm, (Hm + kTileH - 1) / kTileH, (Wm + TW - 1) / TW};
  const long tiles = (long)p.tiles_y * p.tiles_x;
  LD_REQUIRE(workspace_doubles >= F * tiles * C * 2, "ld_clip_ssim_u8: the workspace holds %lld doubles, [%lld][%ld][%lld][2] are "
             "needed (tiles of %d x %d map positions)", (long long)workspace_doubles, (long long)F, tiles, (long long)C, kTileH, TW);
  LD_REQUIRE(F * tiles < (1LL << 31), "ld_clip_ssim_u8: %lld tiles exceed one launch", (long long)(F * tiles));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(F * tiles)), block(kThreads);
  if (C == 3 && mask) hipLaunchKernelGGL((ld_clip_ssim_kernel<3, true>), grid, block, 0, st, p);
  else if (C == 3) hipLaunchKernelGGL((ld_clip_ssim_kernel<3, false>), grid, block, 0, st, p);
  else if (mask) hipLaunchKernelGGL((ld_clip_ssim_kernel<1, true>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((ld_clip_ssim_kernel<1, false>), grid, block, 0, st, p);
  if (int rc = ld_check_launch("ld_clip_ssim_u8")) return rc;
  hipLaunchKernelGGL(ld_clip_ssim_sum_kernel, dim3((unsigned)(F * C)), block, 0, st, workspace, out, (int)tiles, (int)C);
  return ld_check_launch("ld_clip_ssim_u8 (sum)");
}
