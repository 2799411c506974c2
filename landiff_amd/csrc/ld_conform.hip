// The conform stage (landiff_amd/conform.py): input clips, images and keep-masks of any size brought to the model's frame.
//
// ld_resize_u8: antialiased separable resampling of uint8 channels-last frames with a source crop box and a frame gather
// fused in -- the job torchvision's resize does for the reference (landiff/tokenizer/theia_extractor.py:88-90).
// ld_resize_mask_u8: the same geometry over a keep-mask, conservative (a pixel is kept only if its whole tap window is).
//
// The filter lives in tables the caller builds in float64 and rounds to fp32 (per axis: the window [lo, lo + cnt) of every
// output index inside the crop box, and cnt normalised weights in a row of tmax floats): no filter maths here, and no cap on the
// tap count.  One workgroup per destination tile: the tile's source footprint is staged in LDS as uint8 (16-byte loads over the
// aligned middle of every row, byte loads over its unaligned ends: nothing outside the box is read), the horizontal pass
// writes fp32 to LDS, the vertical pass reads it and stores the rounded bytes -- a source byte leaves HBM about once and nothing
// intermediate goes to HBM.  A tile whose footprint does not fit the LDS it was launched with takes the direct form: the
// workgroup's threads share the taps of one output pixel at a time, straight from global memory, and reduce.
#include "ld_common.h"
#include "../../include/landiff_hip.h"

#include <math.h>

namespace {

struct ResizeArgs {
  const uint8_t* src;
  uint8_t* dst;
  const int32_t* frame_idx;
  const int32_t* win_y;      // [Ho][2]: lo, cnt (relative to the box)
  const float* w_y;          // [Ho][tmax_y]  (null in the mask form)
  const int32_t* win_x;
  const float* w_x;
  int Fs, Hs, Ws, C, Ho, Wo, y0, x0, hc, wc, tmax_y, tmax_x;
  int TH, TW, tiles_y, tiles_x;
  int rh_cap, rw_cap;        // footprint rows / columns the launch's LDS holds (0, 0: the direct form only)
};

constexpr int kThreads = 256;
constexpr int kStage = 4;                         // loads of a kind a thread keeps in flight while staging
constexpr int kHeader = 64;                       // int fp[4] (footprint bounds) + float red[12] (the direct form's reduction)

inline __host__ __device__ long align16(long v) { return (v + 15) & ~15L; }
// the row pitch of the staged footprint: a row starts at the 16-byte phase of its global address, so up to 15 bytes of lead
inline __host__ __device__ int row_pitch(int rw, int C) { return (int)align16((long)rw * C + 15); }

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// One tap.  Resize: acc + w * v in one fma.  Mask: v is 0 / 1 and the result is the AND so far.
template <bool MASK>
__device__ __forceinline__ float tap(float acc, float w, float v) { return MASK ? fminf(acc, v) : fmaf(w, v, acc); }
template <bool MASK>
__device__ __forceinline__ float pixel(uint8_t b) { return MASK ? (b ? 1.0f : 0.0f) : (float)b; }

template <bool MASK>
__global__ __launch_bounds__(kThreads) void ld_resize_kernel(ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C, TWC = a.TW * C;
  const long b = blockIdx.x;
  const int tx = (int)(b % a.tiles_x), ty = (int)((b / a.tiles_x) % a.tiles_y);
  const long k = b / ((long)a.tiles_x * a.tiles_y);
  int f = a.frame_idx ? a.frame_idx[k] : (int)k;
  f = min(max(f, 0), a.Fs - 1);                   // the caller checks the range; a bad index still cannot leave src
  const int oy0 = ty * a.TH, th = min(a.TH, a.Ho - oy0), ox0 = tx * a.TW, tw = min(a.TW, a.Wo - ox0);

  int* fp = reinterpret_cast<int*>(smem);
  float* red = reinterpret_cast<float*>(smem + 16);
  int2* wins_y = reinterpret_cast<int2*>(smem + kHeader);
  int2* wins_x = wins_y + a.TH;
  long off = align16(kHeader + (long)(a.TH + a.TW) * 8);
  unsigned char* u8 = smem + off;
  const int pitch = row_pitch(a.rw_cap, C);
  off += align16((long)a.rh_cap * pitch);
  float* inter = reinterpret_cast<float*>(smem + off);
  off += align16((long)a.rh_cap * TWC * 4);
  float* wx_s = reinterpret_cast<float*>(smem + off);
  off += align16((long)a.TW * a.tmax_x * 4);
  float* wy_s = reinterpret_cast<float*>(smem + off);

  // ---- the tile's windows (clamped into the box whatever the tables hold) and its footprint ----
  if (tid == 0) { fp[0] = a.hc; fp[1] = 0; fp[2] = a.wc; fp[3] = 0; }
  __syncthreads();
  if (tid < th + tw) {
    const bool isy = tid < th;
    const int i = isy ? tid : tid - th, n_in = isy ? a.hc : a.wc;
    const int32_t* w = isy ? a.win_y + 2L * (oy0 + i) : a.win_x + 2L * (ox0 + i);
    const int lo = min(max(w[0], 0), n_in);
    int cnt = min(max(w[1], 0), n_in - lo);
    if (!MASK) cnt = min(cnt, isy ? a.tmax_y : a.tmax_x);
    (isy ? wins_y : wins_x)[i] = make_int2(lo, cnt);
    atomicMin(&fp[isy ? 0 : 2], lo);
    atomicMax(&fp[isy ? 1 : 3], lo + cnt);
  }
  __syncthreads();
  const int ry0 = fp[0], rh = fp[1] - fp[0], rx0 = fp[2], rw = fp[3] - fp[2];
  uint8_t* out = a.dst + ((k * a.Ho + oy0) * a.Wo + ox0) * C;

  if (rh > 0 && rw > 0 && rh <= a.rh_cap && rw <= a.rw_cap) {
    // ---- stage the footprint.  A row sits in LDS at the 16-byte phase of its global address, so the aligned 16-byte chunks that
    // lie wholly inside it move as one load and one store each; the up to 15 bytes at either end move byte by byte.  A thread
    // issues kStage loads of each kind before its first store: the loop is bound by memory latency otherwise. ----
    const uint8_t* g0 = a.src + (((long)f * a.Hs + a.y0 + ry0) * a.Ws + a.x0 + rx0) * C;
    const uintptr_t gph = (uintptr_t)g0;
    const long gstep = (long)a.Ws * C;
    const int n = rw * C, nch = pitch >> 4;
    const int nci = rh * nch, nei = rh * 32;                      // chunk items; per row 16 candidates for head bytes, 16 for tail bytes
    for (int base = tid; base < max(nci, nei); base += kStage * kThreads) {
      u32x4_t cv[kStage];
      unsigned char ev[kStage];
      int co[kStage], eo[kStage];
#pragma unroll
      for (int u = 0; u < kStage; ++u) {
        const int i = base + u * kThreads, r = i / nch, c = i - r * nch;
        const int ph = (int)((gph + r * gstep) & 15);
        const int lo = 16 * c - ph;                               // the chunk's first byte, counted from the row's first
        co[u] = i < nci && lo >= 0 && lo + 16 <= n ? r * pitch + 16 * c : -1;
        if (co[u] >= 0) cv[u] = *reinterpret_cast<const u32x4_t*>(g0 + r * gstep + lo);
      }
#pragma unroll
      for (int u = 0; u < kStage; ++u) {
        const int i = base + u * kThreads, r = i >> 5, e = i & 15;
        const int ph = (int)((gph + r * gstep) & 15);
        const int head = min(n, (16 - ph) & 15), tail = (n - head) & 15;
        const int k = (i & 16) ? n - tail + e : e;                // byte of the row
        eo[u] = i < nei && e < ((i & 16) ? tail : head) ? r * pitch + ph + k : -1;
        if (eo[u] >= 0) ev[u] = g0[r * gstep + k];
      }
#pragma unroll
      for (int u = 0; u < kStage; ++u)
        if (co[u] >= 0) *reinterpret_cast<u32x4_t*>(u8 + co[u]) = cv[u];
#pragma unroll
      for (int u = 0; u < kStage; ++u)
        if (eo[u] >= 0) u8[eo[u]] = ev[u];
    }
    if (!MASK) {
      for (int i = tid; i < tw * a.tmax_x; i += kThreads) wx_s[i] = a.w_x[(long)ox0 * a.tmax_x + i];
      for (int i = tid; i < th * a.tmax_y; i += kThreads) wy_s[i] = a.w_y[(long)oy0 * a.tmax_y + i];
    }
    __syncthreads();
    // ---- horizontal pass: footprint row r, output column ox, channel c -> inter[r][ox][c].  A thread carries four rows at once
    // (they share the weights) and four taps per sweep: sixteen independent LDS reads in flight.  A tap past the window reads the
    // window's last pixel with weight 0 (mask form: 1, the neutral value), which leaves the sum as it is. ----
    for (int rq = 4 * wave; rq < rh; rq += kThreads / 16) {
      const unsigned char* row[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = min(rq + q, rh - 1);
        row[q] = u8 + (long)r * pitch + (int)((gph + r * gstep) & 15);
      }
      for (int j = lane; j < tw * C; j += 64) {
        const int ox = C == 3 ? j / 3 : j;
        const int2 wn = wins_x[ox];
        const int so = (wn.x - rx0) * C + (j - ox * C);
        const float* w = wx_s + ox * a.tmax_x;
        float acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = MASK ? 1.0f : 0.0f;
        for (int t0 = 0; t0 < wn.y; t0 += 4) {
          float wv[4], pv[4][4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const bool in = t0 + u < wn.y;
            const int t = in ? t0 + u : wn.y - 1;
            wv[u] = MASK ? 0.0f : w[t];
            if (!in) wv[u] = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) pv[u][q] = in || !MASK ? pixel<MASK>(row[q][so + t * C]) : 1.0f;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = tap<MASK>(acc[q], wv[u], pv[u][q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (rq + q < rh) inter[(rq + q) * TWC + j] = acc[q];
      }
    }
    __syncthreads();
    // ---- vertical pass and the one rounding: eight taps per sweep ----
    for (int oy = wave; oy < th; oy += kThreads / 64) {
      const int2 wn = wins_y[oy];
      const float* w = wy_s + oy * a.tmax_y;
      for (int j = lane; j < tw * C; j += 64) {
        const float* s = inter + (wn.x - ry0) * TWC + j;
        float acc = MASK ? 1.0f : 0.0f;
        for (int t0 = 0; t0 < wn.y; t0 += 8) {
          float wv[8], pv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const bool in = t0 + u < wn.y;
            const int t = in ? t0 + u : wn.y - 1;
            wv[u] = MASK ? 0.0f : w[t];
            if (!in) wv[u] = 0.0f;
            pv[u] = in || !MASK ? s[t * TWC] : 1.0f;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) acc = tap<MASK>(acc, wv[u], pv[u]);
        }
        out[(long)oy * a.Wo * C + j] = (uint8_t)fminf(fmaxf(rintf(acc), 0.0f), 255.0f);
      }
    }
    return;
  }

  // ---- direct form: the workgroup shares the taps of one output pixel (16 tap rows x 16 tap columns per sweep) ----
  for (int p = 0; p < th * tw; ++p) {
    const int oy = p / tw, ox = p - oy * tw;
    const int2 wy = wins_y[oy], wx = wins_x[ox];
    const uint8_t* g0 = a.src + (((long)f * a.Hs + a.y0 + wy.x) * a.Ws + a.x0 + wx.x) * C;
    float acc[3];
    for (int c = 0; c < 3; ++c) acc[c] = MASK ? 1.0f : 0.0f;
    for (int ky = tid >> 4; ky < wy.y; ky += 16) {
      const uint8_t* row = g0 + (long)ky * a.Ws * C;
      float h[3];
      for (int c = 0; c < 3; ++c) h[c] = MASK ? 1.0f : 0.0f;
      for (int kx = tid & 15; kx < wx.y; kx += 16) {
        const float w = MASK ? 0.0f : a.w_x[(long)(ox0 + ox) * a.tmax_x + kx];
        for (int c = 0; c < 3; ++c)
          if (c < C) h[c] = tap<MASK>(h[c], w, pixel<MASK>(row[kx * C + c]));
      }
      const float w = MASK ? 0.0f : a.w_y[(long)(oy0 + oy) * a.tmax_y + ky];
      for (int c = 0; c < 3; ++c) acc[c] = tap<MASK>(acc[c], w, h[c]);
    }
    for (int c = 0; c < 3; ++c) {
      acc[c] = MASK ? wave_min(acc[c]) : wave_sum(acc[c]);
      if (lane == 0) red[wave * 3 + c] = acc[c];
    }
    __syncthreads();
    if (tid < C) {
      float v = red[tid];
      for (int w = 1; w < kThreads / 64; ++w) v = MASK ? fminf(v, red[w * 3 + tid]) : v + red[w * 3 + tid];
      out[((long)oy * a.Wo + ox) * C + tid] = (uint8_t)fminf(fmaxf(rintf(v), 0.0f), 255.0f);
    }
    __syncthreads();
  }
}

// Footprint rows (columns) that `t` consecutive outputs of an axis can span: hi(i + t - 1) - lo(i) < (t - 1) scale + 2 support + 1.
int span_cap(int t, long n_in, long n_out, int half) {
  const double scale = (double)n_in / (double)n_out, support = scale >= 1.0 ? half * scale : (double)half;
  const double s = floor((t - 1) * scale + 2.0 * support + 1.0) + 1.0;
  return (int)fmin(s, (double)n_in);
}

long lds_bytes(int TH, int TW, int rh, int rw, int C, int tmax_y, int tmax_x) {
  return align16(kHeader + (long)(TH + TW) * 8) + align16((long)rh * row_pitch(rw, C)) + align16((long)rh * TW * C * 4) +
         align16((long)TW * tmax_x * 4) + align16((long)TH * tmax_y * 4);
}

// The largest tile of the list whose LDS leaves room for four workgroups per CU (40 of the 160 KiB: at 1080p and 2160p sources
// -> 480 x 720, budgets of 32 - 40 KiB measured fastest of 20 .. 160 for both filters and the mask; 80 KiB took 1.2x, 160 KiB
// 1.9x as long -- profiles/conform.txt), else the largest that fits one CU, else 1 x 1 with no staging room: every tile then
// takes the direct form.
void pick_tile(ResizeArgs& a, int half, long* smem) {
  static const int tiles[][2] = {{16, 64}, {8, 64}, {8, 32}, {4, 32}, {4, 16}, {2, 16}, {2, 8}, {1, 8}, {1, 4}, {1, 1}};
  const long budgets[2] = {40 * 1024, 160 * 1024};
  for (long budget : budgets)
    for (const auto& t : tiles) {
      const int rh = span_cap(t[0], a.hc, a.Ho, half), rw = span_cap(t[1], a.wc, a.Wo, half);
      const long need = lds_bytes(t[0], t[1], rh, rw, a.C, a.tmax_y, a.tmax_x);
      if (need <= budget) {
        a.TH = t[0]; a.TW = t[1]; a.rh_cap = rh; a.rw_cap = rw; *smem = need;
        return;
      }
    }
  a.TH = a.TW = 1; a.rh_cap = a.rw_cap = 0;
  *smem = lds_bytes(1, 1, 0, 0, a.C, 0, 0);
}

template <bool MASK>
int ld_conform_run(const char* name, ResizeArgs a, int64_t n_out, int filter, void* stream) {
  long smem = 0;
  pick_tile(a, filter == 0 ? 1 : 2, &smem);
  a.tiles_y = (a.Ho + a.TH - 1) / a.TH;
  a.tiles_x = (a.Wo + a.TW - 1) / a.TW;
  const long blocks = (long)a.tiles_y * a.tiles_x * n_out;
  LD_REQUIRE(blocks < (1L << 31), "%s: %ld destination tiles exceed one launch", name, blocks);
  static thread_local LdSmemCache cache{};
  if (int rc = ld_ensure_dyn_smem((const void*)ld_resize_kernel<MASK>, (size_t)smem, &cache)) return rc;
  hipLaunchKernelGGL(ld_resize_kernel<MASK>, dim3((unsigned)blocks), dim3(kThreads), (size_t)smem, (hipStream_t)stream, a);
  return ld_check_launch(name);
}

}  // namespace

// shapes arrive as int64 and are range-checked before they are narrowed
#define LD_CONFORM_SHAPES(name)                                                                                                 \
  LD_REQUIRE(Fs > 0 && Hs > 0 && Ws > 0 && n_out > 0 && Ho > 0 && Wo > 0 && hc > 0 && wc > 0, name ": empty shape");            \
  LD_REQUIRE(Fs < (1 << 30) && Hs < (1 << 30) && Ws < (1 << 30) && n_out < (1 << 30) && Ho < (1 << 30) && Wo < (1 << 30),       \
             name ": shape too large");                                                                                         \
  LD_REQUIRE(y0 >= 0 && x0 >= 0 && y0 + hc <= Hs && x0 + wc <= Ws, name ": the crop box (%lld, %lld, %lld, %lld) leaves the "   \
             "%lld x %lld source", (long long)y0, (long long)x0, (long long)hc, (long long)wc, (long long)Hs, (long long)Ws);   \
  LD_REQUIRE(frame_idx || n_out <= Fs, name ": without frame_idx n_out (%lld) must not exceed the source's %lld frames",        \
             (long long)n_out, (long long)Fs)

LD_API int ld_resize_u8(const uint8_t* src, uint8_t* dst, const int32_t* frame_idx, const int32_t* win_y, const float* w_y,
                        int64_t tmax_y, const int32_t* win_x, const float* w_x, int64_t tmax_x, int64_t Fs, int64_t Hs, int64_t Ws,
                        int64_t C, int64_t n_out, int64_t Ho, int64_t Wo, int64_t y0, int64_t x0, int64_t hc, int64_t wc,
                        int32_t filter, void* stream) {
  LD_REQUIRE(src && dst && win_y && w_y && win_x && w_x, "ld_resize_u8: null pointer");
  LD_REQUIRE(C == 1 || C == 3, "ld_resize_u8: C must be 1 or 3, got %lld", (long long)C);
  LD_CONFORM_SHAPES("ld_resize_u8");
  LD_REQUIRE(filter == 0 || filter == 1, "ld_resize_u8: unknown filter %d (0 = bilinear, 1 = bicubic)", (int)filter);
  LD_REQUIRE(tmax_y > 0 && tmax_x > 0 && tmax_y <= hc && tmax_x <= wc, "ld_resize_u8: a weight row holds between 1 and the box's "
             "size taps, got %lld and %lld", (long long)tmax_y, (long long)tmax_x);
  ResizeArgs a{src, dst, frame_idx, win_y, w_y, win_x, w_x, (int)Fs, (int)Hs, (int)Ws, (int)C, (int)Ho, (int)Wo, (int)y0, (int)x0,
               (int)hc, (int)wc, (int)tmax_y, (int)tmax_x, 0, 0, 0, 0, 0, 0};
  return ld_conform_run<false>("ld_resize_u8", a, n_out, filter, stream);
}

LD_API int ld_resize_mask_u8(const uint8_t* src, uint8_t* dst, const int32_t* frame_idx, const int32_t* win_y, const int32_t* win_x,
                             int64_t Fs, int64_t Hs, int64_t Ws, int64_t n_out, int64_t Ho, int64_t Wo, int64_t y0, int64_t x0,
                             int64_t hc, int64_t wc, int32_t filter, void* stream) {
  LD_REQUIRE(src && dst && win_y && win_x, "ld_resize_mask_u8: null pointer");
  LD_CONFORM_SHAPES("ld_resize_mask_u8");
  LD_REQUIRE(filter == 0 || filter == 1, "ld_resize_mask_u8: unknown filter %d (0 = bilinear, 1 = bicubic)", (int)filter);
  ResizeArgs a{src, dst, frame_idx, win_y, nullptr, win_x, nullptr, (int)Fs, (int)Hs, (int)Ws, 1, (int)Ho, (int)Wo, (int)y0, (int)x0,
               (int)hc, (int)wc, 0, 0, 0, 0, 0, 0, 0, 0};
  return ld_conform_run<true>("ld_resize_mask_u8", a, n_out, filter, stream);
}
