// Shared declarations of the gfx950 attention family.  ld_attn.hip: the plain online-softmax kernel, the plan (which kernel a
// problem gets, every LD_ATTN_* knob), the executor and the entry points.  The pipelined kernels and their launchers:
// ld_attn_q64.hip (64-row wave tile: dense, frame-window and dynamic forms; shared body ld_attn_q64_body.h), ld_attn_q64_exact.hip
// (two-pass exact softmax), ld_attn_p16.hip (32-row wave tile) and, in the variants build only, ld_attn_pipe.hip (round-1 pipeline)
// and ld_attn_q128.hip (128-row tile).  What the pipelined kernels share on the device -- LDS layout, the ring's LDS-DMA plan,
// fragment offsets, key indices, the window test and vote, the DMA drain, the O epilogue -- is stated once in ld_attn_dev.h; their
// launchers share attn_launch below.  A launcher takes its knob values as arguments -- it reads no environment -- and reports
// what it launched through an AttnRan; attn_run (ld_attn.hip) is the one writer of what ld_attn_last_kernel / _fallbacks answer.
#pragma once
#include "ld_common.h"
#include "../../include/landiff_hip.h"
#include <type_traits>

struct AttnParams {
  const bf16_t* Q;    // [BH][Npad][64]
  const bf16_t* K;    // [BH][Npad][64]
  const bf16_t* Vt;   // [BH][64][Npad]
  bf16_t* O;          // [B][Nq][H*64] (row stride o_rs, batch stride o_bs)
  int B, H, Nq, Nk, Npad;
  long o_bs, o_rs;
  float c;            // softmax_scale * log2(e)
  const int* fid_q;   // [Npad] or null
  const int* fid_k;   // [Npad] or null (padding keys must carry INT_MAX)
  const int* kt_min;  // [Npad/64]
  const int* kt_max;
};

// What a launcher launched.  name: the kernel, as ld_attn_last_kernel reports it.  Where the launch counts the query blocks that left
// the fast pass's window (ld_attn_last_fallbacks): fb_kind 0 = the kernel has no such window (running-max or two-pass softmax:
// nothing to count), 1 = counted at fb_src (device address, valid until the next launch on that stream), 2 = a max-free fast pass
// that keeps no count (static dispatch, 32-row tile).  Left untouched by a launcher that fails before its launch.
struct AttnRan {
  const char* name;
  const unsigned* fb_src;
  int fb_kind;
};

// The launchers.  safe != 0 forces the running-max pass; the other arguments are the knobs of the table at attn_plan.
// q64: win = null for the dense kernels, else {prefix, group, frames} of the frame-window form (validated by
// ld_attn_fwd_bf16_window); want_dyn asks for the dynamic form, which the launcher grants by device, grid, stream and capture.
int ld_attn_q64_launch(const AttnParams& p, hipStream_t st, const int* win, int safe, bool want_dyn, AttnRan* ran);
int ld_attn_q64_exact_launch(const AttnParams& p, hipStream_t st, AttnRan* ran);
int ld_attn_p16_launch(const AttnParams& p, hipStream_t st, int safe, int msum, int nw, AttnRan* ran);
#ifdef LD_VARIANTS   // measured alternatives, only in the variants build (build.sh: LD_BUILD_VARIANTS=1)
int ld_attn_pipe2_launch(const AttnParams& p, hipStream_t st, int safe, int nw, AttnRan* ran);
int ld_attn_q128_launch(const AttnParams& p, hipStream_t st, int safe, int npre, AttnRan* ran);
#endif

namespace {

constexpr int QB = 128;   // query rows per workgroup
constexpr int KT = 64;    // keys per tile
constexpr int D = 64;
constexpr int ATTN_PIPELINED_MIN_TILES = 6;   // unmasked problems of at least this many key tiles take the pipelined kernels, whose loops count on it
constexpr int KTILE_BYTES = KT * D * 2;       // 8 KB
constexpr int STAGE_BYTES = 2 * KTILE_BYTES;  // K + V^T
constexpr float NEG_BIG = -1.0e30f;


// Frame-window attention (ld_attn_fwd_bf16_window): the key tiles that 256-row query block `b` of a sequence
// [P prefix keys | frames of G tokens ...] of N tokens walks with a window of w frames each side -- the logical list
// 0 .. pt-1, t_lo .. t_hi-1 (pt = ceil(P / 64)), n_eff tiles long.  A block that holds a prefix row walks every tile (t_lo = pt,
// t_hi = n).  The ONE statement of the rule: the kernels derive their tile list from it, the launcher validates with it and
// ld_attn_window_plan reports it.  int arithmetic: the host clamps G to N and w to the frame count first (attn_window_clamp),
// which changes no result and keeps (f_hi + w + 1) * G below 2^31 for N < 2^28.
__host__ __device__ inline void attn_window_block(int N, int P, int G, int w, int b, int* t_lo, int* t_hi, int* n_eff) {
  const int n = (N + 63) / 64, pt = (P + 63) / 64;
  const int r0 = 256 * b, r1 = (r0 + 256 < N ? r0 + 256 : N) - 1;
  int lo = pt, hi = n;
  if (r0 >= P) {
    const int f_lo = (r0 - P) / G, f_hi = (r1 - P) / G;
    const int k_lo = P + (f_lo > w ? f_lo - w : 0) * G;
    int k_hi = P + (f_hi + w + 1) * G;
    k_hi = k_hi < N ? k_hi : N;
    lo = k_lo / 64 > pt ? k_lo / 64 : pt;
    hi = (k_hi + 63) / 64;
  }
  *t_lo = lo; *t_hi = hi; *n_eff = pt + hi - lo;
}

// G >= N is one frame and w >= the frame count is every frame: clamp both (same plan, no overflow in attn_window_block)
inline void attn_window_clamp(int64_t N, int64_t P, int64_t* G, int64_t* w) {
  if (*G > N) *G = N;
  const int64_t frames = P < N ? (N - P + *G - 1) / *G : 0;
  if (*w > frames) *w = frames;
}

// What a launch without a fallback count reports.  name / name_safe: the kernel and the kernel "[safe pass forced]" (ATTN_KNAMES
// writes the pair, so the suffix rule stands here alone); a forced safe pass has no window to leave (fb_kind 0), a fast pass of a
// static launch has one and keeps no count (fb_kind 2).
#define ATTN_KNAMES(kernel) #kernel, #kernel "[safe pass forced]"
inline AttnRan attn_ran_static(const char* name, const char* name_safe, int safe) {
  return AttnRan{safe ? name_safe : name, nullptr, safe ? 0 : 2};
}

// The launch of a pipelined kernel: its dynamic shared memory (cache: the kernel's own `static thread_local` LdSmemCache), what it
// reports, the launch.  *ran is written only once nothing before the launch can fail any more.
template <class Kernel, class... Args>
int attn_launch(Kernel kernel, LdSmemCache* cache, size_t smem, dim3 grid, dim3 block, hipStream_t st, AttnRan* ran, const AttnRan& what_ran,
                const char* what, Args... args) {
  if (int rc = ld_ensure_dyn_smem((const void*)kernel, smem, cache)) return rc;
  *ran = what_ran;
  hipLaunchKernelGGL(kernel, grid, block, smem, st, args...);
  return ld_check_launch(what);
}

__device__ __forceinline__ float lane32_max(float x) {
  // max(x, value of lane^32)
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float lane32_sum(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

__device__ __forceinline__ int swap23(int i) {
  return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1);
}

}  // namespace
