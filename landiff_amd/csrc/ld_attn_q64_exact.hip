// ld_attn_fwd_bf16_exact: the DiT attention with an exact safe softmax for ANY logit range, at a fixed ~1.55 x the cost of the headline
// launch -- for checkpoints whose q.k/8 row maxima leave the window of the max-free fast pass (beyond ~76; profiles/
// r06_attn_logit_sweep.txt), where the headline launch re-runs affected 256-row blocks through its running-max pass (up to 2.6 x).
// Same reference op (sat attention_fn_default -> F.scaled_dot_product_attention, landiff/diffusion/dit_video_concat.py:636-664), same
// tile, LDS images and pipelined loop as ld_attn_q64.hip (shared body: ld_attn_q64_body.h, Q64_EXACT): pass A computes every query
// row's maximum scaled score over all keys (QK^T MFMAs only), pass B is the fast pass's loop with -max as the initial value of the score
// accumulators, so the exponentials are 2^(s - max) <= 1 and no denominator can overflow or vanish.  No data-dependent branch, run to
// run identical.  One workgroup per query block, dealt by the hardware.
#include "ld_attn.h"
#include "ld_attn_dev.h"

namespace {

#include "ld_attn_q64_body.h"

__global__ __launch_bounds__(256, 2) void ld_attn_q64_exact_kernel(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  attn_q64_body<Q64_EXACT>(p, 0, smem, xcd_remap(blockIdx.x, gridDim.x));
}

}  // namespace

int ld_attn_q64_exact_launch(const AttnParams& p, hipStream_t st, AttnRan* ran) {
  static thread_local LdSmemCache cache{};
  const int total = (int)((long)p.B * p.H * ((p.Npad + Q64_ROWS - 1) / Q64_ROWS));
  return attn_launch(ld_attn_q64_exact_kernel, &cache, ATTN_SMEM_BYTES, dim3((unsigned)total), dim3(256), st, ran,
                     AttnRan{"ld_attn_q64_exact_kernel", nullptr, 0},          // a two-pass softmax: no window to leave
                     "ld_attn_fwd_bf16_exact(q64)", p);
}
