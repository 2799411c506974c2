// Clip editing (LanDiffPipeline.edit_video): the sampler's masked re-noise / pin of known latents, and the reduction of a pixel
// keep-mask to the latent grid.
//
// Generalises the `sdedit` branch of VPSDEDPMPP2MSampler.__call__ (landiff/diffusion/sgm/modules/diffusionmodules/sampling.py:
// 800-835: `alpha_cumprod_sqrt[i] * prefix + randn * sqrt(1 - alpha_cumprod_sqrt[i]**2)` written over the first frames before
// every step) from "the first k frames" to any set of latent cells.  Both kernels are HBM-bound streaming passes.
#include "ld_common.h"
#include "../../include/landiff_hip.h"

namespace {

// x [T][C][H][W] f32 in place; mask [T][H][W] u8 broadcast over C (null: every element).  Where the mask is set
//   x = alpha*known + sigma*noise   (products rounded separately, then one rounded sum: eager torch's three ops)
// or, with noise null, x = known (a copy: no multiply, so -0.0 and NaN payloads pass through).  Elsewhere x is not written.
// noise may alias x: an element is read before it is written, by the thread that writes it.
__global__ void ld_latent_pin_kernel(float* x, const float* known, const float* noise, const uint8_t* mask, float alpha, float sigma,
                                     long C, long HW, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    if (mask) {
      const long t = i / (C * HW), hw = i % HW;
      if (!mask[t * HW + hw]) continue;
    }
    x[i] = noise ? __fadd_rn(__fmul_rn(alpha, known[i]), __fmul_rn(sigma, noise[i])) : known[i];
  }
}

// mask_px [F][Hp][Wp] u8 (non-zero = keep) -> out [T][Hp/8][Wp/8] u8 (1 = keep), T = (F + 3) / 4: a latent cell is kept only if
// every pixel of its block is -- frames {0} for t = 0 and {4t-3 .. 4t} for t >= 1 (the VAE's causal 1 + 4k frame mapping), rows
// 8i .. 8i+7, columns 8j .. 8j+7.  One thread per cell; a row of 8 pixels is one 8-byte load (Wp % 8 == 0 and an 8-byte aligned
// base make every row start aligned).
__global__ void ld_mask_to_latent_kernel(const uint8_t* mask_px, uint8_t* out, int T, int Hp, int Wp) {
  const int h = Hp / 8, w = Wp / 8;
  const long cells = (long)T * h * w;
  for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long)gridDim.x * blockDim.x) {
    const int j = (int)(c % w), i = (int)((c / w) % h), t = (int)(c / ((long)w * h));
    const int f0 = t == 0 ? 0 : 4 * t - 3, f1 = 4 * t;
    bool keep = true;
    for (int f = f0; f <= f1; ++f) {
      const uint8_t* row = mask_px + ((long)f * Hp + 8 * i) * Wp + 8 * j;
      for (int r = 0; r < 8; ++r) {
        const uint64_t v = *reinterpret_cast<const uint64_t*>(row + (long)r * Wp);
        keep = keep && !((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull);      // no zero byte among the eight
      }
    }
    out[c] = keep ? 1 : 0;
  }
}

inline dim3 grid_for(long total, int block = 256) {
  long b = (total + block - 1) / block;
  return dim3((unsigned)(b < 16384 ? (b > 0 ? b : 1) : 16384));
}

}  // namespace

LD_API int ld_latent_pin(float* x, const float* known, const float* noise, const uint8_t* mask, float alpha, float sigma,
                         int64_t T, int64_t C, int64_t H, int64_t W, void* stream) {
  LD_REQUIRE(x && known, "ld_latent_pin: null pointer");
  LD_REQUIRE(T > 0 && C > 0 && H > 0 && W > 0, "ld_latent_pin: empty shape");
  LD_REQUIRE(known != x, "ld_latent_pin: known must not alias x (noise may)");
  const long n = T * C * H * W;
  hipLaunchKernelGGL(ld_latent_pin_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, x, known, noise, mask, alpha, sigma,
                     (long)C, (long)(H * W), n);
  return ld_check_launch("ld_latent_pin");
}

LD_API int ld_mask_to_latent(const uint8_t* mask_px, uint8_t* out, int64_t F, int64_t Hp, int64_t Wp, void* stream) {
  LD_REQUIRE(mask_px && out, "ld_mask_to_latent: null pointer");
  LD_REQUIRE(F > 0 && Hp > 0 && Wp > 0, "ld_mask_to_latent: empty shape");
  LD_REQUIRE(F % 4 == 1, "ld_mask_to_latent: the frame count must be 4k + 1 (the VAE's causal 1 + 4k frame mapping)");
  LD_REQUIRE(Hp % 8 == 0 && Wp % 8 == 0, "ld_mask_to_latent: height and width must be multiples of 8");
  LD_REQUIRE((uintptr_t)mask_px % 8 == 0, "ld_mask_to_latent: mask_px must be 8-byte aligned");
  LD_REQUIRE(F < (1 << 30) && Hp < (1 << 30) && Wp < (1 << 30), "ld_mask_to_latent: mask too large");
  const long T = (F + 3) / 4;
  hipLaunchKernelGGL(ld_mask_to_latent_kernel, grid_for(T * (Hp / 8) * (Wp / 8)), dim3(256), 0, (hipStream_t)stream, mask_px, out,
                     (int)T, (int)Hp, (int)Wp);
  return ld_check_launch("ld_mask_to_latent");
}
