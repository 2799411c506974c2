// CogVideoX 3D-VAE ENCODER: the three kernels that are not the decoder's building blocks run backwards.
//   ld_vae_enc_place_input  frames -> the zero-bordered, time-haloed, channel-padded input of conv_in
//   ld_vae_enc_downsample   DownSample3D's time pool + the space-to-depth layout its stride-2 conv runs on as a stride-1 conv
//   ld_vae_posterior        DiagonalGaussianRegularizer: mean / clamped logvar, mode or reparameterised sample, * scale_factor
// The convolutions, GroupNorms and residual adds are ld_conv_cl_bf16[_gn] / ld_groupnorm_* unchanged (landiff_amd/vae_encoder.py).
#include "ld_common.h"
#include "../../include/landiff_hip.h"

namespace {

inline dim3 grid_for(long total, int block = 256) {
  long b = (total + block - 1) / block;
  return dim3((unsigned)(b < 16384 ? (b > 0 ? b : 1) : 16384));
}

// out [F+2][H+2][W+2][Cpad]: every element written (border / padding channels zero), frames 0 and 1 = frame 0 (the causal halo
// of _fake_cp_pass_from_previous_rank without a cache, cp_enc_dec.py:249-300).  One thread per 8-channel chunk.
__global__ void ld_vae_enc_place_input_kernel(const void* in, int in_u8, bf16_t* out, int F, int H, int W, int Cpad) {
  const int chunks = Cpad >> 3;
  const long total = (long)(F + 2) * (H + 2) * (W + 2) * chunks;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % chunks);
    long r = i / chunks;
    const int w = (int)(r % (W + 2)); r /= (W + 2);
    const int h = (int)(r % (H + 2));
    const int t = (int)(r / (H + 2));
    float v[3] = {0.f, 0.f, 0.f};
    if (ch == 0 && h >= 1 && h <= H && w >= 1 && w <= W) {
      const int f = t < 2 ? 0 : t - 2;
      const long src = (((long)f * H + (h - 1)) * W + (w - 1)) * 3;
      for (int c = 0; c < 3; ++c)
        v[c] = in_u8 ? ((const uint8_t*)in)[src + c] / 127.5f - 1.0f : ((const float*)in)[src + c];
    }
    u32x4_t o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], 0.f), 0u, 0u};
    *(u32x4_t*)(out + i * 8) = o;
  }
}

// in [T][H][W][C] -> out [To][H/2+2][W/2+2][4C], out[t][a][b][(2p+q)C + c] = x'[t][2a+p][2b+q][c] (0 outside H x W) where x' is
// the time-pooled input: frame 0 kept and later frames averaged in pairs for odd T, plain pairs for even T (DownSample3D,
// cp_enc_dec.py:647-664; fp32 mean of two bf16 values, rounded once), or x itself.
__global__ void ld_vae_enc_downsample_kernel(const bf16_t* in, bf16_t* out, int T, int H, int W, int C, int To, int pool) {
  const int Ha = H / 2 + 2, Wb = W / 2 + 2, cch = C >> 3;
  const long total = (long)To * Ha * Wb * 4 * cch;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % cch);
    long r = i / cch;
    const int pq = (int)(r % 4); r /= 4;
    const int b = (int)(r % Wb); r /= Wb;
    const int a = (int)(r % Ha);
    const int t = (int)(r / Ha);
    const int h = 2 * a + (pq >> 1), w = 2 * b + (pq & 1);
    u32x4_t o = {0u, 0u, 0u, 0u};
    if (h < H && w < W) {
      int t0 = t, t1 = -1;
      if (pool) {
        if (T & 1) { if (t > 0) { t0 = 2 * t - 1; t1 = 2 * t; } }
        else { t0 = 2 * t; t1 = 2 * t + 1; }
      }
      const long pix = ((long)h * W + w) * C + ch * 8;
      const u32x4_t x0 = *(const u32x4_t*)(in + (long)t0 * H * W * C + pix);
      if (t1 < 0) {
        o = x0;
      } else {
        const u32x4_t x1 = *(const u32x4_t*)(in + (long)t1 * H * W * C + pix);
        for (int e = 0; e < 4; ++e)
          o[e] = pack_bf16x2((bf_lo(x0[e]) + bf_lo(x1[e])) * 0.5f, (bf_hi(x0[e]) + bf_hi(x1[e])) * 0.5f);
      }
    }
    *(u32x4_t*)(out + i * 8) = o;
  }
}

// x [T*H*W][ldx] f32 (conv_out: mean = channels [0, Z), logvar = [Z, 2Z)) -> z [T][Z][H][W] f32; eps [Z][T][H][W] f32
// (torch.randn_like of the reference's [1, Z, T, H, W] mean) or null (mode).
__global__ void ld_vae_posterior_kernel(const float* x, long ldx, const float* eps, float* z, float* mean, float* logvar,
                                        int T, int Z, int H, int W, float scale) {
  const long total = (long)T * Z * H * W;
  const long HW = (long)H * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long hw = i % HW;
    const int c = (int)((i / HW) % Z);
    const int t = (int)(i / (HW * Z));
    const long row = (long)t * HW + hw;
    const float m = x[row * ldx + c];
    const float lv = fminf(fmaxf(x[row * ldx + Z + c], -30.0f), 20.0f);
    float v = m;
    if (eps) {
      const float s = expf(0.5f * lv);
      v = m + s * eps[((long)c * T + t) * HW + hw];
    }
    z[i] = scale * v;
    if (mean) mean[i] = m;
    if (logvar) logvar[i] = lv;
  }
}

}  // namespace

LD_API int ld_vae_enc_place_input(const void* frames, int32_t frames_u8, void* out_padded, int64_t F, int64_t H, int64_t W,
                                  int64_t Cpad, void* stream) {
  LD_REQUIRE(frames && out_padded && F > 0 && H > 0 && W > 0, "ld_vae_enc_place_input: bad args");
  LD_REQUIRE(Cpad >= 8 && Cpad % 8 == 0, "ld_vae_enc_place_input: Cpad must be a multiple of 8");
  const long total = (F + 2) * (H + 2) * (W + 2) * (Cpad / 8);
  hipLaunchKernelGGL(ld_vae_enc_place_input_kernel, grid_for(total), dim3(256), 0, (hipStream_t)stream, frames, (int)frames_u8,
                     (bf16_t*)out_padded, (int)F, (int)H, (int)W, (int)Cpad);
  return ld_check_launch("ld_vae_enc_place_input");
}

LD_API int ld_vae_enc_downsample(const void* in, void* out, int64_t T, int64_t H, int64_t W, int64_t C, int32_t compress_time,
                                 void* stream) {
  LD_REQUIRE(in && out && T > 0 && H > 0 && W > 0, "ld_vae_enc_downsample: bad args");
  LD_REQUIRE(C % 8 == 0 && H % 2 == 0 && W % 2 == 0, "ld_vae_enc_downsample: C %% 8, H and W even");
  const int pool = compress_time && T > 1;
  const long To = pool ? ((T & 1) ? 1 + (T - 1) / 2 : T / 2) : T;
  const long total = To * (H / 2 + 2) * (W / 2 + 2) * 4 * (C / 8);
  hipLaunchKernelGGL(ld_vae_enc_downsample_kernel, grid_for(total), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)in,
                     (bf16_t*)out, (int)T, (int)H, (int)W, (int)C, (int)To, pool);
  return ld_check_launch("ld_vae_enc_downsample");
}

LD_API int ld_vae_posterior(const float* x, int64_t ldx, const float* eps, float* z, float* mean, float* logvar, int64_t T,
                            int64_t Z, int64_t H, int64_t W, float scale, void* stream) {
  LD_REQUIRE(x && z && T > 0 && Z > 0 && H > 0 && W > 0 && ldx >= 2 * Z, "ld_vae_posterior: bad args");
  hipLaunchKernelGGL(ld_vae_posterior_kernel, grid_for(T * Z * H * W), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, eps, z,
                     mean, logvar, (int)T, (int)Z, (int)H, (int)W, scale);
  return ld_check_launch("ld_vae_posterior");
}
