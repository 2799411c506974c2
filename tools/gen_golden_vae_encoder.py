"""Writes tests/golden/vae_encoder_fp32.npz from the REFERENCE's own 3D-VAE encoder (test infrastructure, like
oracle/gen_golden.py, whose stubs and save() it imports unchanged; needs the reference checkout, never runs on the GPU box).

Run:  python tools/gen_golden_vae_encoder.py

ContextParallelEncoder3D (cp_enc_dec.py:785-911) at VAEConfig.tiny() on init_state(vae_encoder_spec) weights (seed stored),
fp32 on CPU, one rank; a 9-frame and an 8-frame 32 x 48 clip (odd T: first-frame split of the time pool, even T: plain
pairs).  Per clip: the uint8 frames, the encoder input x / 127.5 - 1, mean and clamped logvar of DiagonalGaussianDistribution
(regularizers.py:10-28), and a seeded posterior.sample() * scale_factor (encode_first_stage, diffusion_video.py:233-254) with
the eps its randn_like drew.  Plus the encoder's state-dict key list.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden  # noqa: E402

WEIGHT_SEED = 21
CLIPS = {"odd": (9, 101), "even": (8, 102)}        # name -> (frames, seed of the pixels)
SAMPLE_SEED = 7


def main():
    gen_golden.install_stubs()
    import torch.distributed as dist
    from landiff.diffusion.sgm.util import initialize_context_parallel
    from landiff.diffusion.vae_modules.cp_enc_dec import ContextParallelEncoder3D
    from landiff.diffusion.vae_modules.regularizers import DiagonalGaussianDistribution, DiagonalGaussianRegularizer
    from landiff_amd.config import VAEConfig
    from landiff_amd.weights import init_state, vae_encoder_spec

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        dist.init_process_group("gloo", rank=0, world_size=1)
    initialize_context_parallel(1)
    cfg = VAEConfig.tiny()
    enc = ContextParallelEncoder3D(double_z=True, z_channels=cfg.z_channels, resolution=256, in_channels=3, out_ch=3, ch=cfg.ch,
                                   ch_mult=list(cfg.ch_mult), attn_resolutions=[], num_res_blocks=cfg.num_res_blocks,
                                   dropout=0.0, gather_norm=False, temporal_compress_times=cfg.temporal_compress_times)
    sd = init_state(vae_encoder_spec(cfg), seed=WEIGHT_SEED)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items()}, strict=True)
    enc.eval()
    out = {"weight_seed": np.array(WEIGHT_SEED), "scale_factor": np.array(cfg.scale_factor),
           "keys": np.array(sorted("encoder." + k for k in enc.state_dict().keys()))}
    reg = DiagonalGaussianRegularizer(sample=True)
    for name, (F, seed) in CLIPS.items():
        g = torch.Generator().manual_seed(seed)
        frames = torch.randint(0, 256, (F, 32, 48, 3), generator=g, dtype=torch.uint8)
        x = frames.float() / 127.5 - 1.0                                  # [F, H, W, 3]
        with torch.no_grad():
            moments = enc(x.permute(3, 0, 1, 2).unsqueeze(0).contiguous())   # [1, 32, T, h, w]
            post = DiagonalGaussianDistribution(moments)
            torch.manual_seed(SAMPLE_SEED)
            eps = torch.randn_like(post.mean)
            torch.manual_seed(SAMPLE_SEED)
            z, _ = reg(moments)
        assert torch.allclose(z, post.mean + post.std * eps)
        out.update({f"{name}_frames": frames.numpy(), f"{name}_x": x.numpy(), f"{name}_mean": post.mean.numpy(),
                    f"{name}_logvar": post.logvar.numpy(), f"{name}_eps": eps.numpy(),
                    f"{name}_sample": (cfg.scale_factor * z).numpy()})
    gen_golden.save("vae_encoder_fp32", **out)


if __name__ == "__main__":
    main()
