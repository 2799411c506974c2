"""Times the 3D-VAE encode of a 49-frame 480 x 720 clip (LanDiffPipeline.extend_video's clip window, full-width VAEEncoder on
synthetic weights) with device events after warm-up, and puts it against the bf16 MFMA peak.

Run:  python tools/vae_encode_time.py [--frames 49] [--reps 3] [--json out.json]
Kernel breakdown: rocprofv3 --kernel-trace --stats -- python tools/vae_encode_time.py --reps 1   (a run of its own)

FLOP: 2 M N K of every conv / GEMM as executed (conv_in's K with its 64 padded input channels, the space-to-depth downsample
convs' 3 x 3 taps over 4C channels, 36 of which carry the 9 real ones) and as useful (3 input channels, 3 x 3 stride-2 taps).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BF16 = 2.5e15          # MI355X dense bf16 MFMA peak, FLOP/s (MI355X_MICROARCH.md)


def encoder_flops(cfg, F: int, H: int, W: int):
    from landiff_amd.vae_encoder import IN_PAD
    from landiff_amd.weights import vae_encoder_levels
    executed = useful = 0.0
    T = F
    M = T * H * W
    executed += 2 * M * cfg.ch * 27 * IN_PAD
    useful += 2 * M * cfg.ch * 27 * 3
    def res(cin, cout, M):
        f = 2 * M * cout * 27 * cin + 2 * M * cout * 27 * cout + (2 * M * cout * cin if cin != cout else 0)
        return f
    C = cfg.ch
    for _, blocks, down in vae_encoder_levels(cfg):
        for cin, cout in blocks:
            f = res(cin, cout, T * H * W)
            executed += f; useful += f
            C = cout
        if down:
            if down == "space_time" and T > 1:
                T = (T + 1) // 2 if T % 2 else T // 2
            H, W = H // 2, W // 2
            executed += 2 * T * H * W * C * 9 * 4 * C     # 3 x 3 taps over 4C, 4 of 9 carry weights
            useful += 2 * T * H * W * C * 9 * C
    for _ in range(2):
        f = res(C, C, T * H * W)
        executed += f; useful += f
    f = 2 * T * H * W * 2 * cfg.z_channels * 27 * C
    return executed + f, useful + f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from landiff_amd.config import VAEConfig
    from landiff_amd.vae_encoder import VAEEncoder
    from landiff_amd.weights import init_state, vae_encoder_spec
    dev = torch.device("cuda:0")
    cfg = VAEConfig()
    enc = VAEEncoder(init_state(vae_encoder_spec(cfg), seed=5, device=dev), cfg, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    frames = torch.randint(0, 256, (a.frames, a.height, a.width, 3), generator=g, device=dev, dtype=torch.uint8)
    z = enc.encode(frames)                                      # warm-up: allocates and zero-fills the padded windows
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        z2 = enc.encode(frames)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    assert torch.equal(z, z2) and torch.isfinite(z).all()
    ex, us = encoder_flops(cfg, a.frames, a.height, a.width)
    best = min(times)
    res = {"frames": a.frames, "height": a.height, "width": a.width, "latent_shape": list(z.shape), "seconds": times,
           "best_s": best, "tflop_executed": ex / 1e12, "tflop_useful": us / 1e12,
           "tflops_executed": ex / best / 1e12, "share_of_bf16_peak": ex / best / PEAK_BF16,
           "workspace_gb": enc.workspace_bytes() / 1e9, "peak_alloc_gb": torch.cuda.max_memory_allocated(dev) / 1e9}
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
