"""Times the Theia extraction of a 13-frame 480 x 720 clip (the tokenizer's temporal size; frames padded to 720 x 720 by the first
kernel: 45 x 45 patches + CLS = 2026 tokens per frame) on DeiT-base-shaped random weights, with device events after warm-up, and
puts it against the bf16 MFMA peak.

Run:  python tools/theia_time.py [--frames 13] [--reps 5] [--json out.json]
Kernel breakdown: rocprofv3 --kernel-trace --stats -- python tools/theia_time.py --reps 1   (a run of its own)

FLOP: 2 M N K of every GEMM (patch Conv2d, q|k|v, output, MLP in / out) + 4 N^2 d per head and frame for QK^T and PV.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BF16 = 2.5e15          # MI355X dense bf16 MFMA peak, FLOP/s (MI355X_MICROARCH.md)


def deit_base_state(seed: int = 0, width: int = 768, layers: int = 12) -> dict:
    """Random tensors under the keys landiff_amd.theia reads, at DeiT-base shapes."""
    from landiff_amd.theia import theia_keys
    g = torch.Generator().manual_seed(seed)
    shapes = {"embeddings.cls_token": (1, 1, width), "embeddings.position_embeddings": (1, 197, width),
              "embeddings.patch_embeddings.projection.weight": (width, 3, 16, 16)}
    st = {}
    for k in theia_keys(layers):
        if k in shapes:
            sh = shapes[k]
        elif "intermediate.dense.weight" in k:
            sh = (4 * width, width)
        elif "intermediate.dense.bias" in k:
            sh = (4 * width,)
        elif "output.dense.weight" in k and "attention" not in k:
            sh = (width, 4 * width)
        elif k.endswith(".weight") and "layernorm" not in k:
            sh = (width, width)
        else:
            sh = (width,)
        t = torch.randn(sh, generator=g)
        if "layernorm" in k and k.endswith("weight"):
            t = 1.0 + 0.1 * t
        elif len(sh) >= 2 and "embeddings.c" not in k and "position" not in k:
            t = t / (t[0].numel() ** 0.5)
        else:
            t = 0.05 * t
        st[k] = t
    return st


def flops(T: int, s: int, width: int = 768, layers: int = 12) -> float:
    P, N = s * s, s * s + 1
    f = 2.0 * T * P * width * 768
    per_layer = 2.0 * T * N * width * (3 * width + width + 8 * width) + 4.0 * T * (width // 64) * N * N * 64
    return f + layers * per_layer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=13)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from landiff_amd.theia import TheiaExtractor
    dev = torch.device("cuda:0")
    ext = TheiaExtractor(deit_base_state(), dev)
    g = torch.Generator(device=dev).manual_seed(1)
    frames = torch.randint(0, 256, (a.frames, 480, 720, 3), generator=g, device=dev, dtype=torch.uint8)
    sq = torch.full((a.frames, 3, 720, 720), 127, dtype=torch.uint8, device=dev)
    sq[:, :, :480] = frames.permute(0, 3, 1, 2)
    ext(sq)                                                          # warm-up (position table, first launches)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ext(sq)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    best, med = min(times), sorted(times)[len(times) // 2]
    fl = flops(a.frames, 45)
    res = dict(frames=a.frames, size="480x720 -> 720x720", tokens_per_frame=2026, seconds_best=best, seconds_median=med,
               tflop=fl / 1e12, tflops_best=fl / best / 1e12, peak_share=fl / best / PEAK_BF16)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
