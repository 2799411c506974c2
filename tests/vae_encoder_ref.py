"""Plain-torch restatement of the CogVideoX 3D-VAE encoder (ContextParallelEncoder3D, cp_enc_dec.py:785-911, one rank, no
cache) + its posterior (regularizers.py:10-28), for the encoder tests (test helper, not part of the package).

Channels-last [T, H, W, C] activations; every convolution is a sum of per-tap matrix products (no cuDNN / MIOpen kernels, so it
runs alike on CPU and GPU); `dtype` is the storage and matmul dtype of activations and weights (float32: the reference's
arithmetic up to summation order; bfloat16: the noise floor of a bf16 implementation), GroupNorm statistics in fp32.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from landiff_amd.weights import vae_encoder_levels


def _causal_conv(x, w, b, dtype):
    """3x3x3 causal conv: time halo = two copies of frame 0, spatial zero pad 1 (ContextParallelCausalConv3d, :416-473)."""
    T, H, W, C = x.shape
    Co = w.shape[0]
    xp = F.pad(torch.cat([x[:1], x[:1], x], 0), (0, 0, 1, 1, 1, 1))
    w = w.to(dtype)
    out = torch.zeros(T * H * W, Co, device=x.device, dtype=torch.float32)
    for dt in range(3):
        for dh in range(3):
            for dw in range(3):
                a = xp[dt:dt + T, dh:dh + H, dw:dw + W].reshape(-1, C)
                out += (a @ w[:, :, dt, dh, dw].t()).float()
    return (out + b.float()).to(dtype).reshape(T, H, W, Co)


def _group_norm_swish(x, g, b, groups=32, eps=1e-6, swish=True):
    T, H, W, C = x.shape
    xf = x.float().reshape(-1, groups, C // groups)
    mean = xf.mean(dim=(0, 2), keepdim=True)
    var = xf.var(dim=(0, 2), unbiased=False, keepdim=True)
    y = ((xf - mean) / torch.sqrt(var + eps)).reshape(T, H, W, C) * g.float() + b.float()
    if swish:
        y = y * torch.sigmoid(y)
    return y.to(x.dtype)


def _resblock(x, sd, p, cin, cout, dtype):
    h = _group_norm_swish(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
    h = _causal_conv(h, sd[p + "conv1.conv.weight"], sd[p + "conv1.conv.bias"], dtype)
    h = _group_norm_swish(h, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
    h = _causal_conv(h, sd[p + "conv2.conv.weight"], sd[p + "conv2.conv.bias"], dtype)
    if cin != cout:
        wn = sd[p + "nin_shortcut.weight"].reshape(cout, cin).to(dtype)
        x = ((x.reshape(-1, cin) @ wn.t()).float() + sd[p + "nin_shortcut.bias"].float()).to(dtype).reshape(*x.shape[:3], cout)
    return (x.float() + h.float()).to(dtype)


def time_pool(x):
    """DownSample3D's time compression (cp_enc_dec.py:647-664) on [T, H, W, C]: frame 0 kept + pairs (odd T), pairs (even T);
    mean of two values in fp32, stored in x's dtype."""
    T = x.shape[0]
    if T == 1:
        return x
    first, rest = (x[:1], x[1:]) if T % 2 else (x[:0], x)
    pooled = ((rest[0::2].float() + rest[1::2].float()) * 0.5).to(x.dtype)
    return torch.cat([first, pooled], 0)


def _downsample(x, w, b, compress_time, dtype):
    """DownSample3D: [time pool], pad (0, 1, 0, 1), 3x3 stride-2 Conv2d per frame (:634-681), as per-tap matrix products."""
    if compress_time:
        x = time_pool(x)
    T, H, W, C = x.shape
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    xp = F.pad(x, (0, 0, 0, 1, 0, 1))
    w = w.to(dtype)
    out = torch.zeros(T * Ho * Wo, w.shape[0], device=x.device, dtype=torch.float32)
    for dh in range(3):
        for dw in range(3):
            a = xp[:, dh:dh + 2 * Ho - 1:2, dw:dw + 2 * Wo - 1:2].reshape(-1, C)
            out += (a @ w[:, :, dh, dw].t()).float()
    return (out + b.float()).to(dtype).reshape(T, Ho, Wo, -1)


@torch.no_grad()
def encode_moments_ref(sd: dict, cfg, x: torch.Tensor, dtype=torch.float32):
    """x [F, H, W, 3] in [-1, 1] -> (mean, clamped logvar), each [1, Z, T', H/8, W/8] fp32 (the reference's layout)."""
    sd = {k: v.to(x.device) for k, v in sd.items()}
    p = "encoder."
    h = _causal_conv(x.to(dtype), sd[p + "conv_in.conv.weight"], sd[p + "conv_in.conv.bias"], dtype)
    C = cfg.ch
    for lvl, blocks, down in vae_encoder_levels(cfg):
        for j, (cin, cout) in enumerate(blocks):
            h = _resblock(h, sd, p + f"down.{lvl}.block.{j}.", cin, cout, dtype)
            C = cout
        if down:
            h = _downsample(h, sd[p + f"down.{lvl}.downsample.conv.weight"], sd[p + f"down.{lvl}.downsample.conv.bias"],
                            down == "space_time", dtype)
    h = _resblock(h, sd, p + "mid.block_1.", C, C, dtype)
    h = _resblock(h, sd, p + "mid.block_2.", C, C, dtype)
    h = _group_norm_swish(h, sd[p + "norm_out.weight"], sd[p + "norm_out.bias"])
    m = _causal_conv(h, sd[p + "conv_out.conv.weight"], sd[p + "conv_out.conv.bias"], dtype).float()
    m = m.permute(3, 0, 1, 2).unsqueeze(0)                 # [1, 2Z, T, h, w]
    Z = cfg.z_channels
    return m[:, :Z].contiguous(), m[:, Z:].clamp(-30.0, 20.0).contiguous()


def space_to_depth(x: torch.Tensor) -> torch.Tensor:
    """[..., H, W, C] -> [..., H/2+2, W/2+2, 4C] with out[a, b, (2p+q)C + c] = x[2a+p, 2b+q, c], zero outside (the layout
    ld_vae_enc_downsample writes)."""
    *lead, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 0, 4, 0, 4))                       # [.., H+4, W+4, C]
    y = xp.reshape(*lead, H // 2 + 2, 2, W // 2 + 2, 2, C)  # [.., a, p, b, q, c]
    n = len(lead)
    y = y.permute(*range(n), n, n + 2, n + 1, n + 3, n + 4)
    return y.reshape(*lead, H // 2 + 2, W // 2 + 2, 4 * C)
