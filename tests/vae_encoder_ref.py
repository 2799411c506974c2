"""Plain-torch restatement of the CogVideoX 3D-VAE encoder (ContextParallelEncoder3D, cp_enc_dec.py:785-911, one rank, no
cache) + its posterior (regularizers.py:10-28), for the encoder tests (test helper, not part of the package).

Channels-last [T, H, W, C] activations; every convolution is a sum of per-tap matrix products (no cuDNN / MIOpen kernels, so it
runs alike on CPU and GPU); `dtype` is the storage and matmul dtype of activations and weights (float32: the reference's
arithmetic up to summation order; bfloat16: the noise floor of a bf16 implementation), GroupNorm statistics in fp32.

Sliced mode (encode_moments_ref(..., slice_frames=S)): every activation is a list of S-frame pieces, so that no tensor reaches
2^31 elements (a 49-frame 480 x 720 clip's level-0 activation is 2.2e9) and nothing relies on torch / rocBLAS handling such
tensors.  Causal convs and the downsample run per piece with their halo frames, GroupNorm statistics are summed in float64
over the pieces and applied per piece.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from landiff_amd.weights import vae_encoder_levels


def _causal_conv(x, w, b, dtype):
    """3x3x3 causal conv: time halo = two copies of frame 0, spatial zero pad 1 (ContextParallelCausalConv3d, :416-473)."""
    return _conv_window(torch.cat([x[:1], x[:1], x], 0), w, b, dtype)


def _conv_window(xw, w, b, dtype):
    """3x3x3 conv over frames that already carry their two halo frames in front: xw [T+2, H, W, C] -> [T, H, W, Co]."""
    T, H, W, C = xw.shape
    T -= 2
    Co = w.shape[0]
    xp = F.pad(xw, (0, 0, 1, 1, 1, 1))
    w = w.to(dtype)
    out = torch.zeros(T * H * W, Co, device=xw.device, dtype=torch.float32)
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
    return (_shortcut(x, sd, p, cin, cout, dtype).float() + h.float()).to(dtype)


def _shortcut(x, sd, p, cin, cout, dtype):
    if cin == cout:
        return x
    wn = sd[p + "nin_shortcut.weight"].reshape(cout, cin).to(dtype)
    return ((x.reshape(-1, cin) @ wn.t()).float() + sd[p + "nin_shortcut.bias"].float()).to(dtype).reshape(*x.shape[:3], cout)


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


# ---- sliced mode: an activation is a list of pieces of S frames each (the last one may be shorter) ----
def _frames(hs, idx):
    """Frames idx of a sliced activation, stacked; indices below 0 give frame 0 (the causal time halo)."""
    S = hs[0].shape[0]
    return torch.stack([hs[max(t, 0) // S][max(t, 0) % S] for t in idx])


def _causal_conv_sliced(hs, w, b, dtype):
    out, t0 = [], 0
    for h in hs:
        out.append(_conv_window(torch.cat([_frames(hs, [t0 - 2, t0 - 1]), h], 0), w, b, dtype))
        t0 += h.shape[0]
    return out


def _group_norm_swish_sliced(hs, g, b, groups=32, eps=1e-6, swish=True):
    C = hs[0].shape[-1]
    s = torch.zeros(groups, dtype=torch.float64, device=hs[0].device)
    ss, n = torch.zeros_like(s), 0
    for h in hs:
        xd = h.double().reshape(-1, groups, C // groups)
        s += xd.sum(dim=(0, 2)); ss += (xd * xd).sum(dim=(0, 2)); n += xd.shape[0] * xd.shape[2]
        del xd
    mean = s / n
    var = (ss / n - mean * mean).clamp_min(0)
    mean, rstd = mean.float()[:, None], torch.rsqrt(var + eps).float()[:, None]
    out = []
    for h in hs:
        T, H, W, _ = h.shape
        y = ((h.float().reshape(-1, groups, C // groups) - mean) * rstd).reshape(T, H, W, C) * g.float() + b.float()
        if swish:
            y = y * torch.sigmoid(y)
        out.append(y.to(h.dtype))
    return out


def _resblock_sliced(xs, sd, p, cin, cout, dtype):
    h = _group_norm_swish_sliced(xs, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
    h = _causal_conv_sliced(h, sd[p + "conv1.conv.weight"], sd[p + "conv1.conv.bias"], dtype)
    h = _group_norm_swish_sliced(h, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
    h = _causal_conv_sliced(h, sd[p + "conv2.conv.weight"], sd[p + "conv2.conv.bias"], dtype)
    return [(_shortcut(x, sd, p, cin, cout, dtype).float() + hh.float()).to(dtype) for x, hh in zip(xs, h)]


def _downsample_sliced(hs, w, b, compress_time, dtype):
    """DownSample3D per S output frames: each output frame gathers its one or two source frames (time_pool's pairing)."""
    S, T = hs[0].shape[0], sum(h.shape[0] for h in hs)
    pool = compress_time and T > 1
    To = ((T + 1) // 2 if T % 2 else T // 2) if pool else T
    out = []
    for j0 in range(0, To, S):
        frames = []
        for j in range(j0, min(j0 + S, To)):
            if not pool:
                frames.append(_frames(hs, [j])[0])
            elif T % 2 and j == 0:
                frames.append(_frames(hs, [0])[0])
            else:
                a, c = _frames(hs, [2 * j - 1, 2 * j] if T % 2 else [2 * j, 2 * j + 1])
                frames.append(((a.float() + c.float()) * 0.5).to(a.dtype))
        out.append(_downsample(torch.stack(frames), w, b, False, dtype))
    return out


def _encode_sliced(sd, cfg, x, dtype, S):
    p = "encoder."
    h = _causal_conv_sliced(list(x.to(dtype).split(S)), sd[p + "conv_in.conv.weight"], sd[p + "conv_in.conv.bias"], dtype)
    C = cfg.ch
    for lvl, blocks, down in vae_encoder_levels(cfg):
        for j, (cin, cout) in enumerate(blocks):
            h = _resblock_sliced(h, sd, p + f"down.{lvl}.block.{j}.", cin, cout, dtype)
            C = cout
        if down:
            h = _downsample_sliced(h, sd[p + f"down.{lvl}.downsample.conv.weight"], sd[p + f"down.{lvl}.downsample.conv.bias"],
                                   down == "space_time", dtype)
    h = _resblock_sliced(h, sd, p + "mid.block_1.", C, C, dtype)
    h = _resblock_sliced(h, sd, p + "mid.block_2.", C, C, dtype)
    h = _group_norm_swish_sliced(h, sd[p + "norm_out.weight"], sd[p + "norm_out.bias"])
    return torch.cat(_causal_conv_sliced(h, sd[p + "conv_out.conv.weight"], sd[p + "conv_out.conv.bias"], dtype), 0).float()


@torch.no_grad()
def encode_moments_ref(sd: dict, cfg, x: torch.Tensor, dtype=torch.float32, slice_frames: int | None = None):
    """x [F, H, W, 3] in [-1, 1] -> (mean, clamped logvar), each [1, Z, T', H/8, W/8] fp32 (the reference's layout).
    slice_frames: run in the sliced mode, on pieces of that many frames."""
    sd = {k: v.to(x.device) for k, v in sd.items()}
    if slice_frames:
        return _moments(_encode_sliced(sd, cfg, x, dtype, slice_frames), cfg)
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
    return _moments(_causal_conv(h, sd[p + "conv_out.conv.weight"], sd[p + "conv_out.conv.bias"], dtype).float(), cfg)


def _moments(m, cfg):
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
