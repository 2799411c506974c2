"""CogVideoX 3D-VAE encode on MI355X: pixels -> the latent the sampler pins as a continuation prefix.

Mirrors SATVideoDiffusionEngine.encode_first_stage (landiff/diffusion/diffusion_video.py:233-254: scale_factor * encode(x))
-> VideoAutoencoderInferenceWrapper.encode (vae_modules/autoencoder.py:218-230,626-656) -> ContextParallelEncoder3D.forward
(vae_modules/cp_enc_dec.py:785-911) + DiagonalGaussianRegularizer (vae_modules/regularizers.py:10-28,96-114), on one rank and
without the conv caches: the whole clip is ONE encoder call, so every GroupNorm takes its statistics over the whole clip, as
the reference's does.

The decoder's building blocks run in the other order (landiff_amd/vae.py): causal 3x3x3 convs on zero-bordered channels-last
windows [T+2][H+2][W+2][C] whose two halo frames are copies of the first frame, GroupNorm(32, eps 1e-6) + swish written
straight into the next conv's window, 1x1x1 shortcuts as GEMMs, the residual add in the conv epilogue.  New kernels
(ld_vae_enc.hip): the input placement, DownSample3D's time pool + space-to-depth layout (its 3x3 stride-2 conv then runs as a
stride-1 conv over 4C channels: the same products, summed in another order) and the posterior.  bf16 activations with
fp32 accumulation where the reference runs fp32 (disable_first_stage_autocast): judged by the 2x-floor rule.
"""
from __future__ import annotations

import os

import torch

from . import _lib, ops
from .config import VAEConfig
from .detokenizer import _conv_w, _dev
from .weights import vae_encoder_levels, vae_encoder_spec

BF = torch.bfloat16
IN_PAD = 64          # conv_in's 3 input channels zero-padded to the MFMA K-tile (the conv's Cin % 64 rule)


def s2d_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight [Co, C, 3, 3] of a stride-2 conv with right / bottom pad (0, 1, 0, 1) -> the channels-last weight
    [Co, 1, 3, 3, 4C] of the equivalent stride-1 conv over the space-to-depth layout (ld_vae_enc_downsample):
    Ws[o, 0, A, B, (2p+q)C + c] = w[o, c, 2A+p, 2B+q] for A, B in {0, 1}, zero for the taps 2A+p = 3 or 2B+q = 3 that do not
    exist and for A = 2 or B = 2 (ld_conv_cl_bf16 takes odd kernel sizes: the 2 x 2 conv is a 3 x 3 one whose last row and
    column of taps are zero, 9/4 of the MACs)."""
    Co, C, kh, kw = w.shape
    assert kh == 3 and kw == 3
    wp = torch.nn.functional.pad(w, (0, 3, 0, 3))                          # [Co, C, 6, 6]: taps >= 3 are zero
    ws = wp.reshape(Co, C, 3, 2, 3, 2)                                      # [o, c, A, p, B, q]
    return ws.permute(0, 2, 4, 3, 5, 1).reshape(Co, 1, 3, 3, 4 * C).contiguous()   # [o, A, B, p, q, c]


def encoder_convs(cfg: VAEConfig, F: int, H: int, W: int):
    """Every convolution an F-frame H x W encode launches, in order: [(name, (T, H, W, Cin, Cout, kT, kH, kW))], the arguments
    of ld_conv_route (the 1 x 1 x 1 shortcuts are GEMMs and are not listed)."""
    T, C = F, cfg.ch
    out = [("conv_in", (T, H, W, IN_PAD, C, 3, 3, 3))]
    for lvl, blocks, down in vae_encoder_levels(cfg):
        for j, (cin, cout) in enumerate(blocks):
            out += [(f"down.{lvl}.block.{j}.conv1", (T, H, W, cin, cout, 3, 3, 3)),
                    (f"down.{lvl}.block.{j}.conv2", (T, H, W, cout, cout, 3, 3, 3))]
            C = cout
        if down:
            T, H, W = ops.vae_enc_downsample_out_frames(T, down == "space_time"), H // 2, W // 2
            out.append((f"down.{lvl}.downsample", (T, H, W, 4 * C, C, 1, 3, 3)))
    for b in ("mid.block_1", "mid.block_2"):
        out += [(f"{b}.conv1", (T, H, W, C, C, 3, 3, 3)), (f"{b}.conv2", (T, H, W, C, C, 3, 3, 3))]
    out.append(("conv_out", (T, H, W, C, 2 * cfg.z_channels, 3, 3, 3)))
    return out


def max_clip_frames(cfg: VAEConfig, H: int, W: int) -> int:
    """The longest clip encode_moments takes at H x W: every convolution of the encode must have a route (ld_conv_route >= 0,
    the launcher's own size rules, run dry).  The level-0 window is the first to reach the convolution's 8 GiB input limit:
    94 frames at 480 x 720.  0 if not even one frame fits."""
    lib = _lib.load()
    fits = lambda F: all(lib.ld_conv_route(*shape) >= 0 for _, shape in encoder_convs(cfg, F, H, W))
    if not fits(1):
        return 0
    lo, hi = 1, 2                       # fits(lo), and the input grows with F: double, then bisect
    while fits(hi):
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


class VAEEncoder:
    def __init__(self, sd: dict, cfg: VAEConfig, device):
        self.cfg, self.dev = cfg, torch.device(device)
        missing = [n for n, _, _ in vae_encoder_spec(cfg) if n not in sd]
        if missing:
            raise KeyError(f"VAE encoder state lacks {len(missing)} keys, e.g. {missing[:3]} (3d-vae.pt['state_dict'] 'encoder.*')")
        self.w = {}
        for k, v in sd.items():
            if not k.startswith("encoder."):
                continue
            if k.endswith("downsample.conv.weight"):
                self.w[k] = _dev(s2d_conv_weight(v.float()), self.dev)
            elif k.endswith("weight") and v.dim() == 5:
                if v.shape[-3:] == (1, 1, 1):                                 # 1x1x1 shortcut -> GEMM weight [Cout, Cin]
                    self.w[k] = _dev(v.reshape(v.shape[0], v.shape[1]), self.dev)
                else:
                    self.w[k] = _conv_w(v, self.dev, cin_pad=IN_PAD if v.shape[1] < IN_PAD else None)
            else:
                self.w[k] = _dev(v, self.dev)
        # same switch as the decoder's: GroupNorm statistics from the producing conv's epilogue (LD_VAE_GN_FUSE=0: a separate pass)
        self.fuse_gn_stats = os.environ.get("LD_VAE_GN_FUSE", "1") != "0"
        self._max_frames = {}           # (H, W) -> max_clip_frames
        # zero-bordered conv inputs, one per shape, zero-filled once: every producer rewrites the whole interior (and the halo
        # frames), never the border; the encoder is a chain, so stream order is the only hazard between users of one buffer
        self._padded = {}

    def latent_frames(self, F: int) -> int:
        """Latent frames of an F-frame clip: (F + 3) // 4 at temporal_compress_times 4."""
        T = F
        for _, _, down in vae_encoder_levels(self.cfg):
            if down:
                T = ops.vae_enc_downsample_out_frames(T, down == "space_time")
        return T

    def workspace_bytes(self) -> int:
        """HBM held by the padded conv inputs (kept across encodes: no second zero-fill).  About 13 GB for a 49-frame 480 x 720
        clip (the level-0 128-channel window alone is 4.5 GB)."""
        return sum(b.numel() * b.element_size() for b in self._padded.values())

    def release(self) -> None:
        """Drop the padded-input buffers (the next encode allocates and zero-fills them again; same results)."""
        self._padded.clear()
        torch.cuda.empty_cache()

    def _buf(self, *shape):
        buf = self._padded.get(shape)
        if buf is None:
            buf = self._padded[shape] = torch.zeros(*shape, device=self.dev, dtype=BF)
        return buf

    def _gn_ok(self, C: int) -> bool:
        q = C // 4
        return (self.fuse_gn_stats and C % 8 == 0 and 0 < q <= 256 and 256 % q == 0 and q % self.cfg.gn_groups == 0
                and self.cfg.gn_groups <= 64)

    def _conv(self, xp, name, T, H, W, **epi):
        gn = self._gn_ok(self.w[name + ".conv.bias"].numel())
        r = ops.conv_cl(xp, self.w[name + ".conv.weight"], T, H, W, bias=self.w[name + ".conv.bias"], gn_partials=gn, **epi)
        return r if gn else (r, None)

    def _norm_swish(self, xg, name, T, H, W, C):
        """swish(GroupNorm(x)) over the whole clip -> the interior of a causal conv's window, halo frames = frame 0."""
        cfg = self.cfg
        x, part = xg
        stats = torch.empty(1, cfg.gn_groups, 2, device=self.dev, dtype=torch.float64)
        if part is None:
            ops.groupnorm_stats(x, stats, 1, T * H * W, C, cfg.gn_groups)
        else:
            ops.groupnorm_stats_from_conv(part, stats, T * H * W, C, cfg.gn_groups)
        xp = self._buf(T + 2, H + 2, W + 2, C)
        ops.groupnorm_apply(x, xp, stats, self.w[name + ".weight"], self.w[name + ".bias"], 1, T, H, W, C, cfg.gn_groups,
                            tpad=2, hpad=1, wpad=1, swish=True, eps=cfg.gn_eps)
        xp[0].copy_(xp[2]); xp[1].copy_(xp[2])
        return xp

    def _resblock(self, xg, p, cin, cout, T, H, W):
        hp = self._norm_swish(xg, p + "norm1", T, H, W, cin)
        hg = self._conv(hp, p + "conv1", T, H, W)
        hp = self._norm_swish(hg, p + "norm2", T, H, W, cout)
        del hg
        x = xg[0]
        if cin != cout:
            x = ops.gemm(x, self.w[p + "nin_shortcut.weight"], bias=self.w[p + "nin_shortcut.bias"])
        return self._conv(hp, p + "conv2", T, H, W, resid=x)

    @torch.no_grad()
    def encode_moments(self, frames: torch.Tensor, eps: torch.Tensor | None = None, want_moments: bool = False):
        """frames [F, H, W, 3] (uint8, or f32 in [-1, 1]) on the device -> z f32 [T', 16, H/8, W/8] = scale_factor *
        (mean + exp(0.5 logvar) * eps) or scale_factor * mean (eps None); eps [16, T', h, w] f32.  want_moments: also
        (mean, clamped logvar) [T', 16, h, w]."""
        cfg = self.cfg
        F, H, W, _ = frames.shape
        if H % 8 or W % 8:
            raise ValueError(f"frame size {H}x{W}: height and width must be multiples of 8")
        if (H, W) not in self._max_frames:
            self._max_frames[H, W] = max_clip_frames(cfg, H, W)
        if F > self._max_frames[H, W]:
            raise ValueError(f"a {F}-frame clip at {H}x{W} is too long: the encoder takes at most {self._max_frames[H, W]} frames "
                             f"at this size (its level-0 convolution input would pass the 8 GiB the kernels address)")
        frames = frames.to(self.dev).contiguous()
        if frames.dtype != torch.uint8:
            frames = frames.float().contiguous()
        p = "encoder."
        xp = self._buf(F + 2, H + 2, W + 2, IN_PAD)
        ops.vae_enc_place_input(frames, xp)
        T = F
        h = self._conv(xp, p + "conv_in", T, H, W)
        for lvl, blocks, down in vae_encoder_levels(cfg):
            for j, (cin, cout) in enumerate(blocks):
                h = self._resblock(h, p + f"down.{lvl}.block.{j}.", cin, cout, T, H, W)
                C = cout
            if down:
                To = ops.vae_enc_downsample_out_frames(T, down == "space_time")
                s2d = self._buf(To, H // 2 + 2, W // 2 + 2, 4 * C)
                ops.vae_enc_downsample(h[0], s2d, T, H, W, C, down == "space_time")
                T, H, W = To, H // 2, W // 2
                h = self._conv(s2d, p + f"down.{lvl}.downsample", T, H, W)
        h = self._resblock(h, p + "mid.block_1.", C, C, T, H, W)
        h = self._resblock(h, p + "mid.block_2.", C, C, T, H, W)
        hp = self._norm_swish(h, p + "norm_out", T, H, W, C)
        del h
        Z = cfg.z_channels
        moments = ops.conv_cl(hp, self.w[p + "conv_out.conv.weight"], T, H, W, bias=self.w[p + "conv_out.conv.bias"],
                              out_f32=True)
        z = torch.empty(T, Z, H, W, device=self.dev, dtype=torch.float32)
        mean = torch.empty_like(z) if want_moments else None
        logvar = torch.empty_like(z) if want_moments else None
        if eps is not None:
            eps = eps.to(device=self.dev, dtype=torch.float32).reshape(Z, T, H, W).contiguous()
        ops.vae_posterior(moments, z, T, Z, H, W, cfg.scale_factor, eps=eps, mean=mean, logvar=logvar)
        return (z, mean, logvar) if want_moments else z

    @torch.no_grad()
    def encode(self, frames: torch.Tensor, *, sample: bool = False, eps: torch.Tensor | None = None) -> torch.Tensor:
        """frames uint8 [F, H, W, 3] (or f32 in [-1, 1]) -> latent [1, (F+3)//4, 16, H/8, W/8] fp32, scale_factor included (the
        `prefix` the sampler takes).  sample=False: the posterior's mode; sample=True: mean + std * eps with eps given in the
        reference's [1, 16, T', h, w] order, or drawn with torch.randn_like on the device's global generator (the reference's
        posterior.sample())."""
        if sample and eps is None:
            F, H, W, _ = frames.shape
            eps = torch.randn(1, self.cfg.z_channels, self.latent_frames(F), H // 8, W // 8, device=self.dev, dtype=torch.float32)
        z = self.encode_moments(frames, eps if sample else None)
        return z.unsqueeze(0)
