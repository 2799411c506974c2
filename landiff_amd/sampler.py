"""The diffusion sampling loop on the device (VPSDE DPM-Solver++(2M) SDE, or deterministic DDIM).

Mirrors SATVideoDiffusionEngine.sample (landiff/diffusion/diffusion_video.py:256-315) and
VPSDEDPMPP2MSampler / VideoDDIMSampler (landiff/diffusion/sgm/modules/diffusionmodules/sampling.py:538-837):
initial randn from the global device generator, two randn_like draws per step from step 2 on, last step returns
the denoised sample, result cast to bf16.  The state stays fp32 in HBM; the elementwise updates are HIP kernels,
torch supplies only the RNG (K10: kept for RNG-stream parity).
"""
from __future__ import annotations

import torch

from . import ops
from .config import SamplerConfig
from .schedule import build_plan, step_alphas


class DiffusionSampler:
    def __init__(self, cfg: SamplerConfig):
        self.cfg = cfg
        self.plan = build_plan(cfg)
        self.alphas = step_alphas(cfg)          # (alpha, sigma) of the state on entry to step i; [num_steps]: of the result

    @torch.no_grad()
    def run(self, denoise_step, noise: torch.Tensor, randn_like=torch.randn_like, prefix=None, trace=None,
            fixed_frames: int = 0, *, start: int = 0, known: torch.Tensor | None = None, known_mask: torch.Tensor | None = None,
            known_noise: bool = True):
        """denoise_step(x, timestep, c_out, c_skip, cfg_scale, out) -> out (fp32, same shape as x).
        noise [1,T,C,H,W] fp32 on the device.  `prefix` latents overwrite the first frames (diffusion_video.py:287-288);
        `fixed_frames` > 0 pins the first frames to their initial value before every step and at the end
        (VPSDEDPMPP2MSampler.__call__, sampling.py:800-835, sdedit=False) -- the streaming primitive.

        Editing a given latent (keyword-only; not together with prefix / fixed_frames):
        `start` > 0 runs self.plan[start:], the first executed step first-order as on a fresh run.  With `known` [1,T,C,H,W] fp32 the
        state is first set to alpha[start] * known + sigma[start] * noise (the SDEdit start; at start == 0 that is `noise` itself and
        nothing is launched).  `known_mask` [T,H,W] (uint8 / bool, broadcast over C; needs `known`) marks cells to keep: before every
        executed step i they are overwritten with alpha[i] * known + sigma[i] * randn_like(x) -- the reference's sdedit=True branch
        over any set of cells, its draw before the step's own draws -- or, with known_noise=False, with `known` itself and no draw
        (the sdedit=False analogue); after the last step they are `known`.  The mask form draws full-shape noise."""
        S = len(self.plan)
        editing = start != 0 or known is not None or known_mask is not None
        if editing:
            if prefix is not None or fixed_frames:
                raise ValueError("DiffusionSampler.run: start / known / known_mask do not go together with prefix / fixed_frames")
            if not isinstance(start, int) or isinstance(start, bool) or not 0 <= start < S:
                raise ValueError(f"DiffusionSampler.run: start={start!r} outside [0, {S}) (the sampler's steps)")
            if known_mask is not None and known is None:
                raise ValueError("DiffusionSampler.run: known_mask marks cells of `known` to keep; known is missing")
            if known is not None and (known.shape != noise.shape or known.dtype != torch.float32 or known.device != noise.device):
                raise ValueError(f"DiffusionSampler.run: known must be float32 {tuple(noise.shape)} on {noise.device}, got "
                                 f"{known.dtype} {tuple(known.shape)} on {known.device}")
        x = noise.clone()
        if known is not None:
            known = known.contiguous()
            if start > 0:
                ops.latent_pin(x, known, x, None, *self.alphas[start])
        if prefix is not None:
            x[:, : prefix.shape[1]] = prefix
        pinned = x[:, :fixed_frames].clone() if fixed_frames > 0 else None
        den = torch.empty_like(x)
        den_d = torch.empty_like(x)
        old = torch.empty_like(x)
        have_old = False
        for sp in (self.plan[start:] if start else self.plan):
            if pinned is not None:
                x[:, :fixed_frames] = pinned                    # slab copy (plumbing)
            if known_mask is not None:
                ops.latent_pin(x, known, randn_like(x) if known_noise else None, known_mask, *self.alphas[sp.index])
            denoise_step(x, sp.timestep, sp.c_out, sp.c_skip, sp.cfg_scale, den)
            if trace is not None:
                trace.append((sp.index, sp.timestep, sp.cfg_scale))
            if self.cfg.sampler == "ddim":
                ops.axpbypcz(x, x, sp.a_t, den, sp.b_t)
                continue
            if sp.last:
                x.copy_(den)
                continue
            n1 = randn_like(x)
            if not have_old:
                ops.axpbypcz(x, x, sp.m1, den, -sp.m2, n1, sp.m_noise)
            else:
                n2 = randn_like(x)                              # x_standard's draw is discarded, as in the reference
                ops.axpbypcz(den_d, den, sp.m3, old, -sp.m4)
                ops.axpbypcz(x, x, sp.m1, den_d, -sp.m2, n2, sp.m_noise)
            old, den = den, old
            have_old = True
        if pinned is not None:
            x[:, :fixed_frames] = pinned
        if known_mask is not None:
            ops.latent_pin(x, known, None, known_mask, 1.0, 0.0)
        return x
