"""Task API of landiff/diffusion/dif_infer.py:84-302 on the MI355X path: CogModelInferWrapper(ckpt_path, infer_cfg_path,
model_cfg_path)(VideoTask) and, one level down, CogWrapper.forward(inputs, seed, semantic_token,
semantic_feature_before_upsample, vae_feature_prefix) -> CogOutput.  Every shape comes from the two YAML files (PyYAML;
landiff_amd.config.load_diffusion_config), every weight from the reference's checkpoint tree."""
from __future__ import annotations

import os
from dataclasses import dataclass

import torch

from landiff.utils import set_seed_for_single_process, stable_hash
from landiff_amd.config import DiffusionInferConfig, load_diffusion_config
from landiff_amd.detokenizer import Detokenizer
from landiff_amd.dit import ControlDiTRunner
from landiff_amd.config import AttnWindowConfig
from landiff_amd.dit_cache import as_config
from landiff_amd.dit_guidance import as_config as as_guidance_config
from landiff_amd.sampler import DiffusionSampler
from landiff_amd.text import encode_t5_v11
from landiff_amd.vae import VAEDecoder
from landiff_amd.weights import load_diffusion_states, load_tokenizer_encoder_state, load_vae_encoder_state, resolve_ckpt_path

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_INFER_CFG = "landiff/diffusion/configs/infer_cfgs/2b.yaml"
DEFAULT_MODEL_CFG = "landiff/diffusion/configs/cogvideox_2b_control_theia_interpolate_video_vq.yaml"


def _cfg_path(path: str) -> str:
    """The reference opens its YAML paths relative to the working directory (the repository root); when run from elsewhere the
    copy shipped next to this file is used for the two default names."""
    if os.path.exists(path):
        return path
    cand = os.path.join(os.path.dirname(os.path.dirname(_HERE)), path)
    if os.path.exists(cand):
        return cand
    raise FileNotFoundError(f"config file {path!r} not found (cwd {os.getcwd()!r})")


def _pre_process_cog_video(video: torch.Tensor) -> torch.Tensor:
    """dif_infer.py:22-34: [0,1] -> [-1,1]."""
    return torch.clamp(video * 2.0 - 1.0, -1.0, 1.0)


@dataclass
class CogOutput:
    video: torch.Tensor   # rgb video tensor, shape [B, C, T, H, W], range [0,1]
    latent: torch.Tensor  # latent tensor, shape [B, T, C, H, W]


@dataclass
class VideoTask:
    save_file_name: str
    prompt: str
    seed: int
    fps: int = 8
    mp4: None | torch.Tensor = None
    semantic_token: None | torch.Tensor = None
    result: None | torch.Tensor = None


class CogWrapper(torch.nn.Module):
    """dif_infer.py:101-271.  Built from the parsed configs instead of an argument string; `seed` is sat's --seed default (1234),
    used only when forward() gets no seed (then hashed with the prompt, :190-194)."""

    def __init__(self, cfg: DiffusionInferConfig, ckpt_path: str, device, seed: int = 1234, text_encoder=None,
                 feature_extractor=None, theia_ckpt: str | None = None, dit_cache=None, attn_window=None,
                 dit_guidance=None):
        super().__init__()
        if feature_extractor is not None and theia_ckpt is not None:
            raise ValueError("give the Theia extractor as one of feature_extractor and theia_ckpt")
        self.cfg, self.device_, self.seed = cfg, device, seed
        self.image_size = list(cfg.image_size)
        self.text_encoder, self.feature_extractor = text_encoder, feature_extractor
        self.theia = None               # landiff_amd.theia.TheiaExtractor of theia_ckpt
        if theia_ckpt is not None:
            from landiff_amd.theia import build_theia
            self.theia = build_theia(theia_ckpt, cfg.tok, device)
        st = load_diffusion_states(resolve_ckpt_path(ckpt_path), None, base_dit_ckpt=cfg.base_dit_ckpt, vae_ckpt=cfg.vae_ckpt,
                                   tokenizer_ckpt=cfg.tokenizer_ckpt or None)
        self.detok = Detokenizer(st["tok"], st["ups"], cfg.tok, cfg.ups, device)
        self.sampler = DiffusionSampler(cfg.sampler)
        # dit_cache (not in the reference): None, a threshold or a landiff_amd.dit_cache.StepCacheConfig -- the DiT step cache
        self.dit_cache = as_config(dit_cache)
        # attn_window (not in the reference): None, a window in frames or a landiff_amd.config.AttnWindowConfig -- frame-window attention
        self.attn_window = AttnWindowConfig.as_config(attn_window)
        win = {} if self.attn_window is None else {"attn_window": self.attn_window}
        # dit_guidance (not in the reference): None, a scale tolerance or a landiff_amd.dit_guidance.GuidanceSkipConfig -- cond-only steps
        self.dit_guidance = as_guidance_config(dit_guidance)
        if self.dit_guidance is not None:
            win["dit_guidance"] = self.dit_guidance
        planned = self.dit_cache is not None or self.dit_guidance is not None
        self.dit = ControlDiTRunner(st["dit_main"], st["dit_control"], cfg.dit, device, step_cache=self.dit_cache, **win,
                                    plan_timesteps=[sp.timestep for sp in self.sampler.plan] if planned else None)
        self.vae = VAEDecoder(st["vae"], cfg.vae, device)
        self._encoder = None            # tokenizer encoder half: built on the first video-conditioned call
        self._vae_encoder = None        # 3D-VAE encoder: built on the first encode_first_stage call
        self._ckpt_path = ckpt_path

    def _context(self, text: str) -> torch.Tensor:
        """FrozenT5Embedder on the prompt, padded to text_length, pad positions not masked (encoders/modules.py:246-295); the
        unconditional branch is zeroed by force_uc_zero_embeddings=["txt"] (dif_infer.py:176,214-218), which
        ControlDiTRunner.set_condition does."""
        d = self.cfg.dit
        if self.text_encoder is not None:
            ctx = self.text_encoder([text])
            ctx = ctx[0] if isinstance(ctx, (list, tuple)) else ctx
            ctx = ctx.reshape(1, d.text_len, d.text_dim)
        else:
            ctx = encode_t5_v11([text], resolve_ckpt_path(self.cfg.t5_dir), d.text_len, self.device_)
        return ctx

    def _semantic_from_video(self, mp4_btchw: torch.Tensor) -> torch.Tensor:
        """Control signal from a conditioning video (ControlDiffusionTransformer.forward :960-975 -> SemanticCond.forward(visual)
        :112-137 -> VideoVQWrap.forward(images) vq_warp.py:88-118): t equally spaced frames, [-1,1] -> uint8, padded to a square
        with grey 127, Theia features -> tokenizer encoder -> nearest code -> tokenizer decoder -> upsampler.  The Theia backbone
        is `feature_extractor` (any callable), or the HIP extractor of `theia_ckpt` (landiff_amd.theia), which makes the square
        padding inside its first kernel and hands the tokenizer encoder channels-last rows."""
        if self.feature_extractor is None and self.theia is None:
            raise NotImplementedError(
                "VideoTask.mp4 (video-conditioned generation) needs the Theia feature extractor (landiff/tokenizer/models/"
                "feature_extractor/theia_extractor.py): pass CogModelInferWrapper(..., theia_ckpt=<Theia model.safetensors>) or "
                "CogModelInferWrapper(..., feature_extractor=callable uint8 [T,3,S,S] -> features [T,C,h,w]), or give semantic_token")
        d, tc = self.cfg.dit, self.cfg.tok
        v = mp4_btchw[0]
        idx = torch.linspace(0, v.shape[0] - 1, d.latent_frames).long().to(v.device)
        v = v[idx]
        v = ((v + 1.0) / 2.0).clamp(0, 1)
        # torchvision v2.functional.to_dtype(uint8, scale=True) on a float image: image.mul(255 + 1 - 1e-3).to(uint8), i.e.
        # truncation of x * 255.999 (torchvision is not in this image: restated from its float -> int conversion rule)
        v = v.float().mul(255.0 + 1.0 - 1e-3).to(torch.uint8)
        if self.theia is not None:
            self.theia.encoder = self._tokenizer_encoder()
            tokens = self.theia.tokenize_video(v.permute(0, 2, 3, 1).contiguous())       # [T, H, W, 3], padded by the kernel
            return self.detok.semantic_condition(tokens)
        H, W = v.shape[-2:]
        S = max(H, W)
        sq = torch.full((v.shape[0], v.shape[1], S, S), 127, dtype=torch.uint8, device=v.device)
        sq[..., :H, :W] = v                                                # pad_to_square: right / bottom (condition.py:14-27)
        feats = self.feature_extractor(sq)
        assert feats.shape == (tc.temporal, tc.out_channels, tc.grid_h, tc.grid_w), f"feature_extractor returned {tuple(feats.shape)}"
        tokens = self._tokenizer_encoder().encode_to_index(feats.to(self.device_))
        return self.detok.semantic_condition(tokens)

    def _tokenizer_encoder(self):
        if self._encoder is None:
            from landiff_amd.tokenizer_encoder import TokenizerEncoder
            self._encoder = TokenizerEncoder(load_tokenizer_encoder_state(resolve_ckpt_path(self.cfg.tokenizer_ckpt)),
                                             self.cfg.tok, self.device_)
        return self._encoder

    @torch.no_grad()
    def encode_first_stage(self, x: torch.Tensor) -> torch.Tensor:
        """SATVideoDiffusionEngine.encode_first_stage (diffusion_video.py:233-254) with the reference's regularizer:
        x [B, 3, T, H, W] in [-1, 1] -> scale_factor * posterior.sample() [B, 16, (T+3)//4, H/8, W/8] fp32, the sample drawn
        with randn_like on the device's global generator.  Permuted to [B, T', 16, h, w] it is the `vae_feature_prefix`
        forward() takes.  The encoder's weights: 'encoder.*' of the VAE checkpoint, then of the diffusion checkpoint's
        first_stage_model (weights.load_vae_encoder_state)."""
        if self._vae_encoder is None:
            from landiff_amd.vae_encoder import VAEEncoder
            sd = load_vae_encoder_state(None, vae_ckpt=self.cfg.vae_ckpt, diffusion_dir=resolve_ckpt_path(self._ckpt_path))
            self._vae_encoder = VAEEncoder(sd, self.cfg.vae, self.device_)
        B, _, T, H, W = x.shape
        enc = self._vae_encoder
        # one randn_like over the whole [B, 16, T', h, w] posterior, as the reference draws it
        eps = torch.randn(B, enc.cfg.z_channels, enc.latent_frames(T), H // 8, W // 8, device=self.device_, dtype=torch.float32)
        out = []
        for b in range(B):
            frames = x[b].permute(1, 2, 3, 0).to(self.device_, torch.float32).contiguous()      # [T, H, W, 3]
            out.append(enc.encode(frames, sample=True, eps=eps[b:b + 1]).permute(0, 2, 1, 3, 4))
        return torch.cat(out, dim=0)

    @torch.no_grad()
    def forward(self, inputs: dict, seed: int | None = None, semantic_token: torch.Tensor | None = None,
                semantic_feature_before_upsample: torch.Tensor | None = None,
                vae_feature_prefix: torch.Tensor | None = None) -> CogOutput:
        d, dev = self.cfg.dit, self.device_
        text, mp4 = inputs["caption"], inputs.get("video")
        if mp4 is not None:
            mp4 = _pre_process_cog_video(mp4.permute(0, 2, 1, 3, 4))       # b c t h w -> b t c h w
        text_seed = seed if seed is not None else (stable_hash(str(text)) + self.seed) % 2 ** 32
        set_seed_for_single_process(text_seed)
        ctx = self._context(text)
        # the control DiT evaluates the semantic condition once, at the first denoiser call, and caches it
        # (InferValueRegistry, dit_video_concat.py:939-982); precedence token > feature-before-upsample > video as there
        if semantic_token is not None:
            sem = self.detok.semantic_condition(semantic_token.to(dev).reshape(-1))
        elif semantic_feature_before_upsample is not None:
            sem = self.detok.semantic_condition_from_features(semantic_feature_before_upsample.to(dev))
        elif mp4 is not None:
            sem = self._semantic_from_video(mp4.to(dev))
        else:
            raise KeyError("mp4")            # the reference's kwargs["mp4"] lookup with nothing registered
        self.dit.set_condition(ctx, sem)
        noise = torch.randn(1, d.latent_frames, d.in_channels, d.latent_h, d.latent_w, device=dev, dtype=torch.float32)
        prefix = vae_feature_prefix.to(dev, torch.float32) if vae_feature_prefix is not None else None
        z = self.sampler.run(self.dit.step, noise, prefix=prefix)
        z = z.to(torch.bfloat16) if self.cfg.bf16 else z                   # samples.to(self.dtype), diffusion_video.py:314
        _, video = self.vae.decode(z.float(), want_float=True)
        return CogOutput(video=video[None], latent=z)


class CogModelInferWrapper(torch.nn.Module):
    """CogModelInferWrapper(ckpt_path, infer_cfg_path, model_cfg_path)(VideoTask) -> VideoTask with .result FloatTensor
    [3, 4T-3, H, W] in [0,1] on CPU (dif_infer.py:274-302).
    text_encoder: optional callable prompts -> [1, text_length, 4096] T5 states (pre-computed embeddings) replacing the
    T5-v1.1-XXL run; feature_extractor: the Theia backbone for VideoTask.mp4 (see CogWrapper._semantic_from_video), or
    theia_ckpt: a Theia model.safetensors (or its directory) that the HIP extractor is built from (landiff_amd.theia).
    dit_cache: None, a threshold or a landiff_amd.dit_cache.StepCacheConfig -- the opt-in DiT step cache (not in the reference).
    attn_window: None, a window in frames or a landiff_amd.config.AttnWindowConfig -- the opt-in frame-window attention of the DiT (not in
    the reference; its effect on a trained checkpoint's output is unmeasured).
    dit_guidance: None, a scale tolerance or a landiff_amd.dit_guidance.GuidanceSkipConfig -- the opt-in CFG branch skipping of the DiT (not
    in the reference; its effect on a trained checkpoint's output is unmeasured; refused together with dit_cache)."""

    def __init__(self, ckpt_path: str, infer_cfg_path: str = DEFAULT_INFER_CFG, model_cfg_path: str = DEFAULT_MODEL_CFG,
                 device="cuda", text_encoder=None, feature_extractor=None, theia_ckpt: str | None = None, dit_cache=None,
                 attn_window=None, dit_guidance=None):
        super().__init__()
        self.infer_cfg_path, self.model_cfg_path, self.ckpt_path = infer_cfg_path, model_cfg_path, ckpt_path
        cfg = load_diffusion_config(_cfg_path(model_cfg_path), _cfg_path(infer_cfg_path))
        dev = torch.device(device if device != "cuda" else f"cuda:{torch.cuda.current_device()}")
        self.init_infer_model = CogWrapper(cfg, ckpt_path, dev, text_encoder=text_encoder, feature_extractor=feature_extractor,
                                           theia_ckpt=theia_ckpt, dit_cache=dit_cache, attn_window=attn_window,
                                           dit_guidance=dit_guidance)

    def dit_cache_report(self):
        """dit_cache: the step cache's report of the last forward() (ControlDiTRunner.cache_report), else None."""
        m = self.init_infer_model
        return [dict(r) for r in m.dit.cache_report] if m.dit_cache is not None else None

    def dit_guidance_report(self):
        """dit_guidance: the report of the last forward() (ControlDiTRunner.guidance_report), else None."""
        m = self.init_infer_model
        return [dict(r) for r in m.dit.guidance_report] if m.dit_guidance is not None else None

    @torch.no_grad()
    def forward(self, x: VideoTask) -> VideoTask:
        inputs = dict(caption=x.prompt, video=x.mp4 if x.mp4 is not None else None)
        output = self.init_infer_model.forward(inputs, seed=x.seed, semantic_token=x.semantic_token)
        video = output.video
        assert video.shape[0] == 1, f"video.shape[0] != 1, {video.shape[0]}"
        x.result = video.cpu()[0]
        return x
