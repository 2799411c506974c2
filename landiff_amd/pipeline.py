"""Per-prompt pipeline on one MI355X and prompt-batch data parallelism over the GPUs of a node.

Stage order of landiff/infer_video.py:105-114: AR token decode (ArModelInferWrapper, landiff/llm/llm_infer.py:74-105)
-> CogWrapper.forward (landiff/diffusion/dif_infer.py:152-243): semantic condition once per video, 50 sampler steps over
the control+main DiT, chunked VAE decode, post-process.  Unlike the reference nothing leaves the device between the
stages (no .npy round trip of the tokens, no model .cpu()/.cuda() shuffling, VAE caches in HBM).
"""
from __future__ import annotations

import os
import sys
import time
from dataclasses import dataclass

import torch

from . import _lib, ops
from .config import AttnWindowConfig, PipelineConfig
from .conform import ConformConfig, conform_clip, conform_mask, conform_plan
from .detokenizer import Detokenizer
from .dit import ControlDiTRunner
from .dit_cache import as_config
from .dit_guidance import as_config as as_guidance_config
from .llm import LLMRunner
from .sampler import DiffusionSampler
from .vae import VAEDecoder
from .vae_encoder import VAEEncoder


# latent frames of the previous chunk a streamed chunk pins as its prefix: the shipped sampler's "fixed_frames: 7 # 49 frames,
# 13 latent, prefix_length=7" (cogvideox_2b_control_theia_interpolate_video_vq.yaml :213,231)
STREAM_PREFIX_FRAMES = 7
# frames per second of the model's clips (sampling_fps of the shipped config; infer_video writes its videos at it): where the
# conform stage puts output frame k of a clip whose own rate is given, k / MODEL_FPS seconds
MODEL_FPS = 8


@dataclass
class PromptInputs:
    """What the boundary hands to the hot path for one prompt (T5 encoders are outside the path)."""
    llm_text_emb: torch.Tensor        # [n, text_dim]   FLAN-T5-XXL states of the prompt (LLM condition)
    dit_context: torch.Tensor         # [1, text_len, text_dim]  T5-v1.1-XXL states, padded to text_len
    seed: int = 42
    cfg: float = 7.5
    motion_score: float = 0.1


class LanDiffPipeline:
    def __init__(self, cfg: PipelineConfig, states: dict, device="cuda:0", max_llm_frames: int | None = None,
                 fp8_gemm: bool = False, theia=None, max_samples: int = 1, wide_samples: int = 0, dit_cache=None, attn_window=None,
                 dit_guidance=None):
        if not torch.cuda.is_available():
            raise _lib.LandiffHipError("LanDiffPipeline needs an MI355X GPU: there is no CPU fallback")
        _lib.load()
        self.cfg = cfg.check()
        self.dev = torch.device(device)
        torch.cuda.set_device(self.dev)
        # max_llm_frames > segment_length sizes the KV cache / position tables for multi-segment (streaming) decodes
        # max_samples > 1: generate_samples decodes that many samples of a prompt side by side (LLMRunner.sample_many);
        # wide_samples (0..16): as many with generate_samples(engine="mfma") (the MFMA decode engine, ~0.36 GB of KV cache per row)
        self.llm = LLMRunner(states["llm"], cfg.llm, self.dev, max_frames=max_llm_frames or cfg.llm.segment_length,
                             max_samples=max_samples, wide_samples=wide_samples) if "llm" in states else None
        self.detok = Detokenizer(states["tok"], states["ups"], cfg.tok, cfg.ups, self.dev)
        # fp8_gemm: BASELINE configs[4] (e4m3 operands for the DiT's four large linears); never the headline configuration
        # dit_cache: None (off), a threshold or a dit_cache.StepCacheConfig -- sampler steps whose first-block input barely moved reuse
        # the last computed step's residual across the transformer stack (ControlDiTRunner(step_cache=...)); never the headline
        # configuration, and what a threshold costs in quality on a trained checkpoint is not measured
        self.sampler = DiffusionSampler(cfg.sampler)
        self.dit_cache = as_config(dit_cache)
        # attn_window: None (off), a window in frames or a config.AttnWindowConfig -- frame-window attention in the DiT
        # (ControlDiTRunner(attn_window=...)); never the headline configuration, and what a window does to a trained
        # checkpoint's output is not measured; handed on only when given
        self.attn_window = AttnWindowConfig.as_config(attn_window)
        win = {} if self.attn_window is None else {"attn_window": self.attn_window}
        # dit_guidance: None (off), a scale tolerance or a dit_guidance.GuidanceSkipConfig -- sampler steps that evaluate the cond
        # branch alone (ControlDiTRunner(dit_guidance=...)); never the headline configuration, and what any setting costs in quality on
        # a trained checkpoint is not measured; handed on only when given.  With dit_cache or fp8_gemm the runner refuses.
        self.dit_guidance = as_guidance_config(dit_guidance)
        if self.dit_guidance is not None:
            win["dit_guidance"] = self.dit_guidance
        planned = self.dit_cache is not None or self.dit_guidance is not None
        self.dit = ControlDiTRunner(states["dit_main"], states["dit_control"], cfg.dit, self.dev, fp8_gemm=fp8_gemm,
                                    step_cache=self.dit_cache, **win,
                                    plan_timesteps=[sp.timestep for sp in self.sampler.plan] if planned else None)
        self.dit_guidance_reports = []    # one ControlDiTRunner.guidance_report per sampler run (see dit_guidance_report())
        self.dit_cache_reports = []       # one ControlDiTRunner.cache_report per sampler run (see dit_cache_report())
        self.vae = VAEDecoder(states["vae"], cfg.vae, self.dev)
        # the 3D-VAE encoder of extend_video(frames=...): built when the VAE state carries 'encoder.*' keys
        # (weights.load_vae_encoder_state, or a synthetic tree whose states["vae"] has them)
        self.encoder = (VAEEncoder(states["vae"], cfg.vae, self.dev)
                        if any(k.startswith("encoder.") for k in states["vae"]) else None)
        # the Theia extractor of extend_video(clip_tokens="from_frames"): a landiff_amd.theia.TheiaExtractor whose `encoder` is
        # the tokenizer's encoder half (optional; nothing else uses it)
        self.theia = theia
        self.timings = {}
        self.last_candidates = None       # generate_samples(keep=k): every candidate's ids and scores
        self.last_edit = None             # edit_video: what the last call ran (strength, start_step, steps_run, ...)
        self.last_conform = None          # extend_video / edit_video(conform=...): ConformPlan.as_dict() of the last conformed clip
        self.last_conform_frames = None   # ... and that clip at the model's frame, uint8 on the device (None: nothing was conformed)
        self.last_metrics = None          # compare: the ClipMetrics of the last comparison
        self.last_retime = None           # retime: RetimePlan.as_dict() of the last retimed clip
        self.last_encode = None           # encode: encode.encode_report() of the last encoded clip
        self.last_decode = None           # decode: decode.decode_report() of the last decoded clip

    def _conform(self, frames, conform, keep_mask=None):
        """The conform stage of extend_video / edit_video: `frames` of any size / frame rate -> the 4T-3 frames of
        8h x 8w the rest of the call takes, and a pixel keep_mask in the source clip's geometry with them; timed as "conform"."""
        d = self.cfg.dit
        if frames is None:
            raise ValueError("conform= fits a clip given as frames=; a clip latent is already at the model's size")
        if frames.dim() != 4 or frames.dtype != torch.uint8 or frames.shape[-1] != 3:
            raise ValueError(f"clip frames must be uint8 [F, H, W, 3], got {frames.dtype} {tuple(frames.shape)}")
        t0 = time.perf_counter()
        plan = conform_plan(tuple(frames.shape), 4 * d.latent_frames - 3, 8 * d.latent_h, 8 * d.latent_w, conform)
        if keep_mask is not None and tuple(keep_mask.shape) == tuple(frames.shape[:3]):
            if keep_mask.dtype != torch.bool:
                raise ValueError(f"keep_mask must be bool, got {keep_mask.dtype} {tuple(keep_mask.shape)}")
            keep_mask = conform_mask(keep_mask, plan, self.dev)
        frames = conform_clip(frames, plan, self.dev)
        self.last_conform = plan.as_dict()
        self.last_conform_frames = frames
        self._t("conform", t0)
        return frames, keep_mask

    def compare(self, frames, reference, mask=None):
        """PSNR, SSIM and exact difference counts of two uint8 clips [F, H, W, C] of one shape (landiff_amd.metrics.compare_clips,
        DESIGN 8.10), e.g. what this pipeline returned with and without an opt-in switch; `mask` [F, H, W] bool keeps pixels.  The
        tensors may live anywhere and are moved to the pipeline's device.  Timed as "metrics"; the result is also self.last_metrics."""
        from .metrics import compare_clips
        t0 = time.perf_counter()
        to = lambda t: t.to(self.dev) if isinstance(t, torch.Tensor) else t
        with torch.cuda.device(self.dev):
            self.last_metrics = compare_clips(to(frames), to(reference), to(mask))
        self._t("metrics", t0)
        return self.last_metrics

    def retime(self, frames, cfg):
        """uint8 frames [F, H, W, C] at the model's MODEL_FPS -> uint8 frames at cfg.out_fps on the pipeline's device (cfg: a
        retime.RetimeConfig or a ready RetimePlan; landiff_amd.retime.retime_clip).  A function of the frames alone: it
        takes what __call__, generate_stream, extend_video or edit_video returned.  Timed as "retime"; the plan is self.last_retime."""
        from .retime import _as_plan, retime_clip
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.dtype != torch.uint8:
            raise ValueError(f"retime: frames must be uint8 [F, H, W, C], got {getattr(frames, 'dtype', type(frames))} "
                             f"{tuple(getattr(frames, 'shape', ()))}")
        t0 = time.perf_counter()
        plan = _as_plan(frames, cfg)
        with torch.cuda.device(self.dev):
            out = retime_clip(frames.to(self.dev).contiguous(), plan)
        self.last_retime = plan.as_dict()
        self._t("retime", t0)
        return out

    def encode(self, frames, cfg=None, verify: bool = False, rate=None):
        """uint8 frames [F, H, W, 3] -> list of F `bytes`, each a complete baseline JPEG, encoded on the pipeline's device (cfg: an
        encode.JpegConfig, default quality 95 at 4:2:0; landiff_amd.encode.encode_jpeg): the frames of a Motion-JPEG
        AVI (landiff.utils.write_mjpeg_avi_encoded) or stills.  A function of the frames alone: it takes what __call__,
        generate_stream, extend_video, edit_video or retime returned.  Timed as "encode"; the figures are self.last_encode.
        verify: the streams are decoded again where they are (landiff_amd.decode) and self.last_encode["verify"] holds
        metrics.compare_clips(frames, decoded) -- PSNR, SSIM, the largest difference: what the written file loses.
        rate (an encode.JpegRateConfig): the qualities are searched on the device so that the streams fit a byte budget (DESIGN
        8.15; cfg.quality is the ceiling); self.last_encode["rate"] holds the mode, the budget, the chosen qualities and the frames
        over budget, and with verify the figures state the loss at those qualities."""
        from .encode import JpegConfig, encode_jpeg, encode_report
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.dtype != torch.uint8 or frames.shape[-1] != 3:
            raise ValueError(f"encode: frames must be uint8 [F, H, W, 3], got {getattr(frames, 'dtype', type(frames))} "
                             f"{tuple(getattr(frames, 'shape', ()))}")
        cfg = JpegConfig() if cfg is None else cfg
        t0 = time.perf_counter()
        with torch.cuda.device(self.dev):
            on_dev = frames.to(self.dev)
            if verify:
                from .decode import decode_jpeg
                from .metrics import compare_clips
                buf, offs, lens, *info = encode_jpeg(on_dev, cfg, return_device=True, rate=rate, return_rate=rate is not None)
                raw = buf.cpu().numpy().tobytes()
                jpegs = [raw[o:o + n] for o, n in zip(offs.tolist(), lens.tolist())]
                m = compare_clips(on_dev.contiguous(), decode_jpeg((buf, offs, lens))).as_dict()
            elif rate is None:
                jpegs = encode_jpeg(on_dev, cfg)
            else:
                jpegs, *info = encode_jpeg(on_dev, cfg, rate=rate, return_rate=True)
        self.last_encode = encode_report(jpegs, cfg) if rate is None else encode_report(jpegs, cfg, rate, info[0])
        if verify:
            self.last_encode["verify"] = {"clip": m["clip"], "frames": {k: m["frames"][k] for k in ("psnr", "ssim", "max_abs")}}
        self._t("encode", t0)
        return jpegs

    def decode_jpegs(self, jpegs, frames=None, entropy: str = "segment", sub_bytes: int = 256, max_rounds: int = 32):
        """(Named decode_jpegs: decode is the VAE's, latent -> frames.)  Baseline JPEG streams (a list of `bytes`, or the device triple of encode_jpeg(return_device=True)) -> uint8 frames
        [F, H, W, 3] on the pipeline's device, equal to PIL's decode (landiff_amd.decode.decode_jpeg).  frames: the
        indices to decode.  entropy, sub_bytes, max_rounds: decode_jpeg's entropy route ("sync" / "auto": one lane per sub_bytes
        bytes of a restart segment, for streams without restart markers).  Timed as "decode"; the figures are
        self.last_decode."""
        from .decode import decode_jpeg
        t0 = time.perf_counter()
        report = {}
        with torch.cuda.device(self.dev):
            out = decode_jpeg(jpegs, self.dev, frames=frames, report=report, entropy=entropy, sub_bytes=sub_bytes, max_rounds=max_rounds)
        self.last_decode = report
        self._t("decode", t0)
        return out

    def _t(self, name, t0):
        torch.cuda.current_stream(self.dev).synchronize()      # (the stage's own stream: an overlapped AR decode keeps running)
        self.timings[name] = self.timings.get(name, 0.0) + time.perf_counter() - t0

    @torch.no_grad()
    def generate_tokens(self, inp: PromptInputs) -> torch.Tensor:
        """ArModelInferWrapper.forward: set_seed_for_single_process(seed) then Semantic1DLM.sample(seed=seed)."""
        torch.manual_seed(inp.seed)
        torch.cuda.manual_seed(inp.seed)
        return self.llm.sample(inp.llm_text_emb, motion_score=inp.motion_score, num_frames=self.cfg.llm.segment_length,
                               guidance_scale=inp.cfg, temperature=1.0, seed=inp.seed)

    @torch.no_grad()
    def generate_latent(self, tokens: torch.Tensor, inp: PromptInputs, noise: torch.Tensor | None = None) -> torch.Tensor:
        """CogWrapper.forward up to model.sample: seeds, semantic condition, sampler.  Returns [1,T,C,h,w] fp32."""
        d = self.cfg.dit
        torch.manual_seed(inp.seed)
        torch.cuda.manual_seed(inp.seed)
        t0 = time.perf_counter()
        sem = self.detok.semantic_condition(tokens.to(self.dev))
        self.dit.set_condition(inp.dit_context, sem)
        self._t("detokenize", t0)
        t0 = time.perf_counter()
        if noise is None:
            noise = torch.randn(1, d.latent_frames, d.in_channels, d.latent_h, d.latent_w, device=self.dev, dtype=torch.float32)
        z = self._sample(noise)
        self._t("dit", t0)
        return z

    def _sample(self, noise, **kw):
        """One sampler run over the DiT (set_condition() before it has emptied the step cache); with dit_cache its report is kept."""
        z = self.sampler.run(self.dit.step, noise, **kw)
        if self.dit_cache is not None:
            self.dit_cache_reports.append([dict(r) for r in self.dit.cache_report])
        if self.dit_guidance is not None:
            self.dit_guidance_reports.append([dict(r) for r in self.dit.guidance_report])
        return z

    def dit_guidance_report(self):
        """dit_guidance: what the last sampler run did -- one dict per step (index, timestep, cfg_scale, mode, cos, delta_rel_l1,
        delta_from; ControlDiTRunner.guidance_report).  None with the feature off or before the first run.
        self.dit_guidance_reports holds one report per sampler run, cleared where dit_cache_reports is."""
        return self.dit_guidance_reports[-1] if self.dit_guidance_reports else None

    def dit_cache_report(self):
        """dit_cache: what the step cache did in the last sampler run -- one dict per step (index, timestep, input_rel_l1, accumulated,
        computed, output_rel_l1; ControlDiTRunner.cache_report).  None with the cache off or before the first run.
        self.dit_cache_reports holds the report of every run of the last generate_samples / generate_many / generate_stream /
        extend_video call (one per sample, prompt or chunk; a streamed chunk is a sampler run of its own and starts with an empty
        cache), and of every generate_latent / __call__ since."""
        return self.dit_cache_reports[-1] if self.dit_cache_reports else None

    @torch.no_grad()
    def decode(self, latent: torch.Tensor, want_float: bool = False):
        t0 = time.perf_counter()
        lat = latent.to(torch.bfloat16).float()        # samples.to(self.dtype) (diffusion_video.py:314)
        out = self.vae.decode(lat, want_float=want_float)
        self._t("vae", t0)
        return out

    @torch.no_grad()
    def __call__(self, inp: PromptInputs, want_float: bool = False):
        """prompt embeddings -> uint8 frames [4T-3, H, W, 3] in device memory (BASELINE metric region)."""
        t0 = time.perf_counter()
        tokens = self.generate_tokens(inp)
        self._t("llm", t0)
        z = self.generate_latent(tokens, inp)
        return self.decode(z, want_float=want_float)

    @torch.no_grad()
    def generate_samples(self, inp: PromptInputs, seeds, keep: int | None = None, want_float: bool = False,
                         engine: str = "gemv") -> list:
        """Several candidates of one prompt: result i is identical to `self(replace(inp, seed=seeds[i]))`.  The AR decode of all
        seeds is one LLMRunner.sample_many (the LLM's weights streamed once per step for all of them; needs
        LanDiffPipeline(..., max_samples >= len(seeds)) and non-zero seeds); detokenize, DiT and VAE then run per sample.
        keep=k (1 <= k <= len(seeds)): best-of-N.  The decode also returns every candidate's total log-probability under the
        distribution it was sampled from (sample_many(return_logprobs=True)), the candidates are ranked by it (rank_candidates)
        and detokenize, DiT and VAE run for the k most likely only -> [(seed, score, frames)] in rank order, frames what the
        keep=None call returns for that seed.  self.last_candidates keeps every candidate: {"seeds", "tokens" [N, n_visual],
        "scores" [N], "order"}.  Whether likelihood rank tracks visual quality is not measured.
        engine="mfma": the decode runs on the MFMA engine (sample_many(engine="mfma"); needs LanDiffPipeline(..., wide_samples >=
        len(seeds)), up to 16 seeds).  Result i is then identical to the ONE-seed call generate_samples(inp, [seeds[i]],
        engine="mfma") -- whatever the other seeds are -- and equals `self(replace(inp, seed=seeds[i]))` only up to the first
        near-tie of the draw that the engines' different summation orders decide differently."""
        from dataclasses import replace
        seeds = [int(s) for s in seeds]
        self.dit_cache_reports = []
        self.dit_guidance_reports = []
        if keep is not None and not 1 <= int(keep) <= len(seeds):
            raise ValueError(f"generate_samples: keep={keep} outside [1, {len(seeds)}] (the number of seeds)")
        kw = dict(motion_score=inp.motion_score, num_frames=self.cfg.llm.segment_length, guidance_scale=inp.cfg, temperature=1.0,
                  engine=engine)
        t0 = time.perf_counter()
        if keep is None:
            tokens = self.llm.sample_many(inp.llm_text_emb, seeds, **kw)
            self._t("llm", t0)
            return [self.decode(self.generate_latent(tokens[i], replace(inp, seed=s)), want_float=want_float)
                    for i, s in enumerate(seeds)]
        tokens, logprobs = self.llm.sample_many(inp.llm_text_emb, seeds, return_logprobs=True, **kw)
        scores = logprobs.double().sum(1).tolist()
        self._t("llm", t0)
        order = rank_candidates(scores)
        self.last_candidates = {"seeds": seeds, "tokens": tokens.clone(), "scores": scores, "order": order}
        return [(seeds[i], scores[i], self.decode(self.generate_latent(tokens[i], replace(inp, seed=seeds[i])), want_float=want_float))
                for i in order[:int(keep)]]

    @torch.no_grad()
    def score_tokens(self, inp: PromptInputs, tokens: torch.Tensor):
        """How well the prompt explains a token sequence: LLMRunner.score of `tokens` (one segment's ids, as generate_tokens
        returns them) under the distribution generate_tokens samples from for this prompt -> (logprobs [n_visual], total)."""
        return self.llm.score(inp.llm_text_emb, tokens, motion_score=inp.motion_score, num_frames=self.cfg.llm.segment_length,
                              guidance_scale=inp.cfg, temperature=1.0)

    @torch.no_grad()
    def score_clip(self, inp: PromptInputs, frames: torch.Tensor):
        """score_tokens of a real clip's ids (tokenize_frames: needs the Theia extractor, and fails as that method does)."""
        return self.score_tokens(inp, self.tokenize_frames(frames))

    # ---- several prompts on one GPU: prompt-level software pipeline ---------------------------------------
    @torch.no_grad()
    def generate_many(self, inputs: list, want_float: bool = False) -> list:
        """Frames for a list of prompts, each identical to what `self(inp)` returns for it, with the AR token decode of
        prompt i+1 issued from a helper thread on a second, high-priority HIP stream while prompt i is in detokenize / DiT /
        VAE on the current stream.

        Why it pays on MI355X: the DiT loop runs at the package power cap (1390 W) and is bound by energy, the AR decode
        is a chain of short HBM-bound launches at 980 W; next to each other the decode costs only its incremental energy
        (measured: 16.9 s for the pair of stages instead of 1.67 + 16.1 s, tools/overlap_prompts_probe.py).  No kernel
        changes: the hardware interleaves the decode's workgroups as the MFMA kernels' workgroups retire.

        RNG: the decode draws from its own generator seeded with the prompt's seed (as Semantic1DLM.sample(seed=...) does,
        lm_model.py:398-402) and never touches the default generator, which stays with the sampler of the prompt in flight --
        so per-prompt results do not depend on the overlap.  Stage timings are not recorded here (they would need
        device-wide synchronisation between the stages)."""
        from concurrent.futures import ThreadPoolExecutor
        if not inputs:
            return []
        self.dit_cache_reports = []
        self.dit_guidance_reports = []
        for inp in inputs:
            assert inp.seed, "generate_many needs a non-zero seed per prompt (a zero seed would draw from the shared default generator)"
        side = torch.cuda.Stream(device=self.dev, priority=-1)
        main = torch.cuda.current_stream(self.dev)

        def decode_tokens(inp):
            torch.cuda.set_device(self.dev)
            with torch.cuda.stream(side):
                tok = self.llm.sample(inp.llm_text_emb, motion_score=inp.motion_score, num_frames=self.cfg.llm.segment_length,
                                      guidance_scale=inp.cfg, temperature=1.0, seed=inp.seed,
                                      mode="chain").clone()   # (the runner reuses its token buffer; mode="chain": the decode runs under the DiT loop)
                tok.record_stream(main)               # allocated on the side stream, read on the main one: keep the block until that read is done
                side.synchronize()                    # the tokens are complete before any other stream reads them
            return tok

        def submit(pool, inp):
            # The decode reads the prompt embedding (and the LLM's buffers) on the side stream: order it after everything the
            # caller has queued on the current stream so far -- e.g. a text encoder that has just produced inp.llm_text_emb.
            side.wait_stream(main)
            return pool.submit(decode_tokens, inp)

        out = []
        with ThreadPoolExecutor(max_workers=1) as pool:
            fut = submit(pool, inputs[0])
            for i, inp in enumerate(inputs):
                tokens = fut.result()
                if i + 1 < len(inputs):
                    fut = submit(pool, inputs[i + 1])
                d = self.cfg.dit
                torch.manual_seed(inp.seed)
                torch.cuda.manual_seed(inp.seed)
                sem = self.detok.semantic_condition(tokens.to(self.dev))
                self.dit.set_condition(inp.dit_context, sem)
                noise = torch.randn(1, d.latent_frames, d.in_channels, d.latent_h, d.latent_w, device=self.dev, dtype=torch.float32)
                z = self._sample(noise)
                out.append(self.vae.decode(z.to(torch.bfloat16).float(), want_float=want_float))
        return out

    @torch.no_grad()
    def generate_batch(self, inputs: list, rank: int = 0, world: int = 1) -> list:
        """A batch of prompts data-parallel over the GPUs of a node (BASELINE configs[3]; the reference's only hook is
        LOCAL_RANK -> set_device, infer_video.py:109-110): this rank runs prompts rank, rank + world, ... through
        generate_many (per-prompt seeds, so a prompt's frames do not depend on the number of GPUs) and one RCCL all_gather
        returns every prompt's uint8 frames, in prompt order, on every rank."""
        mine = shard_prompts(len(inputs), rank, world)
        local = self.generate_many([inputs[i] for i in mine])
        return gather_prompt_frames(local, len(inputs), rank, world)

    # ---- streaming long video (BASELINE config 3) --------------------------------
    def stream_plan(self, n_chunks: int, prefix_frames: int):
        """(latent frames per chunk, new latent frames per later chunk, LLM segments needed)."""
        return stream_plan(self.cfg, n_chunks, prefix_frames)

    def _sem_windows(self, seg_tokens, T: int):
        """sem_window(f0, f1): latent frames [f0, f1) of the concatenated per-segment semantic features; a segment is detokenized
        (and timed) when a window first needs it.  seg_tokens(s) -> segment s's token ids."""
        sem_seg = {}               # segment -> semantic features [T, C, H, W]
        def sem_window(f0, f1):
            parts = []
            for sidx in range(f0 // T, (f1 - 1) // T + 1):
                if sidx not in sem_seg:
                    tok = seg_tokens(sidx)                 # (overlapped decode: blocks until the segment's last token is queued)
                    t1 = time.perf_counter()
                    sem_seg[sidx] = self.detok.semantic_condition(tok)
                    self._t("detokenize", t1)
                lo, hi = max(f0, sidx * T) - sidx * T, min(f1, (sidx + 1) * T) - sidx * T
                parts.append(sem_seg[sidx][lo:hi])
            return torch.cat(parts, dim=0).contiguous()
        return sem_window

    def _stream_chunk(self, inp: PromptInputs, c: int, sem, noise, prev, prefix_frames: int, randn_like, want_float: bool,
                      keep: bool, latents_out=None):
        """Chunk c of a stream: seed inp.seed + c, the sampler on semantic window `sem` (prefix = the last `prefix_frames`
        latents of `prev`, the previous chunk's bf16 latent, unless prev is None), then the VAE decode of its new latent frames
        against the causal-conv caches the previous chunk left (kept for the next chunk when `keep`).  -> (latent, frames)."""
        d = self.cfg.dit
        T = d.latent_frames
        t0 = time.perf_counter()
        torch.manual_seed(inp.seed + c); torch.cuda.manual_seed(inp.seed + c)
        self.dit.set_condition(inp.dit_context, sem)
        noise = noise.to(self.dev) if noise is not None else torch.randn(
            1, T, d.in_channels, d.latent_h, d.latent_w, device=self.dev, dtype=torch.float32)
        if prev is None:
            z = self._sample(noise, randn_like=randn_like)
        else:
            z = self._sample(noise, randn_like=randn_like, prefix=prev[:, T - prefix_frames:], fixed_frames=prefix_frames)
        first = prev is None
        prev = z.to(torch.bfloat16).float()              # samples.to(self.dtype) (diffusion_video.py:314)
        if latents_out is not None:
            latents_out.append(prev.clone())
        self._t("dit", t0)
        t0 = time.perf_counter()
        lat = prev if first else prev[:, prefix_frames:]
        r = self.vae.decode(lat, want_float=want_float, stream_continue=not first, stream_keep=keep)
        self._t("vae", t0)
        return prev, r

    @torch.no_grad()
    def generate_stream(self, inp: PromptInputs, n_chunks: int, prefix_frames: int = STREAM_PREFIX_FRAMES, want_float: bool = False,
                        tokens: torch.Tensor | None = None, noises=None, randn_like=torch.randn_like, overlap_decode: bool = True,
                        latents_out: list | None = None):
        """Chunked long-video generation out of the reference's streaming primitives -- the reference ships the pieces
        (yaml :213,231 "fixed_frames: 7 # 49 frames, 13 latent, prefix_length=7"), not the loop:
          * ONE multi-segment AR decode (Semantic1DLM.sample with num_frames = n_seg * segment_length, lm_model.py:278-291,
            361-396): the KV cache carries over the segments, tokens never leave the device;
          * per segment detokenize + upsample -> semantic features for all latent frames, resident in HBM;
          * chunk c > 0: CogWrapper.forward(vae_feature_prefix = last `prefix_frames` latents of chunk c-1)
            (dif_infer.py:159,232; diffusion_video.py:287-288) with the sampler pinning those frames
            (sampling.py:800-835), conditioned on the semantic-feature window of its 13 latent frames;
          * the new latent frames are decoded against the VAE's causal-conv caches of the previous chunk
            (cp_enc_dec.py:436-466), which stay in HBM.
        Chunk c is seeded with inp.seed + c.  Returns uint8 frames [4T-3 + (n_chunks-1)*4*new, H, W, 3] (+ fp32 video).
        latents_out: a list that receives every chunk's sampled latent [1, T, C, h, w] (fp32 values of the bf16 result), for tests."""
        d, lc = self.cfg.dit, self.cfg.llm
        T, new, n_seg = self.stream_plan(n_chunks, prefix_frames)
        per_seg = self.cfg.tok.num_latent_tokens
        self.dit_cache_reports = []
        self.dit_guidance_reports = []
        t0 = time.perf_counter()
        seg_tokens = None          # segment s -> its token ids, int64 [per_seg] on the device
        decode_thread = None
        if tokens is None and overlap_decode and inp.seed:
            # The multi-segment AR decode runs on a second, high-priority stream issued by a helper thread; chunk c only needs
            # the segments its 13 latent frames fall into, so the DiT loop of the first chunk starts as soon as segment 0 is
            # decoded and the later segments are decoded underneath it (980 W of HBM-bound launches next to the power-capped
            # MFMA kernels: see generate_many).  The decode draws from its own generator (seed given), so the tokens equal
            # those of the serial path.
            import threading
            side = torch.cuda.Stream(device=self.dev, priority=-1)
            queued = [threading.Event() for _ in range(n_seg)]
            done = [torch.cuda.Event() for _ in range(n_seg)]
            def on_segment(sidx):
                done[sidx].record(side)
                queued[sidx].set()
            decode_state = {"t_start": time.perf_counter()}
            def run_decode():
                try:
                    torch.cuda.set_device(self.dev)
                    with torch.cuda.stream(side):
                        self.llm.sample(inp.llm_text_emb, motion_score=inp.motion_score, num_frames=n_seg * lc.segment_length,
                                        guidance_scale=inp.cfg, temperature=1.0, seed=inp.seed, on_segment=on_segment, segment_tokens=per_seg,
                                        mode="chain")
                        side.synchronize()
                    decode_state["seconds"] = time.perf_counter() - decode_state["t_start"]
                except BaseException as e:              # never leave the consumer waiting on a segment that will not come
                    decode_state["error"] = e
                    for ev in queued:
                        ev.set()
            side.wait_stream(torch.cuda.current_stream(self.dev))     # the decode reads inp.llm_text_emb: after whatever produced it
            decode_thread = threading.Thread(target=run_decode)
            decode_thread.start()
            def seg_tokens(sidx):
                queued[sidx].wait()
                if "error" in decode_state:
                    raise decode_state["error"]
                torch.cuda.current_stream(self.dev).wait_event(done[sidx])
                return self.llm.out_tokens[sidx * per_seg:(sidx + 1) * per_seg].clamp(0, lc.visual_vocab - 1)
        else:
            if tokens is None:
                torch.manual_seed(inp.seed); torch.cuda.manual_seed(inp.seed)
                tokens = self.llm.sample(inp.llm_text_emb, motion_score=inp.motion_score, num_frames=n_seg * lc.segment_length,
                                         guidance_scale=inp.cfg, temperature=1.0, seed=inp.seed)
            self._t("llm", t0)
            tokens = tokens.to(self.dev).reshape(n_seg, per_seg)
            seg_tokens = lambda sidx: tokens[sidx]
        sem_window = self._sem_windows(seg_tokens, T)
        outs, vids, prev = [], [], None
        for c in range(n_chunks):
            t_w = time.perf_counter()
            d0 = self.timings.get("detokenize", 0.0)
            sem = sem_window(c * new, c * new + T)             # (may wait on the overlapped decode; detokenize is timed inside)
            wait = time.perf_counter() - t_w - (self.timings.get("detokenize", 0.0) - d0)
            if decode_thread is not None:
                self.timings["segment_wait"] = self.timings.get("segment_wait", 0.0) + wait
            prev, r = self._stream_chunk(inp, c, sem, noises[c] if noises is not None else None, prev, prefix_frames, randn_like,
                                         want_float, keep=c < n_chunks - 1, latents_out=latents_out)
            if want_float:
                outs.append(r[0]); vids.append(r[1])
            else:
                outs.append(r)
        if decode_thread is not None:
            decode_thread.join()
            if "error" in decode_state:
                raise decode_state["error"]
            self.timings["llm_overlapped"] = self.timings.get("llm_overlapped", 0.0) + decode_state["seconds"]   # wall time of the decode thread
        frames = torch.cat(outs, dim=0)
        return (frames, torch.cat(vids, dim=1)) if want_float else frames


    # ---- continuation of a given clip ------------------------------------------------------------------
    @torch.no_grad()
    def extend_video(self, inp: PromptInputs, n_chunks: int, *, frames: torch.Tensor | None = None,
                     clip_latent: torch.Tensor | None = None, clip_tokens: torch.Tensor | None = None,
                     tokens: torch.Tensor | None = None, prefix_frames: int = STREAM_PREFIX_FRAMES, want_float: bool = False, noises=None,
                     latents_out: list | None = None, conform: ConformConfig | None = None):
        """Continues a given clip: the clip is chunk 0 of a generate_stream run, and chunks 1..n_chunks are produced exactly as
        generate_stream(inp, n_chunks + 1, prefix_frames, ...) produces its chunks 1.. (seed inp.seed + k, semantic window
        [k new, k new + T), prefix = the last `prefix_frames` latents of the previous chunk, decode against the VAE caches).

        The clip latent (exactly one of the two): `clip_latent` [1, T, 16, h, w] as given, or `frames` uint8 [F >= 4T-3, 8h, 8w, 3] whose LAST 4T-3
        frames are encoded (VAEEncoder: scale_factor * posterior.sample(), the sample drawn on the device's generator seeded
        with inp.seed, as encode_first_stage does -- diffusion_video.py:233-254); it is rounded to bf16 like a sampled latent.
        Its T latent frames are decoded once (frames discarded) to prime the decoder's causal-conv caches.

        Semantic tokens (at most one of the two): `tokens` = every segment's ids (n_seg * num_latent_tokens, as generate_stream takes them); otherwise
        one multi-segment AR decode from the prompt, with segment 0 forced to `clip_tokens` (int64 [num_latent_tokens], e.g.
        the .npy llm_infer saves next to a video) when given.  clip_tokens="from_frames": the clip's own tokens, from the Theia
        extractor (`theia`) on T frames of the encoded window picked as CogWrapper._semantic_from_video picks them (linspace),
        timed as "theia".  Without clip_tokens every segment is sampled from the prompt: the prefix frames' control features
        then come from the prompt, not from the clip.

        `noises[k-1]` is chunk k's initial noise.  Returns the NEW frames only, uint8 [n_chunks * 4 new, H, W, 3] (new =
        T - prefix_frames), plus the fp32 video [3, frames, H, W] when want_float.  latents_out receives every new chunk's latent.

        conform (a conform.ConformConfig with fit "cover" / "stretch"): `frames` may have any size and frame rate -- they go through
        the conform stage first (timed as "conform"; what it did is self.last_conform, its output self.last_conform_frames) and
        everything after sees the 4T-3 frames of 8h x 8w it made.  None or fit="exact": nothing is resized, as above."""
        d, lc = self.cfg.dit, self.cfg.llm
        T, new, n_seg = self.stream_plan(n_chunks + 1, prefix_frames)
        per_seg = self.cfg.tok.num_latent_tokens
        self.dit_cache_reports = []
        self.dit_guidance_reports = []
        if (frames is None) == (clip_latent is None):
            raise ValueError("extend_video takes the clip as exactly one of frames and clip_latent")
        if tokens is not None and clip_tokens is not None:
            raise ValueError("extend_video: tokens already holds every segment; clip_tokens goes with a decode from the prompt")
        if conform is not None and conform.fit != "exact":
            frames, _ = self._conform(frames, conform)
        if isinstance(clip_tokens, str):
            if clip_tokens != "from_frames":
                raise ValueError(f"extend_video: clip_tokens must be a tensor or 'from_frames', got {clip_tokens!r}")
            if frames is None or self.theia is None:
                raise ValueError("extend_video(clip_tokens='from_frames') needs frames= and a pipeline built with theia=")
            t0 = time.perf_counter()
            clip_tokens = self.tokenize_frames(continuation_window(frames, self.cfg))
            self._t("theia", t0)
        if clip_latent is None:
            window = continuation_window(frames, self.cfg)
            if self.encoder is None:
                raise ValueError("extend_video(frames=...) needs the VAE encoder's weights ('encoder.*' in the VAE state)")
            t0 = time.perf_counter()
            torch.manual_seed(inp.seed); torch.cuda.manual_seed(inp.seed)
            clip_latent = self.encoder.encode(window.to(self.dev), sample=True)
            self._t("vae_encode", t0)
        if tuple(clip_latent.shape) != (1, T, d.in_channels, d.latent_h, d.latent_w):
            raise ValueError(f"clip_latent must be [1, {T}, {d.in_channels}, {d.latent_h}, {d.latent_w}], got {tuple(clip_latent.shape)}")
        if self.encoder is not None:
            self.encoder.release()                        # its windows (13 GB at 480 x 720) are not needed by the DiT loop
        prev = clip_latent.to(self.dev).to(torch.bfloat16).float()
        t0 = time.perf_counter()
        self.vae.decode(prev, stream_keep=True)           # chunk 0's decode: the caches generate_stream holds after it
        self._t("vae", t0)
        if tokens is None:
            t0 = time.perf_counter()
            torch.manual_seed(inp.seed); torch.cuda.manual_seed(inp.seed)
            tokens = self.llm.sample(inp.llm_text_emb, motion_score=inp.motion_score, num_frames=n_seg * lc.segment_length,
                                     guidance_scale=inp.cfg, temperature=1.0, seed=inp.seed, prefix_tokens=clip_tokens)
            self._t("llm", t0)
        tokens = tokens.to(self.dev).reshape(n_seg, per_seg)
        sem_window = self._sem_windows(lambda sidx: tokens[sidx], T)
        outs, vids = [], []
        for k in range(1, n_chunks + 1):
            prev, r = self._stream_chunk(inp, k, sem_window(k * new, k * new + T), noises[k - 1] if noises is not None else None,
                                         prev, prefix_frames, torch.randn_like, want_float, keep=k < n_chunks,
                                         latents_out=latents_out)
            if want_float:
                outs.append(r[0]); vids.append(r[1])
            else:
                outs.append(r)
        out = torch.cat(outs, dim=0)
        return (out, torch.cat(vids, dim=1)) if want_float else out


    # ---- editing a given clip --------------------------------------------------------------------------
    @torch.no_grad()
    def edit_video(self, inp: PromptInputs, *, frames: torch.Tensor | None = None, clip_latent: torch.Tensor | None = None,
                   strength: float = 1.0, keep_mask: torch.Tensor | None = None, tokens: torch.Tensor | None = None,
                   clip_tokens: str | None = None, known_noise: bool = True, composite: bool = True,
                   noise: torch.Tensor | None = None, want_float: bool = False, latents_out: list | None = None,
                   conform: ConformConfig | None = None):
        """Changes a given clip, training-free: an SDEdit start (`strength` < 1: the sampler begins at step start =
        edit_start_step(num_steps, strength) from alpha[start] * clip latent + sigma[start] * noise and runs the remaining steps) and /
        or masked inpainting (`keep_mask`: the marked cells are held on the clip's own trajectory, the rest is generated) -- the
        sampler's start / known / known_mask arguments (DiffusionSampler.run) over one chunk.  DESIGN 8.8.

        The clip (exactly one of the two): `frames` uint8 [4T-3, 8h, 8w, 3], exactly that shape (no resizing), encoded as extend_video
        encodes its window (posterior sample on the device's generator seeded with inp.seed, rounded to bf16); or `clip_latent`
        [1, T, 16, h, w], rounded to bf16 likewise.

        Semantic tokens: `tokens` as given; clip_tokens="from_frames": the clip's own Theia tokens (needs frames= and theia=; timed
        as "theia") -- the clip's layout and motion, re-rendered under the prompt; neither: generate_tokens(inp), from the prompt.

        keep_mask: bool, True = keep the clip; [4T-3, 8h, 8w] in pixels (a latent cell is kept only if every pixel of its block is:
        ld_mask_to_latent) or [T, h, w] in latent cells.  All True is refused (nothing left to edit), all False is no mask.
        known_noise=False pins the kept cells to the clean clip latent at every step instead of its re-noised version.  With a pixel
        mask, frames= and `composite`, the kept pixels of the returned uint8 frames are the clip's own (the fp32 video of want_float
        is the decoder's output as it is).

        The run is generate_latent's: seeds, semantic condition, the same initial-noise draw (or `noise`), the sampler, the decode;
        strength 1.0 without a mask returns what self.decode(self.generate_latent(tokens, inp)) returns.  -> uint8 frames [4T-3, 8h,
        8w, 3] (+ the fp32 video when want_float; with an even T the decoder leaves the last latent frame undecoded, as in
        generation, and the composite covers the frames it returns).  latents_out receives the sampled latent (fp32 values of the bf16 result);
        self.last_edit says what ran: strength, start_step, steps_run, alpha_start, sigma_start, kept_cells, total_cells,
        tokens_source.  With dit_cache / dit_guidance the reports have steps_run rows whose index begins at start_step;
        attn_window's dense_steps counts executed steps.

        conform (a conform.ConformConfig with fit "cover" / "stretch"): `frames` of any size and frame rate, and a bool keep_mask
        [F, Hs, Ws] in that clip's own geometry, go through the conform stage first (timed as "conform"; self.last_conform,
        self.last_conform_frames): the call then equals edit_video(frames=conform_clip(frames, plan), keep_mask=conform_mask(
        keep_mask, plan)) bit for bit, and the composite uses the conformed clip.  None or fit="exact": nothing is resized."""
        d = self.cfg.dit
        T, S = d.latent_frames, len(self.sampler.plan)
        shape = (1, T, d.in_channels, d.latent_h, d.latent_w)
        self.dit_cache_reports = []
        self.dit_guidance_reports = []
        if (frames is None) == (clip_latent is None):
            raise ValueError("edit_video takes the clip as exactly one of frames and clip_latent")
        if tokens is not None and clip_tokens is not None:
            raise ValueError("edit_video: tokens already holds the clip's segment; clip_tokens='from_frames' computes it instead")
        if clip_tokens is not None and clip_tokens != "from_frames":
            raise ValueError(f"edit_video: clip_tokens must be None or 'from_frames', got {clip_tokens!r}")
        if clip_tokens == "from_frames" and (frames is None or self.theia is None):
            raise ValueError("edit_video(clip_tokens='from_frames') needs frames= and a pipeline built with theia=")
        start = edit_start_step(S, strength)
        if conform is not None and conform.fit != "exact":
            frames, keep_mask = self._conform(frames, conform, keep_mask)
        if frames is not None:
            frames = edit_clip(frames, self.cfg)
            if self.encoder is None:
                raise ValueError("edit_video(frames=...) needs the VAE encoder's weights ('encoder.*' in the VAE state)")
        elif tuple(clip_latent.shape) != shape:
            raise ValueError(f"clip_latent must be [1, {T}, {d.in_channels}, {d.latent_h}, {d.latent_w}], got {tuple(clip_latent.shape)}")
        mask, mask_px = None, None
        if keep_mask is not None:
            px, lat = (4 * T - 3, 8 * d.latent_h, 8 * d.latent_w), (T, d.latent_h, d.latent_w)
            if keep_mask.dtype != torch.bool or tuple(keep_mask.shape) not in (px, lat):
                raise ValueError(f"keep_mask must be bool [{px[0]}, {px[1]}, {px[2]}] (pixels) or [{lat[0]}, {lat[1]}, {lat[2]}] "
                                 f"(latent cells), got {keep_mask.dtype} {tuple(keep_mask.shape)}")
            keep_mask = keep_mask.to(self.dev).contiguous()
            if tuple(keep_mask.shape) == px:
                mask_px = keep_mask
                mask = ops.mask_to_latent(mask_px)
            else:
                mask = keep_mask.to(torch.uint8)
            kept = int(mask.sum())
            if kept == mask.numel():
                raise ValueError("edit_video: keep_mask keeps every latent cell: nothing is left to edit")
            if kept == 0:
                mask = None
        if clip_tokens == "from_frames":
            t0 = time.perf_counter()
            tokens = self.tokenize_frames(frames)
            self._t("theia", t0)
            source = "from_frames"
        elif tokens is not None:
            source = "given"
        else:
            t0 = time.perf_counter()
            tokens = self.generate_tokens(inp)
            self._t("llm", t0)
            source = "prompt"
        if frames is not None:
            t0 = time.perf_counter()
            torch.manual_seed(inp.seed); torch.cuda.manual_seed(inp.seed)
            clip_latent = self.encoder.encode(frames.to(self.dev), sample=True)
            self._t("vae_encode", t0)
        if self.encoder is not None:
            self.encoder.release()                        # its windows (13 GB at 480 x 720) are not needed by the DiT loop
        z0 = clip_latent.to(self.dev).to(torch.bfloat16).float().contiguous()
        torch.manual_seed(inp.seed)
        torch.cuda.manual_seed(inp.seed)
        t0 = time.perf_counter()
        sem = self.detok.semantic_condition(tokens.to(self.dev))
        self.dit.set_condition(inp.dit_context, sem)
        self._t("detokenize", t0)
        t0 = time.perf_counter()
        noise = noise.to(self.dev) if noise is not None else torch.randn(*shape, device=self.dev, dtype=torch.float32)
        z = self._sample(noise, start=start, known=z0, known_mask=mask, known_noise=known_noise)
        self._t("dit", t0)
        alpha, sigma = self.sampler.alphas[start]
        self.last_edit = dict(strength=float(strength), start_step=start, steps_run=S - start, alpha_start=alpha, sigma_start=sigma,
                              kept_cells=int(mask.sum()) if mask is not None else 0, total_cells=T * d.latent_h * d.latent_w,
                              tokens_source=source)
        if latents_out is not None:
            latents_out.append(z.to(torch.bfloat16).float())
        out = self.decode(z, want_float=want_float)
        if composite and mask_px is not None and frames is not None:
            edited = out[0] if want_float else out
            n = edited.shape[0]           # (4T-3; an even T leaves its last latent frame undecoded, as in generation: VAEDecoder.decode)
            edited = torch.where(mask_px[:n, :, :, None], frames[:n].to(self.dev), edited)      # uint8 select (plumbing)
            out = (edited, out[1]) if want_float else edited
        return out

    @torch.no_grad()
    def tokenize_frames(self, frames: torch.Tensor) -> torch.Tensor:
        """uint8 frames [F, H, W, 3] -> the clip's semantic token ids int64 [num_latent_tokens]: T = tok.temporal equally spaced
        frames (theia.select_frames) through the Theia extractor and the tokenizer encoder."""
        from .theia import select_frames
        if self.theia is None:
            raise ValueError("tokenize_frames needs a pipeline built with theia= (landiff_amd.theia.TheiaExtractor)")
        if self.theia.encoder is None:
            raise ValueError("tokenize_frames: the Theia extractor has no tokenizer encoder attached")
        return self.theia.tokenize_video(select_frames(frames.to(self.dev), self.cfg.tok.temporal))


def rank_candidates(scores) -> list:
    """Indices of `scores` (total log-probabilities) from most to least likely.  Ties go to the lower index; a score that is
    not finite (-inf: a filter removed one of the ids; NaN) ranks after every finite one, again by index."""
    import math
    vals = [float(v) for v in scores]
    return sorted(range(len(vals)), key=lambda i: (0, -vals[i], i) if math.isfinite(vals[i]) else (1, 0.0, i))


def write_scores_json(path: str, seeds, scores, kept) -> list:
    """<name>_scores.json of infer_video --keep: [{index, seed, logprob, kept}] for every candidate, in candidate order (a score
    that is not finite is written as null: JSON has no infinity)."""
    import json
    import math
    kept = set(int(i) for i in kept)
    rows = [{"index": i, "seed": int(s), "logprob": float(v) if math.isfinite(float(v)) else None, "kept": i in kept}
            for i, (s, v) in enumerate(zip(seeds, scores))]
    with open(path, "w") as f:
        json.dump(rows, f, indent=1)
    return rows


def edit_start_step(S: int, strength: float) -> int:
    """The sampler step LanDiffPipeline.edit_video starts at: of S steps the last n_run = floor(strength * S + 0.5) run, so
    start = S - n_run (strength 1.0: 0, a fresh run).  strength must lie in (0, 1] and run at least one step."""
    import math
    strength = float(strength)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"edit strength must be in (0, 1], got {strength!r}")
    n_run = math.floor(strength * S + 0.5)
    if n_run < 1:
        raise ValueError(f"edit strength {strength!r} runs no step of {S}: the smallest strength that runs one step is {0.5 / S!r}")
    return S - n_run


def edit_clip(frames, cfg: PipelineConfig):
    """The clip LanDiffPipeline.edit_video takes: uint8 frames [4T-3, 8 latent_h, 8 latent_w, 3], exactly (T = cfg.dit.latent_frames:
    49 frames of 480 x 720 in the shipped config).  Anything else raises ValueError with the expected shape; nothing is resized."""
    d = cfg.dit
    want = (4 * d.latent_frames - 3, 8 * d.latent_h, 8 * d.latent_w, 3)
    if frames.dtype != torch.uint8 or tuple(frames.shape) != want:
        raise ValueError(f"edit_video: clip frames must be uint8 [{want[0]}, {want[1]}, {want[2]}, 3], got {frames.dtype} "
                         f"{tuple(frames.shape)} (one chunk, not resized)")
    return frames


def write_edit_json(path: str, last_edit: dict) -> dict:
    """<name>_edit.json of infer_video --edit_video: LanDiffPipeline.last_edit (a float that is not finite is written as null: JSON
    has no infinity)."""
    import json
    import math
    row = {k: (None if isinstance(v, float) and not math.isfinite(v) else v) for k, v in last_edit.items()}
    with open(path, "w") as f:
        json.dump(row, f, indent=1, allow_nan=False)
    return row


def stream_plan(cfg: PipelineConfig, n_chunks: int, prefix_frames: int):
    """(latent frames per chunk, new latent frames per later chunk, LLM segments needed) of an n_chunks stream."""
    T, seg = cfg.dit.latent_frames, cfg.llm.segment_length
    new = T - prefix_frames
    assert 0 < prefix_frames < T and new % 2 == 0, "later chunks decode their new latent frames in pairs"
    total = T + (n_chunks - 1) * new
    return T, new, -(-total // seg)


def continuation_window(frames, cfg: PipelineConfig):
    """The clip frames LanDiffPipeline.extend_video encodes: the LAST 4T-3 of uint8 frames [F, 8 latent_h, 8 latent_w, 3]
    (T = cfg.dit.latent_frames: 49 of a 480 x 720 clip in the shipped config).  A shorter clip, another frame size, dtype or
    layout raises ValueError (resizing is not done here)."""
    d = cfg.dit
    n = 4 * d.latent_frames - 3
    want = (8 * d.latent_h, 8 * d.latent_w, 3)
    if frames.dim() != 4 or tuple(frames.shape[1:]) != want:
        raise ValueError(f"clip frames must be [F, {want[0]}, {want[1]}, 3], got {tuple(frames.shape)}")
    if frames.dtype != torch.uint8:
        raise ValueError(f"clip frames must be uint8, got {frames.dtype}")
    if frames.shape[0] < n:
        raise ValueError(f"a clip of {frames.shape[0]} frames is too short: continuation encodes its last {n} frames "
                         f"({d.latent_frames} latent frames)")
    return frames[frames.shape[0] - n:]


def synthetic_inputs(cfg: PipelineConfig, device, n_text: int = 64, seed: int = 42) -> PromptInputs:
    """Synthetic prompt embeddings: N(0,1), seeds 42 / 43."""
    g = torch.Generator().manual_seed(seed)
    llm_text = torch.randn(n_text, cfg.llm.text_dim, generator=g)
    g2 = torch.Generator().manual_seed(seed + 1)
    ctx = torch.randn(1, cfg.dit.text_len, cfg.dit.text_dim, generator=g2)
    return PromptInputs(llm_text.to(device), ctx.to(device), seed=seed)


# ------------------------------------------------------------------------------------------------
# prompt-batch data parallelism (one process per GPU; the only collective is the final gather)
# ------------------------------------------------------------------------------------------------
def shard_prompts(n_prompts: int, rank: int, world: int) -> list[int]:
    """Rank r processes prompts r, r+world, ...; each keeps the user's seed, so a prompt's result
    does not depend on the number of GPUs."""
    return list(range(rank, n_prompts, world))


def gather_frames(frames: torch.Tensor, world: int, force: bool = False):
    """all_gather of uint8 frames [n_local, T, H, W, 3] over RCCL/xGMI (gloo on CPU in tests).
    force: issue the collective even for a single rank (exercises the RCCL path on a 1-GPU box)."""
    import torch.distributed as dist
    if not dist.is_initialized() or (world == 1 and not force):
        return [frames]
    out = [torch.empty_like(frames) for _ in range(world)]
    dist.all_gather(out, frames.contiguous())
    return out


def gather_prompt_frames(local_frames: list, n_prompts: int, rank: int, world: int, force: bool = False) -> list:
    """The final gather of a prompt batch (BASELINE configs[3]): rank r holds the uint8 frames [T, H, W, 3] of prompts
    shard_prompts(n_prompts, r, world), in that order; every rank gets back the frames of ALL prompts in prompt order.
    Shards may be uneven (n_prompts not a multiple of world): the short ranks pad with one zero video, which is dropped again.
    One all_gather per batch -- the only collective of the data-parallel path."""
    mine = shard_prompts(n_prompts, rank, world)
    assert len(local_frames) == len(mine), (len(local_frames), len(mine))
    per_rank = -(-n_prompts // world)
    if not local_frames and per_rank == 0:
        return []
    ref = local_frames[0] if local_frames else None
    import torch.distributed as dist
    live = dist.is_initialized() and world > 1
    if ref is not None:
        dev = ref.device
    else:                  # a rank with no prompt at all (world > n_prompts) learns the frame shape from rank 0
        dev = torch.device("cuda", torch.cuda.current_device()) if live and dist.get_backend() == "nccl" else torch.device("cpu")
    shape = torch.tensor(ref.shape if ref is not None else (0, 0, 0, 0), dtype=torch.int64, device=dev)
    if live:
        dist.broadcast(shape, src=0)
    T, H, W, C = (int(v) for v in shape.tolist())
    stack = torch.zeros(per_rank, T, H, W, C, dtype=torch.uint8, device=dev)
    for i, f in enumerate(local_frames):
        stack[i] = f
    gathered = gather_frames(stack, world, force=force)
    out = [None] * n_prompts
    for r, g in enumerate(gathered):
        for i, pid in enumerate(shard_prompts(n_prompts, r if len(gathered) > 1 else rank, world)):
            out[pid] = g[i]
    return out


def rank_core_slice(local_rank: int, local_world: int, cores: list | None = None) -> list:
    """The host cores of one rank: the cores this process may run on (its cpuset), cut into `local_world` contiguous, disjoint
    slices.  One process per GPU each runs a latency-sensitive enqueue loop (the AR decode queues ~125 launches per 1.2 ms
    step from one thread, 0.54 ms of host time per step): eight of them left to the scheduler migrate across cores and share
    caches; a fixed slice per rank keeps every rank's enqueue thread, its helper thread (generate_many / generate_stream) and
    its RCCL proxy thread on cores of their own."""
    if cores is None:
        cores = sorted(os.sched_getaffinity(0))
    n = len(cores)
    if local_world <= 1 or n < local_world:
        return list(cores)
    per = n // local_world
    return list(cores[local_rank * per:(local_rank + 1) * per])


def _parse_cpulist(text: str) -> list:
    out = []
    for part in text.strip().split(","):
        if not part:
            continue
        a, _, b = part.partition("-")
        out.extend(range(int(a), int(b or a) + 1))
    return out


def gpu_numa_nodes(sysfs: str = "/sys") -> tuple:
    """(numa node of every visible AMD compute GPU in device order, {node: [cpus]}) read from sysfs WITHOUT touching HIP: the
    cards whose PCI vendor is 0x1002 AND that expose a compute hwmon (hwmon*/freq1_input: display-only parts and iGPUs without an
    sclk file are skipped), sorted by PCI address (the order the runtime enumerates them in on one node), then filtered the way the
    runtimes compose their filters: ROCR_VISIBLE_DEVICES first (it hides devices from HIP), then HIP_VISIBLE_DEVICES or, if that
    is unset, CUDA_VISIBLE_DEVICES (indices into what ROCR left).  Plain integer lists only: a UUID list, an index out of range
    or an unreadable file yields an EMPTY list -- no claim about the order, and rank_core_plan falls back to the plain core cut
    (as it does whenever the visible-card count is smaller than the local world).  A node of -1 gives None for that GPU."""
    import glob
    cards = []
    for dev in glob.glob(os.path.join(sysfs, "class/drm/card[0-9]*/device")):
        try:
            if open(os.path.join(dev, "vendor")).read().strip() != "0x1002":
                continue
            if not glob.glob(os.path.join(dev, "hwmon", "hwmon*", "freq1_input")):
                continue                        # not a compute part (no shader clock): HIP does not enumerate it
            pci = os.path.basename(os.path.realpath(dev))
            try:
                node = int(open(os.path.join(dev, "numa_node")).read())
            except (OSError, ValueError):
                node = -1
            cards.append((pci, node if node >= 0 else None))
        except OSError:
            continue
    cards = [n for _, n in sorted(set(cards))]

    def pick(cur, var):
        v = os.environ.get(var)
        if not v:
            return cur, False
        try:
            return [cur[int(i)] for i in v.split(",")], True
        except (ValueError, IndexError):
            return [], True                     # UUID lists etc.: no claim about the order
    cards, _ = pick(cards, "ROCR_VISIBLE_DEVICES")
    cards, used_hip = pick(cards, "HIP_VISIBLE_DEVICES")
    if not used_hip:
        cards, _ = pick(cards, "CUDA_VISIBLE_DEVICES")
    cpus = {}
    for n in {c for c in cards if c is not None}:
        try:
            cpus[n] = _parse_cpulist(open(os.path.join(sysfs, f"devices/system/node/node{n}/cpulist")).read())
        except OSError:
            cpus[n] = []
    return cards, cpus


def rank_core_plan(local_world: int, cores: list, gpu_nodes: list | None = None, node_cpus: dict | None = None) -> list:
    """Core slice of EVERY local rank (a pure function of its arguments, so all ranks compute the same plan).  When the NUMA node
    of every rank's GPU is known and each node has at least as many allowed cores as ranks on it, a rank gets a contiguous share
    of the allowed cores of ITS GPU's node (ranks that share a node split it in rank order): launches, the RCCL proxy and the
    pinned prompt buffers stay on the socket the GPU hangs off.  Otherwise the plain cut of the cpuset into `local_world`
    contiguous slices (rank_core_slice)."""
    plain = [rank_core_slice(r, local_world, cores) for r in range(local_world)]
    if not gpu_nodes or len(gpu_nodes) < local_world or any(n is None for n in gpu_nodes[:local_world]) or not node_cpus:
        return plain
    allowed = set(cores)
    by_node = {}
    for r in range(local_world):
        by_node.setdefault(gpu_nodes[r], []).append(r)
    plan = [None] * local_world
    for node, ranks in by_node.items():
        mine = [c for c in sorted(node_cpus.get(node, [])) if c in allowed]
        if len(mine) < len(ranks):
            return plain
        per = len(mine) // len(ranks)
        for i, r in enumerate(ranks):
            plan[r] = mine[i * per:(i + 1) * per]
    return plan


def pin_rank_cores(local_rank: int, local_world: int) -> list:
    """Applies this rank's slice of rank_core_plan (the cores of its GPU's NUMA node when sysfs exposes it, else the plain cut) to
    this process -- call it BEFORE the first HIP call: all threads created afterwards inherit it -- and sizes torch's intra-op pool
    to it.  Returns the slice.  LD_NO_PIN=1 leaves the affinity alone."""
    if os.environ.get("LD_NO_PIN") == "1" or not hasattr(os, "sched_setaffinity"):
        return sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else []
    cores = sorted(os.sched_getaffinity(0))
    try:
        nodes, cpus = gpu_numa_nodes()
    except Exception:                            # sysfs layout surprises must never stop a run
        nodes, cpus = None, None
    mine = rank_core_plan(local_world, cores, nodes, cpus)[local_rank] if local_world > 1 else cores
    if local_world > 1 and os.environ.get("LD_PIN_VERBOSE", "1") != "0":
        numa = (nodes[local_rank] if nodes and len(nodes) >= local_world else None)
        print(f"[landiff_amd] local rank {local_rank}/{local_world}: {len(mine)} host cores "
              f"({mine[0]}..{mine[-1]})" + (f" on NUMA node {numa} of its GPU" if numa is not None else " (plain cut of the cpuset: GPU NUMA nodes unknown)"),
              file=sys.stderr, flush=True) if mine else None
    if mine:
        os.sched_setaffinity(0, mine)
        torch.set_num_threads(max(1, min(len(mine), torch.get_num_threads())))
        if local_world > 1 and len(mine) < 2:
            import warnings
            warnings.warn(f"rank {local_rank}: {len(mine)} host core(s) per rank -- the AR decode's enqueue loop (~0.5 ms of host time per "
                          "1.2 ms step) shares its core with the process's other threads; expect a lower decode rate")
    return mine


def gather_rank_reports(report: dict, world: int) -> list:
    """Every rank's small report dict (stage seconds, frames/s, ...) on every rank, in rank order: how an N > 1 bench line
    carries per-rank numbers next to the max-over-ranks time.  One all_gather_object outside the timed region."""
    import torch.distributed as dist
    if not dist.is_initialized() or world == 1:
        return [report]
    out = [None] * world
    dist.all_gather_object(out, report)
    return out
