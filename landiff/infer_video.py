"""python -m landiff.infer_video --prompt ... : the reference's CLI (landiff/infer_video.py:12-118) on the MI355X path."""
from pathlib import Path

import numpy as np
import torch

from landiff.diffusion.dif_infer import CogModelInferWrapper, VideoTask
from landiff.llm.llm_cfg import build_llm
from landiff.llm.llm_infer import ArModelInferWrapper, ARSampleCfg, CodeTask
from landiff.utils import cthw_to_numpy_images, save_video_tensor
from landiff_amd.pipeline import STREAM_PREFIX_FRAMES


def parse_args(argv=None):
    import argparse

    parser = argparse.ArgumentParser(description="Landiff Video Inference")
    parser.add_argument("--prompt", type=str, help="Prompt for the video generation.")
    parser.add_argument("--llm_ckpt", type=str, default="ckpts/LanDiff/llm/model.safetensors", help="Path to the LLM checkpoint.")
    parser.add_argument("--diffusion_ckpt", type=str, default="ckpts/LanDiff/diffusion", help="Path to the diffusion checkpoint.")
    parser.add_argument("--save_file_name", type=str, default="results/video", help="Path to save the generated video.")
    parser.add_argument("--cfg", type=float, default=7.5, help="CFG scale for the video generation.")
    parser.add_argument("--motion_score", type=float, default=0.1, help="Motion score for the video generation.")
    parser.add_argument("--seed", type=int, default=42, help="Random seed for video generation.")
    parser.add_argument("--num_samples", type=int, default=1,
                        help="Candidates of the prompt (1-4; 1-16 with --decode_engine mfma), seeds --seed .. --seed + N - 1, their tokens from ONE batched AR decode; "
                             "N > 1 writes <save_file_name>_<i>.mp4 / _<i>.npy, each what --seed (seed + i) alone produces.")
    parser.add_argument("--decode_engine", choices=("gemv", "mfma"), default="gemv",
                        help="Engine of the batched AR decode (--num_samples N > 1).  gemv: register GEMV, candidate i bit-identical "
                             "to --seed (seed + i) alone, N <= 4.  mfma: MFMA skinny GEMM, N <= 16; candidate i depends on its own seed "
                             "alone and equals the single run up to near-ties of the draw.")
    parser.add_argument("--keep", type=int, default=None,
                        help="Best-of-N: with --num_samples N >= K, rank the N candidates by the total log-probability of their "
                             "tokens under the distribution they were sampled from and run the diffusion stage for the K most "
                             "likely only.  All N .npy are written, videos for the kept ones (named by candidate index), and "
                             "<save_file_name>_scores.json lists {index, seed, logprob, kept} for every candidate.")
    parser.add_argument("--extend_video", type=str, default=None,
                        help="Continue this clip instead of generating from scratch: a uint8 [F, H, W, 3] .npy (the format "
                             "save_video_tensor falls back to) or an mp4 when imageio can read it.")
    parser.add_argument("--extend_chunks", type=int, default=1, help="Chunks appended to --extend_video.")
    parser.add_argument("--extend_prefix_frames", type=int, default=STREAM_PREFIX_FRAMES,
                        help="Latent frames of the previous chunk pinned as each new chunk's prefix.")
    parser.add_argument("--extend_tokens", type=str, default=None,
                        help="The clip's own semantic tokens (.npy of llm_infer, one segment): the AR decode continues from "
                             "them instead of sampling every segment from the prompt.")
    parser.add_argument("--theia_ckpt", type=str, default=None,
                        help="Theia model.safetensors (or its directory).  With --extend_video and no --extend_tokens the clip's "
                             "own tokens, from its frames, are the decode's first segment.  Also where --first_frame looks "
                             "(default: $LANDIFF_THEIA_CKPT, then a local Hugging Face cache snapshot; never downloaded).")
    parser.add_argument("--first_frame", type=str, default=None,
                        help="Image-guided generation (use_gt_first_frame): a uint8 [H, W, 3] .npy or an image imageio can "
                             "read, tokenized by the Theia extractor; its I-frame tokens start the AR decode.")
    parser.add_argument("--edit_video", type=str, default=None,
                        help="Edit this clip instead of generating from scratch (LanDiffPipeline.edit_video): a uint8 [4T-3, H, W, 3] "
                             ".npy or an mp4 when imageio can read it -- exactly one chunk at the model's frame size (49 frames of "
                             "480 x 720), never resized unless --clip_fit says how.  Writes the edited clip and <save_file_name>_edit.json.")
    parser.add_argument("--edit_strength", type=float, default=0.6, metavar="S",
                        help="With --edit_video: the share of the sampler's steps that run, in (0, 1].  1.0 regenerates from pure "
                             "noise; smaller values start later, from the re-noised clip, and stay closer to it.")
    parser.add_argument("--edit_mask", type=str, default=None,
                        help="With --edit_video: a .npy keep-mask (bool or uint8, non-zero = keep the clip), [4T-3, H, W] in pixels or "
                             "[T, H/8, W/8] in latent cells; the rest is regenerated.")
    parser.add_argument("--edit_tokens", type=str, default=None, metavar="{from_frames,prompt,PATH.npy}",
                        help="With --edit_video: where the semantic tokens come from -- the clip's own frames (Theia extractor; the "
                             "default with --theia_ckpt), an AR decode from the prompt (the default without), or a token .npy of "
                             "llm_infer.")
    parser.add_argument("--edit_clean_known", action="store_true",
                        help="With --edit_video and --edit_mask: pin the kept cells to the clean clip latent at every step instead "
                             "of its re-noised version.")
    parser.add_argument("--clip_fit", choices=("exact", "cover", "stretch"), default="exact",
                        help="How the input of --extend_video, --edit_video (with its --edit_mask) or --first_frame is brought to the "
                             "model's frame (the conform stage, on the GPU).  exact: it must already be that size (the default: "
                             "nothing is resized).  cover: the largest centred box of the frame's aspect ratio, resampled.  "
                             "stretch: the whole picture, resampled.  Writes <save_file_name>_conform.json.")
    parser.add_argument("--clip_fps", type=str, default=None, metavar="F",
                        help="With --clip_fit cover / stretch: the input clip's frame rate (a number or a ratio such as 30000/1001); "
                             "the model's frames are then picked at 8 fps from it.  Without it frames are taken one to one.  (Not "
                             "read from the container.)")
    parser.add_argument("--clip_start", type=float, default=None, metavar="S",
                        help="With --clip_fps: take the frames from S seconds into the clip on (--edit_video) instead of its "
                             "first ones; --extend_video always continues the clip's end.")
    parser.add_argument("--clip_filter", choices=("bilinear", "bicubic"), default=None,
                        help="With --clip_fit cover / stretch: the antialiased resampling filter (default bilinear).")
    parser.add_argument("--dit_cache", type=str, default=None, metavar="THRESH",
                        help="DiT step cache (off by default): a sampler step whose first-block input moved by less than THRESH "
                             "(accumulated relative L1, a float >= 0) since the last computed step reuses that step's residual across "
                             "the transformer stack instead of running it.  0 computes every step.  What each step did is written "
                             "to <save_file_name>_dit_cache.json.  The quality at a given threshold is not measured.")
    parser.add_argument("--attn_window", type=int, default=None, metavar="W",
                        help="Frame-window attention in the DiT (off by default): a video token attends to the text and to the W "
                             "latent frames each side of its own (W >= 0; per 256-row block, a ragged superset) instead of to every "
                             "frame.  The effect on quality is not measured.")
    parser.add_argument("--attn_window_dense_steps", type=int, default=0, metavar="K",
                        help="With --attn_window: the first K sampler steps of a video run full attention (executed steps: with "
                             "--edit_video they count from the step the edit starts at).")
    parser.add_argument("--dit_cfg_tol", type=float, default=None, metavar="T",
                        help="CFG branch skipping in the DiT (off by default): a sampler step whose guidance scale lies within T of 1 "
                             "(T >= 0) evaluates the cond branch alone.  What each step did is written to "
                             "<save_file_name>_dit_guidance.json.  The effect on quality is not measured.  (--cfg is the AR scale.)")
    parser.add_argument("--dit_cfg_refresh", type=int, default=None, metavar="K",
                        help="CFG branch skipping: both branches every K-th guided step (K >= 1), the steps between evaluate the cond "
                             "branch alone and reuse the last cond - uncond difference.  The effect on quality is not measured.")
    parser.add_argument("--dit_cfg_cos", type=float, default=None, metavar="C",
                        help="CFG branch skipping: once the two branches' outputs reach a cosine of C (-1 < C <= 1) every later step "
                             "of the video evaluates the cond branch alone.  The effect on quality is not measured.")
    parser.add_argument("--save_frames", action="store_true",
                        help="Also write the exact uint8 frames of every video as <name>.frames.npy next to it (an mp4 is lossy: "
                             "this file is what --compare_to takes).")
    parser.add_argument("--compare_to", type=str, default=None, metavar="REF.npy",
                        help="Compare every video written with the uint8 [F, H, W, 3] frames in this file (a --save_frames output "
                             "of another run), on the GPU: PSNR, SSIM and exact difference counts per frame and for the clip, plus "
                             "the frame-to-frame profile of both clips, to <name>_metrics.json.  The shapes must be equal; nothing "
                             "is resized.")
    parser.add_argument("--out_fps", type=int, default=None, metavar="N",
                        help="Write every video at N frames per second (an integer >= 1) instead of the model's 8: the frames go "
                             "through the retime stage on the GPU (in-between frames by block matching and motion-compensated "
                             "blending in integer arithmetic; landiff_amd/retime.py).  Writes <name>_retime.json (the plan and the "
                             "clip's motion profile).  --save_frames / --compare_to keep using the model's own 8 fps frames.  What "
                             "block-matched interpolation looks like on a trained checkpoint's output is not measured.")
    parser.add_argument("--out_search", type=int, default=None, metavar="R",
                        help="With --out_fps: the block search range in pixels per axis, 0..32 (default 8, untuned; 0: a cross-fade).")
    parser.add_argument("--video_encoder", choices=("host", "gpu"), default="host",
                        help="gpu: every video is written as a Motion-JPEG <name>.avi whose frames are encoded on the GPU (baseline "
                             "JPEG in integer arithmetic, one restart interval per MCU row; landiff_amd/encode.py), with "
                             "<name>_encode.json beside it; with --out_fps the retimed frames never leave the device unencoded.  "
                             "host (the default): the writer of save_video_tensor, unchanged.")
    parser.add_argument("--jpeg_quality", type=int, default=None, metavar="Q",
                        help="With --video_encoder gpu: IJG quality 1..100 (default 95, the host writer's).")
    parser.add_argument("--jpeg_frame_bytes", type=int, default=None, metavar="N",
                        help="With --video_encoder gpu: every frame's JPEG stream takes at most N bytes; each frame's quality is "
                             "searched on the GPU below --jpeg_quality (a stated bisection on exact sizes; landiff_amd/encode.py, "
                             "DESIGN 8.15).  A frame that does not fit at quality 1 is written there and reported.")
    parser.add_argument("--video_max_bytes", type=int, default=None, metavar="N",
                        help="With --video_encoder gpu: the .avi on disk takes at most N bytes; one quality for every frame, searched "
                             "on the GPU below --jpeg_quality.  <name>_encode.json says so if even quality 1 does not fit.")
    parser.add_argument("--encode_verify", action="store_true",
                        help="With --video_encoder gpu: decode the written streams again on the GPU and add what the file loses "
                             "against the frames it was made from (PSNR, SSIM, the largest difference) to <name>_encode.json.")
    parser.add_argument("--video_decoder", choices=("host", "gpu"), default="host",
                        help="gpu: a Motion-JPEG .avi given to --extend_video, --edit_video or --compare_to is decoded on the GPU "
                             "(baseline JPEG, equal to PIL's decode byte for byte; landiff_amd/decode.py): only the compressed bytes "
                             "are uploaded, with --clip_fit only the frames the conform stage reads are decoded, and "
                             "<name>_decode.json is written.  host (the default): PIL, frame by frame, unchanged.")
    parser.add_argument("--jpeg_entropy", choices=("segment", "sync", "auto"), default="segment",
                        help="With --video_decoder gpu: how the Huffman decode is spread over the GPU.  segment (the default): one "
                             "lane per restart segment, unchanged.  sync: one lane per 256 bytes of a segment, for files written "
                             "without restart markers (PIL, ffmpeg, cameras; landiff_amd/decode.py, DESIGN 8.14); the same frames "
                             "byte for byte.  auto: sync where the file's segments are long.")
    args = parser.parse_args(argv)
    if args.jpeg_entropy != "segment" and args.video_decoder != "gpu":
        parser.error("--jpeg_entropy goes with --video_decoder gpu")
    args.jpeg = args.jpeg_rate = None
    if args.video_encoder == "gpu":
        from landiff_amd.encode import JpegConfig
        try:
            args.jpeg = JpegConfig(quality=95 if args.jpeg_quality is None else args.jpeg_quality)
        except ValueError as e:
            parser.error(f"--jpeg_quality: {e}")
        if args.jpeg_frame_bytes is not None and args.video_max_bytes is not None:
            parser.error("--jpeg_frame_bytes and --video_max_bytes are mutually exclusive")
        if args.jpeg_frame_bytes is not None:
            from landiff_amd.encode import JpegRateConfig
            try:
                args.jpeg_rate = JpegRateConfig(frame_bytes=args.jpeg_frame_bytes)
            except ValueError as e:
                parser.error(f"--jpeg_frame_bytes: {e}")
        if args.video_max_bytes is not None and args.video_max_bytes < 1:
            parser.error(f"--video_max_bytes: must be an integer >= 1, got {args.video_max_bytes}")
    elif args.jpeg_quality is not None:
        parser.error("--jpeg_quality goes with --video_encoder gpu")
    elif args.jpeg_frame_bytes is not None:
        parser.error("--jpeg_frame_bytes goes with --video_encoder gpu")
    elif args.video_max_bytes is not None:
        parser.error("--video_max_bytes goes with --video_encoder gpu")
    elif args.encode_verify:
        parser.error("--encode_verify goes with --video_encoder gpu")
    args.retime = None
    if args.out_fps is None:
        if args.out_search is not None:
            parser.error("--out_search goes with --out_fps")
    else:
        if args.out_fps < 1:
            parser.error(f"--out_fps takes an integer >= 1, got {args.out_fps}")
        from landiff_amd.retime import RetimeConfig
        try:
            args.retime = RetimeConfig(out_fps=args.out_fps, **({} if args.out_search is None else {"search": args.out_search}))
        except ValueError as e:
            parser.error(f"--out_search: {e}")
    args.dit_guidance = None
    if args.dit_cfg_tol is not None or args.dit_cfg_refresh is not None or args.dit_cfg_cos is not None:
        from landiff_amd.dit_guidance import REFUSE_STEP_CACHE, GuidanceSkipConfig
        if args.dit_cache is not None:
            parser.error(f"--dit_cache with --dit_cfg_tol / --dit_cfg_refresh / --dit_cfg_cos: {REFUSE_STEP_CACHE}")
        try:
            args.dit_guidance = GuidanceSkipConfig(scale_tolerance=args.dit_cfg_tol, refresh=args.dit_cfg_refresh,
                                                   cos_threshold=args.dit_cfg_cos)
        except ValueError as e:
            parser.error(str(e))
    if args.attn_window is not None and args.attn_window < 0:
        parser.error(f"--attn_window takes an integer >= 0, got {args.attn_window}")
    if args.attn_window_dense_steps < 0 or (args.attn_window_dense_steps and args.attn_window is None):
        parser.error("--attn_window_dense_steps takes an integer >= 0 and goes with --attn_window")
    if args.dit_cache is not None:
        import math
        try:
            args.dit_cache = float(args.dit_cache)
        except ValueError:
            parser.error(f"--dit_cache takes a float >= 0, got {args.dit_cache!r}")
        if math.isnan(args.dit_cache) or args.dit_cache < 0:
            parser.error(f"--dit_cache takes a float >= 0, got {args.dit_cache!r}")
    max_n = 16 if args.decode_engine == "mfma" else 4
    if not 1 <= args.num_samples <= max_n:
        parser.error(f"--num_samples must be between 1 and {max_n}" + ("" if max_n == 16 else " (1 and 16 with --decode_engine mfma)"))
    if args.edit_video:
        if args.extend_video:
            parser.error("--edit_video changes a clip, --extend_video continues one: give one of them")
        if args.keep is not None:
            parser.error("--keep ranks candidates generated from a prompt, not --edit_video")
        if args.num_samples > 1:
            parser.error("--num_samples applies to generation from a prompt, not to --edit_video")
        if args.first_frame:
            parser.error("--first_frame guides generation from a prompt, not --edit_video")
        if not 0.0 < args.edit_strength <= 1.0:
            parser.error(f"--edit_strength (the share of steps --edit_video runs) must be in (0, 1], got {args.edit_strength}")
        if args.edit_tokens is None:
            args.edit_tokens = "from_frames" if args.theia_ckpt else "prompt"
    if args.num_samples > 1 and args.extend_video:
        parser.error("--num_samples applies to generation from a prompt, not to --extend_video")
    args.conform = None
    if args.clip_fit == "exact":
        if args.clip_fps is not None or args.clip_start is not None or args.clip_filter is not None:
            parser.error("--clip_fps / --clip_start / --clip_filter go with --clip_fit cover or stretch")
    else:
        if not (args.extend_video or args.edit_video or args.first_frame):
            parser.error("--clip_fit fits the input of --extend_video, --edit_video or --first_frame: give one of them")
        if args.clip_start is not None and (args.clip_fps is None or not args.edit_video):
            parser.error("--clip_start goes with --clip_fps and --edit_video (--extend_video continues the clip's end)")
        if args.clip_fps is not None and not (args.extend_video or args.edit_video):
            parser.error("--clip_fps is the frame rate of the --extend_video / --edit_video clip")
        from landiff_amd.conform import ConformConfig
        try:
            args.conform = ConformConfig(fit=args.clip_fit, src_fps=args.clip_fps,
                                         window="last" if args.extend_video or args.clip_fps is None or args.clip_start is None else "first",
                                         start_s=args.clip_start or 0.0, filter=args.clip_filter or "bilinear")
        except (ValueError, ZeroDivisionError) as e:
            parser.error(f"--clip_fps / --clip_start: {e}")
    if args.num_samples > 1 and not all(args.seed + i for i in range(args.num_samples)):
        parser.error("--num_samples needs non-zero seeds (--seed .. --seed + N - 1)")
    if args.keep is not None:
        if args.num_samples < 2:
            parser.error("--keep ranks the candidates of --num_samples N (N >= 2)")
        if not 1 <= args.keep <= args.num_samples:
            parser.error(f"--keep must be between 1 and --num_samples ({args.num_samples})")
    return args


def load_image(path: str) -> torch.Tensor:
    """uint8 image [H, W, 3] from a .npy or, through imageio, an image file."""
    if path.endswith(".npy"):
        arr = np.load(path)
    else:
        try:
            import imageio
        except ImportError as e:
            raise ValueError(f"{path}: reading an image file needs imageio; give the uint8 [H, W, 3] pixels as .npy instead") from e
        arr = np.asarray(imageio.imread(path))
        if arr.ndim == 3 and arr.shape[-1] == 4:
            arr = arr[..., :3]
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[-1] != 3:
        raise ValueError(f"{path}: expected a uint8 image [H, W, 3], got {arr.dtype} {arr.shape}")
    return torch.from_numpy(np.ascontiguousarray(arr))


def build_theia_tokenizer(args, dev):
    """The Theia extractor (--theia_ckpt, else $LANDIFF_THEIA_CKPT / the HF cache) with the tokenizer's encoder half attached
    (tokenizer_ckpt of the diffusion stage's YAML), its output grid the tokenizer's."""
    from landiff.diffusion.dif_infer import DEFAULT_INFER_CFG, DEFAULT_MODEL_CFG, _cfg_path
    from landiff_amd.config import load_diffusion_config
    from landiff_amd.theia import build_theia
    from landiff_amd.tokenizer_encoder import TokenizerEncoder
    from landiff_amd.weights import load_tokenizer_encoder_state, resolve_ckpt_path
    dcfg = load_diffusion_config(_cfg_path(DEFAULT_MODEL_CFG), _cfg_path(DEFAULT_INFER_CFG))
    enc = TokenizerEncoder(load_tokenizer_encoder_state(resolve_ckpt_path(dcfg.tokenizer_ckpt)), dcfg.tok, dev)
    return build_theia(args.theia_ckpt, dcfg.tok, dev, encoder=enc)


def first_frame_tokens(args) -> torch.Tensor:
    """--first_frame: the image's semantic tokens (TheiaExtractor.tokenize_image; the LLM keeps the I-frame ones)."""
    img = load_image(args.first_frame)
    dev = torch.device(f"cuda:{torch.cuda.current_device()}")
    theia = build_theia_tokenizer(args, dev)
    if getattr(args, "conform", None) is not None:
        from landiff.diffusion.dif_infer import DEFAULT_INFER_CFG, DEFAULT_MODEL_CFG, _cfg_path
        from landiff_amd.config import load_diffusion_config
        from landiff_amd.conform import conform_image, image_plan
        d = load_diffusion_config(_cfg_path(DEFAULT_MODEL_CFG), _cfg_path(DEFAULT_INFER_CFG)).dit
        _write_conform_json(args, image_plan(tuple(img.shape), 8 * d.latent_h, 8 * d.latent_w, args.conform).as_dict())
        img = conform_image(img, 8 * d.latent_h, 8 * d.latent_w, args.conform, dev)
    tokens = theia.tokenize_image(img.to(dev)).cpu()
    del theia
    torch.cuda.empty_cache()
    return tokens


def llm_infer(args):
    llm_model_cfg = build_llm()
    first = first_frame_tokens(args) if args.first_frame else None
    llm = ArModelInferWrapper(args.llm_ckpt, llm_model_cfg)
    # one segment of semantic frames = one 49-frame clip: 13 for the shipped configuration (ARSampleCfg's default, which the
    # reference's llm_infer relies on); a configuration with another segment length (BASELINE configs[0]: 8) decodes its own
    task = CodeTask(save_file_name=f"{args.save_file_name}.npy", prompt=args.prompt, seed=args.seed,
                    sample_cfg=ARSampleCfg(temperature=1.0, cfg=args.cfg, motion_score=args.motion_score,
                                           num_frames=llm_model_cfg.segment_length, use_gt_first_frame=first is not None),
                    first_frame_tokens=first)
    task = llm(task)
    tokens = task.result.reshape(-1)
    path = Path(task.save_file_name)
    path.parent.mkdir(parents=True, exist_ok=True)
    np.save(path, tokens.cpu().numpy())
    del llm
    torch.cuda.empty_cache()
    return tokens.cuda()


def sample_names(args) -> list:
    """(seed, file stem) per candidate: --num_samples 1 is the plain name, N > 1 numbers them."""
    if args.num_samples == 1:
        return [(args.seed, args.save_file_name)]
    return [(args.seed + i, f"{args.save_file_name}_{i}") for i in range(args.num_samples)]


def llm_infer_samples(args):
    """--num_samples N > 1: llm_infer for seeds seed .. seed + N - 1 from one batched decode -> tokens [N, n_visual] (cuda).
    -> (tokens, kept): kept = the candidate indices --keep K selects, in rank order (<save_file_name>_scores.json is written next to
    the .npy files), or None without --keep: every candidate."""
    llm_model_cfg = build_llm()
    first = first_frame_tokens(args) if args.first_frame else None
    wide = args.decode_engine == "mfma"
    llm = ArModelInferWrapper(args.llm_ckpt, llm_model_cfg, max_samples=1 if wide else args.num_samples,
                              wide_samples=args.num_samples if wide else 0)
    names = sample_names(args)
    task = CodeTask(save_file_name=f"{args.save_file_name}.npy", prompt=args.prompt, seed=args.seed,
                    sample_cfg=ARSampleCfg(temperature=1.0, cfg=args.cfg, motion_score=args.motion_score,
                                           num_frames=llm_model_cfg.segment_length, use_gt_first_frame=first is not None),
                    first_frame_tokens=first)
    task = llm(task, seeds=[s for s, _ in names], return_logprobs=args.keep is not None, engine=args.decode_engine)
    tokens = task.result
    for row, (_, stem) in zip(tokens, names):
        path = Path(f"{stem}.npy")
        path.parent.mkdir(parents=True, exist_ok=True)
        np.save(path, row.numpy())
    del llm
    torch.cuda.empty_cache()
    if args.keep is None:
        return tokens.cuda(), None
    from landiff_amd.pipeline import rank_candidates, write_scores_json
    scores = task.logprobs.double().sum(1).tolist()
    kept = rank_candidates(scores)[:args.keep]
    write_scores_json(f"{args.save_file_name}_scores.json", [s for s, _ in names], scores, kept)
    return tokens.cuda(), kept


def _diffusion_model(args):
    """CogModelInferWrapper of the run; --dit_cache and --attn_window are handed on only when given (without them the call is the
    reference's)."""
    return CogModelInferWrapper(ckpt_path=args.diffusion_ckpt, **_dit_options(args))


def _dit_options(args) -> dict:
    """The opt-in DiT switches of the command line as keyword arguments, each present only when its flag was given."""
    kw = {}
    if getattr(args, "dit_cache", None) is not None:
        kw["dit_cache"] = args.dit_cache
    if getattr(args, "dit_guidance", None) is not None:
        kw["dit_guidance"] = args.dit_guidance
    if getattr(args, "attn_window", None) is not None:
        from landiff_amd.config import AttnWindowConfig
        kw["attn_window"] = AttnWindowConfig(frames=args.attn_window, dense_steps=getattr(args, "attn_window_dense_steps", 0))
    return kw


def _conform_options(args) -> dict:
    """--clip_fit cover / stretch as the conform= keyword of extend_video / edit_video, present only when the flag was given."""
    return {} if getattr(args, "conform", None) is None else {"conform": args.conform}


def _write_dit_cache_report(args, stem, report):
    """--dit_cache: <stem>_dit_cache.json, what the step cache did in the run that produced <stem>.mp4."""
    if getattr(args, "dit_cache", None) is None:
        return
    from landiff_amd.dit_cache import write_report_json
    path = Path(f"{stem}_dit_cache.json")
    path.parent.mkdir(parents=True, exist_ok=True)
    write_report_json(str(path), report)


def _write_dit_guidance_report(args, stem, report):
    """--dit_cfg_*: <stem>_dit_guidance.json, what each sampler step of the run that produced <stem>.mp4 evaluated."""
    if getattr(args, "dit_guidance", None) is None:
        return
    from landiff_amd.dit_guidance import write_report_json
    path = Path(f"{stem}_dit_guidance.json")
    path.parent.mkdir(parents=True, exist_ok=True)
    write_report_json(str(path), report)


def _write_conform_json(args, last_conform):
    """--clip_fit cover / stretch: <save_file_name>_conform.json, what the conform stage did (box, scales, frame indices, fit, filter,
    src_fps)."""
    if getattr(args, "conform", None) is None or last_conform is None:
        return
    import json
    path = Path(f"{args.save_file_name}_conform.json")
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as f:
        json.dump(last_conform, f, indent=1, allow_nan=False)


def _save_encoded(frames, path: str, fps: int, jpeg, verify: bool = False, rate=None, max_bytes=None):
    """--video_encoder gpu: uint8 frames [F, H, W, 3] on the device -> <name>.avi (Motion-JPEG, the frames encoded where they are)
    and <name>_encode.json (quality, subsampling, frame count, bytes per frame, total bytes, the table source).  --encode_verify:
    the streams decoded again on the device (landiff_amd.decode) and compared with the frames: "verify" in the same file.
    rate (--jpeg_frame_bytes: a JpegRateConfig) or max_bytes (--video_max_bytes: the cap on the .avi, turned into the clip budget
    mjpeg_avi_stream_budget leaves for this many frames; refused before any launch if nothing is left): the rate-controlled encode
    (DESIGN 8.15), its report under "rate"."""
    import json
    from landiff.utils import mjpeg_avi_stream_budget, write_mjpeg_avi_encoded
    from landiff_amd.encode import JpegRateConfig, encode_jpeg, encode_report
    if max_bytes is not None:
        rate = JpegRateConfig(clip_bytes=mjpeg_avi_stream_budget(max_bytes, int(frames.shape[0])))
    info = None
    if rate is None:
        jpegs = encode_jpeg(frames, jpeg)
    else:
        jpegs, info = encode_jpeg(frames, jpeg, rate=rate, return_rate=True)
    stem = Path(path).with_suffix("")
    stem.parent.mkdir(parents=True, exist_ok=True)
    write_mjpeg_avi_encoded(jpegs, (int(frames.shape[2]), int(frames.shape[1])), f"{stem}.avi", fps=fps)
    report = encode_report(jpegs, jpeg, rate, info)
    if max_bytes is not None:
        report["rate"]["video_max_bytes"] = int(max_bytes)
    if verify:
        from landiff_amd.decode import decode_jpeg
        from landiff_amd.metrics import _jsonable, compare_clips
        m = compare_clips(frames, decode_jpeg(jpegs, frames.device)).as_dict()
        report["verify"] = _jsonable({"clip": m["clip"], "frames": {k: m["frames"][k] for k in ("psnr", "ssim", "max_abs")}})
    with open(f"{stem}_encode.json", "w") as f:
        json.dump(report, f, indent=1, allow_nan=False)
    print(f"encoded {len(jpegs)} frames on the GPU: {stem}.avi, {stem}_encode.json")


def _device_frames(video):
    dev = torch.device(f"cuda:{torch.cuda.current_device()}")
    return (video if video.dtype == torch.uint8 else torch.from_numpy(cthw_to_numpy_images(video))).to(dev).contiguous()


def _save_retimed(video, path: str, fps: int, retime, jpeg=None, verify: bool = False, rate=None, max_bytes=None):
    """--out_fps: the clip's frames at `fps` -> the retime stage on the current device -> save_video_tensor at the new rate (with
    --video_encoder gpu: _save_encoded, the retimed frames stay on the device), and <name>_retime.json: the plan (source frame and
    phase of every frame written) and the motion profile of the model's frames."""
    import json
    from landiff_amd.retime import motion_profile, retime_clip, retime_plan
    frames = _device_frames(video)
    plan = retime_plan(frames.shape[0], retime, src_fps=fps)
    if jpeg is None:
        save_video_tensor(retime_clip(frames, plan), path, fps=int(plan.out_fps))
    else:
        _save_encoded(retime_clip(frames, plan), path, int(plan.out_fps), jpeg, verify, rate, max_bytes)
    report = {"plan": plan.as_dict(),
              "motion": motion_profile(frames, retime.search, retime.penalty, retime.max_sad).as_dict() if frames.shape[0] > 1 else None}
    stem = Path(path).with_suffix("")
    with open(f"{stem}_retime.json", "w") as f:
        json.dump(report, f, indent=1, allow_nan=False)
    print(f"retimed {frames.shape[0]} frames at {fps} fps to {plan.n_out} at {int(plan.out_fps)} fps: {stem}_retime.json")


def _save_video(args, video, path: str, fps: int = 8):
    """Every video this module writes goes through here: save_video_tensor, then --save_frames (<name>.frames.npy, the exact uint8
    frames) and --compare_to (<name>_metrics.json: landiff_amd.metrics.compare_clips of the frames against the reference file's, and
    temporal_profile of both clips).  Without the two flags it is save_video_tensor alone.  --out_fps N: what is written is the
    clip retimed to N fps on the current device (landiff_amd.retime), with <name>_retime.json beside it; the two flags keep using the
    model's own frames, and <name>.frames.npy is written after the video so that it holds them whatever the writer left there.
    --video_encoder gpu: the video is <name>.avi, its JPEG frames encoded on the device (landiff_amd.encode), with <name>_encode.json."""
    retime, jpeg = getattr(args, "retime", None), getattr(args, "jpeg", None)
    verify = getattr(args, "encode_verify", False)
    rate, max_bytes = getattr(args, "jpeg_rate", None), getattr(args, "video_max_bytes", None)
    if retime is not None:
        _save_retimed(video, path, fps, retime, jpeg, verify, rate, max_bytes)
    elif jpeg is not None:
        _save_encoded(_device_frames(video), path, fps, jpeg, verify, rate, max_bytes)
    else:
        save_video_tensor(video, path, fps=fps)
    ref_path = getattr(args, "compare_to", None)
    if not (getattr(args, "save_frames", False) or ref_path):
        return
    frames = video.cpu() if video.dtype == torch.uint8 else torch.from_numpy(cthw_to_numpy_images(video))
    stem = Path(path).with_suffix("")
    stem.parent.mkdir(parents=True, exist_ok=True)
    if getattr(args, "save_frames", False):
        np.save(f"{stem}.frames.npy", frames.numpy())
    if ref_path:
        from landiff_amd.metrics import compare_clips, temporal_profile, write_metrics_json
        ref = load_clip(ref_path, getattr(args, "video_decoder", "host"), report=f"{stem}_decode.json",
                        entropy=getattr(args, "jpeg_entropy", "segment"))
        if tuple(ref.shape) != tuple(frames.shape):
            raise ValueError(f"--compare_to {ref_path}: the reference is {tuple(ref.shape)}, the video written to {path} is "
                             f"{tuple(frames.shape)}; the shapes must be equal (nothing is resized)")
        dev = torch.device(f"cuda:{torch.cuda.current_device()}")
        out_d, ref_d = frames.to(dev), ref.to(dev)
        row = compare_clips(out_d, ref_d).as_dict()
        row["reference"] = ref_path
        row["temporal"] = {"video": temporal_profile(out_d) if frames.shape[0] > 1 else None,
                           "reference": temporal_profile(ref_d) if frames.shape[0] > 1 else None}
        write_metrics_json(f"{stem}_metrics.json", row)
        print(f"compared with {ref_path}: {stem}_metrics.json")


def infer_diffusion_samples(args, tokens, kept=None):
    """kept (--keep): the candidate indices to run, in rank order; None: every candidate."""
    model = _diffusion_model(args)
    names = sample_names(args)
    for i in (range(len(names)) if kept is None else kept):
        row, (seed, stem) = tokens[i], names[i]
        task = model(VideoTask(save_file_name=f"{stem}.mp4", prompt=args.prompt, seed=seed, fps=8, semantic_token=row))
        _write_dit_cache_report(args, stem, model.dit_cache_report() if args.dit_cache is not None else None)
        _write_dit_guidance_report(args, stem, model.dit_guidance_report() if getattr(args, "dit_guidance", None) is not None else None)
        _save_video(args, task.result, task.save_file_name, fps=task.fps)
        print(f"save video to {task.save_file_name}")


def infer_diffusion(args, semantic_token):
    model = _diffusion_model(args)
    task = VideoTask(save_file_name=f"{args.save_file_name}.mp4", prompt=args.prompt, seed=args.seed, fps=8,
                     semantic_token=semantic_token)
    task = model(task)
    _write_dit_cache_report(args, args.save_file_name, model.dit_cache_report() if args.dit_cache is not None else None)
    _write_dit_guidance_report(args, args.save_file_name,
                               model.dit_guidance_report() if getattr(args, "dit_guidance", None) is not None else None)
    _save_video(args, task.result, task.save_file_name, fps=task.fps)
    print(f"save video to {task.save_file_name}")


def load_clip(path: str, decoder: str = "host", needed=None, report: str | None = None, entropy: str = "segment") -> torch.Tensor:
    """uint8 frames [F, H, W, 3] from a .npy (save_video_tensor's fallback format) or, through imageio, a video file; without
    imageio a Motion-JPEG .avi (what this project writes) is read with landiff.utils.read_mjpeg_avi.
    decoder="gpu" (--video_decoder gpu): a Motion-JPEG .avi is decoded on the current device (landiff_amd.decode: equal to PIL's
    decode) and the frames returned are a device tensor; anything else is read as with "host".  needed: a function (F, H, W) ->
    the frame indices that will be read (--clip_fit: conform_plan's); only those are decoded, the others are zero.  report: where
    decode_report's figures are written (<name>_decode.json).  entropy (--jpeg_entropy): decode_jpeg's entropy route, with
    decoder="gpu" only."""
    if entropy != "segment" and decoder != "gpu":
        raise ValueError(f"load_clip: entropy={entropy!r} goes with decoder=\"gpu\"")
    if decoder == "gpu" and path.lower().endswith(".avi"):
        import json
        from landiff.utils import read_mjpeg_avi_chunks
        from landiff_amd.decode import decode_jpeg
        chunks, (W, H), _ = read_mjpeg_avi_chunks(path)
        dev = torch.device(f"cuda:{torch.cuda.current_device()}")
        figures = {}
        if needed is None:
            clip = decode_jpeg(chunks, dev, report=figures, entropy=entropy)
        else:
            idx = sorted({int(k) for k in needed(len(chunks), H, W)})
            clip = torch.zeros(len(chunks), H, W, 3, dtype=torch.uint8, device=dev)
            clip[torch.tensor(idx, device=dev)] = decode_jpeg(chunks, dev, frames=idx, report=figures, entropy=entropy)
            figures["decoded_frames"] = idx
        if report:
            figures["source"], figures["clip_frames"] = path, len(chunks)
            Path(report).parent.mkdir(parents=True, exist_ok=True)
            with open(report, "w") as f:
                json.dump(figures, f, indent=1, allow_nan=False)
        return clip
    if path.endswith(".npy"):
        arr = np.load(path)
    else:
        try:
            import imageio
        except ImportError as e:
            if not path.lower().endswith(".avi"):
                raise ValueError(f"{path}: reading a video file needs imageio; give the uint8 frames as .npy or a Motion-JPEG "
                                 ".avi instead") from e
            from landiff.utils import read_mjpeg_avi
            arr = read_mjpeg_avi(path)[0]
        else:
            arr = np.stack(list(imageio.get_reader(path)))
    if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[-1] != 3:
        raise ValueError(f"{path}: expected uint8 frames [F, H, W, 3], got {arr.dtype} {arr.shape}")
    return torch.from_numpy(np.ascontiguousarray(arr))


def _gpu_decoder(args) -> bool:
    return getattr(args, "video_decoder", "host") == "gpu"


def _load_clip_on_gpu(args, path: str, pipe) -> torch.Tensor:
    """--video_decoder gpu: the clip of --extend_video / --edit_video through load_clip's device path, once the pipeline exists: with
    --clip_fit only the frames the conform stage will read are decoded (its plan needs the header's size and the chunk count alone)."""
    needed = None
    if getattr(args, "conform", None) is not None:
        from landiff_amd.conform import conform_plan
        d = pipe.cfg.dit
        needed = lambda F, H, W: conform_plan((F, H, W), 4 * d.latent_frames - 3, 8 * d.latent_h, 8 * d.latent_w, args.conform).frame_idx
    return load_clip(path, "gpu", needed=needed, report=f"{args.save_file_name}_decode.json",
                     entropy=getattr(args, "jpeg_entropy", "segment"))


def build_continuation(args, n_seg=None, theia=None):
    """The pipeline and prompt inputs --extend_video runs (and, with n_seg = 1 and its own `theia` choice, --edit_video): the diffusion stage's YAML files and checkpoint tree (as
    CogModelInferWrapper reads them), the VAE encoder's weights ('encoder.*' of the VAE checkpoint, then of the diffusion
    checkpoint's first stage), the LLM checkpoint, and the prompt through both T5 encoders.  -> (LanDiffPipeline, PromptInputs)."""
    from landiff.diffusion.dif_infer import DEFAULT_INFER_CFG, DEFAULT_MODEL_CFG, _cfg_path
    from landiff_amd.config import load_diffusion_config
    from landiff_amd.pipeline import LanDiffPipeline, PromptInputs, stream_plan
    from landiff_amd.text import encode_flan_t5, encode_t5_v11
    from landiff_amd.weights import load_diffusion_states, load_llm_state, load_vae_encoder_state, resolve_ckpt_path
    dcfg = load_diffusion_config(_cfg_path(DEFAULT_MODEL_CFG), _cfg_path(DEFAULT_INFER_CFG))
    cfg = dcfg.pipeline(build_llm()).check()
    dev = torch.device(f"cuda:{torch.cuda.current_device()}")
    ckpt = resolve_ckpt_path(args.diffusion_ckpt)
    st = load_diffusion_states(ckpt, None, base_dit_ckpt=dcfg.base_dit_ckpt, vae_ckpt=dcfg.vae_ckpt,
                               tokenizer_ckpt=dcfg.tokenizer_ckpt or None)
    st["vae"] = {**st["vae"], **load_vae_encoder_state(None, vae_ckpt=dcfg.vae_ckpt, diffusion_dir=ckpt)}
    st["llm"] = load_llm_state(args.llm_ckpt)
    c = cfg.llm
    # the clip is chunk 0 of the stream: its multi-segment AR decode needs n_seg segments of KV cache
    if n_seg is None:
        _, _, n_seg = stream_plan(cfg, args.extend_chunks + 1, args.extend_prefix_frames)
    win = {k: v for k, v in _dit_options(args).items() if k in ("attn_window", "dit_guidance")}
    pipe = LanDiffPipeline(cfg, st, dev, max_llm_frames=n_seg * c.segment_length, dit_cache=getattr(args, "dit_cache", None), **win)
    text = encode_flan_t5([args.prompt], dev, max_length=c.max_cond_tokens, model_path=c.text_encoder_path)[0]
    ctx = encode_t5_v11([args.prompt], resolve_ckpt_path(dcfg.t5_dir), cfg.dit.text_len, dev)
    inp = PromptInputs(text, ctx, seed=args.seed, cfg=args.cfg, motion_score=args.motion_score)
    if (args.theia_ckpt and not args.extend_tokens) if theia is None else theia:
        pipe.theia = build_theia_tokenizer(args, dev)
    return pipe, inp


def extend_diffusion(args):
    """--extend_video: LanDiffPipeline.extend_video on the clip -- its last 4T-3 frames encoded, the chunks after it run as
    generate_stream runs its later chunks (sliding semantic windows of one multi-segment AR decode, the prefix latents pinned,
    the decode continued against the VAE caches); --extend_tokens forces the decode's first segment to the clip's own tokens, and
    so does --theia_ckpt without --extend_tokens, with the tokens computed from the clip's frames.
    Writes the clip followed by the new frames; with --clip_fit cover / stretch the conformed window followed by the new frames."""
    clip = None if _gpu_decoder(args) else load_clip(args.extend_video)
    pipe, inp = build_continuation(args)
    if clip is None:
        clip = _load_clip_on_gpu(args, args.extend_video, pipe)
    if args.extend_tokens:
        clip_tokens = torch.from_numpy(np.load(args.extend_tokens)).reshape(-1)
    else:
        clip_tokens = "from_frames" if args.theia_ckpt else None
    new = pipe.extend_video(inp, args.extend_chunks, frames=clip, clip_tokens=clip_tokens,
                            prefix_frames=args.extend_prefix_frames, **_conform_options(args))
    if getattr(args, "conform", None) is not None:
        clip = pipe.last_conform_frames.cpu()
        _write_conform_json(args, pipe.last_conform)
    _write_dit_cache_report(args, args.save_file_name, pipe.dit_cache_reports)        # one list per appended chunk
    _write_dit_guidance_report(args, args.save_file_name, pipe.dit_guidance_reports)
    frames = torch.cat([clip.cpu(), new.cpu()], dim=0)        # (--video_decoder gpu left the clip on the device)
    path = f"{args.save_file_name}.mp4"
    _save_video(args, frames, path, fps=8)
    print(f"save video to {path} ({frames.shape[0]} frames, {new.shape[0]} new)")
    return frames


def load_mask(path: str) -> torch.Tensor:
    """--edit_mask: a bool or uint8 .npy [F, H, W] (pixels) or [T, h, w] (latent cells), non-zero = keep -> bool tensor."""
    arr = np.load(path)
    if arr.dtype not in (np.bool_, np.uint8) or arr.ndim != 3:
        raise ValueError(f"{path}: expected a bool or uint8 keep-mask [F, H, W] or [T, h, w], got {arr.dtype} {arr.shape}")
    return torch.from_numpy(np.ascontiguousarray(arr != 0))


def edit_diffusion(args):
    """--edit_video: LanDiffPipeline.edit_video on the clip -- the sampler started at the step --edit_strength picks from the
    re-noised clip latent, the cells --edit_mask keeps held on the clip, the semantic tokens from the clip's frames (--edit_tokens
    from_frames: the default with --theia_ckpt), from the prompt or from a file.  Writes the edited clip and <name>_edit.json."""
    from landiff_amd.pipeline import write_edit_json
    clip = None if _gpu_decoder(args) else load_clip(args.edit_video)
    mask = load_mask(args.edit_mask) if args.edit_mask else None
    pipe, inp = build_continuation(args, n_seg=1, theia=args.edit_tokens == "from_frames")
    if clip is None:
        clip = _load_clip_on_gpu(args, args.edit_video, pipe)
    kw = {}
    if args.edit_tokens == "from_frames":
        kw["clip_tokens"] = "from_frames"
    elif args.edit_tokens != "prompt":
        kw["tokens"] = torch.from_numpy(np.load(args.edit_tokens)).reshape(-1)
    frames = pipe.edit_video(inp, frames=clip, strength=args.edit_strength, keep_mask=mask,
                             known_noise=not args.edit_clean_known, **kw, **_conform_options(args)).cpu()
    _write_conform_json(args, pipe.last_conform)
    _write_dit_cache_report(args, args.save_file_name, pipe.dit_cache_report() if getattr(args, "dit_cache", None) is not None else None)
    _write_dit_guidance_report(args, args.save_file_name,
                               pipe.dit_guidance_report() if getattr(args, "dit_guidance", None) is not None else None)
    path = Path(f"{args.save_file_name}_edit.json")
    path.parent.mkdir(parents=True, exist_ok=True)
    write_edit_json(str(path), pipe.last_edit)
    _save_video(args, frames, f"{args.save_file_name}.mp4", fps=8)
    e = pipe.last_edit
    print(f"save video to {args.save_file_name}.mp4 (steps {e['start_step']}..{e['start_step'] + e['steps_run'] - 1}, "
          f"{e['kept_cells']} of {e['total_cells']} latent cells kept, tokens: {e['tokens_source']})")
    return frames


def main():
    import os

    args = parse_args()
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if int(os.environ.get("LOCAL_WORLD_SIZE", "1")) > 1:      # one process per GPU (prompt-level data parallelism): own core slice per rank
        from landiff_amd.pipeline import pin_rank_cores
        pin_rank_cores(local_rank, int(os.environ["LOCAL_WORLD_SIZE"]))
    torch.cuda.set_device(local_rank)
    if args.edit_video:
        edit_diffusion(args)
        return
    if args.extend_video:
        extend_diffusion(args)
        return
    if args.num_samples > 1:
        infer_diffusion_samples(args, *llm_infer_samples(args))
        return
    infer_diffusion(args, llm_infer(args))


if __name__ == "__main__":
    main()
