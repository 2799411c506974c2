"""GPU tests of the 3D-VAE encoder (ld_vae_enc.hip + landiff_amd/vae_encoder.py), LanDiffPipeline.extend_video, the
prefix_tokens form of the AR decode and CogWrapper.encode_first_stage."""
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden", "vae_encoder_fp32.npz")
BF = torch.bfloat16


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.fixture(scope="module")
def setup(cuda):
    from landiff_amd.config import PipelineConfig
    from landiff_amd.weights import init_pipeline_state, init_state, vae_encoder_spec
    cfg = PipelineConfig.tiny(num_steps=3).check()
    states = init_pipeline_state(cfg, seed=1234)
    states["vae"] = dict(states["vae"], **init_state(vae_encoder_spec(cfg.vae), seed=77))
    return cfg, states


@pytest.mark.gpu
def test_placement_downsample_posterior_kernels(cuda):
    from landiff_amd import ops
    from vae_encoder_ref import space_to_depth, time_pool
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (5, 6, 10, 3), generator=g, dtype=torch.uint8)
    xp = torch.full((7, 8, 12, 64), 7.0, dtype=BF, device=cuda)           # every element must be overwritten
    ops.vae_enc_place_input(frames.to(cuda), xp)
    x = (frames.float() / 127.5 - 1.0).to(BF)
    want = torch.zeros(7, 8, 12, 64, dtype=BF)
    want[2:, 1:-1, 1:-1, :3] = x
    want[0, 1:-1, 1:-1, :3] = x[0]
    want[1, 1:-1, 1:-1, :3] = x[0]
    assert torch.equal(xp.cpu(), want)
    f32 = (torch.rand(5, 6, 10, 3, generator=g) * 2 - 1)
    ops.vae_enc_place_input(f32.to(cuda), xp)
    assert torch.equal(xp[2:, 1:-1, 1:-1, :3].cpu(), f32.to(BF)) and torch.count_nonzero(xp[:, :, :, 3:]) == 0
    for T in (1, 4, 5, 9):
        for compress in (False, True):
            H, W, C = 6, 10, 24
            h = torch.randn(T, H, W, C, generator=g).to(BF)
            To = ops.vae_enc_downsample_out_frames(T, compress)
            out = torch.full((To, H // 2 + 2, W // 2 + 2, 4 * C), 3.0, dtype=BF, device=cuda)
            ops.vae_enc_downsample(h.reshape(-1, C).to(cuda), out, T, H, W, C, compress)
            ref = space_to_depth(time_pool(h) if compress else h)        # fp32 mean of two bf16 values, rounded once
            assert torch.equal(out.cpu(), ref), (T, compress)
    T, Z, H, W = 3, 16, 4, 6
    mom = torch.randn(T * H * W, 2 * Z, generator=g) * 4
    eps = torch.randn(Z, T, H, W, generator=g)
    z = torch.empty(T, Z, H, W, device=cuda)
    mean, lv = torch.empty_like(z), torch.empty_like(z)
    ops.vae_posterior(mom.to(cuda), z, T, Z, H, W, 1.5, eps=eps.to(cuda), mean=mean, logvar=lv)
    m = mom[:, :Z].reshape(T, H, W, Z).permute(0, 3, 1, 2)
    l = mom[:, Z:].clamp(-30, 20).reshape(T, H, W, Z).permute(0, 3, 1, 2)
    assert torch.equal(mean.cpu(), m) and torch.equal(lv.cpu(), l)
    assert rel(z, 1.5 * (m + torch.exp(0.5 * l) * eps.permute(1, 0, 2, 3))) < 1e-6
    ops.vae_posterior(mom.to(cuda), z, T, Z, H, W, 1.5)
    assert torch.equal(z.cpu(), 1.5 * m)


@pytest.mark.gpu
@pytest.mark.parametrize("clip", ["odd", "even"])
def test_encoder_tiny_against_the_reference(cuda, clip):
    """Mean and the seeded sample of VAEEncoder vs the reference's fp32 outputs, within twice the bf16 restatement's distance."""
    from landiff_amd.config import VAEConfig
    from landiff_amd.vae_encoder import VAEEncoder
    from landiff_amd.weights import init_state, vae_encoder_spec
    from vae_encoder_ref import encode_moments_ref
    gold = np.load(G)
    cfg = VAEConfig.tiny()
    sd = init_state(vae_encoder_spec(cfg), seed=int(gold["weight_seed"]))
    enc = VAEEncoder(sd, cfg, cuda)
    frames = torch.from_numpy(gold[f"{clip}_frames"])
    eps = torch.from_numpy(gold[f"{clip}_eps"])
    z, mean, _ = enc.encode_moments(frames.to(cuda), eps=eps, want_moments=True)
    mean32 = torch.from_numpy(gold[f"{clip}_mean"])[0].permute(1, 0, 2, 3)          # [T, Z, h, w]
    sample32 = torch.from_numpy(gold[f"{clip}_sample"])[0].permute(1, 0, 2, 3)
    mb, lb = encode_moments_ref(sd, cfg, torch.from_numpy(gold[f"{clip}_x"]).to(cuda), dtype=BF)
    floor = rel(mb[0].permute(1, 0, 2, 3), mean32)
    zb = cfg.scale_factor * (mb + torch.exp(0.5 * lb) * eps.to(cuda))
    zfloor = rel(zb[0].permute(1, 0, 2, 3), sample32)
    err, zerr = rel(mean, mean32), rel(z, sample32)
    print(f"tiny encoder ({clip}): mean err {err:.4f} (bf16 floor {floor:.4f}), sample err {zerr:.4f} (floor {zfloor:.4f})")
    assert err < max(2 * floor, 1e-2) and zerr < max(2 * zfloor, 1e-2)
    lat = enc.encode(frames.to(cuda), sample=True, eps=eps[None])
    assert lat.shape == (1, frames.shape[0] // 4 + (frames.shape[0] % 4 > 0), 16, 4, 6) and torch.equal(lat[0], z)
    assert enc.workspace_bytes() > 0
    enc.release()
    assert enc.workspace_bytes() == 0 and torch.equal(enc.encode(frames.to(cuda), sample=True, eps=eps[None])[0], z)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [17, 49])
def test_encoder_full_width_17_frames(cuda, F):
    """ch 128, ch_mult (1, 2, 2, 4), three blocks per level, a 17- and a 49-frame 480 x 720 clip (extend_video's: level-0 windows
    of 4.2 GiB, activations of 2.2e9 elements): against the fp32 restatement on the GPU within the 2x-floor rule; two runs give
    the same bits.  At 49 frames the restatements run in their sliced mode (no tensor of 2^31 elements)."""
    from landiff_amd.config import VAEConfig
    from landiff_amd.vae_encoder import VAEEncoder
    from landiff_amd.weights import init_state, vae_encoder_spec
    from vae_encoder_ref import encode_moments_ref
    cfg = VAEConfig()
    sd = init_state(vae_encoder_spec(cfg), seed=5, device=cuda)
    enc = VAEEncoder(sd, cfg, cuda)
    g = torch.Generator(device=cuda).manual_seed(3)
    # smooth content (a low-resolution field upsampled) plus noise: closer to video than white noise
    base = torch.rand(F, 3, 30, 45, generator=g, device=cuda)
    img = torch.nn.functional.interpolate(base, size=(480, 720), mode="bilinear", align_corners=False)
    img = img + 0.1 * torch.rand(F, 3, 480, 720, generator=g, device=cuda)
    frames = (img.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    _, mean, _ = enc.encode_moments(frames, want_moments=True)
    _, mean2, _ = enc.encode_moments(frames, want_moments=True)
    assert mean.shape == ((F + 3) // 4, 16, 60, 90) and torch.equal(mean, mean2)
    del mean2
    enc.release()
    x = frames.float() / 127.5 - 1.0
    S = 8 if F > 17 else None
    m32, _ = encode_moments_ref(sd, cfg, x, slice_frames=S)
    m32 = m32[0].permute(1, 0, 2, 3)
    mb, _ = encode_moments_ref(sd, cfg, x, dtype=BF, slice_frames=S)
    floor = rel(mb[0].permute(1, 0, 2, 3), m32)
    err = rel(mean, m32)
    print(f"full-width encoder, {F} x 480 x 720: mean err {err:.4f} (bf16 floor {floor:.4f})")
    assert err < max(2 * floor, 1e-2), (err, floor)


@pytest.mark.gpu
def test_extend_video_equals_the_stream(cuda, setup):
    """extend_video from chunk 0's latent reproduces generate_stream's later chunks bit for bit (same tokens, noises, seeds)."""
    from landiff_amd.pipeline import LanDiffPipeline, synthetic_inputs
    cfg, st = setup
    pipe = LanDiffPipeline(cfg, st, cuda, max_llm_frames=3 * cfg.llm.segment_length)
    d = cfg.dit
    T, new, n_seg = pipe.stream_plan(3, 1)
    inp = synthetic_inputs(cfg, cuda, n_text=6, seed=42)
    tok = pipe.llm.sample(inp.llm_text_emb, motion_score=0.1, num_frames=n_seg * cfg.llm.segment_length, guidance_scale=7.5,
                          seed=42).clone()
    g = torch.Generator().manual_seed(12)
    N = [torch.randn(1, T, d.in_channels, d.latent_h, d.latent_w, generator=g) for _ in range(3)]
    L = []
    Fs = pipe.generate_stream(inp, 3, prefix_frames=1, tokens=tok, noises=N, latents_out=L).clone()
    L2 = []
    ext = pipe.extend_video(inp, 2, prefix_frames=1, clip_latent=L[0], tokens=tok, noises=N[1:], latents_out=L2)
    assert ext.shape == (2 * 4 * new, 8 * d.latent_h, 8 * d.latent_w, 3)
    assert torch.equal(ext, Fs[4 * T - 3:])
    assert all(torch.equal(a, b) for a, b in zip(L2, L[1:]))


@pytest.mark.gpu
def test_extend_video_from_pixels(cuda, setup):
    from landiff_amd.pipeline import LanDiffPipeline, continuation_window, synthetic_inputs
    cfg, st = setup
    pipe = LanDiffPipeline(cfg, st, cuda, max_llm_frames=2 * cfg.llm.segment_length)
    d = cfg.dit
    T, new, n_seg = pipe.stream_plan(2, 1)
    inp = synthetic_inputs(cfg, cuda, n_text=6, seed=43)
    g = torch.Generator().manual_seed(4)
    clip = torch.randint(0, 256, (4 * T - 3 + 2, 8 * d.latent_h, 8 * d.latent_w, 3), generator=g, dtype=torch.uint8)
    tok = torch.randint(0, cfg.tok.codebook_size, (n_seg * cfg.tok.num_latent_tokens,), generator=g).to(cuda)
    L = []
    frames, video = pipe.extend_video(inp, 1, frames=clip, tokens=tok, prefix_frames=1, want_float=True, latents_out=L)
    assert frames.shape == (4 * new, 8 * d.latent_h, 8 * d.latent_w, 3) and frames.dtype == torch.uint8
    assert video.shape == (3, 4 * new, 8 * d.latent_h, 8 * d.latent_w) and torch.isfinite(video).all()
    torch.manual_seed(inp.seed); torch.cuda.manual_seed(inp.seed)
    z = pipe.encoder.encode(continuation_window(clip, cfg).to(cuda), sample=True)
    assert z.shape == (1, T, 16, d.latent_h, d.latent_w) and torch.isfinite(z).all()
    assert torch.equal(L[0][:, :1], z.to(BF).float()[:, T - 1:])
    again = pipe.extend_video(inp, 1, frames=clip, tokens=tok, prefix_frames=1)
    assert torch.equal(again, frames)


@pytest.mark.gpu
def test_llm_prefix_tokens(cuda, setup):
    """prefix_tokens: segment 0 is given (with the schedule's markers), segments 1.. are sampled; the result starts with the
    given ids and the logits after the prefix match the oracle's teacher-forced logits of the whole sequence (2x-floor rule)."""
    from landiff_amd.llm import LLMRunner, forced_token_schedule
    from oracle.llm import LLMOracle
    cfg, st = setup
    c = cfg.llm
    g = torch.Generator().manual_seed(21)
    text = torch.randn(6, c.text_dim, generator=g)
    per_seg = cfg.tok.num_latent_tokens
    seg0 = torch.randint(0, c.visual_vocab, (per_seg,), generator=g)
    nf = 2 * c.segment_length
    run = LLMRunner(st["llm"], c, cuda, max_text=32, max_frames=nf)
    gen = torch.Generator(device=cuda); gen.manual_seed(5)
    log = []
    codes = run.sample(text, num_frames=nf, guidance_scale=7.5, generator=gen, logits_log=log, prefix_tokens=seg0.to(cuda))
    S = text.shape[0] + 3
    full_len, forced, _, n_vis = forced_token_schedule(c, S, nf)
    assert codes.shape == (n_vis,) and n_vis == 2 * per_seg and torch.equal(codes[:per_seg].cpu(), seg0)
    block = c.iframe_len + (c.segment_length - 1) * c.pframe_len + 2 * c.segment_length
    assert forced[S + block] == c.START_I and forced[S + 1 + c.iframe_len] == c.END_I
    # the whole sequence from position S + 1: segment 0 with its forced markers, then what the device emitted
    pre = iter(seg0.tolist())
    raw = iter(run.out_tokens[: n_vis - per_seg].cpu().tolist())
    fed = []
    for i in range(S + 1, full_len):
        if i in forced:
            fed.append(forced[i])
        else:
            fed.append(next(pre) if i < S + block else next(raw))
    dev_logits = torch.cat(log, 0).cpu()
    _, ref = LLMOracle(st["llm"], c, torch.bfloat16).sample(text, num_frames=nf, guidance_scale=7.5, return_logits=True,
                                                           multinomial_fn=lambda p: torch.multinomial(p, 1),
                                                           teacher_tokens=torch.tensor(fed))
    _, ref32 = LLMOracle(st["llm"], c, torch.float32).sample(text, num_frames=nf, guidance_scale=7.5, return_logits=True,
                                                             multinomial_fn=lambda p: torch.multinomial(p, 1),
                                                             teacher_tokens=torch.tensor(fed))
    ref, ref32 = ref[block:], ref32[block:]                  # the steps after the prefix
    assert dev_logits.shape == ref32.shape, (dev_logits.shape, ref32.shape)
    scale = ref32.abs().max().item()
    floor = (ref - ref32).abs().max().item() / scale
    err = (dev_logits - ref32).abs().max().item() / scale
    assert err < max(2 * floor, 2e-2), (err, floor)
    markers = [i for i in range(S + block + 1, full_len) if i in forced]
    assert all(fed[i - S - 1] == forced[i] for i in markers)


@pytest.mark.gpu
def test_cogwrapper_encode_first_stage(cuda, setup, tmp_path):
    """encode_first_stage on a synthetic checkpoint tree whose VAE state carries encoder keys == VAEEncoder.encode(sample=True)
    under the same RNG state; its result, as vae_feature_prefix, runs through forward()."""
    from landiff.diffusion.dif_infer import CogWrapper
    from landiff_amd.config import DiffusionInferConfig
    from landiff_amd.vae_encoder import VAEEncoder
    from landiff_amd.weights import save_checkpoint_tree
    cfg, st = setup
    root = save_checkpoint_tree(str(tmp_path / "ckpt"), st)
    dcfg = DiffusionInferConfig(dit=cfg.dit, tok=cfg.tok, ups=cfg.ups, vae=cfg.vae, sampler=cfg.sampler, t5_dir="",
                                tokenizer_ckpt="", vae_ckpt=os.path.join(root, "CogVideoX-2b-sat", "vae", "3d-vae.pt"),
                                base_dit_ckpt=os.path.join(root, "CogVideoX-2b-sat", "transformer", "1000",
                                                           "mp_rank_00_model_states.pt"),
                                image_size=(8 * cfg.dit.latent_h, 8 * cfg.dit.latent_w), fps=8, bf16=True, force_inference=True)
    d = cfg.dit
    ctx = torch.randn(1, d.text_len, d.text_dim)
    wrap = CogWrapper(dcfg, os.path.join(root, "diffusion"), cuda, text_encoder=lambda prompts: ctx.to(cuda))
    g = torch.Generator().manual_seed(6)
    x = torch.rand(1, 3, 4 * d.latent_frames - 3, 8 * d.latent_h, 8 * d.latent_w, generator=g) * 2 - 1
    torch.cuda.manual_seed(99)
    z = wrap.encode_first_stage(x)
    assert z.shape == (1, 16, d.latent_frames, d.latent_h, d.latent_w)
    enc = VAEEncoder(st["vae"], cfg.vae, cuda)
    torch.cuda.manual_seed(99)
    z2 = enc.encode(x[0].permute(1, 2, 3, 0).contiguous().to(cuda), sample=True)
    assert torch.equal(z, z2.permute(0, 2, 1, 3, 4))
    tok = torch.randint(0, cfg.tok.codebook_size, (cfg.tok.num_latent_tokens,), generator=g)
    out = wrap.forward({"caption": "a", "video": None}, seed=3, semantic_token=tok,
                       vae_feature_prefix=z.permute(0, 2, 1, 3, 4)[:, :1])
    assert out.video.shape == (1, 3, 4 * d.latent_frames - 3, 8 * d.latent_h, 8 * d.latent_w) and torch.isfinite(out.video).all()


@pytest.mark.gpu
def test_infer_video_extend_flag_config0(cuda, tmp_path, monkeypatch):
    """`landiff.infer_video --extend_video` on a synthetic checkpoint tree (BASELINE configs[0] sizes, encoder keys added to the
    VAE checkpoint) writes the clip followed by exactly what LanDiffPipeline.extend_video returns for the same clip, prompt and
    seed; extend_video refuses a clip given twice."""
    import warnings
    import landiff.infer_video as iv
    from facade_helpers import build_config0_workdir
    from landiff_amd.pipeline import LanDiffPipeline, PromptInputs, stream_plan
    from landiff_amd.text import encode_flan_t5, encode_t5_v11
    from landiff_amd.weights import init_state, vae_encoder_spec
    work = str(tmp_path)
    cfg, states = build_config0_workdir(work)
    enc = init_state(vae_encoder_spec(cfg.vae), seed=77)
    vae_path = os.path.join(work, "ckpts", "LanDiff", "CogVideoX-2b-sat", "vae", "3d-vae.pt")
    torch.save({"state_dict": {**torch.load(vae_path, weights_only=False)["state_dict"], **enc}}, vae_path)
    monkeypatch.chdir(work)
    monkeypatch.delenv("LANDIFF_HOME", raising=False)
    monkeypatch.setattr(iv, "build_llm", lambda: cfg.llm)
    d = cfg.dit
    P = 2
    g = torch.Generator().manual_seed(9)
    clip = torch.randint(0, 256, (4 * d.latent_frames - 3 + 3, 8 * d.latent_h, 8 * d.latent_w, 3), generator=g, dtype=torch.uint8)
    np.save("clip.npy", clip.numpy())
    prompt, seed = "a cat runs on the beach", 11
    args = iv.parse_args(["--prompt", prompt, "--seed", str(seed), "--save_file_name", "results/ext", "--extend_video", "clip.npy",
                          "--extend_chunks", "1", "--extend_prefix_frames", str(P)])
    captured = {}
    monkeypatch.setattr(iv, "save_video_tensor", lambda v, p, fps=8: captured.update(video=v, path=p))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = iv.extend_diffusion(args)
    T, new, n_seg = stream_plan(cfg, 2, P)
    assert out.shape == (clip.shape[0] + 4 * new, 8 * d.latent_h, 8 * d.latent_w, 3) and torch.equal(out[:clip.shape[0]], clip)
    assert torch.equal(captured["video"], out) and captured["path"] == "results/ext.mp4"
    # the library call on the same weights, prompt states and seed
    st = dict(states, vae={**states["vae"], **enc})
    pipe = LanDiffPipeline(cfg, st, cuda, max_llm_frames=n_seg * cfg.llm.segment_length)
    text = encode_flan_t5([prompt], cuda, max_length=cfg.llm.max_cond_tokens, model_path=cfg.llm.text_encoder_path)[0]
    ctx = encode_t5_v11([prompt], os.path.join(work, "ckpts", "LanDiff", "CogVideoX-2b-sat", "t5-v1_1-xxl"), d.text_len, cuda)
    inp = PromptInputs(text, ctx, seed=seed, cfg=7.5, motion_score=0.1)
    ref = pipe.extend_video(inp, 1, frames=clip, prefix_frames=P)
    assert torch.equal(out[clip.shape[0]:], ref.cpu())
    with pytest.raises(ValueError, match="exactly one"):
        pipe.extend_video(inp, 1, frames=clip, clip_latent=torch.zeros(1, T, 16, d.latent_h, d.latent_w), prefix_frames=P)
