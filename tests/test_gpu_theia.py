"""GPU tests of the HIP Theia extractor (ld_theia.hip + landiff_amd/theia.py) and its public surfaces.

Oracle: transformers' ViTModel (the DeiT backbone) with seeded random weights at the true DeiT-base shapes, inside a restatement
of TheiaExtractor's interpolate branch (tests/theia_helpers.py).  Error against the fp32 oracle must stay within 2x the same
oracle's own error under bf16 autocast (the project's bf16-floor rule)."""
import os

import numpy as np
import pytest
import torch

from landiff_amd import ops
from landiff_amd.theia import TheiaExtractor, build_theia, load_theia_state
from theia_helpers import hf_vit, oracle_features, pad_square, theia_layout, write_theia

pytestmark = pytest.mark.gpu


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


@pytest.fixture(scope="module")
def deit_base(cuda, tmp_path_factory):
    m = hf_vit(768, 12, 12, seed=11)
    path = write_theia(str(tmp_path_factory.mktemp("theia") / "model.safetensors"), m)
    return m.to(cuda), path


def _frames(cuda, T, H, W, seed):
    """Smooth content plus noise, uint8 [T, H, W, 3]."""
    g = torch.Generator(device=cuda).manual_seed(seed)
    base = torch.rand(T, 3, max(H // 16, 2), max(W // 16, 2), generator=g, device=cuda)
    img = torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
    img = img + 0.15 * torch.rand(T, 3, H, W, generator=g, device=cuda)
    return (img.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _check_vs_oracle(ext, model, frames, shape, what):
    sq = pad_square(frames)
    got = ext(sq)
    want = oracle_features(model, sq, shape, autocast=False)
    floor = rel(oracle_features(model, sq, shape, autocast=True), want)
    err = rel(got, want)
    print(f"theia {what}: err {err:.4f} (bf16 floor {floor:.4f})")
    assert got.shape == want.shape and err <= 2 * floor, (err, floor)
    return got, sq


def test_theia_small_matches_oracle_and_layouts_agree(cuda, deit_base):
    """4 frames at 96 x 128 (-> 128 x 128, an 8 x 8 grid zero-padded to 30 x 45); the unpadded NHWC input (square padding made
    by the kernel) gives the same bits as the padded square, and two runs the same bits."""
    model, path = deit_base
    ext = TheiaExtractor(load_theia_state(path), cuda)
    frames = _frames(cuda, 4, 96, 128, 1)
    got, sq = _check_vs_oracle(ext, model, frames, (30, 45), "4 x 96 x 128")
    assert torch.equal(got[..., 8:, :], torch.zeros_like(got[..., 8:, :])) and torch.equal(got[..., 8:], torch.zeros_like(got[..., 8:]))
    x1, s1 = ext.backbone(frames, nhwc=True)
    x2, s2 = ext.backbone(sq, nhwc=False)
    assert s1 == s2 == 8 and torch.equal(x1, x2)
    assert torch.equal(ext(sq), got)


def test_theia_full_size_13_frames(cuda, deit_base):
    """13 frames at 480 x 720 (-> 720 x 720, 45 x 45 grid, N = 2026 tokens, cropped to the first 30 rows): [13, 768, 30, 45]
    within the 2x-floor rule, bit-identical from run to run."""
    model, path = deit_base
    ext = TheiaExtractor(load_theia_state(path), cuda)
    frames = _frames(cuda, 13, 480, 720, 2)
    got, sq = _check_vs_oracle(ext, model, frames, (30, 45), "13 x 480 x 720")
    assert got.shape == (13, 768, 30, 45)
    assert torch.equal(ext(sq), got)


def test_theia_large_logits_take_the_fallback(cuda, deit_base):
    """q / k of the last layer scaled until the row max of q.k / 8 reaches >= 90 (ViT has no QK-LayerNorm): beyond the window of
    the default launch's max-free fast pass (~76), whose kernel recomputes the query blocks that leave it, and the features stay
    within the 2x-floor rule.  (At 2 frames the launch is the static dispatch, which has the window but keeps no count: -1.)"""
    model, _ = deit_base
    import copy
    big = copy.deepcopy(model)
    last = big.layers[-1]
    grab = {}
    h = last.attention.register_forward_pre_hook(lambda mod, args: grab.update(x=args[0]))
    frames = _frames(cuda, 2, 480, 720, 3)
    sq = pad_square(frames)
    f = 1.0
    for _ in range(8):
        oracle_features(big, sq, (30, 45), autocast=False)
        x = grab["x"][:1]
        q = last.attention.q_proj(x).reshape(x.shape[1], 12, 64).transpose(0, 1)
        k = last.attention.k_proj(x).reshape(x.shape[1], 12, 64).transpose(0, 1)
        mx = (q @ k.transpose(1, 2) / 8).amax().item()
        if mx >= 90:
            break
        s = min(max((95.0 / max(mx, 1.0)) ** 0.5, 1.2), 4.0)
        with torch.no_grad():
            for p in (last.attention.q_proj, last.attention.k_proj):
                p.weight.mul_(s); p.bias.mul_(s)
        f *= s
    h.remove()
    assert mx >= 90, mx
    sd = {k[len("backbone.model."):]: v.cpu() for k, v in theia_layout(big).items()
          if k.startswith("backbone.model.") and "pooler" not in k}
    ext = TheiaExtractor(sd, cuda)
    got = ext(sq)
    cnt = torch.zeros(1, dtype=torch.int32, device=cuda)
    ops.attn_last_fallbacks(cnt)
    want = oracle_features(big, sq, (30, 45), autocast=False)
    floor = rel(oracle_features(big, sq, (30, 45), autocast=True), want)
    err = rel(got, want)
    print(f"theia large logits (max q.k/8 {mx:.1f}, q/k x{f:.2f}): err {err:.4f} (bf16 floor {floor:.4f}), "
          f"fallback blocks in the last launch {int(cnt.item())}")
    from landiff_amd import _lib
    assert _lib.load().ld_attn_last_kernel().decode() in ("ld_attn_q64_kernel", "ld_attn_q64_dyn_kernel")
    assert int(cnt.item()) != 0                                      # a kernel with the window ran (0: none to leave)
    assert err <= 2 * floor, (err, floor)


@pytest.fixture(scope="module")
def small_theia(cuda, tmp_path_factory):
    """config0 widths: Theia width = the tokenizer's out_channels (128), 2 heads, 2 layers; plus a synthetic tokenizer encoder."""
    from landiff_amd.config import TokenizerConfig
    from landiff_amd.tokenizer_encoder import TokenizerEncoder
    from landiff_amd.weights import init_state, tokenizer_encoder_spec
    tc = TokenizerConfig.config0()
    m = hf_vit(128, 2, 2, seed=21)
    path = write_theia(str(tmp_path_factory.mktemp("theia_small") / "model.safetensors"), m)
    enc = TokenizerEncoder(init_state(tokenizer_encoder_spec(tc), 77), tc, cuda)
    return tc, path, enc


def test_tokenize_image_is_the_clip_first_frame(cuda, small_theia):
    """tokenize_image(img) = the first iframe_tokens ids of tokenize_video on any clip that starts with img; tokenize_video equals
    the feature path (extractor -> TokenizerEncoder.encode_to_index) bit for bit."""
    tc, path, enc = small_theia
    ext = build_theia(path, tc, cuda, encoder=enc)
    img = _frames(cuda, 1, 512, 512, 4)[0]
    nI = tc.iframe_tokens
    one = ext.tokenize_image(img)
    assert one.shape == (tc.num_latent_tokens,)
    for seed in (5, 6):
        clip = torch.cat([img[None], _frames(cuda, tc.temporal - 1, 512, 512, seed)])
        ids = ext.tokenize_video(clip)
        assert torch.equal(ids[:nI], one[:nI])
        assert torch.equal(ids, enc.encode_to_index(ext(pad_square(clip))))
    # a non-square frame: padded to the square by the kernel, the 8 x 8 grid zero-padded to 32 x 32
    small = _frames(cuda, tc.temporal, 96, 128, 7)
    assert torch.equal(ext.tokenize_video(small), enc.encode_to_index(ext(pad_square(small))))


@pytest.fixture(scope="module")
def theia_workdir(tmp_path_factory):
    """The config0 checkpoint tree of tests/facade_helpers.py with a tokenizer encoder half, the VAE encoder and a Theia file."""
    from safetensors.torch import load_file, save_file
    from facade_helpers import build_config0_workdir
    from landiff_amd.weights import init_state, tokenizer_encoder_spec, vae_encoder_spec
    work = str(tmp_path_factory.mktemp("theia_config0"))
    cfg, states = build_config0_workdir(work)
    tok_file = os.path.join(work, "ckpts/LanDiff/tokenizer/model.safetensors")
    sd = load_file(tok_file)
    enc = init_state(tokenizer_encoder_spec(cfg.tok), 77)
    enc["quantizer._codebook.embed"] = sd["quantizer._codebook.embed"]
    save_file({**{k: v.contiguous() for k, v in enc.items()}, **sd}, tok_file)
    venc = init_state(vae_encoder_spec(cfg.vae), seed=78)
    vae_path = os.path.join(work, "ckpts", "LanDiff", "CogVideoX-2b-sat", "vae", "3d-vae.pt")
    torch.save({"state_dict": {**torch.load(vae_path, weights_only=False)["state_dict"], **venc}}, vae_path)
    theia = write_theia(os.path.join(work, "theia.safetensors"), hf_vit(cfg.tok.out_channels, cfg.tok.out_channels // 64, 2, seed=31))
    return work, cfg, states, enc, venc, theia


def test_video_task_mp4_with_theia_ckpt(cuda, theia_workdir, monkeypatch):
    """CogModelInferWrapper(theia_ckpt=...)(VideoTask(mp4=...)) = forward(semantic_token=<the explicit extractor's features ->
    TokenizerEncoder>) bit for bit (96 x 128 frames: an 8 x 8 grid zero-padded to the tokenizer's 32 x 32)."""
    from landiff.diffusion.dif_infer import CogModelInferWrapper, VideoTask
    from landiff_amd.tokenizer_encoder import TokenizerEncoder
    work, cfg, states, enc, _, theia = theia_workdir
    monkeypatch.chdir(work)
    monkeypatch.delenv("LANDIFF_HOME", raising=False)
    tc, d = cfg.tok, cfg.dit
    g = torch.Generator().manual_seed(2)
    ctx_states = torch.randn(1, d.text_len, d.text_dim, generator=g)
    mp4 = torch.rand(1, 3, 20, 96, 128, generator=g)
    wrap = CogModelInferWrapper("ckpts/LanDiff/diffusion", text_encoder=lambda p: ctx_states.to(cuda), theia_ckpt=theia)
    task = wrap(VideoTask("v.mp4", "p", 5, mp4=mp4))
    # the explicit path: the facade's frame selection and square padding, the extractor as a feature_extractor callable
    v = (mp4.permute(0, 2, 1, 3, 4) * 2.0 - 1.0).clamp(-1, 1)[0].to(cuda)
    v = v[torch.linspace(0, v.shape[0] - 1, d.latent_frames).long().to(cuda)]
    v = ((v + 1.0) / 2.0).clamp(0, 1).float().mul(255.0 + 1.0 - 1e-3).to(torch.uint8)
    feats = build_theia(theia, tc, cuda)(pad_square(v.permute(0, 2, 3, 1).contiguous()))
    tokens = TokenizerEncoder({**enc}, tc, cuda).encode_to_index(feats)
    want = wrap.init_infer_model.forward(dict(caption="p", video=None), seed=5, semantic_token=tokens)
    assert torch.equal(task.result, want.video.cpu()[0])
    with pytest.raises(ValueError, match="one of"):
        CogModelInferWrapper("ckpts/LanDiff/diffusion", feature_extractor=lambda x: x, theia_ckpt=theia)


def test_extend_video_tokens_from_frames(cuda, theia_workdir):
    """extend_video(clip_tokens="from_frames") = extend_video(clip_tokens=<the Theia tokens of the window's linspace frames>)."""
    from landiff_amd.pipeline import LanDiffPipeline, continuation_window, stream_plan, synthetic_inputs
    from landiff_amd.theia import select_frames
    from landiff_amd.tokenizer_encoder import TokenizerEncoder
    work, cfg, states, enc, venc, theia = theia_workdir
    d, P = cfg.dit, 2
    T, new, n_seg = stream_plan(cfg, 2, P)
    ext = build_theia(theia, cfg.tok, cuda, encoder=TokenizerEncoder({**enc}, cfg.tok, cuda))
    pipe = LanDiffPipeline(cfg, dict(states, vae={**states["vae"], **venc}), cuda,
                           max_llm_frames=n_seg * cfg.llm.segment_length, theia=ext)
    inp = synthetic_inputs(cfg, cuda, n_text=6, seed=12)
    g = torch.Generator().manual_seed(9)
    clip = torch.randint(0, 256, (4 * d.latent_frames - 3 + 2, 8 * d.latent_h, 8 * d.latent_w, 3), generator=g, dtype=torch.uint8)
    out = pipe.extend_video(inp, 1, frames=clip, clip_tokens="from_frames", prefix_frames=P)
    assert pipe.timings.get("theia", 0.0) > 0.0
    tokens = ext.tokenize_video(select_frames(continuation_window(clip, cfg).to(cuda), cfg.tok.temporal))
    assert tokens.shape == (cfg.tok.num_latent_tokens,)
    ref = pipe.extend_video(inp, 1, frames=clip, clip_tokens=tokens, prefix_frames=P)
    assert torch.equal(out, ref)
    with pytest.raises(ValueError, match="from_frames"):
        pipe.extend_video(inp, 1, frames=clip, clip_tokens="frames", prefix_frames=P)


def test_cli_first_frame(cuda, theia_workdir, monkeypatch):
    """`--first_frame img.npy --theia_ckpt ...`: llm_infer decodes from the image's I-frame tokens (use_gt_first_frame) and the
    run writes the token file and the video."""
    import warnings
    import landiff.infer_video as iv
    work, cfg, states, enc, _, theia = theia_workdir
    monkeypatch.chdir(work)
    monkeypatch.delenv("LANDIFF_HOME", raising=False)
    monkeypatch.setattr(iv, "build_llm", lambda: cfg.llm)
    img = _frames(cuda, 1, 8 * cfg.dit.latent_h, 8 * cfg.dit.latent_w, 8)[0].cpu()
    np.save("first.npy", img.numpy())
    args = iv.parse_args(["--prompt", "a dog runs", "--seed", "3", "--save_file_name", "results/ff", "--first_frame", "first.npy",
                          "--theia_ckpt", theia])
    tokens = iv.llm_infer(args)
    nI = cfg.tok.iframe_tokens
    from landiff_amd.tokenizer_encoder import TokenizerEncoder
    want = build_theia(theia, cfg.tok, cuda, encoder=TokenizerEncoder({**enc}, cfg.tok, cuda)).tokenize_image(img.to(cuda))
    assert torch.equal(tokens[:nI].cpu(), want[:nI].cpu())
    assert np.array_equal(np.load("results/ff.npy"), tokens.cpu().numpy())
    monkeypatch.setattr(iv, "save_video_tensor", lambda v, p, fps=8: np.save(p + ".npy", (v * 255).byte().numpy()))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        iv.infer_diffusion(args, tokens)
    assert os.path.exists("results/ff.mp4.npy")
