"""The conform stage on the GPU: ld_resize_u8 against the float64 restatement (tests/conform_ref.py) within half a grey level plus
the fp32 bound of the case's own tables, its exactness properties (copy, constants, crop, gather), ld_resize_mask_u8 against the
restated rule, and extend_video / edit_video / infer_video with conform= against the same calls on pre-conformed inputs."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import conform_ref as ref

pytestmark = pytest.mark.gpu
FILTERS = ["bilinear", "bicubic"]


def rand_u8(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def checkerboard():
    """0 / 255 squares of 4 pixels, [1, 32, 48, 3]: sharp edges everywhere, so the bicubic lobes overshoot both ways."""
    y, x = torch.meshgrid(torch.arange(32), torch.arange(48), indexing="ij")
    return ((((y // 4) + (x // 4)) % 2) * 255).to(torch.uint8)[None, :, :, None].expand(1, 32, 48, 3).contiguous()


# name -> (source builder, (Ho, Wo), crop box or None)
CASES = {
    "down_odd_rows": (lambda: rand_u8((2, 37, 53, 3), 1), (16, 24), None),           # non-integer down-scale, odd row bytes
    "up": (lambda: rand_u8((2, 16, 24, 3), 2), (40, 56), None),
    "taps_36": (lambda: rand_u8((1, 90, 61, 3), 3), (10, 7), None),                  # ratio 9 bicubic: 36 taps, no fixed tap cap
    "row_1x9": (lambda: rand_u8((1, 1, 9, 3), 4), (4, 4), None),
    "pixel_1x1": (lambda: rand_u8((1, 1, 1, 3), 5), (3, 5), None),
    "one_channel": (lambda: rand_u8((2, 37, 53, 1), 6), (16, 24), None),
    "beyond_lds": (lambda: rand_u8((1, 4096, 64, 3), 7), (2, 4), None),              # a footprint of 4096 rows: the direct form
    "workload_ratio": (lambda: rand_u8((1, 2160, 3840, 3), 8), (480, 720), (0, 300, 2160, 3240)),      # the cover box of 4K -> 480 x 720
    "checkerboard_up": (checkerboard, (50, 75), None),
    "checkerboard_down": (checkerboard, (23, 17), None),
}


@functools.lru_cache(maxsize=None)
def source(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name, filt):
    """The case's float64 result, computed once and left unchanged."""
    _, (Ho, Wo), box = CASES[name]
    return ref.resize_ref(source(name), Ho, Wo, filt, box=box)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("name", list(CASES))
def test_resize_within_half_a_level_of_float64(cuda, name, filt):
    """|got - ref64| <= 0.5 + eps for EVERY element, eps = (2 (t_y + t_x) + 4) 2^-24 255 L_y L_x from the case's own tables (about
    3.5e-3 for the 36-tap case; the 4096-row case's own tables give 0.15).  ref64 is the unrounded float64 value clamped to
    [0, 255]: the kernel's one rounding is clamp(round-half-even(v), 0, 255), and where bicubic overshoots the range the clamp, not
    the rounding, decides the byte."""
    from landiff_amd import ops
    _, (Ho, Wo), box = CASES[name]
    src = source(name)
    want = reference(name, filt)
    got = ops.resize_u8(src.to(cuda), (Ho, Wo), box=box, filter=filt)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (src.shape[0], Ho, Wo, src.shape[3])
    hc, wc = (box[2], box[3]) if box else src.shape[1:3]
    eps = ref.eps_bound(hc, wc, Ho, Wo, filt)
    err = (got.cpu().double() - want.clamp(0, 255)).abs()
    print(f"{name} {filt}: max |got - ref64| = {err.max().item():.6f}, eps = {eps:.2e}, "
          f"ref range [{want.min().item():.2f}, {want.max().item():.2f}]")
    assert err.max().item() <= 0.5 + eps
    if name.startswith("checkerboard") and filt == "bicubic":
        assert want.min().item() < -1.0 and want.max().item() > 256.0           # the overshoot is there, and it was clamped
        assert got.min().item() == 0 and got.max().item() == 255


@pytest.mark.parametrize("filt", FILTERS)
def test_copy_and_constants_are_exact(cuda, filt):
    from landiff_amd import ops
    x = rand_u8((2, 33, 47, 3), 11).to(cuda)
    assert torch.equal(ops.resize_u8(x, (33, 47), filter=filt), x)               # same size: weights (1, 0)
    for size in ((16, 24), (70, 90), (3, 200)):
        for v in (0, 255):
            c = torch.full((1, 33, 47, 3), v, dtype=torch.uint8, device=cuda)
            out = ops.resize_u8(c, size, filter=filt)
            assert out.shape == (1,) + size + (3,) and bool((out == v).all()), (size, v)


@pytest.mark.parametrize("filt", FILTERS)
def test_crop_box_reads_nothing_outside(cuda, filt):
    from landiff_amd import ops
    box = (3, 5, 30, 45)
    x = rand_u8((2, 41, 59, 3), 12)
    sliced = x[:, 3:33, 5:50].contiguous()
    got = ops.resize_u8(x.to(cuda), (16, 24), box=box, filter=filt)
    assert torch.equal(got, ops.resize_u8(sliced.to(cuda), (16, 24), filter=filt))          # bit for bit
    y = torch.full((1, 41, 59, 3), 255, dtype=torch.uint8)
    y[:, 3:33, 5:50] = 0
    assert not ops.resize_u8(y.to(cuda), (16, 24), box=box, filter=filt).any()
    assert not ops.resize_u8(y.to(cuda), (50, 70), box=box, filter=filt).any()


def test_frame_gather_equals_per_frame_calls(cuda):
    from landiff_amd import ops
    x = rand_u8((5, 37, 53, 3), 13).to(cuda)
    idx = [4, 4, 0, 2]
    got = ops.resize_u8(x, (16, 24), frame_idx=idx, filter="bicubic")
    each = torch.cat([ops.resize_u8(x[i:i + 1].contiguous(), (16, 24), filter="bicubic") for i in idx])
    assert got.shape == (4, 16, 24, 3) and torch.equal(got, each)
    assert torch.equal(ops.resize_u8(x, (16, 24), frame_idx=torch.tensor(idx), filter="bicubic"), got)
    assert torch.equal(ops.resize_u8(x, (16, 24), frame_idx=list(range(5)), filter="bicubic"), ops.resize_u8(x, (16, 24), filter="bicubic"))
    m = (rand_u8((5, 37, 53), 14) > 40).to(cuda)
    assert torch.equal(ops.resize_mask_u8(m, (16, 24), frame_idx=idx),
                       torch.cat([ops.resize_mask_u8(m[i:i + 1].contiguous(), (16, 24)) for i in idx]))


@pytest.mark.parametrize("filt", FILTERS)
def test_mask_single_hole(cuda, filt):
    """One zero source pixel: exactly the destination pixels whose window [lo_y, hi_y) x [lo_x, hi_x) holds it are 0."""
    from landiff_amd import ops
    for (H, W), (Ho, Wo), (py, px) in (((37, 53), (16, 24), (20, 31)), ((16, 24), (40, 56), (0, 23)), ((90, 61), (10, 7), (89, 0))):
        m = torch.ones(1, H, W, dtype=torch.uint8)
        m[0, py, px] = 0
        ly, hy, _ = ref.tables(H, Ho, filt)
        lx, hx, _ = ref.tables(W, Wo, filt)
        want = torch.ones(Ho, Wo, dtype=torch.uint8)
        rows = [i for i in range(Ho) if ly[i] <= py < hy[i]]
        cols = [j for j in range(Wo) if lx[j] <= px < hx[j]]
        assert rows and cols
        for i in rows:
            for j in cols:
                want[i, j] = 0
        got = ops.resize_mask_u8(m.to(cuda), (Ho, Wo), filter=filt)
        assert got.dtype == torch.uint8 and torch.equal(got[0].cpu(), want), ((H, W), filt)


@pytest.mark.parametrize("filt", FILTERS)
def test_mask_matches_the_restatement(cuda, filt):
    from landiff_amd import ops
    for seed, (F, H, W), (Ho, Wo), box, idx, thr in ((1, (2, 37, 53), (16, 24), None, None, 6), (2, (3, 16, 24), (40, 56), None, [2, 0, 2], 40),
                                                     (3, (1, 90, 61), (10, 7), None, None, 1), (4, (2, 41, 59), (16, 24), (3, 5, 30, 45), [1], 3),
                                                     (5, (1, 4096, 64), (2, 4), None, None, 0), (6, (1, 300, 500), (64, 96), None, None, 2)):
        m = (rand_u8((F, H, W), 100 + seed) >= thr).to(torch.uint8)             # sparse holes, so that both outcomes occur
        if seed == 5:
            m[0, 3500, 4] = 0                                                   # the 4096-row case: one hole, in some windows only
        want = ref.mask_ref(m, Ho, Wo, filt, box=box, frame_idx=idx)
        got = ops.resize_mask_u8(m.to(cuda), (Ho, Wo), box=box, frame_idx=idx, filter=filt)
        assert torch.equal(got.cpu(), want), (seed, filt)
        assert 0 < int(want.sum()) < want.numel() or seed == 3, seed
    # any non-zero byte is keep; bool masks are taken as they are
    m = torch.full((1, 20, 30), 2, dtype=torch.uint8)
    m[0, :, 15:] = 255
    assert bool((ops.resize_mask_u8(m.to(cuda), (8, 12), filter=filt) == 1).all())
    b = rand_u8((1, 20, 30), 9) > 10
    assert torch.equal(ops.resize_mask_u8(b.to(cuda), (8, 12), filter=filt), ops.resize_mask_u8(b.to(torch.uint8).to(cuda) * 7, (8, 12), filter=filt))


# ---- the pipelines -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(cuda):
    """The tiny pipeline of tests/test_gpu_edit.py (VAE encoder weights added, a 4-step sampler), a 13-frame 50 x 70 clip at 12 fps
    and a keep-mask in that clip's own geometry: the right part of every frame and the last 3 frames."""
    from landiff_amd.config import PipelineConfig
    from landiff_amd.pipeline import LanDiffPipeline, synthetic_inputs
    from landiff_amd.weights import init_pipeline_state, init_state, vae_encoder_spec
    cfg = PipelineConfig.tiny(num_steps=4).check()
    st = init_pipeline_state(cfg, seed=1234)
    st["vae"] = dict(st["vae"], **init_state(vae_encoder_spec(cfg.vae), seed=77))
    pipe = LanDiffPipeline(cfg, st, cuda, max_llm_frames=2 * cfg.llm.segment_length)
    inp = synthetic_inputs(cfg, cuda, n_text=6, seed=43)
    g = torch.Generator().manual_seed(4)
    clip = torch.randint(0, 256, (13, 50, 70, 3), generator=g, dtype=torch.uint8)
    tok = torch.randint(0, cfg.tok.codebook_size, (2 * cfg.tok.num_latent_tokens,), generator=g).to(cuda)
    keep = torch.zeros(13, 50, 70, dtype=torch.bool)
    keep[:, :, 30:] = True
    keep[10:] = True
    return cfg, pipe, inp, clip, tok, keep


def _plan(cfg, clip, conf):
    from landiff_amd.conform import conform_plan
    d = cfg.dit
    return conform_plan(tuple(clip.shape), 4 * d.latent_frames - 3, 8 * d.latent_h, 8 * d.latent_w, conf)


def test_edit_video_conform_equals_preconformed(cuda, tiny):
    from landiff_amd.conform import ConformConfig, conform_clip, conform_mask
    cfg, pipe, inp, clip, tok, keep = tiny
    tok1 = tok[:cfg.tok.num_latent_tokens]
    conf = ConformConfig(fit="cover", src_fps=12)
    plan = _plan(cfg, clip, conf)
    assert plan.box == (2, 0, 46, 70) and plan.frame_idx == (0, 1, 3, 4, 6, 7, 9, 10, 12) and plan.out_shape == (9, 64, 96)
    pipe.timings.pop("conform", None)
    L, L2 = [], []
    got = pipe.edit_video(inp, frames=clip, keep_mask=keep, conform=conf, tokens=tok1, strength=0.5, latents_out=L)
    assert pipe.timings.get("conform", 0.0) > 0.0
    lc = pipe.last_conform
    assert lc == plan.as_dict() and lc["box"] == [2, 0, 46, 70] and lc["frame_idx"] == list(plan.frame_idx) and lc["fit"] == "cover"
    assert lc["filter"] == "bilinear" and lc["src_fps"] == 12.0 and (lc["scale_y"], lc["scale_x"]) == (46 / 64, 70 / 96)
    assert set(pipe.last_edit) == {"strength", "start_step", "steps_run", "alpha_start", "sigma_start", "kept_cells", "total_cells", "tokens_source"}
    pre_clip, pre_mask = conform_clip(clip, plan, cuda), conform_mask(keep, plan, cuda)
    assert pre_clip.shape == (9, 64, 96, 3) and pre_mask.shape == (9, 64, 96) and pre_mask.dtype == torch.bool
    assert torch.equal(pipe.last_conform_frames, pre_clip)
    want64 = ref.resize_ref(clip, 64, 96, "bilinear", box=plan.box, frame_idx=plan.frame_idx)
    assert (pre_clip.cpu().double() - want64).abs().max().item() <= 0.5 + ref.eps_bound(46, 70, 64, 96, "bilinear")
    assert torch.equal(pre_mask.cpu(), ref.mask_ref(keep, 64, 96, "bilinear", box=plan.box, frame_idx=plan.frame_idx).bool())
    assert 0 < int(pre_mask.sum()) < pre_mask.numel()
    want = pipe.edit_video(inp, frames=pre_clip, keep_mask=pre_mask, tokens=tok1, strength=0.5, latents_out=L2)
    assert torch.equal(got, want) and torch.equal(L[0], L2[0])
    assert torch.equal(got[pre_mask], pre_clip[pre_mask])                        # the composite uses the conformed clip
    # a latent-cell mask is not in the clip's geometry: it is taken as it is
    lat = torch.zeros(3, 8, 12, dtype=torch.bool)
    lat[:, :, 6:] = True
    a = pipe.edit_video(inp, frames=clip, keep_mask=lat, conform=conf, tokens=tok1, strength=0.5)
    assert torch.equal(a, pipe.edit_video(inp, frames=pre_clip, keep_mask=lat, tokens=tok1, strength=0.5))
    with pytest.raises(ValueError, match="frames="):
        pipe.edit_video(inp, clip_latent=torch.zeros(1, 3, 16, 8, 12), conform=conf, tokens=tok1)
    with pytest.raises(ValueError, match=r"need 1\.0 s"):
        pipe.edit_video(inp, frames=clip[:12], conform=conf, tokens=tok1)
    with pytest.raises(ValueError, match="keep_mask must be bool"):
        pipe.edit_video(inp, frames=clip, keep_mask=keep.to(torch.uint8), conform=conf, tokens=tok1)


def test_extend_video_conform_equals_preconformed(cuda, tiny):
    from landiff_amd.conform import ConformConfig, conform_clip
    cfg, pipe, inp, clip, tok, keep = tiny
    conf = ConformConfig(fit="stretch", src_fps=12, filter="bicubic")
    plan = _plan(cfg, clip, conf)
    assert plan.box == (0, 0, 50, 70) and plan.frame_idx[-1] == 12
    L, L2 = [], []
    got = pipe.extend_video(inp, 1, frames=clip, tokens=tok, prefix_frames=1, conform=conf, latents_out=L)
    assert pipe.last_conform == plan.as_dict() and pipe.last_conform["filter"] == "bicubic"
    pre = conform_clip(clip, plan, cuda)
    assert torch.equal(pipe.last_conform_frames, pre)
    want = pipe.extend_video(inp, 1, frames=pre, tokens=tok, prefix_frames=1, latents_out=L2)
    assert got.shape == (8, 64, 96, 3) and torch.equal(got, want) and torch.equal(L[0], L2[0])


def test_conform_off_changes_nothing(cuda, tiny, monkeypatch):
    """conform=None and fit="exact": the bits, the refusals and the launches of the code before the conform stage -- not one
    resize launch, last_conform untouched."""
    from landiff_amd import ops
    from landiff_amd.conform import ConformConfig
    cfg, pipe, inp, clip, tok, keep = tiny
    tok1 = tok[:cfg.tok.num_latent_tokens]
    calls = []
    for name in ("resize_u8", "resize_mask_u8"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, **k: (calls.append(1), _real(*a, **k))[1])
    pipe.last_conform = pipe.last_conform_frames = None
    pipe.timings.pop("conform", None)
    model_clip = rand_u8((11, 64, 96, 3), 21)
    m = torch.zeros(9, 64, 96, dtype=torch.bool)
    m[:, :, 48:] = True
    e0 = pipe.edit_video(inp, frames=model_clip[2:], keep_mask=m, tokens=tok1, strength=0.5)
    e1 = pipe.edit_video(inp, frames=model_clip[2:], keep_mask=m, tokens=tok1, strength=0.5, conform=None)
    e2 = pipe.edit_video(inp, frames=model_clip[2:], keep_mask=m, tokens=tok1, strength=0.5, conform=ConformConfig())
    assert torch.equal(e0, e1) and torch.equal(e0, e2)
    x0 = pipe.extend_video(inp, 1, frames=model_clip, tokens=tok, prefix_frames=1)
    x2 = pipe.extend_video(inp, 1, frames=model_clip, tokens=tok, prefix_frames=1, conform=ConformConfig(fit="exact"))
    assert torch.equal(x0, x2)
    for conf in (None, ConformConfig()):
        with pytest.raises(ValueError, match=r"uint8 \[9, 64, 96, 3\]"):
            pipe.edit_video(inp, frames=clip, tokens=tok1, conform=conf)
        with pytest.raises(ValueError, match=r"clip frames must be \[F, 64, 96, 3\]"):
            pipe.extend_video(inp, 1, frames=clip, tokens=tok, prefix_frames=1, conform=conf)
        with pytest.raises(ValueError, match="keep_mask must be bool"):
            pipe.edit_video(inp, frames=model_clip[2:], keep_mask=keep, tokens=tok1, conform=conf)
    assert not calls and pipe.last_conform is None and pipe.last_conform_frames is None and "conform" not in pipe.timings


def test_conform_image(cuda):
    from landiff_amd.conform import ConformConfig, conform_image
    img = rand_u8((50, 70, 3), 31)
    out = conform_image(img, 64, 96, ConformConfig(fit="cover", filter="bicubic"), cuda)
    want = ref.resize_ref(img[None], 64, 96, "bicubic", box=(2, 0, 46, 70))[0]
    assert out.shape == (64, 96, 3)
    assert (out.cpu().double() - want.clamp(0, 255)).abs().max().item() <= 0.5 + ref.eps_bound(46, 70, 64, 96, "bicubic")


def test_infer_video_edit_with_clip_fit(cuda, tmp_path, monkeypatch):
    """`landiff.infer_video --edit_video ... --clip_fit cover --clip_fps 12` on the synthetic checkpoint tree: a 50 x 70 clip at 12 fps
    with a mask in its own geometry gives the video edit_video(conform=...) gives, and <name>_conform.json holds last_conform."""
    import warnings
    import landiff.infer_video as iv
    from facade_helpers import build_config0_workdir
    from landiff_amd.conform import ConformConfig
    from landiff_amd.pipeline import LanDiffPipeline, PromptInputs
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
    n_frames = 4 * d.latent_frames - 3
    F = (n_frames - 1) * 12 // 8 + 2                       # one frame more than the window needs: window="last" skips frame 0
    clip = rand_u8((F, 50, 70, 3), 9)
    keep = torch.zeros(F, 50, 70, dtype=torch.bool)
    keep[:, :, 35:] = True
    np.save("clip.npy", clip.numpy())
    np.save("mask.npy", keep.numpy().astype(np.uint8))
    prompt, seed = "a cat runs on the beach", 11
    args = iv.parse_args(["--prompt", prompt, "--seed", str(seed), "--save_file_name", "results/ed", "--edit_video", "clip.npy",
                          "--edit_strength", "0.5", "--edit_mask", "mask.npy", "--clip_fit", "cover", "--clip_fps", "12"])
    captured = {}
    monkeypatch.setattr(iv, "save_video_tensor", lambda v, p, fps=8: captured.update(video=v, path=p))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = iv.edit_diffusion(args)
    n = 1 + 8 * ((d.latent_frames - 1) // 2)
    assert out.shape == (n, 8 * d.latent_h, 8 * d.latent_w, 3) and torch.equal(captured["video"], out) and captured["path"] == "results/ed.mp4"
    pipe = LanDiffPipeline(cfg, dict(states, vae={**states["vae"], **enc}), cuda)
    text = encode_flan_t5([prompt], cuda, max_length=cfg.llm.max_cond_tokens, model_path=cfg.llm.text_encoder_path)[0]
    ctx = encode_t5_v11([prompt], os.path.join(work, "ckpts", "LanDiff", "CogVideoX-2b-sat", "t5-v1_1-xxl"), d.text_len, cuda)
    inp = PromptInputs(text, ctx, seed=seed, cfg=7.5, motion_score=0.1)
    want = pipe.edit_video(inp, frames=clip, strength=0.5, keep_mask=keep, conform=ConformConfig(fit="cover", src_fps="12"))
    assert torch.equal(out, want.cpu())
    got = json.load(open("results/ed_conform.json"))
    assert got == pipe.last_conform and got["fit"] == "cover" and got["src_fps"] == 12.0 and got["box"] == [0, 10, 50, 50]
    assert got["frame_idx"][-1] == F - 1 and got["frame_idx"][0] == 1 and len(got["frame_idx"]) == n_frames
    assert os.path.exists("results/ed_edit.json")
