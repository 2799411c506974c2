"""GPU tests of clip editing: the two kernels of ld_edit.hip element by element, the sampler's start / known / known_mask arguments
against the CPU restatement (tests/edit_ref.py), LanDiffPipeline.edit_video end to end on tiny pipelines, and the command line."""
import json
import os

import numpy as np
import pytest
import torch

from edit_ref import edit_run_ref, mask_to_latent_ref, pin_ref
from test_gpu_theia import theia_workdir          # noqa: F401  (the config0 tree with a tokenizer encoder, a VAE encoder and a Theia file)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def nan_sentinels(shape):
    """fp32 NaNs whose payload is the element's index (mod 2^16): an element that moved, or was written, shows in its bits."""
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.int32) & 0xFFFF) | 0x7FC00000).view(torch.float32).reshape(shape)


# ---- 1. ld_latent_pin -----------------------------------------------------------------------------------
# [3, 4, 5, 7]: 420 elements, odd W, a partial last block (an index that forgets C shows); [5, 16, 30, 45]: many blocks;
# [13, 16, 120, 180]: 4.5 M elements, more than the 16384 x 256 threads of the largest grid, so the grid-stride loop iterates.
@pytest.mark.parametrize("shape", [(3, 4, 5, 7), (5, 16, 30, 45), (13, 16, 120, 180)])
def test_latent_pin_is_exact(cuda, shape):
    """Written elements equal CPU fp32 `alpha*known + sigma*noise` bit for bit (the same three separately rounded IEEE operations),
    or `known` with noise None; unwritten elements keep their bits (NaN sentinels)."""
    from landiff_amd import ops
    from landiff_amd.config import SamplerConfig
    from landiff_amd.schedule import step_alphas
    T, C, H, W = shape
    g = torch.Generator().manual_seed(T * 1000 + W)
    known, noise = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    one = torch.zeros(T, H, W, dtype=torch.uint8)
    one[T - 1, H // 2, W - 1] = 1
    masks = {"random": (torch.rand(T, H, W, generator=g) < 0.5).to(torch.uint8), "one cell": one, "all but one": 1 - one,
             "bool": torch.rand(T, H, W, generator=g) < 0.3, "none": None}
    if T == 13:                                                        # the large shape is about the grid stride alone
        masks = {k: masks[k] for k in ("random", "none")}
    al = step_alphas(SamplerConfig(num_steps=6))
    kd, nd = known.to(cuda), noise.to(cuda)
    for name, m in masks.items():
        md = m.to(cuda) if m is not None else None
        for alpha, sigma in (al[2], al[0], al[5]):
            x0 = nan_sentinels(shape)
            x = x0.to(cuda)
            ops.latent_pin(x, kd, nd, md, alpha, sigma)
            assert torch.equal(bits(x), bits(pin_ref(x0, known, noise, m, alpha, sigma))), (name, alpha)
        x0 = nan_sentinels(shape)                                      # noise None: a copy
        x = x0.to(cuda)
        ops.latent_pin(x, kd, None, md, al[2][0], al[2][1])
        assert torch.equal(bits(x), bits(pin_ref(x0, known, None, m, 1.0, 0.0))), name
        x = noise.to(cuda)                                             # noise aliasing x: x = alpha*known + sigma*x
        ops.latent_pin(x, kd, x, md, *al[3])
        assert torch.equal(bits(x), bits(pin_ref(noise, known, noise, m, *al[3]))), name
    x = nan_sentinels((1, 1) + shape).to(cuda)                         # leading 1s, as the sampler's state has
    ops.latent_pin(x, kd.reshape(x.shape), nd.reshape(x.shape), masks["random"].to(cuda), *al[4])
    assert torch.equal(bits(x)[0, 0], bits(pin_ref(nan_sentinels(shape), known, noise, masks["random"], *al[4])))


# ---- 2. ld_mask_to_latent -------------------------------------------------------------------------------
def test_mask_to_latent(cuda):
    """F = 9, 16 x 24 pixels -> [3, 2, 3]: random masks, single-pixel holes at the corners of a block in the frames at the causal
    boundaries (0 | 1 .. 4 | 5 .. 8), any non-zero byte counts as keep; the three refusals."""
    from landiff_amd import _lib, ops
    g = torch.Generator().manual_seed(2)
    full = torch.ones(9, 16, 24, dtype=torch.bool)
    assert torch.equal(ops.mask_to_latent(full.to(cuda)).cpu(), torch.ones(3, 2, 3, dtype=torch.uint8))
    for p in (0.001, 0.01, 0.5):
        m = torch.rand(9, 16, 24, generator=g) >= p
        got = ops.mask_to_latent(m.to(cuda))
        assert got.dtype == torch.uint8 and torch.equal(got.cpu(), mask_to_latent_ref(m)), p
    for f, t in ((0, 0), (1, 1), (4, 1), (5, 2), (8, 2)):
        for r, c in ((8, 16), (8, 23), (15, 16), (15, 23)):            # the corners of block (1, 2)
            m = full.clone()
            m[f, r, c] = False
            want = torch.ones(3, 2, 3, dtype=torch.uint8)
            want[t, 1, 2] = 0
            assert torch.equal(mask_to_latent_ref(m), want)
            assert torch.equal(ops.mask_to_latent(m.to(cuda)).cpu(), want), (f, r, c)
    u8 = torch.randint(0, 256, (9, 16, 24), generator=g, dtype=torch.uint8)          # ~1 zero byte in 256
    assert torch.equal(ops.mask_to_latent(u8.to(cuda)).cpu(), mask_to_latent_ref(u8))
    big = torch.rand(13, 64, 96, generator=g) >= 0.002                                # more cells than one block of threads
    assert torch.equal(ops.mask_to_latent(big.to(cuda)).cpu(), mask_to_latent_ref(big))
    for shape, msg in (((8, 16, 24), "4k \\+ 1"), ((9, 12, 24), "multiples of 8"), ((9, 16, 20), "multiples of 8")):
        with pytest.raises(_lib.LandiffHipError, match=msg):
            ops.mask_to_latent(torch.ones(shape, dtype=torch.uint8, device=cuda))


# ---- 3-5. the sampler loop ------------------------------------------------------------------------------
def _step(x, timestep, c_out, c_skip, scale, out):
    """Analytic denoiser: network eps = 0.5 * x for both CFG halves (torch here only plays the "network")."""
    from landiff_amd import ops
    ops.axpbypcz(out, 0.5 * x, c_out, x, c_skip)
    return out


class Draws:
    """randn_like that hands out a fixed list, counting the calls."""
    def __init__(self, noises, dev=None):
        self.noises, self.dev, self.calls = noises, dev, 0

    def __call__(self, t):
        v = self.noises[self.calls]
        self.calls += 1
        return v.to(self.dev) if self.dev is not None else v


@pytest.fixture(scope="module")
def loop_inputs():
    g = torch.Generator().manual_seed(5)
    shape = (1, 3, 4, 8, 12)
    x0 = torch.randn(shape, generator=g)
    noises = [torch.randn(shape, generator=g) for _ in range(24)]
    known = torch.randn(shape, generator=g)
    mask = torch.rand(3, 8, 12, generator=g) < 0.4
    return x0, noises, known, mask


@pytest.mark.parametrize("kind,n", [("vpsde_dpmpp2m", 6), ("ddim", 5)])
def test_sampler_edit_loop_matches_the_restatement(cuda, loop_inputs, kind, n):
    """start in {0, 2, last} x {unmasked, masked re-noised, masked clean}: the device loop reproduces the fp32 CPU restatement to
    fp32 rounding (test_sampler_loop_matches_oracle's bound), kept cells are `known` exactly, and both sides draw as often."""
    from landiff_amd.config import SamplerConfig
    from landiff_amd.sampler import DiffusionSampler
    x0, noises, known, mask = loop_inputs
    sc = SamplerConfig(num_steps=n, sampler=kind)
    smp = DiffusionSampler(sc)
    net = lambda xx, idx, c: 0.5 * xx
    for start in (0, 2, n - 1):
        for m, kn in ((None, True), (mask, True), (mask, False)):
            cpu, gpu = Draws(noises), Draws(noises, cuda)
            ref = edit_run_ref(sc, net, x0, cpu, start=start, known=known, known_mask=m, known_noise=kn)
            trace = []
            res = smp.run(_step, x0.to(cuda), randn_like=gpu, trace=trace, start=start, known=known.to(cuda),
                          known_mask=None if m is None else m.to(cuda), known_noise=kn)
            what = (kind, start, m is not None, kn)
            assert [t[0] for t in trace] == list(range(start, n)), what
            assert rel(res, ref) < 1e-5, (what, rel(res, ref))
            assert gpu.calls == cpu.calls, (what, gpu.calls, cpu.calls)
            if m is not None:
                assert torch.equal(res.cpu()[:, m[:, None].expand(3, 4, 8, 12)], known[:, m[:, None].expand(3, 4, 8, 12)]), what
                assert cpu.calls >= (n - start if kn else 0)
    # a start step without a known latent runs the tail of the plan on the caller's state
    cpu, gpu = Draws(noises), Draws(noises, cuda)
    ref = edit_run_ref(sc, net, x0, cpu, start=2)
    assert rel(smp.run(_step, x0.to(cuda), randn_like=gpu, start=2), ref) < 1e-5 and gpu.calls == cpu.calls


def test_prefix_mask_equals_fixed_frames(cuda, loop_inputs):
    """A clean pin of the first latent frame is the streaming primitive: the same bits, the same draws."""
    from landiff_amd.config import SamplerConfig
    from landiff_amd.sampler import DiffusionSampler
    x0, noises, known, _ = loop_inputs
    first = torch.zeros(3, 8, 12, dtype=torch.bool)
    first[0] = True
    for kind, n in (("vpsde_dpmpp2m", 6), ("ddim", 5)):
        smp = DiffusionSampler(SamplerConfig(num_steps=n, sampler=kind))
        a, b = Draws(noises, cuda), Draws(noises, cuda)
        want = smp.run(_step, x0.to(cuda), randn_like=a, prefix=known[:, :1].to(cuda), fixed_frames=1)
        got = smp.run(_step, x0.to(cuda), randn_like=b, known=known.to(cuda), known_mask=first.to(cuda), known_noise=False)
        assert torch.equal(got, want) and a.calls == b.calls, kind
        assert torch.equal(got[:, :1].cpu(), known[:, :1])


def test_defaults_change_nothing(cuda, loop_inputs, monkeypatch):
    """With the new arguments at their defaults the run launches no pin and draws nothing more: it equals the oracle's loop as
    before, draw for draw, and a run with the defaults spelled out (or a `known` that has nothing to do at start 0) is the same."""
    from landiff_amd import ops
    from landiff_amd.config import SamplerConfig
    from landiff_amd.sampler import DiffusionSampler
    from oracle.sampler import DiffusionSamplerOracle
    x0, noises, known, _ = loop_inputs
    pins = []
    real = ops.latent_pin
    monkeypatch.setattr(ops, "latent_pin", lambda *a, **k: (pins.append(1), real(*a, **k))[1])
    for kind, n in (("vpsde_dpmpp2m", 6), ("ddim", 5)):
        sc = SamplerConfig(num_steps=n, sampler=kind)
        smp = DiffusionSampler(sc)
        cpu = Draws(noises)
        ref = DiffusionSamplerOracle(sc).run(lambda xx, idx, c: 0.5 * xx, x0.clone(), torch.zeros(1, 2, 4), torch.zeros(1, 2, 4), randn_like=cpu)
        a, b, c = Draws(noises, cuda), Draws(noises, cuda), Draws(noises, cuda)
        plain = smp.run(_step, x0.to(cuda), randn_like=a)
        assert not pins and a.calls == cpu.calls == (0 if kind == "ddim" else 1 + 2 * (n - 2))
        assert rel(plain, ref) < 1e-5
        spelled = smp.run(_step, x0.to(cuda), randn_like=b, start=0, known=None, known_mask=None, known_noise=True)
        idle = smp.run(_step, x0.to(cuda), randn_like=c, known=known.to(cuda))
        assert torch.equal(spelled, plain) and torch.equal(idle, plain) and b.calls == c.calls == a.calls and not pins


# ---- 6. edit_video end to end ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_edit(cuda):
    """The tiny pipeline of test_extend_video_from_pixels (VAE encoder weights added) with a 4-step sampler, a clip, tokens and the
    keep-mask of the issue: the right half of every frame and the last 4 frames."""
    from landiff_amd.config import PipelineConfig
    from landiff_amd.pipeline import LanDiffPipeline, synthetic_inputs
    from landiff_amd.weights import init_pipeline_state, init_state, vae_encoder_spec
    cfg = PipelineConfig.tiny(num_steps=4).check()
    st = init_pipeline_state(cfg, seed=1234)
    st["vae"] = dict(st["vae"], **init_state(vae_encoder_spec(cfg.vae), seed=77))
    pipe = LanDiffPipeline(cfg, st, cuda)
    d = cfg.dit
    inp = synthetic_inputs(cfg, cuda, n_text=6, seed=43)
    g = torch.Generator().manual_seed(4)
    F, Hp, Wp = 4 * d.latent_frames - 3, 8 * d.latent_h, 8 * d.latent_w
    clip = torch.randint(0, 256, (F, Hp, Wp, 3), generator=g, dtype=torch.uint8)
    tok = torch.randint(0, cfg.tok.codebook_size, (cfg.tok.num_latent_tokens,), generator=g).to(cuda)
    keep = torch.zeros(F, Hp, Wp, dtype=torch.bool)
    keep[:, :, Wp // 2:] = True
    keep[F - 4:] = True
    return cfg, st, pipe, inp, clip, tok, keep


def _encoded(pipe, inp, clip, cuda):
    torch.manual_seed(inp.seed); torch.cuda.manual_seed(inp.seed)
    return pipe.encoder.encode(clip.to(cuda), sample=True).to(BF).float()


def test_edit_video_full_strength_is_generation(cuda, tiny_edit):
    cfg, st, pipe, inp, clip, tok, keep = tiny_edit
    L = []
    frames = pipe.edit_video(inp, strength=1.0, tokens=tok, frames=clip, latents_out=L)
    z = pipe.generate_latent(tok, inp)
    assert torch.equal(L[0], z.to(BF).float()) and torch.equal(frames, pipe.decode(z))
    e = pipe.last_edit
    assert (e["start_step"], e["steps_run"], e["alpha_start"], e["sigma_start"]) == (0, 4, 0.0, 1.0)
    assert (e["kept_cells"], e["total_cells"], e["tokens_source"], e["strength"]) == (0, 3 * 8 * 12, "given", 1.0)
    # an all-False mask is no mask; the clip given as its latent gives the same run
    L2 = []
    pipe.edit_video(inp, strength=1.0, tokens=tok, clip_latent=_encoded(pipe, inp, clip, cuda), keep_mask=torch.zeros(3, 8, 12, dtype=torch.bool),
                    latents_out=L2)
    assert torch.equal(L2[0], L[0]) and pipe.last_edit["kept_cells"] == 0


def test_edit_video_masked_half_strength(cuda, tiny_edit):
    from landiff_amd.pipeline import edit_start_step
    cfg, st, pipe, inp, clip, tok, keep = tiny_edit
    d = cfg.dit
    L, L2 = [], []
    frames, video = pipe.edit_video(inp, strength=0.5, tokens=tok, frames=clip, keep_mask=keep, want_float=True, latents_out=L)
    again = pipe.edit_video(inp, strength=0.5, tokens=tok, frames=clip, keep_mask=keep, latents_out=L2)
    assert frames.shape == clip.shape and frames.dtype == torch.uint8 and torch.isfinite(video).all()
    assert torch.equal(again, frames) and torch.equal(L2[0], L[0])
    mlat = mask_to_latent_ref(keep)                                               # [3, 8, 12]: frame 2 and columns 6.. kept
    assert mlat[2].all() and mlat[:, :, 6:].all() and not mlat[:2, :, :6].any()
    start = edit_start_step(4, 0.5)
    e = pipe.last_edit
    assert start == 2 and (e["start_step"], e["steps_run"], e["kept_cells"], e["tokens_source"]) == (2, 2, int(mlat.sum()), "given")
    assert (e["alpha_start"], e["sigma_start"]) == pipe.sampler.alphas[2]
    z0 = _encoded(pipe, inp, clip, cuda)
    cells = (mlat != 0)[:, None].expand(3, d.in_channels, 8, 12)
    assert torch.equal(L[0].cpu()[:, cells], z0.cpu()[:, cells])                  # kept latent cells: the encoded clip's
    assert not torch.equal(L[0].cpu()[:, ~cells], z0.cpu()[:, ~cells])
    assert torch.equal(frames.cpu()[keep], clip[keep])                            # kept pixels: the clip's own (composite)
    raw = pipe.edit_video(inp, strength=0.5, tokens=tok, frames=clip, keep_mask=keep, composite=False)
    assert torch.equal(raw.cpu()[~keep], frames.cpu()[~keep]) and not torch.equal(raw.cpu()[keep], clip[keep])
    # the same run composed by hand from the sampler's arguments
    torch.manual_seed(inp.seed); torch.cuda.manual_seed(inp.seed)
    pipe.dit.set_condition(inp.dit_context, pipe.detok.semantic_condition(tok))
    noise = torch.randn(1, 3, d.in_channels, 8, 12, device=cuda, dtype=torch.float32)
    z = pipe.sampler.run(pipe.dit.step, noise, start=start, known=z0, known_mask=mlat.to(cuda), known_noise=True)
    assert torch.equal(z.to(BF).float(), L[0])
    # a latent-cell mask is used as it is; the clean pin is another trajectory with the same kept cells
    L3, L4 = [], []
    pipe.edit_video(inp, strength=0.5, tokens=tok, frames=clip, keep_mask=mlat.bool(), latents_out=L3)
    pipe.edit_video(inp, strength=0.5, tokens=tok, frames=clip, keep_mask=keep, known_noise=False, latents_out=L4)
    assert torch.equal(L3[0], L[0]) and not torch.equal(L4[0], L[0]) and torch.equal(L4[0].cpu()[:, cells], z0.cpu()[:, cells])
    # tokens from the prompt when none are given
    pipe.edit_video(inp, strength=0.5, frames=clip)
    assert pipe.last_edit["tokens_source"] == "prompt" and pipe.timings.get("llm", 0.0) > 0.0


def test_edit_video_refusals(cuda, tiny_edit):
    cfg, st, pipe, inp, clip, tok, keep = tiny_edit
    z0 = torch.zeros(1, 3, 16, 8, 12)
    with pytest.raises(ValueError, match="exactly one"):
        pipe.edit_video(inp, tokens=tok)
    with pytest.raises(ValueError, match="exactly one"):
        pipe.edit_video(inp, tokens=tok, frames=clip, clip_latent=z0)
    for bad in (torch.cat([clip, clip[:1]]), clip[:5], clip[:, :-8], clip.float()):
        with pytest.raises(ValueError, match=r"uint8 \[9, 64, 96, 3\]"):
            pipe.edit_video(inp, tokens=tok, frames=bad)
    with pytest.raises(ValueError, match=r"\[1, 3, 16, 8, 12\]"):
        pipe.edit_video(inp, tokens=tok, clip_latent=z0[:, :2])
    with pytest.raises(ValueError, match="clip_tokens"):
        pipe.edit_video(inp, tokens=tok, clip_tokens="from_frames", frames=clip)
    with pytest.raises(ValueError, match="from_frames"):
        pipe.edit_video(inp, clip_tokens="frames", frames=clip)
    with pytest.raises(ValueError, match="theia="):
        pipe.edit_video(inp, clip_tokens="from_frames", frames=clip)          # this pipeline has no Theia extractor
    for s in (0.0, 1.5):
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            pipe.edit_video(inp, tokens=tok, frames=clip, strength=s)
    with pytest.raises(ValueError, match="smallest strength"):
        pipe.edit_video(inp, tokens=tok, frames=clip, strength=0.1)           # 4 steps: 0.125 is the smallest
    with pytest.raises(ValueError, match="nothing is left"):
        pipe.edit_video(inp, tokens=tok, frames=clip, keep_mask=torch.ones_like(keep))
    with pytest.raises(ValueError, match="keep_mask must be bool"):
        pipe.edit_video(inp, tokens=tok, frames=clip, keep_mask=keep[:, :-8])
    with pytest.raises(ValueError, match="keep_mask must be bool"):
        pipe.edit_video(inp, tokens=tok, frames=clip, keep_mask=keep.to(torch.uint8))


def test_edit_video_tokens_from_frames(cuda, theia_workdir):
    """edit_video(clip_tokens="from_frames") = edit_video(tokens=tokenize_frames(clip)), timed as "theia"."""
    from landiff_amd.pipeline import LanDiffPipeline, synthetic_inputs
    from landiff_amd.theia import build_theia
    from landiff_amd.tokenizer_encoder import TokenizerEncoder
    work, cfg, states, enc, venc, theia = theia_workdir
    d = cfg.dit
    ext = build_theia(theia, cfg.tok, cuda, encoder=TokenizerEncoder({**enc}, cfg.tok, cuda))
    pipe = LanDiffPipeline(cfg, dict(states, vae={**states["vae"], **venc}), cuda, theia=ext)
    inp = synthetic_inputs(cfg, cuda, n_text=6, seed=12)
    g = torch.Generator().manual_seed(9)
    clip = torch.randint(0, 256, (4 * d.latent_frames - 3, 8 * d.latent_h, 8 * d.latent_w, 3), generator=g, dtype=torch.uint8)
    out = pipe.edit_video(inp, frames=clip, clip_tokens="from_frames", strength=0.5)
    assert pipe.timings.get("theia", 0.0) > 0.0 and pipe.last_edit["tokens_source"] == "from_frames"
    assert pipe.last_edit["start_step"] == len(pipe.sampler.plan) - 1
    tokens = pipe.tokenize_frames(clip)
    assert tokens.shape == (cfg.tok.num_latent_tokens,)
    assert torch.equal(out, pipe.edit_video(inp, frames=clip, tokens=tokens, strength=0.5))


# ---- 7. with the opt-in DiT modes -----------------------------------------------------------------------
def test_edit_video_with_dit_cache_and_guidance(cuda):
    """A run that begins at start > 0: the reports have steps_run rows whose index begins at start; the first executed step has
    nothing to reuse, so it is computed (cache) / full (guidance) whatever the plan says for it."""
    from landiff_amd.config import PipelineConfig
    from landiff_amd.dit_cache import StepCacheConfig
    from landiff_amd.dit_guidance import GuidanceSkipConfig
    from landiff_amd.pipeline import LanDiffPipeline, synthetic_inputs
    from landiff_amd.schedule import build_plan
    from landiff_amd.weights import init_pipeline_state
    cfg = PipelineConfig.tiny(num_steps=6).check()
    st = init_pipeline_state(cfg, seed=1234)
    d = cfg.dit
    inp = synthetic_inputs(cfg, cuda, n_text=6, seed=43)
    g = torch.Generator().manual_seed(4)
    z0 = torch.randn(1, d.latent_frames, d.in_channels, d.latent_h, d.latent_w, generator=g)
    tok = torch.randint(0, cfg.tok.codebook_size, (cfg.tok.num_latent_tokens,), generator=g).to(cuda)
    mask = torch.zeros(d.latent_frames, d.latent_h, d.latent_w, dtype=torch.bool)
    mask[:, :, d.latent_w // 2:] = True
    ts = [sp.timestep for sp in build_plan(cfg.sampler)]
    pipe = LanDiffPipeline(cfg, st, cuda, dit_cache=StepCacheConfig(0.0, plan=(True, False, False, False, False, True)))
    out = pipe.edit_video(inp, clip_latent=z0, tokens=tok, strength=0.5, keep_mask=mask)
    rep = pipe.dit_cache_report()
    assert pipe.last_edit["start_step"] == 3 and len(pipe.dit_cache_reports) == 1
    assert [r["index"] for r in rep] == [3, 4, 5] and [r["timestep"] for r in rep] == ts[3:]
    assert [r["computed"] for r in rep] == [True, False, True] and out.dtype == torch.uint8
    pipe = LanDiffPipeline(cfg, st, cuda, dit_guidance=GuidanceSkipConfig(plan=("full", "reuse", "reuse", "reuse", "reuse", "cond")))
    out = pipe.edit_video(inp, clip_latent=z0, tokens=tok, strength=0.5, keep_mask=mask)
    rep = pipe.dit_guidance_report()
    assert [r["index"] for r in rep] == [3, 4, 5] and [r["timestep"] for r in rep] == ts[3:]
    assert [r["mode"] for r in rep] == ["full", "reuse", "cond"] and rep[1]["delta_from"] == 3 and out.dtype == torch.uint8


# ---- 8. the command line --------------------------------------------------------------------------------
def test_infer_video_edit_flag_config0(cuda, tmp_path, monkeypatch):
    """`landiff.infer_video --edit_video` on the synthetic checkpoint tree of the --extend_video test writes exactly what
    LanDiffPipeline.edit_video returns for the same clip, mask, prompt and seed, and <name>_edit.json."""
    import warnings
    import landiff.infer_video as iv
    from facade_helpers import build_config0_workdir
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
    g = torch.Generator().manual_seed(9)
    F, Hp, Wp = 4 * d.latent_frames - 3, 8 * d.latent_h, 8 * d.latent_w
    clip = torch.randint(0, 256, (F, Hp, Wp, 3), generator=g, dtype=torch.uint8)
    keep = torch.zeros(F, Hp, Wp, dtype=torch.bool)
    keep[:, :, Wp // 2:] = True
    np.save("clip.npy", clip.numpy())
    np.save("mask.npy", keep.numpy().astype(np.uint8))
    prompt, seed = "a cat runs on the beach", 11
    args = iv.parse_args(["--prompt", prompt, "--seed", str(seed), "--save_file_name", "results/ed", "--edit_video", "clip.npy",
                          "--edit_strength", "0.5", "--edit_mask", "mask.npy"])
    assert args.edit_tokens == "prompt"
    captured = {}
    monkeypatch.setattr(iv, "save_video_tensor", lambda v, p, fps=8: captured.update(video=v, path=p))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = iv.edit_diffusion(args)
    n = 1 + 8 * ((d.latent_frames - 1) // 2)          # (config0's 8 latent frames: the decoder leaves the last one, as in generation)
    assert out.shape == (n,) + clip.shape[1:] and torch.equal(captured["video"], out) and captured["path"] == "results/ed.mp4"
    assert torch.equal(out[keep[:n]], clip[:n][keep[:n]])
    st = dict(states, vae={**states["vae"], **enc})
    pipe = LanDiffPipeline(cfg, st, cuda)
    text = encode_flan_t5([prompt], cuda, max_length=cfg.llm.max_cond_tokens, model_path=cfg.llm.text_encoder_path)[0]
    ctx = encode_t5_v11([prompt], os.path.join(work, "ckpts", "LanDiff", "CogVideoX-2b-sat", "t5-v1_1-xxl"), d.text_len, cuda)
    inp = PromptInputs(text, ctx, seed=seed, cfg=7.5, motion_score=0.1)
    ref = pipe.edit_video(inp, frames=clip, strength=0.5, keep_mask=keep)
    assert torch.equal(out, ref.cpu())
    got = json.load(open("results/ed_edit.json"))
    assert got == pipe.last_edit and got["tokens_source"] == "prompt" and got["start_step"] == len(pipe.sampler.plan) - 1
    assert got["kept_cells"] == d.latent_frames * d.latent_h * (d.latent_w // 2)
