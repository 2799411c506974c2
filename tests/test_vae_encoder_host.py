"""CPU checks of the 3D-VAE encoder path: the plain-torch restatement (tests/vae_encoder_ref.py) against the reference's own
outputs (tests/golden/vae_encoder_fp32.npz, tools/gen_golden_vae_encoder.py), the encoder key map, the space-to-depth form of
DownSample3D's stride-2 conv, the encoder_config check and extend_video's clip window."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from landiff_amd.config import PipelineConfig, VAEConfig, check_vae_encoder_config
from landiff_amd.weights import init_state, vae_encoder_spec

G = os.path.join(os.path.dirname(__file__), "golden", "vae_encoder_fp32.npz")
rel = lambda a, b: ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


@pytest.fixture(scope="module")
def gold():
    return np.load(G)


def test_encoder_keys_match_the_reference(gold):
    assert sorted(n for n, _, _ in vae_encoder_spec(VAEConfig.tiny())) == list(gold["keys"])
    full = {n: s for n, s, _ in vae_encoder_spec(VAEConfig())}
    assert full["encoder.conv_in.conv.weight"] == (128, 3, 3, 3, 3) and full["encoder.conv_out.conv.weight"] == (32, 512, 3, 3, 3)
    assert full["encoder.down.0.downsample.conv.weight"] == (128, 128, 3, 3) and "encoder.down.3.downsample.conv.weight" not in full
    assert "encoder.down.0.block.2.conv2.conv.weight" in full and "encoder.down.0.block.3.conv2.conv.weight" not in full


@pytest.mark.parametrize("clip", ["odd", "even"])
def test_restatement_matches_the_reference(gold, clip):
    from vae_encoder_ref import encode_moments_ref
    cfg = VAEConfig.tiny()
    sd = init_state(vae_encoder_spec(cfg), seed=int(gold["weight_seed"]))
    x = torch.from_numpy(gold[f"{clip}_x"])
    assert torch.equal(x, torch.from_numpy(gold[f"{clip}_frames"]).float() / 127.5 - 1.0)
    mean, logvar = encode_moments_ref(sd, cfg, x)
    assert mean.shape == (1, 16, (x.shape[0] + 3) // 4, 4, 6)
    assert rel(mean, torch.from_numpy(gold[f"{clip}_mean"])) < 1e-5
    assert rel(logvar, torch.from_numpy(gold[f"{clip}_logvar"])) < 1e-5
    z = cfg.scale_factor * (mean + torch.exp(0.5 * logvar) * torch.from_numpy(gold[f"{clip}_eps"]))
    assert rel(z, torch.from_numpy(gold[f"{clip}_sample"])) < 1e-5


def test_space_to_depth_weights_equal_the_strided_conv():
    """ld_vae_enc_downsample's layout + s2d_conv_weight as a stride-1 3x3 conv == Conv2d(3, stride 2) after pad (0, 1, 0, 1)."""
    from landiff_amd.vae_encoder import s2d_conv_weight
    from vae_encoder_ref import space_to_depth
    g = torch.Generator().manual_seed(3)
    C, Co, H, W = 8, 5, 10, 14
    x = torch.randn(2, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Co, C, 3, 3, generator=g, dtype=torch.float64)
    want = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    s2d = space_to_depth(x.permute(0, 2, 3, 1))                               # [B, H/2+2, W/2+2, 4C]
    ws = s2d_conv_weight(w)                                                    # [Co, 1, 3, 3, 4C]
    got = F.conv2d(s2d.permute(0, 3, 1, 2), ws[:, 0].permute(0, 3, 1, 2))
    assert got.shape == want.shape == (2, Co, H // 2, W // 2)
    assert (got - want).abs().max().item() < 1e-12
    # the taps that do not exist: row 2A+p = 3 (A = 1, p = 1) and column 2B+q = 3 (B = 1, q = 1); channel block (2p+q) C;
    # A = 2 and B = 2 (the odd kernel size the conv takes)
    assert torch.count_nonzero(ws[:, 0, 2]) == 0 and torch.count_nonzero(ws[:, 0, :, 2]) == 0
    assert torch.count_nonzero(ws[:, 0, 1, :, 2 * C:]) == 0
    assert torch.count_nonzero(ws[:, 0, :, 1, C:2 * C]) == 0 and torch.count_nonzero(ws[:, 0, :, 1, 3 * C:]) == 0


def test_time_pool_branches():
    from vae_encoder_ref import time_pool
    x = torch.arange(5, dtype=torch.float32).reshape(5, 1, 1, 1)
    assert time_pool(x).flatten().tolist() == [0.0, 1.5, 3.5]                 # odd: frame 0, then pairs
    assert time_pool(x[:4]).flatten().tolist() == [0.5, 2.5]                  # even: pairs


def test_encoder_config_check():
    vae = VAEConfig()
    ref = {"target": "landiff.diffusion.vae_modules.cp_enc_dec.ContextParallelEncoder3D",
           "params": {"double_z": True, "z_channels": 16, "resolution": 256, "in_channels": 3, "out_ch": 3, "ch": 128,
                      "ch_mult": [1, 2, 2, 4], "attn_resolutions": [], "num_res_blocks": 3, "dropout": 0.0, "gather_norm": True}}
    check_vae_encoder_config(ref, vae)
    bad = {"target": ref["target"], "params": dict(ref["params"], num_res_blocks=2)}
    with pytest.raises(ValueError, match="num_res_blocks"):
        check_vae_encoder_config(bad, vae)


def test_continuation_window():
    from landiff_amd.pipeline import continuation_window
    cfg = PipelineConfig.tiny()
    d = cfg.dit
    n = 4 * d.latent_frames - 3
    H, W = 8 * d.latent_h, 8 * d.latent_w
    clip = torch.arange(n + 4, dtype=torch.uint8)[:, None, None, None].expand(n + 4, H, W, 3).contiguous()
    win = continuation_window(clip, cfg)
    assert win.shape[0] == n and int(win[0, 0, 0, 0]) == 4 and int(win[-1, 0, 0, 0]) == n + 3
    assert continuation_window(clip[:n], cfg).shape[0] == n
    with pytest.raises(ValueError, match="too short"):
        continuation_window(clip[:n - 1], cfg)
    with pytest.raises(ValueError, match="must be"):
        continuation_window(clip[:, :H - 8], cfg)
    with pytest.raises(ValueError, match="uint8"):
        continuation_window(clip.float(), cfg)


def test_load_clip(tmp_path):
    """--extend_video's reader: uint8 [F, H, W, 3] .npy as saved; anything else is refused."""
    from landiff.infer_video import load_clip
    clip = np.random.default_rng(0).integers(0, 256, (5, 16, 24, 3), dtype=np.uint8)
    np.save(tmp_path / "clip.npy", clip)
    assert np.array_equal(load_clip(str(tmp_path / "clip.npy")).numpy(), clip)
    np.save(tmp_path / "bad.npy", clip.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        load_clip(str(tmp_path / "bad.npy"))


@pytest.mark.parametrize("clip,slice_frames", [("odd", 2), ("odd", 3), ("even", 3)])
def test_sliced_restatement_matches_the_whole_clip_one(gold, clip, slice_frames):
    """The sliced mode of the restatement (activations in pieces of a few frames, each causal conv and downsample with its halo,
    GroupNorm statistics summed in float64 over the pieces) computes what the whole-clip restatement computes: it stands in for
    it where a whole activation would pass 2^31 elements."""
    from vae_encoder_ref import encode_moments_ref
    cfg = VAEConfig.tiny()
    sd = init_state(vae_encoder_spec(cfg), seed=int(gold["weight_seed"]))
    x = torch.from_numpy(gold[f"{clip}_x"])
    assert x.shape[0] > 2 * slice_frames                        # at least three pieces at level 0
    for dtype, tol in ((torch.float32, 1e-5), (torch.bfloat16, 2e-2)):
        mean, logvar = encode_moments_ref(sd, cfg, x, dtype=dtype)
        ms, ls = encode_moments_ref(sd, cfg, x, dtype=dtype, slice_frames=slice_frames)
        assert ms.shape == mean.shape and ls.shape == logvar.shape
        assert rel(ms, mean) < tol and rel(ls, logvar) < tol, (dtype, rel(ms, mean), rel(ls, logvar))


def test_max_clip_frames():
    """At 480 x 720 the encoder takes at most 94 frames: 95 need a 97 x 482 x 722 x 128 bf16 level-0 window (8.05 GiB), beyond
    the 8 GiB ld_conv_cl_bf16 addresses.  encode_moments refuses a longer clip before it allocates or launches anything."""
    from landiff_amd import _lib
    from landiff_amd.vae_encoder import VAEEncoder, encoder_convs, max_clip_frames
    cfg = VAEConfig()
    lib = _lib.load()
    assert max_clip_frames(cfg, 480, 720) == 94
    assert all(lib.ld_conv_route(*s) >= 0 for _, s in encoder_convs(cfg, 94, 480, 720))
    refused = [n for n, s in encoder_convs(cfg, 95, 480, 720) if lib.ld_conv_route(*s) < 0]
    assert refused == [f"down.0.block.{j}.conv{i}" for j in range(3) for i in (1, 2)]
    assert 97 * 482 * 722 * 128 * 2 >= 2 ** 33 > 96 * 482 * 722 * 128 * 2
    enc = VAEEncoder.__new__(VAEEncoder)                        # no weights needed: the check comes first
    enc.cfg, enc.dev, enc._max_frames, enc._padded = cfg, torch.device("cpu"), {}, {}
    clip = torch.zeros(1, 1, 1, 3, dtype=torch.uint8).expand(95, 480, 720, 3)
    with pytest.raises(ValueError, match="at most 94 frames"):
        enc.encode_moments(clip)
    assert enc._padded == {}
