"""Host side of the Theia extractor (landiff_amd/theia.py): checkpoint key map and dimensions, path resolution, the cached
position-table interpolation against transformers' own, both branches of the output_shape rule, the new CLI flags."""
import os

import pytest
import torch
import torch.nn.functional as F

from landiff_amd.theia import (crop_pad, interpolate_pos_table, load_theia_state, resolve_theia_path, select_frames, theia_dims,
                               theia_keys)
from theia_helpers import hf_vit, theia_layout, write_theia


def test_loader_maps_the_theia_layout(tmp_path):
    m = hf_vit(width=128, heads=2, layers=3, seed=1)
    path = write_theia(str(tmp_path / "model.safetensors"), m)
    st = load_theia_state(path)
    assert sorted(st) == sorted(theia_keys(3))                       # translator.* / pooler.* ignored
    assert theia_dims(st) == dict(width=128, heads=2, layers=3, mlp=512, pos_side=14, variant=None)
    sd5 = m.state_dict()
    assert torch.equal(st["encoder.layer.2.attention.attention.key.weight"], sd5["layers.2.attention.k_proj.weight"])
    assert torch.equal(st["encoder.layer.0.attention.output.dense.bias"], sd5["layers.0.attention.o_proj.bias"])
    assert torch.equal(st["encoder.layer.1.intermediate.dense.weight"], sd5["layers.1.mlp.fc1.weight"])
    assert torch.equal(st["encoder.layer.1.output.dense.weight"], sd5["layers.1.mlp.fc2.weight"])
    assert torch.equal(st["embeddings.position_embeddings"], sd5["embeddings.position_embeddings"])
    # a directory holding model.safetensors (an HF snapshot) and $LANDIFF_THEIA_CKPT resolve to the same file
    assert resolve_theia_path(str(tmp_path)) == path


def test_loader_refuses_missing_keys_and_bad_shapes(tmp_path):
    from safetensors.torch import save_file
    sd = theia_layout(hf_vit(width=128, heads=2, layers=2, seed=2))
    bad = dict(sd)
    del bad["backbone.model.encoder.layer.1.layernorm_after.bias"]
    save_file(bad, str(tmp_path / "a.safetensors"))
    with pytest.raises(KeyError, match="layernorm_after.bias"):
        load_theia_state(str(tmp_path / "a.safetensors"))
    save_file({k: v for k, v in sd.items() if k.startswith("translator.")}, str(tmp_path / "b.safetensors"))
    with pytest.raises(KeyError, match="encoder.layer"):
        load_theia_state(str(tmp_path / "b.safetensors"))
    # a DeiT-base width with a layer count DeiT-base does not have
    sd3 = theia_layout(hf_vit(width=768, heads=12, layers=1, seed=3))
    save_file(sd3, str(tmp_path / "c.safetensors"))
    with pytest.raises(ValueError, match="12 layers"):
        load_theia_state(str(tmp_path / "c.safetensors"))


def test_path_resolution_is_lookup_only(tmp_path, monkeypatch):
    monkeypatch.delenv("LANDIFF_THEIA_CKPT", raising=False)
    monkeypatch.setenv("HF_HUB_CACHE", str(tmp_path / "hub"))
    with pytest.raises(FileNotFoundError, match="not downloaded"):
        resolve_theia_path(None)
    snap = tmp_path / "hub" / "models--theaiinstitute--theia-base-patch16-224-cddsv" / "snapshots" / "abc"
    snap.mkdir(parents=True)
    (snap / "model.safetensors").write_bytes(b"x")
    assert resolve_theia_path(None) == str(snap / "model.safetensors")
    other = tmp_path / "env.safetensors"
    other.write_bytes(b"y")
    monkeypatch.setenv("LANDIFF_THEIA_CKPT", str(other))
    assert resolve_theia_path(None) == str(other)
    with pytest.raises(FileNotFoundError):
        resolve_theia_path(str(tmp_path / "missing"))


@pytest.mark.parametrize("S", [224, 128, 720, 512, 96])
def test_position_interpolation_matches_transformers(S):
    from transformers import ViTConfig
    from transformers.models.vit.modeling_vit import ViTEmbeddings
    emb = ViTEmbeddings(ViTConfig(hidden_size=64, image_size=224, patch_size=16))
    with torch.no_grad():
        emb.position_embeddings.copy_(torch.randn(emb.position_embeddings.shape, generator=torch.Generator().manual_seed(S)))
    g = S // 16
    want = emb.interpolate_pos_encoding(torch.zeros(1, 1 + g * g, 64), S, S)
    got = interpolate_pos_table(emb.position_embeddings.detach(), g)
    assert torch.equal(got, want.detach())
    if S == 224:                                                      # the shortcut: the trained table itself
        assert got.data_ptr() == emb.position_embeddings.data_ptr()


def _reference_rule(f, output_shape):
    """theia_extractor.py:119-139, restated line by line."""
    if output_shape[0] < f.shape[-1] and output_shape[1] < f.shape[-2]:
        return f[..., : output_shape[0], : output_shape[1]]
    pad = (output_shape[1] - f.shape[-2], output_shape[0] - f.shape[-1])
    pad = [max(i, 0) for i in pad]
    f = F.pad(f, (0, pad[0], 0, pad[1]))
    return f[..., : output_shape[0], : output_shape[1]]


@pytest.mark.parametrize("s", [45, 46, 60, 8, 32, 30, 31])
def test_crop_pad_rule_both_branches(s):
    f = torch.randn(2, 5, s, s)
    for shape in [(30, 45), (32, 32)]:
        got = crop_pad(f, shape)
        assert torch.equal(got, _reference_rule(f, shape)) and got.shape == (2, 5, *shape)
        # on a square grid both branches keep position (i, j) when i, j < s and zero the rest (what ld_vit_tail does)
        want = torch.zeros(2, 5, *shape)
        h, w = min(s, shape[0]), min(s, shape[1])
        want[..., :h, :w] = f[..., :h, :w]
        assert torch.equal(got, want)
    if s == 45:       # 480 x 720 padded to 720 x 720: the crop keeps the first 30 grid rows = tokens 1..1350 of a frame
        assert torch.equal(crop_pad(f, (30, 45)).flatten(2), f.flatten(2)[..., :1350])


def test_select_frames_is_the_facade_linspace():
    fr = torch.arange(45).reshape(45, 1, 1, 1)
    assert select_frames(fr, 13).flatten().tolist() == torch.linspace(0, 44, 13).long().tolist()


def test_cli_theia_flags(monkeypatch):
    import numpy as np
    import landiff.infer_video as iv
    a = iv.parse_args(["--prompt", "p"])
    assert a.theia_ckpt is None and a.first_frame is None
    a = iv.parse_args(["--prompt", "p", "--extend_video", "c.npy", "--theia_ckpt", "/x/theia", "--first_frame", "img.png"])
    assert a.theia_ckpt == "/x/theia" and a.first_frame == "img.png" and a.extend_tokens is None


def test_cli_first_frame_image_loading(tmp_path):
    import numpy as np
    import landiff.infer_video as iv
    img = np.random.default_rng(0).integers(0, 256, (24, 40, 3), dtype=np.uint8)
    np.save(tmp_path / "i.npy", img)
    assert torch.equal(iv.load_image(str(tmp_path / "i.npy")), torch.from_numpy(img))
    np.save(tmp_path / "f.npy", img.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        iv.load_image(str(tmp_path / "f.npy"))
