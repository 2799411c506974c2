"""Theia test data made by this repo's own code: a seeded Hugging Face ViTModel (the DeiT backbone, pooler removed), its state in
the checkpoint layout real Theia files hold (transformers 4.x module names below `backbone.model.`, next to translator heads),
and the reference extractor's interpolate branch restated on top of the model as the oracle."""
import re

import torch

from landiff_amd.theia import crop_pad

# transformers >= 5 module names -> the 4.x names Theia checkpoints carry (TheiaModel.backbone = DeiT, DeiT.model = ViTModel)
_RENAMES = [
    (r"^layers\.(\d+)\.attention\.q_proj\.", r"encoder.layer.\1.attention.attention.query."),
    (r"^layers\.(\d+)\.attention\.k_proj\.", r"encoder.layer.\1.attention.attention.key."),
    (r"^layers\.(\d+)\.attention\.v_proj\.", r"encoder.layer.\1.attention.attention.value."),
    (r"^layers\.(\d+)\.attention\.o_proj\.", r"encoder.layer.\1.attention.output.dense."),
    (r"^layers\.(\d+)\.mlp\.fc1\.", r"encoder.layer.\1.intermediate.dense."),
    (r"^layers\.(\d+)\.mlp\.fc2\.", r"encoder.layer.\1.output.dense."),
    (r"^layers\.(\d+)\.(layernorm_before|layernorm_after)\.", r"encoder.layer.\1.\2."),
]


def hf_vit(width=768, heads=12, layers=12, seed=0, image_size=224):
    """A ViTModel (no pooler) with seeded random weights at the given shape: linear weights ~ N(0, 1/fan_in), LayerNorm
    weights around 1, small biases, CLS / position table ~ N(0, 0.2^2)."""
    from transformers import ViTConfig, ViTModel
    cfg = ViTConfig(hidden_size=width, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=4 * width,
                    image_size=image_size, patch_size=16, layer_norm_eps=1e-12, hidden_act="gelu", qkv_bias=True)
    m = ViTModel(cfg, add_pooling_layer=False).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "layernorm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif p.dim() >= 2 and "embeddings" not in name:
                p.copy_(torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)
            elif "projection" in name:
                p.copy_(torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)
            else:
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
    return m


def theia_layout(model) -> dict:
    """The model's state_dict under the Theia checkpoint keys, plus translator / pooler tensors the loader must ignore."""
    out = {}
    for k, v in model.state_dict().items():
        for pat, rep in _RENAMES:
            if re.match(pat, k):
                k = re.sub(pat, rep, k)
                break
        out["backbone.model." + k] = v.detach().clone().contiguous()
    C = model.config.hidden_size
    out["backbone.model.pooler.dense.weight"] = torch.zeros(C, C)
    out["translator.translators.google/vit-huge-patch14-224-in21k.0.weight"] = torch.ones(4, C)
    return out


def write_theia(path, model):
    from safetensors.torch import save_file
    save_file(theia_layout(model), path)
    return path


@torch.no_grad()
def oracle_features(model, images, output_shape, autocast: bool):
    """TheiaExtractor.forward, interpolate branch (no resize; yax_processor; ViTModel(interpolate_pos_encoding=True) under
    bf16 autocast when `autocast`; CLS dropped; [n, c, h, w]; output_shape crop / pad).  images uint8 [T, 3, S, S]."""
    x = (images.float() - 127.5) / 127.5
    with torch.autocast(device_type=images.device.type, dtype=torch.bfloat16, enabled=autocast):
        y = model(pixel_values=x, interpolate_pos_encoding=True).last_hidden_state
    y = y[:, 1:].float()
    s = int(y.shape[1] ** 0.5)
    y = y.reshape(y.shape[0], s, s, -1).permute(0, 3, 1, 2)
    return crop_pad(y, output_shape).contiguous()


def pad_square(frames_thwc):
    """uint8 [T, H, W, 3] -> [T, 3, S, S] padded right / bottom with 127 (pad_to_square)."""
    T, H, W, _ = frames_thwc.shape
    S = max(H, W)
    sq = torch.full((T, 3, S, S), 127, dtype=torch.uint8, device=frames_thwc.device)
    sq[:, :, :H, :W] = frames_thwc.permute(0, 3, 1, 2)
    return sq
