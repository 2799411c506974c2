"""Theia feature extractor (pixels -> semantic feature maps -> semantic tokens), the first stage of VideoVQWrap.forward(images).

Mirrors TheiaExtractor(micro_batch_size=1, interpolate=True, output_shape=(30, 45), bfp16=True) of
landiff/tokenizer/tokenizer_cfg.py:18-26 with theaiinstitute/theia-base-patch16-224-cddsv, whose backbone is
facebook/deit-base-patch16-224 (theia_model.py: TheiaModel.backbone = DeiT, DeiT.model = a Hugging Face ViTModel):
  uint8 [T, 3, S, S], not resized (theia_extractor.py:88-90) -> DeiT.yax_processor (x - 127.5) / 127.5 (theia_model.py:446-451)
  -> ViTModel(interpolate_pos_encoding=True) under bf16 autocast: 16x16/16 patch Conv2d, CLS, the 14x14 position table resized
  bicubically to (S/16, S/16), 12 pre-LN layers (eps 1e-12, scale 1/8, exact-erf GELU), final LayerNorm
  -> handle_feature_output drops CLS -> [T, C, S/16, S/16] -> output_shape crop / zero pad (theia_extractor.py:119-139).
All frames go through one launch chain (B = T in the attention); the reference loops over micro-batches of one frame.

Kernels (ld_theia.hip + the shared blocks): ld_vit_patch_rows (uint8 -> bf16 im2col rows, the grey-127 square padding made on
the fly for unpadded [T, H, W, 3] frames) -> ld_gemm_bf16 + bias (the Conv2d) -> ld_vit_embed (CLS + position table into the
fp32 residual stream) -> per layer ld_layernorm, ld_gemm_bf16 (q|k|v, bias), ld_qkv_split mode 2, ld_attn_fwd_bf16,
ld_gemm_bf16 (+ residual), ld_layernorm, ld_gemm_bf16 (GELU-erf), ld_gemm_bf16 (+ residual) -> ld_vit_tail (final LayerNorm,
CLS dropped, crop / pad, fp32 [T, C, gh, gw] and / or the TiTok encoder's bf16 channels-last input rows).
"""
from __future__ import annotations

import glob
import os

import torch
import torch.nn.functional as F

from . import ops

BF = torch.bfloat16
PATCH = 16
LN_EPS = 1e-12
OUTPUT_SHAPE = (30, 45)                                   # TheiaExtractor(output_shape=...) of tokenizer_cfg.py:18-26
THEIA_ENV = "LANDIFF_THEIA_CKPT"
THEIA_REPO = "theaiinstitute/theia-base-patch16-224-cddsv"
PREFIX = "backbone.model."                                # TheiaModel.backbone (DeiT) .model (ViTModel)
# the DeiT backbones Theia is distilled onto: width -> (name, heads); all 12 layers, MLP 4x, head dim 64
DEIT_VARIANTS = {192: ("deit-tiny", 3), 384: ("deit-small", 6), 768: ("deit-base", 12)}


def theia_keys(layers: int) -> list[str]:
    """The checkpoint keys the extractor reads (transformers 4.x ViTModel names, below PREFIX)."""
    keys = ["embeddings.cls_token", "embeddings.position_embeddings", "embeddings.patch_embeddings.projection.weight",
            "embeddings.patch_embeddings.projection.bias", "layernorm.weight", "layernorm.bias"]
    for i in range(layers):
        p = f"encoder.layer.{i}."
        for m in ("attention.attention.query", "attention.attention.key", "attention.attention.value", "attention.output.dense",
                  "intermediate.dense", "output.dense", "layernorm_before", "layernorm_after"):
            keys += [p + m + ".weight", p + m + ".bias"]
    return keys


def theia_dims(state: dict) -> dict:
    """Dimensions from the tensor shapes: width, heads (= width / 64), layers, mlp, the side of the trained position grid."""
    C = state["embeddings.cls_token"].shape[-1]
    layers = 1 + max(int(k.split(".")[2]) for k in state if k.startswith("encoder.layer."))
    mlp = state["encoder.layer.0.intermediate.dense.weight"].shape[0]
    n0 = state["embeddings.position_embeddings"].shape[1] - 1
    side = round(n0 ** 0.5)
    pw = tuple(state["embeddings.patch_embeddings.projection.weight"].shape)
    if C % 64:
        raise ValueError(f"Theia checkpoint: width {C} is not a multiple of the head dim 64")
    if pw != (C, 3, PATCH, PATCH):
        raise ValueError(f"Theia checkpoint: patch embedding {pw}, expected ({C}, 3, {PATCH}, {PATCH})")
    if side * side != n0:
        raise ValueError(f"Theia checkpoint: {n0} position embeddings do not form a square grid")
    if mlp != 4 * C:
        raise ValueError(f"Theia checkpoint: MLP width {mlp}, expected 4 x {C}")
    variant = DEIT_VARIANTS.get(C)
    if variant is not None and layers != 12:
        raise ValueError(f"Theia checkpoint: {variant[0]} has 12 layers, the file holds {layers}")
    return dict(width=C, heads=C // 64, layers=layers, mlp=mlp, pos_side=side, variant=variant[0] if variant else None)


def resolve_theia_path(path: str | None = None) -> str:
    """The Theia model.safetensors: `path` (a file, or a directory holding one, e.g. an HF snapshot), else $LANDIFF_THEIA_CKPT,
    else a snapshot of THEIA_REPO already in the local Hugging Face cache.  Lookup only: nothing is downloaded."""
    def pick(p):
        f = os.path.join(p, "model.safetensors") if os.path.isdir(p) else p
        if not os.path.isfile(f):
            raise FileNotFoundError(f"Theia checkpoint {p!r}: no model.safetensors there")
        return f
    if path:
        return pick(path)
    if os.environ.get(THEIA_ENV):
        return pick(os.environ[THEIA_ENV])
    hub = os.environ.get("HF_HUB_CACHE") or os.path.join(
        os.environ.get("HF_HOME") or os.path.join(os.path.expanduser("~"), ".cache", "huggingface"), "hub")
    snaps = sorted(glob.glob(os.path.join(hub, "models--" + THEIA_REPO.replace("/", "--"), "snapshots", "*", "model.safetensors")))
    if snaps:
        return snaps[-1]
    raise FileNotFoundError(f"no Theia checkpoint: give its path, set ${THEIA_ENV}, or place a snapshot of {THEIA_REPO} in the "
                            f"Hugging Face cache ({hub}); it is not downloaded")


def load_theia_state(path: str | None = None) -> dict:
    """Theia model.safetensors (or the directory holding it) -> the backbone's tensors under the transformers 4.x ViTModel names
    with PREFIX stripped (theia_keys).  translator.*, pooler.* and every other key are ignored; a missing key raises."""
    from safetensors.torch import load_file
    sd = load_file(resolve_theia_path(path))
    state = {k[len(PREFIX):]: v for k, v in sd.items() if k.startswith(PREFIX) and not k.startswith(PREFIX + "pooler.")}
    if not any(k.startswith("encoder.layer.") for k in state):
        raise KeyError(f"Theia checkpoint: no {PREFIX}encoder.layer.* keys (is this a Theia / DeiT file?)")
    layers = 1 + max(int(k.split(".")[2]) for k in state if k.startswith("encoder.layer."))
    missing = [PREFIX + k for k in theia_keys(layers) if k not in state]
    if missing:
        raise KeyError(f"Theia checkpoint: missing keys {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    state = {k: state[k] for k in theia_keys(layers)}
    theia_dims(state)
    return state


def interpolate_pos_table(pos: torch.Tensor, grid: int) -> torch.Tensor:
    """ViTEmbeddings.interpolate_pos_encoding for a square S x S input (grid = S // 16): pos [1, 1 + n0, C] -> [1, 1 + grid^2, C],
    the trained table returned as is when grid^2 == n0, else its patch part resized bicubically (align_corners=False)."""
    n0, C = pos.shape[1] - 1, pos.shape[-1]
    if grid * grid == n0:
        return pos
    side = int(n0 ** 0.5)
    pp = pos[:, 1:].reshape(1, side, side, C).permute(0, 3, 1, 2)
    pp = F.interpolate(pp, size=(grid, grid), mode="bicubic", align_corners=False)
    return torch.cat((pos[:, :1], pp.permute(0, 2, 3, 1).view(1, -1, C)), dim=1)


def crop_pad(features: torch.Tensor, output_shape) -> torch.Tensor:
    """TheiaExtractor's output_shape rule (theia_extractor.py:119-139) on [.., C, h, w]: crop [..., :o0, :o1] when o0 < w and
    o1 < h (the reference compares o0 with the width and o1 with the height), else zero pad the width by o1 - h and the height by
    o0 - w (each at least 0) and crop the same way."""
    o0, o1 = output_shape
    h, w = features.shape[-2:]
    if o0 < w and o1 < h:
        return features[..., :o0, :o1]
    pad = [max(o1 - h, 0), max(o0 - w, 0)]
    return F.pad(features, (0, pad[0], 0, pad[1]))[..., :o0, :o1]


def select_frames(frames: torch.Tensor, T: int) -> torch.Tensor:
    """T equally spaced frames of a clip (torch.linspace(0, F - 1, T).long(), as CogWrapper._semantic_from_video picks them)."""
    idx = torch.linspace(0, frames.shape[0] - 1, T).long().to(frames.device)
    return frames[idx]


class TheiaExtractor:
    """The Theia backbone on the device.  Called as the `feature_extractor` of CogModelInferWrapper: uint8 [T, 3, S, S] ->
    features fp32 [T, C, gh, gw] with (gh, gw) = output_shape (the tokenizer grid).  tokenize_video / tokenize_image go on to
    semantic token ids through `encoder` (a TokenizerEncoder), feeding it channels-last rows without a [T, C, gh, gw] round trip."""

    def __init__(self, state: dict, device, output_shape=OUTPUT_SHAPE, encoder=None):
        self.dims = theia_dims(state)
        self.dev, self.output_shape, self.encoder = torch.device(device), tuple(output_shape), encoder
        g = lambda k: state[k].to(self.dev, BF).contiguous()
        f32 = lambda k: state[k].to(self.dev, torch.float32).contiguous()
        C = self.dims["width"]
        self.patch_w = g("embeddings.patch_embeddings.projection.weight").reshape(C, 3 * PATCH * PATCH)
        self.patch_b = g("embeddings.patch_embeddings.projection.bias")
        self.cls = f32("embeddings.cls_token").reshape(C)
        self.pos = f32("embeddings.position_embeddings")
        self.ln_f = (f32("layernorm.weight"), f32("layernorm.bias"))
        self.blocks = []
        for i in range(self.dims["layers"]):
            p = f"encoder.layer.{i}."
            a = p + "attention.attention."
            self.blocks.append(dict(
                ln1=(g(p + "layernorm_before.weight"), g(p + "layernorm_before.bias")),
                ln2=(g(p + "layernorm_after.weight"), g(p + "layernorm_after.bias")),
                wqkv=torch.cat([g(a + "query.weight"), g(a + "key.weight"), g(a + "value.weight")], 0).contiguous(),
                bqkv=torch.cat([g(a + "query.bias"), g(a + "key.bias"), g(a + "value.bias")], 0).contiguous(),
                wo=(g(p + "attention.output.dense.weight"), g(p + "attention.output.dense.bias")),
                fc=(g(p + "intermediate.dense.weight"), g(p + "intermediate.dense.bias")),
                proj=(g(p + "output.dense.weight"), g(p + "output.dense.bias"))))
        self._pos_cache = {}

    def pos_table(self, grid: int) -> torch.Tensor:
        """fp32 [1 + grid^2, C]: the interpolated position table with the CLS token added to row 0 (fp32, once per grid size)."""
        t = self._pos_cache.get(grid)
        if t is None:
            t = interpolate_pos_table(self.pos, grid)[0].clone()
            t[0] = self.cls + t[0]
            t = self._pos_cache[grid] = t.contiguous()
        return t

    @torch.no_grad()
    def backbone(self, frames: torch.Tensor, nhwc: bool):
        """uint8 frames (on the device) [T, 3, S, S], or [T, H, W, 3] with nhwc (square padding with 127 made by the kernel) ->
        (the fp32 residual stream after the last layer [T * (1 + s^2), C], s = S // 16)."""
        assert frames.dtype == torch.uint8 and frames.dim() == 4, "Theia takes uint8 frames"
        frames = frames.to(self.dev).contiguous()
        T = frames.shape[0]
        S = max(frames.shape[1], frames.shape[2]) if nhwc else frames.shape[-1]
        if not nhwc:
            assert frames.shape[1] == 3 and frames.shape[2] == frames.shape[3], f"expected [T, 3, S, S], got {tuple(frames.shape)}"
        s = S // PATCH
        P, N = s * s, s * s + 1
        C, H = self.dims["width"], self.dims["heads"]
        Npad = -(-N // 128) * 128
        rows = torch.empty(T * P, 3 * PATCH * PATCH, device=self.dev, dtype=BF)
        ops.vit_patch_rows(frames, rows, S, nhwc)
        patch = ops.gemm(rows, self.patch_w, bias=self.patch_b)                                  # Conv2d 16x16/16, bf16
        x = torch.empty(T * N, C, device=self.dev, dtype=torch.float32)                          # fp32 residual stream
        ops.vit_embed(patch, self.pos_table(s), x, T, P)
        del rows, patch
        ln = torch.empty(T * N, C, device=self.dev, dtype=BF)
        qkv = torch.empty(T * N, 3 * C, device=self.dev, dtype=BF)
        q = torch.empty(T, H, Npad, 64, device=self.dev, dtype=BF)                               # (ld_qkv_split writes every row)
        k = torch.empty_like(q)
        vt = torch.empty(T, H, 64, Npad, device=self.dev, dtype=BF)
        att = torch.empty(T, N, C, device=self.dev, dtype=BF)
        hid = torch.empty(T * N, self.dims["mlp"], device=self.dev, dtype=BF)
        for blk in self.blocks:
            ops.layernorm(x, *blk["ln1"], ln, LN_EPS)
            ops.gemm(ln, blk["wqkv"], out=qkv, bias=blk["bqkv"])
            ops.qkv_split(qkv, q, k, vt, T, N, H, Npad)
            ops.attn_fwd(q, k, vt, att, N, N, 64 ** -0.5)                                        # all T frames in one launch
            ops.gemm(att.view(T * N, C), blk["wo"][0], out=x, bias=blk["wo"][1], resid=x, out_f32=True)
            ops.layernorm(x, *blk["ln2"], ln, LN_EPS)
            ops.gemm(ln, blk["fc"][0], out=hid, bias=blk["fc"][1], act="gelu_erf")
            ops.gemm(hid, blk["proj"][0], out=x, bias=blk["proj"][1], resid=x, out_f32=True)
        return x, s

    @torch.no_grad()
    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        """uint8 [T, 3, S, S] -> fp32 [T, C, gh, gw] (TheiaExtractor.forward with interpolate=True, output_shape)."""
        x, s = self.backbone(images, nhwc=False)
        gh, gw = self.output_shape
        T = images.shape[0]
        feat = torch.empty(T, self.dims["width"], gh, gw, device=self.dev, dtype=torch.float32)
        ops.vit_tail(x, *self.ln_f, LN_EPS, T, s, gh, gw, feat=feat)
        return feat

    def _encoder(self):
        if self.encoder is None:
            raise ValueError("TheiaExtractor.tokenize_*: no tokenizer encoder attached (TheiaExtractor(..., encoder=TokenizerEncoder))")
        enc = self.encoder
        assert (enc.tc.grid_h, enc.tc.grid_w) == self.output_shape and enc.tc.out_channels == self.dims["width"], \
            "the tokenizer's grid / input channels must be the extractor's output_shape / width"
        return enc

    @torch.no_grad()
    def encoder_rows(self, frames: torch.Tensor, rows: torch.Tensor | None = None) -> torch.Tensor:
        """uint8 frames [T, H, W, 3] (unpadded; the grey-127 square padding is made on the fly) -> the TiTok encoder's input rows
        bf16 [T * gh * gw, C] = feature_norm_cl(self(square frames)), written into `rows` when given."""
        enc = self._encoder()
        x, s = self.backbone(frames, nhwc=True)
        gh, gw = self.output_shape
        T = frames.shape[0]
        if rows is None:
            rows = torch.empty(T * gh * gw, self.dims["width"], device=self.dev, dtype=BF)
        ops.vit_tail(x, *self.ln_f, LN_EPS, T, s, gh, gw, cl=rows, mean=enc.mean, std=enc.std)
        return rows

    @torch.no_grad()
    def tokenize_video(self, frames: torch.Tensor) -> torch.Tensor:
        """uint8 frames [T, H, W, 3], T = the tokenizer's temporal size (already selected) -> semantic token ids int64 [L]."""
        enc = self._encoder()
        assert frames.shape[0] == enc.tc.temporal, f"tokenize_video takes {enc.tc.temporal} frames, got {frames.shape[0]}"
        return enc.encode_rows_to_index(self.encoder_rows(frames))

    @torch.no_grad()
    def tokenize_image(self, img: torch.Tensor) -> torch.Tensor:
        """uint8 image [H, W, 3] -> token ids int64 [L] of a clip whose frame 0 is `img` and whose other feature frames are 0.
        Theia runs on the one frame: the encoder's I-frame latent tokens attend to frame 0 only (VideoEncoderMask), so the first
        iframe_tokens ids are those of any clip that starts with `img` -- use_gt_first_frame's CodeTask.first_frame_tokens."""
        enc = self._encoder()
        tc = enc.tc
        P, C = tc.grid_h * tc.grid_w, self.dims["width"]
        rows = torch.empty(tc.temporal * P, C, device=self.dev, dtype=BF)
        self.encoder_rows(img.reshape(1, *img.shape), rows[:P])
        if tc.temporal > 1:
            zero = torch.zeros(tc.temporal - 1, C, tc.grid_h, tc.grid_w, device=self.dev, dtype=torch.float32)
            ops.feature_norm_cl(zero, enc.mean, enc.std, rows[P:], tc.temporal - 1, C, P)
        return enc.encode_rows_to_index(rows)


def build_theia(path: str | None, tok_cfg, device, encoder=None) -> TheiaExtractor:
    """TheiaExtractor from a checkpoint (resolve_theia_path) with the tokenizer's grid as output_shape."""
    return TheiaExtractor(load_theia_state(path), device, output_shape=(tok_cfg.grid_h, tok_cfg.grid_w), encoder=encoder)
