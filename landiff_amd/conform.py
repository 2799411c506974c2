"""The conform stage: input clips, images and keep-masks of any size and frame rate brought to the model's frame.

The reference resizes with torchvision (landiff/tokenizer/theia_extractor.py:88-90) and leaves the filter, the crop and the frame
selection of everything else to the user.  Here the step is defined exactly and runs on the device where the frames are consumed:

* the plan (conform_plan: which source frames, which crop box) is pure Python integer / rational arithmetic;
* the filter is PyTorch's antialias one (axis_table: float64 on the host, rounded to fp32 once) and the resampling is one
  ld_resize_u8 launch (fp32 accumulation, nothing rounded between the two passes, one clamp(round-half-even) at the end);
* a keep-mask follows the same geometry conservatively (ld_resize_mask_u8: kept only if its whole tap window is kept).

Nothing here is used unless a ConformConfig with fit != "exact" is given: extend_video / edit_video refuse what is not the model's
frame exactly as before.
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from functools import lru_cache

import numpy as np

FITS = ("exact", "cover", "stretch")
WINDOWS = ("last", "first")
FILTERS = {"bilinear": 0, "bicubic": 1}


@dataclass(frozen=True)
class ConformConfig:
    """fit: "exact" (no conform stage: the clip must already be the model's frame), "cover" (the largest centred box of the
    target's aspect ratio, or `crop`, resampled to the frame) or "stretch" (the whole frame resampled).  src_fps: the clip's frame
    rate (int, float, str such as "30000/1001", or Fraction); None takes frames one to one.  window: which end of the clip the
    frames come from; start_s: with window="first" and src_fps, where the window begins.  crop: (y0, x0, h, w) instead of the
    centred box.  filter: "bilinear" (triangle) or "bicubic" (Keys, a = -0.5), both antialiased."""
    fit: str = "exact"
    src_fps: object = None
    window: str = "last"
    start_s: object = 0.0
    crop: tuple | None = None
    filter: str = "bilinear"

    def __post_init__(self):
        if self.fit not in FITS:
            raise ValueError(f"ConformConfig: fit must be one of {FITS}, got {self.fit!r}")
        if self.window not in WINDOWS:
            raise ValueError(f"ConformConfig: window must be one of {WINDOWS}, got {self.window!r}")
        if self.filter not in FILTERS:
            raise ValueError(f"ConformConfig: filter must be one of {tuple(FILTERS)}, got {self.filter!r}")
        if self.src_fps is not None and not _rational(self.src_fps) > 0:
            raise ValueError(f"ConformConfig: src_fps must be positive, got {self.src_fps!r}")
        if _rational(self.start_s) < 0:
            raise ValueError(f"ConformConfig: start_s must be >= 0, got {self.start_s!r}")
        if _rational(self.start_s) != 0 and (self.src_fps is None or self.window != "first"):
            raise ValueError("ConformConfig: start_s goes with src_fps and window='first'")
        if self.crop is not None and (len(self.crop) != 4 or any(int(v) != v for v in self.crop)):
            raise ValueError(f"ConformConfig: crop must be four integers (y0, x0, h, w), got {self.crop!r}")


@dataclass(frozen=True)
class ConformPlan:
    frame_idx: tuple          # source frame of every output frame
    box: tuple                # (y0, x0, h, w) of the source, in pixels
    out_shape: tuple          # (n_frames, H, W)
    scale_y: float            # box h / H
    scale_x: float
    src_fps: object           # Fraction or None
    fit: str
    filter: str = "bilinear"

    def as_dict(self) -> dict:
        """What LanDiffPipeline.last_conform and <name>_conform.json hold (plain JSON types)."""
        return dict(fit=self.fit, filter=self.filter, box=list(self.box), out_shape=list(self.out_shape), scale_y=self.scale_y,
                    scale_x=self.scale_x, src_fps=None if self.src_fps is None else float(self.src_fps),
                    frame_idx=list(self.frame_idx))


def _rational(v) -> Fraction:
    """Exact rational of an int, a Fraction, a decimal / ratio string or a float's shortest decimal (29.97 -> 2997/100)."""
    return Fraction(str(v)) if isinstance(v, float) else Fraction(v)


def _half_up(q: Fraction) -> int:
    return (q + Fraction(1, 2)).__floor__()


def cover_box(Hs: int, Ws: int, H: int, W: int) -> tuple:
    """The largest centred box of aspect W : H inside Hs x Ws: integer arithmetic, floor, the odd pixel on the bottom / right."""
    if Ws * H >= Hs * W:
        hc, wc = Hs, (Hs * W) // H
    else:
        hc, wc = (Ws * H) // W, Ws
    hc, wc = max(hc, 1), max(wc, 1)
    return ((Hs - hc) // 2, (Ws - wc) // 2, hc, wc)


def conform_plan(src_shape, n_frames: int, H: int, W: int, cfg: ConformConfig) -> ConformPlan:
    """The frames and the box a clip of src_shape (F, Hs, Ws[, C]) gives for n_frames frames of H x W.  Output frame k lies at
    k / MODEL_FPS seconds; with src_fps the source index is round-half-up(start_s fps + k fps / MODEL_FPS) (window="first") or
    F - 1 - round-half-up((n_frames - 1 - k) fps / MODEL_FPS) (window="last": counted back from the last frame), in exact rational
    arithmetic.  A clip too short raises ValueError with the duration it needs."""
    from .pipeline import MODEL_FPS
    F, Hs, Ws = (int(v) for v in src_shape[:3])
    if min(F, Hs, Ws, n_frames, H, W) < 1:
        raise ValueError(f"conform_plan: empty shape (source {tuple(src_shape)}, target {n_frames} x {H} x {W})")
    if cfg.fit == "exact":
        if (Hs, Ws) != (H, W):
            raise ValueError(f"fit='exact' takes frames of {H} x {W}, got {Hs} x {Ws} (fit='cover' or 'stretch' resamples)")
        box = (0, 0, Hs, Ws)
    elif cfg.crop is not None:
        box = tuple(int(v) for v in cfg.crop)
        y0, x0, hc, wc = box
        if y0 < 0 or x0 < 0 or hc < 1 or wc < 1 or y0 + hc > Hs or x0 + wc > Ws:
            raise ValueError(f"conform_plan: crop {box} leaves the {Hs} x {Ws} source")
    elif cfg.fit == "cover":
        box = cover_box(Hs, Ws, H, W)
    else:
        box = (0, 0, Hs, Ws)
    fps = None if cfg.src_fps is None else _rational(cfg.src_fps)
    if fps is None:
        if F < n_frames:
            raise ValueError(f"a clip of {F} frames is too short: {n_frames} frames are taken one to one")
        first = F - n_frames if cfg.window == "last" else 0
        idx = tuple(range(first, first + n_frames))
    else:
        step = fps / MODEL_FPS
        if cfg.window == "first":
            idx = tuple(_half_up(_rational(cfg.start_s) * fps + k * step) for k in range(n_frames))
        else:
            idx = tuple(F - 1 - _half_up((n_frames - 1 - k) * step) for k in range(n_frames))
        if idx[0] < 0 or idx[-1] > F - 1:
            need = _rational(cfg.start_s) + Fraction(n_frames - 1, MODEL_FPS)
            raise ValueError(f"a clip of {F} frames at {float(fps):g} fps ({float((F - 1) / fps):.3f} s between its first and last "
                             f"frame) is too short: {n_frames} frames at {MODEL_FPS} fps need {float(need)} s")
    return ConformPlan(idx, box, (n_frames, H, W), box[2] / H, box[3] / W, fps, cfg.fit, cfg.filter)


def _kernel(filter_id: int, x):
    x = np.abs(x)
    if filter_id == 0:
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0,
                    np.where(x < 2.0, a * (((x - 5.0) * x + 8.0) * x - 4.0), 0.0))


@lru_cache(maxsize=64)
def axis_table64(n_in: int, n_out: int, filter: str):
    """PyTorch's antialias weights of one axis in float64: (lo int64 [n_out], cnt int64 [n_out], w float64 [n_out, tmax], zero past
    cnt).  scale = n_in / n_out; half = 1 (bilinear) or 2 (bicubic); support = half scale and inv = 1 / scale when scale >= 1, else
    half and 1; c = scale (i + 0.5); lo = max(0, int(c - support + 0.5)), hi = min(n_in, int(c + support + 0.5)); tap j in [lo, hi)
    weighs f((j - c + 0.5) inv), divided by the taps' sum."""
    fid = FILTERS[filter]
    half = 1.0 if fid == 0 else 2.0
    scale = n_in / n_out
    support, inv = (half * scale, 1.0 / scale) if scale >= 1.0 else (half, 1.0)
    c = scale * (np.arange(n_out, dtype=np.float64) + 0.5)
    lo = np.maximum(0, np.trunc(c - support + 0.5).astype(np.int64))
    hi = np.minimum(n_in, np.trunc(c + support + 0.5).astype(np.int64))
    cnt = hi - lo
    tmax = int(cnt.max())
    j = lo[:, None] + np.arange(tmax, dtype=np.int64)[None, :]
    w = _kernel(fid, (j - c[:, None] + 0.5) * inv)
    w = np.where(np.arange(tmax)[None, :] < cnt[:, None], w, 0.0)
    w = w / w.sum(axis=1, keepdims=True)
    for arr in (lo, cnt, w):
        arr.setflags(write=False)
    return lo, cnt, w


def axis_table(n_in: int, n_out: int, filter: str):
    """The tables ld_resize_u8 / ld_resize_mask_u8 take for one axis: win int32 [n_out, 2] = (lo, cnt) and w float32 [n_out, tmax],
    the float64 weights rounded once."""
    lo, cnt, w = axis_table64(int(n_in), int(n_out), filter)
    return np.ascontiguousarray(np.stack([lo, cnt], axis=1).astype(np.int32)), np.ascontiguousarray(w.astype(np.float32))


def _needed(frames, plan: ConformPlan, device):
    """Only the source frames the plan reads, selected on the host and uploaded, and the plan's indices into them."""
    import torch
    if frames.is_cuda:
        return frames.contiguous(), list(plan.frame_idx)
    uniq = sorted(set(plan.frame_idx))
    pos = {f: i for i, f in enumerate(uniq)}
    if uniq == list(range(uniq[0], uniq[-1] + 1)):
        sub = frames[uniq[0]:uniq[-1] + 1]
    else:
        sub = frames.index_select(0, torch.tensor(uniq, dtype=torch.long))
    return sub.contiguous().to(device), [pos[f] for f in plan.frame_idx]


def _check_source(t, plan: ConformPlan, what: str, dims: int):
    if t.dim() != dims or t.shape[0] <= max(plan.frame_idx) or plan.box[0] + plan.box[2] > t.shape[1] or plan.box[1] + plan.box[3] > t.shape[2]:
        raise ValueError(f"{what}: {tuple(t.shape)} does not hold the plan's frames (up to {max(plan.frame_idx)}) and box {plan.box}")


def conform_clip(frames, plan: ConformPlan, device):
    """uint8 frames [F, Hs, Ws, C] (host or device) -> uint8 [n_frames, H, W, C] on the device: the frames the plan reads are picked
    on the host, only those are uploaded, and one ld_resize_u8 launch crops, gathers and resamples them."""
    import torch
    from . import ops
    if frames.dtype != torch.uint8:
        raise ValueError(f"conform_clip: clip frames must be uint8 [F, H, W, C], got {frames.dtype} {tuple(frames.shape)}")
    _check_source(frames, plan, "conform_clip", 4)
    sub, idx = _needed(frames, plan, device)
    return ops.resize_u8(sub, plan.out_shape[1:], frame_idx=idx, box=plan.box, filter=plan.filter)


def conform_mask(mask, plan: ConformPlan, device):
    """bool (or uint8, non-zero = keep) keep-mask [F, Hs, Ws] in the source clip's geometry -> bool [n_frames, H, W] on the device:
    an output pixel is kept only if every source pixel in its tap window is kept (ld_resize_mask_u8)."""
    import torch
    from . import ops
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"conform_mask: the mask must be bool or uint8 [F, H, W], got {mask.dtype} {tuple(mask.shape)}")
    _check_source(mask, plan, "conform_mask", 3)
    sub, idx = _needed(mask, plan, device)
    return ops.resize_mask_u8(sub, plan.out_shape[1:], frame_idx=idx, box=plan.box, filter=plan.filter).bool()


def image_plan(img_shape, H: int, W: int, cfg: ConformConfig) -> ConformPlan:
    """The plan of an image [Hs, Ws, C] fitted to H x W: a one-frame clip with cfg's fit, crop and filter (no frame rate)."""
    if len(img_shape) != 3:
        raise ValueError(f"conform_image: expected a uint8 image [H, W, C], got {tuple(img_shape)}")
    return conform_plan((1,) + tuple(img_shape[:2]), 1, H, W, ConformConfig(fit=cfg.fit, crop=cfg.crop, filter=cfg.filter))


def conform_image(img, H: int, W: int, cfg: ConformConfig, device):
    """uint8 image [Hs, Ws, C] -> uint8 [H, W, C] on the device, fitted as a one-frame clip is (image_plan)."""
    return conform_clip(img[None], image_plan(tuple(img.shape), H, W, cfg), device)[0]
