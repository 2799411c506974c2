"""Clip comparison: PSNR, SSIM and exact difference counts of two uint8 clips, computed where the frames already are.

compare_clips runs ld_clip_diff_u8 and ld_clip_ssim_u8 (ld_metrics.hip) and does the few divisions and logarithms left on the host
in float64, from the exact integer sums.  It is an instrument, not a stage: nothing on the generation path calls it."""
from __future__ import annotations

import dataclasses
import json
import math

import torch

from . import ops

PEAK = 255.0


@dataclasses.dataclass
class ClipMetrics:
    """What compare_clips returns; every tensor is on the host.  A *value* is one channel of one pixel.

    Per frame [F]: psnr (float64; inf where the frames agree, nan where nothing is counted), ssim (float64: the mean over channels of
    the channel's mean SSIM, nan where no map position is counted; None as a whole when H or W < 11), mse and mae (float64, over the
    counted values of all channels), max_abs, differing (values with a != b) and counted (values counted) as int64.
    The clip as a whole: clip_psnr from the clip's total squared difference, clip_ssim the mean of the frames' SSIM that exist (nan
    when none does, None with ssim), clip_mse, clip_mae, clip_max_abs, clip_differing, clip_counted.
    Raw: diff int64 [F, C, 5] = (n, sum d^2, sum |d|, max |d|, n differing) and ssim_sums float64 [F, C, 2] = (sum, count) or None."""
    shape: tuple
    psnr: torch.Tensor
    ssim: torch.Tensor | None
    mse: torch.Tensor
    mae: torch.Tensor
    max_abs: torch.Tensor
    differing: torch.Tensor
    counted: torch.Tensor
    clip_psnr: float
    clip_ssim: float | None
    clip_mse: float
    clip_mae: float
    clip_max_abs: int
    clip_differing: int
    clip_counted: int
    diff: torch.Tensor
    ssim_sums: torch.Tensor | None

    def as_dict(self) -> dict:
        """Plain Python types (lists per frame; the raw per-channel arrays under "channels"); non-finite floats stay floats here and
        become null in write_metrics_json."""
        ls = lambda t: None if t is None else t.tolist()
        return {
            "shape": list(self.shape),
            "clip": {"psnr": self.clip_psnr, "ssim": self.clip_ssim, "mse": self.clip_mse, "mae": self.clip_mae,
                     "max_abs": self.clip_max_abs, "differing": self.clip_differing, "counted": self.clip_counted},
            "frames": {"psnr": ls(self.psnr), "ssim": ls(self.ssim), "mse": ls(self.mse), "mae": ls(self.mae),
                       "max_abs": ls(self.max_abs), "differing": ls(self.differing), "counted": ls(self.counted)},
            "channels": {"diff": ls(self.diff), "ssim_sums": ls(self.ssim_sums)},
        }


def psnr_from_sums(ssd, n) -> torch.Tensor:
    """10 log10(255^2 n / SSD) in float64 from exact integer sums (exact in float64 below 2^53): inf where SSD is 0 and n is not,
    nan where n is 0 (0 / 0) -- IEEE division and log10 give both."""
    ssd, n = torch.as_tensor(ssd, dtype=torch.float64), torch.as_tensor(n, dtype=torch.float64)
    return 10.0 * torch.log10(PEAK * PEAK * n / ssd)


def _mean(total: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    """total / count in float64; nan where nothing was counted (the total is 0 there)."""
    return total.double() / count.double()


def metrics_from_sums(shape, diff: torch.Tensor, ssim_sums: torch.Tensor | None) -> ClipMetrics:
    """The host's part of compare_clips: diff int64 [F, C, 5] and ssim_sums float64 [F, C, 2] (or None) -> ClipMetrics."""
    diff = diff.cpu()
    n, ssd, sad = diff[..., 0].sum(1), diff[..., 1].sum(1), diff[..., 2].sum(1)            # exact: int64
    ssim = clip_ssim = None
    if ssim_sums is not None:
        ssim_sums = ssim_sums.cpu()
        ssim = _mean(ssim_sums[..., 0], ssim_sums[..., 1]).mean(1)
        have = ~torch.isnan(ssim)
        clip_ssim = float(ssim[have].mean()) if bool(have.any()) else math.nan
    N, SSD, SAD = int(n.sum()), int(ssd.sum()), int(sad.sum())
    return ClipMetrics(
        shape=tuple(shape), psnr=psnr_from_sums(ssd, n), ssim=ssim, mse=_mean(ssd, n), mae=_mean(sad, n),
        max_abs=diff[..., 3].amax(1), differing=diff[..., 4].sum(1), counted=n,
        clip_psnr=float(psnr_from_sums(SSD, N)), clip_ssim=clip_ssim, clip_mse=SSD / N if N else math.nan,
        clip_mae=SAD / N if N else math.nan, clip_max_abs=int(diff[..., 3].max()), clip_differing=int(diff[..., 4].sum()),
        clip_counted=N, diff=diff, ssim_sums=ssim_sums)


def compare_clips(a: torch.Tensor, b: torch.Tensor, mask: torch.Tensor | None = None) -> ClipMetrics:
    """Two uint8 clips [F, H, W, C] (C 1 or 3) of one shape on one GPU, and an optional bool keep-mask [F, H, W] -> ClipMetrics.
    Only kept pixels enter the integer statistics; SSIM averages the map positions whose centre pixel is kept.  Nothing is resized:
    shapes that differ raise ValueError.  H or W < 11 has no SSIM (ssim is None); everything else is still returned."""
    diff = ops.clip_diff_u8(a, b, mask)
    ssim_sums = ops.clip_ssim_u8(a, b, mask) if min(a.shape[1], a.shape[2]) >= ops.SSIM_TAPS else None
    return metrics_from_sums(a.shape, diff, ssim_sums)


def temporal_profile(a: torch.Tensor) -> ClipMetrics:
    """Frame-to-frame change of one clip: compare_clips(a[1:], a[:-1]), entry k comparing frame k + 1 with frame k (flicker shows
    as low SSIM / PSNR between neighbours).  The clip needs two frames."""
    if not isinstance(a, torch.Tensor) or a.dim() != 4 or a.shape[0] < 2:
        raise ValueError(f"temporal_profile: a clip [F, H, W, C] of at least two frames, got {tuple(getattr(a, 'shape', ()))}")
    return compare_clips(a[1:], a[:-1])


def _jsonable(v):
    if isinstance(v, ClipMetrics):
        v = v.as_dict()
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, float) and not math.isfinite(v):
        return None
    return v


def write_metrics_json(path: str, metrics) -> dict:
    """A ClipMetrics (or a dict / list holding some) as JSON; a float that is not finite is written as null (JSON has no infinity
    and no nan), as write_edit_json does.  -> what was written."""
    row = _jsonable(metrics)
    with open(path, "w") as f:
        json.dump(row, f, indent=1, allow_nan=False)
    return row
