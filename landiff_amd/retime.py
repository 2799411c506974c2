"""The retime stage: the model's clips delivered at another frame rate, on the device, in integer arithmetic.

The model produces frames at MODEL_FPS.  This stage makes uint8 frames [F, H, W, C] (C 1 or 3) at any other rate:

* the plan (retime_plan: which source frame and which phase p / q every output frame has) is pure Python rational arithmetic;
* the frames are one ld_retime_u8 launch: a phase-0 frame is a copy, every other is made from its two neighbours by bilateral
  block matching (8 x 8 blocks, a 16 x 16 luma window, SAD plus a length penalty, a total order on ties) and motion-compensated
  blending, every quantity an integer -- the rule is stated in DESIGN 8.11 and restated in numpy in tests/retime_ref.py;
* the same kernel gives a block motion field per frame pair (motion_profile).

The defaults search=8, penalty=4, max_sad=24 are a starting point nobody has tuned, and what block-matched interpolation looks
like on a trained checkpoint's output is not measured.  Nothing here runs unless it is asked for.
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction

from .conform import _rational

MAX_SEARCH = 32            # kMaxSearch of csrc/ld_retime.hip
MAX_Q = 65535


@dataclass(frozen=True)
class RetimeConfig:
    """out_fps: the rate of the frames to make (int, Fraction, a ratio string such as "30000/1001", or a float's shortest decimal).
    search: candidates are d in [-search, search]^2 (0: a rounded cross-fade).  penalty: cost per unit of |dy| + |dx|.  max_sad: a
    block whose best SAD exceeds max_sad * 256 (max_sad per window pixel) is cross-faded.  The three defaults are untuned."""
    out_fps: object
    search: int = 8
    penalty: int = 4
    max_sad: int = 24

    def __post_init__(self):
        check_search(self.search, self.penalty, self.max_sad, "RetimeConfig")
        try:
            fps = _rational(self.out_fps)
        except (ValueError, TypeError, ZeroDivisionError):
            raise ValueError(f"RetimeConfig: out_fps must be a number or a ratio, got {self.out_fps!r}") from None
        if not fps > 0:
            raise ValueError(f"RetimeConfig: out_fps must be positive, got {self.out_fps!r}")


def check_search(search, penalty, max_sad, who: str):
    for name, v, hi in (("search", search, MAX_SEARCH), ("penalty", penalty, 255), ("max_sad", max_sad, 255)):
        if isinstance(v, bool) or int(v) != v or not 0 <= v <= hi:
            raise ValueError(f"{who}: {name} must be an integer in 0..{hi}, got {v!r}")


@dataclass(frozen=True)
class RetimePlan:
    src_idx: tuple            # i_k: the source frame at or before output frame k
    phase_p: tuple            # p_k: output frame k lies at source position i_k + p_k / q; 0 = a copy of frame i_k
    q: int
    n_out: int
    out_fps: Fraction
    src_fps: Fraction
    search: int = 8
    penalty: int = 4
    max_sad: int = 24

    def as_dict(self) -> dict:
        """What LanDiffPipeline.last_retime and <name>_retime.json hold (plain JSON types)."""
        return dict(out_fps=float(self.out_fps), out_fps_ratio=[self.out_fps.numerator, self.out_fps.denominator],
                    src_fps=float(self.src_fps), q=self.q, n_out=self.n_out, src_idx=list(self.src_idx), phase_p=list(self.phase_p),
                    search=self.search, penalty=self.penalty, max_sad=self.max_sad)


def retime_plan(n_frames: int, cfg: RetimeConfig, src_fps=None) -> RetimePlan:
    """The plan of n_frames source frames at src_fps (default: the model's MODEL_FPS) delivered at cfg.out_fps.  With
    src_fps / out_fps = sn / sd in lowest terms, output frame k lies at source position k sn / sd = i_k + p_k / q: q = sd,
    i_k = (k sn) // sd, p_k = (k sn) mod sd, and n_out = ((n_frames - 1) sd) // sn + 1 -- the last output frame never reads past
    the last source frame.  Exact rational arithmetic; a q above 65535 is refused."""
    if src_fps is None:
        from .pipeline import MODEL_FPS
        src_fps = MODEL_FPS
    src = _rational(src_fps)
    if not src > 0:
        raise ValueError(f"retime_plan: src_fps must be positive, got {src_fps!r}")
    if isinstance(n_frames, bool) or int(n_frames) != n_frames or n_frames < 1:
        raise ValueError(f"retime_plan: a clip has at least 1 frame, got {n_frames!r}")
    F = int(n_frames)
    out = _rational(cfg.out_fps)
    step = src / out
    sn, sd = step.numerator, step.denominator
    if sd > MAX_Q:
        raise ValueError(f"retime_plan: {src} fps -> {out} fps puts the output frames at multiples of 1/{sd} of a source frame; "
                         f"q = {sd} exceeds {MAX_Q}")
    n_out = ((F - 1) * sd) // sn + 1
    idx = tuple((k * sn) // sd for k in range(n_out))
    ph = tuple((k * sn) % sd for k in range(n_out))
    return RetimePlan(idx, ph, sd, n_out, out, src, int(cfg.search), int(cfg.penalty), int(cfg.max_sad))


def _as_plan(frames, cfg_or_plan) -> RetimePlan:
    if isinstance(cfg_or_plan, RetimePlan):
        return cfg_or_plan
    if isinstance(cfg_or_plan, RetimeConfig):
        return retime_plan(int(frames.shape[0]), cfg_or_plan)
    raise TypeError(f"retime: expected a RetimeConfig or a RetimePlan, got {type(cfg_or_plan).__name__}")


def retime_clip(frames, cfg_or_plan, want_motion: bool = False):
    """uint8 frames [F, H, W, C] on the device -> uint8 [n_out, H, W, C] at the plan's rate: one ld_retime_u8 launch.  With
    want_motion also the motion field int16 [n_out, nby, nbx, 2] and the SAD int32 [n_out, nby, nbx] (zero rows for copied frames)."""
    from . import ops
    plan = _as_plan(frames, cfg_or_plan)
    return ops.retime_u8(frames, plan.src_idx, plan.phase_p, plan.q, plan.search, plan.penalty, plan.max_sad, want_motion=want_motion)


@dataclass
class MotionProfile:
    """Per neighbouring frame pair, from the phase-1/2 field: the mean and the max of |dy| + |dx| over the blocks (pixels per frame),
    the mean SAD per window pixel of the chosen candidates, and the share of blocks that fell back to the cross-fade; the raw fields
    (mv int16 [F - 1, nby, nbx, 2] after the fallback, sad int32 [F - 1, nby, nbx]) stay on the device."""
    mean_motion: list
    max_motion: list
    mean_sad_per_pixel: list
    fallback_share: list
    mv: object
    sad: object
    search: int
    penalty: int
    max_sad: int

    def as_dict(self) -> dict:
        n = len(self.mean_motion)
        return dict(pairs=n, blocks=[int(self.sad.shape[1]), int(self.sad.shape[2])], search=self.search, penalty=self.penalty,
                    max_sad=self.max_sad, mean_motion=list(self.mean_motion), max_motion=list(self.max_motion),
                    mean_sad_per_pixel=list(self.mean_sad_per_pixel), fallback_share=list(self.fallback_share),
                    clip_mean_motion=sum(self.mean_motion) / n if n else None,
                    clip_max_motion=max(self.max_motion) if n else None,
                    clip_fallback_share=sum(self.fallback_share) / n if n else None)


def motion_profile(frames, search: int = 8, penalty: int = 4, max_sad: int = 24) -> MotionProfile:
    """How much a clip moves: the block motion field half-way between every two neighbouring frames (one launch over the F - 1
    in-between frames; the frames themselves are made and dropped).  A block that fell back is one whose chosen SAD exceeds
    max_sad * 256: its stored vector is (0, 0)."""
    import torch
    from . import ops
    check_search(search, penalty, max_sad, "motion_profile")
    F = int(frames.shape[0])
    if F < 2:
        raise ValueError(f"motion_profile: a clip of {F} frame(s) has no frame pair")
    _, mv, sad = ops.retime_u8(frames, list(range(F - 1)), [1] * (F - 1), 2, search, penalty, max_sad, want_motion=True)
    l1 = mv.to(torch.int64).abs().sum(dim=-1)
    blocks = sad.shape[1] * sad.shape[2]
    stats = torch.stack([l1.sum(dim=(1, 2)), l1.amax(dim=(1, 2)), sad.to(torch.int64).sum(dim=(1, 2)),
                         (sad > max_sad * 256).sum(dim=(1, 2))]).cpu()          # exact integer sums; one copy to the host
    return MotionProfile(mean_motion=[int(v) / blocks for v in stats[0]], max_motion=[int(v) for v in stats[1]],
                         mean_sad_per_pixel=[int(v) / (blocks * 256) for v in stats[2]],
                         fallback_share=[int(v) / blocks for v in stats[3]], mv=mv, sad=sad, search=int(search),
                         penalty=int(penalty), max_sad=int(max_sad))
