"""CFG branch skipping of the control DiT: the decision whether a sampler step evaluates the CFG pair (uncond, cond) or the cond
branch alone (host logic only; the runner side is ControlDiTRunner(dit_guidance=...), landiff_amd/dit.py, the kernels
ld_dit_guidance.hip).

Training-free, three variants serving stacks ship for CogVideoX-class models behind one mechanism: guidance dropped where its scale
is (nearly) 1 (`scale_tolerance`: u + s (c - u) = c + (s - 1)(c - u), so the unconditional branch moves the result by (s - 1) delta),
the last cond - uncond difference reused for a few steps (`refresh`), and guidance dropped for the rest of a run once the two
branches agree (`cos_threshold`).  Off by default; nothing here claims anything about the quality of a trained checkpoint under any
setting.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

MODES = ("full", "reuse", "cond")

# why ControlDiTRunner refuses the two combinations (infer_video refuses --dit_cache with --dit_cfg_* in the same words)
REFUSE_STEP_CACHE = ("dit_guidance and step_cache cannot be combined: the step cache's residual is a B = 2 object and has no "
                     "meaning on a cond-only step")
REFUSE_FP8 = ("dit_guidance and fp8_gemm cannot be combined: the MXFP8 scale buffers are K-tile-major and have no batch-1 view "
              "for a cond-only step")


@dataclass(frozen=True)
class GuidanceSkipConfig:
    """scale_tolerance: a step whose |cfg_scale - 1| is at most this runs the cond branch alone (None: never on this ground).
    refresh: a full step every `refresh` guided steps, the steps between reuse its difference (1: every step full; None: the same).
    cos_threshold: after a full step whose branch outputs have a cosine of at least this, every later step of the run is cond-only.
    plan: one of "full" / "reuse" / "cond" per sampler step.  Overrides the rules; for tests and for timing."""
    scale_tolerance: "float | None" = None
    refresh: "int | None" = None
    cos_threshold: "float | None" = None
    plan: "tuple | None" = None

    def __post_init__(self):
        if self.scale_tolerance is not None:
            t = float(self.scale_tolerance)
            if math.isnan(t) or t < 0:
                raise ValueError(f"GuidanceSkipConfig: scale_tolerance must be >= 0, got {self.scale_tolerance!r}")
            object.__setattr__(self, "scale_tolerance", t)
        if self.refresh is not None:
            if isinstance(self.refresh, bool) or int(self.refresh) != self.refresh or int(self.refresh) < 1:
                raise ValueError(f"GuidanceSkipConfig: refresh must be an integer >= 1, got {self.refresh!r}")
            object.__setattr__(self, "refresh", int(self.refresh))
        if self.cos_threshold is not None:
            c = float(self.cos_threshold)
            if not -1.0 < c <= 1.0:          # (a NaN fails both comparisons)
                raise ValueError(f"GuidanceSkipConfig: cos_threshold must lie in (-1, 1], got {self.cos_threshold!r}")
            object.__setattr__(self, "cos_threshold", c)
        if self.plan is not None:
            plan = tuple(self.plan)
            for m in plan:
                if m not in MODES:
                    raise ValueError(f"GuidanceSkipConfig: plan entries must be one of {MODES}, got {m!r}")
            object.__setattr__(self, "plan", plan)


def cosine(sum_uc: float, sum_uu: float, sum_cc: float) -> "float | None":
    """Sum e_u e_c / sqrt(Sum e_u^2 Sum e_c^2) in float64; None for a zero or non-finite denominator."""
    den = math.sqrt(float(sum_uu) * float(sum_cc)) if float(sum_uu) >= 0 and float(sum_cc) >= 0 else float("nan")
    if not math.isfinite(den) or den == 0.0:
        return None
    return float(sum_uc) / den


class GuidanceSkipPolicy:
    """Decides the mode of step s of S.  State: how many reuse steps ran since the last full step, and whether the cos rule has fired;
    reset() forgets both.  Whether a difference is kept is the caller's knowledge and comes with every call."""

    def __init__(self, cfg: GuidanceSkipConfig):
        self.cfg = cfg
        self.reset()

    def reset(self):
        self.reused = 0
        self.cos_fired = False

    def decide(self, s: int, S: int, cfg_scale: float, have_delta: bool, last_cos: "float | None" = None) -> str:
        """last_cos: the cosine of the latest full step of this run (None: none yet, or not known)."""
        cfg = self.cfg
        if not 0 <= s < S:
            raise ValueError(f"step index {s} outside [0, {S})")
        if cfg.plan is not None and len(cfg.plan) != S:
            raise ValueError(f"GuidanceSkipConfig.plan has {len(cfg.plan)} entries for a sampler of {S} steps")
        if cfg.cos_threshold is not None and last_cos is not None and float(last_cos) >= cfg.cos_threshold:
            self.cos_fired = True                     # sticky until reset() (a NaN compares False)
        if cfg.plan is not None:
            mode = cfg.plan[s]
        elif self.cos_fired:
            mode = "cond"
        elif cfg.scale_tolerance is not None and abs(float(cfg_scale) - 1.0) <= cfg.scale_tolerance:
            mode = "cond"
        elif cfg.refresh is not None and have_delta and self.reused < cfg.refresh - 1:
            mode = "reuse"
        else:
            mode = "full"
        if mode == "reuse" and not have_delta:
            mode = "full"
        if mode == "full":
            self.reused = 0
        elif mode == "reuse":
            self.reused += 1
        return mode                                   # (a cond step leaves the kept difference and the count alone)


def as_config(value) -> "GuidanceSkipConfig | None":
    """None / a scale tolerance / a GuidanceSkipConfig -> GuidanceSkipConfig or None (what LanDiffPipeline(dit_guidance=...) accepts)."""
    if value is None or isinstance(value, GuidanceSkipConfig):
        return value
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise TypeError(f"dit_guidance must be None, a scale tolerance (float >= 0) or a GuidanceSkipConfig, got {value!r}")
    return GuidanceSkipConfig(scale_tolerance=float(value))


def write_report_json(path: str, report) -> None:
    """<name>_dit_guidance.json of infer_video --dit_cfg_*: the step dicts of ControlDiTRunner.guidance_report (a list of such lists
    for a run of several chunks); values that are not finite are written as null (JSON has no infinity)."""
    import json

    def clean(v):
        if isinstance(v, (list, tuple)):
            return [clean(x) for x in v]
        if isinstance(v, dict):
            return {k: clean(x) for k, x in v.items()}
        if isinstance(v, float) and not math.isfinite(v):
            return None
        return v
    with open(path, "w") as f:
        json.dump(clean(report), f, indent=1)
