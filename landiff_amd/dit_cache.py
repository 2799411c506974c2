"""Step cache of the control DiT: the decision whether a sampler step runs the transformer stack or reuses the residual
the last computed step left across it (host logic only; the runner side is ControlDiTRunner(step_cache=...), landiff_amd/dit.py,
the kernels ld_dit_cache.hip).

Training-free, in the style of the caches serving stacks ship for CogVideoX: before a step, the timestep-modulated input of the
first main block is compared with the previous step's; while the accumulated relative change stays under a threshold the 45
layer-calls of the step are skipped and `h0 + residual` stands in for the stack's output.  Off by default; nothing here claims
anything about the quality of a trained checkpoint at a given threshold.
"""
from __future__ import annotations

import math
from dataclasses import dataclass


@dataclass(frozen=True)
class StepCacheConfig:
    """threshold: skip while the accumulated (rescaled) relative L1 change of the indicator stays below it; 0 computes every step,
    inf skips every step the rules allow.
    coefficients: polynomial applied to the relative change before it is accumulated, highest power first (numpy.polyfit's order;
    tools/fit_dit_cache_poly.py fits one to a checkpoint).  The default is the identity.
    max_consecutive_skips: compute after that many skipped steps in a row, whatever the indicator says (None: no cap).
    plan: one boolean per sampler step, True = compute.  Overrides the threshold; for tests and for timing."""
    threshold: float
    coefficients: tuple = (1.0, 0.0)
    max_consecutive_skips: "int | None" = None
    plan: "tuple | None" = None

    def __post_init__(self):
        t = float(self.threshold)
        if math.isnan(t) or t < 0:
            raise ValueError(f"StepCacheConfig: threshold must be >= 0, got {self.threshold!r}")
        object.__setattr__(self, "threshold", t)
        co = tuple(float(c) for c in self.coefficients)
        if not co or not all(math.isfinite(c) for c in co):
            raise ValueError(f"StepCacheConfig: coefficients must be a non-empty tuple of finite numbers, got {self.coefficients!r}")
        object.__setattr__(self, "coefficients", co)
        if self.max_consecutive_skips is not None:
            m = int(self.max_consecutive_skips)
            if m < 0 or m != self.max_consecutive_skips:
                raise ValueError(f"StepCacheConfig: max_consecutive_skips must be a non-negative integer, got {self.max_consecutive_skips!r}")
            object.__setattr__(self, "max_consecutive_skips", m)
        if self.plan is not None:
            object.__setattr__(self, "plan", tuple(bool(p) for p in self.plan))


def poly(coefficients, x: float) -> float:
    """Horner evaluation in float64, highest power first."""
    y = 0.0
    for c in coefficients:
        y = y * x + c
    return y


@dataclass
class Decision:
    computed: bool
    input_rel_l1: "float | None"      # Sum|cur - prev| / Sum|prev| (None: no previous input, or a zero denominator)
    accumulated: float                # what the threshold was compared with (0.0 on a step that had to be computed)


class StepCachePolicy:
    """Decides step s of S.  State: the accumulated change since the last computed step and the length of the current run of
    skipped steps; reset() forgets both.  Whether a residual is cached is the caller's knowledge and comes with every call."""

    def __init__(self, cfg: StepCacheConfig):
        self.cfg = cfg
        self.reset()

    def reset(self):
        self.acc = 0.0
        self.skipped_in_a_row = 0

    def decide(self, s: int, S: int, sum_absdiff: "float | None", sum_abs_prev: "float | None", have_residual: bool) -> Decision:
        """sum_absdiff, sum_abs_prev: Sum|cur - prev| and Sum|prev| of the indicator (None when there is no previous input)."""
        cfg = self.cfg
        if not 0 <= s < S:
            raise ValueError(f"step index {s} outside [0, {S})")
        if cfg.plan is not None and len(cfg.plan) != S:
            raise ValueError(f"StepCacheConfig.plan has {len(cfg.plan)} entries for a sampler of {S} steps")
        rel = None
        if sum_absdiff is not None and sum_abs_prev is not None and float(sum_abs_prev) != 0.0:
            rel = float(sum_absdiff) / float(sum_abs_prev)            # float64 on the host
        must = (s == 0 or s == S - 1 or not have_residual
                or (cfg.plan is not None and cfg.plan[s])
                or rel is None or not math.isfinite(rel)
                or (cfg.max_consecutive_skips is not None and self.skipped_in_a_row >= cfg.max_consecutive_skips))
        if must:
            return self._computed(rel, 0.0)
        self.acc += poly(cfg.coefficients, rel)
        acc = self.acc
        skip = True if cfg.plan is not None else acc < cfg.threshold          # (a NaN accumulator compares False: compute)
        if not skip:
            return self._computed(rel, acc)
        self.skipped_in_a_row += 1
        return Decision(False, rel, acc)

    def _computed(self, rel, acc) -> Decision:
        self.acc = 0.0
        self.skipped_in_a_row = 0
        return Decision(True, rel, acc)


def as_config(value) -> "StepCacheConfig | None":
    """None / a threshold / a StepCacheConfig -> StepCacheConfig or None (what LanDiffPipeline(dit_cache=...) accepts)."""
    if value is None or isinstance(value, StepCacheConfig):
        return value
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise TypeError(f"dit_cache must be None, a threshold (float >= 0) or a StepCacheConfig, got {value!r}")
    return StepCacheConfig(threshold=float(value))


def write_report_json(path: str, report) -> None:
    """<name>_dit_cache.json of infer_video --dit_cache: the step dicts of ControlDiTRunner.cache_report (a list of such lists for a
    run of several chunks); values that are not finite are written as null (JSON has no infinity)."""
    import json

    def clean(v):
        if isinstance(v, list):
            return [clean(x) for x in v]
        if isinstance(v, dict):
            return {k: clean(x) for k, x in v.items()}
        if isinstance(v, float) and not math.isfinite(v):
            return None
        return v
    with open(path, "w") as f:
        json.dump(clean(report), f, indent=1)
