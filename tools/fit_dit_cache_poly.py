"""Calibrates StepCacheConfig.coefficients for a checkpoint: fits the output-side change of the DiT step cache's reports against the
input-side indicator.

Input: one or more report files of ALL-COMPUTE runs (StepCacheConfig(threshold, plan=(True,) * S): every step runs the stack, so every
step from the second on carries both figures) -- <name>_dit_cache.json as infer_video --dit_cache writes them, or
json.dump(pipe.dit_cache_report()).  A file may hold one report (a list of step dicts) or a list of reports (chunks of a stream).

  input_rel_l1  = sum|mod_s - mod_(s-1)| / sum|mod_(s-1)|    the first main block's modulated input, what the policy sees
  output_rel_l1 = sum|res_s - res_(s-1)| / sum|res_(s-1)|    the residual across the whole stack, what a skipped step gets wrong

numpy.polyfit(input, output, degree) gives the polynomial, highest power first, that turns the first into an estimate of the second;
the policy accumulates that estimate, so a threshold then reads as "tolerated relative drift of the residual".  Prints a
`coefficients=` tuple to paste into StepCacheConfig.  The repository ships no fitted coefficients: they belong to a checkpoint.

    python tools/fit_dit_cache_poly.py run1_dit_cache.json [run2_dit_cache.json ...] [--degree 4]
"""
import argparse
import json
import math

import numpy as np


def pairs_of(report) -> list:
    """(input_rel_l1, output_rel_l1) of every step of one report that has both, after checking that the run computed every step."""
    skipped = [r["index"] for r in report if not r["computed"]]
    if skipped:
        raise ValueError(f"steps {skipped} were skipped: calibrate on all-compute runs (plan=(True,) * S)")
    out = []
    for r in report:
        a, b = r.get("input_rel_l1"), r.get("output_rel_l1")
        if a is not None and b is not None and math.isfinite(a) and math.isfinite(b):
            out.append((float(a), float(b)))
    return out


def load_pairs(paths) -> list:
    out = []
    for p in paths:
        with open(p) as f:
            data = json.load(f)
        reports = data if data and isinstance(data[0], list) else [data]
        for rep in reports:
            out += pairs_of(rep)
    return out


def fit(pairs, degree: int) -> tuple:
    if len(pairs) <= degree:
        raise ValueError(f"{len(pairs)} points cannot determine a polynomial of degree {degree}")
    x, y = np.array([p[0] for p in pairs], np.float64), np.array([p[1] for p in pairs], np.float64)
    return tuple(float(c) for c in np.polyfit(x, y, degree))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("reports", nargs="+")
    ap.add_argument("--degree", type=int, default=4)
    a = ap.parse_args(argv)
    pairs = load_pairs(a.reports)
    co = fit(pairs, a.degree)
    x = np.array([p[0] for p in pairs]); y = np.array([p[1] for p in pairs])
    resid = np.polyval(co, x) - y
    print(f"{len(pairs)} steps from {len(a.reports)} file(s); input_rel_l1 in [{x.min():.4g}, {x.max():.4g}], "
          f"output_rel_l1 in [{y.min():.4g}, {y.max():.4g}]; rms residual of the fit {float(np.sqrt((resid ** 2).mean())):.4g}")
    print("coefficients=(" + ", ".join(repr(c) for c in co) + ("," if len(co) == 1 else "") + ")")
    return co


if __name__ == "__main__":
    main()
