"""Host side of the DiT step cache: the decision table of landiff_amd/dit_cache.py, the --dit_cache switch of the CLI and the
C-ABI entries of ld_dit_cache.hip (no GPU: nothing is launched)."""
import ctypes
import json
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_policy(cfg, rels, S=None, have_residual_after_compute=True):
    """Feeds relative changes rels[s] (None: no previous input) through a fresh policy the way the runner does: a residual exists
    from the first computed step on.  -> list of Decision."""
    from landiff_amd.dit_cache import StepCachePolicy
    pol = StepCachePolicy(cfg)
    S = len(rels) if S is None else S
    have, out = False, []
    for s, r in enumerate(rels):
        d = pol.decide(s, S, None if r is None else r * 4.0, None if r is None else 4.0, have)
        have = have or (d.computed and have_residual_after_compute)
        out.append(d)
    return out


def computed(decisions):
    return [d.computed for d in decisions]


def test_threshold_zero_computes_every_step():
    from landiff_amd.dit_cache import StepCacheConfig
    ds = run_policy(StepCacheConfig(0.0), [None, 0.0, 0.0, 1e-9, 0.0, 0.0])
    assert computed(ds) == [True] * 6


def test_first_and_last_steps_are_always_computed():
    from landiff_amd.dit_cache import StepCacheConfig
    ds = run_policy(StepCacheConfig(math.inf), [None, 0.5, 0.5, 0.5, 0.5, 0.5])
    assert computed(ds) == [True, False, False, False, False, True]
    ds = run_policy(StepCacheConfig(math.inf), [0.0, 0.0])               # a previous input at step 0 changes nothing
    assert computed(ds) == [True, True]


def test_accumulator_adds_up_and_resets_after_a_compute():
    from landiff_amd.dit_cache import StepCacheConfig
    # 0.25 per step under a threshold of 0.6: 0.25 skip, 0.5 skip, 0.75 compute (acc -> 0), 0.25 skip, 0.5 skip, last
    ds = run_policy(StepCacheConfig(0.6), [None, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25])
    assert computed(ds) == [True, False, False, True, False, False, True]
    assert [d.accumulated for d in ds] == [0.0, 0.25, 0.5, 0.75, 0.25, 0.5, 0.0]
    assert [d.input_rel_l1 for d in ds] == [None] + [0.25] * 6
    # skip iff acc < threshold: equality computes
    ds = run_policy(StepCacheConfig(0.5), [None, 0.25, 0.25, 0.25, 0.25])
    assert computed(ds) == [True, False, True, False, True]


def test_polynomial_coefficients_rescale_the_change():
    from landiff_amd.dit_cache import StepCacheConfig, poly
    assert poly((1.0, 0.0), 0.3) == 0.3 and poly((2.0, 3.0, 4.0), 0.5) == 2.0 * 0.25 + 3.0 * 0.5 + 4.0
    # 4 r^2 + 0.125: r = 0.25 -> 0.375 per step
    ds = run_policy(StepCacheConfig(0.5, coefficients=(4.0, 0.0, 0.125)), [None, 0.25, 0.25, 0.25, 0.25])
    assert [d.accumulated for d in ds] == [0.0, 0.375, 0.75, 0.375, 0.0]
    assert computed(ds) == [True, False, True, False, True]
    # the identity default would have skipped all three interior steps
    assert computed(run_policy(StepCacheConfig(0.8), [None, 0.25, 0.25, 0.25, 0.25])) == [True, False, False, False, True]


def test_max_consecutive_skips_caps_a_run():
    from landiff_amd.dit_cache import StepCacheConfig
    ds = run_policy(StepCacheConfig(math.inf, max_consecutive_skips=2), [None] + [0.1] * 8)
    assert computed(ds) == [True, False, False, True, False, False, True, False, True]
    assert computed(run_policy(StepCacheConfig(math.inf, max_consecutive_skips=0), [None] + [0.1] * 4)) == [True] * 5


def test_plan_overrides_the_threshold_but_not_the_guards():
    from landiff_amd.dit_cache import StepCacheConfig, StepCachePolicy
    C, S = True, False
    # the threshold (0: compute everything) is ignored where the plan says skip; step 0 and the last step cannot be skipped
    ds = run_policy(StepCacheConfig(0.0, plan=(S, S, C, S, S, S)), [None, 0.9, 0.9, 0.9, 0.9, 0.9])
    assert computed(ds) == [True, False, True, False, False, True]
    # ... nor a step without a cached residual
    ds = run_policy(StepCacheConfig(0.0, plan=(C, S, S, C)), [None, 0.1, 0.1, 0.1], have_residual_after_compute=False)
    assert computed(ds) == [True, True, True, True]
    # an all-compute plan computes where the threshold alone would skip
    assert computed(run_policy(StepCacheConfig(math.inf, plan=(C,) * 5), [None, 0.0, 0.0, 0.0, 0.0])) == [True] * 5
    with pytest.raises(ValueError, match="plan"):
        StepCachePolicy(StepCacheConfig(0.1, plan=(C, S, C))).decide(0, 4, None, None, False)


def test_zero_denominator_or_nan_forces_a_compute():
    from landiff_amd.dit_cache import StepCacheConfig, StepCachePolicy
    for plan in (None, (True, False, False, True)):
        for num, den in ((0.0, 0.0), (1.0, 0.0), (math.nan, 1.0), (1.0, math.nan), (math.inf, 1.0), (None, None)):
            pol = StepCachePolicy(StepCacheConfig(math.inf, plan=plan))
            assert pol.decide(0, 4, None, None, False).computed
            d = pol.decide(1, 4, num, den, True)
            assert d.computed and d.accumulated == 0.0, (plan, num, den)
            assert pol.decide(2, 4, 0.1, 1.0, True).computed is False          # the policy goes on afterwards
    # the ratio is formed in float64: two float32-sized sums whose quotient float32 would round
    pol = StepCachePolicy(StepCacheConfig(math.inf))
    pol.decide(0, 3, None, None, False)
    assert pol.decide(1, 3, 1.0, 3.0, True).input_rel_l1 == 1.0 / 3.0


def test_config_validation_and_as_config():
    from landiff_amd.dit_cache import StepCacheConfig, as_config
    for bad in (-1.0, math.nan):
        with pytest.raises(ValueError):
            StepCacheConfig(bad)
    with pytest.raises(ValueError):
        StepCacheConfig(0.1, coefficients=())
    with pytest.raises(ValueError):
        StepCacheConfig(0.1, max_consecutive_skips=-1)
    assert as_config(None) is None and as_config(0.25) == StepCacheConfig(0.25) and as_config(0) == StepCacheConfig(0.0)
    cfg = StepCacheConfig(0.1, plan=[1, 0, 1])
    assert as_config(cfg) is cfg and cfg.plan == (True, False, True) and cfg.coefficients == (1.0, 0.0)
    with pytest.raises(TypeError):
        as_config("0.1")


def test_cli_dit_cache_switch(monkeypatch, tmp_path):
    import landiff.infer_video as iv
    assert iv.parse_args(["--prompt", "p"]).dit_cache is None
    assert iv.parse_args(["--prompt", "p", "--dit_cache", "0.15"]).dit_cache == 0.15
    assert iv.parse_args(["--prompt", "p", "--dit_cache", "0"]).dit_cache == 0.0
    for bad in ("-1", "x", "nan", "-0.5"):
        with pytest.raises(SystemExit):
            iv.parse_args(["--prompt", "p", "--dit_cache", bad])
    # the value reaches the diffusion stage, and the report lands beside the video
    seen = {}

    class FakeModel:
        def __init__(self, **kw):
            seen.update(kw)

        def __call__(self, task):
            task.result = "video"
            return task

        def dit_cache_report(self):
            return [dict(index=0, timestep=999, input_rel_l1=None, accumulated=0.0, computed=True, output_rel_l1=None),
                    dict(index=1, timestep=500, input_rel_l1=math.inf, accumulated=0.0, computed=True, output_rel_l1=0.5)]

    monkeypatch.setattr(iv, "CogModelInferWrapper", FakeModel)
    monkeypatch.setattr(iv, "save_video_tensor", lambda *a, **k: None)
    stem = str(tmp_path / "out" / "v")
    iv.infer_diffusion(iv.parse_args(["--prompt", "p", "--dit_cache", "0.2", "--save_file_name", stem]), None)
    assert seen == {"ckpt_path": "ckpts/LanDiff/diffusion", "dit_cache": 0.2}
    rows = json.load(open(stem + "_dit_cache.json"))
    assert [r["computed"] for r in rows] == [True, True] and rows[1]["input_rel_l1"] is None and rows[1]["output_rel_l1"] == 0.5
    seen.clear()
    iv.infer_diffusion(iv.parse_args(["--prompt", "p", "--save_file_name", stem + "2"]), None)      # off: the call as it was
    assert seen == {"ckpt_path": "ckpts/LanDiff/diffusion"} and not os.path.exists(stem + "2_dit_cache.json")


def test_cabi_entries_and_refusals_before_any_launch():
    from landiff_amd import _lib, ops
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "landiff_hip.h")).read()
    for name in ("ld_absdiff_sums", "ld_residual_sub", "ld_residual_add"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(rf"\bint {name}\(", hdr)
    assert int(re.search(r"#define LD_DIT_CACHE_WS_FLOATS (\d+)", hdr).group(1)) == ops.DIT_CACHE_WS_FLOATS
    p16 = ctypes.c_void_p(16)
    assert lib.ld_absdiff_sums(p16, p16, 8, p16, p16, 0, None) < 0 and b"same buffer" in lib.ld_last_error()
    assert lib.ld_absdiff_sums(p16, ctypes.c_void_p(32), 0, p16, p16, 0, None) < 0 and b"at least 1" in lib.ld_last_error()
    assert lib.ld_absdiff_sums(p16, ctypes.c_void_p(32), 8, None, p16, 0, None) < 0 and b"null" in lib.ld_last_error()
    assert lib.ld_residual_sub(p16, p16, p16, 8, p16, None, None, None) < 0 and b"out2" in lib.ld_last_error()
    assert lib.ld_residual_sub(p16, p16, None, 8, None, None, None, None) < 0
    assert lib.ld_residual_add(p16, p16, p16, 0, None) < 0 and b"at least 1" in lib.ld_last_error()


def test_ops_wrappers_refuse_cpu_tensors_and_wrong_operands():
    import torch
    from landiff_amd import _lib, ops
    a, b = torch.zeros(4, 8, dtype=torch.bfloat16), torch.ones(4, 8, dtype=torch.bfloat16)
    for call in (lambda: ops.absdiff_sums(a, b, out=torch.zeros(2), workspace=torch.zeros(ops.DIT_CACHE_WS_FLOATS)),
                 lambda: ops.residual_sub(a, b), lambda: ops.residual_add(a, b)):
        with pytest.raises(_lib.LandiffHipError, match="GPU"):
            call()
    with pytest.raises(TypeError, match="bfloat16"):
        ops.residual_add(a.float(), b)
    with pytest.raises(ValueError, match="one shape"):
        ops.residual_sub(a, b[:2])
    with pytest.raises(ValueError, match="one shape"):
        ops.absdiff_sums(a, b.t())
    with pytest.raises(ValueError, match="workspace"):
        ops.absdiff_sums(a, b, out=torch.zeros(2), workspace=torch.zeros(8))


def test_the_switch_is_off_by_default_at_every_level():
    """step_cache / plan_timesteps of the runner and dit_cache of the pipeline exist and default to None (the refusal of a config
    without plan_timesteps needs device buffers first: tests/test_gpu_dit_cache.py)."""
    import inspect
    from landiff_amd.dit import ControlDiTRunner
    sig = inspect.signature(ControlDiTRunner.__init__)
    assert sig.parameters["step_cache"].default is None and sig.parameters["plan_timesteps"].default is None
    from landiff_amd.pipeline import LanDiffPipeline
    assert inspect.signature(LanDiffPipeline.__init__).parameters["dit_cache"].default is None


def test_fit_tool_recovers_a_polynomial_and_refuses_skipping_runs(tmp_path, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("fit_dit_cache_poly", os.path.join(ROOT, "tools", "fit_dit_cache_poly.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    f = lambda r: 2.0 * r * r + 0.5 * r + 0.01
    rep = [dict(index=0, timestep=999, input_rel_l1=None, accumulated=0.0, computed=True, output_rel_l1=None)]
    rep += [dict(index=s, timestep=999 - s, input_rel_l1=0.02 * s, accumulated=0.0, computed=True, output_rel_l1=f(0.02 * s)) for s in range(1, 9)]
    one, many = tmp_path / "a_dit_cache.json", tmp_path / "b_dit_cache.json"
    json.dump(rep, open(one, "w")); json.dump([rep, rep], open(many, "w"))
    co = mod.main([str(one), str(many), "--degree", "2"])
    assert len(co) == 3 and all(abs(a - b) < 1e-9 for a, b in zip(co, (2.0, 0.5, 0.01)))
    assert "coefficients=(" in capsys.readouterr().out
    from landiff_amd.dit_cache import StepCacheConfig, poly
    assert abs(poly(StepCacheConfig(0.1, coefficients=co).coefficients, 0.1) - f(0.1)) < 1e-9
    rep[3]["computed"] = False
    json.dump(rep, open(one, "w"))
    with pytest.raises(ValueError, match="all-compute"):
        mod.main([str(one)])
