"""CFG branch skipping of the DiT, host side: the config, the policy (table-driven), what the rules select on the shipped 50-step
schedule, the C ABI's declarations and refusals, the runner's and the command line's refusals, the report file, and the GEMM routes
the cond-only step's B = 1 shapes take.  No GPU."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, R, C = "full", "reuse", "cond"


def test_config_validation_and_as_config():
    from landiff_amd.dit_guidance import GuidanceSkipConfig, as_config
    for kw in (dict(scale_tolerance=-1e-9), dict(scale_tolerance=math.nan), dict(refresh=0), dict(refresh=-1), dict(refresh=1.5),
               dict(refresh=True), dict(cos_threshold=-1.0), dict(cos_threshold=1.0000001), dict(cos_threshold=math.nan),
               dict(plan=("full", "skip")), dict(plan=(True, False))):
        with pytest.raises(ValueError):
            GuidanceSkipConfig(**kw)
    c = GuidanceSkipConfig(scale_tolerance=0, refresh=2.0, cos_threshold=1, plan=[F, R, C])
    assert c.scale_tolerance == 0.0 and c.refresh == 2 and isinstance(c.refresh, int) and c.cos_threshold == 1.0 and c.plan == (F, R, C)
    assert GuidanceSkipConfig() == GuidanceSkipConfig(None, None, None, None)
    with pytest.raises(Exception):
        c.refresh = 3                                                            # frozen
    assert as_config(None) is None and as_config(c) is c
    assert as_config(1e-5) == GuidanceSkipConfig(scale_tolerance=1e-5) and as_config(0) == GuidanceSkipConfig(scale_tolerance=0.0)
    for bad in ("0.1", True, [0.1]):
        with pytest.raises(TypeError):
            as_config(bad)
    with pytest.raises(ValueError):
        as_config(-0.5)


def _drive(cfg, scales, cos=None, delta_from_start=False):
    """Runs the policy over a run the way the runner does: a full step leaves a difference (and a cosine, cos[s])."""
    from landiff_amd.dit_guidance import GuidanceSkipPolicy
    pol, have, last_cos, modes = GuidanceSkipPolicy(cfg), delta_from_start, None, []
    for s, sc in enumerate(scales):
        m = pol.decide(s, len(scales), sc, have, last_cos)
        modes.append(m)
        if m == F:
            have, last_cos = True, (cos[s] if cos is not None else None)
    return modes, pol


# (name, config keywords, guidance scale per step, cosine of a full step per step or None, expected modes)
POLICY_TABLE = [
    ("nothing set: every step full", {}, [3.0] * 4, None, [F] * 4),
    ("refresh=1 is all full", dict(refresh=1), [3.0] * 5, None, [F] * 5),
    ("refresh=2 alternates, starting full", dict(refresh=2), [3.0] * 5, None, [F, R, F, R, F]),
    ("refresh=3", dict(refresh=3), [3.0] * 7, None, [F, R, R, F, R, R, F]),
    ("tolerance selects by |s - 1|, both sides", dict(scale_tolerance=0.01), [1.0, 1.005, 1.011, 0.995, 0.98], None, [C, C, F, C, F]),
    ("tolerance 0 takes exactly 1", dict(scale_tolerance=0.0), [1.0, 1.0000001], None, [C, F]),
    ("tolerance precedes refresh; cond steps leave the reuse count alone", dict(scale_tolerance=0.01, refresh=3),
     [3.0, 3.0, 1.0, 1.0, 3.0, 3.0, 3.0], None, [F, R, C, C, R, F, R]),
    ("a cond step first: no difference yet, so the first guided step is full", dict(scale_tolerance=0.01, refresh=2),
     [1.0, 3.0, 3.0], None, [C, F, R]),
    ("cos fires after the full step that reaches it and sticks", dict(cos_threshold=0.9), [3.0] * 5, [0.5, 0.95, 0.1, 0.1, 0.1],
     [F, F, C, C, C]),
    ("cos precedes tolerance and refresh", dict(cos_threshold=0.9, refresh=2, scale_tolerance=0.01), [3.0, 3.0, 3.0, 1.0],
     [0.99, 0.0, 0.0, 0.0], [F, C, C, C]),
    ("cos below the threshold never fires; NaN / None neither", dict(cos_threshold=1.0), [3.0] * 4, [0.9999, math.nan, None, 0.5], [F] * 4),
    ("cos equal to the threshold fires", dict(cos_threshold=1.0), [3.0] * 3, [1.0, 0.0, 0.0], [F, C, C]),
    ("plan precedes everything", dict(plan=(F, C, R, F, R), cos_threshold=0.0, scale_tolerance=10.0, refresh=1), [3.0] * 5, [1.0] * 5,
     [F, C, R, F, R]),
    ("plan: a reuse without a difference becomes full", dict(plan=(R, R, C, R)), [3.0] * 4, None, [F, R, C, R]),
    ("plan: cond steps alone never make a difference", dict(plan=(C, R, C)), [3.0] * 3, None, [C, F, C]),
]


@pytest.mark.parametrize("name,kw,scales,cos,want", POLICY_TABLE, ids=[r[0] for r in POLICY_TABLE])
def test_policy_table(name, kw, scales, cos, want):
    from landiff_amd.dit_guidance import GuidanceSkipConfig
    modes, _ = _drive(GuidanceSkipConfig(**kw), scales, cos)
    assert modes == want


def test_policy_reset_and_argument_checks():
    from landiff_amd.dit_guidance import GuidanceSkipConfig, GuidanceSkipPolicy
    pol = GuidanceSkipPolicy(GuidanceSkipConfig(cos_threshold=0.5, refresh=3))
    assert pol.decide(0, 4, 3.0, False, None) == F
    assert pol.decide(1, 4, 3.0, True, 0.2) == R and pol.reused == 1
    assert pol.decide(2, 4, 3.0, True, 0.7) == C and pol.cos_fired
    assert pol.decide(3, 4, 3.0, True, 0.0) == C                                   # sticky, whatever later cosines say
    pol.reset()
    assert not pol.cos_fired and pol.reused == 0
    assert pol.decide(0, 4, 3.0, True, None) == R                                 # (the caller owns have_delta)
    with pytest.raises(ValueError, match="outside"):
        pol.decide(4, 4, 3.0, True, None)
    with pytest.raises(ValueError, match="entries"):
        GuidanceSkipPolicy(GuidanceSkipConfig(plan=(F, F))).decide(0, 3, 3.0, False, None)


def test_cosine_is_float64_and_guards_its_denominator():
    from landiff_amd.dit_guidance import cosine
    assert cosine(1.0, 3.0, 3.0) == 1.0 / 3.0
    assert cosine(1.0, 0.0, 3.0) is None and cosine(1.0, math.inf, 1.0) is None and cosine(1.0, math.nan, 1.0) is None
    assert cosine(-2.0, 4.0, 1.0) == -1.0


@pytest.mark.parametrize("tol,want", [(1e-5, {47, 48}), (0.01, {10, 47, 48}), (0.07, {6, 10, 27, 46, 47, 48})])
def test_scale_tolerance_on_the_shipped_schedule(tol, want):
    from landiff_amd.config import PipelineConfig
    from landiff_amd.dit_guidance import GuidanceSkipConfig
    from landiff_amd.schedule import build_plan
    plan = build_plan(PipelineConfig.full().sampler)
    assert len(plan) == 50
    modes, _ = _drive(GuidanceSkipConfig(scale_tolerance=tol), [sp.cfg_scale for sp in plan])
    assert {s for s, m in enumerate(modes) if m == C} == want and set(modes) == {F, C}


def test_cabi_entries_and_refusals_before_any_launch():
    from landiff_amd import _lib, ops
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "landiff_hip.h")).read()
    for name in ("ld_unpatchify_cfg_keep", "ld_unpatchify_cond"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(rf"\bint {name}\(", hdr)
    assert int(re.search(r"#define LD_DIT_GUIDANCE_WS_FLOATS (\d+)", hdr).group(1)) == ops.DIT_GUIDANCE_WS_FLOATS
    INVALID = -1
    p = ctypes.c_void_p(256)
    keep = lambda lin=p, x=p, out=p, delta=p, old=p, sums=p, ws=p, shape=(3, 16, 8, 12, 2): lib.ld_unpatchify_cfg_keep(
        lin, x, out, delta, old, sums, ws, *shape, 1.0, 1.0, 1.0, None)
    for k in ("lin", "x", "out", "delta", "sums", "ws"):
        assert keep(**{k: None}) == INVALID and b"null" in lib.ld_last_error(), k
    for shape in ((3, 16, 7, 12, 2), (3, 16, 8, 11, 2), (0, 16, 8, 12, 2), (3, 0, 8, 12, 2), (3, 16, 8, 12, 0), (3, 16, 8, 12, 3)):
        assert keep(shape=shape) == INVALID and b"multiples of p" in lib.ld_last_error(), shape
    cond = lambda lin=p, x=p, out=p, delta=None, shape=(3, 16, 8, 12, 2): lib.ld_unpatchify_cond(lin, x, out, delta, *shape, 1.0, 1.0,
                                                                                               1.0, None)
    for k in ("lin", "x", "out"):
        assert cond(**{k: None}) == INVALID and b"null" in lib.ld_last_error(), k
    for shape in ((3, 16, 7, 12, 2), (3, 16, 8, 11, 2), (3, 16, 8, 12, -2)):
        assert cond(shape=shape) == INVALID and b"multiples of p" in lib.ld_last_error(), shape
        assert cond(delta=p, shape=shape) == INVALID


def test_ops_wrappers_refuse_cpu_tensors_and_wrong_operands():
    from landiff_amd import _lib, ops
    x = torch.zeros(1, 2, 3, 4, 4)
    lin = torch.zeros(2, 8, 12, dtype=torch.bfloat16)
    with pytest.raises(_lib.LandiffHipError, match="GPU"):
        ops.unpatchify_cfg_keep(lin, x, torch.zeros_like(x), torch.zeros_like(x[0]), 2, 1.0, 1.0, 1.0, sums=torch.zeros(5),
                                workspace=torch.zeros(ops.DIT_GUIDANCE_WS_FLOATS))
    with pytest.raises(_lib.LandiffHipError, match="GPU"):
        ops.unpatchify_cond(lin[1], x, torch.zeros_like(x), 2, 1.0, 1.0)
    with pytest.raises(ValueError, match="one size"):
        ops.unpatchify_cond(lin[1], x, torch.zeros_like(x), 2, 1.0, 1.0, delta=torch.zeros(3))
    with pytest.raises(ValueError, match="one size"):
        ops.unpatchify_cfg_keep(lin, x, torch.zeros_like(x), torch.zeros(2, 3, 4, 4, dtype=torch.float64), 2, 1.0, 1.0, 1.0)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.unpatchify_cond(lin[1].float(), x, torch.zeros_like(x), 2, 1.0, 1.0)
    with pytest.raises(ValueError, match="lin_cond"):
        ops.unpatchify_cond(lin, x, torch.zeros_like(x), 2, 1.0, 1.0)
    with pytest.raises(ValueError, match="workspace"):
        ops.unpatchify_cfg_keep(lin, x, torch.zeros_like(x), torch.zeros_like(x[0]), 2, 1.0, 1.0, 1.0, sums=torch.zeros(5),
                                workspace=torch.zeros(8))


def test_runner_refuses_before_it_builds_anything():
    """The refusals of ControlDiTRunner(dit_guidance=...) come before any weight is touched: empty state dicts on the host do."""
    from landiff_amd.config import DiTConfig
    from landiff_amd.dit import ControlDiTRunner
    from landiff_amd.dit_cache import StepCacheConfig
    from landiff_amd.dit_guidance import GuidanceSkipConfig
    cpu, g, ts = torch.device("cpu"), GuidanceSkipConfig(refresh=2), [3, 2, 1]
    with pytest.raises(ValueError, match="step_cache.*B = 2"):
        ControlDiTRunner({}, {}, DiTConfig.tiny(), cpu, dit_guidance=g, step_cache=StepCacheConfig(0.1), plan_timesteps=ts)
    for fp8 in (True, "row", "mx"):
        with pytest.raises(ValueError, match="fp8_gemm.*batch-1"):
            ControlDiTRunner({}, {}, DiTConfig.tiny(), cpu, dit_guidance=g, fp8_gemm=fp8, plan_timesteps=ts)
    with pytest.raises(TypeError, match="GuidanceSkipConfig"):
        ControlDiTRunner({}, {}, DiTConfig.tiny(), cpu, dit_guidance=0.1, plan_timesteps=ts)


def test_signatures_of_the_public_layers():
    import inspect
    from landiff.diffusion.dif_infer import CogModelInferWrapper, CogWrapper
    from landiff_amd.dit import ControlDiTRunner
    from landiff_amd.pipeline import LanDiffPipeline
    for cls in (ControlDiTRunner, LanDiffPipeline, CogWrapper, CogModelInferWrapper):
        assert inspect.signature(cls.__init__).parameters["dit_guidance"].default is None, cls
    for cls in (LanDiffPipeline, CogModelInferWrapper):
        assert callable(cls.dit_guidance_report)


def test_cli_switches_refusal_and_report_file(monkeypatch, tmp_path, capsys):
    import landiff.infer_video as iv
    from landiff_amd.dit_guidance import REFUSE_STEP_CACHE, GuidanceSkipConfig
    assert iv.parse_args(["--prompt", "p"]).dit_guidance is None
    a = iv.parse_args(["--prompt", "p", "--dit_cfg_tol", "1e-5", "--dit_cfg_refresh", "3", "--dit_cfg_cos", "0.99", "--cfg", "7.0"])
    assert a.dit_guidance == GuidanceSkipConfig(scale_tolerance=1e-5, refresh=3, cos_threshold=0.99) and a.cfg == 7.0
    assert iv.parse_args(["--prompt", "p", "--dit_cfg_refresh", "2"]).dit_guidance == GuidanceSkipConfig(refresh=2)
    for bad in (["--dit_cfg_tol", "-1"], ["--dit_cfg_refresh", "0"], ["--dit_cfg_refresh", "1.5"], ["--dit_cfg_cos", "-1"], ["--dit_cfg_cos", "2"]):
        with pytest.raises(SystemExit):
            iv.parse_args(["--prompt", "p"] + bad)
    capsys.readouterr()
    for flags in (["--dit_cfg_tol", "0.01"], ["--dit_cfg_refresh", "2"], ["--dit_cfg_cos", "0.9"]):
        with pytest.raises(SystemExit):
            iv.parse_args(["--prompt", "p", "--dit_cache", "0.1"] + flags)
        assert REFUSE_STEP_CACHE in " ".join(capsys.readouterr().err.split())          # the runner's message
    seen = {}

    class FakeModel:
        def __init__(self, **kw):
            seen.update(kw)

        def __call__(self, task):
            task.result = "video"
            return task

        def dit_cache_report(self):
            return []

        def dit_guidance_report(self):
            return [dict(index=0, timestep=999, cfg_scale=1.5, mode="full", cos=math.nan, delta_rel_l1=None, delta_from=None),
                    dict(index=1, timestep=500, cfg_scale=1.2, mode="reuse", cos=None, delta_rel_l1=math.inf, delta_from=0)]

    monkeypatch.setattr(iv, "CogModelInferWrapper", FakeModel)
    monkeypatch.setattr(iv, "save_video_tensor", lambda *a, **k: None)
    stem = str(tmp_path / "out" / "v")
    iv.infer_diffusion(iv.parse_args(["--prompt", "p", "--dit_cfg_refresh", "2", "--attn_window", "1", "--save_file_name", stem]), None)
    assert seen["dit_guidance"] == GuidanceSkipConfig(refresh=2) and "dit_cache" not in seen and seen["attn_window"].frames == 1
    rows = json.load(open(stem + "_dit_guidance.json"))
    assert [r["mode"] for r in rows] == ["full", "reuse"] and rows[0]["cos"] is None and rows[1]["delta_rel_l1"] is None
    assert rows[1]["delta_from"] == 0 and rows[1]["cfg_scale"] == 1.2
    seen.clear()
    iv.infer_diffusion(iv.parse_args(["--prompt", "p", "--save_file_name", stem + "2"]), None)      # off: the call as it was
    assert seen == {"ckpt_path": "ckpts/LanDiff/diffusion"} and not os.path.exists(stem + "2_dit_guidance.json")


def test_report_json_writes_null_for_non_finite_values(tmp_path):
    from landiff_amd.dit_guidance import write_report_json
    path = str(tmp_path / "r.json")
    write_report_json(path, [[dict(index=0, cos=math.nan, delta_rel_l1=-math.inf, mode="full", cfg_scale=1.0)], [dict(cos=0.5)]])
    text = open(path).read()
    assert "NaN" not in text and "Infinity" not in text
    assert json.loads(text) == [[dict(index=0, cos=None, delta_rel_l1=None, mode="full", cfg_scale=1.0)], [dict(cos=0.5)]]


# the DiT's four linears at the cond-only step's M = 17776 (rows_per_batch = M: one batch).  (route, epilogue kind) as ld_gemm_route
# reports them: 6 = 8-phase rounds + half-tile tail, 7 = 8-phase rounds + 128x128 row tail, 2 = 8-phase alone, 0 = 128x128.  These
# are the values observed when the feature shipped: a retune that moves a B = 1 shape fails here (and tests/test_gpu_dit_guidance.py
# covers the routes by value).
B1_ROUTES = {"qkv": (6, 0), "dense": (6, 2), "h4": (6, 1), "h1": (7, 2)}


def b1_route(name):
    """(route, kind) of linear `name` at M = 17776 with the DiT's epilogue form (host call, no device memory is touched)."""
    from landiff_amd import _lib
    M, D, TEXT = 17776, 1920, 226
    N, K = {"qkv": (3 * D, D), "dense": (D, D), "h4": (4 * D, D), "h1": (D, 4 * D)}[name]
    bias = torch.zeros(N, dtype=torch.bfloat16)
    ada = torch.zeros(1, 12 * D, dtype=torch.bfloat16)
    buf = torch.zeros(2, N, dtype=torch.bfloat16)                   # stands for the [M, N] operands: their presence and row stride count
    gate = dict(gate=ada, gate_bstride=12 * D, rows_per_batch=M, text_len=TEXT)
    epi = {"qkv": dict(bias=bias), "dense": dict(bias=bias, resid=buf, gate_off_img=2 * D, gate_off_txt=8 * D, **gate),
           "h4": dict(bias=bias, act="gelu_tanh"),
           "h1": dict(bias=bias, resid=buf, add2=buf, gate_off_img=5 * D, gate_off_txt=11 * D, **gate)}[name]
    kind = ctypes.c_int32(-1)
    rc = _lib.load().ld_gemm_route(M, N, K, N, ctypes.byref(_host_epilogue(**epi)), ctypes.byref(kind))
    return rc, kind.value


def _host_epilogue(bias, act=None, resid=None, add2=None, gate=None, **scalars):
    """An ld_epilogue_t over host tensors, field by field (ops.make_epilogue insists on device pointers; ld_gemm_route reads which
    pointers are set and the strides, never what they point at)."""
    from landiff_amd import ops
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    e = ops.Epilogue()
    e.bias, e.act, e.mul, e.ldmul = ptr(bias), ops.ACT[act], None, 0
    e.resid, e.ldr, e.resid_f32 = ptr(resid), (resid.stride(-2) if resid is not None else 0), 0
    e.add2, e.ldadd, e.out_f32 = ptr(add2), (add2.stride(-2) if add2 is not None else 0), 0
    e.gate = ptr(gate)
    for k in ("gate_bstride", "gate_off_img", "gate_off_txt", "rows_per_batch", "text_len"):
        setattr(e, k, scalars.get(k, 0))
    return e


@pytest.mark.parametrize("name", list(B1_ROUTES))
def test_gemm_routes_of_the_cond_only_step(name):
    assert b1_route(name) == B1_ROUTES[name]
