"""Host side of the frame-window attention (no GPU: nothing is launched): ld_attn_window_plan against a restatement of the rule,
the refusals of ld_attn_fwd_bf16_window before any HIP call, AttnWindowConfig, the CLI flags and the runner's refusals."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INVALID, UNSUPPORTED = -1, -3          # LD_ERR_INVALID / LD_ERR_UNSUPPORTED (landiff_amd/csrc/ld_common.h)
PTR = ctypes.c_void_p(0x10000)         # never dereferenced: every call below must return before it touches the device


def rule(N, P, G, w):
    """The rule, restated: per 256-row query block (t_lo, t_hi, n_eff); a block that holds a text row walks [0, n)."""
    n, pt = -(-N // 64), -(-P // 64)
    out = []
    for b in range(-(-N // 256)):
        r0 = 256 * b
        r1 = min(r0 + 256, N) - 1
        if r0 < P:
            out.append((pt, n, n))
            continue
        f_lo, f_hi = (r0 - P) // G, (r1 - P) // G
        k_lo, k_hi = P + max(0, f_lo - w) * G, min(N, P + (f_hi + w + 1) * G)
        t_lo, t_hi = max(pt, k_lo // 64), -(-k_hi // 64)
        out.append((t_lo, t_hi, pt + t_hi - t_lo))
    return out


def test_plan_agrees_with_the_rule():
    from landiff_amd import ops
    checked = 0
    for N in (1000, 1024, 1890, 2000, 2048, 2304, 385):                       # ragged and multiples of 256
        for P in (0, 1, 64, 90, 100, 128, 226, 256, 300):                      # none, on and off tile / block boundaries
            for G in (1, 60, 64, 125, 190, 200, 256, 320, 1350, 5000):         # on and off tile / block boundaries, one frame
                frames = -(-(N - P) // G)
                for w in (0, 1, 2, frames - 1, frames, frames + 5, 10 ** 9):
                    if w < 0:
                        continue
                    want = rule(N, P, G, w)
                    assert ops.attn_window_plan(N, P, G, w) == want, (N, P, G, w)
                    if w >= frames:                                             # the window covers every frame: every block walks [0, n)
                        n = -(-N // 64)
                        assert all(ne == n and hi == n for _, hi, ne in want), (N, P, G, w)
                    checked += 1
    assert checked > 3000
    # huge tokens-per-frame and window values neither overflow nor change the plan
    assert ops.attn_window_plan(17776, 226, 2 ** 40, 2 ** 40) == rule(17776, 226, 17776, 1)
    assert ops.attn_window_plan(2000, 2000, 7, 0) == rule(2000, 2000, 7, 0)      # all text


def test_plan_at_the_shipped_shape():
    from landiff_amd import ops
    N, P, G = 17776, 226, 1350
    sums = {w: sum(ne for _, _, ne in ops.attn_window_plan(N, P, G, w)) for w in (0, 1, 2, 3, 12)}
    assert sums == {0: 2319, 1: 4971, 2: 7391, 3: 9602, 12: 19460}
    assert len(ops.attn_window_plan(N, P, G, 1)) == 70 and 19460 == 70 * 278
    assert [ne for _, _, ne in ops.attn_window_plan(1890, 90, 200, 0)] == [30, 11, 9, 10, 10, 12, 9, 6]
    assert [ne for _, _, ne in ops.attn_window_plan(1890, 90, 200, 1)] == [30, 14, 16, 16, 16, 19, 12, 9]


def _fwd(lib, N, P, G, w, ptr=PTR):
    Npad = (N + 127) // 128 * 128
    return lib.ld_attn_fwd_bf16_window(ptr, ptr, ptr, ptr, 1, 2, N, Npad, N * 128, 128, 0.125, P, G, w, None)


def test_refusals_before_any_launch():
    from landiff_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "landiff_hip.h")).read()
    for name in ("ld_attn_fwd_bf16_window", "ld_attn_window_plan"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(rf"\bint {name}\(", hdr)
    for ptr in (PTR, None):                                                      # the window's own rules come first, pointers or not
        assert _fwd(lib, 300, 0, 10, 1, ptr) == UNSUPPORTED                      # n = 5 < 6
        assert b"at least 6" in lib.ld_last_error()
        assert _fwd(lib, 1000, 0, 60, 0, ptr) == UNSUPPORTED                     # a block with n_eff < 6
        assert b"query block" in lib.ld_last_error()
        assert _fwd(lib, 1000, 0, 60, -1, ptr) == INVALID                        # negative window
        assert _fwd(lib, 1000, 0, 0, 1, ptr) == INVALID                          # G = 0
        assert _fwd(lib, 1000, 1001, 60, 1, ptr) == INVALID                      # prefix past N
        assert _fwd(lib, 1000, -1, 60, 1, ptr) == INVALID
        assert _fwd(lib, 0, 0, 60, 1, ptr) == INVALID
    assert _fwd(lib, 1890, 90, 200, 1, None) == INVALID and b"null" in lib.ld_last_error()      # a legal window, no buffers
    assert lib.ld_attn_fwd_bf16_window(PTR, PTR, PTR, PTR, 1, 2, 1890, 1900, 1890 * 128, 128, 0.125, 90, 200, 1, None) == INVALID    # Npad % 128
    lo, hi, ne = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    ref = ctypes.byref
    assert lib.ld_attn_window_plan(1000, 0, 60, 0, 0, ref(lo), ref(hi), ref(ne)) == 0 and ne.value == 5     # unsupported shapes still plan
    assert lib.ld_attn_window_plan(1000, 0, 60, 0, 4, ref(lo), ref(hi), ref(ne)) == INVALID                 # block 4 of 4
    assert lib.ld_attn_window_plan(1000, 0, 60, -1, 0, ref(lo), ref(hi), ref(ne)) == INVALID
    assert lib.ld_attn_window_plan(1000, 0, 0, 1, 0, ref(lo), ref(hi), ref(ne)) == INVALID
    assert lib.ld_attn_window_plan(1000, 0, 60, 1, 0, None, ref(hi), ref(ne)) == INVALID


def test_ops_window_check_names_the_reason():
    from landiff_amd import ops
    assert ops.attn_window_check(1890, 90, 200, 1) == rule(1890, 90, 200, 1)
    with pytest.raises(ValueError, match="at least 6 key tiles"):
        ops.attn_window_check(300, 0, 10, 1)
    with pytest.raises(ValueError, match="query block 0 would walk 5"):
        ops.attn_window_check(1000, 0, 60, 0)


def test_as_config():
    from landiff_amd.config import AttnWindowConfig
    as_config = AttnWindowConfig.as_config
    assert as_config(None) is None
    assert as_config(2) == AttnWindowConfig(frames=2, dense_steps=0)
    assert as_config(0) == AttnWindowConfig(frames=0)
    c = AttnWindowConfig(frames=1, dense_steps=3)
    assert as_config(c) is c
    for bad in (True, 1.5, "2", [1]):
        with pytest.raises(TypeError):
            as_config(bad)
    for kw in (dict(frames=-1), dict(frames=1, dense_steps=-1), dict(frames=1.0), dict(frames=True), dict(frames=1, dense_steps=0.5)):
        with pytest.raises(ValueError):
            AttnWindowConfig(**kw)
    with pytest.raises(Exception):
        c.frames = 2                                                             # frozen


def test_cli_attn_window_switch(monkeypatch, tmp_path):
    import landiff.infer_video as iv
    from landiff_amd.config import AttnWindowConfig
    a = iv.parse_args(["--prompt", "p"])
    assert a.attn_window is None and a.attn_window_dense_steps == 0
    a = iv.parse_args(["--prompt", "p", "--attn_window", "2", "--attn_window_dense_steps", "5"])
    assert a.attn_window == 2 and a.attn_window_dense_steps == 5
    assert iv.parse_args(["--prompt", "p", "--attn_window", "0"]).attn_window == 0
    for bad in (["--attn_window", "-1"], ["--attn_window", "x"], ["--attn_window", "1.5"], ["--attn_window_dense_steps", "2"],
                ["--attn_window", "1", "--attn_window_dense_steps", "-1"]):
        with pytest.raises(SystemExit):
            iv.parse_args(["--prompt", "p"] + bad)
    seen = {}

    class FakeModel:
        def __init__(self, **kw):
            seen.update(kw)

        def __call__(self, task):
            task.result = "video"
            return task

        def dit_cache_report(self):
            return []

    monkeypatch.setattr(iv, "CogModelInferWrapper", FakeModel)
    monkeypatch.setattr(iv, "save_video_tensor", lambda *a, **k: None)
    stem = str(tmp_path / "v")
    iv.infer_diffusion(iv.parse_args(["--prompt", "p", "--attn_window", "1", "--attn_window_dense_steps", "4", "--save_file_name", stem]), None)
    assert seen == {"ckpt_path": "ckpts/LanDiff/diffusion", "attn_window": AttnWindowConfig(frames=1, dense_steps=4)}
    seen.clear()
    iv.infer_diffusion(iv.parse_args(["--prompt", "p", "--attn_window", "3", "--dit_cache", "0.1", "--save_file_name", stem]), None)
    assert seen == {"ckpt_path": "ckpts/LanDiff/diffusion", "dit_cache": 0.1, "attn_window": AttnWindowConfig(frames=3)}
    seen.clear()
    iv.infer_diffusion(iv.parse_args(["--prompt", "p", "--save_file_name", stem]), None)                  # off: the call as it was
    assert seen == {"ckpt_path": "ckpts/LanDiff/diffusion"}


def test_runner_refuses_before_it_builds_anything():
    """The refusals of ControlDiTRunner(attn_window=...) come before any weight is touched: empty state dicts on the host do."""
    from landiff_amd.config import DiTConfig
    from landiff_amd.dit import ControlDiTRunner
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="attn_exact"):
        ControlDiTRunner({}, {}, DiTConfig.config0(), cpu, attn_exact=True, attn_window=1)
    with pytest.raises(ValueError, match="does not fit this DiT shape.*key tiles"):
        ControlDiTRunner({}, {}, DiTConfig.tiny(), cpu, attn_window=1)              # 2 key tiles
    with pytest.raises(TypeError):
        ControlDiTRunner({}, {}, DiTConfig.config0(), cpu, attn_window=1.5)
    with pytest.raises(ValueError):
        ControlDiTRunner({}, {}, DiTConfig.config0(), cpu, attn_window=-1)


def test_signatures_of_the_public_layers():
    import inspect
    from landiff.diffusion.dif_infer import CogModelInferWrapper, CogWrapper
    from landiff_amd.dit import ControlDiTRunner
    from landiff_amd.pipeline import LanDiffPipeline
    for cls in (ControlDiTRunner, LanDiffPipeline, CogWrapper, CogModelInferWrapper):
        assert inspect.signature(cls.__init__).parameters["attn_window"].default is None, cls
