"""Host side of token-sequence scoring (no GPU): candidate ranking, argument refusals of generate_samples / infer_video / the
ops wrappers, the _scores.json schema, the ABI, and a check that the kernel test's cases can tell a wrong kernel from a right one
(tests/llm_score_ref.py: the float64 restatement of lm_model.py:417-454 the GPU test compares ld_llm_token_logprobs with)."""
import ctypes
import json
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_rank_candidates_order_ties_and_non_finite():
    from landiff_amd.pipeline import rank_candidates
    assert rank_candidates([-30.0, -10.0, -20.0]) == [1, 2, 0]
    assert rank_candidates([-5.0, -5.0, -1.0, -5.0]) == [2, 0, 1, 3]                   # ties: the lower index first
    inf, nan = float("inf"), float("nan")
    assert rank_candidates([-inf, -3.0, nan, -2.0, -inf]) == [3, 1, 0, 2, 4]           # not finite: last, by index
    assert rank_candidates([nan, -inf]) == [0, 1]
    assert rank_candidates(torch.tensor([-2.5, -1.5])) == [1, 0]
    assert rank_candidates([]) == []


def test_generate_samples_refuses_bad_keep():
    """keep of 0 and keep > len(seeds) are refused before the LLM is touched (the pipeline object here has none)."""
    from landiff_amd.pipeline import LanDiffPipeline
    pipe = object.__new__(LanDiffPipeline)
    for keep in (0, 3, -1):
        with pytest.raises(ValueError, match="keep"):
            pipe.generate_samples(None, [5, 6], keep=keep)


def test_parse_args_keep():
    os.environ.setdefault("LANDIFF_SKIP_INIT", "1")
    from landiff.infer_video import parse_args
    a = parse_args(["--prompt", "x", "--num_samples", "4", "--keep", "2"])
    assert a.keep == 2 and a.num_samples == 4
    assert parse_args(["--prompt", "x", "--num_samples", "3", "--keep", "3"]).keep == 3
    assert parse_args(["--prompt", "x", "--num_samples", "3"]).keep is None
    for bad in (["--keep", "1"], ["--num_samples", "2", "--keep", "3"], ["--num_samples", "2", "--keep", "0"],
                ["--num_samples", "1", "--keep", "1"]):
        with pytest.raises(SystemExit):
            parse_args(["--prompt", "x"] + bad)


def test_scores_json_schema(tmp_path):
    from landiff_amd.pipeline import rank_candidates, write_scores_json
    seeds, scores = [42, 43, 44, 45], [-812.25, -790.5, float("-inf"), -801.0]
    kept = rank_candidates(scores)[:2]
    path = tmp_path / "video_scores.json"
    write_scores_json(str(path), seeds, scores, kept)
    rows = json.loads(path.read_text())
    assert rows == [{"index": 0, "seed": 42, "logprob": -812.25, "kept": False}, {"index": 1, "seed": 43, "logprob": -790.5, "kept": True},
                    {"index": 2, "seed": 44, "logprob": None, "kept": False}, {"index": 3, "seed": 45, "logprob": -801.0, "kept": True}]


def test_ops_wrappers_refuse_cpu_tensors_and_large_vocabularies():
    from landiff_amd import _lib, ops
    n, V = 2, 16
    cond, tgt, lp = torch.zeros(n, V), torch.zeros(n, dtype=torch.int64), torch.zeros(n)
    with pytest.raises(_lib.LandiffHipError, match="GPU tensors"):
        ops.llm_token_logprobs(cond, None, tgt, lp, False, 1.0, 1.0)
    with pytest.raises(_lib.LandiffHipError, match="GPU tensors"):
        ops.llm_head_f32(torch.zeros(2, 8), torch.zeros(4, 8), torch.zeros(2, 4))
    assert ops.LLM_SAMPLE_MAXV == 4096
    hdr = open(os.path.join(ROOT, "include", "landiff_hip.h")).read()
    assert int(re.search(r"#define LD_SAMPLE_MAXV (\d+)", hdr).group(1)) == ops.LLM_SAMPLE_MAXV
    # V > LD_SAMPLE_MAXV / K % 4 != 0: refused by the library itself.  Every pointer is NULL, so whichever check answers, nothing
    # can be launched (the size checks come first; a null pointer is refused too)
    lib = _lib.load()
    rc = lib.ld_llm_token_logprobs(None, 5000, None, 0, 1, 5000, 0, 1.0, 1.0, None, 0, 0, None, 0, None, 0, 0, -1.0, None, None, None, None, 0, None)
    assert rc != 0 and b"max 4096" in lib.ld_last_error()
    rc = lib.ld_llm_head_f32(None, 12, None, 12, None, 8, 4, 8, 10, None)
    assert rc != 0 and b"multiples of 4" in lib.ld_last_error()


def test_ops_token_logprobs_refuses_large_vocabulary_before_the_library(monkeypatch):
    """The wrapper's own check: V > LD_SAMPLE_MAXV raises ValueError (tensors faked as GPU ones: nothing is launched)."""
    from landiff_amd import ops
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else ctypes.c_void_p(16))
    n, V = 1, 4097
    with pytest.raises(ValueError, match="LD_SAMPLE_MAXV"):
        ops.llm_token_logprobs(torch.zeros(n, V), None, torch.zeros(n, dtype=torch.int64), torch.zeros(n), False, 1.0, 1.0)
    with pytest.raises(TypeError, match="float32"):
        ops.llm_token_logprobs(torch.zeros(n, 8, dtype=torch.float64), None, torch.zeros(n, dtype=torch.int64), torch.zeros(n), False, 1.0, 1.0)
    with pytest.raises(ValueError, match="contiguous rows"):
        ops.llm_head_f32(torch.zeros(8, 4).t(), torch.zeros(4, 8), torch.zeros(4, 4))


def test_abi_15_exports_both_entry_points():
    from landiff_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "landiff_hip.h")).read()
    assert lib.ld_version() == _lib.ABI_VERSION == int(re.search(r"#define LD_ABI_VERSION (\d+)", hdr).group(1)) >= 15      # (they came with 15)
    for name in ("ld_llm_token_logprobs", "ld_llm_head_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(rf"\bint {name}\(", hdr)


def test_kernel_cases_catch_wrong_kernels():
    """With logits drawn as 4 * N(0, 1), each of three wrong kernels moves at least one case of the GPU test by more than 1e-2
    (the asserted bound is below 1e-3): the table row of the wrong position, the temperature dropped, cond / uncond exchanged.
    A change of a value to or from -inf counts as a move."""
    import llm_score_ref as R
    cases = [c for c in R.all_cases() if c["n"] in (3, 5)]

    def moved(**wrong):
        worst = 0.0
        for c in cases:
            right, rv = R.ref_logprobs(c)
            got, gv = R.ref_logprobs(c, **wrong)
            if not torch.equal(torch.isinf(right), torch.isinf(got)) or not torch.equal(rv, gv):
                return math.inf
            fin = torch.isfinite(right)
            worst = max(worst, (right[fin] - got[fin]).abs().max().item() if fin.any() else 0.0)
        return worst

    for wrong in (dict(pos_shift=1), dict(pos_shift=-1), dict(drop_temperature=True), dict(swap_rows=True)):
        assert moved(**wrong) > 1e-2, wrong
    # the right kernel, stated twice, moves nothing
    assert moved() == 0.0


def test_reference_underflow_rows_are_finite():
    import llm_score_ref as R
    for V in (71, 2055):
        c = R.underflow_case(V)
        lp, valid = R.ref_logprobs(c)
        assert torch.isfinite(lp).all() and (lp < -195).all() and valid.tolist() == [1, 1]
        p32 = torch.softmax(c["cond"], -1)
        assert p32[0, c["target"][0]].item() == 0.0              # what an exp-domain kernel would take the logarithm of
