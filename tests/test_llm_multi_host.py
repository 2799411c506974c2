"""Host-side checks of the batched AR decode (no GPU): the _pairs entry points refuse what they do not support before anything
is launched, the CLI's --num_samples parses, sample_many refuses the forms it does not have."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INVALID, UNSUPPORTED = -1, -3          # LD_ERR_INVALID / LD_ERR_UNSUPPORTED (landiff_amd/csrc/ld_common.h)
PTR = ctypes.c_void_p(0x10000)         # never dereferenced: every call below must return before it touches the device


def _gemv_pairs(lib, B, x=PTR, w=PTR, out=PTR, K=2048):
    return lib.ld_gemv_pairs(x, K, 0, w, None, 0, None, None, 0, out, 2048, 0, B, 2048, K, 0, 0, None, 0.0, None)


def test_gemv_pairs_refuses_bad_arguments():
    from landiff_amd import _lib
    lib = _lib.load()
    for B in (1, 3, 5, 7, 0, -2):
        assert _gemv_pairs(lib, B) == INVALID, B
    assert b"pairs" in lib.ld_last_error()
    for B in (10, 12, 64):
        assert _gemv_pairs(lib, B) == UNSUPPORTED, B
    assert _gemv_pairs(lib, 4, x=None) == INVALID and _gemv_pairs(lib, 4, w=None) == INVALID and _gemv_pairs(lib, 4, out=None) == INVALID
    assert _gemv_pairs(lib, 4, K=2044) == INVALID


def _forward_pairs(lib, B, null=None, table=True):
    from landiff_amd import _lib
    layers = (_lib.LlmLayer * 2)()
    for layer in layers:
        for name, _ in _lib.LlmLayer._fields_:
            setattr(layer, name, 0x10000)
    # layers, n, emb, token, pos, pos_value, x, qkv, att, gate, attn_ws, cos, sin, lnf_w, lnf_b, lnf_out, head, logits
    ptrs = {k: PTR for k in ("token", "pos", "x", "qkv", "att", "gate", "attn_ws", "cos", "sin", "lnf_w", "lnf_b", "lnf_out", "head", "logits")}
    if null:
        ptrs[null] = None
    return lib.ld_llm_decode_forward_pairs(ctypes.addressof(layers) if table else None, 2, PTR, ptrs["token"], ptrs["pos"], 5, ptrs["x"], ptrs["qkv"],
                                           ptrs["att"], ptrs["gate"], ptrs["attn_ws"], ptrs["cos"], ptrs["sin"], ptrs["lnf_w"],
                                           ptrs["lnf_b"], ptrs["lnf_out"], ptrs["head"], ptrs["logits"], B, 2048, 16, 11008, 2055, 1024, 8,
                                           1e-5, 1e-5, None)


def test_decode_forward_pairs_refuses_bad_arguments():
    from landiff_amd import _lib
    lib = _lib.load()
    for B in (1, 3, 7):
        assert _forward_pairs(lib, B) == INVALID, B
    for B in (10, 16):
        assert _forward_pairs(lib, B) == UNSUPPORTED, B
    for name in ("token", "pos", "x", "qkv", "att", "gate", "attn_ws", "cos", "sin", "lnf_w", "lnf_b", "lnf_out", "head", "logits"):
        assert _forward_pairs(lib, 4, null=name) == INVALID, name
    assert _forward_pairs(lib, 4, table=False) == INVALID


def _sample_pairs(lib, P, null=None):
    a = {k: PTR for k in ("logits", "pos", "noise", "forced", "token", "out_tokens", "out_count", "emb", "x")}
    if null:
        a[null] = None
    return lib.ld_llm_sample_advance_pairs(a["logits"], None, None, 2055, 1, 7.5, 1.0, a["pos"], None, 0, 0, -1.0, a["noise"], a["forced"],
                                           a["token"], a["out_tokens"], 64, a["out_count"], None, a["emb"], a["x"], P, 256, None)


def test_sample_advance_pairs_refuses_bad_arguments():
    from landiff_amd import _lib
    lib = _lib.load()
    assert _sample_pairs(lib, 0) == INVALID
    for P in (5, 8):
        assert _sample_pairs(lib, P) == UNSUPPORTED, P
    for name in ("logits", "pos", "noise", "forced", "token", "out_tokens", "out_count", "emb", "x"):
        assert _sample_pairs(lib, 3, null=name) == INVALID, name


def test_num_samples_parses():
    from landiff.infer_video import parse_args, sample_names
    a = parse_args(["--prompt", "a cat"])
    assert a.num_samples == 1 and sample_names(a) == [(42, "results/video")]                  # N = 1: the names of today
    a = parse_args(["--prompt", "a cat", "--num_samples", "3", "--seed", "7", "--save_file_name", "out/v"])
    assert a.num_samples == 3 and sample_names(a) == [(7, "out/v_0"), (8, "out/v_1"), (9, "out/v_2")]
    for bad in (["--num_samples", "0"], ["--num_samples", "5"], ["--num_samples", "2", "--seed", "-1"],
                ["--num_samples", "2", "--extend_video", "clip.npy"]):
        with pytest.raises(SystemExit):
            parse_args(["--prompt", "a cat"] + bad)


def test_sample_many_refuses_unsupported_forms():
    from landiff_amd.config import LLMConfig
    from landiff_amd.llm import LLMRunner
    from landiff_amd.weights import init_state, llm_spec
    cfg = LLMConfig.tiny()
    cpu = torch.device("cpu")            # the refusals come before any kernel: a runner holding host tensors is enough
    run = LLMRunner(init_state(llm_spec(cfg), 21, dtype=torch.bfloat16, device=cpu), cfg, cpu, max_text=16, max_frames=3, max_samples=2)
    text = torch.zeros(4, cfg.text_dim)
    for kw in (dict(mode="fused"), dict(mode="chained"), dict(use_graph=True), dict(teacher_fed=torch.zeros(3, dtype=torch.int64))):
        with pytest.raises(ValueError, match="not supported"):
            run.sample_many(text, [1, 2], num_frames=3, **kw)
    with pytest.raises(ValueError, match="max_samples"):
        run.sample_many(text, [1, 2, 3], num_frames=3)
    with pytest.raises(ValueError, match="non-zero"):
        run.sample_many(text, [1, 0], num_frames=3)
    with pytest.raises(AssertionError):
        LLMRunner({}, cfg, cpu, max_samples=5)
