"""Host-side checks of the MFMA engine of the batched AR decode (no GPU): the _wide entry points refuse what they do not support
before anything is launched, the _pairs caps are where they were, the CLI's --decode_engine parses, sample_many(engine="mfma")
refuses the forms it does not have."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INVALID, UNSUPPORTED = -1, -3          # LD_ERR_INVALID / LD_ERR_UNSUPPORTED (landiff_amd/csrc/ld_common.h)
PTR = ctypes.c_void_p(0x10000)         # never dereferenced: every call below must return before it touches the device


def _gemv(fn, B, x=PTR, w=PTR, out=PTR, K=2048, w_f32=0):
    return fn(x, K, 0, w, None, w_f32, None, None, 0, out, 2048, 0, B, 2048, K, 0, 0, None, 0.0, None)


def test_gemv_wide_refuses_bad_arguments():
    from landiff_amd import _lib, ops
    lib = _lib.load()
    assert ops.LLM_MAX_WIDE == 16 and ops.LLM_MAX_PAIRS == 4
    for B in (1, 3, 17, 31, 0, -2):
        assert _gemv(lib.ld_gemv_wide, B) == INVALID, B
    assert b"pairs" in lib.ld_last_error()
    for B in (34, 36, 64):
        assert _gemv(lib.ld_gemv_wide, B) == UNSUPPORTED, B
    assert _gemv(lib.ld_gemv_wide, 32, K=2056) == UNSUPPORTED                  # a multiple of 8, not of one MFMA step
    assert b"16" in lib.ld_last_error()
    assert _gemv(lib.ld_gemv_wide, 32, w_f32=1) == UNSUPPORTED                 # fp32 weights (the head) are not this kernel's
    for null in ("x", "w", "out"):
        assert _gemv(lib.ld_gemv_wide, 32, **{null: None}) == INVALID, null
    # the GEMV engine's cap has not moved
    assert _gemv(lib.ld_gemv_pairs, 10) == UNSUPPORTED


def _forward_wide(lib, B, null=None, table=True, mlp=11008):
    from landiff_amd import _lib
    layers = (_lib.LlmLayer * 2)()
    for layer in layers:
        for name, _ in _lib.LlmLayer._fields_:
            setattr(layer, name, 0x10000)
    ptrs = {k: PTR for k in ("token", "pos", "x", "qkv", "att", "gate", "attn_ws", "cos", "sin", "lnf_w", "lnf_b", "lnf_out", "head", "logits")}
    if null:
        ptrs[null] = None
    return lib.ld_llm_decode_forward_wide(ctypes.addressof(layers) if table else None, 2, PTR, ptrs["token"], ptrs["pos"], 5, ptrs["x"], ptrs["qkv"],
                                          ptrs["att"], ptrs["gate"], ptrs["attn_ws"], ptrs["cos"], ptrs["sin"], ptrs["lnf_w"],
                                          ptrs["lnf_b"], ptrs["lnf_out"], ptrs["head"], ptrs["logits"], B, 2048, 16, mlp, 2055, 1024, 8,
                                          1e-5, 1e-5, None)


def test_decode_forward_wide_refuses_bad_arguments():
    from landiff_amd import _lib
    lib = _lib.load()
    for B in (1, 3, 33):
        assert _forward_wide(lib, B) == INVALID, B
    for B in (34, 64):                                                          # P = 17, 32
        assert _forward_wide(lib, B) == UNSUPPORTED, B
    assert _forward_wide(lib, 32, mlp=11016) == UNSUPPORTED                     # K of the down projection: % 8 but not % 16
    for name in ("token", "pos", "x", "qkv", "att", "gate", "attn_ws", "cos", "sin", "lnf_w", "lnf_b", "lnf_out", "head", "logits"):
        assert _forward_wide(lib, 32, null=name) == INVALID, name
    assert _forward_wide(lib, 32, table=False) == INVALID


def _sample_wide(lib, P, null=None):
    a = {k: PTR for k in ("logits", "pos", "noise", "forced", "token", "out_tokens", "out_count", "emb", "x")}
    if null:
        a[null] = None
    return lib.ld_llm_sample_advance_wide(a["logits"], None, None, 2055, 1, 7.5, 1.0, a["pos"], None, 0, 0, -1.0, a["noise"], a["forced"],
                                          a["token"], a["out_tokens"], 64, a["out_count"], None, a["emb"], a["x"], P, 256, None)


def test_sample_advance_wide_refuses_bad_arguments():
    from landiff_amd import _lib
    lib = _lib.load()
    assert _sample_wide(lib, 0) == INVALID
    for P in (17, 32):
        assert _sample_wide(lib, P) == UNSUPPORTED, P
    for name in ("logits", "pos", "noise", "forced", "token", "out_tokens", "out_count", "emb", "x"):
        assert _sample_wide(lib, 16, null=name) == INVALID, name


def test_decode_engine_parses():
    from landiff.infer_video import parse_args, sample_names
    a = parse_args(["--prompt", "a cat"])
    assert a.decode_engine == "gemv" and a.num_samples == 1
    a = parse_args(["--prompt", "a cat", "--num_samples", "16", "--decode_engine", "mfma", "--seed", "7", "--save_file_name", "out/v"])
    names = sample_names(a)
    assert a.decode_engine == "mfma" and len(names) == 16 and names[0] == (7, "out/v_0") and names[15] == (22, "out/v_15")
    a = parse_args(["--prompt", "a cat", "--num_samples", "3", "--decode_engine", "mfma", "--keep", "2"])
    assert a.num_samples == 3 and a.keep == 2
    for bad in (["--num_samples", "17", "--decode_engine", "mfma"], ["--num_samples", "5"], ["--num_samples", "5", "--decode_engine", "gemv"],
                ["--decode_engine", "lds"], ["--num_samples", "0", "--decode_engine", "mfma"]):
        with pytest.raises(SystemExit):
            parse_args(["--prompt", "a cat"] + bad)


def test_sample_many_mfma_refuses_unsupported_forms():
    from landiff_amd.config import LLMConfig
    from landiff_amd.llm import LLMRunner
    from landiff_amd.weights import init_state, llm_spec
    cfg = LLMConfig.tiny()
    cpu = torch.device("cpu")            # the refusals come before any kernel: a runner holding host tensors is enough
    run = LLMRunner(init_state(llm_spec(cfg), 21, dtype=torch.bfloat16, device=cpu), cfg, cpu, max_text=16, max_frames=3, wide_samples=2)
    assert run.max_samples == 1 and run.wide_samples == 2 and run.kc_all[0].shape[0] == 4
    text = torch.zeros(4, cfg.text_dim)
    with pytest.raises(ValueError, match="wide_samples"):
        run.sample_many(text, [1, 2, 3], num_frames=3, engine="mfma")
    with pytest.raises(ValueError, match="not supported"):
        run.sample_many(text, [1, 2], num_frames=3, engine="mfma", use_graph=True)
    with pytest.raises(ValueError, match="not supported"):
        run.sample_many(text, [1, 2], num_frames=3, engine="mfma", mode="fused")
    with pytest.raises(ValueError, match="unknown engine"):
        run.sample_many(text, [1, 2], num_frames=3, engine="wmma")
    with pytest.raises(ValueError, match="non-zero"):
        run.sample_many(text, [1, 0], num_frames=3, engine="mfma")
    with pytest.raises(ValueError, match="max_samples"):                         # the GEMV engine's limit is max_samples, as before
        run.sample_many(text, [1, 2], num_frames=3)
    with pytest.raises(AssertionError):
        LLMRunner({}, cfg, cpu, wide_samples=17)
    with pytest.raises(AssertionError):
        LLMRunner({}, cfg, cpu, wide_samples=-1)
