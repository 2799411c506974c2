"""ld_attn_route: the attention launch's plan run dry (no GPU: nothing is launched).  The expectations restate the dispatch rule of
ld_attn_fwd_bf16 / _exact / _window on their own -- written from the launch code that preceded the plan, test by test in its
order, not from the plan:
  window form:  fewer than 6 key tiles -> refused (unsupported); else the q64 window kernels, whatever the knobs say;
  exact form:   unmasked and >= 6 key tiles -> the two-pass q64 kernel, decided before LD_ATTN_VARIANT / LD_ATTN_Q64;
  default form: LD_ATTN_VARIANT=0, unmasked, >= 6 key tiles -> q64, or p16 under LD_ATTN_Q64=0;
  everything else -> the plain kernel (LD_ATTN_VARIANT=8 too: the shipped library has no pipe2 kernel).
conftest.py sets LD_TUNING=1, so the knobs are re-read on every call.  The variants-only routes: tests/variants/variant_cases.py."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAIN, Q64, Q64_EXACT, Q64_WIN, P16 = 0, 1, 2, 3, 4
INVALID, UNSUPPORTED = -1, -3          # LD_ERR_INVALID / LD_ERR_UNSUPPORTED (landiff_amd/csrc/ld_common.h)
FORMS = ("default", "exact", "window")
KNOBS = ("LD_ATTN_VARIANT", "LD_ATTN_Q64", "LD_ATTN_Q128", "LD_ATTN_SAFE", "LD_ATTN_DYN", "LD_ATTN_MSUM", "LD_ATTN_NW", "LD_ATTN_NPRE")
PTR = ctypes.c_void_p(0x10000)         # never dereferenced: the launches below are refused before they touch the device


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _route(Nk, masked=False, form="default", B=1, H=2, Nq=None, Npad=None):
    from landiff_amd import _lib
    Nq = Nk if Nq is None else Nq
    Npad = (max(Nq, Nk) + 127) // 128 * 128 if Npad is None else Npad
    return _lib.load().ld_attn_route(B, H, Nq, Nk, Npad, int(masked), FORMS.index(form))


def _error():
    from landiff_amd import _lib
    return _lib.load().ld_last_error().decode()


@pytest.mark.parametrize("Nk,tiles", [(320, 5), (384, 6)])
@pytest.mark.parametrize("masked", [False, True])
def test_default_knobs(Nk, tiles, masked):
    pipelined = not masked and tiles >= 6
    assert _route(Nk, masked, "default") == (Q64 if pipelined else PLAIN)
    assert _route(Nk, masked, "exact") == (Q64_EXACT if pipelined else PLAIN)
    if masked:                                       # (there is no masked window launch to ask about)
        assert _route(Nk, masked, "window") == INVALID and "no masked" in _error()
    elif tiles >= 6:
        assert _route(Nk, masked, "window") == Q64_WIN
    else:
        assert _route(Nk, masked, "window") == UNSUPPORTED
        assert "5 key tiles" in _error() and "at least 6" in _error()


def test_ragged_last_tile_counts_and_rectangular_problems_go_by_the_keys():
    assert _route(321) == Q64 and _route(320) == PLAIN                       # 321 keys are 6 tiles
    assert _route(384, Nq=100) == Q64 and _route(320, Nq=1000) == PLAIN      # Nk decides, not Nq
    assert _route(384, Nq=100, form="window") == INVALID                     # the window form is square


def test_q64_knob(monkeypatch):
    monkeypatch.setenv("LD_ATTN_Q64", "0")
    assert _route(384) == P16
    assert _route(384, form="exact") == Q64_EXACT and _route(384, form="window") == Q64_WIN
    assert _route(320) == PLAIN and _route(384, masked=True) == PLAIN
    monkeypatch.setenv("LD_ATTN_Q64", "1")           # re-read per call
    assert _route(384) == Q64


@pytest.mark.parametrize("variant", ["9", "1", "4", "8"])        # 8: the pipe2 kernel exists in the variants build only
def test_variant_knob(monkeypatch, variant):
    from landiff_amd import _lib
    assert not _lib.has_variants()
    monkeypatch.setenv("LD_ATTN_VARIANT", variant)
    assert _route(384) == PLAIN and _route(320) == PLAIN and _route(384, masked=True) == PLAIN
    assert _route(384, form="exact") == Q64_EXACT and _route(384, form="window") == Q64_WIN
    monkeypatch.setenv("LD_ATTN_Q64", "0")
    assert _route(384) == PLAIN and _route(384, form="exact") == Q64_EXACT and _route(384, form="window") == Q64_WIN


def test_argument_errors_carry_the_launch_messages():
    """The shape errors of the entry points come back from the dry run with the messages the launch gives."""
    from landiff_amd import _lib
    lib = _lib.load()

    def launch(B, H, Nq, Nk, Npad, exact):
        fn = lib.ld_attn_fwd_bf16_exact if exact else lib.ld_attn_fwd_bf16
        return fn(PTR, PTR, PTR, PTR, B, H, Nq, Nk, Npad, Nq * 128, 128, 0.125, None, None, None, None, None), _error()

    for B, H, Nq, Nk, Npad, what in [(1, 2, 384, 384, 400, "multiple of 128"), (1, 2, 384, 500, 384, ">= Nq,Nk"), (1, 2, 500, 384, 384, ">= Nq,Nk"),
                                     (0, 2, 384, 384, 384, "empty problem"), (1, 0, 384, 384, 384, "empty problem"),
                                     (1, 2, 0, 384, 384, "empty problem"), (1, 2, 384, 0, 384, "empty problem")]:
        for form in ("default", "exact"):
            assert _route(Nk, False, form, B, H, Nq, Npad) == INVALID
            msg = _error()
            assert what in msg and msg.startswith("ld_attn_fwd_bf16:"), msg
            assert launch(B, H, Nq, Nk, Npad, form == "exact") == (INVALID, msg)
    # the window form: its launch's messages
    assert _route(384, form="window", Npad=400) == INVALID
    msg = _error()
    assert lib.ld_attn_fwd_bf16_window(PTR, PTR, PTR, PTR, 1, 2, 384, 400, 384 * 128, 128, 0.125, 0, 64, 6, None) == INVALID      # (window 6: every block walks all 6 tiles)
    assert _error() == msg and msg.startswith("ld_attn_fwd_bf16_window: Npad=400")
    assert _route(0, form="window", Npad=128) == INVALID and "N=0 outside" in _error()
    assert _route(384, form="window", B=0) == INVALID and "empty problem" in _error()
    assert lib.ld_attn_route(1, 2, 384, 384, 384, 0, 3) == INVALID and "form 3" in _error()


def test_ops_wrapper_and_the_python_side_constant():
    """ops.attn_route answers the same, raises on a refusal, and ops.ATTN_PIPELINED_MIN_TILES (attn_fwd's q_row0 guard,
    attn_window_check) is the library's constant: the smallest tile count at which the default unmasked route stops being plain."""
    from landiff_amd import _lib, ops
    assert ops.attn_route(1, 2, 384, 384, 384) == Q64 and ops.attn_route(1, 2, 384, 384, 384, form="exact") == Q64_EXACT
    assert ops.attn_route(1, 2, 384, 384, 384, masked=True) == PLAIN and ops.attn_route(1, 2, 384, 384, 384, form="window") == Q64_WIN
    with pytest.raises(_lib.LandiffHipError, match="at least 6"):
        ops.attn_route(1, 2, 320, 320, 384, form="window")
    routes = {n: _route(n * ops.ATTN_KEY_TILE) for n in range(1, 33)}
    assert min(n for n, r in routes.items() if r != PLAIN) == ops.ATTN_PIPELINED_MIN_TILES
    assert all(r == (PLAIN if n < ops.ATTN_PIPELINED_MIN_TILES else Q64) for n, r in routes.items())
    # ... and the window form's minimum is the same number
    assert [n for n in range(1, 33) if _route(n * ops.ATTN_KEY_TILE, form="window") == Q64_WIN][0] == ops.ATTN_PIPELINED_MIN_TILES


def test_vote_case_overflows_one_row_only():
    """The input of test_attention_vote_across_waves (tests/test_gpu_variants.py) does what that test needs: in every head the
    scaled row holds an exp2 exponent beyond 128 (its fast-pass denominator overflows fp32), every other row's exponents stay
    tiny (denominators far inside [2^-80, 2^110]), and the fp32 reference is finite.  The scaled row's top exponent leads the
    runner-up by more than 16: its softmax is one-hot beyond bf16, so the bf16 rounding of q * scale inside the kernels cannot
    move its output."""
    import torch
    import attn_vote_case as c
    q, k, v = c.inputs()
    s = c.log2_scores(q, k)
    top = s[:, :, c.ROW].topk(2, -1).values
    assert (top[..., 0] > 128).all(), top
    assert (top[..., 0] - top[..., 1] > 16).all(), top
    others = torch.cat([s[:, :, :c.ROW], s[:, :, c.ROW + 1:]], 2)
    assert others.abs().max().item() < 16
    assert torch.isfinite(c.reference(q, k, v)).all()
