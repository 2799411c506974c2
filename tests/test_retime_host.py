"""Host-side checks of the retime stage (no GPU): the plan's rational arithmetic on hand-checked cases, every refusal, the entry
point in header / library / SIGNATURES with its refusals before any launch, the wrapper's host checks, the command line's flag, and
the numpy restatement of the frame rule (retime_ref) against the four properties the rule must have."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import retime_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 45, 70                                   # partial blocks on both axes: 6 x 9 blocks
PHASES = [(1, 2), (1, 3), (2, 3), (4, 15)]
SHIFT = (6, -4)


def test_plan_arithmetic():
    from landiff_amd.retime import RetimeConfig, RetimePlan, retime_plan
    p = retime_plan(49, RetimeConfig(out_fps=24))
    assert isinstance(p, RetimePlan) and (p.q, p.n_out) == (3, 145)
    assert p.src_idx == tuple(k // 3 for k in range(145)) and p.phase_p == tuple(k % 3 for k in range(145))
    assert p.src_idx[-1] == 48 and p.phase_p[-1] == 0 and p.out_fps == Fraction(24) and p.src_fps == Fraction(8)
    assert (p.search, p.penalty, p.max_sad) == (8, 4, 24)
    p = retime_plan(49, RetimeConfig(out_fps=30))
    assert (p.q, p.n_out) == (15, 181)                                            # 8 / 30 = 4 / 15
    assert p.src_idx[:5] == (0, 0, 0, 0, 1) and p.phase_p[:5] == (0, 4, 8, 12, 1) and (p.src_idx[-1], p.phase_p[-1]) == (48, 0)
    assert all(15 * i + ph == 4 * k for k, (i, ph) in enumerate(zip(p.src_idx, p.phase_p)))
    p = retime_plan(49, RetimeConfig(out_fps=8))
    assert p.q == 1 and p.n_out == 49 and p.src_idx == tuple(range(49)) and not any(p.phase_p)
    p = retime_plan(49, RetimeConfig(out_fps=4))
    assert p.q == 1 and p.n_out == 25 and p.src_idx == tuple(2 * k for k in range(25)) and not any(p.phase_p)
    p = retime_plan(49, RetimeConfig(out_fps="30000/1001"))
    assert p.q == 3750 and p.n_out == (48 * 3750) // 1001 + 1 == 180                # 8 * 1001 / 30000 = 1001 / 3750
    assert p.src_idx[-1] + (p.phase_p[-1] > 0) <= 48 and (p.src_idx[1], p.phase_p[1]) == (0, 1001)
    assert retime_plan(49, RetimeConfig(out_fps=Fraction(30000, 1001))).phase_p == p.phase_p
    assert retime_plan(49, RetimeConfig(out_fps=12.5)).q == 25                        # the float's shortest decimal: 8 / 12.5 = 16 / 25
    for fps in (24, 30, 4, "30000/1001", 0.5, 1000):
        one = retime_plan(1, RetimeConfig(out_fps=fps))
        assert one.n_out == 1 and one.src_idx == (0,) and one.phase_p == (0,)
    # another source rate: 25 -> 50 fps doubles; every plan stays inside the clip
    p = retime_plan(10, RetimeConfig(out_fps=50, search=3, penalty=0, max_sad=255), src_fps=25)
    assert (p.q, p.n_out, p.src_idx[-1], p.phase_p[-1]) == (2, 19, 9, 0) and (p.search, p.penalty, p.max_sad) == (3, 0, 255)
    for F in (2, 3, 7, 49):
        for fps in (3, 7, 9, 24, 30, 60, "24000/1001"):
            p = retime_plan(F, RetimeConfig(out_fps=fps))
            assert len(p.src_idx) == len(p.phase_p) == p.n_out
            assert all(0 <= ph < p.q and 0 <= i and i + (ph > 0) <= F - 1 for i, ph in zip(p.src_idx, p.phase_p))
    d = retime_plan(5, RetimeConfig(out_fps=24)).as_dict()
    import json
    assert json.loads(json.dumps(d, allow_nan=False)) == d
    assert d["q"] == 3 and d["n_out"] == 13 and d["out_fps"] == 24.0 and d["src_idx"] == [k // 3 for k in range(13)]
    assert d["phase_p"] == [k % 3 for k in range(13)] and (d["search"], d["penalty"], d["max_sad"]) == (8, 4, 24)


def test_plan_refusals_name_the_value():
    from landiff_amd.retime import RetimeConfig, retime_plan
    for kw, msg in ((dict(out_fps=0), "out_fps must be positive, got 0"), (dict(out_fps=-24), "got -24"),
                    (dict(out_fps="-30000/1001"), "-30000/1001"), (dict(out_fps="fast"), "'fast'"),
                    (dict(out_fps=24, search=33), "search must be an integer in 0..32, got 33"),
                    (dict(out_fps=24, search=-1), "search must be an integer in 0..32, got -1"),
                    (dict(out_fps=24, penalty=256), "penalty must be an integer in 0..255, got 256"),
                    (dict(out_fps=24, penalty=-1), "got -1"), (dict(out_fps=24, max_sad=256), "max_sad must be an integer in 0..255, got 256"),
                    (dict(out_fps=24, max_sad=-2), "got -2"), (dict(out_fps=24, search=2.5), "got 2.5")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            retime_plan(49, RetimeConfig(**kw))
    with pytest.raises(ValueError, match="q = 65537 exceeds 65535"):
        retime_plan(49, RetimeConfig(out_fps=65537))
    assert retime_plan(2, RetimeConfig(out_fps=65535)).q == 65535                    # the largest q taken
    for F in (0, -3):
        with pytest.raises(ValueError, match=f"at least 1 frame, got {F}"):
            retime_plan(F, RetimeConfig(out_fps=24))
    with pytest.raises(ValueError, match="src_fps must be positive, got 0"):
        retime_plan(49, RetimeConfig(out_fps=24), src_fps=0)


def test_entry_point_in_header_library_and_signatures():
    from landiff_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "landiff_hip.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    decl = re.search(r"\bint ld_retime_u8\(([^;]*)\);", hdr)
    assert decl and len(decl.group(1).split(",")) == 16 == len(_lib.SIGNATURES["ld_retime_u8"])
    assert re.search(r" T ld_retime_u8\b", syms)
    assert _lib.load().ld_version() == _lib.ABI_VERSION == int(re.search(r"#define LD_ABI_VERSION (\d+)", hdr).group(1))


def test_refusals_before_any_launch():
    """Every LD_REQUIRE of ld_retime_u8 answers before a launch: safe without a GPU."""
    from landiff_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)

    def retime(src=p, dst=p, idx=p, ph=p, q=3, mv=None, sad=None, F=2, n=4, H=10, W=12, C=3, search=8, penalty=4, max_sad=24):
        return lib.ld_retime_u8(src, dst, idx, ph, q, mv, sad, F, n, H, W, C, search, penalty, max_sad, None)

    for kw, msg in ((dict(src=None), b"null pointer"), (dict(dst=None), b"null pointer"), (dict(idx=None), b"null pointer"),
                    (dict(ph=None), b"null pointer"), (dict(C=2), b"C must be 1 or 3, got 2"), (dict(C=4), b"C must be 1 or 3, got 4"),
                    (dict(F=0), b"empty shape"), (dict(n=0), b"empty shape"), (dict(H=0), b"empty shape"), (dict(W=-1), b"empty shape"),
                    (dict(search=33), b"search must be in 0..32, got 33"), (dict(search=-1), b"search must be in 0..32, got -1"),
                    (dict(penalty=256), b"penalty must be in 0..255, got 256"), (dict(penalty=-1), b"penalty must be in 0..255, got -1"),
                    (dict(max_sad=256), b"max_sad must be in 0..255, got 256"), (dict(max_sad=-1), b"max_sad must be in 0..255, got -1"),
                    (dict(q=0), b"q must be in 1..65535, got 0"), (dict(q=65536), b"q must be in 1..65535, got 65536")):
        assert retime(**kw) == -1, kw
        err = lib.ld_last_error()
        assert b"ld_retime_u8:" in err and msg in err, (kw, err)


def test_wrapper_checks_its_arguments_on_the_host():
    """ops.retime_u8 refuses bad arguments -- the two tables' ranges among them -- before anything is uploaded."""
    from landiff_amd import _lib, ops
    x = torch.zeros(3, 10, 12, 3, dtype=torch.uint8)
    ok = dict(src_idx=[0, 0, 1, 2], phase_p=[0, 1, 1, 0], q=2, search=2, penalty=4, max_sad=24)
    for kw, exc, msg in ((dict(phase_p=[0, 2, 1, 0]), ValueError, r"phase_p\[1\] = 2 is not in \[0, 2\)"),
                         (dict(phase_p=[0, -1, 1, 0]), ValueError, r"phase_p\[1\] = -1"),
                         (dict(src_idx=[0, 0, 1, 3]), ValueError, "output frame 3 at source position 3 .* leaves the clip's 3 frames"),
                         (dict(phase_p=[0, 1, 1, 1]), ValueError, r"output frame 3 at source position 2 \+ 1/2 leaves"),
                         (dict(src_idx=[-1, 0, 1, 2]), ValueError, "output frame 0"),
                         (dict(src_idx=[0, 1]), ValueError, "one length"), (dict(src_idx=[], phase_p=[]), ValueError, "non-empty"),
                         (dict(q=0), ValueError, "q must be"), (dict(q=65536), ValueError, "q must be"),
                         (dict(search=33), ValueError, "search must be"), (dict(penalty=256), ValueError, "penalty must be"),
                         (dict(max_sad=-1), ValueError, "max_sad must be")):
        with pytest.raises(exc, match=msg):
            ops.retime_u8(x, **{**ok, **kw})
    with pytest.raises(TypeError, match="uint8"):
        ops.retime_u8(x.float(), **ok)
    with pytest.raises(ValueError, match="C 1 or 3"):
        ops.retime_u8(x[..., :2].contiguous(), **ok)
    with pytest.raises(ValueError, match="contiguous"):
        ops.retime_u8(x[:, :, ::2], **ok)
    with pytest.raises(_lib.LandiffHipError, match="GPU tensors"):                   # valid arguments, host tensors: no CPU fallback
        ops.retime_u8(x, **ok)
    from landiff_amd.retime import motion_profile, retime_clip
    with pytest.raises(ValueError, match="no frame pair"):
        motion_profile(x[:1])
    with pytest.raises(ValueError, match="search must be"):
        motion_profile(x, search=40)
    with pytest.raises(TypeError, match="RetimeConfig or a RetimePlan"):
        retime_clip(x, 24)


def test_parse_args_out_fps(capsys):
    import landiff.infer_video as iv
    base = ["--prompt", "p"]
    a = iv.parse_args(base)
    assert a.out_fps is None and a.out_search is None and a.retime is None
    a = iv.parse_args(base + ["--out_fps", "24"])
    assert a.out_fps == 24 and (a.retime.out_fps, a.retime.search, a.retime.penalty, a.retime.max_sad) == (24, 8, 4, 24)
    assert iv.parse_args(base + ["--out_fps", "30", "--out_search", "16"]).retime.search == 16
    for bad, msg in ((["--out_fps", "0"], "--out_fps takes an integer >= 1"), (["--out_fps", "-8"], "--out_fps takes an integer >= 1"),
                     (["--out_fps", "29.97"], "invalid int value"), (["--out_search", "4"], "--out_search goes with --out_fps"),
                     (["--out_fps", "24", "--out_search", "33"], "search must be an integer in 0..32")):
        with pytest.raises(SystemExit):
            iv.parse_args(base + bad)
        assert msg in capsys.readouterr().err, bad


# ---- the restatement itself: the four properties of the rule, on a 45 x 70 x 3 frame with R = 8 ----
def _interior(shift):
    """Blocks whose windows, moved by up to `shift`, stay inside the frame (nothing is clamped there)."""
    my, mx = abs(shift[0]), abs(shift[1])
    bys = [b for b in range(-(-H // 8)) if 8 * b - 4 - my >= 0 and 8 * b + 11 + my <= H - 1]
    bxs = [b for b in range(-(-W // 8)) if 8 * b - 4 - mx >= 0 and 8 * b + 11 + mx <= W - 1]
    assert bys and bxs
    return bys, bxs


def test_rhu_and_split():
    assert [int(ref.rhu(n, 2)) for n in (-3, -2, -1, 0, 1, 2, 3)] == [-1, -1, 0, 0, 1, 1, 2]      # halves go up: -1.5 -> -1, 0.5 -> 1
    assert [int(ref.rhu(n, 3)) for n in (-4, -2, -1, 1, 2, 4)] == [-1, -1, 0, 0, 1, 1]
    for p, q in PHASES + [(1, 65535), (65534, 65535)]:
        for d in range(-32, 33):
            a, b = (int(v) for v in ref.split(d, p, q))
            assert b - a == d and abs(a) <= abs(d) and abs(b) <= abs(d) and a * d <= 0 <= b * d
    assert tuple(int(v) for v in ref.split(6, 1, 2)) == (-3, 3) and tuple(int(v) for v in ref.split(-4, 1, 3)) == (1, -3)
    assert tuple(int(v) for v in ref.split(5, 1, 2)) == (-3, 2) and tuple(int(v) for v in ref.split(-5, 1, 2)) == (2, -3)


@pytest.mark.parametrize("p,q", PHASES)
def test_reference_translated_texture(p, q):
    """Noise translated by (6, -4): every interior block picks d = (6, -4) with SAD 0, and the interior of the output is A read at
    offset a, exactly, at every phase (A and B read the same texel)."""
    A, B = ref.translated_pair(H, W, 3, SHIFT, seed=11)
    out, mv, sad = ref.interp_frame(A, B, p, q, search=8, penalty=4, max_sad=24)
    bys, bxs = _interior(SHIFT)
    ay, ax = int(ref.split(SHIFT[0], p, q)[0]), int(ref.split(SHIFT[1], p, q)[0])
    for by in bys:
        for bx in bxs:
            assert tuple(mv[by, bx]) == SHIFT and sad[by, bx] == 0
            ys, xs = slice(8 * by, 8 * by + 8), slice(8 * bx, 8 * bx + 8)
            want = A[8 * by + ay:8 * by + ay + 8, 8 * bx + ax:8 * bx + ax + 8]
            assert np.array_equal(out[ys, xs], want)


def test_reference_still_pair():
    A = ref.noise((H, W, 3), 5)
    for p, q in PHASES:
        out, mv, sad = ref.interp_frame(A, A.copy(), p, q)
        assert np.array_equal(out, A) and not mv.any() and not sad.any()


def test_reference_independent_noise_falls_back():
    A, B = ref.noise((H, W, 3), 1), ref.noise((H, W, 3), 2)
    out, mv, sad = ref.interp_frame(A, B, 1, 2)
    assert not mv.any() and sad.min() > 24 * 256                                  # (the smallest best SAD is about 44 per pixel)
    assert np.array_equal(out, ref.crossfade(A, B, 1, 2))
    _, mv255, sad255 = ref.interp_frame(A, B, 1, 2, max_sad=255)                   # never falls back: the chosen vectors stay
    assert np.array_equal(sad255, sad) and mv255.any()
    out0, mv0, _ = ref.interp_frame(A, B, 1, 3, search=0)                          # R = 0: the rounded cross-fade
    assert np.array_equal(out0, ref.crossfade(A, B, 1, 3)) and not mv0.any()
