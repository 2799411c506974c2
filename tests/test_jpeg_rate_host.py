"""Rate control of the encode stage (landiff_amd/encode.py JpegRateConfig) without a GPU: the restatement of the rule
(tests/jpeg_rate_ref.py), the rounds, the header template's DQT offsets, the container arithmetic, and every refusal."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_rate_ref as rr
import jpeg_ref as ref
from landiff_amd import encode as E

SUBS = ("420", "444")
KINDS = ("noise", "ramps", "checker", "bars")


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("H,W", ((24, 40), (17, 33)))
def test_restatement_at_three_kinds_of_budget(H, W, sub):
    for kind in KINDS:
        frame = ref.picture(kind, H, W)
        s1, s95 = rr.frame_size(frame, 1, sub), rr.frame_size(frame, 95, sub)
        assert 629 < s1 < s95, kind
        # one below the quality-1 size: nothing fits; encoded at the floor, and said so
        q, over, trials = rr.rate_search(frame[None], sub, 95, 1, frame_bytes=s1 - 1)
        assert (q, over) == ([1], [True]) and len(trials) == 8 == rr.rounds(1, 95)
        assert all(row[0][1] > s1 - 1 for row in trials if row[0][0]) and trials[0][0] == [95, s95]
        # the midpoint: an interior quality that fits, in at most 8 trials
        mid = (s1 + s95) // 2
        q, over, trials = rr.rate_search(frame[None], sub, 95, 1, frame_bytes=mid)
        assert 1 <= q[0] < 95 and over == [False] and rr.frame_size(frame, q[0], sub) <= mid, kind
        tried = [row[0][0] for row in trials]
        used = [t for t in tried if t]
        assert 2 <= len(used) <= 8 and tried == used + [0] * (8 - len(used)) and len(set(used)) == len(used)
        assert all(row[0] == [t, rr.frame_size(frame, t, sub)] for row, t in zip(trials, used))
        assert q[0] == max(t for t, row in zip(used, trials) if row[0][1] <= mid)        # the largest trial that fitted
        # the quality-95 size: the ceiling, in one trial
        q, over, trials = rr.rate_search(frame[None], sub, 95, 1, frame_bytes=s95)
        assert (q, over) == ([95], [False]) and trials[0][0] == [95, s95] and all(row[0] == [0, 0] for row in trials[1:])
        # clip mode on one frame is frame mode
        assert rr.rate_search(frame[None], sub, 95, 1, clip_bytes=mid)[:2] == rr.rate_search(frame[None], sub, 95, 1, frame_bytes=mid)[:2]


def test_size_is_not_monotone_and_the_rule_says_what_it_finds():
    """Facts of the rule, pinned: the bisection's result fits, and is not always the largest quality that fits."""
    a = ref.picture("checker", 24, 40)
    sizes = [rr.frame_size(a, q, "420") for q in range(1, 101)]
    assert sum(1 for x, y in zip(sizes, sizes[1:]) if y < x) == 18                # stream size shrinks going up one step, 18 times
    q, over, _ = rr.rate_search(a[None], "420", 95, 1, frame_bytes=1098)
    assert (q, over) == ([61], [False]) and sizes[61 - 1] <= 1098 and sizes[66 - 1] <= 1098
    b = ref.picture("checker", 17, 33)
    q, over, _ = rr.rate_search(b[None], "444", 95, 1, frame_bytes=912)
    assert (q, over) == ([58], [False]) and rr.frame_size(b, 60, "444") <= 912 and rr.frame_size(b, 58, "444") <= 912


def test_clip_mode_and_floor_of_the_restatement():
    frames = np.stack([ref.picture(k, 24, 40) for k in KINDS])
    total = lambda q: sum(rr.frame_size(f, q, "420") for f in frames)
    for budget, want_over in ((total(1) - 1, True), ((total(1) + total(95)) // 2, False), (total(95), False)):
        q, over, trials = rr.rate_search(frames, "420", 95, 1, clip_bytes=budget)
        assert len(set(q)) == 1 and over == [want_over] * 4
        assert want_over or total(q[0]) <= budget
        for row in trials:
            assert len({t for t, _ in row}) == 1 and all(n == (rr.frame_size(f, t, "420") if t else 0) for (t, n), f in zip(row, frames))
    q, over, trials = rr.rate_search(frames, "420", 95, 30, clip_bytes=total(1))     # the floor: 30, although 1 would fit
    assert q == [30] * 4 and over == [True] * 4 and len(trials) == rr.rounds(30, 95) == 8
    assert min(t for row in trials for t, _ in row if t) >= 30
    q, over, trials = rr.rate_search(frames, "420", 30, 30, frame_bytes=10 ** 6)
    assert q == [30] * 4 and over == [False] * 4 and len(trials) == 1


def test_rounds():
    from landiff_amd import _lib
    lib = _lib.load()
    for q_min, q_max, want in ((1, 95, 8), (1, 100, 8), (30, 30, 1), (40, 41, 2), (1, 64, 7), (1, 65, 8), (99, 100, 2)):
        assert E.rate_rounds(q_min, q_max) == rr.rounds(q_min, q_max) == want
        assert lib.ld_jpeg_rate_size(0, 3, 24, 40, 420, q_min, q_max) == want
        assert lib.ld_jpeg_rate_size(1, 3, 24, 40, 420, q_min, q_max) == 1 + 3 * want + 4      # the launches: (q_min, q_max) alone
        assert lib.ld_jpeg_rate_size(1, 181, 480, 720, 444, q_min, q_max) == 1 + 3 * want + 4
        assert lib.ld_jpeg_rate_size(2, 3, 24, 40, 420, q_min, q_max) == 9 and lib.ld_jpeg_rate_size(3, 3, 24, 40, 420, q_min, q_max) == 6 * want
    # the bisection never needs more: every budget pattern over the worst range
    for q_min, q_max in ((1, 100), (1, 95), (40, 41), (7, 23)):
        for limit in range(q_min - 1, q_max + 1):                                 # qualities <= limit fit
            q, over, tried = rr.bisect(lambda t: t <= limit, q_min, q_max)
            assert len(tried) <= rr.rounds(q_min, q_max) and q == max(limit, q_min) and over == (limit < q_min)
    with pytest.raises(ValueError):
        E.rate_rounds(5, 4)


def test_header_template_and_dqt_offsets():
    lo, hi = E.jpeg_dqt_offsets()
    for sub in SUBS:
        for H, W in ((24, 40), (480, 720), (16, 4096)):
            heads = {q: E.jpeg_header(H, W, q, sub) for q in (1, 49, 50, 95, 100)}
            assert {len(h) for h in heads.values()} == {E.JPEG_HEADER_BYTES} == {629}
            for q, h in heads.items():
                luma, chroma = E.quant_tables(q)
                assert h[lo - 5:lo] == b"\xff\xdb\x00\x43\x00" and h[hi - 5:hi] == b"\xff\xdb\x00\x43\x01"
                assert h[lo:lo + 64] == bytes(luma) and h[hi:hi + 64] == bytes(chroma)
                other = bytearray(heads[95])                                      # the template, patched: that quality's header
                other[lo:lo + 64], other[hi:hi + 64] = bytes(luma), bytes(chroma)
                assert bytes(other) == h
            diff = [i for i, (x, y) in enumerate(zip(heads[1], heads[100])) if x != y]
            assert diff and all(lo <= i < lo + 64 or hi <= i < hi + 64 for i in diff)


def test_container_arithmetic(tmp_path):
    from landiff.utils import mjpeg_avi_bytes, mjpeg_avi_stream_budget, write_mjpeg_avi_encoded
    frames = np.stack([ref.picture(k, 24, 40, s) for s, k in enumerate(("noise", "ramps", "bars", "checker", "noise"))])
    for quality in (90, 50, 20):
        jpegs = ref.jpeg_encode(frames, quality, "420")
        for n in (1, 2, 5):
            write_mjpeg_avi_encoded(jpegs[:n], (40, 24), tmp_path / "a.avi", fps=24)
            assert mjpeg_avi_bytes([len(j) for j in jpegs[:n]]) == os.path.getsize(tmp_path / "a.avi")
    for sizes in ([7], [8], [7, 9, 11], [700, 701, 702, 703]):                      # odd and even lengths, whatever the bytes are
        write_mjpeg_avi_encoded([b"\xff" * n for n in sizes], (8, 8), tmp_path / "b.avi")
        assert mjpeg_avi_bytes(sizes) == os.path.getsize(tmp_path / "b.avi")
    assert mjpeg_avi_bytes([0] * 3) == 232 + 24 * 3
    # streams within the budget give a file within the cap, all of odd length at worst
    for T, cap in ((3, 5000), (49, 10 ** 6)):
        left = mjpeg_avi_stream_budget(cap, T)
        assert left == cap - 232 - 25 * T
        sizes = [left // T - (1 - left // T % 2)] * T                              # odd sizes within the budget
        assert sum(sizes) <= left and mjpeg_avi_bytes(sizes) <= cap
    with pytest.raises(ValueError, match="leaves nothing"):
        mjpeg_avi_stream_budget(232 + 25 * 4, 4)
    assert mjpeg_avi_stream_budget(232 + 25 * 4 + 1, 4) == 1
    with pytest.raises(ValueError):
        mjpeg_avi_bytes([])


def test_rate_config_validation_and_report():
    assert E.JpegRateConfig(frame_bytes=900).mode == "frame" and E.JpegRateConfig(clip_bytes=5).budget == 5
    assert E.JpegRateConfig(frame_bytes=900) == E.JpegRateConfig(900, None, 1)
    for kw, msg in ((dict(), "exactly one"), (dict(frame_bytes=5, clip_bytes=5), "exactly one"), (dict(frame_bytes=0), "frame_bytes must be an integer >= 1"),
                    (dict(clip_bytes=-3), "clip_bytes must be an integer >= 1"), (dict(frame_bytes=9.5), "frame_bytes"),
                    (dict(frame_bytes=True), "frame_bytes"), (dict(frame_bytes=9, min_quality=0), "min_quality must be an integer in 1..100, got 0"),
                    (dict(frame_bytes=9, min_quality=101), "min_quality"), (dict(clip_bytes=9, min_quality="5"), "min_quality")):
        with pytest.raises(ValueError, match=msg):
            E.JpegRateConfig(**kw)
    frames = np.stack([ref.picture(k, 24, 40) for k in KINDS])
    streams, q, over, trials = rr.rate_encode(frames, "420", 95, 1, frame_bytes=800)
    rep = E.encode_report(streams, E.JpegConfig(95), E.JpegRateConfig(frame_bytes=800), dict(qualities=q, over_budget=over, trials=trials))
    assert rep["quality"] == 95 and rep["total_bytes"] == sum(len(s) for s in streams)
    assert rep["rate"] == dict(mode="frame", budget=800, min_quality=1, max_quality=95, quality=dict(min=min(q), mean=sum(q) / 4, max=max(q)),
                               over_budget_frames=[f for f in range(4) if over[f]], rounds=8,
                               trials_used=max(sum(1 for row in trials if row[f][0]) for f in range(4)))
    assert rep["rate"]["over_budget_frames"] == [2] and "rate" not in E.encode_report(streams, E.JpegConfig(95))     # checker: 845 at quality 1


def test_wrappers_and_command_line_refuse_on_the_host(capsys):
    import torch
    import landiff.infer_video as iv
    from landiff_amd import _lib, ops
    x = torch.zeros(2, 10, 12, 3, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        ops.jpeg_c8_u8(x.float())
    with pytest.raises(ValueError, match=r"\[F, H, W, 3\]"):
        ops.jpeg_c8_u8(x[..., :2])
    with pytest.raises(ValueError, match="on the GPU"):
        ops.jpeg_c8_u8(x)
    with pytest.raises(ValueError, match="subsampling must be '420' or '444', got '422'"):
        ops.jpeg_c8_u8(x, "422")
    c8, q = torch.zeros(2, 6, 64, dtype=torch.int16), torch.ones(2, dtype=torch.int32)
    with pytest.raises(TypeError, match="c8 must be an int16"):
        ops.jpeg_quant_i16(c8.int(), q)
    with pytest.raises(TypeError, match="quality must be an int32"):
        ops.jpeg_quant_i16(c8, q.long())
    with pytest.raises(ValueError, match="on one GPU"):
        ops.jpeg_quant_i16(c8, q)
    for kw, msg in ((dict(), "exactly one"), (dict(frame_bytes=9, clip_bytes=9), "exactly one"), (dict(frame_bytes=0), "budget must be an integer >= 1"),
                    (dict(frame_bytes=9, q_min=96), "q_min must be an integer in 1..q_max = 95"), (dict(clip_bytes=9, q_min=0), "q_min"),
                    (dict(frame_bytes=900), "on the GPU")):
        with pytest.raises(ValueError, match=msg):
            ops.jpeg_encode_rate_u8(x, 95, "420", **kw)
    with pytest.raises(ValueError, match="quality must be an integer in 1..100, got 0"):
        ops.jpeg_encode_rate_u8(x, 0, "420", frame_bytes=900)
    with pytest.raises(_lib.LandiffHipError, match="q_min <= q_max"):
        ops.jpeg_rate_size(0, 1, 16, 16, "420", 9, 3)
    with pytest.raises(TypeError, match="rate must be a JpegRateConfig"):
        E.encode_jpeg(x, E.JpegConfig(), rate=900)
    with pytest.raises(ValueError, match="return_rate goes with rate"):
        E.encode_jpeg(x, E.JpegConfig(), return_rate=True)
    with pytest.raises(ValueError, match="min_quality 60 is above the ceiling"):
        E.encode_jpeg(x, E.JpegConfig(50), rate=E.JpegRateConfig(frame_bytes=900, min_quality=60))
    base = ["--prompt", "p"]
    args = iv.parse_args(base)
    assert args.jpeg_rate is None and args.video_max_bytes is None and args.jpeg_frame_bytes is None
    args = iv.parse_args(base + ["--video_encoder", "gpu", "--jpeg_frame_bytes", "20000", "--jpeg_quality", "90"])
    assert args.jpeg_rate == E.JpegRateConfig(frame_bytes=20000) and args.jpeg.quality == 90
    args = iv.parse_args(base + ["--video_encoder", "gpu", "--video_max_bytes", "4000000"])
    assert args.video_max_bytes == 4000000 and args.jpeg_rate is None and args.jpeg == E.JpegConfig(95, "420")
    for argv, msg in ((["--jpeg_frame_bytes", "900"], "--jpeg_frame_bytes goes with --video_encoder gpu"),
                      (["--video_max_bytes", "900"], "--video_max_bytes goes with --video_encoder gpu"),
                      (["--video_encoder", "host", "--video_max_bytes", "900"], "--video_max_bytes goes with --video_encoder gpu"),
                      (["--video_encoder", "gpu", "--video_max_bytes", "900", "--jpeg_frame_bytes", "9"], "mutually exclusive"),
                      (["--video_encoder", "gpu", "--jpeg_frame_bytes", "0"], "frame_bytes must be an integer >= 1, got 0"),
                      (["--video_encoder", "gpu", "--video_max_bytes", "0"], "--video_max_bytes: must be an integer >= 1, got 0")):
        with pytest.raises(SystemExit):
            iv.parse_args(base + argv)
        assert msg in capsys.readouterr().err
    # a cap that leaves nothing for the streams is refused before the frames are touched (an object with a shape is enough)
    class Shape:
        shape = (49, 480, 720, 3)
    with pytest.raises(ValueError, match="leaves nothing for the streams of 49 frames"):
        iv._save_encoded(Shape(), "unused", 8, E.JpegConfig(), max_bytes=1000)


def test_refusals_before_any_launch():
    """Every refusal of the rate entry points answers before a launch: the pointers are never dereferenced, safe without a GPU."""
    from landiff_amd import _lib
    lib = _lib.load()
    p, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)
    INVALID, UNSUPPORTED = -1, -3

    def c8_u8(frames=p, fs=30 * 40 * 3, rs=40 * 3, tables=p, out=p, F=2, H=30, W=40, sub=420):
        return lib.ld_jpeg_c8_u8(frames, fs, rs, tables, out, F, H, W, sub, None)

    def quant_i16(c8=p, tables=p, quality=p, out=p, F=2, blocks=36, sub=420):
        return lib.ld_jpeg_quant_i16(c8, tables, quality, out, F, blocks, sub, None)

    def encode_rate_u8(frames=p, fs=30 * 40 * 3, rs=40 * 3, tables=p, header=p, hb=629, d0=25, d1=94, c8=p, cw=p, sw=p, st=p, out=p, cap=1 << 40,
                       offs=p, lens=p, quality=p, over=p, trials=p, tcap=1 << 30, F=2, H=30, W=40, sub=420, q_min=1, q_max=95, fb=900, cb=0):
        return lib.ld_jpeg_encode_rate_u8(frames, fs, rs, tables, header, hb, d0, d1, c8, cw, sw, st, out, cap, offs, lens, quality, over,
                                          trials, tcap, F, H, W, sub, q_min, q_max, fb, cb, None)

    cases = [(c8_u8, dict(frames=None), INVALID, b"null pointer"), (c8_u8, dict(out=None), INVALID, b"null pointer"),
             (c8_u8, dict(out=odd), INVALID, b"aligned"), (c8_u8, dict(sub=422), UNSUPPORTED, b"got 422"),
             (c8_u8, dict(F=0), INVALID, b"empty shape"), (c8_u8, dict(rs=100), INVALID, b"row_stride"),
             (c8_u8, dict(W=8200, rs=8200 * 3, fs=30 * 8200 * 3), UNSUPPORTED, b"up to 8192 wide"),
             (quant_i16, dict(c8=None), INVALID, b"null pointer"), (quant_i16, dict(quality=None), INVALID, b"null pointer"),
             (quant_i16, dict(quality=odd), INVALID, b"aligned"), (quant_i16, dict(out=odd), INVALID, b"aligned"),
             (quant_i16, dict(F=0), INVALID, b"empty shape"), (quant_i16, dict(blocks=0), INVALID, b"empty shape"),
             (quant_i16, dict(blocks=35), INVALID, b"no multiple of the 6 blocks"), (quant_i16, dict(sub=411), UNSUPPORTED, b"got 411"),
             (encode_rate_u8, dict(header=None), INVALID, b"null pointer"), (encode_rate_u8, dict(trials=None), INVALID, b"null pointer"),
             (encode_rate_u8, dict(st=None), INVALID, b"null pointer"), (encode_rate_u8, dict(c8=None), INVALID, b"null pointer"),
             (encode_rate_u8, dict(sw=ctypes.c_void_p(260)), INVALID, b"aligned"), (encode_rate_u8, dict(st=odd), INVALID, b"aligned"),
             (encode_rate_u8, dict(quality=ctypes.c_void_p(260)), INVALID, b"aligned"),
             (encode_rate_u8, dict(fb=-1), INVALID, b"a budget must be >= 1"), (encode_rate_u8, dict(fb=0, cb=-5), INVALID, b"a budget must be >= 1"),
             (encode_rate_u8, dict(fb=0, cb=0), INVALID, b"neither frame_bytes nor clip_bytes"),
             (encode_rate_u8, dict(fb=9, cb=9), INVALID, b"frame_bytes and clip_bytes are both given"),
             (encode_rate_u8, dict(q_min=40, q_max=30), INVALID, b"q_min 40 is above q_max 30"),
             (encode_rate_u8, dict(q_min=0), INVALID, b"q_min and q_max must be in 1..100, got 0, 95"),
             (encode_rate_u8, dict(q_max=101), INVALID, b"q_min and q_max must be in 1..100, got 1, 101"),
             (encode_rate_u8, dict(cap=1000), INVALID, b"out_capacity 1000 is below the bound"),
             (encode_rate_u8, dict(tcap=31), INVALID, b"trials_capacity 31 is below the 32 words of 8 rounds"),
             (encode_rate_u8, dict(hb=0), INVALID, b"header_bytes"), (encode_rate_u8, dict(d1=80), INVALID, b"dqt_luma 25 / dqt_chroma 80"),
             (encode_rate_u8, dict(d1=600), INVALID, b"dqt_chroma 600"), (encode_rate_u8, dict(d0=-1), INVALID, b"dqt_luma -1"),
             (encode_rate_u8, dict(sub=0), UNSUPPORTED, b"subsampling"), (encode_rate_u8, dict(F=0), INVALID, b"empty shape"),
             (encode_rate_u8, dict(W=8193, rs=8193 * 3, fs=30 * 8193 * 3), UNSUPPORTED, b"up to 8192 wide")]
    for fn, kw, code, msg in cases:
        assert fn(**kw) == code, (fn.__name__, kw)
        err = lib.ld_last_error()
        assert f"ld_jpeg_{fn.__name__}".encode() in err and msg in err, (kw, err)
    size = lambda what, F=1, H=480, W=720, sub=420, lo=1, hi=95: lib.ld_jpeg_rate_size(what, F, H, W, sub, lo, hi)
    assert (size(0), size(1), size(2, F=49), size(3, F=49)) == (8, 29, 147, 784)
    for kw, code, msg in ((dict(lo=0), INVALID, b"1..100"), (dict(hi=101), INVALID, b"1..100"), (dict(lo=9, hi=8), INVALID, b"q_min <= q_max"),
                          (dict(F=0), INVALID, b"positive"), (dict(W=8193), UNSUPPORTED, b"8192"), (dict(sub=1), UNSUPPORTED, b"subsampling"),
                          (dict(what=9), INVALID, b"unknown quantity 9")):
        assert size(kw.pop("what", 0), **kw) == code and msg in lib.ld_last_error(), kw


def test_entry_points_in_header_library_and_signatures():
    from landiff_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "landiff_hip.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, ret, nargs in (("ld_jpeg_rate_size", "int64_t", 7), ("ld_jpeg_c8_u8", "int", 10), ("ld_jpeg_quant_i16", "int", 8),
                             ("ld_jpeg_encode_rate_u8", "int", 29)):
        decl = re.search(rf"\b{ret} {name}\(([^;]*)\);", hdr)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert re.search(rf" T {name}\b", syms)
    assert _lib.load().ld_jpeg_rate_size.restype is ctypes.c_int64
    assert int(re.search(r"#define LD_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == _lib.load().ld_version() >= 18


@pytest.mark.parametrize("sub", SUBS)
def test_reference_fixture_opens_in_pil_with_each_frames_tables(sub):
    """A rate-controlled clip of the restatement: every stream is a JPEG whose DQT is quant_tables of that frame's quality."""
    frames = np.stack([ref.picture(k, 24, 40) for k in KINDS])
    streams, q, over, _ = rr.rate_encode(frames, sub, 95, 1, frame_bytes=950)
    assert len(set(q)) > 1 and not any(over)
    zig = E.zigzag_order()
    for s, qf in zip(streams, q):
        assert len(s) <= 950
        img = Image.open(io.BytesIO(s))
        img.load()
        assert img.size == (40, 24) and img.mode == "RGB"
        luma, chroma = E.quant_tables(qf)
        got = {k: list(v) for k, v in img.quantization.items()}
        # PIL hands the tables in zigzag or natural order, depending on its version: accept either, the same for both tables
        natural = lambda t: [t[zig.index(n)] for n in range(64)]
        assert got in ({0: list(luma), 1: list(chroma)}, {0: natural(luma), 1: natural(chroma)}), qf
