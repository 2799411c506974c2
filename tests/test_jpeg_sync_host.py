"""The decode stage's second entropy route without a GPU: the restatement of its rule (tests/jpeg_sync_ref.py) against
the serial restatement (tests/jpeg_dec_ref.py) on every family the GPU tests use, the rounds' bound, a stuffed byte at a
subsequence boundary, and the host logic: entropy_route, the refusals of the new arguments, the entry points."""
import ctypes
import re
from functools import lru_cache

import numpy as np
import pytest

import jpeg_dec_ref as dref
import jpeg_ref as ref
import jpeg_sync_ref as sref
from landiff_amd import decode as D
from landiff_amd import encode as E
from test_jpeg_dec_host import MALFORMED, pil_write

SIZES = ((1, 1), (8, 8), (3, 5), (17, 33), (31, 47), (48, 64))
SUB_BYTES = (64, 256)


def reencoded(kind, sub, ri, quality=100):
    """A 24 x 40 frame coded by the restatement's coder at the restart interval ri (0: none)."""
    frame = ref.picture(kind, 24, 40)
    return dref.encode_coefs(ref.jpeg_coefs(frame[None], quality, sub)[0], 24, 40, quality, sub, ri)


def dense_ff(sub, blocks=24):
    """Blocks full of 0xFF bytes, no restart markers: one segment with stuffed bytes on multiples of 64 (24 blocks: 510 bytes, none
    on a multiple of 256) and, with 48 blocks, on a multiple of 256 too."""
    return dref.encode_coefs(ref.dense_ff_blocks(blocks), 8 if sub == "444" else 16, 64 * blocks // 24, 100, sub, 0)


def names():
    out = [("pil", kind, H, W, q, mode) for H, W in SIZES for kind in ("noise", "ramps", "checker") for q in (75, 95, 100)
           for mode in ("420", "444", "optimize")]
    out += [("reencoded", kind, sub, ri) for sub in ("420", "444") for kind, ri in (("noise", 0), ("noise", 1), ("ramps", 5), ("noise", 5))]
    return out + [("dense_ff", sub, blocks) for sub in ("444", "420") for blocks in (24, 48)]


@lru_cache(maxsize=None)
def stream(name):
    if name[0] == "pil":
        _, kind, H, W, q, mode = name
        kw = dict(subsampling=0) if mode == "444" else dict(optimize=True) if mode == "optimize" else {}
        return pil_write(ref.picture(kind, H, W), quality=q, **kw)
    if name[0] == "reencoded":
        return reencoded(*name[1:])
    if name[0] == "dense_ff":
        return dense_ff(*name[1:])
    raise KeyError(name)


@lru_cache(maxsize=None)
def serial(name):
    return dref.decode(stream(name))


@lru_cache(maxsize=None)
def synced(name, sub_bytes, max_rounds=None):
    """The restatement's decode by the sync route (computed once, never modified)."""
    return sref.decode(stream(name), sub_bytes, max_rounds)


@pytest.mark.parametrize("sub_bytes", SUB_BYTES)
def test_sync_restatement_equals_the_serial_one(sub_bytes):
    """Coefficients and status on every family; no fallback is needed when the rounds are not limited, and they never exceed n - 1."""
    most = 0
    for name in names():
        want, got = serial(name), synced(name, sub_bytes)
        assert not want["status"].any(), name
        assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["coefs"], want["coefs"]), name
        assert not got["fell"].any(), name
        for s, n in enumerate(got["n"]):
            assert got["rounds"][s] <= max(n - 1, 0), (name, s, n, got["rounds"][s])
            most = max(most, n)
    assert most >= (90 if sub_bytes == 64 else 20)                             # 48 x 64 noise at quality 100: many subsequences


def test_sizes_below_and_far_above_a_subsequence():
    one = synced(("pil", "noise", 1, 1, 100, "420"), 64)
    also = synced(("pil", "ramps", 8, 8, 75, "444"), 64)
    big = synced(("pil", "noise", 48, 64, 100, "420"), 64)
    assert one["n"] == [1] and also["n"] == [1] and big["n"][0] >= 90
    assert big["rounds"][0] >= big["n"][0] // 2                               # no EOB at quality 100: it hardly re-synchronises


def test_one_round_is_not_enough_for_noise_and_the_fallback_is_exact():
    name = ("pil", "noise", 48, 64, 100, "420")
    for sub_bytes in SUB_BYTES:
        got = synced(name, sub_bytes, 1)
        assert got["fell"].all() and got["rounds"].tolist() == [1]
        assert np.array_equal(got["coefs"], serial(name)["coefs"]) and not got["status"].any()


def test_a_stuffed_byte_sits_on_a_subsequence_boundary():
    """At every sub_bytes the families run at: the 24-block stream has one at a multiple of 64 (and, 510 bytes long, none at a
    multiple of 256); the 48-block stream has one at a multiple of 256."""
    for sub in ("444", "420"):
        for sub_bytes, blocks in ((64, 24), (64, 48), (256, 48)):
            assert ("dense_ff", sub, blocks) in names() and sub_bytes in SUB_BYTES
            jpeg = dense_ff(sub, blocks)
            info = D.parse_jpeg(jpeg)
            scan = jpeg[info.scan_offset:-2]
            at = [i for i in range(1, len(scan)) if scan[i - 1] == 0xFF and i % sub_bytes == 0]
            assert info.restart_interval == 0 and at and scan[at[0]] == 0, (sub, sub_bytes, blocks)
            bits = sref.Bits(scan)
            assert sref.cold_start(bits, at[0] // sub_bytes, sub_bytes)[0] == 8 * (at[0] + 1)      # the position is normalised past it
            assert all(p // 8 != at[0] for p in bits.at)
        scan = dense_ff(sub)[D.parse_jpeg(dense_ff(sub)).scan_offset:-2]
        assert not [i for i in range(256, len(scan), 256) if scan[i - 1] == 0xFF]


@pytest.mark.parametrize("make", MALFORMED)
def test_malformed_streams_give_the_serial_statuses(make):
    jpeg, want = make()
    for sub_bytes in SUB_BYTES:
        got = sref.decode(jpeg, sub_bytes)
        assert got["status"].tolist() == want
        assert np.array_equal(got["coefs"], dref.decode(jpeg)["coefs"])
        assert got["fell"].tolist() == [int(v not in (dref.OK, dref.MARKERS)) for v in want]    # an error is decoded again serially


def test_write_pass_reports_errors_before_any_fallback():
    """The write pass's own status (before the serial kernel repeats the segment) is the serial decoder's."""
    for make in MALFORMED[:2]:
        jpeg, want = make()
        info = D.parse_jpeg(jpeg)
        table, _ = dref.find_segments(jpeg, info.scan_offset, len(jpeg) - info.scan_offset, info.restart_interval, info.mcus, info.segments)
        books = [(dref.code_book(*dc), dref.code_book(*ac)) for dc, ac in info.huffman]
        for s in range(info.segments):
            _, st, ln, _, cnt = (int(v) for v in table[s])
            history, R = sref.rounds(jpeg[st:st + ln], 64, books, 6)
            assert R is not None and R <= max(len(history[0]) - 1, 0)
            assert sref.write_pass(jpeg[st:st + ln], 64, books, 6, cnt * 6, history[-1])[1] == want[s]


def test_dc_pass_is_the_serial_chain():
    rng = np.random.default_rng(5)
    diffs = np.zeros((40, 64), dtype=np.int64)
    diffs[:, 0] = rng.integers(-2047, 2048, 40) * 30                          # sums that wrap
    for bpm, comp in ((6, (0, 0, 0, 0, 1, 2)), (3, (0, 1, 2))):
        got = sref.dc_pass(diffs[:36], bpm)
        pred = [0, 0, 0]
        for b in range(36):
            c = comp[b % bpm]
            pred[c] = ((pred[c] + int(diffs[b, 0]) + 32768) & 0xFFFF) - 32768
            assert got[b, 0] == pred[c]
        assert np.abs(np.cumsum(diffs[:36:bpm, 0])).max() > 32768


def test_entropy_route_is_a_pure_host_function():
    pil = D.parse_jpeg(stream(("pil", "noise", 48, 64, 100, "420")))
    size = len(stream(("pil", "noise", 48, 64, 100, "420")))
    ours = ref.jpeg_encode(ref.picture("noise", 48, 64)[None], 95, "420")[0]
    assert pil.segments == 1 and D.AUTO_SUBSEQUENCES_PER_SEGMENT * 64 < size - pil.scan_offset < D.AUTO_SUBSEQUENCES_PER_SEGMENT * 256
    assert D.entropy_route([pil], [size], sub_bytes=64) == "sync"
    assert D.entropy_route([pil], [size]) == "segment" and D.entropy_route([pil], [size], sub_bytes=1024) == "segment"
    assert D.entropy_route([D.parse_jpeg(ours)], [len(ours)]) == "segment"        # one restart interval per MCU row: short segments
    tiny = stream(("pil", "noise", 8, 8, 100, "420"))
    assert D.entropy_route([D.parse_jpeg(tiny)], [len(tiny)], 64) == "segment"
    per = D.AUTO_SUBSEQUENCES_PER_SEGMENT * 256
    info = D.JpegInfo(64, 48, "420", pil.quant, pil.huffman, 0, 100)
    assert D.entropy_route([info, info], [100 + per, 100 + per]) == "segment" and D.entropy_route([info, info], [100 + per, 101 + per]) == "sync"
    with pytest.raises(ValueError, match="one size per stream"):
        D.entropy_route([pil], [])


def test_new_arguments_are_refused_on_the_host(capsys):
    import landiff.infer_video as iv
    good = ref.jpeg_encode(ref.clip3("ramps", 24, 40), 95, "420")
    for kw, msg in ((dict(entropy="wave"), "entropy must be one of segment, sync, auto"), (dict(sub_bytes=96), "sub_bytes must be a power of two"),
                    (dict(sub_bytes=32), "sub_bytes"), (dict(sub_bytes=2048), "sub_bytes"), (dict(sub_bytes=256.0), "sub_bytes"),
                    (dict(max_rounds=0), "max_rounds must be in 1 .. 4096"), (dict(max_rounds=4097), "max_rounds"), (dict(max_rounds=True), "max_rounds")):
        with pytest.raises(ValueError, match=msg):
            D.decode_jpeg(good, "cpu", **kw)
    with pytest.raises(ValueError, match="goes with decoder"):
        iv.load_clip("clip.npy", entropy="sync")
    assert iv.parse_args(["--prompt", "p"]).jpeg_entropy == "segment"
    assert iv.parse_args(["--prompt", "p", "--video_decoder", "gpu", "--jpeg_entropy", "auto"]).jpeg_entropy == "auto"
    for argv, msg in ((["--jpeg_entropy", "sync"], "--jpeg_entropy goes with --video_decoder gpu"),
                      (["--video_decoder", "gpu", "--jpeg_entropy", "wave"], "invalid choice")):
        with pytest.raises(SystemExit):
            iv.parse_args(["--prompt", "p"] + argv)
        assert msg in capsys.readouterr().err
    rep = D.decode_report([D.parse_jpeg(j) for j in good], [len(j) for j in good])
    assert rep["entropy"] == "segment" and rep["rounds"] is None and rep["segments_fallen_back"] is None and rep["sub_bytes"] is None
    info = np.zeros((3, 2, 2), dtype=np.int64)
    info[1, 0], info[2, 1] = (5, 1), (2, 0)
    rep = D.decode_report([D.parse_jpeg(j) for j in good], [len(j) for j in good], entropy="sync", sub_bytes=128, sync_info=info)
    assert rep["rounds"] == {"max": 5, "mean": 7 / 6} and rep["segments_fallen_back"] == 1 and rep["sub_bytes"] == 128 and rep["frames"] == 3


def test_entry_points_in_header_library_and_signatures():
    import os
    import subprocess
    from landiff_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "landiff_hip.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, ret, nargs in (("ld_jpeg_dec_sync_size", "int64_t", 6), ("ld_jpeg_decode_entropy_sync", "int", 24)):
        decl = re.search(rf"\b{ret} {name}\(([^;]*)\);", hdr)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert re.search(rf" T {name}\b", syms)
    assert _lib.load().ld_jpeg_dec_sync_size.restype is ctypes.c_int64
    assert int(re.search(r"#define LD_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION


def test_refusals_before_any_launch():
    """Every refusal of the two entry points answers before a launch: safe without a GPU."""
    from landiff_amd import _lib, ops
    lib = _lib.load()
    p, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)
    INVALID, UNSUPPORTED = -1, -3
    size = lambda what=0, scan=100000, F=2, S=4, B=256, R=32: lib.ld_jpeg_dec_sync_size(what, scan, F, S, B, R)
    T = (100000 // 256 + 8 + 128 + 63) // 64 * 64
    assert size(1) == T and size(0) >= 2 * T * 16 + 2 * T * 4 + 33 * 8 * 4
    assert size(1, B=64) == (100000 // 64 + 8 + 128 + 63) // 64 * 64
    for kw, msg in ((dict(B=96), b"sub_bytes must be a power of two in 64 .. 1024, got 96"), (dict(B=32), b"sub_bytes"), (dict(B=2048), b"sub_bytes"),
                    (dict(R=0), b"max_rounds must be in 1 .. 4096, got 0"), (dict(R=0, B=7, F=0), b"sub_bytes"), (dict(R=0, F=0), b"max_rounds"),
                    (dict(scan=0), b"must be positive"), (dict(S=0), b"must be positive"), (dict(F=0), b"1 .. 65535 frames"),
                    (dict(what=7), b"unknown quantity 7"), (dict(scan=1 << 42), b"exceed one call")):
        assert size(**kw) == INVALID, kw
        assert b"ld_jpeg_dec_sync_size" in lib.ld_last_error() and msg in lib.ld_last_error(), (kw, lib.ld_last_error())
    need = size(0)

    def sync(data=p, n=200000, seg=p, info=p, ri=p, tables=p, tset=p, sets=1, coefs=p, status=p, F=2, S=4, H=30, W=40, sub=420, scan=100000,
             B=256, R=32, ws=p, ws_bytes=need, sync_info=p, exits=None, index=None):
        return lib.ld_jpeg_decode_entropy_sync(data, n, seg, info, ri, tables, tset, sets, coefs, status, F, S, H, W, sub, scan, B, R, ws,
                                               ws_bytes, sync_info, exits, index, None)

    cases = [(dict(B=100), INVALID, b"sub_bytes"), (dict(R=-1), INVALID, b"max_rounds"), (dict(B=100, data=None), INVALID, b"sub_bytes"),
             (dict(data=None), INVALID, b"null pointer"), (dict(ws=None), INVALID, b"null pointer"), (dict(sync_info=None), INVALID, b"null pointer"),
             (dict(exits=p), INVALID, b"exits and exits_index go together"), (dict(index=p), INVALID, b"go together"),
             (dict(ws=odd), INVALID, b"aligned"), (dict(coefs=odd), INVALID, b"aligned"), (dict(exits=odd, index=p), INVALID, b"aligned"),
             (dict(ws_bytes=need - 1), INVALID, b"are needed"), (dict(scan=300000), INVALID, b"exceed data_bytes"),
             (dict(sets=0), INVALID, b"must be positive"), (dict(F=65536), INVALID, b"1 .. 65535 frames"),
             (dict(sub=422), UNSUPPORTED, b"subsampling must be 420 or 444, got 422"), (dict(W=8193), UNSUPPORTED, b"up to 8192 wide"),
             (dict(H=0), INVALID, b"empty shape")]
    for kw, code, msg in cases:
        assert sync(**kw) == code, kw
        err = lib.ld_last_error()
        assert b"ld_jpeg_decode_entropy_sync" in err and msg in err, (kw, err)
    assert ops.jpeg_dec_sync_size(1, 100000, 2, 4) == T
    with pytest.raises(_lib.LandiffHipError, match="sub_bytes"):
        ops.jpeg_dec_sync_size(0, 100000, 2, 4, sub_bytes=48)
