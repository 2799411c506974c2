"""The decode stage without a GPU (landiff_amd/decode.py): the numpy restatement of the rule (tests/jpeg_dec_ref.py)
against PIL's decode byte for byte, the header parser's refusals on files PIL wrote, the table words, the container walk, the
restatement's statuses on three malformed streams, and the library's refusals that come before any launch."""
import ctypes
import dataclasses
import io
import re

import numpy as np
import pytest
from PIL import Image

import jpeg_dec_ref as dref
import jpeg_ref as ref
from landiff_amd import decode as D
from landiff_amd import encode as E

SUBS = ("420", "444")
SMALL = ((1, 1), (3, 5), (9, 4), (16, 6), (31, 47))


def pil_decode(jpeg):
    return np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))


def pil_write(frame, **kw):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame), kw.pop("mode", "RGB")).save(buf, format="JPEG", **kw)
    return buf.getvalue()


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("quality", ref.QUALITIES)
def test_restatement_equals_pil_and_inverts_the_coder(sub, quality):
    """Every size x family at this quality and subsampling: the restatement's pixels are PIL's, its coefficients the encoder
    restatement's."""
    for H, W in ref.SIZES + SMALL:
        for kind in ref.FAMILIES:
            frame = ref.picture(kind, H, W)
            jpeg = ref.jpeg_encode(frame[None], quality, sub)[0]
            got = dref.decode(jpeg)
            assert not got["status"].any(), (kind, H, W, got["status"])
            assert np.array_equal(got["coefs"], ref.jpeg_coefs(frame[None], quality, sub)[0]), (kind, H, W)
            assert np.array_equal(got["pixels"], pil_decode(jpeg)), (kind, H, W)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("kind", ("noise", "ramps"))
def test_restatement_equals_pil_at_the_workload_size(sub, kind):
    frame = ref.picture(kind, 480, 720)
    jpeg = ref.jpeg_encode(frame[None], 95, sub)[0]
    got = dref.decode(jpeg)
    assert not got["status"].any() and np.array_equal(got["pixels"], pil_decode(jpeg))


@pytest.mark.parametrize("quality", (50, 95))
def test_restatement_equals_pil_on_pils_own_streams(quality):
    """Optimised Huffman tables, 4:4:4, no DRI: one segment per frame."""
    for kind in ("noise", "ramps", "bars"):
        jpeg = pil_write(ref.picture(kind, 50, 70), quality=quality, subsampling=0, optimize=True)
        got = dref.decode(jpeg)
        info = got["info"]
        assert info.restart_interval == 0 and info.segments == 1 and info.subsampling == "444"
        assert not got["status"].any() and np.array_equal(got["pixels"], pil_decode(jpeg)), kind


def test_parse_jpeg_reads_what_the_encoder_wrote():
    for sub in SUBS:
        jpeg = ref.jpeg_encode(ref.picture("noise", 24, 40)[None], 80, sub)[0]
        info = D.parse_jpeg(jpeg)
        luma, chroma = E.quant_tables(80)
        assert (info.width, info.height, info.subsampling) == (40, 24, sub) and info.quant == (luma, chroma, chroma)
        t = {k: (b, v) for k, b, v in E.HUFFMAN_TABLES}
        assert info.huffman == ((t[0x00], t[0x10]), (t[0x01], t[0x11]), (t[0x01], t[0x11]))
        assert info.restart_interval == -(-40 // E.mcu_size(sub)) and info.scan_offset == len(E.jpeg_header(24, 40, 80, sub))
        assert info.segments == -(-24 // E.mcu_size(sub))
        D.check_scan(jpeg, info)


def test_parse_jpeg_refuses_with_the_reason():
    frame = ref.picture("ramps", 24, 40)
    good = ref.jpeg_encode(frame[None], 95, "420")[0]
    cases = [(pil_write(frame, quality=90, progressive=True), "progressive"),
             (pil_write(frame, quality=90, subsampling=1), r"sampling factors 2x1 1x1 1x1 are not supported.*later work"),
             (pil_write(frame[..., 0], mode="L", quality=90), "greyscale is not supported.*later work"),
             (good.replace(b"\xff\xdb\x00\x43\x00", b"\xff\xdb\x00\x43\x10", 1), "16-bit DQT"),
             (good.replace(b"\xff\xc0\x00\x11\x08", b"\xff\xc0\x00\x11\x0c", 1), "12-bit precision"),
             (good.replace(b"\xff\xc0\x00\x11", b"\xff\xe5\x00\x11", 1), "SOS before SOF"),
             (good.replace(b"\xff\xc4\x00\x1f\x00", b"\xff\xe5\x00\x1f\x00", 1), "missing table: Huffman table DC 0"),
             (good.replace(b"\xff\xdb\x00\x43\x01", b"\xff\xe5\x00\x43\x01", 1), "missing table: quantisation table 1"),
             (good[:2] + b"\xff\xee\x00\x0e" + b"Adobe\x00\x64\x00\x00\x00\x00\x00" + good[2:], "Adobe APP14 segment with transform 0"),
             (b"\x00\x00" + good[2:], "no SOI"), (good[:300], "ends inside its headers")]
    sos = good.index(b"\xff\xda\x00\x0c")
    cases.append((good[:sos + 11] + b"\x01" + good[sos + 12:], "Ss = 0, Se = 63"))
    for k, (jpeg, why) in enumerate(cases):
        with pytest.raises(ValueError, match=f"frame {k}: .*{why}"):
            D.parse_jpeg(jpeg, frame=k)
    # an Adobe segment that says YCbCr (transform 1), comments and other APPn are skipped
    ok = good[:2] + b"\xff\xee\x00\x0e" + b"Adobe\x00\x64\x00\x00\x00\x00\x01" + b"\xff\xfe\x00\x05abc" + good[2:]
    info = D.parse_jpeg(good)
    assert D.parse_jpeg(ok) == dataclasses.replace(info, scan_offset=info.scan_offset + 23)
    for jpeg, why in ((good[:-2], "without EOI"), (good[:-2] + b"\xff\xda" + good[-2:], "several scans"),
                      (good[:info.scan_offset + 5] + b"\xff\xff" + good[info.scan_offset + 5:], "fill bytes")):
        with pytest.raises(ValueError, match=f"frame 3: .*{why}"):
            D.check_scan(jpeg, info, frame=3)


def test_decode_tables_round_trip():
    """The words of the stated tables and of an optimised set give back BITS and HUFFVAL; the look-ahead and the limit / offset
    words find every code's symbol."""
    optimised = D.parse_jpeg(pil_write(ref.picture("noise", 50, 70), quality=50, subsampling=0, optimize=True))
    stated = D.parse_jpeg(ref.jpeg_encode(ref.picture("noise", 8, 8)[None], 95, "420")[0])
    assert optimised.huffman != stated.huffman
    for info in (stated, optimised):
        words = D.decode_tables(info)
        assert len(words) == D.TABLE_WORDS and tuple(words[:192]) == info.quant[0] + info.quant[1] + info.quant[2]
        for c in range(3):
            for k in range(2):
                bits, vals = info.huffman[c][k]
                w = words[192 + (2 * c + k) * 544:192 + (2 * c + k + 1) * 544]
                assert w == D.huffman_words(bits, vals) and D.huffman_from_words(w) == (tuple(bits), tuple(vals))
                for sym, (code, n) in E.huffman_codes(bits, vals).items():
                    c16 = code << (16 - n)                   # the code followed by zeros, and by ones
                    for peek in (c16, c16 | ((1 << (16 - n)) - 1)):
                        e = w[288 + (peek >> 8)]
                        if n <= 8:
                            assert e == (n << 8 | sym)
                        else:
                            assert e == 0
                            l = next(l for l in range(9, 17) if peek < w[l - 1])
                            assert l == n and w[32 + w[16 + l - 1] + (peek >> (16 - l))] == sym
    with pytest.raises(ValueError, match="no Huffman table"):
        D.huffman_words((3,) + (0,) * 15, (1, 2, 3))          # three codes of one bit


def test_avi_chunks_agree_with_the_reader(tmp_path):
    from landiff.utils import read_mjpeg_avi, read_mjpeg_avi_chunks, write_mjpeg_avi, write_mjpeg_avi_encoded
    images = np.stack([ref.picture(k, 34, 50, s) for s, k in enumerate(("noise", "ramps", "bars"))])
    write_mjpeg_avi(images, tmp_path / "pil.avi", fps=12, quality=90)
    jpegs = ref.jpeg_encode(images, 90, "420")
    write_mjpeg_avi_encoded(jpegs, (50, 34), tmp_path / "enc.avi", fps=30)
    for name, fps in (("pil.avi", 12), ("enc.avi", 30)):
        chunks, size, got_fps = read_mjpeg_avi_chunks(tmp_path / name)
        frames, fps2 = read_mjpeg_avi(tmp_path / name)
        assert size == (50, 34) and got_fps == fps == fps2 and len(chunks) == 3
        assert np.array_equal(np.stack([pil_decode(c) for c in chunks]), frames)
        assert np.array_equal(np.stack([dref.decode(c)["pixels"] for c in chunks]), frames)
    chunks, _, _ = read_mjpeg_avi_chunks(tmp_path / "enc.avi")
    assert [c[:len(j)] for c, j in zip(chunks, jpegs)] == jpegs and all(len(c) - len(j) == (len(j) & 1) for c, j in zip(chunks, jpegs))
    (tmp_path / "bad.avi").write_bytes(b"RIFF\0\0\0\0WAVE")
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        read_mjpeg_avi_chunks(tmp_path / "bad.avi")


# ---- three malformed streams (24 x 40 at 4:2:0: two segments of three MCUs), shared with tests/test_gpu_jpeg_dec.py ----
def cut_short():
    """The first segment without its last four bytes: the decoder wants bits past its end.  -> (stream, statuses)"""
    jpeg = ref.jpeg_encode(ref.picture("noise", 24, 40)[None], 95, "420")[0]
    at = jpeg.index(b"\xff\xd0", D.parse_jpeg(jpeg).scan_offset)
    assert b"\xff" not in jpeg[at - 6:at]                     # no stuffed pair is split
    return jpeg[:at - 4] + jpeg[at:], [dref.OVERRUN, dref.OK]


def run_past_63():
    """Built, not searched: block 0 is DC 0, sixteen +1 at coefficients 1..16 (2 + 16 x 3 bits), two ZRL (2 x 11 bits: 72 bits, the
    position is 49) and +1 at coefficient 63 = symbol (run 14, size 1), a 16-bit code that starts on byte 9 of the segment.  Its
    high byte is 0xFF (stuffed), its low byte follows the 0x00; the code of (run 15, size 1) is ten symbols on, the same high
    byte.  With that one byte changed the run ends at 49 + 15 = 64.  -> (stream, statuses)"""
    coefs = np.zeros((36, 64), dtype=np.int64)
    coefs[0, 1:17] = 1
    coefs[0, 63] = 1
    jpeg = bytearray(dref.encode_coefs(coefs, 24, 40, 95, "420", 3))
    assert np.array_equal(dref.decode(bytes(jpeg))["coefs"], coefs)
    codes = E.huffman_codes(E.AC_LUMA_BITS, E.AC_LUMA_VALS)
    (honest, n0), (longer, n1) = codes[0xE1], codes[0xF1]
    at = D.parse_jpeg(bytes(jpeg)).scan_offset + 9
    assert n0 == n1 == 16 and honest >> 8 == longer >> 8 == 0xFF and list(jpeg[at:at + 3]) == [0xFF, 0x00, honest & 0xFF]
    jpeg[at + 2] = longer & 0xFF
    return bytes(jpeg), [dref.OVERFLOW, dref.OK]


def marker_removed():
    """The RST0 between the two segments taken out: no marker where one is due.  -> (stream, statuses)"""
    jpeg = ref.jpeg_encode(ref.picture("ramps", 24, 40)[None], 95, "420")[0]
    at = jpeg.index(b"\xff\xd0", D.parse_jpeg(jpeg).scan_offset)
    return jpeg[:at] + jpeg[at + 2:], [dref.MARKERS, dref.MARKERS]


MALFORMED = (cut_short, run_past_63, marker_removed)


@pytest.mark.parametrize("make", MALFORMED)
def test_restatement_statuses_on_malformed_streams(make):
    jpeg, want = make()
    info = D.parse_jpeg(jpeg)
    D.check_scan(jpeg, info)                                  # nothing the host can see before a launch
    got = dref.decode(jpeg)
    assert got["status"].tolist() == want and got["pixels"] is None
    if make is marker_removed:
        assert got["frame_info"].tolist()[:2] == [0, 1] and got["table"][1].tolist() == [0, 0, 0, 3, 3]


def test_segment_table_of_the_restatement():
    jpeg = ref.jpeg_encode(ref.picture("noise", 40, 24)[None], 100, "444")[0]            # five MCU rows of three MCUs
    info = D.parse_jpeg(jpeg)
    table, finfo = dref.find_segments(jpeg, info.scan_offset, len(jpeg) - info.scan_offset, 3, info.mcus, 7, frame=4)
    assert finfo.tolist() == [4, 1, len(jpeg) - 2 - info.scan_offset]
    assert table[:, 0].tolist() == [4] * 7 and table[5:, 1:].tolist() == [[0] * 4] * 2
    assert table[:5, 3].tolist() == [0, 3, 6, 9, 12] and table[:5, 4].tolist() == [3] * 5
    segs = [jpeg[s:s + n] for s, n in table[:5, 1:3].tolist()]
    assert segs == ref.jpeg_entropy(ref.jpeg_coefs(ref.picture("noise", 40, 24)[None], 100, "444"), 3, "444")[0]


def test_refusals_before_any_launch():
    """Every refusal of the entry points answers before a launch: safe without a GPU."""
    from landiff_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    INVALID, UNSUPPORTED = -1, -3

    def find_segments(data=p, n=1000, scan=p, ri=p, seg=p, info=p, F=2, S=4, H=30, W=40, sub=420):
        return lib.ld_jpeg_find_segments(data, n, scan, ri, seg, info, F, S, H, W, sub, None)

    def decode_entropy(data=p, n=1000, seg=p, info=p, ri=p, tables=p, tset=p, sets=1, coefs=p, status=p, F=2, S=4, H=30, W=40, sub=420):
        return lib.ld_jpeg_decode_entropy(data, n, seg, info, ri, tables, tset, sets, coefs, status, F, S, H, W, sub, None)

    def decode_rgb(coefs=p, tables=p, tset=p, sets=1, planes=p, out=p, fs=30 * 120, rs=120, F=2, H=30, W=40, sub=420):
        return lib.ld_jpeg_decode_rgb(coefs, tables, tset, sets, planes, out, fs, rs, F, H, W, sub, None)

    odd = ctypes.c_void_p(258)
    cases = [(find_segments, dict(data=None), INVALID, b"null pointer"), (find_segments, dict(info=None), INVALID, b"null pointer"),
             (find_segments, dict(seg=odd), INVALID, b"aligned"), (find_segments, dict(n=0), INVALID, b"must be positive"),
             (find_segments, dict(S=0), INVALID, b"must be positive"), (find_segments, dict(F=0), INVALID, b"1 .. 65535 frames"),
             (find_segments, dict(sub=422), UNSUPPORTED, b"subsampling must be 420 or 444, got 422"),
             (find_segments, dict(W=8193), UNSUPPORTED, b"up to 8192 wide"), (find_segments, dict(H=0), INVALID, b"empty shape"),
             (decode_entropy, dict(coefs=None), INVALID, b"null pointer"), (decode_entropy, dict(status=None), INVALID, b"null pointer"),
             (decode_entropy, dict(coefs=odd), INVALID, b"aligned"), (decode_entropy, dict(sets=0), INVALID, b"must be positive"),
             (decode_entropy, dict(F=65536), INVALID, b"1 .. 65535 frames"), (decode_entropy, dict(sub=411), UNSUPPORTED, b"got 411"),
             (decode_entropy, dict(H=65536), UNSUPPORTED, b"65535 high"),
             (decode_rgb, dict(out=None), INVALID, b"null pointer"), (decode_rgb, dict(planes=ctypes.c_void_p(260)), INVALID, b"aligned"),
             (decode_rgb, dict(rs=100), INVALID, b"row_stride"), (decode_rgb, dict(fs=1000), INVALID, b"frame_stride"),
             (decode_rgb, dict(sub=0), UNSUPPORTED, b"subsampling"), (decode_rgb, dict(sets=0), INVALID, b"must be positive")]
    for fn, kw, code, msg in cases:
        assert fn(**kw) == code, (fn.__name__, kw)
        err = lib.ld_last_error()
        assert f"ld_jpeg_{fn.__name__}".encode() in err and msg in err, (kw, err)
    size = lambda what, H=480, W=720, sub=420: lib.ld_jpeg_dec_size(what, H, W, sub)
    assert (size(0), size(1), size(2), size(3)) == (45 * 30 * 6, 45 * 30, 3 * 480 * 720, D.TABLE_WORDS)
    assert size(0, 17, 33, 444) == 3 * 5 * 3 and size(2, 17, 33) == 3 * 32 * 48 and size(2, 17, 33, 444) == 3 * 24 * 40
    assert size(0, W=8193) == UNSUPPORTED and size(0, sub=1) == UNSUPPORTED and size(9) == INVALID and size(0, H=0) == INVALID


def test_entry_points_in_header_library_and_signatures():
    import os
    import subprocess
    from landiff_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "landiff_hip.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, ret, nargs in (("ld_jpeg_dec_size", "int64_t", 4), ("ld_jpeg_find_segments", "int", 12),
                             ("ld_jpeg_decode_entropy", "int", 16), ("ld_jpeg_decode_rgb", "int", 13)):
        decl = re.search(rf"\b{ret} {name}\(([^;]*)\);", hdr)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert re.search(rf" T {name}\b", syms)
    assert int(re.search(r"#define LD_JPEG_DEC_TABLE_WORDS (\d+)", hdr).group(1)) == D.TABLE_WORDS
    for code, name in enumerate(D.STATUS):
        assert re.search(rf"#define LD_JPEG_DEC_{name} {code}\b", hdr)
    assert _lib.load().ld_jpeg_dec_size.restype is ctypes.c_int64


def test_wrappers_and_command_line_refuse_on_the_host(capsys):
    import torch
    import landiff.infer_video as iv
    from landiff_amd import _lib
    good = ref.jpeg_encode(ref.clip3("ramps", 24, 40), 95, "420")
    with pytest.raises(ValueError, match="need the device"):
        D.decode_jpeg(good)
    with pytest.raises(ValueError, match="frames must name some of the 3 streams"):
        D.decode_jpeg(good, "cpu", frames=[3])
    other = ref.jpeg_encode(ref.picture("ramps", 24, 48)[None], 95, "420") + ref.jpeg_encode(ref.picture("ramps", 24, 40)[None], 95, "444")
    for k in (0, 1):
        with pytest.raises(ValueError, match="frame 1: .*mixed sizes or subsamplings"):
            D.decode_jpeg(good[:1] + other[k:k + 1], "cpu")
    with pytest.raises(ValueError, match="frame 1: .*progressive"):
        D.decode_jpeg([good[0], pil_write(ref.picture("ramps", 24, 40), progressive=True)], "cpu")
    with pytest.raises(ValueError, match="frame 2: a frame without EOI"):
        D.decode_jpeg(good[:2] + [good[2][:-2]], "cpu")
    with pytest.raises(_lib.LandiffHipError, match="GPU tensors"):                  # valid streams, a host device: no CPU fallback
        D.decode_jpeg(good, torch.device("cpu"))
    args = iv.parse_args(["--prompt", "p"])
    assert args.video_decoder == "host" and args.encode_verify is False
    assert iv.parse_args(["--prompt", "p", "--video_decoder", "gpu"]).video_decoder == "gpu"
    assert iv.parse_args(["--prompt", "p", "--video_encoder", "gpu", "--encode_verify"]).encode_verify is True
    for argv, msg in ((["--encode_verify"], "--encode_verify goes with --video_encoder gpu"), (["--video_decoder", "nvdec"], "invalid choice")):
        with pytest.raises(SystemExit):
            iv.parse_args(["--prompt", "p"] + argv)
        assert msg in capsys.readouterr().err
