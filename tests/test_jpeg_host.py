"""The encode stage without a GPU (landiff_amd/encode.py): the stated tables against the segments PIL writes, the numpy
restatement (tests/jpeg_ref.py) as a JPEG that PIL decodes and whose quality is held against PIL's own encode, its segments and
markers, the DCT's stated bounds, the split AVI writer and its reader, and the refusals that come before any launch."""
import ctypes
import io
import re
import struct

import numpy as np
import pytest
from PIL import Image

import jpeg_ref as ref
from landiff_amd import encode as E

# mse(restatement) <= QUALITY_R * mse(PIL) + QUALITY_A, both decoded by PIL, PIL's encode at the same quality and subsampling with
# restart_marker_rows=1.  Measured on the cases of test_restatement_is_a_jpeg (840 frames; the restatement is deterministic):
#   * among the frames where PIL's mse is >= 10 grey levels^2 the largest ratio is 1.148 (noise 8 x 8, 4:2:0, quality 1:
#     7063.6 against 6152.1 -- one 255-step quantiser decision of a single-MCU picture);
#   * among the frames where it is < 10 the largest absolute excess is 0.934 (ramps 16 x 16, 4:2:0, quality 95: 2.415 against 1.482).
# Both come from coefficients that land exactly half-way between two quantiser steps in integer-valued synthetic pictures (ramps,
# saturated bars): the two encoders round such ties to different sides (five coefficients differ by one step in the 16 x 16 ramp),
# and PIL's side happens to clip in RGB.  The other way round PIL is up to 20 % worse (ramps 8 x 8, quality 50).  Each excess
# doubled, for content nobody tried: r = 1 + 2 * 0.148, a = 2 * 0.934.
QUALITY_R, QUALITY_A = 1.30, 1.87
PIL_SUB = {"420": 2, "444": 0}


def pil_encode(frame, quality, subsampling, **kw):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame), "RGB").save(buf, format="JPEG", quality=quality, subsampling=PIL_SUB[subsampling],
                                                             optimize=False, **kw)
    return buf.getvalue()


def decode(jpeg):
    im = Image.open(io.BytesIO(jpeg))
    return np.asarray(im.convert("RGB")), im.size


def segments_of(jpeg):
    """{marker: [bodies]} of the segments before SOS, and the bytes after SOS's header."""
    out, i = {}, 2
    assert jpeg[:2] == b"\xff\xd8"
    while True:
        assert jpeg[i] == 0xFF
        m, n = jpeg[i + 1], struct.unpack(">H", jpeg[i + 2:i + 4])[0]
        out.setdefault(m, []).append(jpeg[i + 4:i + 2 + n])
        i += 2 + n
        if m == 0xDA:
            return out, jpeg[i:]


def within_pil(mine, pil):
    return mine <= QUALITY_R * pil + QUALITY_A


def test_quantisation_tables_are_pils_for_every_quality():
    frame = ref.picture("noise", 16, 16)
    for q in range(1, 101):
        segs, _ = segments_of(pil_encode(frame, q, "420"))
        luma, chroma = E.quant_tables(q)
        assert segs[0xDB] == [bytes([0]) + bytes(luma), bytes([1]) + bytes(chroma)], q
    assert E.quant_tables(50) == (E.BASE_QUANT_LUMA, E.BASE_QUANT_CHROMA)
    for bad in (0, 101, 50.5, True):
        with pytest.raises(ValueError, match="quality must be an integer in 1..100"):
            E.quant_tables(bad)


def test_huffman_tables_and_header_are_pils():
    frame = ref.picture("noise", 24, 40)
    for sub in ("420", "444"):
        pil = pil_encode(frame, 95, sub, restart_marker_rows=1)
        segs, _ = segments_of(pil)
        assert segs[0xC4] == [bytes([t]) + bytes(bits) + bytes(vals) for t, bits, vals in E.HUFFMAN_TABLES]
        header = E.jpeg_header(24, 40, 95, sub)
        assert pil.startswith(header)                      # SOI, APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS: byte for byte PIL's
        assert segs[0xDD] == [struct.pack(">H", -(-40 // E.mcu_size(sub)))]
    for bits, vals in ((b, v) for _, b, v in E.HUFFMAN_TABLES):
        codes = E.huffman_codes(bits, vals)
        assert len(codes) == len(vals) == sum(bits) and all(c < (1 << n) - 1 for c, n in codes.values())      # no all-ones code word


def test_stated_constants():
    import math
    assert E.DCT_CONST[0] == 8192 and list(E.DCT_CONST[1:]) == [round(8192 * math.sqrt(2) * math.cos(k * math.pi / 16)) for k in range(1, 8)]
    K = np.array(E.dct_matrix(), dtype=np.float64) / 8192
    a = np.array([math.sqrt(1 / 8)] + [0.5] * 7)
    exact = math.sqrt(8) * a[:, None] * np.cos((2 * np.arange(8)[None, :] + 1) * np.arange(8)[:, None] * math.pi / 16)
    assert np.abs(K - exact).max() <= 0.5 / 8192
    zz = E.zigzag_order()
    assert sorted(zz) == list(range(64)) and zz[:10] == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and zz[-3:] == [55, 62, 63]
    words = E.table_words()
    assert len(words) == 800 and words[256 + 0] == (0b00 | 2 << 16) and words[288 + 0x00] == (0b1010 | 4 << 16)      # luma DC 0, luma EOB
    for kw in (dict(quality=0), dict(quality=101), dict(quality=95.0), dict(subsampling="422"), dict(subsampling=420)):
        with pytest.raises(ValueError, match="JpegConfig"):
            E.JpegConfig(**kw)
    assert E.JpegConfig() == E.JpegConfig(95, "420")


@pytest.mark.parametrize("sub", ("420", "444"))
@pytest.mark.parametrize("quality", ref.QUALITIES)
def test_restatement_is_a_jpeg(sub, quality):
    worst = (0.0, ())
    for H, W in ref.SIZES:
        for kind in ref.FAMILIES:
            frames = ref.clip3(kind, H, W)
            for f, jpeg in zip(frames, ref.jpeg_encode(frames, quality, sub)):
                got, size = decode(jpeg)
                assert size == (W, H), (kind, H, W)
                pil, _ = decode(pil_encode(f, quality, sub, restart_marker_rows=1))
                mine, theirs = ref.mse(got, f), ref.mse(pil, f)
                worst = max(worst, (mine - theirs, (kind, H, W, mine, theirs)))
                assert within_pil(mine, theirs), (kind, H, W, mine, theirs)
    print(f"{sub} q{quality}: largest excess over PIL {worst}")


def entropy_markers(jpeg):
    """The markers after SOS with their byte positions, and the segments between them: 0xFF 0x00 is data, anything else a marker."""
    _, data = segments_of(jpeg)
    markers, segs, start, i = [], [], 0, 0
    while i < len(data) - 1:
        if data[i] == 0xFF and data[i + 1] != 0:
            markers.append(data[i + 1])
            segs.append(data[start:i])
            i += 2
            start = i
        else:
            i += 2 if data[i] == 0xFF else 1
    assert start == len(data)                       # the stream ends with a marker
    return markers, segs


def test_restart_markers_and_stuffing():
    frames = ref.clip3("noise", 8 * 11, 24)                          # 4:4:4: 11 MCU rows of 3 MCUs
    for jpeg in ref.jpeg_encode(frames, 100, "444"):
        markers, segs = entropy_markers(jpeg)
        assert markers == [0xD0 + (r & 7) for r in range(10)] + [0xD9] and markers[8] == 0xD0
        assert all(len(s) > 0 for s in segs) and any(b"\xff\x00" in s for s in segs)        # quality-100 noise does need stuffing
        assert decode(jpeg)[1] == (24, 88)
    for sub, bpm in (("420", 6), ("444", 3)):                         # a flat frame: DC difference once, then EOB-only blocks
        flat = np.full((1, 40, 40, 3), 128, np.uint8)
        coefs = ref.jpeg_coefs(flat, 95, sub)
        assert not coefs.any()
        markers, segs = entropy_markers(ref.jpeg_encode(flat, 95, sub)[0])
        mcux = -(-40 // E.mcu_size(sub))
        luma, chroma = "00" + "1010", "00" + "00"                    # DC category 0, EOB
        bits = (luma * (bpm - 2) + chroma * 2) * mcux
        bits += "1" * (-len(bits) % 8)
        want = int(bits, 2).to_bytes(len(bits) // 8, "big")
        assert segs == [want] * len(segs) and len(segs) == -(-40 // E.mcu_size(sub))


def test_dct_bounds_on_the_maximising_patterns():
    """For each of the 64 basis functions the -128 / 127 sign pattern that maximises it (and its negative): every stage inside the
    bound DESIGN 8.12 states (far inside int32), 8 x the coefficient within 8192, and after quantisation by 1 the DC within +-1024
    and the AC within +-1023 before the clamp."""
    pats = ref.maximising_blocks().astype(np.int64) - 128
    trace = {}
    c8 = ref.fdct(np.concatenate([pats, -1 - pats]), trace)            # (-1 - s maps -128 <-> 127)
    assert trace["row_sum"] <= 128 * 65536 and trace["row_out"] <= 2 ** 14 and trace["col_sum"] <= 2 ** 30 + 2 ** 16 < 2 ** 31
    assert trace["c8"] <= 8192
    q = (np.abs(c8) + 4) // 8
    assert q.reshape(-1, 64)[:, 0].max() == 1024 and q.reshape(-1, 64)[:, 1:].max() <= 1023
    for i in range(64):                                                # the pattern does maximise its own coefficient
        assert abs(c8[i].reshape(64)[i]) == np.abs(c8[i]).max()
    # the stages against the float64 DCT: after the rows |t / 16 - exact| <= 128 * 8 * (0.5 / 8192) + 1 / 32 = 0.09375
    # (the constants' rounding, then the shift's); after the columns |c8 - exact| <= 8 * 0.09375 + 8 * 1024 * (0.5 / 8192) + 0.5 =
    # 1.75 in units of 1 / 8 coefficient.  Measured on these patterns and 4096 noise blocks: 0.066 and 0.996.
    a = np.array([np.sqrt(1 / 8)] + [0.5] * 7)
    D = a[:, None] * np.cos((2 * np.arange(8)[None, :] + 1) * np.arange(8)[:, None] * np.pi / 16)
    blocks = np.concatenate([pats, -1 - pats, np.random.default_rng(5).integers(-128, 128, (4096, 8, 8))])
    exact = 8 * np.einsum("vy,nyx,ux->nvu", D, blocks.astype(np.float64), D)
    rows = np.sqrt(8) * np.einsum("ux,nyx->nyu", D, blocks.astype(np.float64))
    assert np.abs(((np.einsum("ux,nyx->nyu", ref.K, blocks) + 256) >> 9) / 16 - rows).max() <= 0.09375
    assert np.abs(ref.fdct(blocks) - exact).max() <= 1.75
    flat = np.full((1, 8, 8), 77, np.int64)
    assert ref.fdct(flat)[0, 0, 0] == 77 * 64 and not ref.fdct(flat).reshape(64)[1:].any()      # the DC term is the exact sum


def test_all_ones_segment_is_doubled_by_the_restatement():
    """No code word is all 1-bits, so no byte string of this coder is 0xFF throughout; the densest one is built from the code table
    (jpeg_ref.dense_ff_blocks) and the restatement must double every 0xFF of it."""
    blocks = ref.dense_ff_blocks(24)
    acc, n = ref.segment_bits(blocks, "444")
    raw = ((acc << (-n % 8)) | ((1 << (-n % 8)) - 1)).to_bytes((n + 7) // 8, "big")
    ff = raw.count(b"\xff")
    assert ff * 2 > len(raw)                                            # most bytes are 0xFF
    out = ref.stuff(acc, n)
    assert len(out) == len(raw) + ff and out.replace(b"\xff\x00", b"\xff") == raw and b"\xff\xff" not in out


def _old_write_mjpeg_avi(images, path, fps=8, quality=95):
    """landiff.utils.write_mjpeg_avi as it was before the RIFF assembly was split off."""
    T, H, W, _ = images.shape
    frames = []
    for img in images:
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img), "RGB").save(buf, format="JPEG", quality=quality)
        b = buf.getvalue()
        frames.append(b + b"\0" * (len(b) & 1))
    chunk = lambda tag, data: tag + struct.pack("<I", len(data)) + data + b"\0" * (len(data) & 1)
    lst = lambda tag, data: b"LIST" + struct.pack("<I", len(data) + 4) + tag + data
    maxb = max(len(f) for f in frames)
    avih = struct.pack("<14I", 1000000 // fps, maxb * fps, 0, 0x10, T, 0, 1, maxb, W, H, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, 1, fps, 0, T, maxb, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    movi_body, idx, off = b"", b"", 4
    for f in frames:
        movi_body += b"00dc" + struct.pack("<I", len(f)) + f
        idx += b"00dc" + struct.pack("<III", 0x10, off, len(f))
        off += 8 + len(f)
    body = b"AVI " + hdrl + lst(b"movi", movi_body) + chunk(b"idx1", idx)
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_avi_writer_split_and_reader(tmp_path):
    from landiff.utils import read_mjpeg_avi, write_mjpeg_avi, write_mjpeg_avi_encoded
    images = np.stack([ref.picture(k, 34, 50, s) for s, k in enumerate(("noise", "ramps", "bars", "checker", "noise"))])
    for fps, quality in ((8, 95), (24, 60)):
        write_mjpeg_avi(images, tmp_path / "new.avi", fps=fps, quality=quality)
        _old_write_mjpeg_avi(images, tmp_path / "old.avi", fps=fps, quality=quality)
        assert (tmp_path / "new.avi").read_bytes() == (tmp_path / "old.avi").read_bytes()
        frames, got_fps = read_mjpeg_avi(tmp_path / "new.avi")
        assert got_fps == fps and frames.shape == images.shape and frames.dtype == np.uint8
    jpegs = ref.jpeg_encode(images, 90, "420")                            # the restatement's streams (odd and even lengths)
    write_mjpeg_avi_encoded(jpegs, (50, 34), tmp_path / "enc.avi", fps=30)
    frames, fps = read_mjpeg_avi(tmp_path / "enc.avi")
    assert fps == 30 and frames.shape == (5, 34, 50, 3)
    for f, j in zip(frames, jpegs):
        assert np.array_equal(f, decode(j)[0])
    (tmp_path / "bad.avi").write_bytes(b"RIFF\0\0\0\0WAVE")
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        read_mjpeg_avi(tmp_path / "bad.avi")
    import landiff.infer_video as iv
    try:
        import imageio  # noqa: F401
    except ImportError:                                                  # the project reads back the file it writes
        clip = iv.load_clip(str(tmp_path / "enc.avi"))
        assert clip.dtype.is_floating_point is False and tuple(clip.shape) == (5, 34, 50, 3) and np.array_equal(clip.numpy(), frames)


def test_refusals_before_any_launch():
    """Every refusal of the four entry points answers before a launch: safe without a GPU."""
    from landiff_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    INVALID, UNSUPPORTED = -1, -3

    def coefs(frames=p, fs=30 * 40 * 3, rs=40 * 3, tables=p, out=p, F=2, H=30, W=40, sub=420, quality=95):
        return lib.ld_jpeg_coefs_u8(frames, fs, rs, tables, out, F, H, W, sub, quality, None)

    def entropy(c=p, tables=p, segs=p, cap=1 << 20, lens=p, n=4, mcux=3, sub=420):
        return lib.ld_jpeg_entropy_i16(c, tables, segs, cap, lens, n, mcux, sub, None)

    def encode(frames=p, fs=30 * 40 * 3, rs=40 * 3, tables=p, header=p, hb=600, cw=p, sw=p, out=p, cap=1 << 40, offs=p, lens=p, F=2, H=30, W=40,
               sub=420, quality=95):
        return lib.ld_jpeg_encode_u8(frames, fs, rs, tables, header, hb, cw, sw, out, cap, offs, lens, F, H, W, sub, quality, None)

    cases = [(coefs, dict(frames=None), INVALID, b"null pointer"), (coefs, dict(tables=None), INVALID, b"null pointer"),
             (coefs, dict(out=None), INVALID, b"null pointer"), (coefs, dict(out=ctypes.c_void_p(258)), INVALID, b"aligned"),
             (coefs, dict(quality=0), INVALID, b"quality must be in 1..100, got 0"),
             (coefs, dict(quality=101), INVALID, b"quality must be in 1..100, got 101"),
             (coefs, dict(sub=422), UNSUPPORTED, b"subsampling must be 420 or 444, got 422"),
             (coefs, dict(W=8200, rs=8200 * 3, fs=30 * 8200 * 3), UNSUPPORTED, b"up to 8192 wide"),
             (coefs, dict(H=65536, fs=65536 * 120), UNSUPPORTED, b"65535 high"),
             (coefs, dict(F=0), INVALID, b"empty shape"), (coefs, dict(rs=100), INVALID, b"row_stride"),
             (coefs, dict(fs=1000), INVALID, b"frame_stride"),
             (entropy, dict(c=None), INVALID, b"null pointer"), (entropy, dict(lens=None), INVALID, b"null pointer"),
             (entropy, dict(sub=411), UNSUPPORTED, b"got 411"), (entropy, dict(mcux=513), UNSUPPORTED, b"at most 3072 blocks"),
             (entropy, dict(cap=100), INVALID, b"below the bound"), (entropy, dict(n=0), INVALID, b"empty shape"),
             (encode, dict(header=None), INVALID, b"null pointer"), (encode, dict(offs=None), INVALID, b"null pointer"),
             (encode, dict(sw=ctypes.c_void_p(260)), INVALID, b"aligned"), (encode, dict(quality=0), INVALID, b"got 0"),
             (encode, dict(quality=101), INVALID, b"got 101"), (encode, dict(sub=0), UNSUPPORTED, b"subsampling"),
             (encode, dict(W=8193, rs=8193 * 3, fs=30 * 8193 * 3), UNSUPPORTED, b"up to 8192 wide"),
             (encode, dict(cap=1000), INVALID, b"below the bound"), (encode, dict(hb=0), INVALID, b"header_bytes")]
    for fn, kw, code, msg in cases:
        assert fn(**kw) == code, (fn.__name__, kw)
        err = lib.ld_last_error()
        assert f"ld_jpeg_{fn.__name__}".encode() in err and msg in err, (kw, err)
    # the sizing rule: 20 + 63 * 26 bits a block, every byte stuffed
    size = lambda what, F=1, H=480, W=720, sub=420, hb=0: lib.ld_jpeg_size(what, F, H, W, sub, hb)
    assert (size(0), size(1), size(2)) == (45 * 30 * 6, 30, 270)
    assert size(3) == 2 * -(-270 * 1658 // 8) and size(4, F=49, hb=623) == 49 * (623 + 30 * (size(3) + 2))
    assert size(0, H=8, W=8, sub=444) == 3 and size(0, H=8, W=8) == 6 and size(1, H=17, W=33) == 2 and size(2, H=17, W=33, sub=444) == 15
    assert size(0, W=8193) == UNSUPPORTED and b"8192" in lib.ld_last_error()
    assert size(0, sub=1) == UNSUPPORTED and size(9) == INVALID and size(0, F=0) == INVALID


def test_entry_points_in_header_library_and_signatures():
    import os
    import subprocess
    from landiff_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "landiff_hip.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, ret, nargs in (("ld_jpeg_size", "int64_t", 6), ("ld_jpeg_coefs_u8", "int", 11), ("ld_jpeg_entropy_i16", "int", 9),
                             ("ld_jpeg_encode_u8", "int", 18)):
        decl = re.search(rf"\b{ret} {name}\(([^;]*)\);", hdr)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert re.search(rf" T {name}\b", syms)
    assert int(re.search(r"#define LD_JPEG_TABLE_WORDS (\d+)", hdr).group(1)) == len(E.table_words())
    assert _lib.load().ld_jpeg_size.restype is ctypes.c_int64


def test_wrappers_and_command_line_refuse_on_the_host(capsys):
    import torch
    import landiff.infer_video as iv
    from landiff_amd import _lib, ops
    x = torch.zeros(2, 10, 12, 3, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        ops.jpeg_encode_u8(x.float(), 95)
    with pytest.raises(ValueError, match=r"\[F, H, W, 3\]"):
        ops.jpeg_encode_u8(x[..., :2], 95)
    with pytest.raises(ValueError, match="quality must be an integer in 1..100, got 0"):
        ops.jpeg_coefs_u8(x, 0)
    with pytest.raises(ValueError, match="subsampling must be '420' or '444', got '422'"):
        ops.jpeg_coefs_u8(x, 95, "422")
    with pytest.raises(_lib.LandiffHipError, match="8192"):
        ops.jpeg_size(0, 1, 16, 9000, "420")
    with pytest.raises(_lib.LandiffHipError, match="GPU tensors"):               # valid arguments, host tensors: no CPU fallback
        ops.jpeg_encode_u8(x, 95)
    with pytest.raises(TypeError, match="JpegConfig"):
        E.encode_jpeg(x, 95)
    assert iv.parse_args(["--prompt", "p"]).jpeg is None
    args = iv.parse_args(["--prompt", "p", "--video_encoder", "gpu"])
    assert args.jpeg == E.JpegConfig(95, "420")
    assert iv.parse_args(["--prompt", "p", "--video_encoder", "gpu", "--jpeg_quality", "80"]).jpeg.quality == 80
    for argv, msg in ((["--jpeg_quality", "80"], "--jpeg_quality goes with --video_encoder gpu"),
                      (["--video_encoder", "host", "--jpeg_quality", "80"], "--jpeg_quality goes with --video_encoder gpu"),
                      (["--video_encoder", "gpu", "--jpeg_quality", "0"], "quality must be an integer in 1..100, got 0"),
                      (["--video_encoder", "nvenc"], "invalid choice")):
        with pytest.raises(SystemExit):
            iv.parse_args(["--prompt", "p"] + argv)
        assert msg in capsys.readouterr().err
