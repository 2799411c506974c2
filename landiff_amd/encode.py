"""The encode stage: uint8 RGB frames on the device -> baseline JPEG streams, in integer arithmetic.

What a user gets from a video model is a file.  This stage makes the frames of a Motion-JPEG AVI (or stills) where the frames
already are: colour conversion, DCT, quantisation and the Huffman coder run on the device (csrc/ld_jpeg.hip), one restart interval
per MCU row so that every MCU row of every frame is coded independently, and only the streams cross the bus.

This module is the one place the tables are stated: the base quantisation tables and the Annex K Huffman tables below were read
from the DQT and DHT segments of a file PIL (libjpeg-turbo) wrote at quality 50 with optimize=False -- tests/test_jpeg_host.py
reads them again and compares -- and the kernels receive them as one device array (device_tables).  The rule itself is stated in
DESIGN 8.12 and restated in numpy in tests/jpeg_ref.py; the kernels are held to that bit for bit.

Rate control (JpegRateConfig, csrc/ld_jpeg_rate.hip, DESIGN 8.15, restated in tests/jpeg_rate_ref.py): the quality is searched on
the device, by a stated bisection over exact stream sizes, so that every frame or the whole clip fits a byte budget; off unless
asked for.

Nothing here runs unless it is asked for.  What quality-95 Motion-JPEG of a trained checkpoint's output looks like is not measured.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

SUBSAMPLINGS = ("420", "444")
MAX_WIDTH, MAX_HEIGHT = 8192, 65535          # kMaxWidth / kMaxHeight of csrc/ld_jpeg_dev.h
TABLE_SOURCE = "Annex K tables as written by PIL (libjpeg-turbo) at quality 50, optimize=False"

# ---- the tables, as the DQT / DHT segments hold them ----
# base quantisation tables (quality 50), in the zigzag order of the DQT segment
BASE_QUANT_LUMA = (16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61,
                   60, 57, 51, 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113,
                   121, 112, 100, 120, 92, 101, 103, 99)
BASE_QUANT_CHROMA = (17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99) + (99,) * 48
# Huffman tables: BITS (codes of length 1..16) and HUFFVAL (the symbols in code order)
DC_LUMA_BITS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
DC_CHROMA_BITS = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
DC_VALS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)                      # both DC tables
AC_LUMA_BITS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125)
AC_LUMA_VALS = (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82,
                209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68,
                69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119,
                120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165,
                166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210,
                211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246,
                247, 248, 249, 250)
AC_CHROMA_BITS = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119)
AC_CHROMA_VALS = (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51,
                  82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58,
                  67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117,
                  118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
                  162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198,
                  199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242,
                  243, 244, 245, 246, 247, 248, 249, 250)
# (table class << 4 | table id, BITS, HUFFVAL) in the order the DHT segments are written
HUFFMAN_TABLES = ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                  (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS))

# ---- the arithmetic's constants ----
# sqrt(8) x the 8-point DCT-II in 13-bit fixed point (two passes give 8 x the 2-D coefficient, which is what the quantiser takes):
# K[0][x] = DCT_CONST[0] = 8192, K[u][x] = +-DCT_CONST[k] = round(8192 sqrt(2) cos(k pi / 16)); k = 0 and k = 4 are exact, so the
# DC term is the exact sum of the samples
DCT_CONST = (8192, 11363, 10703, 9633, 8192, 6436, 4433, 2260)
DCT_ROW_BITS, DCT_COL_BITS = 9, 17             # the shifts after the two passes: 13 -> 4 and 4 + 13 -> 0 fractional bits


def dct_matrix() -> list:
    """K[u][x] = round(8192 sqrt(8) a(u) cos((2 x + 1) u pi / 16)), a(0) = 1 / sqrt(8), else 1 / 2 -- by symmetry +-DCT_CONST[k]."""
    K = [[DCT_CONST[0]] * 8]
    for u in range(1, 8):
        row = []
        for x in range(8):
            k = ((2 * x + 1) * u) % 32
            k = 32 - k if k > 16 else k            # cos(2 pi - t) = cos t
            row.append(DCT_CONST[k] if k < 8 else -DCT_CONST[16 - k])      # cos(pi - t) = -cos t; k = 8 does not occur
        K.append(row)
    return K


def zigzag_order() -> list:
    """zigzag position -> natural index 8 v + u: the anti-diagonals of the block, alternating direction."""
    order = []
    for d in range(15):
        cells = [(v, d - v) for v in range(8) if 0 <= d - v < 8]
        order += [8 * v + u for v, u in (cells if d % 2 else reversed(cells))]
    return order


def quant_tables(quality: int):
    """IJG's rule in integers: s = 5000 // q below 50, else 200 - 2 q; t = clamp((base s + 50) // 100, 1, 255).  -> (luma,
    chroma), 64 ints each in zigzag order."""
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= quality <= 100:
        raise ValueError(f"quant_tables: quality must be an integer in 1..100, got {quality!r}")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    scale = lambda base: tuple(min(max((b * s + 50) // 100, 1), 255) for b in base)
    return scale(BASE_QUANT_LUMA), scale(BASE_QUANT_CHROMA)


def huffman_codes(bits, vals) -> dict:
    """Annex C: symbol -> (code, length), codes of one length consecutive in HUFFVAL order."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def table_words() -> list:
    """The LD_JPEG_TABLE_WORDS int32 words the kernels take (include/landiff_hip.h states the layout)."""
    order = zigzag_order()
    pos = [0] * 64
    for z, n in enumerate(order):
        pos[n] = z
    words = [k for row in dct_matrix() for k in row] + list(BASE_QUANT_LUMA) + list(BASE_QUANT_CHROMA) + pos
    for _, bits, vals in (HUFFMAN_TABLES[0], HUFFMAN_TABLES[2]):
        codes = huffman_codes(bits, vals)
        words += [codes[s][0] | codes[s][1] << 16 if s in codes else 0 for s in range(16)]
    for _, bits, vals in (HUFFMAN_TABLES[1], HUFFMAN_TABLES[3]):
        codes = huffman_codes(bits, vals)
        words += [codes[s][0] | codes[s][1] << 16 if s in codes else 0 for s in range(256)]
    assert len(words) == 800
    return words


_DEVICE_TABLES: dict = {}


def device_tables(device):
    """table_words() as an int32 tensor on `device` (made once per device)."""
    import torch
    key = str(device)
    if key not in _DEVICE_TABLES:
        _DEVICE_TABLES[key] = torch.tensor(table_words(), dtype=torch.int32).to(device)
    return _DEVICE_TABLES[key]


@dataclass(frozen=True)
class JpegConfig:
    """quality: IJG's 1..100 (95 is what the host writer uses).  subsampling: "420" (chroma halved in both axes, what PIL does at
    quality 95) or "444"."""
    quality: int = 95
    subsampling: str = "420"

    def __post_init__(self):
        if isinstance(self.quality, bool) or not isinstance(self.quality, int) or not 1 <= self.quality <= 100:
            raise ValueError(f"JpegConfig: quality must be an integer in 1..100, got {self.quality!r}")
        if self.subsampling not in SUBSAMPLINGS:
            raise ValueError(f"JpegConfig: subsampling must be one of {SUBSAMPLINGS}, got {self.subsampling!r}")


def mcu_size(subsampling: str) -> int:
    return 16 if subsampling == "420" else 8


def jpeg_header(H: int, W: int, quality: int, subsampling: str) -> bytes:
    """SOI, APP0 (JFIF 1.1, no density), two DQT, SOF0, four DHT, DRI (one MCU row), SOS: the bytes before the entropy-coded data,
    equal for every frame of a clip."""
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"jpeg_header: subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}")
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"jpeg_header: a JPEG is 1..65535 pixels per axis, got {H} x {W}")
    seg = lambda marker, body: bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body
    luma, chroma = quant_tables(quality)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += seg(0xDB, bytes([0]) + bytes(luma)) + seg(0xDB, bytes([1]) + bytes(chroma))
    ysamp = 0x22 if subsampling == "420" else 0x11
    out += seg(0xC0, bytes([8]) + struct.pack(">HH", H, W) + bytes([3, 1, ysamp, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in HUFFMAN_TABLES:
        out += seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, struct.pack(">H", -(-W // mcu_size(subsampling))))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


JPEG_HEADER_BYTES = 629                       # len(jpeg_header(...)) for any size, quality and subsampling this stage writes


def jpeg_dqt_offsets() -> tuple:
    """Where jpeg_header's two 64-byte quantisation tables (luma, chroma) lie: after SOI (2), APP0 (18) and the DQT's marker, length
    and table id (5); the chroma DQT follows the luma body.  Headers of two qualities differ in these 128 bytes only, which is what
    lets the rate-controlled writing pass work from one header template."""
    luma = 2 + 18 + 5
    return luma, luma + 64 + 5


def rate_rounds(q_min: int, q_max: int) -> int:
    """The rounds of the rate search: 1 + ceil(log2(q_max - q_min + 1)) (8 for 1..95 and for 1..100), in integers."""
    if not 1 <= q_min <= q_max <= 100:
        raise ValueError(f"rate_rounds: 1 <= q_min <= q_max <= 100, got {q_min!r}, {q_max!r}")
    return 1 + (q_max - q_min).bit_length()


@dataclass(frozen=True)
class JpegRateConfig:
    """A byte budget for encode_jpeg, exactly one of: frame_bytes (every stream <= it; each frame searches its own
    quality) and clip_bytes (the streams of the call together <= it; one quality for all frames).  JpegConfig.quality is the
    search's ceiling and min_quality its floor.  A frame that does not fit at the floor is encoded there and reported over budget."""
    frame_bytes: int | None = None
    clip_bytes: int | None = None
    min_quality: int = 1

    def __post_init__(self):
        if (self.frame_bytes is None) == (self.clip_bytes is None):
            raise ValueError(f"JpegRateConfig: give exactly one of frame_bytes and clip_bytes, got {self.frame_bytes!r} and {self.clip_bytes!r}")
        for name in ("frame_bytes", "clip_bytes"):
            v = getattr(self, name)
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 1):
                raise ValueError(f"JpegRateConfig: {name} must be an integer >= 1, got {v!r}")
        if isinstance(self.min_quality, bool) or not isinstance(self.min_quality, int) or not 1 <= self.min_quality <= 100:
            raise ValueError(f"JpegRateConfig: min_quality must be an integer in 1..100, got {self.min_quality!r}")

    @property
    def mode(self) -> str:
        return "frame" if self.clip_bytes is None else "clip"

    @property
    def budget(self) -> int:
        return self.frame_bytes if self.clip_bytes is None else self.clip_bytes


def encode_jpeg(frames, cfg: JpegConfig | None = None, return_device: bool = False, rate: JpegRateConfig | None = None,
                return_rate: bool = False):
    """uint8 frames [F, H, W, 3] on the device (the rows may be strided, as a crop of a wider clip is) -> list of F `bytes`, each a
    complete baseline JPEG (ops.jpeg_encode_u8: four launches; then one device-to-host copy of the lengths and one of the streams).
    return_device: (stream buffer uint8 on the device, offsets int64 [F], lengths int64 [F] on the host) instead.
    rate (a JpegRateConfig): the qualities are searched on the device so that the streams fit the budget (ops.jpeg_encode_rate_u8,
    DESIGN 8.15; cfg.quality is the ceiling); no frame crosses the bus before the answer is known.  return_rate (with rate): the
    result is followed by dict(qualities [F], over_budget [F] of bool, trials [R][F][2] = the (quality, size) of every trial; (0, 0)
    where a frame had finished), which arrive in the same copy as the lengths."""
    import torch
    from . import ops
    cfg = JpegConfig() if cfg is None else cfg
    if not isinstance(cfg, JpegConfig):
        raise TypeError(f"encode_jpeg: expected a JpegConfig, got {type(cfg).__name__}")
    if rate is not None and not isinstance(rate, JpegRateConfig):
        raise TypeError(f"encode_jpeg: rate must be a JpegRateConfig or None, got {type(rate).__name__}")
    if return_rate and rate is None:
        raise ValueError("encode_jpeg: return_rate goes with rate")
    info = None
    if rate is None:
        buf, offsets, lengths = ops.jpeg_encode_u8(frames, cfg.quality, cfg.subsampling)
        table = torch.stack([offsets, lengths]).cpu()
    else:
        if rate.min_quality > cfg.quality:
            raise ValueError(f"encode_jpeg: min_quality {rate.min_quality} is above the ceiling, JpegConfig.quality = {cfg.quality}")
        buf, table = ops.jpeg_encode_rate_u8(frames, cfg.quality, cfg.subsampling, frame_bytes=rate.frame_bytes,
                                             clip_bytes=rate.clip_bytes, q_min=rate.min_quality)
        table = table.cpu()
        F = table.shape[1]
        info = dict(qualities=table[2].tolist(), over_budget=[bool(v) for v in table[3].tolist()],
                    trials=table[4:].reshape(-1, F, 2).tolist())
    offs, lens = table[0].tolist(), table[1].tolist()
    total = offs[-1] + lens[-1]
    if return_device:
        res = (buf[:total], table[0], table[1])
    else:
        raw = buf[:total].cpu().numpy().tobytes()
        res = [raw[o:o + n] for o, n in zip(offs, lens)]
    if return_rate:
        return (*res, info) if return_device else (res, info)
    return res


def rate_report(rate: JpegRateConfig, cfg: JpegConfig, info: dict) -> dict:
    """encode_report's `rate` entry: the mode, the budget, the floor and the ceiling, the rounds queued and the trials the slowest
    frame took, min / mean / max of the chosen qualities, and the frames that do not fit even at the floor."""
    q = info["qualities"]
    return dict(mode=rate.mode, budget=rate.budget, min_quality=rate.min_quality, max_quality=cfg.quality,
                quality=dict(min=min(q), mean=sum(q) / len(q), max=max(q)),
                over_budget_frames=[f for f, o in enumerate(info["over_budget"]) if o], rounds=len(info["trials"]),
                trials_used=max(sum(1 for row in info["trials"] if row[f][0]) for f in range(len(q))))


def encode_report(jpegs, cfg: JpegConfig, rate: JpegRateConfig | None = None, rate_info: dict | None = None) -> dict:
    """What <name>_encode.json holds.  rate, rate_info (encode_jpeg's return_rate): a rate-controlled encode; `quality` is then the
    search's ceiling and the chosen qualities are under `rate`."""
    sizes = [len(j) for j in jpegs]
    rep = dict(encoder="gpu", quality=cfg.quality, subsampling=cfg.subsampling, frames=len(sizes), total_bytes=sum(sizes),
               bytes_per_frame=dict(min=min(sizes), mean=sum(sizes) / len(sizes), max=max(sizes)), restart_interval="one MCU row",
               table_source=TABLE_SOURCE)
    if rate is not None:
        rep["rate"] = rate_report(rate, cfg, rate_info)
    return rep
