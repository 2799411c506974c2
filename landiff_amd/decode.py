"""The decode stage: baseline JPEG streams -> uint8 RGB frames on the device, equal to PIL's decode byte for byte.

The way back in from a file this project wrote (or PIL wrote): the host parses the headers up to SOS -- pure Python, parse_jpeg --
and refuses what the kernels do not decode before anything is launched; the compressed bytes cross the bus once, and the restart
markers, the Huffman decode, the inverse DCT, the chroma upsampling and the colour conversion run on the device
(csrc/ld_jpeg_dec.hip).  libjpeg's decode is integer arithmetic from the coefficients on; DESIGN 8.13 states it, tests/jpeg_dec_ref.py
restates it in numpy, and the kernels are held to that bit for bit.

Nothing here runs unless it is asked for.
"""
from __future__ import annotations

import re
import struct
from dataclasses import dataclass

from .encode import MAX_HEIGHT, MAX_WIDTH

STATUS = ("OK", "BAD_CODE", "OVERFLOW", "OVERRUN", "RANGE", "MARKERS")           # LD_JPEG_DEC_* of include/landiff_hip.h
TABLE_WORDS = 3456                                                               # LD_JPEG_DEC_TABLE_WORDS
_LIMIT, _VALS = 0, 32                                                            # within one Huffman table's 544 words
LATER = "4:2:2, other sampling factors and greyscale are later work"
ENTROPY_ROUTES = ("segment", "sync", "auto")
SUB_BYTES = (64, 128, 256, 512, 1024)                                            # what ld_jpeg_dec_sync_size accepts
MAX_ROUNDS = 4096
# "auto" takes the sync route when a segment holds more than this many subsequences on average.  Measured (DESIGN 8.14,
# profiles/jpeg_decode_sync.txt): on noise frames at sub_bytes 256 the sync route loses at 17.6 subsequences a segment (0.65 x) and
# wins at 52.8 (1.41 x); nothing between was measured on noise, so the threshold sits where no measured case loses.
AUTO_SUBSEQUENCES_PER_SEGMENT = 32


@dataclass(frozen=True)
class JpegInfo:
    """What the headers of one baseline JPEG say.  quant: per component its 64 quantisers in zigzag order (as DQT holds them);
    huffman: per component ((BITS, HUFFVAL) of its DC table, (BITS, HUFFVAL) of its AC table); restart_interval in MCUs, 0 = none;
    scan_offset: where the entropy-coded data starts."""
    width: int
    height: int
    subsampling: str
    quant: tuple
    huffman: tuple
    restart_interval: int
    scan_offset: int

    @property
    def mcus(self) -> int:
        m = 16 if self.subsampling == "420" else 8
        return -(-self.width // m) * -(-self.height // m)

    @property
    def segments(self) -> int:
        return -(-self.mcus // self.restart_interval) if self.restart_interval else 1


class _Truncated(Exception):
    """The bytes end inside the headers (a prefix was parsed: more is needed)."""


def _valid_huffman(bits, vals) -> bool:
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > 1 << length:
            return False
        code <<= 1
    return sum(bits) == len(vals) <= 256


def parse_jpeg(data, frame=None, _prefix: bool = False) -> JpegInfo:
    """The headers of one JPEG stream up to SOS -> JpegInfo, in pure Python.  Raises ValueError naming the frame and the reason for
    everything the decode stage refuses: anything but SOF0 at 8 bits, sampling other than 4:2:0 / 4:4:4 of three components, 16-bit
    DQT, a scan that is not the one interleaved scan 0..63, an Adobe segment with transform 0, a missing table, SOS before SOF."""
    who = "parse_jpeg" if frame is None else f"frame {frame}"

    def refuse(why):
        raise ValueError(f"{who}: {why}")

    def need(n):
        if n > len(data):
            if _prefix:
                raise _Truncated()
            refuse("the stream ends inside its headers")

    need(2)
    if bytes(data[:2]) != b"\xff\xd8":
        refuse("not a JPEG stream (no SOI)")
    quant, huff, sof, ri, i = {}, {}, None, 0, 2
    while True:
        need(i + 2)
        if data[i] != 0xFF:
            refuse(f"byte {i}: a marker was expected")
        m = data[i + 1]
        if m == 0xFF:                                                            # a fill byte before a marker
            i += 1
            continue
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            refuse(f"marker 0x{m:02X} inside the headers")
        if m == 0xD9:
            refuse("EOI before any scan")
        need(i + 4)
        n = struct.unpack(">H", bytes(data[i + 2:i + 4]))[0]
        if n < 2:
            refuse(f"marker 0x{m:02X}: a segment length below 2")
        need(i + 2 + n)
        body = bytes(data[i + 4:i + 2 + n])
        i += 2 + n
        if m == 0xC0:
            if sof is not None:
                refuse("a second SOF0")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                refuse("a malformed SOF0")
            if body[0] != 8:
                refuse(f"{body[0]}-bit precision is not supported (8-bit only)")
            h, w = struct.unpack(">HH", body[1:5])
            comps = [(body[6 + 3 * k], body[7 + 3 * k], body[8 + 3 * k]) for k in range(body[5])]
            if len(comps) == 1:
                refuse(f"greyscale is not supported ({LATER})")
            if len(comps) != 3:
                refuse(f"{len(comps)} components are not supported (three, read as YCbCr)")
            samp = tuple(c[1] for c in comps)
            if samp not in ((0x22, 0x11, 0x11), (0x11, 0x11, 0x11)):
                refuse("sampling factors " + " ".join(f"{s >> 4}x{s & 15}" for s in samp) + f" are not supported: 4:2:0 (2x2 1x1 1x1) "
                       f"and 4:4:4 only ({LATER})")
            if h == 0 or w == 0:
                refuse("a frame size of 0 (DNL) is not supported")
            sof = (w, h, "420" if samp[0] == 0x22 else "444", comps)
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8):
            kinds = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC9: "arithmetic-coded", 0xCA: "arithmetic-coded progressive",
                     0xCC: "arithmetic conditioning"}
            refuse(f"{kinds.get(m, 'SOF' + str(m - 0xC0))} JPEG (marker 0x{m:02X}) is not supported: baseline SOF0 only")
        elif m == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                if pq != 0:
                    refuse("a 16-bit DQT is not supported (8-bit quantisers only)")
                if tq > 3 or k + 65 > len(body):
                    refuse("a malformed DQT")
                quant[tq] = tuple(body[k + 1:k + 65])
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(body):
                if k + 17 > len(body):
                    refuse("a malformed DHT")
                tc, th, bits = body[k] >> 4, body[k] & 15, tuple(body[k + 1:k + 17])
                vals = tuple(body[k + 17:k + 17 + sum(bits)])
                if tc > 1 or th > 3 or not _valid_huffman(bits, vals):
                    refuse("a malformed DHT")
                huff[(tc, th)] = (bits, vals)
                k += 17 + sum(bits)
        elif m == 0xDD:
            if len(body) != 2:
                refuse("a malformed DRI")
            ri = struct.unpack(">H", body)[0]
        elif m == 0xEE:
            if body[:5] == b"Adobe" and len(body) >= 12 and body[11] == 0:
                refuse("an Adobe APP14 segment with transform 0 (RGB or CMYK data, not YCbCr) is not supported")
        elif m == 0xDA:
            if sof is None:
                refuse("SOS before SOF")
            w, h, sub, comps = sof
            if len(body) < 1 or len(body) != 4 + 2 * body[0]:
                refuse("a malformed SOS")
            if body[0] != 3 or [body[1 + 2 * k] for k in range(3)] != [c[0] for c in comps]:
                refuse("several scans are not supported (one interleaved scan of the three components)")
            if tuple(body[7:10]) != (0, 63, 0):
                refuse("a scan other than Ss = 0, Se = 63, Ah = Al = 0 is not supported")
            qs, hs = [], []
            for k, c in enumerate(comps):
                td, ta = body[2 + 2 * k] >> 4, body[2 + 2 * k] & 15
                if c[2] not in quant:
                    refuse(f"a missing table: quantisation table {c[2]}")
                if (0, td) not in huff or (1, ta) not in huff:
                    refuse(f"a missing table: Huffman table DC {td} or AC {ta}")
                qs.append(quant[c[2]])
                hs.append((huff[(0, td)], huff[(1, ta)]))
            return JpegInfo(w, h, sub, tuple(qs), tuple(hs), ri, i)
        # every other segment (APPn, COM, ...) is skipped


_SCAN_END = re.compile(rb"\xff[^\x00\xd0-\xd7]")


def check_scan(data: bytes, info: JpegInfo, frame=None) -> None:
    """What can be said of the bytes after SOS without decoding them: they end with EOI, hold no fill bytes and no second scan."""
    who = "check_scan" if frame is None else f"frame {frame}"
    m = _SCAN_END.search(data, info.scan_offset)
    if m is None:
        raise ValueError(f"{who}: a frame without EOI")
    nxt = data[m.start() + 1]
    if nxt == 0xFF:
        raise ValueError(f"{who}: fill bytes (0xFF 0xFF) inside the scan are not supported")
    if nxt != 0xD9:
        raise ValueError(f"{who}: marker 0x{nxt:02X} after the scan: several scans are not supported")


def huffman_words(bits, vals) -> list:
    """One Huffman table as the 544 words the kernels take (include/landiff_hip.h): limit[16], offset[16], HUFFVAL[256] and the
    8-bit look-ahead table [256]."""
    if not _valid_huffman(bits, vals):
        raise ValueError("huffman_words: BITS / HUFFVAL are no Huffman table")
    limit, offset, look = [0] * 16, [0] * 16, [0] * 256
    code, k = 0, 0
    for length in range(1, 17):
        offset[length - 1] = k - code
        for _ in range(bits[length - 1]):
            if length <= 8:
                lo = code << (8 - length)
                for p in range(lo, lo + (1 << (8 - length))):
                    look[p] = length << 8 | vals[k]
            code += 1
            k += 1
        limit[length - 1] = code << (16 - length)
        code <<= 1
    return limit + offset + list(vals) + [0] * (256 - len(vals)) + look


def huffman_from_words(words) -> tuple:
    """The inverse of huffman_words on its first 288 words: (BITS, HUFFVAL)."""
    bits, code = [], 0
    for length in range(1, 17):
        n = (words[_LIMIT + length - 1] >> (16 - length)) - code
        bits.append(n)
        code = (code + n) << 1
    return tuple(bits), tuple(words[_VALS:_VALS + sum(bits)])


def decode_tables(info: JpegInfo) -> list:
    """The TABLE_WORDS int32 words of one table set: the three components' quantisers (zigzag order), then their DC and AC Huffman
    tables."""
    words = [q for comp in info.quant for q in comp]
    for dc, ac in info.huffman:
        words += huffman_words(*dc) + huffman_words(*ac)
    assert len(words) == TABLE_WORDS
    return words


def _device_headers(buf, offsets, lengths, sel):
    """The headers of the selected frames of a device stream buffer: a prefix of every frame is copied back (doubled until every
    SOS is inside it); the entropy-coded data past it never is."""
    import torch
    n = 1024
    offs = torch.as_tensor([offsets[k] for k in sel], dtype=torch.int64)
    most = max(lengths[k] for k in sel)
    while True:
        idx = (offs[:, None] + torch.arange(n)[None, :]).clamp_(max=buf.numel() - 1)
        rows = buf[idx.to(buf.device)].cpu().numpy()
        try:
            return [parse_jpeg(rows[r, :min(n, lengths[k])].tobytes(), frame=k, _prefix=n < lengths[k]) for r, k in enumerate(sel)]
        except _Truncated:
            if n >= most:
                raise ValueError("decode_jpeg: a stream ends inside its headers")
            n *= 2


def check_entropy(entropy, sub_bytes, max_rounds, who="decode_jpeg") -> None:
    """The refusals of the entropy route's arguments, on the host."""
    if entropy not in ENTROPY_ROUTES:
        raise ValueError(f"{who}: entropy must be one of {', '.join(ENTROPY_ROUTES)}, got {entropy!r}")
    if isinstance(sub_bytes, bool) or not isinstance(sub_bytes, int) or sub_bytes not in SUB_BYTES:
        raise ValueError(f"{who}: sub_bytes must be a power of two in 64 .. 1024, got {sub_bytes!r}")
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, int) or not 1 <= max_rounds <= MAX_ROUNDS:
        raise ValueError(f"{who}: max_rounds must be in 1 .. {MAX_ROUNDS}, got {max_rounds!r}")


def entropy_route(infos, sizes, sub_bytes: int = 256) -> str:
    """What entropy="auto" decodes a call with, from what the host knows: "sync" when the mean bytes per restart segment (the scans'
    bytes over the segments the headers promise) exceed AUTO_SUBSEQUENCES_PER_SEGMENT x sub_bytes, else "segment".  A pure function."""
    if not infos or len(infos) != len(sizes):
        raise ValueError("entropy_route: one size per stream is expected")
    scan = sum(max(int(n) - i.scan_offset, 0) for i, n in zip(infos, sizes))
    return "sync" if scan > AUTO_SUBSEQUENCES_PER_SEGMENT * sub_bytes * sum(i.segments for i in infos) else "segment"


def decode_jpeg(jpegs, device=None, frames=None, return_coefs: bool = False, out=None, report: dict | None = None,
                entropy: str = "segment", sub_bytes: int = 256, max_rounds: int = 32):
    """Baseline JPEG streams of one size -> uint8 frames [F, H, W, 3] on the device, equal to PIL's decode.

    jpegs: a list of `bytes` on the host (their bytes are uploaded once), or the (buffer, offsets, lengths) that
    encode_jpeg(return_device=True) returns (only a prefix holding the headers is copied back).  frames: the indices to decode, in
    that order (default: all).  out: a uint8 [F, H, W, 3] on the device to write into (rows and frames may be strided).
    return_coefs: (frames, coefficients int16 [F, blocks, 64] in ops.jpeg_coefs_u8's layout).  report: a dict that receives
    decode_report's figures.  Four launches, then one device-to-host copy: the segments' status words; any that is not 0 raises
    ValueError with the frame, the segment and the status name, and no pixels are returned.
    entropy: "segment" (one lane per restart segment: the launches above), "sync" (one lane per sub_bytes bytes of a segment, for
    streams without restart markers; at most max_rounds rounds, then the segment route for what has not settled: DESIGN 8.14; its
    sync_info words come back in the same copy as the status words) or "auto" (entropy_route decides for the call)."""
    import torch
    from . import ops
    check_entropy(entropy, sub_bytes, max_rounds)
    triple = isinstance(jpegs, tuple) and len(jpegs) == 3 and isinstance(jpegs[0], torch.Tensor)
    count = len(jpegs[1]) if triple else len(jpegs)
    sel = list(range(count)) if frames is None else [int(k) for k in frames]
    if not sel or any(not 0 <= k < count for k in sel):
        raise ValueError(f"decode_jpeg: frames must name some of the {count} streams, got {sel}")
    if triple:
        buf = jpegs[0]
        offsets, lengths = ([int(v) for v in t.tolist()] if isinstance(t, torch.Tensor) else [int(v) for v in t] for t in jpegs[1:])
        if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous() or len(offsets) != len(lengths):
            raise ValueError("decode_jpeg: (buffer uint8 [n], offsets [F], lengths [F]) is expected")
        if any(offsets[k] < 0 or lengths[k] < 4 or offsets[k] + lengths[k] > buf.numel() for k in sel):
            raise ValueError("decode_jpeg: a stream's offset and length leave the buffer")
        infos = _device_headers(buf, offsets, lengths, sel)
        data, starts, sizes = buf, [offsets[k] for k in sel], [lengths[k] for k in sel]
    else:
        if device is None:
            raise ValueError("decode_jpeg: streams on the host need the device to decode on")
        if any(not isinstance(jpegs[k], (bytes, bytearray)) for k in sel):
            raise TypeError("decode_jpeg: the streams must be bytes")
        infos = [parse_jpeg(jpegs[k], frame=k) for k in sel]
        for k, info in zip(sel, infos):
            check_scan(jpegs[k], info, frame=k)
        sizes = [len(jpegs[k]) for k in sel]
        starts = [0]
        for n in sizes[:-1]:
            starts.append(starts[-1] + n)
        data = None
    first = infos[0]
    for k, info in zip(sel, infos):
        if (info.width, info.height, info.subsampling) != (first.width, first.height, first.subsampling):
            raise ValueError(f"frame {k}: {info.width} x {info.height} at {info.subsampling}, frame {sel[0]} is {first.width} x "
                             f"{first.height} at {first.subsampling}: mixed sizes or subsamplings within one clip are not supported")
    H, W, sub = first.height, first.width, first.subsampling
    if W > MAX_WIDTH or H > MAX_HEIGHT:
        raise ValueError(f"frame {sel[0]}: frames up to {MAX_WIDTH} wide and {MAX_HEIGHT} high are supported, got {W} x {H}")
    sets, tset = {}, []
    for info in infos:                                                           # distinct table sets are uploaded once each
        tset.append(sets.setdefault((info.quant, info.huffman), len(sets)))
    words = [decode_tables(next(i for i, t in zip(infos, tset) if t == s)) for s in range(len(sets))]
    if torch.device(device if data is None else data.device).type != "cuda":
        from ._lib import LandiffHipError
        raise LandiffHipError("decode_jpeg: the decode stage needs GPU tensors (no CPU fallback)")
    if data is None:
        data = torch.frombuffer(bytearray(b"".join(bytes(jpegs[k]) for k in sel)), dtype=torch.uint8).to(device)
    dev = data.device
    small = torch.tensor([[s + i.scan_offset, n - i.scan_offset] for s, n, i in zip(starts, sizes, infos)], dtype=torch.int64).to(dev)
    meta = torch.tensor([[i.restart_interval for i in infos], tset], dtype=torch.int32).to(dev)
    tables = torch.tensor(words, dtype=torch.int32).to(dev)
    rows = max(i.segments for i in infos)
    with torch.cuda.device(dev):
        seg, finfo = ops.jpeg_find_segments(data, small, meta[0], rows, H, W, sub)
        route = entropy_route(infos, sizes, sub_bytes) if entropy == "auto" else entropy
        sync = None
        if route == "sync":
            coefs, status, sync = ops.jpeg_decode_entropy_sync(data, seg, finfo, meta[0], tables, meta[1], H, W, sub, sub_bytes, max_rounds,
                                                               scan_bytes=sum(n - i.scan_offset for n, i in zip(sizes, infos)))
        else:
            coefs, status = ops.jpeg_decode_entropy(data, seg, finfo, meta[0], tables, meta[1], H, W, sub)
        pixels = ops.jpeg_decode_rgb(coefs, tables, meta[1], H, W, sub, out=out)
        if sync is None:
            bad = status.cpu()                                                   # the one device-to-host copy
        else:                                                                    # (still one: the sync_info words ride along)
            both = torch.cat([status[..., None], sync], dim=-1).cpu()
            bad, sync = both[..., 0], both[..., 1:]
    if bool(bad.any()):
        r, s = (int(v) for v in bad.nonzero()[0])
        code = int(bad[r, s])
        raise ValueError(f"decode_jpeg: frame {sel[r]} segment {s}: {STATUS[code] if 0 <= code < len(STATUS) else code}")
    if report is not None:
        report.update(decode_report(infos, sizes, entropy=route, sub_bytes=sub_bytes, sync_info=sync))
    return (pixels, coefs) if return_coefs else pixels


def decode_report(infos, sizes, entropy: str = "segment", sub_bytes: int = 256, sync_info=None) -> dict:
    """What <name>_decode.json holds: infos the decoded frames' JpegInfo, sizes their streams' bytes; entropy the route that
    decoded them, and for "sync" its sub_bytes and sync_info [F, rows, 2] (the rows a frame uses are counted)."""
    first = infos[0]
    segs = [i.segments for i in infos]
    rounds, fallen = [], 0
    if sync_info is not None:
        for f, i in enumerate(infos):
            rounds += [int(v) for v in sync_info[f, :i.segments, 0]]
            fallen += int(sync_info[f, :i.segments, 1].sum())
    extra = dict(entropy=entropy, sub_bytes=sub_bytes if entropy == "sync" else None,
                 rounds=dict(max=max(rounds), mean=sum(rounds) / len(rounds)) if rounds else None,
                 segments_fallen_back=fallen if entropy == "sync" else None)
    return dict(decoder="gpu", frames=len(infos), width=first.width, height=first.height, subsampling=first.subsampling,
                total_bytes=sum(sizes), bytes_per_frame=dict(min=min(sizes), mean=sum(sizes) / len(sizes), max=max(sizes)),
                table_sets=len({(i.quant, i.huffman) for i in infos}), restart_intervals=sorted({i.restart_interval for i in infos}),
                segments_per_frame=dict(min=min(segs), max=max(segs)),
                frames_without_restarts=sum(1 for i in infos if i.segments == 1 and i.mcus > 1),
                rule="libjpeg islow inverse DCT, triangle chroma upsampling, 16-bit colour constants (DESIGN 8.13)", **extra)
