"""The decode stage's rule restated in numpy and plain Python, for the tests of landiff_amd/decode.py and
csrc/ld_jpeg_dec.hip.

Written from the rule's text, int64 throughout, and built differently from the kernels on purpose: the scan is walked byte by byte
in order, a segment is one string of '0' / '1' characters and a Huffman table a dict from code strings to symbols, the inverse DCT
is two stacked passes over all blocks of a frame at once, and the chroma is upsampled by shifted whole planes.  The headers are
read by landiff_amd.decode.parse_jpeg (host code, tested against PIL's own files in tests/test_jpeg_dec_host.py).
"""
import struct

import numpy as np

import jpeg_ref
from landiff_amd import decode as D
from landiff_amd import encode as E

ZIGZAG = np.array(E.zigzag_order())                           # zigzag position -> 8 v + u
OK, BAD_CODE, OVERFLOW, OVERRUN, RANGE, MARKERS = range(6)


# ---- segments ----
def find_segments(data, start, length, ri, mcus, rows, frame=0):
    """The bytes data[start : start + length] walked in order -> (table int64 [rows, 5] = (frame, start, length, first MCU, MCU
    count), info int64 [3] = (markers, numbered in order, length of the entropy-coded data))."""
    p = data[start:start + length]
    n, i, marks, end = len(p), 0, [], len(p)
    while i < n:
        if p[i] != 0xFF:
            i += 1
        elif i + 1 < n and p[i + 1] == 0:
            i += 2
        elif i + 1 < n and 0xD0 <= p[i + 1] <= 0xD7:
            marks.append((i, p[i + 1] - 0xD0))
            i += 2
        else:
            end = i
            break
    nf = min(-(-mcus // ri) if ri > 0 else 1, rows)
    table = np.zeros((rows, 5), dtype=np.int64)
    table[:, 0] = frame
    bounds = [0] + [m[0] + 2 for m in marks]                 # where segment s starts
    for s in range(nf):
        table[s, 3] = s * ri if ri > 0 else 0
        table[s, 4] = min(ri, mcus - s * ri) if ri > 0 else mcus
        if s <= len(marks):
            table[s, 1] = start + bounds[s]
            table[s, 2] = (marks[s][0] if s < len(marks) else end) - bounds[s]
    order = all(m[1] == (k & 7) for k, m in enumerate(marks))
    return table, np.array([len(marks), int(order), end], dtype=np.int64)


# ---- entropy decode ----
def code_book(bits, vals):
    """Annex C: {code as a string of '0' / '1': symbol}."""
    return {format(code, f"0{n}b"): sym for sym, (code, n) in E.huffman_codes(bits, vals).items()}


def segment_bit_string(seg):
    """The segment's bytes as one bit string; the byte after every 0xFF (the stuffed 0x00) is dropped."""
    out, skip = [], False
    for b in seg:
        if skip:
            skip = False
            continue
        out.append(format(b, "08b"))
        skip = b == 0xFF
    return "".join(out)


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


def decode_segment(seg, n_blocks, subsampling, books):
    """Annex F.2.2 on one segment -> (int16 [n_blocks, 64] in zigzag order, status).  books: per component (DC book, AC book).
    After an error the remaining values are 0."""
    bits, pos = segment_bit_string(seg), 0
    comp_of = (0, 0, 0, 0, 1, 2) if subsampling == "420" else (0, 1, 2)

    def symbol(book):
        nonlocal pos
        for n in range(1, 17):
            if pos + n > len(bits):
                raise _Stop(OVERRUN)
            if bits[pos:pos + n] in book:
                pos += n
                return book[bits[pos - n:pos]]
        raise _Stop(BAD_CODE)

    def receive(n):
        nonlocal pos
        if pos + n > len(bits):
            raise _Stop(OVERRUN)
        v = int(bits[pos:pos + n], 2)
        pos += n
        return v - (1 << n) + 1 if v < 1 << (n - 1) else v   # EXTEND

    out = np.zeros((n_blocks, 64), dtype=np.int64)
    pred = [0, 0, 0]
    try:
        for b in range(n_blocks):
            c = comp_of[b % len(comp_of)]
            dc, ac = books[c]
            t = symbol(dc)
            if t > 11:
                raise _Stop(BAD_CODE)
            pred[c] = ((pred[c] + (receive(t) if t else 0) + 32768) & 0xFFFF) - 32768
            out[b, 0] = pred[c]
            k = 1
            while k < 64:
                rs = symbol(ac)
                r, n = rs >> 4, rs & 15
                if n == 0:
                    if r != 15:
                        break                                # EOB
                    k += 16
                    if k > 64:
                        raise _Stop(OVERFLOW)
                    continue
                if n > 10:
                    raise _Stop(BAD_CODE)
                k += r
                if k > 63:
                    raise _Stop(OVERFLOW)
                out[b, k] = receive(n)
                k += 1
    except _Stop as stop:
        return out.astype(np.int16), stop.status
    return out.astype(np.int16), OK


# ---- coefficients -> pixels ----
def _pass(x, axis, shift):
    """jidctint's pass over the eight values along `axis` of an int64 array."""
    i = [np.take(x, k, axis=axis) for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    outs = (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)
    return np.stack([(o + (1 << (shift - 1))) >> shift for o in outs], axis=axis)


def idct_blocks(coefs, quant):
    """int [..., 64] coefficients and quantisers [64], both in zigzag order -> samples int64 [..., 8, 8] in 0..255."""
    nat = np.zeros(coefs.shape, dtype=np.int64)
    nat[..., ZIGZAG] = coefs.astype(np.int64) * np.asarray(quant, dtype=np.int64)
    v = _pass(_pass(nat.reshape(coefs.shape[:-1] + (8, 8)), -2, 11), -1, 18)      # down the columns, then along the rows
    return np.clip(v + 128, 0, 255)                # libjpeg's range-limit table for -512 <= v + 128 <= 511; saturated beyond, as PIL does


def upsample420(c, H, W):
    """The real chroma samples int64 [ceil(H / 2), ceil(W / 2)] -> [H, W]."""
    h, w = c.shape
    if w <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:H, :W]
    up, down = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    s = np.empty((2 * h, w), dtype=np.int64)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + down
    left, right = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((2 * h, 2 * w), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
    return out[:H, :W]


def pixels_of(coefs, info):
    """int16 [blocks, 64] of one frame in scan order -> uint8 [H, W, 3]."""
    H, W = info.height, info.width
    if info.subsampling == "420":
        my, mx = -(-H // 16), -(-W // 16)
        m = coefs.reshape(my, mx, 6, 64)
        y = idct_blocks(m[:, :, :4], info.quant[0]).reshape(my, mx, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(16 * my, 16 * mx)
        planes = [idct_blocks(m[:, :, 4 + k], info.quant[1 + k]).transpose(0, 2, 1, 3).reshape(8 * my, 8 * mx) for k in range(2)]
        cb, cr = (upsample420(p[:-(-H // 2), :-(-W // 2)], H, W) for p in planes)
    else:
        my, mx = -(-H // 8), -(-W // 8)
        m = coefs.reshape(my, mx, 3, 64)
        y, cb, cr = (idct_blocks(m[:, :, k], info.quant[k]).transpose(0, 2, 1, 3).reshape(8 * my, 8 * mx) for k in range(3))
    y, cb, cr = y[:H, :W], cb[:H, :W] - 128, cr[:H, :W] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


# ---- whole streams ----
def decode(jpeg, rows=None, frame=0):
    """One stream -> dict(info, table [rows, 5], frame_info [3], coefs int16 [blocks, 64], status int [rows], pixels uint8
    [H, W, 3] or None when a status is not OK).  rows: the table's rows (default: the frame's segment count)."""
    info = D.parse_jpeg(jpeg)
    rows = info.segments if rows is None else rows
    bpm = 6 if info.subsampling == "420" else 3
    table, finfo = find_segments(jpeg, info.scan_offset, len(jpeg) - info.scan_offset, info.restart_interval, info.mcus, rows, frame)
    books = [(code_book(*dc), code_book(*ac)) for dc, ac in info.huffman]
    coefs = np.zeros((info.mcus * bpm, 64), dtype=np.int16)
    status = np.zeros(rows, dtype=np.int64)
    nf = min(info.segments, rows)
    markers_ok = finfo[0] == nf - 1 and finfo[1] == 1
    for s in range(nf):
        if not markers_ok:
            status[s] = MARKERS
            continue
        _, st, ln, fm, cnt = (int(v) for v in table[s])
        coefs[fm * bpm:(fm + cnt) * bpm], status[s] = decode_segment(jpeg[st:st + ln], cnt * bpm, info.subsampling, books)
    pixels = None if status.any() else pixels_of(coefs, info)
    return dict(info=info, table=table, frame_info=finfo, coefs=coefs, status=status, pixels=pixels)


def encode_coefs(coefs, H, W, quality, subsampling, ri):
    """int [blocks, 64] of one frame -> a complete stream coded by jpeg_ref's coder with the restart interval ri in MCUs (0: no
    restart markers), the header jpeg_header's with its DRI segment changed (or dropped)."""
    header = E.jpeg_header(H, W, quality, subsampling)
    at = header.index(b"\xff\xdd\x00\x04")
    header = header[:at] + (b"\xff\xdd\x00\x04" + struct.pack(">H", ri) if ri else b"") + header[at + 6:]
    bpm = 6 if subsampling == "420" else 3
    mcus = len(coefs) // bpm
    per = (ri or mcus) * bpm
    segs = [jpeg_ref.stuff(*jpeg_ref.segment_bits(coefs[b:b + per], subsampling)) for b in range(0, mcus * bpm, per)]
    body = b"".join(s + bytes([0xFF, 0xD0 + (k & 7)]) for k, s in enumerate(segs[:-1]))
    return header + body + segs[-1] + b"\xff\xd9"
