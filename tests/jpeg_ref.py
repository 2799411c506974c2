"""The encode stage's rule restated in numpy, for the tests of landiff_amd/encode.py and csrc/ld_jpeg.hip.

Written from the rule's text, integers throughout (int64), and built differently from the kernels on purpose: whole planes are
converted, padded and cut into blocks at once, the DCT is two matrix products over all blocks, and the entropy coder appends to one
Python integer per segment -- no bit offsets, no scan, no window.  The tables come from landiff_amd/encode.py, the one place they
are stated (tests/test_jpeg_host.py compares them with the segments of a file PIL writes).
"""
import numpy as np

from landiff_amd import encode as E

K = np.array(E.dct_matrix(), dtype=np.int64)                  # [u][x]
ZIGZAG = np.array(E.zigzag_order())                           # zigzag position -> 8 v + u


def jpeg_tables(quality):
    """(luma, chroma) quantisers int64 [64] in zigzag order."""
    l, c = E.quant_tables(quality)
    return np.array(l, dtype=np.int64), np.array(c, dtype=np.int64)


def ycc_planes(frame):
    """uint8 [H, W, 3] -> (Y, Cb, Cr) int64 [H, W]: the JFIF matrix in 16-bit fixed point, rounded, clamped."""
    r, g, b = (frame[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32768) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32768) >> 16
    return tuple(np.clip(p, 0, 255) for p in (y, cb, cr))


def _pad(plane, mcu):
    H, W = plane.shape
    return np.pad(plane, ((0, -H % mcu), (0, -W % mcu)), mode="edge")


def _blocks(plane):
    """[8 a, 8 b] -> [a, b, 8, 8]."""
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    return plane.reshape(a, 8, b, 8).transpose(0, 2, 1, 3)


def fdct(blocks, trace=None):
    """int64 [..., 8, 8] level-shifted samples [y][x] -> c8 [..., 8, 8] = 8 x the coefficient [v][u].  trace (a dict): the largest
    magnitude of every stage's values, for the int32 bound."""
    s1 = np.einsum("ux,...yx->...yu", K, blocks)
    t = (s1 + 256) >> 9
    s2 = np.einsum("vy,...yu->...vu", K, t)
    c8 = (s2 + 65536) >> 17
    if trace is not None:
        for name, v in (("row_sum", s1), ("row_out", t), ("col_sum", s2), ("c8", c8)):
            trace[name] = max(trace.get(name, 0), int(np.abs(v).max()))
    return c8


def quantise(c8, table):
    """c8 [..., 8, 8], table [64] in zigzag order -> int64 [..., 64] in zigzag order: round half away from zero, AC clamped to +-1023."""
    z = c8.reshape(c8.shape[:-2] + (64,))[..., ZIGZAG]
    q = (np.abs(z) + 4 * table) // (8 * table)
    q[..., 1:] = np.minimum(q[..., 1:], 1023)
    return np.where(z < 0, -q, q)


def frame_coefs(frame, quality, subsampling):
    """uint8 [H, W, 3] -> int16 [blocks, 64] in scan order."""
    ql, qc = jpeg_tables(quality)
    y, cb, cr = ycc_planes(frame)
    if subsampling == "420":
        y, cb, cr = (_pad(p, 16) for p in (y, cb, cr))
        half = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
        cb, cr = half(cb), half(cr)
    elif subsampling == "444":
        y, cb, cr = (_pad(p, 8) for p in (y, cb, cr))
    else:
        raise ValueError(subsampling)
    Y, Cb, Cr = (quantise(fdct(_blocks(p - 128)), t) for p, t in ((y, ql), (cb, qc), (cr, qc)))
    my, mx = Cb.shape[:2]
    if subsampling == "420":
        Y = Y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)            # Y00 Y01 Y10 Y11 of an MCU
        mcus = np.concatenate([Y, Cb[:, :, None], Cr[:, :, None]], axis=2)
    else:
        mcus = np.stack([Y, Cb, Cr], axis=2)
    return mcus.reshape(-1, 64).astype(np.int16)


def jpeg_coefs(frames, quality, subsampling="420"):
    """uint8 [F, H, W, 3] (numpy) -> int16 [F, blocks, 64]: blocks in scan order, coefficients in zigzag order."""
    return np.stack([frame_coefs(f, quality, subsampling) for f in frames])


_CODES = {tc_th: E.huffman_codes(bits, vals) for tc_th, bits, vals in E.HUFFMAN_TABLES}


def _value_bits(v, s):
    return (v if v >= 0 else v - 1) & ((1 << s) - 1)


def segment_bits(blocks, subsampling):
    """int [n, 64] the blocks of one segment in scan order -> (value, nbits): Annex F.1.2, the DC predictors starting at 0."""
    bpm = 6 if subsampling == "420" else 3
    comp_of = (0, 0, 0, 0, 1, 2) if bpm == 6 else (0, 1, 2)
    pred = [0, 0, 0]
    words = []                                     # one binary string per symbol (a segment can be megabits: no big-integer shifts)
    put = lambda code, ln, v, s: words.append(format((code << s) | _value_bits(v, s), f"0{ln + s}b"))
    for b, blk in enumerate(np.asarray(blocks).tolist()):
        c = comp_of[b % bpm]
        dc, ac = _CODES[0x00 + (c > 0)], _CODES[0x10 + (c > 0)]
        diff, pred[c] = blk[0] - pred[c], blk[0]
        s = abs(diff).bit_length()
        put(*dc[s], diff, s)
        run = 0
        for v in blk[1:]:
            if v == 0:
                run += 1
                continue
            while run > 15:
                put(*ac[0xF0], 0, 0)
                run -= 16
            s = abs(v).bit_length()
            put(*ac[run << 4 | s], v, s)
            run = 0
        if run:
            put(*ac[0x00], 0, 0)
    bits = "".join(words)
    return int(bits, 2), len(bits)


def stuff(acc, n):
    """A bit string -> bytes: padded with 1-bits to a byte boundary, every 0xFF followed by 0x00."""
    pad = -n % 8
    raw = ((acc << pad) | ((1 << pad) - 1)).to_bytes((n + pad) // 8, "big")
    return raw.replace(b"\xff", b"\xff\x00")


def jpeg_entropy(coefs, mcus_per_row, subsampling="420"):
    """int16 [F, blocks, 64] -> per frame the list of its segments' bytes (one per MCU row, without markers)."""
    per = mcus_per_row * (6 if subsampling == "420" else 3)
    out = []
    for fc in np.asarray(coefs):
        assert fc.shape[0] % per == 0
        out.append([stuff(*segment_bits(fc[r:r + per], subsampling)) for r in range(0, fc.shape[0], per)])
    return out


def jpeg_encode(frames, quality=95, subsampling="420"):
    """uint8 [F, H, W, 3] (numpy) -> list of F bytes: header, then every segment followed by RST(row mod 8), the last by EOI."""
    H, W = frames.shape[1:3]
    header = E.jpeg_header(H, W, quality, subsampling)
    mcux = -(-W // E.mcu_size(subsampling))
    out = []
    for segs in jpeg_entropy(jpeg_coefs(frames, quality, subsampling), mcux, subsampling):
        body = b"".join(s + bytes([0xFF, 0xD0 + (r & 7)]) for r, s in enumerate(segs[:-1]))
        out.append(header + body + segs[-1] + b"\xff\xd9")
    return out


# ---- the inputs the tests share ----
SIZES = ((8, 8), (16, 16), (17, 33), (24, 40), (50, 70))
FAMILIES = ("noise", "ramps", "flat0", "flat255", "flat128", "checker", "bars")
QUALITIES = (1, 50, 95, 100)


def picture(kind, H, W, seed=0):
    """uint8 [H, W, 3] of one content family (never modified)."""
    y, x = np.mgrid[0:H, 0:W]
    if kind == "noise":
        p = np.random.default_rng(1000 + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif kind == "ramps":
        p = np.stack([(3 * x + y + 40 * seed) % 256, (2 * y + 7 * seed) % 256, (x + 2 * y) * 255 // max(1, W + 2 * H - 3)], axis=-1)
    elif kind.startswith("flat"):
        p = np.full((H, W, 3), int(kind[4:]))
    elif kind == "checker":                        # one-pixel checkerboard, the phase and the two levels by seed
        lo, hi = ((0, 255), (16, 235), (255, 0))[seed % 3]
        p = np.repeat(np.where((y + x + seed) % 2 == 0, lo, hi)[..., None], 3, axis=-1)
    elif kind == "bars":                           # saturated colour bars, 5 pixels wide
        cols = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [255, 255, 255], [0, 0, 0]])
        p = cols[((x + 2 * seed) // 5) % 8]
    else:
        raise KeyError(kind)
    p = np.ascontiguousarray(p.astype(np.uint8))
    p.setflags(write=False)
    return p


def clip3(kind, H, W):
    """F = 3 different frames of one family."""
    return np.stack([picture(kind, H, W, seed) for seed in range(3)])


def maximising_blocks():
    """uint8 [64, 8, 8]: for basis function (v, u) the -128 / 127 sign pattern (as 0 / 255 pixels) that maximises its coefficient."""
    k = K.astype(np.float64)
    basis = np.einsum("vy,ux->vuyx", k, k).reshape(64, 8, 8)
    return np.where(basis >= 0, 255, 0).astype(np.uint8)


def maximising_frames():
    """The 64 patterns (and their negatives) as grey frames: uint8 [2, 64, 64, 3], pattern (v, u) the block at (8 v, 8 u)."""
    m = maximising_blocks().reshape(8, 8, 8, 8).transpose(0, 2, 1, 3).reshape(64, 64)
    return np.stack([np.repeat(f[..., None], 3, axis=-1) for f in (m, 255 - m)])


def mse(a, b):
    return float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())


def dense_ff_blocks(n):
    """int [n, 64]: blocks (4:4:4 scan order) whose code is as many 1-bits as the code table allows -- every code word holds a
    0-bit, so no byte string is 0xFF throughout.  DC difference 0; +1023 (ten 1-bits) after runs of 15 zeros, whose (15, 10) symbol
    has the tables' longest code, sixteen bits of which only the last is 0, and at coefficient 63 (no EOB)."""
    blocks = np.zeros((n, 64), dtype=np.int64)
    blocks[:, [16, 32, 48, 63]] = 1023
    return blocks
