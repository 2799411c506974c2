"""The decode stage's second entropy route restated in plain Python and numpy, for the tests of
csrc/ld_jpeg_dec_sync.hip and landiff_amd/decode.py.

Written from the rule's text and built differently from the kernels on purpose, as tests/jpeg_dec_ref.py is: a segment is one
string of '0' / '1' characters beside the list of the raw positions its bits come from, a Huffman table a dict from code strings to
symbols, and the exits of a round are a list of tuples.

The rule.  A segment is `len` raw bytes, cut into n = max(1, ceil(len / B)) subsequences of B = sub_bytes bytes; subsequence i owns
the raw bytes [i B, min((i + 1) B, len)).  A 0x00 that follows a 0xFF is a stuffed byte and belongs to nobody.  A position p is
8 x (raw byte) + bit and names a bit of a data byte, or is 8 len.  A codeword is one Huffman symbol with its extra bits and belongs
to the subsequence in which its first bit lies.  The state is (p, j, k): j the block within the MCU, k the next zigzag index (0: a
DC is due).  exit(i, entry) decodes codewords from `entry` while p < 8 min((i + 1) B, len) and returns the state reached and the
blocks completed; a codeword that needs bits past the segment's end stops it at p = 8 len with j, k unchanged; where no code of
<= 16 bits matches, or a DC size is above 11 or an AC size above 10, p goes one bit on; a run past 63 ends the block, p past the
symbol.  Rounds: E0[i] = exit(i, (8 i B normalised, 0, 0)), Er[i] = exit(i, Er-1[i - 1]), Er[0] = E0[0].  The write pass decodes
once more from E[i - 1] with the block index known, stores DC differences, and reports what the serial decoder reports; the DC pass
turns differences into values by a running sum modulo 2^16 per component.
"""
import numpy as np

import jpeg_dec_ref as dref
from landiff_amd import decode as D

OK, BAD_CODE, OVERFLOW, OVERRUN = dref.OK, dref.BAD_CODE, dref.OVERFLOW, dref.OVERRUN


class Bits:
    """The data bits of a segment: .s the bit string, .at[q] the position p of bit q (.at[len(s)] = 8 len), .index {p: q}."""

    def __init__(self, seg):
        chars, at = [], []
        for i, b in enumerate(seg):
            if i > 0 and seg[i - 1] == 0xFF:                 # preceded by 0xFF: stuffed (0xFF 0xFF is refused before the scan)
                continue
            chars.append(format(b, "08b"))
            at += [8 * i + k for k in range(8)]
        self.s, self.len = "".join(chars), len(seg)
        self.at = at + [8 * len(seg)]
        self.index = {p: q for q, p in enumerate(self.at)}
        assert self.s == dref.segment_bit_string(seg)


def subsequences(length, sub_bytes):
    """The raw byte ranges [(lo, hi)] of the subsequences of a segment of `length` bytes."""
    n = max(1, -(-length // sub_bytes))
    return [(i * sub_bytes, min((i + 1) * sub_bytes, length)) for i in range(n)]


def cold_start(bits, i, sub_bytes):
    """(8 i B normalised, 0, 0): the first data bit at or after raw byte i B."""
    p = 8 * i * sub_bytes
    while p < 8 * bits.len and p not in bits.index:
        p += 8
    return (min(p, 8 * bits.len), 0, 0)


class _End(Exception):
    pass


def _codeword(bits, q, j, k, books, bpm):
    """One codeword at bit q in state (j, k) -> (q after it, k after it or None where the block ends, (zigzag index, value) or
    None, status): status BAD_CODE / OVERFLOW is what the serial decoder reports here (q is then where the counting pass goes on);
    raises _End where the codeword needs bits past the end."""
    comp = ((0, 0, 0, 0, 1, 2) if bpm == 6 else (0, 1, 2))[j]
    book = books[comp][0 if k == 0 else 1]
    sym = None
    for n in range(1, 17):
        if q + n > len(bits.s):
            raise _End()
        if bits.s[q:q + n] in book:
            sym, after = book[bits.s[q:q + n]], q + n
            break
    size = None if sym is None else sym if k == 0 else sym & 15
    if sym is None or size > (11 if k == 0 else 10):
        return q + 1, k, None, BAD_CODE

    def receive(at, n):
        if at + n > len(bits.s):
            raise _End()
        v = int(bits.s[at:at + n], 2)
        return v - (1 << n) + 1 if v < 1 << (n - 1) else v

    if k == 0:
        return after + size, 1, (0, receive(after, size) if size else 0), OK
    run = sym >> 4
    if size == 0:
        if run != 15:
            return after, None, None, OK                     # EOB
        if k + 16 > 64:
            return after, None, None, OVERFLOW
        return after, (k + 16 if k + 16 < 64 else None), None, OK
    if k + run > 63:
        return after, None, None, OVERFLOW
    v = receive(after, size)
    return after + size, (k + run + 1 if k + run + 1 < 64 else None), (k + run, v), OK


def exit_state(bits, i, entry, sub_bytes, books, bpm):
    """exit(i, entry) -> ((p, j, k), blocks completed)."""
    p, j, k = entry
    limit = 8 * min((i + 1) * sub_bytes, bits.len)
    n = 0
    while p < limit:
        try:
            q, k2, _, _ = _codeword(bits, bits.index[p], j, k, books, bpm)
        except _End:
            return (8 * bits.len, j, k), n
        p = bits.at[q]
        if k2 is None:
            j, k, n = (j + 1) % bpm, 0, n + 1
        else:
            k = k2
    return (p, j, k), n


def rounds(seg, sub_bytes, books, bpm, most=None):
    """-> (the exits [(state, blocks)] after every round, E0 first, up to and including the first round that equals the one before
    it, or `most` rounds; R, the round of the fixed point: E[R] == E[R + 1], None if `most` rounds did not show it)."""
    bits = Bits(seg)
    n = len(subsequences(len(seg), sub_bytes))
    E = [exit_state(bits, i, cold_start(bits, i, sub_bytes) if i else (0, 0, 0), sub_bytes, books, bpm) for i in range(n)]
    out, r = [E], 0
    while most is None or r < most:
        r += 1
        E = [out[-1][0]] + [exit_state(bits, i, out[-1][i - 1][0], sub_bytes, books, bpm) for i in range(1, n)]
        out.append(E)
        if E == out[-2]:
            return out, r - 1
    return out, None


def write_pass(seg, sub_bytes, books, bpm, n_blocks, E):
    """The write pass from the exits E -> (int64 [n_blocks, 64] with the DC differences in [:, 0], status, converged)."""
    bits = Bits(seg)
    out = np.zeros((n_blocks, 64), dtype=np.int64)
    first = np.concatenate([[0], np.cumsum([e[1] for e in E])]).tolist()
    errors, converged = [], True
    for i in range(len(E)):
        (p, j, k), b = ((0, 0, 0) if i == 0 else E[i - 1][0]), first[i]
        limit, n, whole = 8 * min((i + 1) * sub_bytes, bits.len), 0, True
        while p < limit:
            if b + n >= n_blocks:
                whole = False
                break
            try:
                q, k2, store, status = _codeword(bits, bits.index[p], j, k, books, bpm)
            except _End:
                errors.append((i, OVERRUN))
                whole = None
                break
            if status:
                errors.append((i, status))
                whole = None
                break
            if store is not None:
                out[b + n, store[0]] = store[1]
            p = bits.at[q]
            if k2 is None:
                j, k, n = (j + 1) % bpm, 0, n + 1
            else:
                k = k2
        if whole:
            converged &= ((p, j, k), n) == E[i]
            if i == len(E) - 1 and b + n < n_blocks:
                errors.append((i, OVERRUN))                  # the bits ran out while blocks are owed
        elif whole is False:
            converged &= b + E[i][1] >= n_blocks             # every later lane must start at the block count too
    return out, (min(errors)[1] if errors else OK), converged


def dc_pass(blocks, bpm):
    """Differences -> DC values: per component a running sum modulo 2^16 (as int16)."""
    out = blocks.copy()
    comp = np.array((0, 0, 0, 0, 1, 2) if bpm == 6 else (0, 1, 2))[np.arange(len(blocks)) % bpm]
    for c in range(3):
        out[comp == c, 0] = ((np.cumsum(blocks[comp == c, 0]) + 32768) & 0xFFFF) - 32768
    return out


def decode(jpeg, sub_bytes, max_rounds=None, rows=None):
    """One stream by the sync route -> dict(coefs int16 [blocks, 64], status [rows], rounds [rows] (rounds that changed an exit,
    at most max_rounds), fell [rows], exits: per segment the list of (p, j, k, blocks) after the rounds that were run, n: per
    segment its subsequences).  A segment that did not converge, or reports an error, is decoded by jpeg_dec_ref.decode_segment."""
    info = D.parse_jpeg(jpeg)
    rows = info.segments if rows is None else rows
    bpm = 6 if info.subsampling == "420" else 3
    table, finfo = dref.find_segments(jpeg, info.scan_offset, len(jpeg) - info.scan_offset, info.restart_interval, info.mcus, rows)
    books = [(dref.code_book(*dc), dref.code_book(*ac)) for dc, ac in info.huffman]
    coefs = np.zeros((info.mcus * bpm, 64), dtype=np.int16)
    status, nrounds, fell = (np.zeros(rows, dtype=np.int64) for _ in range(3))
    nf = min(info.segments, rows)
    exits, counts = [[] for _ in range(rows)], [0] * rows
    if not (finfo[0] == nf - 1 and finfo[1] == 1):
        status[:nf] = dref.MARKERS
        return dict(info=info, coefs=coefs, status=status, rounds=nrounds, fell=fell, exits=exits, n=counts)
    for s in range(nf):
        _, st, ln, fm, cnt = (int(v) for v in table[s])
        seg = jpeg[st:st + ln]
        history, R = rounds(seg, sub_bytes, books, bpm, most=max_rounds)
        E = history[-1]
        nrounds[s] = R if R is not None else max_rounds
        blocks, status[s], converged = write_pass(seg, sub_bytes, books, bpm, cnt * bpm, E)
        exits[s], counts[s] = [e[0] + (e[1],) for e in E], len(E)
        fell[s] = int(not converged or status[s] != OK)
        if fell[s]:
            coefs[fm * bpm:(fm + cnt) * bpm], status[s] = dref.decode_segment(seg, cnt * bpm, info.subsampling, books)
        else:
            coefs[fm * bpm:(fm + cnt) * bpm] = dc_pass(blocks, bpm).astype(np.int16)
    return dict(info=info, coefs=coefs, status=status, rounds=nrounds, fell=fell, exits=exits, n=counts)
