"""The rate control rule of the encode stage restated in plain Python / numpy on tests/jpeg_ref.py, for the tests of
landiff_amd/encode.py's JpegRateConfig and csrc/ld_jpeg_rate.hip's entry points.

Sizes are exact: the size of frame f at quality q is len(jpeg_ref.jpeg_encode(frame[None], q, sub)[0]) -- the header, every stuffed
segment and its marker.  "Fits" means size <= budget.  Two modes: frame (every frame searches its own quality under frame_bytes) and
clip (one quality for all frames, the sum of the sizes under clip_bytes).  The search is this bisection, held per frame or per clip:

    lo, hi = q_min - 1, q_max + 1;  the first trial is q_max
    a trial that fits sets lo = q, another hi = q;  the next trial is (lo + hi) // 2 while hi - lo > 1
    result max(lo, q_min), over_budget = (lo == q_min - 1)

R = 1 + ceil(log2(q_max - q_min + 1)) rounds are tabulated; where a search has finished the row reads (0, 0).  Stream size is not
monotone in quality, so the result is this bisection's and fits, not necessarily the largest quality that fits.
"""
import math

import numpy as np

import jpeg_ref as ref


def rounds(q_min, q_max):
    return 1 + math.ceil(math.log2(q_max - q_min + 1))


_SIZES: dict = {}


def frame_size(frame, quality, subsampling):
    """The exact stream size of one uint8 [H, W, 3] frame (cached by content: the searches of a test session share trials)."""
    key = (frame.shape, frame.tobytes(), quality, subsampling)
    if key not in _SIZES:
        _SIZES[key] = len(ref.jpeg_encode(np.ascontiguousarray(frame)[None], quality, subsampling)[0])
    return _SIZES[key]


def bisect(fits, q_min, q_max):
    """The stated bisection; fits(q) -> bool.  -> (quality, over_budget, the trial qualities in order)."""
    lo, hi, q, tried = q_min - 1, q_max + 1, q_max, []
    while True:
        tried.append(q)
        if fits(q):
            lo = q
        else:
            hi = q
        if hi - lo <= 1:
            break
        q = (lo + hi) // 2
    return max(lo, q_min), lo == q_min - 1, tried


def rate_search(frames, subsampling="420", q_max=95, q_min=1, frame_bytes=None, clip_bytes=None):
    """uint8 [F, H, W, 3] -> (qualities [F], over_budget [F], trials [R][F][2]): the (quality, that frame's size) of every trial."""
    assert (frame_bytes is None) != (clip_bytes is None)
    F, R = len(frames), rounds(q_min, q_max)
    trials = [[[0, 0] for _ in range(F)] for _ in range(R)]
    if clip_bytes is None:
        qualities, over = [], []
        for f, frame in enumerate(frames):
            q, o, tried = bisect(lambda t: frame_size(frame, t, subsampling) <= frame_bytes, q_min, q_max)
            for r, t in enumerate(tried):
                trials[r][f] = [t, frame_size(frame, t, subsampling)]
            qualities.append(q)
            over.append(o)
        return qualities, over, trials
    q, o, tried = bisect(lambda t: sum(frame_size(fr, t, subsampling) for fr in frames) <= clip_bytes, q_min, q_max)
    for r, t in enumerate(tried):
        trials[r] = [[t, frame_size(fr, t, subsampling)] for fr in frames]
    return [q] * F, [o] * F, trials


def rate_encode(frames, subsampling="420", q_max=95, q_min=1, frame_bytes=None, clip_bytes=None):
    """-> (streams: list of F bytes, each jpeg_ref.jpeg_encode of the frame at its quality; qualities; over_budget; trials)."""
    qualities, over, trials = rate_search(frames, subsampling, q_max, q_min, frame_bytes, clip_bytes)
    streams = [ref.jpeg_encode(np.ascontiguousarray(fr)[None], q, subsampling)[0] for fr, q in zip(frames, qualities)]
    return streams, qualities, over, trials


def frame_c8(frame, subsampling):
    """uint8 [H, W, 3] -> int16 [blocks, 64]: jpeg_ref.frame_coefs up to the quantiser -- c8 in scan order, zigzag order."""
    y, cb, cr = ref.ycc_planes(frame)
    if subsampling == "420":
        y, cb, cr = (ref._pad(p, 16) for p in (y, cb, cr))
        half = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
        cb, cr = half(cb), half(cr)
    else:
        y, cb, cr = (ref._pad(p, 8) for p in (y, cb, cr))
    zig = lambda p: (lambda c: c.reshape(c.shape[:-2] + (64,))[..., ref.ZIGZAG])(ref.fdct(ref._blocks(p - 128)))
    Y, Cb, Cr = zig(y), zig(cb), zig(cr)
    my, mx = Cb.shape[:2]
    if subsampling == "420":
        Y = Y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
        mcus = np.concatenate([Y, Cb[:, :, None], Cr[:, :, None]], axis=2)
    else:
        mcus = np.stack([Y, Cb, Cr], axis=2)
    out = mcus.reshape(-1, 64)
    assert np.abs(out).max() <= 8192
    return out.astype(np.int16)


def jpeg_c8(frames, subsampling="420"):
    return np.stack([frame_c8(f, subsampling) for f in frames])
