"""Host-side checks of the conform stage (no GPU): the float64 restatement against F.interpolate(antialias=True), the product's
tables against the restatement, the plan's integer / rational arithmetic on hand-checked cases, the command line's defaults and
refusals, the two entry points in header / library / SIGNATURES, and the refusals that come before any launch."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conform_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((37, 53), (16, 24)), ((16, 24), (40, 56)), ((90, 61), (10, 7)), ((33, 47), (33, 47)), ((5, 7), (3, 2)), ((1, 9), (4, 4))]


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
@pytest.mark.parametrize("src,dst", SHAPES)
def test_restatement_matches_torch_antialias(src, dst, filt):
    """The tables as the issue states them are PyTorch's: max |difference| <= 1e-9 in float64 (measured: <= 4e-13)."""
    g = torch.Generator().manual_seed(src[0] * 100 + dst[1])
    x = torch.randint(0, 256, (2, src[0], src[1], 3), generator=g, dtype=torch.uint8)
    got = ref.resize_ref(x, dst[0], dst[1], filt)
    want = F.interpolate(x.permute(0, 3, 1, 2).double(), size=dst, mode=filt, antialias=True, align_corners=False).permute(0, 2, 3, 1)
    assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-9
    if src == dst:
        assert torch.equal(got, x.double())                   # same size: weights (1, 0), an exact copy


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
def test_product_tables_are_the_restatement_rounded_once(filt):
    from landiff_amd.conform import axis_table, axis_table64
    for n_in, n_out in [(37, 16), (53, 24), (16, 40), (90, 10), (61, 7), (33, 33), (1, 4), (9, 4), (4096, 2), (2160, 480), (1620, 720)]:
        lo, hi, ws = ref.tables(n_in, n_out, filt)
        lo64, cnt64, w64 = axis_table64(n_in, n_out, filt)
        win, w = axis_table(n_in, n_out, filt)
        assert win.dtype == np.int32 and w.dtype == np.float32 and win.shape == (n_out, 2)
        assert win[:, 0].tolist() == lo == lo64.tolist() and (win[:, 0] + win[:, 1]).tolist() == hi
        assert w.shape[1] == max(b - a for a, b in zip(lo, hi))
        for i in range(n_out):
            row = np.array(ws[i])
            assert np.abs(w64[i, :len(row)] - row).max() <= 1e-15 and not w64[i, len(row):].any()
            assert np.array_equal(w[i, :len(row)], w64[i, :len(row)].astype(np.float32)) and not w[i, len(row):].any()
    assert axis_table(2160, 480, filt)[1].shape[1] == (9 if filt == "bilinear" else 18)      # 2 * half * 4.5
    assert axis_table(90, 10, "bicubic")[1].shape[1] == 36                      # 2 * 2 * 9: no fixed tap cap


def test_plan_cover_box_and_frames():
    from landiff_amd.conform import ConformConfig, conform_plan, cover_box
    assert cover_box(1080, 1920, 480, 720) == (0, 150, 1080, 1620)
    assert cover_box(1920, 1080, 480, 720) == (600, 0, 720, 1080)
    assert cover_box(51, 70, 64, 96) == (2, 0, 46, 70)                          # 70 * 64 // 96 = 46; (51 - 46) // 2 = 2: odd pixel below
    assert cover_box(480, 720, 480, 720) == (0, 0, 480, 720)
    p = conform_plan((184, 1080, 1920, 3), 49, 480, 720, ConformConfig(fit="cover", src_fps=30, window="first"))
    assert p.box == (0, 150, 1080, 1620) and p.out_shape == (49, 480, 720) and (p.scale_y, p.scale_x) == (2.25, 2.25)
    assert p.frame_idx[:9] == (0, 4, 8, 11, 15, 19, 23, 26, 30) and p.frame_idx[-1] == 180 and p.src_fps == Fraction(30)
    last = conform_plan((184, 1080, 1920, 3), 49, 480, 720, ConformConfig(fit="cover", src_fps=30))
    assert last.frame_idx[-1] == 183 and last.frame_idx[0] == 3 and last.frame_idx[-3:] == (175, 179, 183)
    assert all(b > a for a, b in zip(last.frame_idx, last.frame_idx[1:]))
    off = conform_plan((184, 1080, 1920, 3), 49, 480, 720, ConformConfig(fit="stretch", src_fps=30, window="first", start_s=0.1))
    assert off.frame_idx[:3] == (3, 7, 11) and off.frame_idx[-1] == 183 and off.box == (0, 0, 1080, 1920)
    ntsc = conform_plan((400, 8, 8), 3, 8, 8, ConformConfig(fit="stretch", src_fps="30000/1001", window="first"))
    assert ntsc.frame_idx == (0, 4, 7) and ntsc.src_fps == Fraction(30000, 1001)        # 3.746 -> 4, 7.49 -> 7
    assert conform_plan((9, 8, 8), 3, 8, 8, ConformConfig(fit="stretch", src_fps=29.97, window="first")).src_fps == Fraction(2997, 100)
    # one to one without a rate: the last or the first n frames, exactly as extend_video takes them today
    assert conform_plan((60, 100, 100, 3), 49, 480, 720, ConformConfig(fit="stretch")).frame_idx == tuple(range(11, 60))
    assert conform_plan((60, 100, 100, 3), 49, 480, 720, ConformConfig(fit="stretch", window="first")).frame_idx == tuple(range(49))
    crop = conform_plan((49, 100, 200, 3), 49, 480, 720, ConformConfig(fit="cover", crop=(3, 5, 30, 45)))
    assert crop.box == (3, 5, 30, 45) and crop.scale_y == 30 / 480
    d = crop.as_dict()
    assert d["box"] == [3, 5, 30, 45] and d["fit"] == "cover" and d["filter"] == "bilinear" and d["src_fps"] is None and len(d["frame_idx"]) == 49


def test_plan_refusals_and_exact():
    from landiff_amd.conform import ConformConfig, conform_plan
    with pytest.raises(ValueError, match=r"need 6\.0 s"):                       # 5 s at 30 fps: 49 frames at 8 fps span 6 s
        conform_plan((150, 1080, 1920, 3), 49, 480, 720, ConformConfig(fit="cover", src_fps=30))
    with pytest.raises(ValueError, match=r"need 6\.0 s"):
        conform_plan((150, 1080, 1920, 3), 49, 480, 720, ConformConfig(fit="cover", src_fps=30, window="first"))
    conform_plan((181, 1080, 1920, 3), 49, 480, 720, ConformConfig(fit="cover", src_fps=30))           # 6.0 s exactly: enough
    with pytest.raises(ValueError, match="too short"):
        conform_plan((48, 100, 100, 3), 49, 480, 720, ConformConfig(fit="stretch"))
    with pytest.raises(ValueError, match="leaves the"):
        conform_plan((49, 100, 100, 3), 49, 480, 720, ConformConfig(fit="cover", crop=(0, 60, 50, 50)))
    ex = conform_plan((60, 480, 720, 3), 49, 480, 720, ConformConfig())
    assert ex.fit == "exact" and ex.box == (0, 0, 480, 720) and ex.frame_idx == tuple(range(11, 60)) and (ex.scale_y, ex.scale_x) == (1.0, 1.0)
    with pytest.raises(ValueError, match="exact"):
        conform_plan((60, 481, 720, 3), 49, 480, 720, ConformConfig())
    for bad in (dict(fit="fill"), dict(window="middle"), dict(filter="lanczos"), dict(src_fps=0), dict(src_fps=-3), dict(start_s=-1.0),
                dict(start_s=1.0), dict(start_s=1.0, src_fps=30), dict(crop=(0, 0, 4)), dict(crop=(0, 0, 4.5, 4))):
        with pytest.raises(ValueError, match="ConformConfig"):
            ConformConfig(**bad)


def test_parse_args_clip_flags(capsys):
    import landiff.infer_video as iv
    base = ["--prompt", "p"]
    a = iv.parse_args(base + ["--edit_video", "c.npy"])
    assert a.clip_fit == "exact" and a.clip_fps is None and a.clip_start is None and a.clip_filter is None and a.conform is None
    a = iv.parse_args(base + ["--edit_video", "c.npy", "--clip_fit", "cover", "--clip_fps", "12"])
    c = a.conform
    assert (c.fit, c.src_fps, c.window, c.start_s, c.filter) == ("cover", "12", "last", 0.0, "bilinear")
    c = iv.parse_args(base + ["--edit_video", "c.npy", "--clip_fit", "stretch", "--clip_fps", "30000/1001", "--clip_start", "1.5",
                              "--clip_filter", "bicubic"]).conform
    assert (c.fit, c.window, c.start_s, c.filter) == ("stretch", "first", 1.5, "bicubic")
    assert iv.parse_args(base + ["--extend_video", "c.npy", "--clip_fit", "cover"]).conform.window == "last"
    assert iv.parse_args(base + ["--first_frame", "i.npy", "--clip_fit", "cover"]).conform.fit == "cover"
    for bad, msg in ((["--clip_fit", "cover"], "give one of them"),
                     (["--edit_video", "c.npy", "--clip_fps", "30"], "go with --clip_fit"),
                     (["--edit_video", "c.npy", "--clip_filter", "bicubic"], "go with --clip_fit"),
                     (["--edit_video", "c.npy", "--clip_fit", "exact", "--clip_start", "1"], "go with --clip_fit"),
                     (["--extend_video", "c.npy", "--clip_fit", "cover", "--clip_fps", "30", "--clip_start", "1"], "--clip_start goes with"),
                     (["--edit_video", "c.npy", "--clip_fit", "cover", "--clip_start", "1"], "--clip_start goes with"),
                     (["--first_frame", "i.npy", "--clip_fit", "cover", "--clip_fps", "30"], "frame rate of the"),
                     (["--edit_video", "c.npy", "--clip_fit", "cover", "--clip_fps", "0"], "positive"),
                     (["--edit_video", "c.npy", "--clip_fit", "cover", "--clip_fps", "fast"], "--clip_fps"),
                     (["--edit_video", "c.npy", "--clip_fit", "fill"], "invalid choice")):
        with pytest.raises(SystemExit):
            iv.parse_args(base + bad)
        assert msg in capsys.readouterr().err, bad


def test_entry_points_in_header_library_and_signatures():
    from landiff_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "landiff_hip.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, nargs in (("ld_resize_u8", 22), ("ld_resize_mask_u8", 17)):
        decl = re.search(rf"\bint {name}\(([^;]*)\);", hdr)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name])
        assert re.search(rf" T {name}\b", syms)
    assert _lib.load().ld_version() == _lib.ABI_VERSION == int(re.search(r"#define LD_ABI_VERSION (\d+)", hdr).group(1))


def test_refusals_before_any_launch():
    """Every LD_REQUIRE of the two entry points answers before a launch: safe without a GPU."""
    from landiff_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)

    def resize(src=p, dst=p, idx=None, wy=p, fy=p, ty=3, wx=p, fx=p, tx=3, Fs=2, Hs=10, Ws=12, C=3, n=2, Ho=4, Wo=5, y0=0, x0=0,
               hc=10, wc=12, filt=0):
        return lib.ld_resize_u8(src, dst, idx, wy, fy, ty, wx, fx, tx, Fs, Hs, Ws, C, n, Ho, Wo, y0, x0, hc, wc, filt, None)

    def mask(src=p, dst=p, idx=None, wy=p, wx=p, Fs=2, Hs=10, Ws=12, n=2, Ho=4, Wo=5, y0=0, x0=0, hc=10, wc=12, filt=0):
        return lib.ld_resize_mask_u8(src, dst, idx, wy, wx, Fs, Hs, Ws, n, Ho, Wo, y0, x0, hc, wc, filt, None)

    for fn, name in ((resize, b"ld_resize_u8"), (mask, b"ld_resize_mask_u8")):
        for kw, msg in ((dict(src=None), b"null pointer"), (dict(dst=None), b"null pointer"), (dict(wy=None), b"null pointer"),
                        (dict(wx=None), b"null pointer"), (dict(Ho=0), b"empty shape"), (dict(n=0), b"empty shape"),
                        (dict(hc=0), b"empty shape"), (dict(Fs=0), b"empty shape"),
                        (dict(y0=1), b"leaves the 10 x 12 source"), (dict(x0=-1), b"leaves the"), (dict(wc=13), b"leaves the"),
                        (dict(y0=5, hc=6), b"crop box (5, 0, 6, 12)"), (dict(n=3), b"must not exceed the source's 2 frames"),
                        (dict(filt=2), b"unknown filter 2"), (dict(filt=-1), b"unknown filter")):
            assert fn(**kw) == -1, kw
            err = lib.ld_last_error()
            assert name + b":" in err and msg in err, (kw, err)
    for kw, msg in ((dict(fy=None), b"null pointer"), (dict(fx=None), b"null pointer"), (dict(C=2), b"C must be 1 or 3, got 2"),
                    (dict(C=4), b"C must be 1 or 3"), (dict(ty=0), b"weight row"), (dict(tx=13), b"weight row")):
        assert resize(**kw) == -1 and msg in lib.ld_last_error(), kw


def test_wrappers_check_their_arguments_on_the_host():
    """ops.resize_u8 / resize_mask_u8 refuse bad arguments -- the frame_idx range among them -- before anything is uploaded."""
    from landiff_amd import _lib, ops
    x = torch.zeros(3, 10, 12, 3, dtype=torch.uint8)
    m = torch.ones(3, 10, 12, dtype=torch.bool)
    for kw, exc, msg in ((dict(frame_idx=[0, 3]), ValueError, r"in \[0, 3\)"), (dict(frame_idx=[-1]), ValueError, r"in \[0, 3\)"),
                         (dict(frame_idx=[]), ValueError, "non-empty"), (dict(box=(0, 0, 11, 12)), ValueError, "leaves the 10 x 12"),
                         (dict(box=(0, 4, 10, 9)), ValueError, "leaves the"), (dict(filter="lanczos"), ValueError, "filter must be")):
        with pytest.raises(exc, match=msg):
            ops.resize_u8(x, (4, 5), **kw)
        with pytest.raises(exc, match=msg):
            ops.resize_mask_u8(m, (4, 5), **kw)
    with pytest.raises(ValueError, match="empty shape"):
        ops.resize_u8(x, (0, 5))
    with pytest.raises(ValueError, match="C must be 1 or 3"):
        ops.resize_u8(x[..., :2].contiguous(), (4, 5))
    with pytest.raises(TypeError, match="uint8"):
        ops.resize_u8(x.float(), (4, 5))
    with pytest.raises(TypeError, match="uint8 or bool"):
        ops.resize_mask_u8(m.float(), (4, 5))
    with pytest.raises(ValueError, match="contiguous 4-d"):
        ops.resize_u8(x[:, :, ::2], (4, 5))
    with pytest.raises(_lib.LandiffHipError, match="GPU tensors"):               # valid arguments, host tensors: no CPU fallback
        ops.resize_u8(x, (4, 5))
    with pytest.raises(_lib.LandiffHipError, match="GPU tensors"):
        ops.resize_mask_u8(m, (4, 5))


def test_mask_restatement_single_hole():
    """The restated rule on a case small enough to check by hand: 8 -> 4 bilinear has windows [0,3) [1,5) [3,7) [5,8)."""
    lo, hi, _ = ref.tables(8, 4, "bilinear")
    assert (lo, hi) == ([0, 1, 3, 5], [3, 5, 7, 8])
    m = torch.ones(1, 8, 8, dtype=torch.uint8)
    m[0, 4, 2] = 0
    out = ref.mask_ref(m, 4, 4, "bilinear")[0]
    want = torch.ones(4, 4, dtype=torch.uint8)
    want[1:3, 0:2] = 0                                                           # rows whose window holds 4: 1, 2; columns holding 2: 0, 1
    assert torch.equal(out, want)
