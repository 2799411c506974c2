"""The retime stage on the GPU (ld_retime_u8; landiff_amd/retime.py) against the numpy restatement of the frame rule
(tests/retime_ref.py): frames, motion field and SAD, torch.equal everywhere -- the rule is integer arithmetic, there is no tolerance."""
import json
import struct
from functools import lru_cache

import numpy as np
import pytest
import torch

import retime_ref as ref

pytestmark = pytest.mark.gpu

H, W = 45, 70                                   # partial blocks on both axes: 6 x 9 blocks
PHASES = [(1, 2), (1, 3), (2, 3), (4, 15)]
SHIFT = (6, -4)


@lru_cache(maxsize=None)
def pair(kind, C, h=H, w=W):
    """The shared inputs (numpy uint8 [h, w, C] each, never modified)."""
    if kind == "noise":
        A, B = ref.noise((h, w, C), 1), ref.noise((h, w, C), 2)
    elif kind == "translated":
        A, B = ref.translated_pair(h, w, C, SHIFT, seed=11)
    elif kind == "gradient":
        A, B = ref.gradient_noise(h, w, C, seed=3)
    elif kind == "constant":
        A, B = np.full((h, w, C), 100, np.uint8), np.full((h, w, C), 100, np.uint8)
    elif kind == "stripes":                       # vertical stripes of period 4; B is A moved by two columns: dx = 2, -2, 6, -6 all match
        x = np.arange(w + 2)
        row = np.where(x % 4 < 2, 40, 200).astype(np.uint8)
        full = np.broadcast_to(row[None, :, None], (h, w + 2, C))
        A, B = full[:, 2:].copy(), full[:, :w].copy()
    elif kind == "checker":                       # 2 x 2 cells; B is A moved by two rows: the inverse board
        y, x = np.mgrid[0:h + 2, 0:w]
        full = np.broadcast_to(np.where((y // 2 + x // 2) % 2 == 0, 30, 220).astype(np.uint8)[..., None], (h + 2, w, C))
        A, B = full[2:].copy(), full[:h].copy()
    else:
        raise KeyError(kind)
    for a in (A, B):
        a.setflags(write=False)
    return A, B


@lru_cache(maxsize=None)
def want(kind, C, p, q, search=8, penalty=4, max_sad=24, h=H, w=W):
    A, B = pair(kind, C, h, w)
    return tuple(torch.from_numpy(v) for v in ref.interp_frame(A, B, p, q, search, penalty, max_sad))


def gpu(cuda, A, B, p, q, search=8, penalty=4, max_sad=24):
    from landiff_amd import ops
    frames = torch.from_numpy(np.stack([A, B])).to(cuda)
    out, mv, sad = ops.retime_u8(frames, [0], [p], q, search, penalty, max_sad, want_motion=True)
    return out[0].cpu(), mv[0].cpu(), sad[0].cpu()


def check(cuda, kind, C, p, q, search=8, penalty=4, max_sad=24, h=H, w=W):
    got = gpu(cuda, *pair(kind, C, h, w), p, q, search, penalty, max_sad)
    exp = want(kind, C, p, q, search, penalty, max_sad, h, w)
    assert got[1].dtype == torch.int16 and got[2].dtype == torch.int32 and got[0].dtype == torch.uint8
    assert got[1].shape == (-(-h // 8), -(-w // 8), 2) and got[2].shape == got[1].shape[:2] and got[0].shape == (h, w, C)
    assert torch.equal(got[2], exp[2]), "SAD"
    assert torch.equal(got[1], exp[1]), "motion field"
    assert torch.equal(got[0], exp[0]), "frame"
    return got


@pytest.mark.parametrize("p,q", PHASES)
@pytest.mark.parametrize("kind", ["noise", "translated", "gradient"])
@pytest.mark.parametrize("C", [3, 1])
def test_matches_reference(cuda, C, kind, p, q):
    check(cuda, kind, C, p, q)


@pytest.mark.parametrize("C", [3, 1])
def test_frame_smaller_than_the_window(cuda, C):
    for p, q in PHASES:
        for kind in ("noise", "gradient"):
            check(cuda, kind, C, p, q, h=5, w=7)


def test_search_zero_is_the_rounded_crossfade(cuda):
    for p, q in PHASES:
        out, mv, _ = check(cuda, "noise", 3, p, q, search=0)
        assert not mv.any() and torch.equal(out, torch.from_numpy(ref.crossfade(*pair("noise", 3), p, q)))
    check(cuda, "translated", 1, 1, 2, search=0, max_sad=255)


def test_search_32(cuda):
    check(cuda, "gradient", 3, 2, 5, search=32, max_sad=255, h=40, w=40)             # 4225 candidates per block
    check(cuda, "noise", 1, 2, 5, search=32, penalty=0, max_sad=255, h=40, w=40)


@pytest.mark.parametrize("penalty", [0, 4])
@pytest.mark.parametrize("kind", ["constant", "stripes", "checker"])
def test_ties_follow_the_tuple_order(cuda, kind, penalty):
    """Many candidates share a cost: (cost, |dy| + |dx|, dy, dx) must decide as the reference does."""
    for C in (3, 1):
        _, mv, sad = check(cuda, kind, C, 1, 2, penalty=penalty)
        check(cuda, kind, C, 1, 3, penalty=penalty)
    if kind == "constant":
        assert not mv.any() and not sad.any()
    if kind == "stripes":                          # dx = -2 and dx = 2 both give SAD 0 in the interior: the smaller dx wins
        assert tuple(mv[2, 4]) == (0, -2) and sad[2, 4] == 0
    if kind == "checker":                          # dy = -2 / 2 and dx = -2 / 2 all match: the smallest dy wins
        assert tuple(mv[2, 4]) == (-2, 0) and sad[2, 4] == 0


def test_fallback(cuda):
    A, B = pair("noise", 3)
    out, mv, sad = check(cuda, "noise", 3, 1, 3)
    assert not mv.any() and sad.min() > 24 * 256 and torch.equal(out, torch.from_numpy(ref.crossfade(A, B, 1, 3)))
    out255, mv255, sad255 = check(cuda, "noise", 3, 1, 3, max_sad=255)            # never falls back
    assert torch.equal(sad255, sad) and mv255.any() and not torch.equal(out255, out)
    check(cuda, "gradient", 3, 1, 3, max_sad=0)                                   # falls back wherever the SAD is not 0


@pytest.mark.parametrize("p,q", PHASES)
def test_translated_texture_properties(cuda, p, q):
    """The field in the interior is the translation with SAD 0, and the output there is A read at offset a."""
    A, B = pair("translated", 3)
    out, mv, sad = gpu(cuda, A, B, p, q)
    ay, ax = int(ref.split(SHIFT[0], p, q)[0]), int(ref.split(SHIFT[1], p, q)[0])
    my, mx = abs(SHIFT[0]), abs(SHIFT[1])
    n = 0
    for by in range(6):
        for bx in range(9):
            if 8 * by - 4 - my < 0 or 8 * by + 11 + my > H - 1 or 8 * bx - 4 - mx < 0 or 8 * bx + 11 + mx > W - 1:
                continue
            n += 1
            assert tuple(mv[by, bx].tolist()) == SHIFT and sad[by, bx] == 0
            shifted = torch.from_numpy(A[8 * by + ay:8 * by + ay + 8, 8 * bx + ax:8 * bx + ax + 8].copy())
            assert torch.equal(out[8 * by:8 * by + 8, 8 * bx:8 * bx + 8], shifted)
    assert n == 12


@lru_cache(maxsize=None)
def clip5():
    rng = np.random.default_rng(21)
    T = rng.integers(0, 256, (H + 40, W + 40, 3), dtype=np.uint8)
    frames = np.stack([T[20 + 2 * t:20 + 2 * t + H, 20 - 3 * t:20 - 3 * t + W] for t in range(5)])   # the texture moves by (-2, 3) a frame
    frames[4] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)                    # a cut: the last pair falls back
    frames.setflags(write=False)
    return frames


def test_retime_clip_5_frames_to_24_fps(cuda):
    from landiff_amd.retime import RetimeConfig, retime_clip, retime_plan
    frames = clip5()
    dev = torch.from_numpy(frames.copy()).to(cuda)
    cfg = RetimeConfig(out_fps=24)
    out = retime_clip(dev, cfg)
    assert out.shape == (13, H, W, 3) and out.dtype == torch.uint8 and out.device == dev.device
    exp, exp_mv, exp_sad = ref.retime(frames, [k // 3 for k in range(13)], [k % 3 for k in range(13)], 3)
    for k in (0, 3, 6, 9, 12):
        assert torch.equal(out[k], dev[k // 3])
    assert torch.equal(out.cpu(), torch.from_numpy(exp))
    out2, mv, sad = retime_clip(dev, retime_plan(5, cfg), want_motion=True)
    assert torch.equal(out2, out)
    assert torch.equal(mv.cpu(), torch.from_numpy(exp_mv)) and torch.equal(sad.cpu(), torch.from_numpy(exp_sad))
    assert not mv[0::3].any() and not sad[0::3].any() and mv[1].any()              # copied frames have zero rows
    assert retime_clip(dev, RetimeConfig(out_fps=4)).shape[0] == 3 and torch.equal(retime_clip(dev, RetimeConfig(out_fps=4)), dev[::2])
    assert torch.equal(retime_clip(dev, RetimeConfig(out_fps=8)), dev)


def test_two_runs_same_bits(cuda):
    from landiff_amd.retime import RetimeConfig, retime_clip
    dev = torch.from_numpy(clip5().copy()).to(cuda)
    a = retime_clip(dev, RetimeConfig(out_fps=30), want_motion=True)
    b = retime_clip(dev, RetimeConfig(out_fps=30), want_motion=True)
    assert a[0].shape[0] == 16 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_motion_profile(cuda):
    from landiff_amd.retime import motion_profile
    frames = clip5()
    prof = motion_profile(torch.from_numpy(frames.copy()).to(cuda))
    _, mv, sad = ref.retime(frames, [0, 1, 2, 3], [1, 1, 1, 1], 2)
    assert torch.equal(prof.mv.cpu(), torch.from_numpy(mv)) and torch.equal(prof.sad.cpu(), torch.from_numpy(sad))
    l1 = np.abs(mv.astype(np.int64)).sum(-1)
    blocks = 6 * 9
    assert prof.mean_motion == [int(l1[i].sum()) / blocks for i in range(4)]
    assert prof.max_motion == [int(l1[i].max()) for i in range(4)] and prof.max_motion[0] == 5
    assert prof.mean_sad_per_pixel == [int(sad[i].astype(np.int64).sum()) / (blocks * 256) for i in range(4)]
    assert prof.fallback_share == [int((sad[i] > 24 * 256).sum()) / blocks for i in range(4)]
    assert prof.fallback_share[3] == 1.0 and prof.max_motion[3] == 0 and prof.fallback_share[0] < 0.5        # the cut
    d = prof.as_dict()
    assert json.loads(json.dumps(d, allow_nan=False)) == d and d["pairs"] == 4 and d["blocks"] == [6, 9]
    assert d["clip_max_motion"] == max(prof.max_motion) and d["mean_motion"] == prof.mean_motion


def test_offsets_past_2_31(cuda):
    """2 source frames of 480 x 720 x 3 and 2100 output frames: n_out H W C = 2 177 280 000 > 2^31.  The last frame and a middle
    one must equal the same (index, phase) computed by a one-frame launch, whose rule the small cases pin."""
    from landiff_amd import ops
    Hh, Ww, n, q = 480, 720, 2100, 2100
    assert n * Hh * Ww * 3 > 2 ** 31
    g = torch.Generator().manual_seed(7)
    base = torch.randint(0, 256, (Hh + 4, Ww + 4, 3), generator=g, dtype=torch.uint8)
    src = torch.stack([base[2:2 + Hh, 2:2 + Ww], base[1:1 + Hh, 4:4 + Ww]]).contiguous().to(cuda)      # moved by (1, -2)
    ph = list(range(n))
    out, mv, sad = ops.retime_u8(src, [0] * n, ph, q, 2, 4, 24, want_motion=True)
    assert out.numel() > 2 ** 31 and torch.equal(out[0], src[0]) and not mv[0].any()
    for k in (n - 1, 1051):
        o1, m1, s1 = ops.retime_u8(src, [0], [ph[k]], q, 2, 4, 24, want_motion=True)
        assert torch.equal(out[k], o1[0]) and torch.equal(mv[k], m1[0]) and torch.equal(sad[k], s1[0])
        assert tuple(m1[0, 30, 45].tolist()) == (1, -2) and s1[0, 30, 45] == 0
    del out


def _written(path_stem):
    """(fps, frames) of the video file save_video_tensor left: the Motion-JPEG AVI's header, or the mp4 through imageio."""
    avi = path_stem.with_suffix(".avi")
    if avi.exists():
        raw = avi.read_bytes()
        at = raw.index(b"avih") + 8
        usec, _, _, _, total = struct.unpack("<5I", raw[at:at + 20])
        at = raw.index(b"strh") + 8
        scale, rate = struct.unpack("<2I", raw[at + 20:at + 28])
        assert usec == 1000000 // (rate // scale)
        return rate // scale, total
    import imageio
    rd = imageio.get_reader(str(path_stem.with_suffix(".mp4")))
    return round(rd.get_meta_data()["fps"]), rd.count_frames()


def test_save_video_out_fps(cuda, tmp_path):
    """_save_video with --out_fps 24: the file is written at 24 fps with 3 (F - 1) + 1 frames, <name>_retime.json holds the plan and
    the motion profile, and --save_frames still writes the exact model frames.  Without the flag nothing of this exists."""
    import warnings
    import landiff.infer_video as iv
    from landiff_amd.retime import RetimeConfig, retime_clip
    frames = torch.from_numpy(clip5().copy())
    torch.cuda.set_device(cuda)
    args = iv.parse_args(["--prompt", "p", "--out_fps", "24", "--save_frames"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        iv._save_video(args, frames, str(tmp_path / "a" / "clip.mp4"), fps=8)
        iv._save_video(iv.parse_args(["--prompt", "p"]), frames, str(tmp_path / "b" / "clip.mp4"), fps=8)
    stem = tmp_path / "a" / "clip"
    assert _written(stem) == (24, 13)
    assert np.array_equal(np.load(f"{stem}.frames.npy"), frames.numpy())
    rep = json.load(open(f"{stem}_retime.json"))
    assert rep["plan"]["n_out"] == 13 and rep["plan"]["q"] == 3 and rep["plan"]["out_fps"] == 24.0 and rep["plan"]["search"] == 8
    assert rep["motion"]["pairs"] == 4 and rep["motion"]["max_motion"][0] == 5 and rep["motion"]["fallback_share"][3] == 1.0
    assert _written(tmp_path / "b" / "clip") == (8, 5) and not (tmp_path / "b" / "clip_retime.json").exists()
    # what was written is retime_clip's output: the float [C, T, H, W] form the model returns goes the same way
    video = (frames.permute(3, 0, 1, 2).float() + 0.5) / 255
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        iv._save_video(iv.parse_args(["--prompt", "p", "--out_fps", "24", "--out_search", "4"]), video, str(tmp_path / "c" / "clip.mp4"))
    assert _written(tmp_path / "c" / "clip") == (24, 13)
    assert json.load(open(tmp_path / "c" / "clip_retime.json"))["plan"]["search"] == 4
    fb = tmp_path / "c" / "clip.frames.npy"                                        # (the writer's fallback leaves the written frames there)
    if fb.exists():
        exp = retime_clip(frames.to(cuda), RetimeConfig(out_fps=24, search=4)).cpu().numpy()
        assert np.array_equal(np.load(fb), exp)


def test_pipeline_retime(cuda):
    from landiff_amd.config import PipelineConfig
    from landiff_amd.pipeline import LanDiffPipeline, synthetic_inputs
    from landiff_amd.retime import RetimeConfig, retime_clip
    from landiff_amd.weights import init_pipeline_state
    cfg = PipelineConfig.tiny(num_steps=2).check()
    pipe = LanDiffPipeline(cfg, init_pipeline_state(cfg, seed=1234), cuda)
    assert pipe.last_retime is None
    x = pipe(synthetic_inputs(cfg, cuda, n_text=6, seed=42)).clone()
    assert "retime" not in pipe.timings                                            # off: the stage does not run
    y = pipe.retime(x.cpu(), RetimeConfig(out_fps=24))                             # any device
    F = x.shape[0]
    assert y.shape == (3 * (F - 1) + 1,) + tuple(x.shape[1:]) and y.device == x.device and pipe.timings["retime"] > 0
    assert torch.equal(y[::3], x) and torch.equal(y, retime_clip(x, RetimeConfig(out_fps=24)))
    assert pipe.last_retime["n_out"] == y.shape[0] and pipe.last_retime["q"] == 3
    with pytest.raises(ValueError, match="uint8"):
        pipe.retime(x.float(), RetimeConfig(out_fps=24))
