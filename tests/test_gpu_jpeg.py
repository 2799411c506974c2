"""The encode stage on the GPU (csrc/ld_jpeg.hip; landiff_amd/encode.py) against the numpy restatement of its rule
(tests/jpeg_ref.py): coefficients with torch.equal, segments and streams byte for byte -- the rule is integer arithmetic, there is
no tolerance; PIL decodes what comes out, and at the workload's size PIL's own encode is the quality yardstick."""
import json
from functools import lru_cache

import numpy as np
import pytest
import torch

import jpeg_ref as ref
from landiff_amd import encode as E
from test_jpeg_host import decode, entropy_markers, pil_encode, within_pil

pytestmark = pytest.mark.gpu

SUBS = ("420", "444")


@lru_cache(maxsize=None)
def clip(kind, H, W):
    if kind == "maximising":
        return ref.maximising_frames()
    return ref.clip3(kind, H, W)


CASES = [(k, H, W) for H, W in ref.SIZES for k in ref.FAMILIES] + [("maximising", 64, 64)]


@lru_cache(maxsize=None)
def want_coefs(kind, H, W, quality, sub):
    return torch.from_numpy(ref.jpeg_coefs(clip(kind, H, W), quality, sub))


@lru_cache(maxsize=None)
def want_streams(kind, H, W, quality, sub):
    frames = clip(kind, H, W)
    mcux = -(-W // E.mcu_size(sub))
    header = E.jpeg_header(H, W, quality, sub)
    out = []
    for segs in ref.jpeg_entropy(want_coefs(kind, H, W, quality, sub).numpy(), mcux, sub):
        body = b"".join(s + bytes([0xFF, 0xD0 + (r & 7)]) for r, s in enumerate(segs[:-1]))
        out.append(header + body + segs[-1] + b"\xff\xd9")
    assert len(out) == len(frames)
    return out


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("quality", ref.QUALITIES)
def test_coefficients_match_the_restatement(cuda, quality, sub):
    from landiff_amd import ops
    for kind, H, W in CASES:
        got = ops.jpeg_coefs_u8(torch.from_numpy(clip(kind, H, W)).to(cuda), quality, sub)
        want = want_coefs(kind, H, W, quality, sub)
        assert got.shape == want.shape and got.dtype == torch.int16, (kind, H, W)
        assert torch.equal(got.cpu(), want), (kind, H, W, int((got.cpu() != want).sum()))


def test_coefficients_of_strided_frames(cuda):
    """The frames as a window of a wider, taller buffer: a padded row stride and a frame stride that is no multiple of it."""
    from landiff_amd import ops
    frames = clip("noise", 50, 70)
    big = torch.full((3, 57, 90, 3), 201, dtype=torch.uint8)
    big[:, 4:54, 11:81] = torch.from_numpy(frames)
    view = big.to(cuda)[:, 4:54, 11:81]
    assert not view.is_contiguous() and view.stride(1) == 270
    for sub in SUBS:
        assert torch.equal(ops.jpeg_coefs_u8(view, 95, sub).cpu(), want_coefs("noise", 50, 70, 95, sub))
        got = E.encode_jpeg(view, E.JpegConfig(95, sub))
        assert got == want_streams("noise", 50, 70, 95, sub)


def designed_segments():
    """[(name, subsampling, mcus per row, int16 [n_seg, blocks, 64])]: coefficient patterns no picture produces on demand."""
    out = []
    z = lambda n_seg, nb: np.zeros((n_seg, nb, 64), dtype=np.int16)
    for sub, bpm in (("420", 6), ("444", 3)):
        out.append((f"all zero {sub}", sub, 5, z(3, 5 * bpm)))
        c = z(2, 7 * bpm)
        c[:, :, 0] = np.random.default_rng(1).integers(-1023, 1025, (2, 7 * bpm))
        out.append((f"only DC {sub}", sub, 7, c))
        c = z(2, 6 * bpm)                                              # DC steps of +-2047 between neighbours of every component
        comp = np.array(((0, 0, 0, 0, 1, 2) if bpm == 6 else (0, 1, 2)) * 6)
        for k in range(3):
            idx = np.flatnonzero(comp == k)
            c[0, idx, 0] = np.where(np.arange(len(idx)) % 2 == 0, -1023, 1024)
            c[1, idx, 0] = np.where(np.arange(len(idx)) % 2 == 0, 1024, -1023)
        out.append((f"DC steps {sub}", sub, 6, c))
    mags = sorted({m for s in range(1, 11) for m in (1 << (s - 1), (1 << s) - 1)})          # 1, 2, 3, 4, 7, 8, .. 512, 1023
    c = z(2, 2 * 3)
    for b in range(6):
        for k in range(1, 64):
            m = mags[(k + 5 * b) % len(mags)]
            c[0, b, k], c[1, b, k] = (m if (k + b) % 2 else -m), (-m if (k + b) % 2 else m)
    out.append(("category edges", "444", 2, c))
    runs = (14, 15, 16, 17, 31, 32, 47, 48, 62)
    c = z(1, 9 * 3)
    for i, r in enumerate(runs):                                       # run r before a non-zero, in luma and both chroma blocks
        c[0, 3 * i:3 * i + 3, 1 + r] = (-3, 5, 1023)
    out.append(("zero runs", "444", 9, c))
    c = z(1, 6)
    c[0, :, 63] = (1, -1, 512, -1023, 7, -8)
    c[0, 1, 1] = 2
    out.append(("coefficient 63", "420", 1, c))
    for sign in (1, -1):                                              # the 1658-bit block filling whole segments
        c = np.full((2, 4 * 6, 64), 1023 * sign, dtype=np.int16)
        c[:, :, 0] = np.where(np.arange(24) % 2 == 0, -1023, 1024) * sign
        out.append((f"every coefficient {1023 * sign}", "420", 4, c))
    out.append(("densest 0xFF", "444", 8, ref.dense_ff_blocks(24).astype(np.int16)[None]))
    out.append(("densest 0xFF 4:2:0", "420", 4, ref.dense_ff_blocks(24).astype(np.int16)[None]))
    wide = np.random.default_rng(2).integers(-1023, 1024, (2, 512 * 6, 64)).astype(np.int16)      # 3072 blocks: the window in 18 pieces
    out.append(("widest segment, random", "420", 512, wide))
    return out


def test_entropy_coder_on_designed_coefficients(cuda):
    from landiff_amd import ops
    for name, sub, mcux, coefs in designed_segments():
        segs, lens = ops.jpeg_entropy_i16(torch.from_numpy(coefs).to(cuda), mcux, sub)
        segs, lens = segs.cpu().numpy(), lens.cpu().tolist()
        want = ref.jpeg_entropy(coefs.reshape(1, -1, 64), mcux, sub)[0]
        assert len(want) == len(lens) == coefs.shape[0]
        bound = ops.jpeg_size(3, 1, 8, mcux * E.mcu_size(sub), sub)
        for i, w in enumerate(want):
            assert lens[i] == len(w) <= bound == segs.shape[1], (name, i, lens[i], len(w))
            assert segs[i, :lens[i]].tobytes() == w, (name, i)
        if name.startswith("every coefficient"):                        # the sizing rule's block: 20 + 63 * 26 bits after a +-2047 DC step
            one, two = ref.segment_bits(coefs[0, :1], sub)[1], ref.segment_bits(coefs[0, :2], sub)[1]
            assert two - one == 1658 == 20 + 63 * 26 and 2 * -(-24 * 1658 // 8) == bound
        if name.startswith("densest"):
            raw = want[0].replace(b"\xff\x00", b"\xff")
            assert len(want[0]) == len(raw) + raw.count(b"\xff") and 2 * raw.count(b"\xff") > len(raw)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("quality", ref.QUALITIES)
def test_streams_match_the_restatement(cuda, quality, sub):
    cfg = E.JpegConfig(quality, sub)
    for kind, H, W in CASES:
        frames = torch.from_numpy(clip(kind, H, W)).to(cuda)
        got = E.encode_jpeg(frames, cfg)
        want = want_streams(kind, H, W, quality, sub)
        assert got == want, (kind, H, W, [len(g) for g in got], [len(w) for w in want])
        img, size = decode(got[-1])                                    # one stream per call through PIL, on this machine
        assert size == (W, H) and img.shape == (H, W, 3)


def test_two_calls_same_bytes_and_the_layout_tiles_the_buffer(cuda):
    from landiff_amd import ops
    frames = torch.from_numpy(np.concatenate([clip("noise", 50, 70), clip("ramps", 50, 70), clip("bars", 50, 70)])).to(cuda)
    cfg = E.JpegConfig(95, "420")
    a, b = E.encode_jpeg(frames, cfg), E.encode_jpeg(frames, cfg)
    assert a == b and len(a) == 9
    buf, offs, lens = E.encode_jpeg(frames, cfg, return_device=True)
    offs, lens = offs.tolist(), lens.tolist()
    assert offs[0] == 0 and all(offs[i + 1] == offs[i] + lens[i] for i in range(8)) and buf.numel() == offs[-1] + lens[-1]
    raw = buf.cpu().numpy().tobytes()
    assert [raw[o:o + n] for o, n in zip(offs, lens)] == a
    assert buf.numel() <= ops.jpeg_size(4, 9, 50, 70, "420", len(E.jpeg_header(50, 70, 95, "420")))
    for j in a:
        assert j.startswith(b"\xff\xd8") and j.endswith(b"\xff\xd9")


@pytest.mark.parametrize("H,W,sub", [(4096, 16, "420"), (16, 4096, "420"), (16, 4096, "444"), (160, 16, "444")])
def test_long_and_wide_frames(cuda, H, W, sub):
    """4096 rows (256 segments), 4096 columns (a segment of 1536 blocks: at quality 100 on noise its bits pass the 32 KiB window, the
    strip goes in pieces), and 20 MCU rows in 4:4:4 (the RST index wraps twice)."""
    frame = np.random.default_rng(H + W).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    got = E.encode_jpeg(torch.from_numpy(frame).to(cuda), E.JpegConfig(100, sub))
    want = ref.jpeg_encode(frame, 100, sub)
    assert got == want
    markers, segs = entropy_markers(got[0])
    rows = -(-H // E.mcu_size(sub))
    assert markers == [0xD0 + (r & 7) for r in range(rows - 1)] + [0xD9]
    if W == 4096:
        assert max(len(s.replace(b"\xff\x00", b"\xff")) for s in segs) > 32768          # more than one window
    assert decode(got[0])[1] == (W, H)


def moving_pattern(F=49, H=480, W=720, seed=3):
    """A seeded textured pattern sliding over a smooth background: uint8 [F, H, W, 3]."""
    rng = np.random.default_rng(seed)
    tex = rng.integers(0, 256, (H + 2 * F, W + 3 * F, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    smooth = np.stack([(x * 255 // (W - 1)), (y * 255 // (H - 1)), ((x + y) * 255 // (H + W - 2))], axis=-1).astype(np.uint8)
    ph, pw, y0 = H // 2, W // 3, H // 5
    frames = np.empty((F, H, W, 3), dtype=np.uint8)
    for t in range(F):
        x0 = W // 8 + t * (W // 2) // F                                 # the patch moves right, its texture slides under it
        frames[t] = smooth
        frames[t, y0:y0 + ph, x0:x0 + pw] = tex[2 * t:2 * t + ph, 3 * t:3 * t + pw]
        band = slice(H * 5 // 6, H * 11 // 12)
        frames[t, band] = (frames[t, band].astype(np.int64) + 5 * t).clip(0, 255)
    return frames


def test_workload_size_by_properties(cuda):
    from landiff_amd import ops
    frames = moving_pattern()
    cfg = E.JpegConfig(95, "420")
    got = E.encode_jpeg(torch.from_numpy(frames).to(cuda), cfg)
    assert len(got) == 49
    for k, want in zip((0, 48), ref.jpeg_encode(frames[[0, 48]], 95, "420")):
        assert got[k] == want, k
    total = sum(len(j) for j in got)
    assert total <= ops.jpeg_size(4, 49, 480, 720, "420", len(E.jpeg_header(480, 720, 95, "420")))
    worst = (0.0, ())
    for k, (f, j) in enumerate(zip(frames, got)):
        img, size = decode(j)
        assert size == (720, 480)
        pil, _ = decode(pil_encode(f, 95, "420", restart_marker_rows=1))
        mine, theirs = ref.mse(img, f), ref.mse(pil, f)
        worst = max(worst, (mine - theirs, (k, mine, theirs)))
        assert within_pil(mine, theirs), (k, mine, theirs)
    print(f"49 x 480 x 720: {total} bytes, largest mse excess over PIL {worst}")


def test_default_off_and_the_gpu_encoded_file(cuda, tmp_path, monkeypatch):
    """Without --video_encoder nothing of the stage runs (its wrappers raise if touched) and the file is the host writer's, byte for
    byte; with --video_encoder gpu --out_fps 24 the 49 frames become a 145-frame, 24 fps Motion-JPEG AVI whose every frame is PIL's
    decode of encode_jpeg of the retimed frame, with <name>_encode.json beside it."""
    import warnings
    import landiff.infer_video as iv
    from landiff.utils import read_mjpeg_avi, save_video_tensor
    from landiff_amd import ops
    from landiff_amd.retime import RetimeConfig, retime_clip
    frames = torch.from_numpy(moving_pattern(49, 40, 56, seed=9))
    torch.cuda.set_device(cuda)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with monkeypatch.context() as m:
            def boom(*a, **k):
                raise AssertionError("the encode stage ran although it is off")
            for name in ("jpeg_encode_u8", "jpeg_coefs_u8", "jpeg_entropy_i16", "jpeg_size"):
                m.setattr(ops, name, boom)
            iv._save_video(iv.parse_args(["--prompt", "p"]), frames, str(tmp_path / "off" / "clip.mp4"), fps=8)
        save_video_tensor(frames, str(tmp_path / "today" / "clip.mp4"), fps=8)
        off = sorted(p.name for p in (tmp_path / "off").iterdir())
        assert off == sorted(p.name for p in (tmp_path / "today").iterdir()) and "clip_encode.json" not in off
        for name in off:
            assert (tmp_path / "off" / name).read_bytes() == (tmp_path / "today" / name).read_bytes(), name
        args = iv.parse_args(["--prompt", "p", "--video_encoder", "gpu", "--out_fps", "24", "--save_frames"])
        iv._save_video(args, frames, str(tmp_path / "on" / "clip.mp4"), fps=8)
    on = sorted(p.name for p in (tmp_path / "on").iterdir())
    assert on == ["clip.avi", "clip.frames.npy", "clip_encode.json", "clip_retime.json"]
    assert np.array_equal(np.load(tmp_path / "on" / "clip.frames.npy"), frames.numpy())          # --save_frames keeps its meaning
    got, fps = read_mjpeg_avi(tmp_path / "on" / "clip.avi")
    assert fps == 24 and got.shape == (145, 40, 56, 3)
    retimed = retime_clip(frames.to(cuda), RetimeConfig(out_fps=24))
    jpegs = E.encode_jpeg(retimed, E.JpegConfig())
    for k in range(145):
        assert np.array_equal(got[k], decode(jpegs[k])[0]), k
    rep = json.load(open(tmp_path / "on" / "clip_encode.json"))
    sizes = [len(j) for j in jpegs]
    assert rep["quality"] == 95 and rep["subsampling"] == "420" and rep["frames"] == 145 and rep["total_bytes"] == sum(sizes)
    assert rep["bytes_per_frame"] == {"min": min(sizes), "mean": sum(sizes) / 145, "max": max(sizes)} and "PIL" in rep["table_source"]
    # the model's float [C, T, H, W] form without --out_fps goes the same way
    video = (frames.permute(3, 0, 1, 2).float() + 0.5) / 255
    iv._save_video(iv.parse_args(["--prompt", "p", "--video_encoder", "gpu", "--jpeg_quality", "60"]), video, str(tmp_path / "q" / "clip.mp4"))
    got, fps = read_mjpeg_avi(tmp_path / "q" / "clip.avi")
    want = E.encode_jpeg(frames.to(cuda), E.JpegConfig(60))
    assert fps == 8 and got.shape == (49, 40, 56, 3) and np.array_equal(got[7], decode(want[7])[0])
    assert json.load(open(tmp_path / "q" / "clip_encode.json"))["quality"] == 60


def test_pipeline_encode(cuda):
    from landiff_amd.config import PipelineConfig
    from landiff_amd.pipeline import LanDiffPipeline, synthetic_inputs
    from landiff_amd.weights import init_pipeline_state
    cfg = PipelineConfig.tiny(num_steps=2).check()
    pipe = LanDiffPipeline(cfg, init_pipeline_state(cfg, seed=1234), cuda)
    assert pipe.last_encode is None
    x = pipe(synthetic_inputs(cfg, cuda, n_text=6, seed=42)).clone()
    assert "encode" not in pipe.timings                                             # off: the stage does not run
    jpegs = pipe.encode(x.cpu(), E.JpegConfig(90, "444"))                           # any device
    assert jpegs == ref.jpeg_encode(x.cpu().numpy(), 90, "444") and pipe.timings["encode"] > 0
    assert pipe.last_encode["frames"] == x.shape[0] and pipe.last_encode["total_bytes"] == sum(len(j) for j in jpegs)
    assert decode(jpegs[0])[1] == (x.shape[2], x.shape[1])
    with pytest.raises(ValueError, match="uint8"):
        pipe.encode(x.float())
