"""Rate control of the encode stage on the GPU (landiff_amd/encode.py JpegRateConfig, csrc/ld_jpeg_rate.hip) against the
restatement tests/jpeg_rate_ref.py: torch.equal and bytes == throughout, no tolerance."""
import io
import json
import os
from functools import lru_cache

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_rate_ref as rr
import jpeg_ref as ref
from landiff_amd import encode as E

pytestmark = pytest.mark.gpu

SUBS = ("420", "444")
SIX = ("noise", "ramps", "flat0", "flat128", "checker", "bars")       # one frame per content family (the three flat levels differ by a few bytes: two of them)


@lru_cache(maxsize=None)
def six(H, W):
    return np.stack([ref.picture(k, H, W) for k in SIX])                 # (shared: never modified)


@lru_cache(maxsize=None)
def want_c8(kind, H, W, sub):
    return torch.from_numpy(rr.jpeg_c8(ref.maximising_frames() if kind == "maximising" else ref.clip3(kind, H, W), sub))


def run(cuda, frames, q_max, sub, **kw):
    """-> (streams, info) of the rate-controlled encode of numpy frames."""
    return E.encode_jpeg(torch.from_numpy(np.ascontiguousarray(frames)).to(cuda), E.JpegConfig(q_max, sub), rate=E.JpegRateConfig(**kw), return_rate=True)


def check_against_restatement(cuda, frames, q_max, sub, **kw):
    got, info = run(cuda, frames, q_max, sub, **kw)
    ref_kw = dict(kw)
    q_min = ref_kw.pop("min_quality", 1)
    want, q, over, trials = rr.rate_encode(frames, sub, q_max, q_min, **ref_kw)
    assert info["qualities"] == q and info["over_budget"] == over, (kw, info["qualities"], q)
    assert info["trials"] == trials, kw
    assert len(info["trials"]) == E.rate_rounds(q_min, q_max)
    assert got == want, kw
    return got, info


@pytest.mark.parametrize("sub", SUBS)
def test_c8_matches_the_restatement(cuda, sub):
    """The extreme: |c8| = 8192 is reached on the maximising frames, by -8192 (the DC of a block of samples -128).  +8192 would take
    a sample of +128, which 8-bit pixels do not have: the largest positive value there is the restatement's, 8160 at 4:2:0."""
    from landiff_amd import ops
    top = 0
    for kind, H, W in [(k, H, W) for H, W in ref.SIZES for k in ref.FAMILIES] + [("maximising", 64, 64)]:
        frames = ref.maximising_frames() if kind == "maximising" else ref.clip3(kind, H, W)
        got = ops.jpeg_c8_u8(torch.from_numpy(frames).to(cuda), sub)
        want = want_c8(kind, H, W, sub)
        assert got.shape == want.shape and got.dtype == torch.int16, (kind, H, W)
        assert torch.equal(got.cpu(), want), (kind, H, W, int((got.cpu() != want).sum()))
        top = max(top, int(got.max()), -int(got.min()))
        if kind == "maximising":
            assert int(got.min()) == -8192 == int(want.min()) and 8100 < int(got.max()) == int(want.max()) <= 8192   # the extreme an int16 has to hold
    assert top == 8192
    # the frames as a window of a wider, taller buffer
    big = torch.full((3, 57, 90, 3), 201, dtype=torch.uint8)
    big[:, 4:54, 11:81] = torch.from_numpy(ref.clip3("noise", 50, 70))
    view = big.to(cuda)[:, 4:54, 11:81]
    assert not view.is_contiguous() and view.stride(1) == 270
    assert torch.equal(ops.jpeg_c8_u8(view, sub).cpu(), want_c8("noise", 50, 70, sub))


@pytest.mark.parametrize("sub", SUBS)
def test_per_frame_quantiser_is_the_coefficient_kernels(cuda, sub):
    from landiff_amd import ops
    qualities = (1, 49, 50, 95, 100)
    for frames in (np.stack([ref.picture(k, 50, 70, s) for s, k in enumerate(("noise", "ramps", "checker", "bars", "noise"))]),
                   np.concatenate([ref.maximising_frames()] * 3)[:5]):
        x = torch.from_numpy(frames).to(cuda)
        got = ops.jpeg_quant_i16(ops.jpeg_c8_u8(x, sub), torch.tensor(qualities, dtype=torch.int32, device=cuda), sub)
        for f, q in enumerate(qualities):
            alone = ops.jpeg_coefs_u8(x[f:f + 1], q, sub)
            assert torch.equal(got[f:f + 1], alone), (f, q, int((got[f:f + 1] != alone).sum()))
            assert torch.equal(alone.cpu(), torch.from_numpy(ref.jpeg_coefs(frames[f:f + 1], q, sub)))


@pytest.mark.parametrize("H,W", ((24, 40), (17, 33)))
@pytest.mark.parametrize("sub", SUBS)
def test_frame_mode(cuda, sub, H, W):
    frames = six(H, W)
    at = lambda kind, q: rr.frame_size(frames[SIX.index(kind)], q, sub)
    for q_max in (95, 100):
        for budget in (900, 700):
            got, info = check_against_restatement(cuda, frames, q_max, sub, frame_bytes=budget)
            q, over = info["qualities"], info["over_budget"]
            for f, kind in enumerate(SIX):                                           # what the restatement's sizes say must happen
                assert over[f] == (at(kind, 1) > budget) and (q[f] == q_max) == (at(kind, q_max) <= budget), (kind, q[f])
                assert over[f] or len(got[f]) <= budget
                if over[f]:
                    assert q[f] == 1 and len(got[f]) == at(kind, 1)
            for f in range(len(SIX)):                                                # the existing fixed-quality path writes the same bytes
                alone = E.encode_jpeg(torch.from_numpy(frames[f:f + 1].copy()).to(cuda), E.JpegConfig(q[f], sub))
                assert alone == [got[f]], (f, q[f])
    if (H, W, sub) == (24, 40, "420"):                                               # the figures the issue was written with
        assert at("ramps", 95) == 889 and at("noise", 1) == 713
        _, info = run(cuda, frames, 95, sub, frame_bytes=900)
        q = dict(zip(SIX, info["qualities"]))
        assert q["ramps"] == 95 and 1 < q["noise"] < 95 and 1 < q["checker"] < 95 and not any(info["over_budget"])
        _, info = run(cuda, frames, 95, sub, frame_bytes=700)
        assert dict(zip(SIX, info["over_budget"]))["noise"] and dict(zip(SIX, info["qualities"]))["noise"] == 1
        # the rule's non-monotone case: 61, although 66 fits as well
        _, info = run(cuda, frames[4:5], 95, sub, frame_bytes=1098)
        assert info["qualities"] == [61] and at("checker", 66) <= 1098


@pytest.mark.parametrize("H,W", ((24, 40), (17, 33)))
@pytest.mark.parametrize("sub", SUBS)
def test_clip_mode(cuda, sub, H, W):
    frames = six(H, W)
    total = lambda q: sum(rr.frame_size(f, q, sub) for f in frames)
    for budget, want_over, want_q in ((total(1) - 1, True, 1), ((total(1) + total(95)) // 2, False, None), (total(95), False, 95)):
        got, info = check_against_restatement(cuda, frames, 95, sub, clip_bytes=budget)
        assert len(set(info["qualities"])) == 1 and info["over_budget"] == [want_over] * 6
        assert want_over or sum(len(j) for j in got) <= budget
        assert want_q is None or info["qualities"][0] == want_q
        if want_q is None:
            assert 1 < info["qualities"][0] < 95
    got, info = check_against_restatement(cuda, frames, 95, sub, clip_bytes=(total(1) + total(95)) // 2, min_quality=30)
    assert 30 <= info["qualities"][0] < 95
    got, info = check_against_restatement(cuda, frames, 95, sub, clip_bytes=total(1), min_quality=30)    # the floor holds although 1 would fit
    assert info["qualities"] == [30] * 6 and info["over_budget"] == [True] * 6
    check_against_restatement(cuda, frames, 100, sub, clip_bytes=(total(1) + total(95)) // 2)
    check_against_restatement(cuda, frames, 41, sub, frame_bytes=800, min_quality=40)                   # two rounds
    check_against_restatement(cuda, frames, 30, sub, frame_bytes=800, min_quality=30)                   # one round


def test_round_trip_and_pipeline(cuda):
    from landiff_amd.decode import decode_jpeg
    frames = six(24, 40)
    zig = E.zigzag_order()
    natural = lambda t: [t[zig.index(n)] for n in range(64)]
    for sub in SUBS:
        got, info = run(cuda, frames, 95, sub, frame_bytes=900)
        assert len(set(info["qualities"])) >= 3                                      # a clip of mixed DQT
        pixels = []
        for j, q in zip(got, info["qualities"]):
            img = Image.open(io.BytesIO(j))
            img.load()
            luma, chroma = E.quant_tables(q)
            tables = {k: list(v) for k, v in img.quantization.items()}
            assert tables in ({0: list(luma), 1: list(chroma)}, {0: natural(luma), 1: natural(chroma)}), q
            pixels.append(np.asarray(img.convert("RGB")))
        assert torch.equal(decode_jpeg(got, cuda).cpu(), torch.from_numpy(np.stack(pixels)))
    from landiff_amd.config import PipelineConfig
    from landiff_amd.pipeline import LanDiffPipeline
    from landiff_amd.weights import init_pipeline_state
    cfg = PipelineConfig.tiny(num_steps=2).check()
    pipe = LanDiffPipeline(cfg, init_pipeline_state(cfg, seed=1234), cuda)
    x = torch.from_numpy(frames.copy())
    for verify in (True, False):
        rate = E.JpegRateConfig(frame_bytes=900)
        jpegs = pipe.encode(x, E.JpegConfig(95, "420"), verify=verify, rate=rate)
        want, q, over, trials = rr.rate_encode(frames, "420", 95, 1, frame_bytes=900)
        assert jpegs == want
        rep = pipe.last_encode
        assert rep["rate"] == E.rate_report(rate, E.JpegConfig(95, "420"), dict(qualities=q, over_budget=over, trials=trials))
        assert rep["rate"]["mode"] == "frame" and rep["rate"]["budget"] == 900 and rep["rate"]["rounds"] == 8
        assert rep["rate"]["quality"]["max"] == 95 and rep["rate"]["over_budget_frames"] == []
        assert ("verify" in rep) == verify
        if verify:
            assert len(rep["verify"]["frames"]["psnr"]) == 6 and 0 < rep["verify"]["clip"]["max_abs"] <= 255
    pipe.encode(x, E.JpegConfig(95, "420"))
    assert "rate" not in pipe.last_encode


@lru_cache(maxsize=None)
def big_frames():
    from test_gpu_jpeg import moving_pattern
    return moving_pattern(2, 480, 720, seed=5)


def check_against_fixed_quality(cuda, frames, q_max, sub, **kw):
    """Final streams and every trial's size against the fixed-quality path, encode_jpeg(JpegConfig(q)) (held to the restatement by
    tests/test_gpu_jpeg.py)."""
    x = torch.from_numpy(np.ascontiguousarray(frames)).to(cuda)
    fixed = lru_cache(maxsize=None)(lambda q: E.encode_jpeg(x, E.JpegConfig(q, sub)))
    got, info = E.encode_jpeg(x, E.JpegConfig(q_max, sub), rate=E.JpegRateConfig(**kw), return_rate=True)
    F = len(frames)
    assert len(info["trials"]) == E.rate_rounds(1, q_max) and info["trials"][0] == [[q_max, len(fixed(q_max)[f])] for f in range(F)]
    for f in range(F):
        assert got[f] == fixed(info["qualities"][f])[f], f
        tried = [row[f] for row in info["trials"]]
        used = [t for t in tried if t[0]]
        assert tried == used + [[0, 0]] * (len(tried) - len(used))
        for q, n in used:
            assert n == len(fixed(q)[f]), (f, q)
    # the rule, replayed on those sizes
    size = lambda f, q: len(fixed(q)[f])
    if "frame_bytes" in kw:
        for f in range(F):
            q, over, tried = rr.bisect(lambda t: size(f, t) <= kw["frame_bytes"], 1, q_max)
            assert (info["qualities"][f], info["over_budget"][f]) == (q, over) and [row[f][0] for row in info["trials"] if row[f][0]] == tried
    else:
        q, over, tried = rr.bisect(lambda t: sum(size(f, t) for f in range(F)) <= kw["clip_bytes"], 1, q_max)
        assert info["qualities"] == [q] * F and info["over_budget"] == [over] * F and [row[0][0] for row in info["trials"] if row[0][0]] == tried
    return got, info


@pytest.mark.parametrize("mode", ("frame", "clip"))
def test_full_size_against_the_fixed_quality_path(cuda, mode):
    frames = big_frames()
    x = torch.from_numpy(frames).to(cuda)
    at95 = [len(j) for j in E.encode_jpeg(x, E.JpegConfig(95, "420"))]
    if mode == "frame":
        budget = min(at95) // 2
        got, info = check_against_fixed_quality(cuda, frames, 95, "420", frame_bytes=budget)
        assert all(len(j) <= budget for j in got) and all(1 < q < 95 for q in info["qualities"]) and not any(info["over_budget"])
    else:
        budget = sum(at95) // 2
        got, info = check_against_fixed_quality(cuda, frames, 95, "420", clip_bytes=budget)
        assert sum(len(j) for j in got) <= budget and 1 < info["qualities"][0] < 95 and not any(info["over_budget"])


def test_wide_frame_whose_segment_passes_the_window(cuda):
    frame = np.random.default_rng(16 + 4096).integers(0, 256, (1, 16, 4096, 3), dtype=np.uint8)
    x = torch.from_numpy(frame).to(cuda)
    top = len(E.encode_jpeg(x, E.JpegConfig(100, "420"))[0])
    assert top - 629 - 2 > 32768                                                     # one segment, longer than the 32 KiB window
    got, info = check_against_fixed_quality(cuda, frame, 100, "420", frame_bytes=top // 2)
    assert len(got[0]) <= top // 2 and 1 < info["qualities"][0] < 100
    got, info = check_against_fixed_quality(cuda, frame, 100, "420", frame_bytes=top)
    assert info["qualities"] == [100] and len(got[0]) == top                         # the final encode itself walks the window in pieces


def test_off_is_unchanged_and_runs_repeat(cuda):
    frames = six(24, 40)
    x = torch.from_numpy(frames.copy()).to(cuda)
    for sub in SUBS:
        cfg = E.JpegConfig(95, sub)
        assert E.encode_jpeg(x, cfg) == E.encode_jpeg(x, cfg, rate=None) == ref.jpeg_encode(frames, 95, sub)
        a = E.encode_jpeg(x, cfg, rate=E.JpegRateConfig(frame_bytes=850), return_rate=True)
        b = E.encode_jpeg(x, cfg, rate=E.JpegRateConfig(frame_bytes=850), return_rate=True)
        assert a == b
        buf, offs, lens, info = E.encode_jpeg(x, cfg, return_device=True, rate=E.JpegRateConfig(frame_bytes=850), return_rate=True)
        assert buf.is_cuda and info == a[1] and lens.tolist() == [len(j) for j in a[0]]
        assert offs.tolist() == [sum(lens.tolist()[:f]) for f in range(6)] and buf.numel() == sum(lens.tolist())
        assert E.encode_jpeg(x, cfg, rate=E.JpegRateConfig(frame_bytes=850)) == a[0]
        a = E.encode_jpeg(x, cfg, rate=E.JpegRateConfig(clip_bytes=5000), return_rate=True)
        assert a == E.encode_jpeg(x, cfg, rate=E.JpegRateConfig(clip_bytes=5000), return_rate=True)


def test_command_line_caps_the_file(cuda, tmp_path):
    """--video_max_bytes N: the .avi on disk takes at most N bytes (one quality), --jpeg_frame_bytes N: every stream at most N;
    <name>_encode.json carries the rate report."""
    import landiff.infer_video as iv
    from landiff.utils import mjpeg_avi_bytes, mjpeg_avi_stream_budget, read_mjpeg_avi_chunks
    from test_gpu_jpeg import moving_pattern
    frames = torch.from_numpy(moving_pattern(9, 40, 56, seed=9))
    torch.cuda.set_device(cuda)
    plain = E.encode_jpeg(frames.to(cuda), E.JpegConfig())
    cap = mjpeg_avi_bytes([len(j) for j in plain]) * 2 // 3
    iv._save_video(iv.parse_args(["--prompt", "p", "--video_encoder", "gpu", "--video_max_bytes", str(cap), "--encode_verify"]), frames,
                   str(tmp_path / "clip.mp4"), fps=8)
    assert os.path.getsize(tmp_path / "clip.avi") <= cap
    rep = json.load(open(tmp_path / "clip_encode.json"))
    budget = mjpeg_avi_stream_budget(cap, 9)
    want, q, over, trials = rr.rate_encode(frames.numpy(), "420", 95, 1, clip_bytes=budget)
    unpad = lambda chunks, streams: [c[:len(j)] for c, j in zip(chunks, streams) if len(c) == len(j) + (len(j) & 1)]     # (chunks are word aligned)
    assert unpad(read_mjpeg_avi_chunks(tmp_path / "clip.avi")[0], want) == want
    assert rep["rate"]["mode"] == "clip" and rep["rate"]["budget"] == budget and rep["rate"]["video_max_bytes"] == cap
    assert rep["rate"]["quality"] == {"min": q[0], "mean": q[0], "max": q[0]} and rep["rate"]["over_budget_frames"] == [] and 1 < q[0] < 95
    assert rep["total_bytes"] == sum(len(j) for j in want) <= budget and 0 < rep["verify"]["clip"]["max_abs"] <= 255
    iv._save_video(iv.parse_args(["--prompt", "p", "--video_encoder", "gpu", "--jpeg_frame_bytes", "1500"]), frames, str(tmp_path / "f" / "clip.mp4"))
    chunks = read_mjpeg_avi_chunks(tmp_path / "f" / "clip.avi")[0]
    want, q, over, _ = rr.rate_encode(frames.numpy(), "420", 95, 1, frame_bytes=1500)
    assert unpad(chunks, want) == want and all(len(j) <= 1500 or o for j, o in zip(want, over))
    assert json.load(open(tmp_path / "f" / "clip_encode.json"))["rate"]["mode"] == "frame"
    with pytest.raises(ValueError, match="leaves nothing"):
        iv._save_video(iv.parse_args(["--prompt", "p", "--video_encoder", "gpu", "--video_max_bytes", "300"]), frames, str(tmp_path / "n" / "clip.mp4"))
    assert not (tmp_path / "n").exists()
