"""The decode stage's second entropy route on the GPU (csrc/ld_jpeg_dec_sync.hip) against the lane-per-segment route,
the restatement of its rule (tests/jpeg_sync_ref.py) and PIL: coefficients, status words, the exit table and pixels with
torch.equal -- integer arithmetic, there is no tolerance."""
import numpy as np
import pytest
import torch

import jpeg_dec_ref as dref
import jpeg_ref as ref
import jpeg_sync_ref as sref
from landiff_amd import decode as D
from landiff_amd import encode as E
from test_gpu_jpeg_dec import stage_inputs, streams
from test_jpeg_dec_host import MALFORMED, pil_decode, pil_write
from test_jpeg_sync_host import SUB_BYTES, names, reencoded, serial, stream, synced

pytestmark = pytest.mark.gpu


def run_both(jpegs, dev, sub_bytes=256, max_rounds=32, exits=False):
    """Both routes on the same segment table -> (inputs, (coefs, status) of the segment route, what the sync route returns)."""
    from landiff_amd import ops
    inp = stage_inputs(jpegs, dev)
    i0 = inp["infos"][0]
    args = (inp["data"],) + ops.jpeg_find_segments(inp["data"], inp["scan"], inp["ri"], inp["rows"], i0.height, i0.width, i0.subsampling) + (
        inp["ri"], inp["tables"], inp["tset"], i0.height, i0.width, i0.subsampling)
    return inp, ops.jpeg_decode_entropy(*args), ops.jpeg_decode_entropy_sync(*args, sub_bytes=sub_bytes, max_rounds=max_rounds, return_exits=exits)


def want_exits(got, s=0):
    return torch.tensor(got["exits"][s], dtype=torch.int64).reshape(-1, 4)


@pytest.mark.parametrize("sub_bytes", SUB_BYTES)
def test_routes_agree_and_the_exit_table_is_the_restatements(cuda, sub_bytes):
    """(a) every family, one stream a call, max_rounds >= the stream's subsequences: no fallback, and E is the restatement's."""
    for name in names():
        want = synced(name, sub_bytes)
        rounds = max(max(want["n"]), 1)
        _, (c0, s0), (c1, s1, info, (exits, index)) = run_both([stream(name)], cuda, sub_bytes, rounds, exits=True)
        assert torch.equal(c1, c0) and torch.equal(s1, s0) and not s1.any(), (name, int((c1 != c0).sum()), s1.tolist())
        assert np.array_equal(c1[0].cpu().numpy(), serial(name)["coefs"]), name
        info, index, exits = info.cpu(), index.cpu(), exits.cpu()
        assert not info[..., 1].any(), (name, info.tolist())
        assert info[0, :, 0].tolist() == want["rounds"].tolist(), (name, info.tolist(), want["rounds"])
        assert index[0, :, 1].tolist() == want["n"], name
        for s in range(len(want["n"])):
            at, n = index[0, s].tolist()
            assert torch.equal(exits[at:at + n], want_exits(want, s)), (name, s)


@pytest.mark.parametrize("sub_bytes", SUB_BYTES)
def test_one_round_falls_back_and_stays_exact(cuda, sub_bytes):
    """(b) max_rounds = 1: what has not settled is decoded by the lane-per-segment kernel in the same call."""
    noise = ("pil", "noise", 48, 64, 100, "420")
    assert synced(noise, sub_bytes, 1)["fell"].all()                           # the restatement: the fallback is really taken
    for name in names():
        want = synced(name, sub_bytes, 1)
        _, (c0, s0), (c1, s1, info) = run_both([stream(name)], cuda, sub_bytes, 1)
        assert torch.equal(c1, c0) and torch.equal(s1, s0) and not s1.any(), name
        assert info[0, :, 1].tolist() == want["fell"].tolist() and info[0, :, 0].tolist() == want["rounds"].tolist(), name
        if name == noise:
            assert info[..., 1].any()


def test_segments_of_every_kind_in_one_call(cuda):
    """(c) restart intervals 1, 5 and 0 together (rows a frame does not use), and table sets that differ per frame."""
    for sub in ("420", "444"):
        jpegs = [reencoded("noise", sub, 1), reencoded("ramps", sub, 5), reencoded("bars", sub, 0), reencoded("ramps", sub, 4)]
        for sub_bytes, rounds in ((64, 64), (256, 1)):
            inp, (c0, s0), (c1, s1, info, (exits, index)) = run_both(jpegs, cuda, sub_bytes, rounds, exits=True)
            assert torch.equal(c1, c0) and torch.equal(s1, s0) and not s1.any()
            for f, (j, i) in enumerate(zip(jpegs, inp["infos"])):
                want = sref.decode(j, sub_bytes, rounds, rows=inp["rows"])
                assert info[f, :, 0].tolist() == want["rounds"].tolist() and info[f, :, 1].tolist() == want["fell"].tolist()
                assert index[f, :, 1].tolist() == want["n"] and not index[f, i.segments:, 1].any()
                for s in range(i.segments):
                    at, n = index[f, s].tolist()
                    assert torch.equal(exits[at:at + n].cpu(), want_exits(want, s)), (f, s)
    jpegs = list(streams(("optimised",)))
    assert len(set(stage_inputs(jpegs, cuda)["tset"].tolist())) == 3
    for sub_bytes in SUB_BYTES:
        _, (c0, s0), (c1, s1, info) = run_both(jpegs, cuda, sub_bytes, 64)
        assert torch.equal(c1, c0) and torch.equal(s1, s0) and not s1.any() and not info[..., 1].any()


@pytest.mark.parametrize("make", MALFORMED)
def test_malformed_streams_give_the_segment_routes_status(cuda, make):
    """(d) the same status rows and coefficients as the segment route, the same ValueError text."""
    bad, statuses = make()
    good = ref.jpeg_encode(ref.picture("bars", 24, 40)[None], 95, "420")[0]
    for sub_bytes in SUB_BYTES:
        _, (c0, s0), (c1, s1, info) = run_both([good, bad], cuda, sub_bytes, 32)
        assert s1.tolist() == [[0, 0], statuses] == s0.tolist() and torch.equal(c1, c0)
        assert info[..., 1].tolist() == [[0, 0], [int(v not in (dref.OK, dref.MARKERS)) for v in statuses]]
    first = next(s for s, v in enumerate(statuses) if v)
    texts = []
    for route in ("segment", "sync"):
        with pytest.raises(ValueError, match=f"frame 1 segment {first}: {D.STATUS[statuses[first]]}") as e:
            D.decode_jpeg([good, bad], cuda, entropy=route)
        texts.append(str(e.value))
    assert texts[0] == texts[1]


def test_pixels_and_reports(cuda):
    """(e) decode_jpeg by the three routes: equal pixels, PIL's; repeatable; frames=, a strided out= and the device triple."""
    jpegs = [pil_write(ref.picture(k, 50, 70, s), quality=95) for s, k in enumerate(("noise", "ramps", "checker"))]
    want = np.stack([pil_decode(j) for j in jpegs])
    seg = D.decode_jpeg(jpegs, cuda)
    for route in ("sync", "auto"):
        report = {}
        got = D.decode_jpeg(jpegs, cuda, entropy=route, sub_bytes=128, report=report)
        assert torch.equal(got, seg) and np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(D.decode_jpeg(jpegs, cuda, entropy=route, sub_bytes=128), got)                  # bit-repeatable
        chosen = route if route == "sync" else D.entropy_route([D.parse_jpeg(j) for j in jpegs], [len(j) for j in jpegs], 128)
        assert report["entropy"] == chosen and report["frames"] == 3 and report["frames_without_restarts"] == 3
        if chosen == "sync":
            assert report["sub_bytes"] == 128 and report["segments_fallen_back"] == 0
            assert 0 <= report["rounds"]["mean"] <= report["rounds"]["max"] <= 32
    report = {}
    D.decode_jpeg(jpegs, cuda, report=report)
    assert report["entropy"] == "segment" and report["rounds"] is None and report["decoder"] == "gpu"
    ours = ref.jpeg_encode(np.stack([ref.picture("noise", 50, 70)]), 95, "420")
    D.decode_jpeg(ours, cuda, entropy="auto", report=report)
    assert report["entropy"] == "segment"                                      # short segments: auto keeps the lane per segment
    big = torch.full((3, 57, 90, 3), 201, dtype=torch.uint8, device=cuda)
    view = big[:, 4:54, 11:81]
    out = D.decode_jpeg(jpegs, cuda, out=view, entropy="sync")
    assert out.data_ptr() == view.data_ptr() and np.array_equal(view.cpu().numpy(), want)
    outside = big.cpu().numpy().copy()
    outside[:, 4:54, 11:81] = 201
    assert (outside == 201).all()
    part, coefs = D.decode_jpeg(jpegs, cuda, frames=[2, 0], entropy="sync", return_coefs=True)
    assert np.array_equal(part.cpu().numpy(), want[[2, 0]])
    assert torch.equal(coefs, D.decode_jpeg(jpegs, cuda, frames=[2, 0], return_coefs=True)[1])
    frames = torch.from_numpy(np.concatenate([ref.clip3("noise", 50, 70), ref.clip3("ramps", 50, 70)])).to(cuda)
    triple = E.encode_jpeg(frames, E.JpegConfig(90, "444"), return_device=True)
    for kw in (dict(), dict(frames=[4, 1])):
        assert torch.equal(D.decode_jpeg(triple, entropy="sync", sub_bytes=64, **kw), D.decode_jpeg(triple, **kw))


def test_full_size_against_pil(cuda):
    """(f) two 480 x 720 frames written by PIL (no restart markers) and by encode_jpeg, the defaults: PIL's pixels, no fallback."""
    frames = np.stack([ref.picture("noise", 480, 720), ref.picture("ramps", 480, 720)])
    ours = E.encode_jpeg(torch.from_numpy(frames).to(cuda), E.JpegConfig(95, "420"))
    pils = [pil_write(f, quality=95) for f in frames]
    for jpegs in (ours, pils):
        report = {}
        got = D.decode_jpeg(jpegs, cuda, entropy="sync", report=report).cpu().numpy()
        assert np.array_equal(got, np.stack([pil_decode(j) for j in jpegs]))
        assert report["segments_fallen_back"] == 0 and report["sub_bytes"] == 256, report
    report = {}
    got = D.decode_jpeg(pils, cuda, entropy="auto", report=report).cpu().numpy()               # long segments: auto takes the sync route
    assert report["entropy"] == "sync" and report["segments_fallen_back"] == 0 and np.array_equal(got, np.stack([pil_decode(j) for j in pils]))


def test_load_clip_and_the_pipeline_take_the_route(cuda, tmp_path):
    """(g) load_clip(..., "gpu", entropy="sync") on a host-written .avi equals read_mjpeg_avi; LanDiffPipeline.decode_jpegs."""
    import json
    import landiff.infer_video as iv
    from landiff.utils import read_mjpeg_avi, read_mjpeg_avi_chunks, write_mjpeg_avi
    from landiff_amd.config import PipelineConfig
    from landiff_amd.pipeline import LanDiffPipeline
    from landiff_amd.weights import init_pipeline_state
    torch.cuda.set_device(cuda)
    images = np.concatenate([ref.clip3("noise", 34, 50), ref.clip3("ramps", 34, 50)])
    path = str(tmp_path / "host.avi")
    write_mjpeg_avi(images, path, fps=8)
    frames, _ = read_mjpeg_avi(path)
    for route in ("sync", "auto"):
        clip = iv.load_clip(path, "gpu", report=str(tmp_path / "clip_decode.json"), entropy=route)
        assert clip.is_cuda and np.array_equal(clip.cpu().numpy(), frames)
        rep = json.load(open(tmp_path / "clip_decode.json"))
        assert rep["entropy"] in ("sync", "segment") and rep["frames"] == 6 and (route != "sync" or rep["segments_fallen_back"] == 0)
    part = iv.load_clip(path, "gpu", needed=lambda F, H, W: (F - 1, 1), entropy="sync")
    assert np.array_equal(part[[1, 5]].cpu().numpy(), frames[[1, 5]]) and not part[[0, 2, 3, 4]].any()
    cfg = PipelineConfig.tiny(num_steps=2).check()
    pipe = LanDiffPipeline(cfg, init_pipeline_state(cfg, seed=1234), cuda)
    chunks = read_mjpeg_avi_chunks(path)[0]
    got = pipe.decode_jpegs(chunks, entropy="sync", sub_bytes=64, max_rounds=8)
    assert np.array_equal(got.cpu().numpy(), frames) and pipe.last_decode["entropy"] == "sync" and pipe.last_decode["sub_bytes"] == 64
