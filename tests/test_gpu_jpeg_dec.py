"""The decode stage on the GPU (csrc/ld_jpeg_dec.hip; landiff_amd/decode.py) against the numpy restatement of its rule
(tests/jpeg_dec_ref.py) and against PIL: segment tables, coefficients and pixels with torch.equal -- the rule is integer
arithmetic, there is no tolerance."""
import json
from functools import lru_cache

import numpy as np
import pytest
import torch

import jpeg_dec_ref as dref
import jpeg_ref as ref
from landiff_amd import decode as D
from landiff_amd import encode as E
from test_jpeg_dec_host import MALFORMED, SMALL, pil_decode, pil_write

pytestmark = pytest.mark.gpu


def _names():
    names = [("ref", k, H, W, 95, "420") for H, W in ref.SIZES for k in ref.FAMILIES]
    names += [("ref", k, H, W, q, "444") for H, W in ref.SIZES for k, q in (("noise", 100), ("ramps", 50), ("bars", 1))]
    names += [("ref", k, H, W, 95, sub) for H, W in SMALL for k in ("noise", "ramps") for sub in ("420", "444")]
    return names + [("maximising", q) for q in (95, 100)] + [("dense_ff", sub) for sub in ("444", "420")] + [("optimised",)]


@lru_cache(maxsize=None)
def streams(name):
    """The JPEG streams of one clip (a tuple of bytes)."""
    if name[0] == "ref":
        _, kind, H, W, quality, sub = name
        return tuple(ref.jpeg_encode(ref.clip3(kind, H, W), quality, sub))
    if name[0] == "maximising":
        return tuple(ref.jpeg_encode(ref.maximising_frames(), name[1], "420"))
    if name[0] == "dense_ff":                                # 24 blocks: 8 MCUs at 4:4:4 (8 x 64), 4 at 4:2:0 (16 x 64); quantisers 1
        H = 8 if name[1] == "444" else 16
        return (dref.encode_coefs(ref.dense_ff_blocks(24), H, 64, 100, name[1], 64 // E.mcu_size(name[1])),)
    if name[0] == "optimised":                               # three frames, three table sets PIL fitted to each, no restart markers
        out = tuple(pil_write(ref.picture(k, 34, 50, s), quality=q, optimize=True) for s, (k, q) in enumerate((("noise", 95), ("ramps", 75), ("bars", 50))))
        assert len({(i.quant, i.huffman) for i in map(D.parse_jpeg, out)}) == 3
        return out
    raise KeyError(name)


@lru_cache(maxsize=None)
def want(name):
    """The restatement's decode of every stream of the clip (computed once, never modified)."""
    return tuple(dref.decode(j) for j in streams(name))


def stage_inputs(jpegs, dev):
    """What decode_jpeg hands the kernels, built here from the headers: -> dict of device tensors and the host's infos."""
    infos = [D.parse_jpeg(j) for j in jpegs]
    starts = np.cumsum([0] + [len(j) for j in jpegs[:-1]]).tolist()
    sets = {}
    tset = [sets.setdefault((i.quant, i.huffman), len(sets)) for i in infos]
    words = [D.decode_tables(next(i for i, t in zip(infos, tset) if t == s)) for s in range(len(sets))]
    return dict(infos=infos, starts=starts, rows=max(i.segments for i in infos),
                data=torch.frombuffer(bytearray(b"".join(jpegs)), dtype=torch.uint8).to(dev),
                scan=torch.tensor([[s + i.scan_offset, len(j) - i.scan_offset] for s, i, j in zip(starts, infos, jpegs)], dtype=torch.int64).to(dev),
                ri=torch.tensor([i.restart_interval for i in infos], dtype=torch.int32).to(dev),
                tset=torch.tensor(tset, dtype=torch.int32).to(dev), tables=torch.tensor(words, dtype=torch.int32).to(dev))


def want_tables(jpegs, inp):
    joined = b"".join(jpegs)
    rows = [dref.find_segments(joined, s + i.scan_offset, len(j) - i.scan_offset, i.restart_interval, i.mcus, inp["rows"], frame=f)
            for f, (s, i, j) in enumerate(zip(inp["starts"], inp["infos"], jpegs))]
    return torch.from_numpy(np.stack([r[0] for r in rows])), torch.from_numpy(np.stack([r[1] for r in rows]))


def run_stages(jpegs, dev):
    from landiff_amd import ops
    inp = stage_inputs(jpegs, dev)
    i0 = inp["infos"][0]
    seg, finfo = ops.jpeg_find_segments(inp["data"], inp["scan"], inp["ri"], inp["rows"], i0.height, i0.width, i0.subsampling)
    coefs, status = ops.jpeg_decode_entropy(inp["data"], seg, finfo, inp["ri"], inp["tables"], inp["tset"], i0.height, i0.width, i0.subsampling)
    return inp, seg.cpu(), finfo.cpu(), coefs, status.cpu()


def reencoded(kind, sub, ri, quality=100):
    """A 24 x 40 frame coded by the restatement's coder at the restart interval ri (0: none)."""
    frame = ref.picture(kind, 24, 40)
    return dref.encode_coefs(ref.jpeg_coefs(frame[None], quality, sub)[0], 24, 40, quality, sub, ri)


def test_segments_match_the_restatement(cuda):
    """One MCU row per interval (scans of several 4 KiB chunks), intervals of 1 and 5 MCUs (fourteen markers: the numbering wraps;
    a last segment that is shorter), no DRI, and the three in one call (rows the frame does not use)."""
    clips = [streams(("ref", "noise", 50, 70, 100, "444")), streams(("ref", "noise", 50, 70, 95, "420")), streams(("optimised",))]
    for sub in ("420", "444"):
        clips += [(reencoded("noise", sub, 1),), (reencoded("noise", sub, 5),), (reencoded("ramps", sub, 0),),
                  (reencoded("noise", sub, 1), reencoded("ramps", sub, 5), reencoded("bars", sub, 0), reencoded("ramps", sub, 4))]
    assert len(clips[0][0]) > 3 * 4096
    for jpegs in clips:
        inp, seg, finfo, _, status = run_stages(list(jpegs), cuda)
        w_seg, w_info = want_tables(jpegs, inp)
        assert torch.equal(finfo, w_info), (finfo, w_info)
        assert torch.equal(seg, w_seg), [(i.restart_interval, i.segments) for i in inp["infos"]]
        assert not status.any()
        for f, i in enumerate(inp["infos"]):                               # the table tiles the entropy-coded data
            assert int(finfo[f, 0]) == i.segments - 1 and int(seg[f, :i.segments, 4].sum()) == i.mcus


def test_entropy_matches_the_restatement(cuda):
    for name in _names():
        jpegs = list(streams(name))
        _, _, _, coefs, status = run_stages(jpegs, cuda)
        w = torch.from_numpy(np.stack([d["coefs"] for d in want(name)]))
        assert not status.any(), (name, status)
        assert coefs.dtype == torch.int16 and coefs.shape == w.shape and torch.equal(coefs.cpu(), w), (name, int((coefs.cpu() != w).sum()))


def test_decode_inverts_the_encoder_on_the_device(cuda):
    """encode_jpeg's own output, never copied back but for its headers: the coefficients are ops.jpeg_coefs_u8's."""
    from landiff_amd import ops
    for sub in ("420", "444"):
        frames = torch.from_numpy(np.concatenate([ref.clip3("noise", 50, 70), ref.clip3("ramps", 50, 70)])).to(cuda)
        triple = E.encode_jpeg(frames, E.JpegConfig(90, sub), return_device=True)
        pixels, coefs = D.decode_jpeg(triple, return_coefs=True)
        assert torch.equal(coefs, ops.jpeg_coefs_u8(frames, 90, sub))
        jpegs = E.encode_jpeg(frames, E.JpegConfig(90, sub))
        assert np.array_equal(pixels.cpu().numpy(), np.stack([pil_decode(j) for j in jpegs]))
        part = D.decode_jpeg(triple, frames=[4, 1])
        assert torch.equal(part, pixels[[4, 1]])


def test_pixels_match_the_restatement_and_pil(cuda):
    for name in _names():
        jpegs = list(streams(name))
        got = D.decode_jpeg(jpegs, cuda)
        again = D.decode_jpeg(jpegs, cuda)
        w = np.stack([d["pixels"] for d in want(name)])
        assert got.dtype == torch.uint8 and tuple(got.shape) == w.shape and got.device == cuda
        assert torch.equal(got, again), name                               # bit-repeatable
        assert np.array_equal(got.cpu().numpy(), w), (name, int((got.cpu().numpy() != w).sum()))
        assert np.array_equal(w, np.stack([pil_decode(j) for j in jpegs])), name


def test_strided_output_and_chosen_frames(cuda):
    name = ("ref", "noise", 50, 70, 95, "420")
    jpegs = list(streams(name))
    w = np.stack([d["pixels"] for d in want(name)])
    big = torch.full((3, 57, 90, 3), 201, dtype=torch.uint8, device=cuda)
    view = big[:, 4:54, 11:81]
    assert not view.is_contiguous() and view.stride(1) == 270
    out = D.decode_jpeg(jpegs, cuda, out=view)
    assert out.data_ptr() == view.data_ptr() and np.array_equal(view.cpu().numpy(), w)
    outside = big.cpu().numpy().copy()
    outside[:, 4:54, 11:81] = 201
    assert (outside == 201).all()                                          # nothing beyond the window is touched
    report = {}
    got = D.decode_jpeg(jpegs, cuda, frames=[2, 0], report=report)
    assert np.array_equal(got.cpu().numpy(), w[[2, 0]])
    assert report["frames"] == 2 and report["table_sets"] == 1 and report["segments_per_frame"] == {"min": 4, "max": 4}
    assert report["total_bytes"] == len(jpegs[2]) + len(jpegs[0])
    mixed = [streams(("optimised",))[0], ref.jpeg_encode(ref.picture("ramps", 34, 50)[None], 95, "420")[0]]      # tables, DHT and DRI differ
    assert np.array_equal(D.decode_jpeg(mixed, cuda).cpu().numpy(), np.stack([pil_decode(j) for j in mixed]))


def test_full_size_against_pil(cuda):
    frames = np.stack([ref.picture("noise", 480, 720), ref.picture("ramps", 480, 720)])
    ours = E.encode_jpeg(torch.from_numpy(frames).to(cuda), E.JpegConfig(95, "420"))
    pils = [pil_write(f, quality=95) for f in frames]                      # no restart markers: one lane per frame
    for jpegs in (ours, pils):
        got = D.decode_jpeg(jpegs, cuda).cpu().numpy()
        assert np.array_equal(got, np.stack([pil_decode(j) for j in jpegs]))


def test_encode_verify_reports_the_loss(cuda):
    from landiff_amd.config import PipelineConfig
    from landiff_amd.metrics import compare_clips
    from landiff_amd.pipeline import LanDiffPipeline
    from landiff_amd.weights import init_pipeline_state
    cfg = PipelineConfig.tiny(num_steps=2).check()
    pipe = LanDiffPipeline(cfg, init_pipeline_state(cfg, seed=1234), cuda)
    frames = torch.from_numpy(np.concatenate([ref.clip3("noise", 50, 70), ref.clip3("ramps", 50, 70)]))
    jpegs = pipe.encode(frames, E.JpegConfig(80, "420"), verify=True)
    assert jpegs == ref.jpeg_encode(frames.numpy(), 80, "420")
    decoded = torch.from_numpy(np.stack([pil_decode(j) for j in jpegs])).to(cuda)
    m = compare_clips(frames.to(cuda), decoded).as_dict()
    v = pipe.last_encode["verify"]
    assert v["clip"] == m["clip"] and v["frames"] == {k: m["frames"][k] for k in ("psnr", "ssim", "max_abs")}
    assert 0 < v["clip"]["max_abs"] <= 255 and v["clip"]["psnr"] > 10 and pipe.last_encode["frames"] == 6
    pipe.encode(frames, E.JpegConfig(80, "420"))
    assert "verify" not in pipe.last_encode                                # opt-in
    got = pipe.decode_jpegs(jpegs, frames=[5])
    assert torch.equal(got, decoded[5:]) and pipe.last_decode["frames"] == 1 and pipe.timings["decode"] > 0


@pytest.mark.parametrize("make", MALFORMED)
def test_malformed_streams_are_refused_by_status(cuda, make):
    """The restatement's status per segment, and a ValueError naming the first; the stream beside it in the call decodes clean."""
    bad, statuses = make()
    good = ref.jpeg_encode(ref.picture("bars", 24, 40)[None], 95, "420")[0]
    _, _, _, _, status = run_stages([good, bad], cuda)
    assert status.tolist() == [[0, 0], statuses]
    assert dref.decode(bad)["status"].tolist() == statuses
    first = next(s for s, v in enumerate(statuses) if v)
    with pytest.raises(ValueError, match=f"frame 1 segment {first}: {D.STATUS[statuses[first]]}"):
        D.decode_jpeg([good, bad], cuda)


def test_load_clip_with_the_gpu_decoder(cuda, tmp_path):
    """--video_decoder gpu at the load_clip level: a file of the GPU encoder and one of the host writer, each equal to
    read_mjpeg_avi's frames; with a plan only the frames it reads are decoded."""
    import landiff.infer_video as iv
    from landiff.utils import read_mjpeg_avi, write_mjpeg_avi, write_mjpeg_avi_encoded
    torch.cuda.set_device(cuda)
    images = np.concatenate([ref.clip3("noise", 34, 50), ref.clip3("ramps", 34, 50)])
    write_mjpeg_avi_encoded(E.encode_jpeg(torch.from_numpy(images).to(cuda), E.JpegConfig()), (50, 34), tmp_path / "gpu.avi", fps=8)
    write_mjpeg_avi(images, tmp_path / "host.avi", fps=8)
    for name in ("gpu.avi", "host.avi"):
        path = str(tmp_path / name)
        frames, _ = read_mjpeg_avi(path)
        clip = iv.load_clip(path, "gpu", report=str(tmp_path / "out" / "clip_decode.json"))
        assert clip.is_cuda and clip.dtype == torch.uint8 and np.array_equal(clip.cpu().numpy(), frames)
        host = iv.load_clip(path)
        assert not host.is_cuda and np.array_equal(host.numpy(), frames)
        rep = json.load(open(tmp_path / "out" / "clip_decode.json"))
        assert rep["frames"] == rep["clip_frames"] == 6 and rep["decoder"] == "gpu" and (rep["width"], rep["height"]) == (50, 34)
        assert rep["frames_without_restarts"] == (0 if name == "gpu.avi" else 6)
        part = iv.load_clip(path, "gpu", needed=lambda F, H, W: (F - 1, 1, 1) if (F, H, W) == (6, 34, 50) else None)
        want_part = np.zeros_like(frames)
        want_part[[1, 5]] = frames[[1, 5]]
        assert np.array_equal(part.cpu().numpy(), want_part)
    args = iv.parse_args(["--prompt", "p", "--video_encoder", "gpu", "--encode_verify"])
    iv._save_video(args, torch.from_numpy(images), str(tmp_path / "v" / "clip.mp4"), fps=8)
    rep = json.load(open(tmp_path / "v" / "clip_encode.json"))
    frames, _ = read_mjpeg_avi(tmp_path / "v" / "clip.avi")
    assert rep["verify"]["clip"]["max_abs"] == int(np.abs(frames.astype(int) - images.astype(int)).max()) > 0
