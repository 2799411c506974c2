"""Clip comparison, the part that needs no GPU: the two restatements of tests/metrics_ref.py against each other and against closed
forms, the host arithmetic of landiff_amd.metrics (PSNR rules, the JSON writer), the argument checks and the CLI's two flags."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def test_window_table_matches_the_product():
    from landiff_amd import ops
    w = R.window32()
    assert w.dtype == torch.float32 and w.numel() == 11 == ops.SSIM_TAPS
    assert torch.equal(w, torch.from_numpy(ops.ssim_window()))
    assert torch.equal(w, w.flip(0)) and abs(float(w.double().sum()) - 1.0) < 1e-7


def test_tile_constants_match_the_header():
    from landiff_amd import ops
    hdr = open(os.path.join(ROOT, "include", "landiff_hip.h")).read()
    d = {k: int(v) for k, v in re.findall(r"#define (LD_SSIM_[A-Z_]+) (\d+)", hdr)}
    assert d == {"LD_SSIM_TAPS": ops.SSIM_TAPS, "LD_SSIM_TILE_H": ops.SSIM_TILE_H, "LD_SSIM_TILE_ELEMS": ops.SSIM_TILE_ELEMS}


def test_restatements_agree():
    """fp32 in the kernel's order against float64 by the definition: random frames agree to fp32's few 1e-7 per mean; the masked
    sums count the kept centres."""
    a, b = _rand((2, 23, 31, 3), 1), _rand((2, 23, 31, 3), 2)
    mask = torch.rand(2, 23, 31, generator=torch.Generator().manual_seed(3)) < 0.6
    for m in (None, mask):
        r64, r32 = R.ssim_ref64(a, b, m), R.ssim_ref32(a, b, m)
        assert torch.equal(r64[..., 1], r32[..., 1])
        want = 13 * 21 if m is None else None
        if want:
            assert (r64[..., 1] == want).all()
        else:
            assert torch.equal(r64[..., 1], mask[:, 5:18, 5:26].sum((1, 2)).double()[:, None].expand(2, 3))
        assert (R.mean_of(r64) - R.mean_of(r32)).abs().max() < 2e-6
    # The offset changes nothing for a window that sums to 1.  The fp32 table sums to S = 1 - 1.4e-9 per axis, which moves each
    # variance by (1 - S^2)(128^2 - 256 mu), at most 1.4e-4 against C2 = 58.5: float64 with and without the offset differ by that.
    S = float(R.window32().double().sum())
    assert abs(1.0 - S) < 2e-9
    m0, m128 = R.ssim_map(a, b, torch.float64, 0.0), R.ssim_map(a, b, torch.float64, 128.0)
    assert (m0 - m128).abs().max() < 2.0 * (1.0 - S * S) * 256.0 * 191.0 / R.C2


def test_ssim_of_a_clip_with_itself_is_exactly_one():
    a = _rand((1, 17, 19, 3), 4)
    for ref in (R.ssim_ref64, R.ssim_ref32):
        s = ref(a, a)
        assert torch.equal(s[..., 0], s[..., 1])


@pytest.mark.parametrize("u,v", [(0, 0), (0, 255), (255, 255), (17, 200), (128, 129), (254, 255)])
def test_constant_frames_closed_form(u, v):
    a = torch.full((1, 12, 14, 1), u, dtype=torch.uint8)
    b = torch.full((1, 12, 14, 1), v, dtype=torch.uint8)
    want = (2.0 * u * v + R.C1) / (u * u + v * v + R.C1)
    # The fp32 table sums to S per axis, a hair under 1, so by the definition a constant frame has the variance u^2 S^2 (1 - S^2):
    # the contrast term is 1 - (u - v)^2 S^2 (1 - S^2) / (.. + C2), and the luminance term moves by less than 2 (1 - S^2).
    S2 = float(R.window32().double().sum()) ** 2
    tol = (u - v) ** 2 * (1.0 - S2) / R.C2 + 2.0 * (1.0 - S2) + 1e-12
    assert abs(float(R.mean_of(R.ssim_ref64(a, b))) - want) < tol < 4e-6
    assert abs(float(R.mean_of(R.ssim_ref32(a, b))) - want) < 1e-4


def test_diff_ref_by_hand():
    a = torch.tensor([[[[0, 10, 255]], [[3, 3, 3]]]], dtype=torch.uint8)          # [1, 2, 1, 3]
    b = torch.tensor([[[[255, 10, 0]], [[4, 3, 1]]]], dtype=torch.uint8)
    got = R.diff_ref(a, b)
    assert got.tolist() == [[[2, 255 * 255 + 1, 256, 255, 2], [2, 0, 0, 0, 0], [2, 255 * 255 + 4, 257, 255, 2]]]
    mask = torch.tensor([[[True], [False]]])
    assert R.diff_ref(a, b, mask).tolist() == [[[1, 255 * 255, 255, 255, 1], [1, 0, 0, 0, 0], [1, 255 * 255, 255, 255, 1]]]


def test_psnr_rules_and_host_metrics():
    from landiff_amd.metrics import metrics_from_sums, psnr_from_sums
    p = psnr_from_sums(torch.tensor([0, 0, 100, 65025 * 7]), torch.tensor([5, 0, 100, 7]))
    assert p[0] == math.inf and math.isnan(p[1]) and abs(p[2] - 10 * math.log10(65025.0)) < 1e-12 and p[3] == 0.0
    # two frames, three channels: frame 0 identical, frame 1 nothing counted
    diff = torch.zeros(2, 3, 5, dtype=torch.int64)
    diff[0, :, 0] = 50
    ssim = torch.zeros(2, 3, 2, dtype=torch.float64)
    ssim[0, :, 0] = ssim[0, :, 1] = 20.0
    m = metrics_from_sums((2, 10, 5, 3), diff, ssim)
    assert m.psnr[0] == math.inf and math.isnan(m.psnr[1]) and m.ssim[0] == 1.0 and math.isnan(m.ssim[1])
    assert m.mse[0] == 0.0 and math.isnan(m.mse[1]) and m.counted.tolist() == [150, 0] and m.differing.tolist() == [0, 0]
    assert m.clip_psnr == math.inf and m.clip_ssim == 1.0 and m.clip_counted == 150 and m.clip_mse == 0.0
    # the clip's PSNR comes from the clip's total squared difference, not from the frames' PSNRs
    diff = torch.tensor([[[10, 40, 20, 2, 10]], [[10, 0, 0, 0, 0]]])
    m = metrics_from_sums((2, 2, 5, 1), diff, None)
    assert m.ssim is None and m.clip_ssim is None
    assert abs(m.clip_psnr - 10 * math.log10(65025.0 * 20 / 40)) < 1e-12 and m.psnr[1] == math.inf and m.clip_max_abs == 2
    none = metrics_from_sums((1, 2, 2, 1), torch.zeros(1, 1, 5, dtype=torch.int64), torch.zeros(1, 1, 2, dtype=torch.float64))
    assert math.isnan(none.clip_psnr) and math.isnan(none.clip_ssim) and math.isnan(none.clip_mse)


def test_metrics_json_writes_null_for_non_finite(tmp_path):
    from landiff_amd.metrics import metrics_from_sums, write_metrics_json
    diff = torch.zeros(2, 1, 5, dtype=torch.int64)
    diff[0, :, 0] = 4
    ssim = torch.zeros(2, 1, 2, dtype=torch.float64)
    ssim[0] = 3.0
    m = metrics_from_sums((2, 13, 12, 1), diff, ssim)
    path = str(tmp_path / "v_metrics.json")
    row = write_metrics_json(path, {"cmp": m, "list": [math.nan, 1.5, -math.inf], "n": 3})
    got = json.load(open(path))
    assert got == row and "NaN" not in open(path).read() and "Infinity" not in open(path).read()
    assert got["cmp"]["clip"]["psnr"] is None and got["cmp"]["frames"]["psnr"] == [None, None]
    assert got["cmp"]["frames"]["ssim"] == [1.0, None] and got["cmp"]["clip"]["ssim"] == 1.0
    assert got["list"] == [None, 1.5, None] and got["n"] == 3 and got["cmp"]["shape"] == [2, 13, 12, 1]
    assert got["cmp"]["channels"]["diff"][0] == [[4, 0, 0, 0, 0]]


def test_argument_checks_need_no_gpu():
    from landiff_amd import ops
    from landiff_amd.metrics import compare_clips, temporal_profile
    a = torch.zeros(2, 12, 13, 3, dtype=torch.uint8)
    for fn in (ops.clip_diff_u8, ops.clip_ssim_u8, compare_clips):
        with pytest.raises(ValueError, match="uint8"):
            fn(a.float(), a)
        with pytest.raises(ValueError, match=r"\(2, 12, 13, 3\) and \(2, 12, 14, 3\)"):
            fn(a, torch.zeros(2, 12, 14, 3, dtype=torch.uint8))
        with pytest.raises(ValueError, match=r"C 1 or 3, got \(2, 12, 13, 2\)"):
            fn(a[..., :2], a[..., :2])
        with pytest.raises(ValueError, match=r"\[F, H, W, C\].*\(2, 12, 13\)"):
            fn(a[..., 0], a[..., 0])
        with pytest.raises(ValueError, match=r"mask must be \(2, 12, 13\).*got \(2, 12, 12\)"):
            fn(a, a, torch.ones(2, 12, 12, dtype=torch.bool))
        with pytest.raises(ValueError, match="bool"):
            fn(a, a, torch.ones(2, 12, 13, dtype=torch.uint8))
        with pytest.raises(ValueError, match="one device"):
            fn(a, a.to("meta"))
    with pytest.raises(ValueError, match="at least two frames"):
        temporal_profile(a[:1])


def test_cli_flag_defaults_and_parsing():
    from landiff.infer_video import parse_args
    args = parse_args(["--prompt", "x"])
    assert args.save_frames is False and args.compare_to is None
    args = parse_args(["--prompt", "x", "--save_frames", "--compare_to", "results/video.frames.npy", "--dit_cache", "0.1"])
    assert args.save_frames is True and args.compare_to == "results/video.frames.npy" and args.dit_cache == 0.1


def test_save_helper_without_flags_is_save_video_tensor_alone(tmp_path, monkeypatch):
    """_save_video with neither flag calls save_video_tensor and writes nothing of its own; --save_frames adds the exact frames;
    a reference of another shape is refused with both shapes named before anything is compared."""
    import argparse
    import landiff.infer_video as iv
    calls = []
    monkeypatch.setattr(iv, "save_video_tensor", lambda v, p, fps=8: calls.append((p, fps)))
    frames = _rand((3, 12, 16, 3), 9)
    out = str(tmp_path / "r" / "video.mp4")
    iv._save_video(argparse.Namespace(save_frames=False, compare_to=None), frames, out, fps=8)
    assert calls == [(out, 8)] and not os.path.exists(tmp_path / "r")
    iv._save_video(argparse.Namespace(save_frames=True, compare_to=None), frames, out)
    assert sorted(os.listdir(tmp_path / "r")) == ["video.frames.npy"]
    assert np.array_equal(np.load(tmp_path / "r" / "video.frames.npy"), frames.numpy())
    # a float [C, T, H, W] video in [0, 1], as the diffusion wrapper returns: the frames saved are the ones the video file holds
    video = frames.permute(3, 0, 1, 2).float() / 255
    iv._save_video(argparse.Namespace(save_frames=True, compare_to=None), video, str(tmp_path / "f" / "v.mp4"))
    from landiff.utils import cthw_to_numpy_images
    assert np.array_equal(np.load(tmp_path / "f" / "v.frames.npy"), cthw_to_numpy_images(video))
    ref = str(tmp_path / "ref.npy")
    np.save(ref, np.zeros((3, 12, 18, 3), np.uint8))
    with pytest.raises(ValueError, match=r"\(3, 12, 18, 3\).*\(3, 12, 16, 3\)"):
        iv._save_video(argparse.Namespace(save_frames=False, compare_to=ref), frames, out)
