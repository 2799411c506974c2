"""Clip comparison on the GPU: ld_clip_diff_u8 bit for bit against int64 torch, ld_clip_ssim_u8 against the float64 restatement
(tests/metrics_ref.py) within four times what the fp32 restatement loses on the same family of cases, the exactness properties of
compare_clips, LanDiffPipeline.compare and the two CLI flags on the synthetic checkpoint tree."""
import json
import math
import os

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu

DIFF_SHAPES = [(2, 1, 1, 3), (3, 7, 13, 1), (3, 37, 53, 3), (1, 45, 139, 3), (1, 260, 260, 3), (2, 480, 720, 3)]
SSIM_SHAPES = [(1, 11, 11, 3), (2, 12, 27, 1), (3, 37, 53, 3), (1, 45, 139, 3), (1, 139, 45, 3), (2, 480, 720, 3)]
# case -> family: the bound of a case is 4 x the largest error of the fp32 restatement over its family (every shape, both masks)
CASES = {"random": "random", "noise1": "noise", "noise3": "noise", "bright": "bright", "checker": "checker",
         "const_17_200": "const", "const_254_255": "const"}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=_gen(seed))


def _mask(shape, seed, p=0.7):
    return torch.rand(shape[:3], generator=_gen(seed)) < p


def _case(name, shape, seed):
    F, H, W, C = shape
    if name == "random":
        return _rand(shape, seed), _rand(shape, seed + 1)
    if name.startswith("noise"):
        k = int(name[5:])
        a = _rand(shape, seed)
        n = torch.randint(0, 2, shape, generator=_gen(seed + 2)) * (2 * k) - k            # +-k
        return a, (a.int() + n.int()).clamp(0, 255).to(torch.uint8)
    if name == "bright":                                   # bright, low variance: where E[x^2] - mu^2 cancels
        a = (254 + torch.randint(0, 2, shape, generator=_gen(seed))).to(torch.uint8)
        b = (253 + 2 * torch.randint(0, 2, shape, generator=_gen(seed + 3))).to(torch.uint8)
        return a, b
    if name == "checker":                                  # against its inverse: negative SSIM
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        a = (((yy + xx) % 2) * 255).to(torch.uint8)[None, :, :, None].expand(shape).contiguous()
        return a, 255 - a
    u, v = (int(t) for t in name.split("_")[1:])
    return torch.full(shape, u, dtype=torch.uint8), torch.full(shape, v, dtype=torch.uint8)


def build_ssim_cases():
    """Every SSIM case once, on the host: inputs, the float64 sums and the fp32 restatement's error per (frame, channel) mean, and
    from those the family bounds (also what tools/video_metrics_bench.py tabulates)."""
    cases, fam_err = {}, {f: 0.0 for f in CASES.values()}
    for si, shape in enumerate(SSIM_SHAPES):
        mask = _mask(shape, 500 + si)
        for ci, (name, fam) in enumerate(CASES.items()):
            a, b = _case(name, shape, 1000 + 10 * si + 100 * ci)
            m64, m32 = R.ssim_map(a, b, torch.float64, 0.0), R.ssim_map(a, b, torch.float32, 128.0)
            for mk in (None, mask):
                r64, r32 = R._sums(m64, mk), R._sums(m32, mk)
                counted = r64[..., 1] > 0
                err = float((R.mean_of(r64) - R.mean_of(r32))[counted].abs().max()) if bool(counted.any()) else 0.0
                fam_err[fam] = max(fam_err[fam], err)
                cases[(shape, name, mk is not None)] = (a, b, mk, r64, err)
    return cases, fam_err


@pytest.fixture(scope="module")
def ssim_cases():
    """build_ssim_cases(), computed once, shared and left unchanged."""
    return build_ssim_cases()


# ---- integer statistics ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", DIFF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_clip_diff_exact(cuda, shape):
    from landiff_amd import ops
    if shape == (1, 260, 260, 3):       # sum d^2 = 260 * 260 * 255^2 = 4 395 690 000 per channel: past 2^32
        a, b = torch.zeros(shape, dtype=torch.uint8), torch.full(shape, 255, dtype=torch.uint8)
        assert 260 * 260 * 255 * 255 > 2 ** 32
    else:
        a, b = _rand(shape, 11), _rand(shape, 12)
    ad, bd = a.to(cuda), b.to(cuda)
    mask = _mask(shape, 13)
    empty = mask.clone()
    empty[0] = False                                       # a frame in which nothing is counted
    for name, m in (("none", None), ("random", mask), ("empty frame", empty)):
        got = ops.clip_diff_u8(ad, bd, None if m is None else m.to(cuda)).cpu()
        want = R.diff_ref(a, b, m)
        assert got.dtype == torch.int64 and torch.equal(got, want), (shape, name, got.tolist(), want.tolist())
    assert (ops.clip_diff_u8(ad, bd, empty.to(cuda))[0].cpu() == 0).all()
    same = ops.clip_diff_u8(ad, ad).cpu()
    assert torch.equal(same, R.diff_ref(a, a)) and (same[..., 1:] == 0).all() and (same[..., 0] == shape[1] * shape[2]).all()


def test_clip_diff_unaligned_views(cuda):
    """Clips that start at different 16-byte phases (a[1:] against a[:-1] of an odd-sized clip: temporal_profile's call) and a
    non-contiguous view."""
    from landiff_amd import ops
    a = _rand((4, 9, 11, 3), 21)
    ad = a.to(cuda)
    assert torch.equal(ops.clip_diff_u8(ad[1:], ad[:-1]).cpu(), R.diff_ref(a[1:], a[:-1]))
    g = _rand((2, 33, 20, 3), 22)
    gd = g.to(cuda)
    assert torch.equal(ops.clip_diff_u8(gd[:, 1:, 3:], gd[:, :-1, :-3]).cpu(), R.diff_ref(g[:, 1:, 3:], g[:, :-1, :-3]))
    ss = ops.clip_ssim_u8(gd[:, 1:, 3:], gd[:, :-1, :-3]).cpu()
    assert (R.mean_of(ss) - R.mean_of(R.ssim_ref64(g[:, 1:, 3:], g[:, :-1, :-3]))).abs().max() < 1e-5


# ---- SSIM against float64 --------------------------------------------------------------------------------------------------
def test_ssim_shapes_cross_the_tile():
    from landiff_amd import ops
    assert (1, 45, 139, 3) in SSIM_SHAPES and (1, 139, 45, 3) in SSIM_SHAPES
    th, tw = ops.SSIM_TILE_H, ops.SSIM_TILE_ELEMS // 3      # a tile's map rows and (C = 3) map columns
    assert 139 - 10 > 2 * th and 139 - 10 > 2 * tw            # the long side: several tiles, the last one partial
    assert 45 - 10 > th and 45 - 10 > tw                      # the short side crosses a tile too
    assert (139 - 10) % th and (139 - 10) % tw and (45 - 10) % th and (45 - 10) % tw


@pytest.mark.parametrize("shape", SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_clip_ssim_vs_float64(cuda, shape, ssim_cases):
    """|mean SSIM - float64| per (frame, channel) <= 4 x the largest error of the fp32 restatement (tests/metrics_ref.py: ssim_ref32,
    the kernel's order of operations in torch on the CPU) over the case's family -- every shape of SSIM_SHAPES, with and without the
    mask.  The factor covers another legitimate summation order.  The restatement's largest errors, measured on the host
    (profiles/video_metrics.txt):  random 2.5e-08, noise 1.2e-07, bright 6.0e-05, checker 9.2e-08, const 2.7e-07 -- each set by the
    11 x 11 frames, whose mean is a single map value; over the 470 x 710 map they are 1.1e-08, 4.5e-09, 6.0e-06, 9.2e-08, 2.7e-07.
    The counts are exact.  Every case's error is printed (pytest -s)."""
    from landiff_amd import ops
    cases, fam_err = ssim_cases
    bad = []
    for name, fam in CASES.items():
        for masked in (False, True):
            a, b, mk, r64, ref_err = cases[(shape, name, masked)]
            got = ops.clip_ssim_u8(a.to(cuda), b.to(cuda), None if mk is None else mk.to(cuda)).cpu()
            assert got.dtype == torch.float64 and got.shape == r64.shape
            assert torch.equal(got[..., 1], r64[..., 1]), (shape, name, masked, "counts")
            counted = r64[..., 1] > 0
            assert (got[..., 0][~counted] == 0).all()
            err = float((R.mean_of(got) - R.mean_of(r64))[counted].abs().max()) if bool(counted.any()) else 0.0
            bound = 4.0 * fam_err[fam]
            print(f"ssim {'x'.join(map(str, shape)):>12} {name:<14} mask={int(masked)}  kernel err {err:.3e}  fp32 restatement "
                  f"{ref_err:.3e}  bound (4 x family {fam}) {bound:.3e}")
            if not err <= bound:
                bad.append((name, masked, err, bound))
    assert not bad, bad


def test_constant_frames_closed_form(cuda):
    from landiff_amd import ops
    for u, v in ((0, 0), (0, 255), (255, 255), (17, 200)):
        a = torch.full((1, 20, 30, 3), u, dtype=torch.uint8, device=cuda)
        b = torch.full((1, 20, 30, 3), v, dtype=torch.uint8, device=cuda)
        got = R.mean_of(ops.clip_ssim_u8(a, b).cpu())
        assert (got - (2.0 * u * v + R.C1) / (u * u + v * v + R.C1)).abs().max() < 1e-4, (u, v, got)


# ---- exactness properties --------------------------------------------------------------------------------------------------
def _fields(m):
    import dataclasses
    return dataclasses.asdict(m)


def _same(x, y):
    """Two ClipMetrics agree bit for bit (nan equal to nan)."""
    fx, fy = _fields(x), _fields(y)
    for k in fx:
        p, q = fx[k], fy[k]
        if isinstance(p, torch.Tensor):
            ok = p.dtype == q.dtype and p.shape == q.shape and torch.equal(torch.nan_to_num(p.double(), nan=-7.0), torch.nan_to_num(q.double(), nan=-7.0))
        elif isinstance(p, float):
            ok = p == q or (math.isnan(p) and math.isnan(q))
        else:
            ok = p == q
        assert ok, (k, p, q)


def test_compare_clips_exactness(cuda):
    from landiff_amd.metrics import compare_clips
    shape = (3, 45, 70, 3)
    a, b = _rand(shape, 31).to(cuda), _rand(shape, 32).to(cuda)
    # a clip against itself
    m = compare_clips(a, a)
    assert torch.equal(m.ssim, torch.ones(3, dtype=torch.float64)) and m.clip_ssim == 1.0
    assert torch.equal(m.ssim_sums[..., 0], m.ssim_sums[..., 1])
    assert (m.psnr == math.inf).all() and m.clip_psnr == math.inf and int(m.differing.sum()) == 0 and m.clip_differing == 0
    assert compare_clips(a, a.clone()).clip_ssim == 1.0
    # symmetric, repeatable
    ab = compare_clips(a, b)
    _same(ab, compare_clips(b, a))
    _same(ab, compare_clips(a, b))
    assert 0 < ab.clip_psnr < 12 and abs(ab.clip_ssim) < 0.1 and ab.clip_counted == 3 * 45 * 70 * 3
    # a frame's figures do not depend on the call's other frames
    for k in range(3):
        one = compare_clips(a[k:k + 1], b[k:k + 1])
        assert torch.equal(one.diff[0], ab.diff[k]) and torch.equal(one.ssim_sums[0], ab.ssim_sums[k])
        assert one.psnr[0] == ab.psnr[k] and one.ssim[0] == ab.ssim[k]
    # an all-true mask is no mask
    _same(ab, compare_clips(a, b, torch.ones(shape[:3], dtype=torch.bool, device=cuda)))


def test_masked_out_pixels_do_not_count(cuda):
    """Garbage written over the masked-out pixels leaves the integer statistics alone, and the SSIM of every frame in which no kept
    centre's window reaches it: here frame 0 (everything kept: no garbage) and frame 3 (nothing kept: nothing counted).  In frames
    1 and 2 windows of kept centres do reach masked-out pixels; their SSIM may move, their counts may not."""
    from landiff_amd.metrics import compare_clips
    shape = (4, 40, 50, 3)
    a, b = _rand(shape, 41), _rand(shape, 42)
    mask = torch.ones(shape[:3], dtype=torch.bool)
    mask[1, 25:, 30:] = False
    mask[2] = _mask(shape, 43)[2]
    mask[3] = False
    garbage = _rand(shape, 44)
    a2 = torch.where(mask[..., None], a, garbage)
    b2 = torch.where(mask[..., None], b, 255 - garbage)
    assert not torch.equal(a2[1], a[1]) and torch.equal(a2[0], a[0])
    m1 = compare_clips(a.to(cuda), b.to(cuda), mask.to(cuda))
    m2 = compare_clips(a2.to(cuda), b2.to(cuda), mask.to(cuda))
    assert torch.equal(m1.diff, m2.diff) and torch.equal(m1.diff, R.diff_ref(a, b, mask))
    assert torch.equal(m1.ssim_sums[..., 1], m2.ssim_sums[..., 1])
    assert torch.equal(m1.ssim_sums[0], m2.ssim_sums[0]) and m1.ssim[0] == m2.ssim[0]
    assert math.isnan(m1.ssim[3]) and math.isnan(m2.ssim[3]) and math.isnan(m1.psnr[3]) and m1.counted[3] == 0
    assert (m1.ssim_sums[3] == 0).all() and not math.isnan(m1.clip_ssim)


def test_small_frames_have_no_ssim(cuda):
    from landiff_amd import ops
    from landiff_amd._lib import LandiffHipError
    from landiff_amd.metrics import compare_clips
    a, b = _rand((2, 10, 40, 3), 51), _rand((2, 10, 40, 3), 52)
    with pytest.raises(LandiffHipError, match=r"11-tap window needs H, W >= 11, got 10 x 40"):
        ops.clip_ssim_u8(a.to(cuda), b.to(cuda))
    m = compare_clips(a.to(cuda), b.to(cuda))
    assert m.ssim is None and m.clip_ssim is None and m.ssim_sums is None
    want = R.diff_ref(a, b)
    assert torch.equal(m.diff, want)
    ssd, n = want[..., 1].sum(1).double(), want[..., 0].sum(1).double()
    assert torch.equal(m.psnr, 10.0 * torch.log10(255.0 * 255.0 * n / ssd)) and m.as_dict()["frames"]["ssim"] is None


def test_temporal_profile(cuda):
    from landiff_amd.metrics import compare_clips, temporal_profile
    a = _rand((4, 21, 25, 3), 61)
    a[2] = a[1]
    t = temporal_profile(a.to(cuda))
    assert t.shape == (3, 21, 25, 3) and t.psnr[1] == math.inf and t.ssim[1] == 1.0 and t.differing[1] == 0
    _same(t, compare_clips(a[1:].to(cuda), a[:-1].to(cuda)))
    assert torch.equal(t.diff, R.diff_ref(a[1:], a[:-1]))


# ---- pipeline ----------------------------------------------------------------------------------------------------------------
def test_pipeline_compare(cuda):
    from landiff_amd.config import PipelineConfig
    from landiff_amd.pipeline import LanDiffPipeline, synthetic_inputs
    from landiff_amd.weights import init_pipeline_state
    cfg = PipelineConfig.tiny(num_steps=6).check()
    st = init_pipeline_state(cfg, seed=1234)
    inp = synthetic_inputs(cfg, cuda, n_text=6, seed=42)
    pipe = LanDiffPipeline(cfg, st, cuda)
    assert pipe.last_metrics is None and "metrics" not in pipe.timings
    x = pipe(inp).clone()
    m = pipe.compare(x, x.cpu())                           # any device
    assert m is pipe.last_metrics and pipe.timings["metrics"] > 0
    assert m.clip_psnr == math.inf and m.clip_ssim == 1.0 and m.clip_differing == 0 and m.shape == tuple(x.shape)
    cached = LanDiffPipeline(cfg, st, cuda, dit_cache=0.5)
    y = cached(inp)
    assert y.shape == x.shape
    t0 = pipe.timings["metrics"]
    m = pipe.compare(y, x)
    assert (math.isfinite(m.clip_psnr) and m.clip_psnr > 0) or m.clip_psnr == math.inf
    assert -1.0 <= m.clip_ssim <= 1.0 and pipe.timings["metrics"] > t0
    assert torch.equal(m.diff, R.diff_ref(y.cpu(), x.cpu()))
    with pytest.raises(ValueError, match="one shape"):
        pipe.compare(x, x[:-1])


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_infer_video_save_frames_and_compare_to(cuda, tmp_path, monkeypatch):
    """`landiff.infer_video` on the synthetic checkpoint tree: without the flags the helper adds no file; --save_frames writes the
    returned frames; --compare_to that file gives a perfect comparison for the same run and compare_clips' figures for another
    seed; a reference of another shape is refused."""
    import warnings
    import landiff.infer_video as iv
    from facade_helpers import build_config0_workdir
    from landiff.utils import cthw_to_numpy_images
    from landiff_amd.metrics import _jsonable, compare_clips, temporal_profile
    work = str(tmp_path)
    cfg, _ = build_config0_workdir(work)
    monkeypatch.chdir(work)
    monkeypatch.delenv("LANDIFF_HOME", raising=False)
    monkeypatch.setattr(iv, "build_llm", lambda: cfg.llm)
    captured = {}
    monkeypatch.setattr(iv, "save_video_tensor", lambda v, p, fps=8: captured.update(video=v, path=p))    # (no video file: only the helper's own files)
    base = ["--prompt", "a dog walking in the rain", "--seed", "7"]

    def run(extra, name, seed=None):
        args = iv.parse_args(base + ["--save_file_name", f"{name}/video"] + extra)
        if seed is not None:
            args.seed = seed
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            iv.infer_diffusion(args, tokens)
        return torch.from_numpy(cthw_to_numpy_images(captured["video"]))

    args = iv.parse_args(base + ["--save_file_name", "tok/video"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tokens = iv.llm_infer(args)
    plain = run([], "plain")
    assert not os.path.exists("plain")                     # nothing but the (captured) video
    first = run(["--save_frames"], "first")
    assert sorted(os.listdir("first")) == ["video.frames.npy"] and captured["path"] == "first/video.mp4"
    saved = np.load("first/video.frames.npy")
    assert saved.dtype == np.uint8 and np.array_equal(saved, first.numpy()) and torch.equal(first, plain)
    again = run(["--compare_to", "first/video.frames.npy"], "again")
    assert sorted(os.listdir("again")) == ["video_metrics.json"] and torch.equal(again, first)
    got = json.load(open("again/video_metrics.json"))
    assert got["clip"]["psnr"] is None and got["clip"]["ssim"] == 1.0 and got["clip"]["differing"] == 0
    assert got["frames"]["psnr"] == [None] * first.shape[0] and got["shape"] == list(first.shape)
    assert got["reference"] == "first/video.frames.npy" and got["temporal"]["video"] == got["temporal"]["reference"]
    other = run(["--compare_to", "first/video.frames.npy", "--save_frames"], "other", seed=8)
    assert sorted(os.listdir("other")) == ["video.frames.npy", "video_metrics.json"] and not torch.equal(other, first)
    got = json.load(open("other/video_metrics.json"))
    want = compare_clips(other.to(cuda), first.to(cuda))
    assert math.isfinite(want.clip_psnr) and math.isfinite(want.clip_ssim) and want.clip_differing > 0
    assert {k: got[k] for k in ("shape", "clip", "frames", "channels")} == _jsonable(want)
    assert got["clip"]["psnr"] == want.clip_psnr and got["clip"]["ssim"] == want.clip_ssim
    assert got["temporal"]["video"] == _jsonable(temporal_profile(other.to(cuda)))
    assert got["temporal"]["reference"] == _jsonable(temporal_profile(first.to(cuda)))
    np.save("wrong.npy", first.numpy()[:, :, :-8])
    n, H, W, _ = first.shape
    with pytest.raises(ValueError, match=rf"\({n}, {H}, {W - 8}, 3\).*\({n}, {H}, {W}, 3\)"):
        iv._save_video(iv.parse_args(base + ["--compare_to", "wrong.npy"]), captured["video"], "bad/video.mp4")
