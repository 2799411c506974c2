"""Host-side checks of clip editing (no GPU): the schedule's (alpha, sigma) table, the strength -> start step rule, the command
line's refusals and defaults, the JSON writer, the wrappers' refusals before any launch, and the CPU restatements themselves."""
import json
import math

import pytest
import torch

from landiff_amd.config import SamplerConfig


@pytest.mark.parametrize("kind,n", [("vpsde_dpmpp2m", 50), ("vpsde_dpmpp2m", 6), ("ddim", 5)])
def test_step_alphas_reproduce_the_plan(kind, n):
    """alpha[0] == 0, sigma[0] == 1, alpha strictly increasing up to 1; a_t / b_t of every StepPlan recomputed from the table with
    build_plan's fp32 expressions are the same floats."""
    from landiff_amd.schedule import build_plan, step_alphas
    cfg = SamplerConfig(num_steps=n, sampler=kind)
    al = step_alphas(cfg)
    assert len(al) == n + 1 and all(isinstance(v, float) for pair in al for v in pair)
    assert al[0] == (0.0, 1.0) and al[n] == (1.0, 0.0)
    assert all(al[i][0] < al[i + 1][0] for i in range(n))
    f32 = lambda v: torch.ones(1) * torch.tensor(v, dtype=torch.float32)
    for sp in build_plan(cfg):
        cur, nxt = f32(al[sp.index][0]), f32(al[sp.index + 1][0])
        assert float(cur) == al[sp.index][0]                                   # fp32-exact values
        a_t = ((1 - nxt ** 2) / (1 - cur ** 2)) ** 0.5
        assert (float(a_t), float(nxt - cur * a_t)) == (sp.a_t, sp.b_t), sp.index
        assert al[sp.index][1] == float((1 - cur ** 2) ** 0.5)


def test_edit_start_step():
    from landiff_amd.pipeline import edit_start_step
    assert [edit_start_step(50, s) for s in (1.0, 0.6, 0.58, 0.01)] == [0, 20, 21, 49]
    assert edit_start_step(3, 0.5) == 1 and edit_start_step(2, 0.5) == 1 and edit_start_step(6, 0.5) == 3
    with pytest.raises(ValueError, match="0.01"):                              # names the smallest strength that runs a step
        edit_start_step(50, 0.005)
    for bad in (0.0, -0.1, 1.01, math.nan):
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            edit_start_step(50, bad)


def test_edit_clip_shape():
    from landiff_amd.config import PipelineConfig
    from landiff_amd.pipeline import edit_clip
    cfg = PipelineConfig.tiny()
    d = cfg.dit
    ok = torch.zeros(4 * d.latent_frames - 3, 8 * d.latent_h, 8 * d.latent_w, 3, dtype=torch.uint8)
    assert edit_clip(ok, cfg) is ok
    for bad in (torch.zeros(ok.shape[0] + 1, *ok.shape[1:], dtype=torch.uint8), ok[:, :-8], ok.float(), ok[..., 0]):
        with pytest.raises(ValueError, match=rf"\[{ok.shape[0]}, {ok.shape[1]}, {ok.shape[2]}, 3\]"):
            edit_clip(bad, cfg)


def test_parse_args_edit_flags(capsys):
    import landiff.infer_video as iv
    base = ["--prompt", "p", "--edit_video", "c.npy"]
    a = iv.parse_args(base)
    assert a.edit_tokens == "prompt" and a.edit_strength == 0.6 and a.edit_mask is None and not a.edit_clean_known
    assert iv.parse_args(base + ["--theia_ckpt", "/x/theia"]).edit_tokens == "from_frames"
    assert iv.parse_args(base + ["--theia_ckpt", "/x/theia", "--edit_tokens", "prompt"]).edit_tokens == "prompt"
    assert iv.parse_args(base + ["--edit_tokens", "tok.npy", "--edit_clean_known", "--edit_strength", "1"]).edit_tokens == "tok.npy"
    assert iv.parse_args(["--prompt", "p"]).edit_video is None
    for extra, msg in ((["--extend_video", "d.npy"], "--extend_video"),
                       (["--num_samples", "2"], "--num_samples"),
                       (["--num_samples", "2", "--keep", "1"], "--keep"),
                       (["--first_frame", "i.npy"], "--first_frame"),
                       (["--edit_strength", "0"], "--edit_strength"),
                       (["--edit_strength", "1.5"], "--edit_strength")):
        with pytest.raises(SystemExit):
            iv.parse_args(base + extra)
        err = capsys.readouterr().err
        assert "--edit_video" in err and msg in err, err


def test_write_edit_json(tmp_path):
    from landiff_amd.pipeline import write_edit_json
    e = dict(strength=0.5, start_step=25, steps_run=25, alpha_start=math.nan, sigma_start=math.inf, kept_cells=3, total_cells=10,
             tokens_source="prompt")
    path = str(tmp_path / "v_edit.json")
    row = write_edit_json(path, e)
    got = json.load(open(path))
    assert got == row and got["alpha_start"] is None and got["sigma_start"] is None
    assert {k: v for k, v in got.items() if v is not None} == {k: v for k, v in e.items() if k not in ("alpha_start", "sigma_start")}
    assert "NaN" not in open(path).read() and "Infinity" not in open(path).read()


def test_wrappers_refuse_before_any_launch():
    """Shapes and dtypes are checked on the host; CPU tensors never reach the library (there is no CPU fallback)."""
    from landiff_amd import _lib, ops
    x = torch.zeros(1, 3, 4, 8, 12)
    with pytest.raises(TypeError, match="float32"):
        ops.latent_pin(x, x.double())
    with pytest.raises(ValueError, match="shape"):
        ops.latent_pin(x, x[:, :2])
    with pytest.raises(ValueError, match=r"\[3, 8, 12\]"):
        ops.latent_pin(x, x.clone(), mask=torch.zeros(3, 8, 11, dtype=torch.uint8))
    with pytest.raises(TypeError, match="uint8 or bool"):
        ops.latent_pin(x, x.clone(), mask=torch.zeros(3, 8, 12))
    with pytest.raises(_lib.LandiffHipError, match="GPU"):
        ops.latent_pin(x, x.clone())
    with pytest.raises(TypeError, match="uint8 or bool"):
        ops.mask_to_latent(torch.zeros(9, 16, 24))
    # the library's own refusals (null stream, fake aligned pointers: nothing is launched)
    import ctypes
    lib, p = _lib.load(), ctypes.c_void_p(64)
    for F, Hp, Wp, msg in ((8, 16, 24, b"4k + 1"), (9, 12, 24, b"multiples of 8"), (9, 16, 20, b"multiples of 8")):
        assert lib.ld_mask_to_latent(p, p, F, Hp, Wp, None) < 0 and msg in lib.ld_last_error()
    assert lib.ld_mask_to_latent(ctypes.c_void_p(68), p, 9, 16, 24, None) < 0 and b"aligned" in lib.ld_last_error()
    assert lib.ld_latent_pin(p, p, None, None, 1.0, 0.0, 3, 4, 8, 12, None) < 0 and b"alias" in lib.ld_last_error()
    assert lib.ld_latent_pin(p, None, None, None, 1.0, 0.0, 3, 4, 8, 12, None) < 0 and b"null" in lib.ld_last_error()


def test_sampler_refusals_need_no_gpu():
    from landiff_amd.sampler import DiffusionSampler
    s = DiffusionSampler(SamplerConfig(num_steps=4))
    x = torch.zeros(1, 3, 4, 8, 12)
    m = torch.ones(3, 8, 12, dtype=torch.bool)
    step = lambda *a: None
    for kw in (dict(start=1, prefix=x[:, :1]), dict(known=x, fixed_frames=1), dict(known=x, known_mask=m, prefix=x[:, :1], fixed_frames=1)):
        with pytest.raises(ValueError, match="prefix / fixed_frames"):
            s.run(step, x, **kw)
    with pytest.raises(ValueError, match="known is missing"):
        s.run(step, x, known_mask=m)
    for bad in (-1, 4, 1.0):
        with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
            s.run(step, x, start=bad)
    with pytest.raises(ValueError, match="known must be float32"):
        s.run(step, x, known=x[:, :2])
    with pytest.raises(TypeError):
        s.run(step, x, None, None, None, 0, 1)                                 # the new arguments are keyword-only


def test_restatements():
    """mask_to_latent_ref on hand-made cases; edit_run_ref with nothing to edit is the oracle's own loop, draw for draw."""
    from edit_ref import edit_run_ref, mask_to_latent_ref
    from oracle.sampler import DiffusionSamplerOracle
    m = torch.ones(9, 16, 24, dtype=torch.bool)
    assert mask_to_latent_ref(m).shape == (3, 2, 3) and mask_to_latent_ref(m).all()
    for f, t in ((0, 0), (1, 1), (4, 1), (5, 2), (8, 2)):
        h = m.clone()
        h[f, 15, 16] = False
        want = torch.ones(3, 2, 3, dtype=torch.uint8)
        want[t, 1, 2] = 0
        assert torch.equal(mask_to_latent_ref(h), want), f
    for kind, n in (("vpsde_dpmpp2m", 6), ("ddim", 5)):
        sc = SamplerConfig(num_steps=n, sampler=kind)
        g = torch.Generator().manual_seed(5)
        x0 = torch.randn(1, 3, 4, 8, 12, generator=g)
        noises = [torch.randn(1, 3, 4, 8, 12, generator=g) for _ in range(2 * n)]
        ia, ib = iter(noises), iter(noises)
        net = lambda xx, idx, c: 0.5 * xx
        ref = DiffusionSamplerOracle(sc).run(net, x0.clone(), torch.zeros(1, 2, 4), torch.zeros(1, 2, 4), randn_like=lambda t: next(ia))
        got = edit_run_ref(sc, net, x0, lambda t: next(ib), known=x0 * 0.25)
        assert torch.equal(got, ref) and len(list(ia)) == len(list(ib))
