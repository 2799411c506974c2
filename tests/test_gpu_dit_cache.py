"""DiT step cache on the GPU: the two kernel families of ld_dit_cache.hip against torch, the cached ControlDiTRunner against the
uncached one (a computed step is the uncached step bit for bit; a skipped step is embed + bf16(h0 + residual) + final layer,
bit for bit), one run at the BASELINE shape, and the pipeline switch.  Tiny DiT, 6 sampler steps, unless said otherwise."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
# tails only, exactly one 16-byte vector, workgroup edges, the tiny DiT's M * d, many workgroups plus a tail
SIZES = [1, 7, 8, 255, 256, 257, 164 * 128, 2 ** 20 + 3]
C, S = True, False


def _pair(cuda, n, seed, offset=0):
    """Two bf16 vectors of n elements that differ by about 10 %; offset = 1: views that start 2 bytes past a 16-byte boundary."""
    g = torch.Generator(device=cuda).manual_seed(seed)
    a = torch.randn(n + offset, device=cuda, generator=g).to(BF)
    b = (a.float() + 0.1 * torch.randn(n + offset, device=cuda, generator=g)).to(BF)
    return a[offset:], b[offset:]


def _close(got, want, what):
    """|got - want| <= 1e-5 |want|: non-negative terms, an fp32 sum tree no deeper than ~40 additions is accurate to 40 * 2^-24 =
    2.4e-6 relative (plus 2^-24 per term for the fp32 difference)."""
    print(f"{what}: got {got!r} want {want!r} rel {abs(got - want) / want if want else 0.0:.3e}")
    assert abs(got - want) <= 1e-5 * abs(want), (what, got, want)


# ---- kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_absdiff_sums(cuda, n, offset):
    from landiff_amd import ops
    cur, prev = _pair(cuda, n, n, offset)
    assert cur.data_ptr() % 16 == 2 * offset             # offset 1: the unaligned path, every element through the scalar loop
    want = ((cur.double() - prev.double()).abs().sum().item(), prev.double().abs().sum().item())
    out = ops.absdiff_sums(cur, prev)
    assert out.dtype == torch.float32 and out.shape == (2,)
    _close(out[0].item(), want[0], f"n={n} sum|cur-prev|")
    _close(out[1].item(), want[1], f"n={n} sum|prev|")
    assert torch.equal(ops.absdiff_sums(cur, prev), out)                     # run to run: the same bits
    # update_prev: the sums are those against the OLD prev, and prev is cur afterwards (nothing beyond n is touched)
    old = prev.clone()
    out2 = ops.absdiff_sums(cur, prev, update_prev=True)
    assert torch.equal(out2, out) and torch.equal(prev, cur) and not (n > 8 and torch.equal(prev, old))
    # an all-zero prev: a zero denominator, exactly
    z = torch.zeros_like(cur)
    out3 = ops.absdiff_sums(cur, z)
    assert out3[1].item() == 0.0
    _close(out3[0].item(), cur.double().abs().sum().item(), f"n={n} sum|cur|")


def test_absdiff_sums_leaves_neighbours_alone(cuda):
    """prev <- cur writes exactly n elements: the guard elements on both sides of a view keep their values."""
    from landiff_amd import ops
    for n in (1, 7, 8, 257, 164 * 128):
        cur, _ = _pair(cuda, n, 5)
        buf = torch.full((n + 16,), 3.0, device=cuda, dtype=BF)
        ops.absdiff_sums(cur, buf[8:8 + n], update_prev=True)
        assert torch.equal(buf[8:8 + n], cur) and bool((buf[:8] == 3.0).all()) and bool((buf[8 + n:] == 3.0).all())


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_residual_sub_and_add(cuda, n, offset):
    from landiff_amd import ops
    a, b = _pair(cuda, n, 100 + n, offset)
    sub = (a.float() - b.float()).to(BF)                 # one fp32 operation, one rounding
    add = (a.float() + b.float()).to(BF)
    got = ops.residual_sub(a, b)
    assert got.dtype == BF and torch.equal(got, sub)
    assert torch.equal(ops.residual_add(a, b), add)
    a2 = a.clone()
    assert ops.residual_add(a2, b, out=a2) is a2 and torch.equal(a2, add)            # in place
    # round trip of the cache: a skipped step's h0 + (h - h0)
    assert torch.equal(ops.residual_add(b, got), (b.float() + sub.float()).to(BF))
    # the output-side sums, against an older residual -- which may be the buffer the new one overwrites
    old = (sub.float() * 1.05 + 0.01).to(BF)
    want = ((sub.double() - old.double()).abs().sum().item(), old.double().abs().sum().item())
    out, sums = ops.residual_sub(a, b, out=torch.empty_like(a), old=old)
    assert torch.equal(out, sub)
    _close(sums[0].item(), want[0], f"n={n} sum|out-old|")
    _close(sums[1].item(), want[1], f"n={n} sum|old|")
    buf = old.clone()
    out_b, sums_b = ops.residual_sub(a, b, out=buf, old=buf)
    assert out_b is buf and torch.equal(buf, sub) and torch.equal(sums_b, sums)


# ---- runner ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(cuda):
    """Tiny DiT, the 6 sampler steps' scalars, a slowly moving input per step, and the uncached runner's outputs (computed once)."""
    from landiff_amd.config import PipelineConfig
    from landiff_amd.dit import ControlDiTRunner
    from landiff_amd.schedule import build_plan
    from landiff_amd.weights import init_pipeline_state
    cfg = PipelineConfig.tiny(num_steps=6).check()
    st = init_pipeline_state(cfg, seed=1234)
    d = cfg.dit
    assert d.seq_len * 2 * d.hidden == 164 * 128
    plan = build_plan(cfg.sampler)
    g = torch.Generator().manual_seed(21)
    shape = (1, d.latent_frames, d.in_channels, d.latent_h, d.latent_w)
    x0, dx = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    xs = [(x0 + 0.03 * s * dx).to(cuda) for s in range(6)]
    ctx = torch.randn(1, d.text_len, d.text_dim, generator=g)
    sem = (0.5 * torch.randn(d.latent_frames, d.in_channels, d.latent_h, d.latent_w, generator=g)).to(BF)
    t = dict(cfg=cfg, st=st, d=d, plan=plan, xs=xs, ctx=ctx, sem=sem, ts=[sp.timestep for sp in plan])
    t["ref"] = {}
    for fp8 in (False, "mx"):
        t["ref"][fp8] = _run(_runner(t, cuda, None, fp8_gemm=fp8), t)
    return t


def _runner(t, cuda, cache, **kw):
    from landiff_amd.dit import ControlDiTRunner
    run = ControlDiTRunner(t["st"]["dit_main"], t["st"]["dit_control"], t["d"], cuda, step_cache=cache,
                           plan_timesteps=t["ts"] if cache is not None else None, **kw)
    run.set_condition(t["ctx"], t["sem"])
    return run


def _step(run, t, s):
    sp = t["plan"][s]
    out = torch.empty_like(t["xs"][s])
    run.step(t["xs"][s], sp.timestep, sp.c_out, sp.c_skip, sp.cfg_scale, out)
    return out


def _run(run, t):
    return [_step(run, t, s).clone() for s in range(6)]


def _cfg(threshold=0.0, **kw):
    from landiff_amd.dit_cache import StepCacheConfig
    return StepCacheConfig(threshold, **kw)


@pytest.mark.parametrize("overlap,fp8", [("0", False), ("1", False), ("1", "mx")])
def test_all_compute_plan_is_the_uncached_runner(cuda, tiny, monkeypatch, overlap, fp8):
    monkeypatch.setenv("LD_DIT_OVERLAP", overlap)
    run = _runner(tiny, cuda, _cfg(math.inf, plan=(C,) * 6), fp8_gemm=fp8)
    assert run.overlap == (overlap == "1") and run.sc_residual.shape == (run.M, tiny["d"].hidden)
    for s in range(6):
        assert torch.equal(_step(run, tiny, s), tiny["ref"][fp8][s]), s
    rep = run.cache_report
    assert [r["computed"] for r in rep] == [True] * 6 and [r["index"] for r in rep] == list(range(6))
    assert [r["timestep"] for r in rep] == tiny["ts"]
    assert rep[0]["input_rel_l1"] is None and rep[0]["output_rel_l1"] is None
    assert all(r["input_rel_l1"] > 0 and r["output_rel_l1"] > 0 and math.isfinite(r["output_rel_l1"]) for r in rep[1:])


def test_uncached_runner_allocates_and_launches_nothing_new(cuda, tiny):
    run = _runner(tiny, cuda, None)
    assert run._sc is None and not hasattr(run, "sc_residual") and run.cache_report == []
    run.reset_step_cache()                                # a no-op
    from landiff_amd.dit import ControlDiTRunner
    with pytest.raises(ValueError, match="plan_timesteps"):
        ControlDiTRunner(tiny["st"]["dit_main"], tiny["st"]["dit_control"], tiny["d"], cuda, step_cache=_cfg(0.1))


@pytest.mark.parametrize("overlap", ["0", "1"])
def test_plan_c_s_c_s_s_c(cuda, tiny, monkeypatch, overlap):
    """Computed steps: the uncached step, and the residual kept is bf16(stack output - embedded stream).  Skipped steps: embed,
    bf16(h0 + residual), final layer -- formed here from a fresh uncached runner's pieces -- and not one attention launch."""
    monkeypatch.setenv("LD_DIT_OVERLAP", overlap)
    d = tiny["d"]
    plan = (C, S, C, S, S, C)
    run = _runner(tiny, cuda, _cfg(0.0, plan=plan), attn_exact=False)
    ref = _runner(tiny, cuda, None, attn_exact=False)
    run.attn_events = []
    for s in range(6):
        sp, x = tiny["plan"][s], tiny["xs"][s]
        before = len(run.attn_events)
        got = _step(run, tiny, s)
        ref._use(0)
        ref._time_emb(ref.main, sp.timestep)
        ref._embed(ref.main, x, ref.h, ref.txt_main, None)
        h0 = ref.h.clone()
        assert torch.equal(run.sc_h0, h0), s
        if plan[s]:
            assert len(run.attn_events) - before == d.layers_control + d.layers_main
            want = _step(ref, tiny, s)                    # (leaves the stack's output in ref.h)
            assert torch.equal(run.sc_residual, (ref.h.float() - h0.float()).to(BF)), s
        else:
            assert len(run.attn_events) == before
            h = (h0.float() + run.sc_residual.float()).to(BF)
            want = torch.empty_like(x)
            ref._final(h, x, sp.c_out, sp.c_skip, sp.cfg_scale, want)
            assert not torch.equal(want, tiny["ref"][False][s])          # the skipped step is not the computed one
        assert torch.equal(got, want), s
        assert torch.isfinite(got).all()
    rep = run.cache_report
    assert [r["computed"] for r in rep] == list(plan)
    assert [r["output_rel_l1"] is not None for r in rep] == [False, False, True, False, False, True]


def test_thresholds_inf_and_zero(cuda, tiny):
    run = _runner(tiny, cuda, _cfg(math.inf))
    outs = _run(run, tiny)
    assert [r["computed"] for r in run.cache_report] == [True, False, False, False, False, True]
    assert torch.equal(outs[0], tiny["ref"][False][0]) and all(torch.isfinite(o).all() for o in outs)
    acc = [r["accumulated"] for r in run.cache_report]
    assert acc[0] == 0.0 and acc[1] < acc[2] < acc[3] < acc[4] and acc[5] == 0.0
    run0 = _runner(tiny, cuda, _cfg(0.0))
    for s, o in enumerate(_run(run0, tiny)):
        assert torch.equal(o, tiny["ref"][False][s]), s
    assert all(r["computed"] for r in run0.cache_report)


def test_a_run_depends_on_its_inputs_alone(cuda, tiny):
    """The same six steps twice in one runner: equal outputs and equal reports, with set_condition() in between and without it
    (a timestep that does not decrease empties the cache), whatever ran before."""
    run = _runner(tiny, cuda, _cfg(math.inf, max_consecutive_skips=2))
    first = _run(run, tiny)
    rep1 = [dict(r) for r in run.cache_report]
    assert [r["computed"] for r in rep1] == [True, False, False, True, False, True]
    run.set_condition(tiny["ctx"], tiny["sem"])
    assert run.cache_report == []
    second = _run(run, tiny)
    rep2 = [dict(r) for r in run.cache_report]
    third = _run(run, tiny)                               # no set_condition: step 0's timestep is larger than step 5's
    rep3 = [dict(r) for r in run.cache_report]
    _step(run, tiny, 0); _step(run, tiny, 1)              # a run broken off after two steps ...
    fourth = _run(run, tiny)                              # ... leaves nothing behind either
    rep4 = [dict(r) for r in run.cache_report]
    for outs, rep in ((second, rep2), (third, rep3), (fourth, rep4)):
        assert rep == rep1
        for a, b in zip(first, outs):
            assert torch.equal(a, b)
    run.reset_step_cache()
    assert run.cache_report == [] and not run._sc_have_residual


def test_report_matches_the_buffers(cuda, tiny):
    """input_rel_l1 of step s = sum|mod_s - mod_(s-1)| / sum|mod_(s-1)| over the runner's own buffers (the previous input is kept on
    every step, computed or skipped); output_rel_l1 likewise over the residual."""
    run = _runner(tiny, cuda, _cfg(0.0, plan=(C, S, C, C, S, C)))
    prev_mod = prev_res = None
    for s in range(6):
        _step(run, tiny, s)
        r = run.cache_report[s]
        mod, res = run.sc_prev_mod.double(), run.sc_residual.double()
        if prev_mod is None:
            assert r["input_rel_l1"] is None
        else:
            want = ((mod - prev_mod).abs().sum() / prev_mod.abs().sum()).item()
            assert abs(r["input_rel_l1"] - want) <= 1e-5 * want, (s, r, want)
        if r["computed"] and prev_res is not None:
            want = ((res - prev_res).abs().sum() / prev_res.abs().sum()).item()
            assert abs(r["output_rel_l1"] - want) <= 1e-5 * want, (s, r, want)
        else:
            assert r["output_rel_l1"] is None
        if not r["computed"]:
            assert torch.equal(res, prev_res)
        prev_mod, prev_res = mod.clone(), res.clone()


# ---- BASELINE shape -------------------------------------------------------------------------------------------------------
def test_full_shape_c_s_c(cuda):
    """1 control + 1 main layer at the BASELINE shape (2 x 17 776 rows x 1920 = 68 M elements per buffer: the grid-stride path and
    64-bit element offsets): plan C S C against the uncached runner and the torch emulation of the skipped step."""
    from landiff_amd.dit import ControlDiTRunner
    from oracle_jobs import dit_layer_inputs
    d1, sd_main, sd_ctrl, _, _ = dit_layer_inputs()
    g = torch.Generator().manual_seed(8)
    shape = (1, d1.latent_frames, d1.in_channels, d1.latent_h, d1.latent_w)
    x0, dx = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    xs = [(x0 + 0.05 * s * dx).to(cuda) for s in range(3)]
    ctx = torch.randn(1, d1.text_len, d1.text_dim, generator=g)
    sem = (0.5 * torch.randn(d1.latent_frames, d1.in_channels, d1.latent_h, d1.latent_w, generator=g)).to(BF)
    ts, scal = [900, 600, 300], (-0.8, 0.6, 4.0)
    run = ControlDiTRunner(sd_main, sd_ctrl, d1, cuda, attn_exact=False, step_cache=_cfg(0.0, plan=(C, S, C)), plan_timesteps=ts)
    ref = ControlDiTRunner(sd_main, sd_ctrl, d1, cuda, attn_exact=False)
    assert run.sc_h0.numel() == 2 * 17776 * 1920
    run.set_condition(ctx, sem); ref.set_condition(ctx, sem)
    for s in range(3):
        got, want = torch.empty_like(xs[s]), torch.empty_like(xs[s])
        run.step(xs[s], ts[s], *scal, got)
        if s != 1:
            ref.step(xs[s], ts[s], *scal, want)
            ref._use(0)
            ref._time_emb(ref.main, ts[s])                # (ref.h holds the stack's output; the embedded stream goes to ref.hc)
            ref._embed(ref.main, xs[s], ref.hc, ref.txt_main, None)
            assert torch.equal(run.sc_residual, (ref.h.float() - ref.hc.float()).to(BF)), s
        else:
            ref._use(0)
            ref._time_emb(ref.main, ts[s])
            ref._embed(ref.main, xs[s], ref.h, ref.txt_main, None)
            assert torch.equal(run.sc_h0, ref.h)
            h = (ref.h.float() + run.sc_residual.float()).to(BF)
            ref._final(h, xs[s], *scal, want)
            del h
        assert torch.equal(got, want), s
        assert torch.isfinite(got).all()
    rep = run.cache_report
    assert [r["computed"] for r in rep] == [True, False, True]
    assert 0 < rep[1]["input_rel_l1"] < 1 and 0 < rep[2]["output_rel_l1"] < 10


# ---- pipeline --------------------------------------------------------------------------------------------------------------
def test_pipeline_switch(cuda, tiny):
    from landiff_amd.pipeline import LanDiffPipeline, synthetic_inputs
    cfg = tiny["cfg"]
    st = {k: v for k, v in tiny["st"].items() if k != "llm"}          # (the AR decode is not part of this: tokens are given)
    d = cfg.dit
    inp = synthetic_inputs(cfg, cuda, n_text=6, seed=42)
    g = torch.Generator().manual_seed(4)
    tokens = torch.randint(0, cfg.tok.codebook_size, (cfg.tok.num_latent_tokens,), generator=g)
    noise = torch.randn(1, d.latent_frames, d.in_channels, d.latent_h, d.latent_w, generator=g).to(cuda)
    lat = {}
    for name, dc in (("off", None), ("zero", 0.0), ("plan", _cfg(0.0, plan=(C, S, C, S, S, C)))):
        pipe = LanDiffPipeline(cfg, st, cuda, dit_cache=dc)
        assert pipe.dit_cache_report() is None
        lat[name] = pipe.generate_latent(tokens, inp, noise=noise).clone()
        rep = pipe.dit_cache_report()
        if dc is None:
            assert rep is None and pipe.dit._sc is None
        else:
            assert len(rep) == 6 and [r["timestep"] for r in rep] == tiny["ts"]
            assert [r["computed"] for r in rep] == ([True] * 6 if name == "zero" else [True, False, True, False, False, True])
    assert torch.equal(lat["zero"], lat["off"])
    assert torch.isfinite(lat["plan"]).all() and not torch.equal(lat["plan"], lat["off"])
    # a stream: every chunk is a sampler run of its own and starts with an empty cache
    T, new, n_seg = pipe.stream_plan(2, 1)
    toks = torch.randint(0, cfg.tok.codebook_size, (n_seg * cfg.tok.num_latent_tokens,), generator=g)
    noises = [torch.randn(1, T, d.in_channels, d.latent_h, d.latent_w, generator=g) for _ in range(2)]
    frames = pipe.generate_stream(inp, 2, prefix_frames=1, tokens=toks, noises=noises)
    assert frames.dtype == torch.uint8 and len(pipe.dit_cache_reports) == 2
    for rep in pipe.dit_cache_reports:
        assert len(rep) == 6 and rep[0]["index"] == 0 and rep[0]["computed"] and rep[0]["input_rel_l1"] is None
        assert [r["computed"] for r in rep] == [True, False, True, False, False, True]
    assert pipe.dit_cache_report() == pipe.dit_cache_reports[-1]
