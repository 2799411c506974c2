"""CFG branch skipping of the DiT on the GPU: the two entry points of ld_dit_guidance.hip against torch (op by op, on the CPU), the
guided ControlDiTRunner against the featureless one (a full step is the featureless step bit for bit; a reuse step is a cond step
plus g * delta, bit for bit; a cond step sits within the project's bounds of the oracle's cond branch), one run at the config0 shape
with a window, one at the BASELINE shape, the DiT's four GEMMs at the B = 1 row count, and the pipeline switch.

Whether a cond-only step's network output equals the cond row of a B = 2 step bit for bit is printed, not asserted."""
import math
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F, R, C = "full", "reuse", "cond"
NAN32 = 0x7FC0A5A5
# a single patch; odd C; the tiny DiT; several workgroups (120) and several trips per lane (4)
SHAPES = [(1, 1, 2, 2, 2), (2, 3, 6, 10, 2), (3, 16, 8, 12, 2), (5, 16, 32, 48, 2)]
SCAL = (-0.8125, 0.59375, 3.7)                 # c_out, c_skip, scale


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _unpatch(lin_row, T, Cc, H, W, p):
    """lin row [n_img, C*p*p] (CPU) -> fp32 [T, C, H, W]: unpatchify (a pure permutation)."""
    return lin_row.float().view(T, H // p, W // p, Cc, p, p).permute(0, 3, 1, 4, 2, 5).reshape(T, Cc, H, W).contiguous()


def _torch_step(lin, x, c_out, c_skip, scale, shape):
    """The arithmetic of the three modes, one rounded fp32 torch op at a time, on the CPU.  -> dict(e_u, e_c, d_u, d_c, delta, full)."""
    T, Cc, H, W, p = shape
    lin, x = lin.cpu(), x.cpu().reshape(T, Cc, H, W)
    eu, ec = _unpatch(lin[0], *shape), _unpatch(lin[1], *shape)
    xs = x * _f32(c_skip)
    du = eu * _f32(c_out) + xs
    dc = ec * _f32(c_out) + xs
    delta = dc - du
    return dict(e_u=eu, e_c=ec, d_u=du, d_c=dc, delta=delta, full=du + _f32(scale) * delta)


def _inputs(cuda, shape, seed):
    T, Cc, H, W, p = shape
    g = torch.Generator().manual_seed(seed)
    n_img, K = T * (H // p) * (W // p), Cc * p * p
    u = torch.randn(n_img, K, generator=g)
    lin = torch.stack([u, u + 0.3 * torch.randn(n_img, K, generator=g)]).to(BF).to(cuda)
    x = torch.randn(1, T, Cc, H, W, generator=g).to(cuda)
    return lin, x


def _guarded(cuda, x, guard=16):
    """A tensor of x's shape inside a buffer of NaN sentinels -> (buffer bits, view)."""
    n = x.numel()
    bits = torch.full((n + 2 * guard,), NAN32, device=cuda, dtype=torch.int32)
    return bits, bits.view(torch.float32)[guard:guard + n].view(x.shape)


def _guards_intact(bits, n, guard=16):
    return bool((bits[:guard] == NAN32).all()) and bool((bits[guard + n:] == NAN32).all())


def _close(got, want, scale, what):
    """|got - want| <= 1e-5 * sum|terms|: the bound tests/test_gpu_dit_cache.py::_close derives for an fp32 sum tree of this depth
    (here at most 5 trips + 6 + 2 + 4 + 6 + 2 = 25 additions, 25 * 2^-24 = 1.5e-6, plus 2^-24 per product / difference), taken
    against the sum of the terms' magnitudes (the signed sum's own value can be small)."""
    print(f"{what}: got {got!r} want {want!r} |err| / sum|terms| {abs(got - want) / scale if scale else 0.0:.3e}")
    assert abs(got - want) <= 1e-5 * scale, (what, got, want, scale)


# ---- kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_unpatchify_cfg_keep(cuda, shape):
    from landiff_amd import ops
    p = shape[4]
    lin, x = _inputs(cuda, shape, zlib.crc32(repr(shape).encode()))
    n = x.numel()
    ref = _torch_step(lin, x, *SCAL, shape)
    want_out = torch.empty_like(x)
    ops.unpatchify_cfg(lin, x, want_out, p, *SCAL)
    ob, out = _guarded(cuda, x)
    db, delta = _guarded(cuda, x[0])
    sums = ops.unpatchify_cfg_keep(lin, x, out, delta, p, *SCAL)
    assert sums.dtype == torch.float32 and sums.shape == (5,)
    assert torch.equal(out, want_out), "out must be the bits of ld_unpatchify_cfg"
    assert torch.equal(delta.cpu(), ref["delta"])
    assert _guards_intact(ob, n) and _guards_intact(db, n)
    eu, ec = ref["e_u"].double(), ref["e_c"].double()
    s = sums.tolist()
    _close(s[0], (eu * ec).sum().item(), (eu * ec).abs().sum().item(), f"{shape} sum e_u e_c")
    _close(s[1], (eu * eu).sum().item(), (eu * eu).sum().item(), f"{shape} sum e_u^2")
    _close(s[2], (ec * ec).sum().item(), (ec * ec).sum().item(), f"{shape} sum e_c^2")
    assert s[3] == 0.0 and s[4] == 0.0                                            # no older difference
    # an older difference: as a separate buffer, and as the buffer the new one overwrites -- the same sums, bit for bit
    g = torch.Generator().manual_seed(1)
    old = (ref["delta"] * 1.05 + 0.01 * torch.randn(ref["delta"].shape, generator=g)).to(cuda)
    want3 = (ref["delta"].double() - old.cpu().double()).abs().sum().item()
    want4 = old.cpu().double().abs().sum().item()
    d2 = torch.empty_like(delta)
    sums_sep = ops.unpatchify_cfg_keep(lin, x, out, d2, p, *SCAL, delta_old=old).clone()
    assert torch.equal(d2, delta) and torch.equal(out, want_out) and torch.equal(sums_sep[:3], sums[:3])
    _close(sums_sep[3].item(), want3, want3, f"{shape} sum|delta - old|")
    _close(sums_sep[4].item(), want4, want4, f"{shape} sum|old|")
    ab, alias = _guarded(cuda, x[0])
    alias.copy_(old)
    sums_alias = ops.unpatchify_cfg_keep(lin, x, out, alias, p, *SCAL, delta_old=alias)
    assert torch.equal(sums_alias, sums_sep) and torch.equal(alias, delta) and _guards_intact(ab, n)
    # run to run: the same bits
    assert torch.equal(ops.unpatchify_cfg_keep(lin, x, out, d2, p, *SCAL, delta_old=old), sums_sep)
    assert _guards_intact(ob, n)


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_unpatchify_cond(cuda, shape):
    from landiff_amd import ops
    p = shape[4]
    lin, x = _inputs(cuda, shape, zlib.crc32(repr(shape).encode()) + 1)
    n = x.numel()
    ref = _torch_step(lin, x, *SCAL, shape)
    c_out, c_skip, scale = SCAL
    ob, out = _guarded(cuda, x)
    ops.unpatchify_cond(lin[1], x, out, p, c_out, c_skip)
    assert torch.equal(out.cpu()[0], ref["d_c"]) and _guards_intact(ob, n)
    delta = ref["delta"].to(cuda)
    ops.unpatchify_cond(lin[1], x, out, p, c_out, c_skip, scale, delta=delta)
    g = _f32(scale) - _f32(1.0)                                                   # fp32, from the fp32 scale
    assert torch.equal(out.cpu()[0], ref["d_c"] + g * ref["delta"]) and _guards_intact(ob, n)
    assert not torch.equal(out.cpu()[0], ref["d_c"])
    ops.unpatchify_cond(lin[1], x, out, p, c_out, c_skip, 1.0, delta=delta)       # scale 1, a finite delta: d_c exactly
    assert torch.equal(out.cpu()[0], ref["d_c"]) and _guards_intact(ob, n)
    assert torch.equal(delta.cpu(), ref["delta"])                                # (read only)


# ---- runner on the tiny DiT ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(cuda):
    """Tiny DiT, the 6 sampler steps' scalars, an input per step, and the featureless runner's outputs (computed once)."""
    from landiff_amd.config import PipelineConfig
    from landiff_amd.schedule import build_plan
    from landiff_amd.weights import init_pipeline_state
    cfg = PipelineConfig.tiny(num_steps=6).check()
    st = init_pipeline_state(cfg, seed=1234)
    d = cfg.dit
    plan = build_plan(cfg.sampler)
    g = torch.Generator().manual_seed(22)
    shape = (1, d.latent_frames, d.in_channels, d.latent_h, d.latent_w)
    x0, dx = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    xs = [(x0 + 0.03 * s * dx).to(cuda) for s in range(6)]
    ctx = torch.randn(1, d.text_len, d.text_dim, generator=g)
    sem = (0.5 * torch.randn(d.latent_frames, d.in_channels, d.latent_h, d.latent_w, generator=g)).to(BF)
    t = dict(cfg=cfg, st=st, d=d, plan=plan, xs=xs, ctx=ctx, sem=sem, ts=[sp.timestep for sp in plan])
    t["ref"] = _run(_runner(t, cuda, None), t)
    return t


def _gcfg(**kw):
    from landiff_amd.dit_guidance import GuidanceSkipConfig
    return GuidanceSkipConfig(**kw)


def _runner(t, cuda, guidance, **kw):
    from landiff_amd.dit import ControlDiTRunner
    if guidance is not None:
        kw.update(dit_guidance=guidance, plan_timesteps=t["ts"])
    run = ControlDiTRunner(t["st"]["dit_main"], t["st"]["dit_control"], t["d"], cuda, **kw)
    run.set_condition(t["ctx"], t["sem"])
    return run


def _step(run, t, s, scale=None):
    sp = t["plan"][s]
    out = torch.empty_like(t["xs"][s])
    run.step(t["xs"][s], sp.timestep, sp.c_out, sp.c_skip, sp.cfg_scale if scale is None else scale, out)
    return out


def _run(run, t):
    return [_step(run, t, s).clone() for s in range(6)]


@pytest.mark.parametrize("overlap", ["0", "1"])
def test_all_full_plan_is_the_featureless_runner(cuda, tiny, monkeypatch, overlap):
    from landiff_amd import ops
    monkeypatch.setenv("LD_DIT_OVERLAP", overlap)
    run = _runner(tiny, cuda, _gcfg(plan=(F,) * 6))
    d = tiny["d"]
    assert run.overlap == (overlap == "1") and run.guidance_delta is None
    for s in range(6):
        sp = tiny["plan"][s]
        assert torch.equal(_step(run, tiny, s), tiny["ref"][s]), s
        delta, out = torch.empty_like(run.guidance_delta), torch.empty_like(tiny["xs"][s])
        ops.unpatchify_cfg_keep(run.lin, tiny["xs"][s], out, delta, d.patch, sp.c_out, sp.c_skip, sp.cfg_scale)
        assert torch.equal(run.guidance_delta, delta) and run.guidance_delta.shape == tuple(tiny["xs"][s].shape[1:])
    rep = run.guidance_report
    assert [r["mode"] for r in rep] == [F] * 6 and [r["index"] for r in rep] == list(range(6))
    assert [r["timestep"] for r in rep] == tiny["ts"] and [r["cfg_scale"] for r in rep] == [sp.cfg_scale for sp in tiny["plan"]]
    assert rep[0]["delta_rel_l1"] is None and all(r["delta_rel_l1"] > 0 and math.isfinite(r["delta_rel_l1"]) for r in rep[1:])
    assert all(-1.0 <= r["cos"] <= 1.0 and r["delta_from"] is None for r in rep)


def test_featureless_runner_has_nothing_new(cuda, tiny):
    from landiff_amd.dit import ControlDiTRunner
    run = _runner(tiny, cuda, None)
    assert run._gd is None and run.guidance_report == [] and run.guidance_delta is None
    assert not [k for k in vars(run) if k.startswith("_gd_")] and "B" not in vars(run) and "_step_B" not in vars(run)
    # (the one addition outside the feature: under attn_exact="auto" the host list _fb_blocks, the block count a step's fallback
    #  fraction is taken against -- two integers, no device memory)
    assert not run.attn_auto or run._fb_blocks == [0, 0]
    run.reset_guidance()                                  # a no-op
    with pytest.raises(ValueError, match="plan_timesteps"):
        ControlDiTRunner(tiny["st"]["dit_main"], tiny["st"]["dit_control"], tiny["d"], cuda, dit_guidance=_gcfg(refresh=2))
    with pytest.raises(ValueError, match="entries"):
        ControlDiTRunner(tiny["st"]["dit_main"], tiny["st"]["dit_control"], tiny["d"], cuda, dit_guidance=_gcfg(plan=(F, C)),
                         plan_timesteps=tiny["ts"])


def test_attn_auto_fraction_is_taken_against_the_launch_that_was_made(cuda, tiny):
    """attn_exact="auto": a cond-only step's launches have half the 256-row blocks of a full step's, and the 25 % limit is applied to
    that count -- a layer's decision does not depend on the guidance plan."""
    run = _runner(tiny, cuda, _gcfg(plan=(F, C, R, F, C, F)), attn_exact="auto")
    full, L = run._attn_blocks, tiny["d"].layers_control + tiny["d"].layers_main
    assert full % 2 == 0 and full >= 4
    for s, want in enumerate((full, full // 2, full // 2, full, full // 2, full)):
        par = run._fb_par                                 # the slot this step's end writes
        _step(run, tiny, s)
        assert run._fb_blocks[par] == want, (s, run._fb_blocks)
    torch.cuda.synchronize()
    # the limit itself: a quarter of the B = 2 blocks falling back is not "more than 25 %" of a full step's launch, and is of a
    # cond-only step's (the counts of one call are acted on by the next)
    for step_B, want in ((2, set()), (1, set(range(L)))):
        run.reset_attn_auto()
        run._fb.fill_(full // 4)
        run._attn_auto_end_of_step(step_B)
        run._attn_auto_end_of_step(step_B)
        assert run.exact_layers == want, (step_B, run.exact_layers)


def test_cond_step_against_the_oracle(cuda, tiny):
    """The cond branch alone, against the oracle's cond row: the bf16 oracle within tests/test_gpu_stages.py's 2e-2, the fp32
    oracle within that test's floor rule max(2 * floor, 1e-2)."""
    from oracle.dit import ControlDiTOracle
    d, st, s = tiny["d"], tiny["st"], 1
    sp, x, ctx, sem = tiny["plan"][s], tiny["xs"][s].cpu(), tiny["ctx"], tiny["sem"][None]
    run = _runner(tiny, cuda, _gcfg(plan=(C,) * 6))
    out = _step(run, tiny, s)
    assert run.guidance_report[-1]["mode"] == C and run.guidance_delta is None
    den = {}
    for dt in (torch.bfloat16, torch.float32):
        orc = ControlDiTOracle(st["dit_main"], st["dit_control"], d, dt)
        net = orc(torch.cat([x, x]), torch.full((2,), float(sp.timestep)), torch.cat([torch.zeros_like(ctx), ctx]), sem.to(dt))
        den[dt] = net[1:].float() * sp.c_out + x * sp.c_skip
    e16, e32, floor = rel(out, den[torch.bfloat16]), rel(out, den[torch.float32]), rel(den[torch.bfloat16], den[torch.float32])
    print(f"cond step: rel to the bf16 oracle's d_c {e16:.4e}, to the fp32 oracle's {e32:.4e} (bf16 floor {floor:.4e})")
    assert e16 < 2e-2, e16
    assert e32 < max(2 * floor, 1e-2), (e32, floor)
    # for the record: is the cond-only step's network output the cond row of the B = 2 step, bit for bit?
    lin_cond = run.lin[1].clone()
    full = _runner(tiny, cuda, None)
    _step(full, tiny, s)
    print(f"tiny: cond-only lin == cond row of the B = 2 step: {torch.equal(lin_cond, full.lin[1])}")


@pytest.mark.parametrize("overlap", ["0", "1"])
def test_plan_full_reuse_reuse_full_cond_full(cuda, tiny, monkeypatch, overlap):
    monkeypatch.setenv("LD_DIT_OVERLAP", overlap)
    plan = (F, R, R, F, C, F)
    run = _runner(tiny, cuda, _gcfg(plan=plan))
    cond = _runner(tiny, cuda, _gcfg(plan=(C,) * 6))
    deltas, lins, checked_a_visible_reuse = {}, {}, False
    for s in range(6):
        sp = tiny["plan"][s]
        got = _step(run, tiny, s)
        assert torch.isfinite(got).all()
        if plan[s] == F:                                  # nothing leaks from the batch-1 steps before it
            assert torch.equal(got, tiny["ref"][s]), s
            deltas[s], lins[s] = run.guidance_delta.clone(), run.lin.clone()
            last_full = s
        else:
            d_c = _step(cond, tiny, s)
            if plan[s] == C:
                assert torch.equal(got, d_c), s
            else:
                g = _f32(sp.cfg_scale) - _f32(1.0)
                want = d_c.cpu()[0] + g * deltas[last_full].cpu()
                assert torch.equal(got.cpu()[0], want), s
                dl = deltas[last_full]
                print(f"step {s} (reuse of step {last_full}): max|delta| {dl.abs().max().item():.3e}, non-zero {int((dl != 0).sum())} of {dl.numel()}; "
                      f"elements off the cond step's {int((got != d_c).sum())}, off the featureless step's {int((got != tiny['ref'][s]).sum())}")
                if abs(g.item()) * dl.abs().max().item() > 1e-3:          # (this schedule's scale is within 1e-6 of 1 on some steps)
                    assert not torch.equal(got, d_c) and not torch.equal(got, tiny["ref"][s])
                    checked_a_visible_reuse = True
            assert torch.equal(run.guidance_delta, deltas[last_full])            # kept, untouched
    assert checked_a_visible_reuse
    rep = run.guidance_report
    assert [r["mode"] for r in rep] == list(plan)
    assert [r["delta_from"] for r in rep] == [None, 0, 0, None, None, None]
    assert [r["delta_rel_l1"] is not None for r in rep] == [False, False, False, True, False, True]
    assert [r["cos"] is not None for r in rep] == [m == F for m in plan]
    for s, prev in ((3, 0), (5, 3)):
        a, b = deltas[s].double(), deltas[prev].double()
        want = ((a - b).abs().sum() / b.abs().sum()).item()
        assert abs(rep[s]["delta_rel_l1"] - want) <= 3e-5 * want, (s, rep[s]["delta_rel_l1"], want)
    for s in (0, 3, 5):
        eu, ec = lins[s][0].double(), lins[s][1].double()
        den = math.sqrt((eu * eu).sum().item() * (ec * ec).sum().item())
        want = (eu * ec).sum().item() / den
        assert abs(rep[s]["cos"] - want) <= 1e-5 * (eu * ec).abs().sum().item() / den + 3e-5, (s, rep[s]["cos"], want)


def test_same_six_steps_twice_in_one_runner(cuda, tiny):
    """A timestep that does not decrease starts a new run; so does set_condition(): equal outputs and equal reports."""
    run = _runner(tiny, cuda, _gcfg(refresh=3, scale_tolerance=0.0))
    outs, reps = [], []
    for again in range(3):
        if again == 2:
            run.set_condition(tiny["ctx"], tiny["sem"])
            assert run.guidance_report == [] and run.guidance_delta is None
        outs.append(_run(run, tiny))
        reps.append([dict(r) for r in run.guidance_report])
    assert [r["mode"] for r in reps[0]] == [F, R, R, F, R, R] and [r["delta_from"] for r in reps[0]] == [None, 0, 0, None, 3, 3]
    for again in (1, 2):
        assert reps[again] == reps[0]
        assert all(torch.equal(a, b) for a, b in zip(outs[again], outs[0]))


def test_cos_rule(cuda, tiny):
    run = _runner(tiny, cuda, _gcfg(cos_threshold=-0.999999))
    cond = _runner(tiny, cuda, _gcfg(plan=(C,) * 6))
    for s in range(6):
        got = _step(run, tiny, s)
        assert torch.equal(got, tiny["ref"][0] if s == 0 else _step(cond, tiny, s)), s
    rep = run.guidance_report
    assert [r["mode"] for r in rep] == [F] + [C] * 5 and rep[0]["cos"] >= -0.999999
    run = _runner(tiny, cuda, _gcfg(cos_threshold=1.0))                           # distinct branches: never reached
    for s in range(6):
        assert torch.equal(_step(run, tiny, s), tiny["ref"][s]), s
    rep = run.guidance_report
    assert [r["mode"] for r in rep] == [F] * 6 and all(r["cos"] < 1.0 for r in rep)


# ---- config0 shape with a window; BASELINE shape ------------------------------------------------------------------------------
def test_cond_step_with_attn_window_at_config0(cuda):
    from landiff_amd.config import DiTConfig
    from landiff_amd.dit import ControlDiTRunner
    from landiff_amd.weights import dit_spec, init_state
    d = DiTConfig.config0()
    g = torch.Generator().manual_seed(32)
    x = torch.randn(1, d.latent_frames, d.in_channels, d.latent_h, d.latent_w, generator=g).to(cuda)
    ctx = torch.randn(1, d.text_len, d.text_dim, generator=g)
    sem = (0.5 * torch.randn(d.latent_frames, d.in_channels, d.latent_h, d.latent_w, generator=g)).to(BF)
    main, ctrl = init_state(dit_spec(d, False), 5), init_state(dit_spec(d, True), 6)
    outs, lin = {}, {}
    for name, gd in (("full", _gcfg(plan=(F, F))), ("cond", _gcfg(plan=(C, C)))):
        run = ControlDiTRunner(main, ctrl, d, cuda, attn_window=1, dit_guidance=gd, plan_timesteps=[900, 500])
        run.set_condition(ctx, sem)
        outs[name] = torch.empty_like(x)
        run.step(x, 900, -0.8, 0.6, 1.0, outs[name])
        assert run._win_on and run.guidance_report[-1]["mode"] == name
        lin[name] = run.lin[1].clone()
    err = rel(outs["cond"], outs["full"])
    print(f"config0, attn_window=1: cond step against a full step at cfg_scale 1.0: rel {err:.4e}; "
          f"cond-only lin == cond row of the B = 2 step: {torch.equal(lin['cond'], lin['full'])}")
    assert torch.isfinite(outs["cond"]).all() and err < 2e-2, err


def test_full_shape_full_reuse_cond(cuda):
    """1 control + 1 main layer at the BASELINE shape (B = 1: 17 776 rows), plan full / reuse / cond."""
    from landiff_amd.dit import ControlDiTRunner
    from oracle_jobs import dit_layer_inputs
    d1, sd_main, sd_ctrl, _, _ = dit_layer_inputs()
    g = torch.Generator().manual_seed(9)
    shape = (1, d1.latent_frames, d1.in_channels, d1.latent_h, d1.latent_w)
    x0, dx = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    xs = [(x0 + 0.05 * s * dx).to(cuda) for s in range(3)]
    ctx = torch.randn(1, d1.text_len, d1.text_dim, generator=g)
    sem = (0.5 * torch.randn(d1.latent_frames, d1.in_channels, d1.latent_h, d1.latent_w, generator=g)).to(BF)
    ts, c_out, c_skip, scale = [900, 600, 300], -0.8, 0.6, 4.0
    run = ControlDiTRunner(sd_main, sd_ctrl, d1, cuda, dit_guidance=_gcfg(plan=(F, R, C)), plan_timesteps=ts)
    cond = ControlDiTRunner(sd_main, sd_ctrl, d1, cuda, dit_guidance=_gcfg(plan=(C, C, C)), plan_timesteps=ts)
    assert run.N == 17776 and run.M == 2 * 17776
    run.set_condition(ctx, sem); cond.set_condition(ctx, sem)
    got = [torch.empty_like(x) for x in xs]
    for s in range(3):
        run.step(xs[s], ts[s], c_out, c_skip, scale, got[s])
        assert torch.isfinite(got[s]).all(), s
        assert (run.B, run.M) == (2, 2 * 17776)
    lin_full = run.lin[1].clone()
    delta = run.guidance_delta.cpu()
    d_c = torch.empty_like(xs[1])
    cond.step(xs[1], ts[1], c_out, c_skip, scale, d_c)
    assert torch.equal(got[1].cpu()[0], d_c.cpu()[0] + (_f32(scale) - _f32(1.0)) * delta)           # the reuse identity, exactly
    full1 = torch.empty_like(xs[2])
    ref = ControlDiTRunner(sd_main, sd_ctrl, d1, cuda)
    ref.set_condition(ctx, sem)
    ref.step(xs[2], ts[2], c_out, c_skip, 1.0, full1)
    err = rel(got[2], full1)
    print(f"BASELINE shape, 1 + 1 layers: cond step against a full step at cfg_scale 1.0: rel {err:.4e}; "
          f"cond-only lin == cond row of the B = 2 step: {torch.equal(lin_full, ref.lin[1])}")
    assert err < 2e-2, err
    assert [r["mode"] for r in run.guidance_report] == [F, R, C] and run.guidance_report[1]["delta_from"] == 0


# ---- the DiT's four GEMMs at the cond-only step's row count ------------------------------------------------------------------
M1, D, TEXT = 17776, 1920, 226
# (id, N, K, lda pad, ldo pad, form).  qkv bias / dense gate / 4h -> h gate + add2 in place: exact operands, bit-equal to the float64
# reference.  4h GELU: tests/test_gpu_gemm_routes.py's reference refuses an activation on exact operands (tanh of an integer is no bf16
# number, so there is no exact form); it takes that file's random form -- every element inside its own derived error bound.
B1_GEMMS = [("qkv_bias", 3 * D, D, 64, 64, "bias"), ("dense_gate", D, D, 64, 64, "gate"),
            ("h4_gelu_tanh", 4 * D, D, 64, 64, "gelu"), ("h1_gate_add2_inplace", D, 4 * D, 0, 64, "gate_add2_inplace")]


@pytest.mark.parametrize("case", B1_GEMMS, ids=[c[0] for c in B1_GEMMS])
def test_dit_gemms_at_one_batch_of_rows(cuda, case):
    from landiff_amd import ops
    from test_dit_guidance_host import B1_ROUTES
    from test_gpu_gemm_routes import _check_sentinels, _gate_values, _operands, _reference, _route, _sentinel_buffer, _small
    name, N, K, lda_pad, ldo_pad, form = case
    exact = form != "gelu"
    a, w, g = _operands(M1, N, K, exact, zlib.crc32(name.encode()), cuda, lda_pad)
    bits, out = _sentinel_buffer(M1, N, N + ldo_pad, BF, cuda)
    epi = dict(bias=_small((N,), g, cuda, -4, 4, exact, 0.5))
    if form == "gelu":
        epi["act"] = "gelu_tanh"
    elif form != "bias":                                  # the DiT's gate layout, one batch: ada [1, 12 N], rows_per_batch = M
        epi.update(gate=_gate_values((1, 12 * N), g, cuda, True), gate_bstride=12 * N, rows_per_batch=M1, text_len=TEXT)
        if form == "gate":
            epi.update(gate_off_img=2 * N, gate_off_txt=8 * N, resid=_small((M1, N), g, cuda, -8, 8, True))
        else:
            out.copy_(_small((M1, N), g, cuda, -8, 8, True))
            epi.update(gate_off_img=5 * N, gate_off_txt=11 * N, add2=_small((M1, N), g, cuda, -8, 8, True), resid=out)
    assert _route(M1, N, K, out.stride(0), **epi) == B1_ROUTES[name.split("_")[0]]
    ref, err = _reference(a, w, dict(epi, resid=out.clone()) if epi.get("resid") is out else epi, exact, N)
    ops.gemm(a, w, out=out, **epi)
    torch.cuda.synchronize()
    got = out.double()
    if exact:
        bad = got != ref
        assert not bool(bad.any()), f"{int(bad.sum())} of {M1 * N} elements differ; NaN (unwritten): {int(torch.isnan(got).sum())}"
    else:
        dlt = (got - ref).abs()
        print(f"\n{name}: worst element at {(dlt / err).max().item():.3f} of its bound")
        assert not bool((dlt > err).any()), f"{int((dlt > err).sum())} elements over their bound"
    _check_sentinels(bits, M1, N)


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
    base = LanDiffPipeline(cfg, st, cuda)
    lat = base.generate_latent(tokens, inp, noise=noise).clone()
    frames_base = base.decode(lat, want_float=True)[0].clone()
    off = LanDiffPipeline(cfg, st, cuda, dit_guidance=None)
    assert off.dit._gd is None and off.dit_guidance is None
    lat_off = off.generate_latent(tokens, inp, noise=noise).clone()
    assert off.dit_guidance_report() is None and off.dit_guidance_reports == []
    assert torch.equal(lat_off, lat) and torch.equal(off.decode(lat_off, want_float=True)[0], frames_base)
    pipe = LanDiffPipeline(cfg, st, cuda, dit_guidance=_gcfg(refresh=2))
    assert pipe.dit_guidance_report() is None
    z = pipe.generate_latent(tokens, inp, noise=noise).clone()
    frames = pipe.decode(z, want_float=True)[0]
    rep = pipe.dit_guidance_report()
    assert [r["mode"] for r in rep] == [F, R, F, R, F, R] and [r["timestep"] for r in rep] == tiny["ts"]
    assert torch.isfinite(z).all() and not torch.equal(z, lat)
    assert frames.dtype == torch.uint8 and frames.shape == frames_base.shape
    with pytest.raises(ValueError, match="step_cache"):
        LanDiffPipeline(cfg, st, cuda, dit_guidance=0.01, dit_cache=0.1)
