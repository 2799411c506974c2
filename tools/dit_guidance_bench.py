"""What CFG branch skipping in the DiT costs and saves at full size (15 control + 30 main layers, 17 776 tokens per branch, the
sampler's 50 steps), random-init weights, one session on one box -> profiles/dit_guidance.txt:

  * ms per step of the featureless loop, parent commit and this commit (--parent DIR: a checkout of the parent commit with its library
    built; both legs are this file's `--leg featureless` in a child process each, alternated, so they share code, box and session),
    with the spread of the parent leg's own repeats beside the difference;
  * ms per full step with the feature on (ld_unpatchify_cfg_keep and its sums) against the featureless step;
  * ms per cond and per reuse step and their ratio to a full step, with per-kernel times (HIP events around the attention launches
    and the large linears of the layers that run alone) that account for the ratio's distance from 0.5;
  * the 50-step loop in seconds and the relative L2 of the final latent against the dense run, for scale_tolerance = 1e-5,
    refresh = 2, refresh = 3, and refresh = 2 with attn_window = 1.

Random-init weights say nothing about what any of these settings costs a trained checkpoint in quality; every L2 line says so.

    python tools/dit_guidance_bench.py --parent /path/to/parent/checkout [--steps 50] [--repeats 3] [--out profiles/dit_guidance.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
NOTE = "random-init weights: not evidence about a trained checkpoint"


def setup(root, steps):
    sys.path.insert(0, root)
    import dataclasses
    import torch
    from landiff_amd.config import PipelineConfig
    from landiff_amd.sampler import DiffusionSampler
    from landiff_amd.weights import init_pipeline_state
    dev = torch.device("cuda:0")
    cfg = PipelineConfig.full()
    cfg = dataclasses.replace(cfg, sampler=dataclasses.replace(cfg.sampler, num_steps=steps)).check()
    st = init_pipeline_state(cfg, seed=1234, dtype=torch.bfloat16, device=dev, parts=["dit_main", "dit_control"])
    d = cfg.dit
    g = torch.Generator(device=dev).manual_seed(0)
    noise = torch.randn(1, d.latent_frames, d.in_channels, d.latent_h, d.latent_w, device=dev, generator=g)
    ctx = torch.randn(1, d.text_len, d.text_dim, device=dev, generator=g)
    sem = torch.randn(d.latent_frames, d.in_channels, d.latent_h, d.latent_w, device=dev, generator=g).to(torch.bfloat16)
    return torch, cfg, st, DiffusionSampler(cfg.sampler), noise, ctx, sem, dev


def loop(torch, run, sampler, noise, ctx, sem, per_step=False):
    """One sampler run (same noise, same draws) -> (seconds, latent, [ms per step] when per_step: a synchronise after every step)."""
    torch.manual_seed(0); torch.cuda.manual_seed(0)
    run.set_condition(ctx, sem)
    ms = []

    def step(*a):
        t0 = time.perf_counter()
        r = run.step(*a)
        if per_step:
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return r
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    z = sampler.run(step, noise)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, z, ms


def leg_featureless(root, steps):
    """The loop as the parent commit knows it (no dit_guidance argument anywhere): one JSON line."""
    torch, cfg, st, sampler, noise, ctx, sem, dev = setup(root, steps)
    from landiff_amd.dit import ControlDiTRunner
    run = ControlDiTRunner(st["dit_main"], st["dit_control"], cfg.dit, dev)
    out = torch.empty_like(noise)
    run.set_condition(ctx, sem)
    for i in range(2):
        run.step(noise, 500 - i, -0.7, 0.7, 6.0, out)
    sec, z, _ = loop(torch, run, sampler, noise, ctx, sem)
    print(json.dumps({"seconds": sec, "ms_per_step": sec * 1e3 / steps, "checksum": z.double().sum().item()}), flush=True)


def child(root, steps):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "featureless", "--root", root, "--steps", str(steps)],
                       cwd=root, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"leg in {root} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def kernel_times(torch, run, noise, out, timestep):
    """One step with HIP events around every attention launch and every large linear -> (ms of the attention launches that ran
    alone, ms of the four linears of the same layers by name, wall ms of the step).  Only the main layers behind the last
    control state run with the GPU to themselves (ControlDiTRunner._solo); the overlapped layers' events include their partner."""
    run.attn_events, run.gemm_events = [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run.step(noise, timestep, -0.7, 0.7, 6.0, out)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    attn = [a.elapsed_time(b) for a, b, solo in run.attn_events if solo]
    lin = {}
    # the main branch's events come last (the main stream's launches are issued after the side stream's): four per layer
    for i, (a, b, _) in enumerate(run.gemm_events[-4 * len(attn):]):
        lin.setdefault(("qkv", "dense", "4h", "4h->h")[i % 4], []).append(a.elapsed_time(b))
    run.attn_events = run.gemm_events = None
    return attn, lin, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit, its library built")
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3, help="runs of each featureless leg")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "dit_guidance.txt"))
    ap.add_argument("--leg", default=None)
    a = ap.parse_args()
    a.root = os.path.abspath(a.root)
    a.parent = os.path.abspath(a.parent) if a.parent else None
    if a.leg == "featureless":
        return leg_featureless(a.root, a.steps)
    S = a.steps
    lines = [f"CFG branch skipping in the DiT, full size (15 control + 30 main layers, 17 776 tokens per branch), {S} sampler steps, "
             "random-init weights.",
             "tools/dit_guidance_bench.py; all figures from one session on one box; the featureless legs are child processes, alternated.",
             "Every figure below is taken with random-init weights.", ""]
    say = lambda s: (print(s, flush=True), lines.append(s))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    # the featureless loop, before this process opens the GPU: parent, this commit, parent, this commit, ...
    legs = {"parent commit": [], "this commit, dit_guidance=None": []}
    for rep in range(a.repeats):
        for name, root in (("parent commit", a.parent), ("this commit, dit_guidance=None", a.root)):
            if root is None:
                continue
            r = child(root, S)
            legs[name].append(r)
            say(f"{name:32s} run {rep}: {r['ms_per_step']:8.2f} ms per step  ({r['seconds']:.2f} s per {S}-step loop, random-init weights, latent checksum {r['checksum']:.6f})")
            flush()
    mean = lambda v: sum(v) / len(v)
    base = None
    for name, rs in legs.items():
        if rs:
            v = [r["ms_per_step"] for r in rs]
            say(f"{name:32s} mean {mean(v):8.2f}  min {min(v):8.2f}  max {max(v):8.2f} ms per step; spread of its own repeats (max - min) {max(v) - min(v):.2f} ms = {100 * (max(v) - min(v)) / mean(v):.2f} %  (random-init weights)")
            base = base if base is not None else mean(v)
    if legs["parent commit"]:
        p = [r["ms_per_step"] for r in legs["parent commit"]]
        t = [r["ms_per_step"] for r in legs["this commit, dit_guidance=None"]]
        diff, spread = mean(t) - mean(p), max(p) - min(p)
        say(f"  -> this commit - parent commit: {diff:+.2f} ms per step = {100 * diff / mean(p):+.2f} %; the parent leg's own spread: {spread:.2f} ms "
            f"= {100 * spread / mean(p):.2f} %; the difference lies {'inside' if abs(diff) <= spread else 'OUTSIDE'} it  (random-init weights)")
        say(f"  -> latent checksums equal across all legs: {len({r['checksum'] for rs in legs.values() for r in rs}) == 1}")
    else:
        say("(no --parent given: the parent commit was not measured)")
    say("")
    flush()
    torch, cfg, st, sampler, noise, ctx, sem, dev = setup(a.root, S)
    from landiff_amd.dit import ControlDiTRunner
    from landiff_amd.dit_guidance import GuidanceSkipConfig
    ts = [sp.timestep for sp in sampler.plan]
    mk = lambda c, **kw: ControlDiTRunner(st["dit_main"], st["dit_control"], cfg.dit, dev, dit_guidance=c,
                                          plan_timesteps=ts if c is not None else None, **kw)
    run = mk(None)
    out = torch.empty_like(noise)
    run.set_condition(ctx, sem)
    for i in range(2):
        run.step(noise, 500 - i, -0.7, 0.7, 6.0, out)
    sec0, z0, _ = loop(torch, run, sampler, noise, ctx, sem)
    say(f"{'this process, dit_guidance=None':32s}      : {sec0 * 1e3 / S:8.2f} ms per step  ({sec0:.2f} s; the dense latent of the lines below; random-init weights)")
    attn_f, gem_f, wall_f = kernel_times(torch, run, noise, out, 500)
    del run
    # feature on, every step full: the cost of ld_unpatchify_cfg_keep and its sums over ld_unpatchify_cfg
    run = mk(GuidanceSkipConfig(plan=("full",) * S))
    best = None
    for rep in range(2):
        sec, z, _ = loop(torch, run, sampler, noise, ctx, sem)
        best = sec if best is None else min(best, sec)
        say(f"{'feature on, all-full plan':32s} run {rep}: {sec * 1e3 / S:8.2f} ms per step  ({sec:.2f} s; latent equal to the dense one: {bool(torch.equal(z, z0))}; random-init weights)")
    say(f"  -> full step with the feature on vs this process's featureless loop: {(best - sec0) * 1e3 / S:+.2f} ms per step = {100 * (best / sec0 - 1):+.2f} %  (random-init weights)")
    cosv = [r["cos"] for r in run.guidance_report]
    say(f"{NOTE}: cosine of the two branches' outputs over that run: min {min(cosv):.4f} max {max(cosv):.4f}")
    del run
    flush()
    # per mode, synchronised after every step: full, reuse, cond in turn
    plan = tuple(("full", "reuse", "cond")[s % 3] for s in range(S))
    run = mk(GuidanceSkipConfig(plan=plan))
    loop(torch, run, sampler, noise, ctx, sem)
    _, _, ms = loop(torch, run, sampler, noise, ctx, sem, per_step=True)
    per = {m: [t for t, r in zip(ms, run.guidance_report) if r["mode"] == m] for m in ("full", "reuse", "cond")}
    say("")
    for m in ("full", "reuse", "cond"):
        v = per[m]
        say(f"plan full/reuse/cond in turn, synchronised after every step: {m:5s} step {mean(v):8.2f} ms (n = {len(v)}, min {min(v):.2f}, max {max(v):.2f}); "
            f"ratio to a full step {mean(v) / mean(per['full']):.3f}  (random-init weights)")
    # where the distance from 0.5 comes from: a cond step and a full step, kernel by kernel (the layers that run alone)
    run2 = mk(GuidanceSkipConfig(plan=("cond",) * S))
    run2.set_condition(ctx, sem)
    run2.step(noise, ts[0], -0.7, 0.7, 6.0, out)
    attn_c, gem_c, wall_c = kernel_times(torch, run2, noise, out, ts[1])
    say("")
    say(f"per kernel, the {len(attn_f)} main layers that run alone (HIP events; B = 2 step / B = 1 step; random-init weights):")
    say(f"  attention launch : {mean(attn_f):7.3f} / {mean(attn_c):7.3f} ms, ratio {mean(attn_c) / mean(attn_f):.3f}  (4200 / 2100 workgroups on 512 slots: 8.2 / 4.1 rounds, i.e. 9 / 5 with the partial one = 0.556)")
    for name in gem_f:
        say(f"  linear {name:9s} : {mean(gem_f[name]):7.3f} / {mean(gem_c[name]):7.3f} ms, ratio {mean(gem_c[name]) / mean(gem_f[name]):.3f}")
    lay_f = mean(attn_f) + sum(mean(v) for v in gem_f.values())
    lay_c = mean(attn_c) + sum(mean(v) for v in gem_c.values())
    say(f"  attention + linears per layer: {lay_f:.3f} / {lay_c:.3f} ms, ratio {lay_c / lay_f:.3f}; step wall time with the events on: {wall_f:.2f} / {wall_c:.2f} ms, ratio {wall_c / wall_f:.3f}")
    say(f"  the rest of a step (LayerNorms, embeddings, modulation GEMVs, final layer, launch gaps): {wall_f - 45 * lay_f:.2f} / {wall_c - 45 * lay_c:.2f} ms "
        "when every one of the 45 layers is priced as a solo layer (the overlapped layers cost less than that: a lower bound of the rest)")
    del run, run2
    flush()
    say("")
    from landiff_amd.config import AttnWindowConfig
    dense_win = None
    for name, gc, kw in (("scale_tolerance = 1e-5", GuidanceSkipConfig(scale_tolerance=1e-5), {}),
                         ("refresh = 2", GuidanceSkipConfig(refresh=2), {}),
                         ("refresh = 3", GuidanceSkipConfig(refresh=3), {}),
                         ("attn_window = 1 alone", None, dict(attn_window=AttnWindowConfig(frames=1))),
                         ("refresh = 2 with attn_window = 1", GuidanceSkipConfig(refresh=2), dict(attn_window=AttnWindowConfig(frames=1)))):
        run = mk(gc, **kw)
        sec, z, _ = loop(torch, run, sampler, noise, ctx, sem)
        modes = [r["mode"] for r in run.guidance_report]
        rel = ((z.double() - z0.double()).norm() / z0.double().norm()).item()
        extra = ""
        if name == "attn_window = 1 alone":
            dense_win = z
        elif kw and dense_win is not None:
            extra = f", against the windowed run with both branches {((z.double() - dense_win.double()).norm() / dense_win.double().norm()).item():.4f}"
        what = (f"{modes.count('full'):2d} full / {modes.count('reuse'):2d} reuse / {modes.count('cond'):2d} cond steps" if gc is not None
                else "both branches on every step (dit_guidance=None)")
        say(f"{NOTE}: {name:34s}: {what}, DiT loop {sec:.2f} s "
            f"instead of {sec0:.2f} s, relative L2 of the final latent against the dense run {rel:.4f}{extra}")
        del run
        flush()


if __name__ == "__main__":
    main()
