"""What the DiT step cache costs and saves at full size (15 control + 30 main layers, B = 2, the sampler's 50 steps), random-init
weights, one session on one box -> profiles/dit_step_cache.txt:

  * ms per step of the uncached loop, parent commit and this commit (--parent DIR: a checkout of the parent commit with its library
    built; both legs are this file's `--leg uncached` in a child process each, alternated, so they share code, box and session);
  * ms per step with the cache on and an all-compute plan (what the indicator and residual passes cost);
  * ms of a computed and of a skipped step, and the DiT-loop seconds, for a plan that skips every second interior step;
  * for thresholds 0.05 / 0.1 / 0.2 / 0.4: skipped steps and the relative L2 of the final latent against the uncached run.

Random-init weights say nothing about how many steps a trained checkpoint lets the cache skip or what that costs in quality; every
threshold line of the output says so.

    python tools/dit_step_cache_bench.py --parent /path/to/parent/checkout [--steps 50] [--out profiles/dit_step_cache.txt]
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


def leg_uncached(root, steps):
    """The loop as the parent commit knows it (no step-cache argument anywhere): one JSON line."""
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
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "uncached", "--root", root, "--steps", str(steps)],
                       cwd=root, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"leg in {root} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit, its library built")
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "dit_step_cache.txt"))
    ap.add_argument("--leg", default=None)
    a = ap.parse_args()
    a.root = os.path.abspath(a.root)
    a.parent = os.path.abspath(a.parent) if a.parent else None
    if a.leg == "uncached":
        return leg_uncached(a.root, a.steps)
    S = a.steps
    lines = [f"DiT step cache, full size (15 control + 30 main layers, B = 2, 17 776 tokens), {S} sampler steps, random-init weights.",
             "tools/dit_step_cache_bench.py; all figures from one session on one box; the uncached legs are child processes, alternated.", ""]
    say = lambda s: (print(s, flush=True), lines.append(s))
    # the uncached loop, before this process opens the GPU: parent, this commit, parent, this commit
    legs = {"parent commit": [], "this commit, step_cache=None": []}
    for rep in range(2):
        for name, root in (("parent commit", a.parent), ("this commit, step_cache=None", a.root)):
            if root is None:
                continue
            r = child(root, S)
            legs[name].append(r)
            say(f"{name:30s} run {rep}: {r['ms_per_step']:8.2f} ms per step  ({r['seconds']:.2f} s per {S}-step loop, latent checksum {r['checksum']:.6f})")
    base = None
    for name, rs in legs.items():
        if rs:
            best = min(r["ms_per_step"] for r in rs)
            say(f"{name:30s} best : {best:8.2f} ms per step")
            base = base if base is not None else best
    if not legs["parent commit"]:
        say("(no --parent given: the parent commit was not measured)")
    say("")
    torch, cfg, st, sampler, noise, ctx, sem, dev = setup(a.root, S)
    from landiff_amd.dit import ControlDiTRunner
    from landiff_amd.dit_cache import StepCacheConfig
    ts = [sp.timestep for sp in sampler.plan]
    mk = lambda c: ControlDiTRunner(st["dit_main"], st["dit_control"], cfg.dit, dev, step_cache=c, plan_timesteps=ts if c is not None else None)
    run = mk(None)
    out = torch.empty_like(noise)
    run.set_condition(ctx, sem)
    for i in range(2):
        run.step(noise, 500 - i, -0.7, 0.7, 6.0, out)
    sec0, z0, _ = loop(torch, run, sampler, noise, ctx, sem)
    say(f"{'this process, step_cache=None':30s}      : {sec0 * 1e3 / S:8.2f} ms per step  ({sec0:.2f} s; the reference latent of the lines below)")
    del run
    # cache on, every step computed: the cost of the indicator + residual passes, the extra embed and the host wait
    run = mk(StepCacheConfig(0.0, plan=(True,) * S))
    best = None
    for rep in range(2):
        sec, z, _ = loop(torch, run, sampler, noise, ctx, sem)
        best = sec if best is None else min(best, sec)
        say(f"{'cache on, all-compute plan':30s} run {rep}: {sec * 1e3 / S:8.2f} ms per step  ({sec:.2f} s; latent equal to the uncached one: {bool(torch.equal(z, z0))})")
    ref = base if base is not None else sec0 * 1e3 / S
    ref_name = "the parent commit's best" if legs["parent commit"] else "this process's uncached loop"
    say(f"  -> all-compute step with the cache on vs {ref_name}: {best * 1e3 / S - ref:+.2f} ms per step = {100 * (best * 1e3 / S / ref - 1):+.2f} %")
    rep_all = run.cache_report
    rels = [r["input_rel_l1"] for r in rep_all[1:]]
    say(f"{NOTE}: indicator of this run (relative L1 change of the first block's modulated input, steps 1..{S - 1}): min {min(rels):.4f} median {sorted(rels)[len(rels) // 2]:.4f} max {max(rels):.4f}")
    del run
    # every second interior step skipped
    plan = tuple(True if s in (0, S - 1) else s % 2 == 0 for s in range(S))
    run = mk(StepCacheConfig(0.0, plan=plan))
    sec, z, _ = loop(torch, run, sampler, noise, ctx, sem)
    n_skip = sum(1 for r in run.cache_report if not r["computed"])
    say("")
    say(f"plan skipping every second interior step ({n_skip} of {S} skipped): DiT loop {sec:.2f} s instead of {sec0:.2f} s")
    _, _, ms = loop(torch, run, sampler, noise, ctx, sem, per_step=True)
    comp = [m for m, r in zip(ms, run.cache_report) if r["computed"]]
    skip = [m for m, r in zip(ms, run.cache_report) if not r["computed"]]
    say(f"  per step, synchronised after every step: computed {sum(comp) / len(comp):.2f} ms (n = {len(comp)}), skipped {sum(skip) / len(skip):.2f} ms (n = {len(skip)}, min {min(skip):.2f}, max {max(skip):.2f})")
    rel = ((z.double() - z0.double()).norm() / z0.double().norm()).item()
    say(f"{NOTE}: that plan's relative L2 of the final latent against the uncached run {rel:.4f}")
    del run
    say("")
    for thr in (0.05, 0.1, 0.2, 0.4):
        run = mk(StepCacheConfig(thr))
        sec, z, _ = loop(torch, run, sampler, noise, ctx, sem)
        n_skip = sum(1 for r in run.cache_report if not r["computed"])
        rel = ((z.double() - z0.double()).norm() / z0.double().norm()).item()
        say(f"{NOTE}: threshold {thr:4.2f}: {n_skip:2d} of {S} steps skipped, DiT loop {sec:.2f} s, relative L2 of the final latent against the uncached run {rel:.4f}")
        del run
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
