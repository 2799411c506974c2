"""What clip editing (LanDiffPipeline.edit_video) costs at full size (15 control + 30 main layers, 13 x 60 x 90 latent, the sampler's
50 steps), random-init weights, one session on one box -> profiles/edit_video.txt:

  * ms per step of the featureless 50-step loop, parent commit and this commit (--parent DIR: a checkout of the parent commit with its
    library built; both legs are this file's `--leg featureless` in a child process each, alternated, so they share code, box and
    session), with the spread of the parent leg's own repeats beside the difference;
  * microseconds per ld_latent_pin launch at the full latent (HIP events over many launches), with the bytes it moves, and per
    randn_like draw that goes with it on a masked step;
  * wall seconds of edit_video at strengths 1.0 / 0.6 / 0.3, without a mask and with a pixel mask that keeps half of every frame,
    the clip given as its latent and the tokens given (the VAE encode and the Theia extractor have tools of their own:
    vae_encode_time.py, theia_time.py), each run repeated.

Random-init weights: the times are those of the shipped shapes; nothing here says what an edit looks like on a trained checkpoint.

    python tools/edit_video_bench.py --parent /path/to/parent/checkout [--steps 50] [--repeats 2] [--out profiles/edit_video.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def setup(root, steps, tiny, parts):
    sys.path.insert(0, root)
    import dataclasses
    import torch
    from landiff_amd.config import PipelineConfig
    from landiff_amd.weights import init_pipeline_state
    dev = torch.device("cuda:0")
    cfg = PipelineConfig.tiny() if tiny else PipelineConfig.full()
    cfg = dataclasses.replace(cfg, sampler=dataclasses.replace(cfg.sampler, num_steps=steps)).check()
    st = init_pipeline_state(cfg, seed=1234, dtype=torch.float32 if tiny else torch.bfloat16, device=dev, parts=parts)
    return torch, cfg, st, dev


def leg_featureless(root, steps, tiny):
    """The sampler loop over the DiT as the parent commit knows it (none of the editing arguments anywhere): one JSON line."""
    torch, cfg, st, dev = setup(root, steps, tiny, ["dit_main", "dit_control"])
    from landiff_amd.dit import ControlDiTRunner
    from landiff_amd.sampler import DiffusionSampler
    d = cfg.dit
    g = torch.Generator(device=dev).manual_seed(0)
    noise = torch.randn(1, d.latent_frames, d.in_channels, d.latent_h, d.latent_w, device=dev, generator=g)
    ctx = torch.randn(1, d.text_len, d.text_dim, device=dev, generator=g)
    sem = torch.randn(d.latent_frames, d.in_channels, d.latent_h, d.latent_w, device=dev, generator=g).to(torch.bfloat16)
    run = ControlDiTRunner(st["dit_main"], st["dit_control"], d, dev)
    sampler = DiffusionSampler(cfg.sampler)
    out = torch.empty_like(noise)
    run.set_condition(ctx, sem)
    for i in range(2):
        run.step(noise, 500 - i, -0.7, 0.7, 6.0, out)
    torch.manual_seed(0); torch.cuda.manual_seed(0)
    run.set_condition(ctx, sem)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    z = sampler.run(run.step, noise)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    print(json.dumps({"seconds": sec, "ms_per_step": sec * 1e3 / steps, "checksum": z.double().sum().item()}), flush=True)


def child(root, steps, tiny):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "featureless", "--root", root, "--steps", str(steps)] + (["--tiny"] if tiny else [])
    p = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"leg in {root} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit, its library built")
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=2, help="runs of each featureless leg and of each edit")
    ap.add_argument("--tiny", action="store_true", help="the tiny configuration: a rehearsal of this script, not a measurement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "edit_video.txt"))
    ap.add_argument("--leg", default=None)
    a = ap.parse_args()
    a.root = os.path.abspath(a.root)
    a.parent = os.path.abspath(a.parent) if a.parent else None
    if a.leg == "featureless":
        return leg_featureless(a.root, a.steps, a.tiny)
    S = a.steps
    size = "TINY configuration (a rehearsal of the script: no figure below is a measurement)" if a.tiny else \
        "full size (15 control + 30 main layers, 13 x 60 x 90 latent, 49 frames of 480 x 720)"
    lines = [f"Clip editing (LanDiffPipeline.edit_video), {size}, {S} sampler steps, random-init weights.",
             "tools/edit_video_bench.py; all figures from one session on one box; the featureless legs are child processes, alternated.",
             "Random-init weights: times of the shipped shapes, nothing about the quality of an edit on a trained checkpoint (not measured).", ""]
    say = lambda s: (print(s, flush=True), lines.append(s))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    mean = lambda v: sum(v) / len(v)
    # ---- the featureless loop, before this process opens the GPU: parent, this commit, parent, this commit, ...
    legs = {"parent commit": [], "this commit, no editing argument": []}
    for rep in range(a.repeats):
        for name, root in (("parent commit", a.parent), ("this commit, no editing argument", a.root)):
            if root is None:
                continue
            r = child(root, S, a.tiny)
            legs[name].append(r)
            say(f"{name:34s} run {rep}: {r['ms_per_step']:8.2f} ms per step  ({r['seconds']:.2f} s per {S}-step loop, latent checksum {r['checksum']:.6f})")
            flush()
    for name, rs in legs.items():
        if rs:
            v = [r["ms_per_step"] for r in rs]
            say(f"{name:34s} mean {mean(v):8.2f}  min {min(v):8.2f}  max {max(v):8.2f} ms per step; spread of its own repeats (max - min) "
                f"{max(v) - min(v):.2f} ms = {100 * (max(v) - min(v)) / mean(v):.2f} %")
    if legs["parent commit"]:
        p = [r["ms_per_step"] for r in legs["parent commit"]]
        t = [r["ms_per_step"] for r in legs["this commit, no editing argument"]]
        diff, spread = mean(t) - mean(p), max(max(p) - min(p), max(t) - min(t))
        say(f"  -> this commit - parent commit: {diff:+.2f} ms per step = {100 * diff / mean(p):+.2f} %; the larger of the two legs' own spreads: "
            f"{spread:.2f} ms = {100 * spread / mean(p):.2f} %; the difference lies {'inside' if abs(diff) <= spread else 'OUTSIDE'} it")
        say(f"  -> latent checksums equal across all legs: {len({r['checksum'] for rs in legs.values() for r in rs}) == 1}")
    else:
        say("(no --parent given: the parent commit was not measured)")
    say("")
    flush()
    # ---- this process: the pin launch, then edit_video
    torch, cfg, st, dev = setup(a.root, S, a.tiny, ["tok", "ups", "dit_main", "dit_control", "vae"])
    from landiff_amd import ops
    from landiff_amd.pipeline import LanDiffPipeline, synthetic_inputs
    d = cfg.dit
    T, C, h, w = d.latent_frames, d.in_channels, d.latent_h, d.latent_w
    g = torch.Generator(device=dev).manual_seed(1)
    z0 = torch.randn(1, T, C, h, w, device=dev, generator=g).to(torch.bfloat16).float()
    keep_px = torch.zeros(4 * T - 3, 8 * h, 8 * w, dtype=torch.bool, device=dev)
    keep_px[:, :, 4 * w:] = True                                       # the right half of every frame is kept
    t0 = time.perf_counter()
    mlat = ops.mask_to_latent(keep_px)
    torch.cuda.synchronize()
    kept, cells, n = int(mlat.sum()), mlat.numel(), z0.numel()
    say(f"half-frame pixel mask {tuple(keep_px.shape)} -> latent mask {tuple(mlat.shape)}: {kept} of {cells} cells kept "
        f"(first ld_mask_to_latent call, with its code-object load: {(time.perf_counter() - t0) * 1e3:.2f} ms)")
    x, rd = torch.randn_like(z0), torch.randn_like(z0)
    N = 20 if a.tiny else 200
    for name, m, k in (("half mask", mlat, kept), ("no mask (the SDEdit start)", None, cells)):
        for _ in range(10):
            ops.latent_pin(x, z0, rd, m, 0.6, 0.8)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            ops.latent_pin(x, z0, rd, m, 0.6, 0.8)
        e1.record(); e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / N
        moved = 3 * 4 * C * k + (cells if m is not None else 0)      # known and noise read, x written (fp32, C per kept cell); the mask read
        say(f"ld_latent_pin, {n} fp32 elements, {name:27s}: {us:7.2f} us per launch, back to back ({N} launches between two events; "
            f"{moved / 1e6:.2f} MB needed -> {moved / us / 1e6:.3f} TB/s; the same operands every launch, so they are cache-resident)")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        rd = torch.randn_like(x)
    e1.record(); e1.synchronize()
    say(f"torch.randn_like of the state (the draw a masked step adds with known_noise): {e0.elapsed_time(e1) * 1e3 / N:7.2f} us per draw")
    say("")
    flush()
    del x, rd
    pipe = LanDiffPipeline(cfg, st, dev)
    del st
    torch.cuda.empty_cache()
    inp = synthetic_inputs(cfg, dev, n_text=6, seed=42)
    tok = torch.randint(0, cfg.tok.codebook_size, (cfg.tok.num_latent_tokens,), device=dev, generator=g)
    smallest = 0.5 / S
    strengths = [s for s in (1.0, 0.6, 0.3) if s >= smallest]
    pipe.edit_video(inp, clip_latent=z0, tokens=tok, strength=strengths[-1], keep_mask=keep_px)          # warm-up: every launch of the runs below
    say("edit_video(clip_latent=..., tokens=...): wall seconds of the whole call (host clock, device synchronised), of which the sampler "
        "loop (\"dit\") and the VAE decode (\"vae\")")
    for s in strengths:
        for name, m in (("no mask", None), ("half-frame mask", keep_px)):
            if s == 1.0 and m is None:
                name = "no mask = generation"
            walls = []
            for rep in range(a.repeats):
                pipe.timings = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.edit_video(inp, clip_latent=z0, tokens=tok, strength=s, keep_mask=m)
                torch.cuda.synchronize()
                walls.append(time.perf_counter() - t0)
            e, tm = pipe.last_edit, pipe.timings
            say(f"  strength {s:.1f}, {name:20s}: steps {e['start_step']:2d}..{S - 1} ({e['steps_run']:2d} run), {e['kept_cells']:5d} cells kept: "
                + "  ".join(f"run {i}: {v:6.2f} s" for i, v in enumerate(walls))
                + f"  (last run: dit {tm.get('dit', 0.0):.2f} s = {tm.get('dit', 0.0) * 1e3 / e['steps_run']:.1f} ms per step, vae {tm.get('vae', 0.0):.2f} s, "
                f"detokenize {tm.get('detokenize', 0.0):.2f} s); spread of the repeats {max(walls) - min(walls):.2f} s")
            flush()


if __name__ == "__main__":
    main()
