"""What the retime stage (landiff_amd/retime.py: ld_retime_u8) costs at the size the model produces, one session on one box
-> profiles/retime.txt:

  * 49 frames of 480 x 720 x 3 at 8 fps -> 145 frames at 24 fps (96 interpolated, 49 copied), search 8 and search 16: warm launches
    timed by HIP events, several windows, with their run-to-run spread;
  * the same clip's motion_profile (48 in-between frames, nothing copied) at search 8;
  * beside each: the bytes the launch must read and write divided by the box's measured streaming-read bandwidth
    (bench.py's calibration: ld_calib_stream_read over 1 GiB), and the work counted from the shapes (candidates x window texels);
  * the numpy restatement of the frame rule (tests/retime_ref.py) for ONE frame pair on the CPU with 16 threads, scaled to the
    clip's 96 interpolated frames and labelled as scaled; its output is compared with the kernel's for that pair.

    python tools/retime_bench.py [--launches 10] [--windows 5] [--small] [--out profiles/retime.txt]
"""
import argparse
import os
import socket
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))


def moving_clip(np, F, H, W):
    """A smooth random texture that drifts by (1, -2) pixels a frame, plus a little noise of each frame's own."""
    rng = np.random.default_rng(0)
    m = 2 * F + 8
    coarse = rng.integers(0, 256, ((H + 2 * m) // 8 + 2, (W + 2 * m) // 8 + 2, 3)).astype(np.float64)
    tex = np.kron(coarse, np.ones((8, 8, 1)))[:H + 2 * m, :W + 2 * m]
    tex = (tex + np.roll(tex, 3, 0) + np.roll(tex, 5, 1)) / 3
    frames = np.stack([tex[m - t:m - t + H, m + 2 * t:m + 2 * t + W] for t in range(F)])
    return np.clip(frames + rng.integers(-4, 5, frames.shape), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10, help="kernel launches between the two events of a window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per configuration (their spread is reported)")
    ap.add_argument("--small", action="store_true", help="quarter-size frames: a rehearsal of this script, not a measurement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "retime.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import retime_ref as ref
    from conform_bench import stream_read_gbs
    from landiff_amd.retime import RetimeConfig, motion_profile, retime_clip, retime_plan
    if not torch.cuda.is_available():
        raise SystemExit("tools/retime_bench.py measures on the GPU: no device found")
    lines = ["The retime stage (landiff_amd/retime.py): 49 frames of 480 x 720 x 3 at 8 fps delivered at 24 fps on the GPU."
             + ("  SMALL shapes (a rehearsal of the script: no figure below is a measurement)" if a.small else ""),
             "tools/retime_bench.py; all figures from one session on one box.", ""]
    say = lambda s: (print(s, flush=True), lines.append(s))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.set_num_threads(16)
    say(f"box: {socket.gethostname()}, {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; CPU leg with {torch.get_num_threads()} threads")
    gbs = stream_read_gbs(torch, dev)
    say(f"streaming-read bandwidth of this box (ld_calib_stream_read, 16 B per lane over 1 GiB, bench.py's calibration): {gbs:.0f} GB/s")
    say("")
    flush()
    qd = 4 if a.small else 1
    F, H, W = 49, 480 // qd, 720 // qd
    host = moving_clip(np, F, H, W)
    clip = torch.from_numpy(host).to(dev)
    frame = H * W * 3
    blocks = -(-H // 8) * -(-W // 8)

    def windows(fn):
        fn(); fn(); torch.cuda.synchronize()
        ms = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record(); e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.launches)
        return ms

    def report(name, ms, n_interp, n_copy, R):
        mean = sum(ms) / len(ms)
        # bytes that must move: every source frame read once (each is a neighbour of some output), every output frame written once
        moved = F * frame + (n_interp + n_copy) * frame
        floor_ms = moved / gbs / 1e6
        cands = (2 * R + 1) ** 2
        texels = n_interp * blocks * cands * 256
        say(f"  {name}: {mean:.3f} ms per launch (mean of {len(ms)} windows of {a.launches} launches; min {min(ms):.3f}, max {max(ms):.3f}, "
            f"spread (max - min) {max(ms) - min(ms):.3f} ms = {100 * (max(ms) - min(ms)) / mean:.1f} %)")
        say(f"      bytes that must move (the {F} source frames read once, {n_interp + n_copy} frames written): {moved / 1e6:.0f} MB -> "
            f"bytes / bandwidth = {floor_ms:.3f} ms = {100 * floor_ms / mean:.1f} % of the launch")
        say(f"      counted work: {n_interp} frames x {blocks} blocks x {cands} candidates x 256 window texels = {texels / 1e9:.1f} G absolute "
            f"differences -> {texels / mean / 1e9:.2f} T absolute differences per second; staged per block: 2 x {(16 + 2 * R) ** 2} luma bytes")
        flush()
    say(f"{F} frames of {H} x {W} x 3 ({clip.numel() / 1e6:.0f} MB) at 8 fps -> 24 fps: 145 frames, 96 interpolated + 49 copied; penalty 4, max_sad 24")
    outs = {}
    for R in (8, 16):
        plan = retime_plan(F, RetimeConfig(out_fps=24, search=R))
        assert plan.n_out == 145
        ms = windows(lambda: retime_clip(clip, plan))
        report(f"ld_retime_u8, search {R:2d}", ms, 96, 49, R)
        outs[R] = retime_clip(clip, plan, want_motion=True)
    ms = windows(lambda: motion_profile(clip, search=8))
    report("motion_profile, search 8 (48 in-between frames + the host summary)", ms, 48, 0, 8)
    prof = motion_profile(clip, search=8)
    say(f"      the clip drifts by (1, -2) a frame: mean |dy| + |dx| per pair {min(prof.mean_motion):.2f} .. {max(prof.mean_motion):.2f}, "
        f"fallback share {min(prof.fallback_share):.3f} .. {max(prof.fallback_share):.3f}")
    say("")
    # ---- the numpy restatement, one pair, on the CPU
    for R in (8, 16):
        t0 = time.perf_counter()
        o, mv, sad = ref.interp_frame(host[0], host[1], 1, 3, search=R, penalty=4, max_sad=24)
        sec = time.perf_counter() - t0
        same = (np.array_equal(o, outs[R][0][1].cpu().numpy()) and np.array_equal(mv, outs[R][1][1].cpu().numpy())
                and np.array_equal(sad, outs[R][2][1].cpu().numpy()))
        say(f"  numpy restatement (tests/retime_ref.py), search {R:2d}, ONE frame pair at phase 1/3 on the CPU: {sec:.2f} s; SCALED to the "
            f"clip's 96 interpolated frames (not run): {96 * sec:.0f} s; frame, field and SAD equal the kernel's: {same}")
        flush()
    say("")
    say("Where the time goes inside the kernel was not profiled: no counter or trace run was made.  What is counted above: the bytes "
        "alone would take the stated share of a launch.")
    flush()


if __name__ == "__main__":
    main()
