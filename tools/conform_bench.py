"""What the conform stage (landiff_amd/conform.py: ld_resize_u8, ld_resize_mask_u8) costs at the sizes a user brings, one session
on one box -> profiles/conform.txt:

  * a 184-frame 1080 x 1920 clip at 30 fps and a 49-frame 2160 x 3840 clip, each conformed (fit="cover") to 49 x 480 x 720: the host
    selection + upload of the frames the plan reads, and the kernel (HIP events over repeated launches), reported separately, for
    both filters; the keep-mask kernel on the same geometry;
  * beside each: F.interpolate(antialias=True) on the CPU with 16 threads for the same frames and box, and the bytes the kernel
    must read and write divided by the box's measured streaming-read bandwidth (bench.py's calibration: ld_calib_stream_read
    over 1 GiB);
  * ms per step of the featureless 50-step DiT loop, parent commit and this commit (--parent DIR: a checkout of the parent commit
    with its library built; the legs are tools/edit_video_bench.py's `--leg featureless` children, alternated).

    python tools/conform_bench.py --parent /path/to/parent/checkout [--steps 50] [--repeats 2] [--out profiles/conform.txt]
"""
import argparse
import ctypes
import os
import socket
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def stream_read_gbs(torch, dev):
    """bench.py's calibration figure: a 16-byte-per-lane streaming read of 1 GiB, for about a second."""
    from landiff_amd import _lib
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.empty(1 << 28, device=dev, dtype=torch.int32).random_()
    sink = torch.zeros(4, device=dev, dtype=torch.int32)
    launch = lambda: _lib.check(lib.ld_calib_stream_read(ctypes.c_void_p(buf.data_ptr()), buf.numel() * 4, ctypes.c_void_p(sink.data_ptr()), st),
                                "ld_calib_stream_read")
    launch(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0, n = time.perf_counter(), 0
    e0.record()
    while time.perf_counter() - t0 < 1.0:
        for _ in range(4):
            launch()
        n += 4
        torch.cuda.synchronize()
    e1.record(); torch.cuda.synchronize()
    return buf.numel() * 4 / (e0.elapsed_time(e1) * 1e-3 / n) / 1e9


def events_ms(torch, fn, n):
    fn(); fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit, its library built")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=2, help="runs of each featureless leg")
    ap.add_argument("--launches", type=int, default=10, help="kernel launches between the two events")
    ap.add_argument("--small", action="store_true", help="quarter-size clips and the tiny DiT: a rehearsal of this script, not a measurement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "conform.txt"))
    a = ap.parse_args()
    root = os.path.dirname(HERE)
    a.parent = os.path.abspath(a.parent) if a.parent else None
    from edit_video_bench import child
    lines = ["The conform stage (landiff_amd/conform.py): input clips brought to 49 frames of 480 x 720 on the GPU."
             + ("  SMALL shapes (a rehearsal of the script: no figure below is a measurement)" if a.small else ""),
             "tools/conform_bench.py; all figures from one session on one box; the featureless legs are child processes, alternated.", ""]
    say = lambda s: (print(s, flush=True), lines.append(s))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    mean = lambda v: sum(v) / len(v)
    # ---- the featureless DiT loop, before this process opens the GPU: parent, this commit, parent, this commit, ...
    S = a.steps
    legs = {"parent commit": [], "this commit, no conform argument": []}
    for rep in range(a.repeats):
        for name, r_ in (("parent commit", a.parent), ("this commit, no conform argument", root)):
            if r_ is None:
                continue
            r = child(r_, S, a.small)
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
        t = [r["ms_per_step"] for r in legs["this commit, no conform argument"]]
        diff, spread = mean(t) - mean(p), max(max(p) - min(p), max(t) - min(t))
        say(f"  -> this commit - parent commit: {diff:+.2f} ms per step = {100 * diff / mean(p):+.2f} %; the larger of the two legs' own spreads: "
            f"{spread:.2f} ms = {100 * spread / mean(p):.2f} %; the difference lies {'inside' if abs(diff) <= spread else 'OUTSIDE'} it")
        say(f"  -> latent checksums equal across all legs: {len({r['checksum'] for rs in legs.values() for r in rs}) == 1}")
    else:
        say("(no --parent given: the parent commit was not measured)")
    say("")
    flush()
    # ---- this process: the conform stage
    import torch
    import torch.nn.functional as F
    from landiff_amd import ops
    from landiff_amd.conform import ConformConfig, _needed, conform_plan
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.set_num_threads(16)
    say(f"box: {socket.gethostname()}, {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; CPU legs with {torch.get_num_threads()} threads")
    gbs = stream_read_gbs(torch, dev)
    say(f"streaming-read bandwidth of this box (ld_calib_stream_read, 16 B per lane over 1 GiB, bench.py's calibration): {gbs:.0f} GB/s")
    say("")
    flush()
    q = 4 if a.small else 1
    n, H, W = 49, 480 // q, 720 // q
    g = torch.Generator().manual_seed(0)
    for title, shape, fps in ((f"184 frames of {1080 // q} x {1920 // q} at 30 fps", (184, 1080 // q, 1920 // q, 3), 30),
                              (f"49 frames of {2160 // q} x {3840 // q}, taken one to one", (49, 2160 // q, 3840 // q, 3), None)):
        clip = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        keep = torch.randint(0, 40, shape[:3], generator=g, dtype=torch.uint8)
        say(f"{title} ({clip.numel() / 1e6:.0f} MB on the host) -> {n} x {H} x {W}, fit=\"cover\"")
        for filt in ("bilinear", "bicubic"):
            plan = conform_plan(shape, n, H, W, ConformConfig(fit="cover", src_fps=fps, filter=filt))
            y0, x0, hc, wc = plan.box
            ups = []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sub, idx = _needed(clip, plan, dev)
                torch.cuda.synchronize()
                ups.append((time.perf_counter() - t0) * 1e3)
            run = lambda: ops.resize_u8(sub, (H, W), frame_idx=idx, box=plan.box, filter=filt)
            ms = events_ms(torch, run, a.launches)
            moved = n * hc * wc * 3 + n * H * W * 3
            floor_ms = moved / gbs / 1e6
            say(f"  {filt:8s}: box {plan.box}, scale {plan.scale_y:.3f}; host selection + upload of {sub.shape[0]} of {shape[0]} frames "
                f"({sub.numel() / 1e6:.0f} MB, pageable memory): {ups[0]:.1f} / {ups[1]:.1f} ms (two runs)")
            say(f"            ld_resize_u8: {ms:.3f} ms per launch ({a.launches} launches between two events); {moved / 1e6:.0f} MB read + written "
                f"-> {moved / ms / 1e6:.0f} GB/s = {100 * floor_ms / ms:.0f} % of the box's stream figure (bytes / bandwidth: {floor_ms:.3f} ms)")
            flush()
            if filt == "bilinear":
                sub_m, _ = _needed(keep, plan, dev)
                mrun = lambda: ops.resize_mask_u8(sub_m, (H, W), frame_idx=idx, box=plan.box, filter=filt)
                mms = events_ms(torch, mrun, a.launches)
                mmoved = n * hc * wc + n * H * W
                say(f"            ld_resize_mask_u8 (one byte per pixel): {mms:.3f} ms per launch; {mmoved / 1e6:.0f} MB -> {mmoved / mms / 1e6:.0f} GB/s "
                    f"(bytes / bandwidth: {mmoved / gbs / 1e6:.3f} ms)")
                del sub_m
            # the same frames and box through torch on the CPU: uint8 where this torch takes it (torchvision's path), else fp32
            src = clip[list(plan.frame_idx)][:, y0:y0 + hc, x0:x0 + wc].permute(0, 3, 1, 2)
            x = None
            for dtype in (torch.uint8, torch.float32):
                try:
                    x = src.to(dtype).contiguous(memory_format=torch.channels_last)
                    t0 = time.perf_counter()
                    F.interpolate(x, size=(H, W), mode=filt, antialias=True, align_corners=False)
                    cpu_ms = (time.perf_counter() - t0) * 1e3
                    t0 = time.perf_counter()
                    F.interpolate(x, size=(H, W), mode=filt, antialias=True, align_corners=False)
                    cpu_ms = min(cpu_ms, (time.perf_counter() - t0) * 1e3)
                    say(f"            F.interpolate(antialias=True) on the CPU, {str(dtype).split('.')[-1]} channels-last, {torch.get_num_threads()} threads, "
                        f"resampling alone (frames already cropped and gathered): {cpu_ms:.0f} ms (the faster of two) = {cpu_ms / ms:.0f} x the kernel")
                except (RuntimeError, NotImplementedError) as e:
                    say(f"            F.interpolate(antialias=True) on the CPU, {str(dtype).split('.')[-1]}: not supported by this torch ({str(e)[:60]})")
                flush()
            del sub, src, x
        del clip, keep
        say("")
    flush()


if __name__ == "__main__":
    main()
