"""The decode stage's two entropy routes side by side (landiff_amd/decode.py): ld_jpeg_decode_entropy (one lane per
restart segment) against ld_jpeg_decode_entropy_sync (one lane per sub_bytes bytes of a segment), one session on one box ->
profiles/jpeg_decode_sync.txt.  tools/jpeg_decode_bench.py's clips: 49 frames of 480 x 720 written by PIL (no restart markers) and
the 49 / 145 / 181 frames written by encode_jpeg (one restart interval per MCU row):

  * the entropy decode of both routes, warm, timed by HIP events in windows that alternate between the routes, with the spread; the
    sync route at sub_bytes 128 / 256 / 512 with its rounds and fallbacks (the sum of its launches: one call);
  * end to end, a Motion-JPEG AVI file -> frames on the device: the host path, the device path by the segment route and by the sync
    route, after one discarded warm-up read, their order rotating from read to read;
  * the crossover that entropy="auto" needs: one noise frame coded by the restatement's coder (tests/jpeg_dec_ref.encode_coefs) at
    restart intervals from one MCU to none, sixteen copies a call, both routes.

    python tools/jpeg_sync_bench.py [--launches 5] [--windows 5] [--files 5] [--small] [--out profiles/jpeg_decode_sync.txt]
"""
import argparse
import os
import socket
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=5, help="calls between the two events of a window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per figure (their spread is reported)")
    ap.add_argument("--files", type=int, default=5, help="files read per path and clip, the paths alternating")
    ap.add_argument("--small", action="store_true", help="quarter-size frames: a rehearsal of this script, not a measurement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "jpeg_decode_sync.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import jpeg_dec_ref as dref
    import jpeg_ref as ref
    from jpeg_decode_bench import stage_clip
    from retime_bench import moving_clip
    from landiff.utils import read_mjpeg_avi, read_mjpeg_avi_chunks, write_mjpeg_avi, write_mjpeg_avi_encoded
    from landiff_amd import decode as D
    from landiff_amd import ops
    from landiff_amd.encode import JpegConfig, encode_jpeg
    from landiff_amd.retime import RetimeConfig, retime_clip
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpeg_sync_bench.py measures on the GPU: no device found")
    lines = ["The decode stage's entropy routes (landiff_amd/decode.py, DESIGN 8.14): one lane per restart segment against one lane per subsequence."
             + ("  SMALL shapes (a rehearsal of the script: no figure below is a measurement)" if a.small else ""),
             "tools/jpeg_sync_bench.py; all figures from one session on one box.", ""]
    say = lambda s: (print(s, flush=True), lines.append(s))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.set_num_threads(16)
    say(f"box: {socket.gethostname()}, {torch.cuda.get_device_name(dev)}; torch {torch.__version__}")
    say("")
    qd = 4 if a.small else 1
    H, W = 480 // qd, 720 // qd
    base = torch.from_numpy(moving_clip(np, 49, H, W)).to(dev)

    def windows(fns):
        """The functions' windows alternate: -> per function its ms per call, one figure a window."""
        for fn in fns:
            fn(); fn()
        torch.cuda.synchronize()
        ms = [[] for _ in fns]
        for _ in range(a.windows):
            for k, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record(); e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.launches)
        return ms

    def fmt(ms, unit="ms"):
        mean = sum(ms) / len(ms)
        return f"{mean:.3f} {unit} (mean of {len(ms)}; min {min(ms):.3f}, max {max(ms):.3f}, spread (max - min) {max(ms) - min(ms):.3f} {unit})"

    def stage(chunks):
        st = stage_clip(chunks, dev)
        i0 = st["infos"][0]
        return st["infos"], (st["data"], st["seg"], st["finfo"], st["ri"], st["tables"], st["tset"], i0.height, i0.width, i0.subsampling), st["scan_bytes"]

    def routes(args, scan_bytes, sizes):
        """Both routes on one segment table, interleaved -> (ms of the segment route, {B: (ms, rounds max, rounds mean, fallen)})."""
        c0, s0 = ops.jpeg_decode_entropy(*args)
        fns, facts = [lambda: ops.jpeg_decode_entropy(*args)], {}
        for B in sizes:
            c1, s1, info = ops.jpeg_decode_entropy_sync(*args, sub_bytes=B, scan_bytes=scan_bytes)
            assert torch.equal(c1, c0) and torch.equal(s1, s0) and not bool(s1.any())
            r = info[..., 0].float()
            facts[B] = (int(r.max()), float(r.mean()), int(info[..., 1].sum()))
            fns.append(lambda B=B: ops.jpeg_decode_entropy_sync(*args, sub_bytes=B, scan_bytes=scan_bytes))
        ms = windows(fns)
        return ms[0], {B: (ms[1 + k],) + facts[B] for k, B in enumerate(sizes)}

    tmp = tempfile.mkdtemp(prefix="ld_jpeg_sync_bench_")
    clips = [("PIL (no restart markers)", 8, base, "pil"), ("encode_jpeg, 8 fps", 8, base, "gpu"),
             ("encode_jpeg, retimed to 24 fps", 24, retime_clip(base, RetimeConfig(out_fps=24)), "gpu"),
             ("encode_jpeg, retimed to 30 fps", 30, retime_clip(base, RetimeConfig(out_fps=30)), "gpu")]
    for name, fps, clip, writer in clips:
        F = int(clip.shape[0])
        path = os.path.join(tmp, "clip.avi")
        if writer == "gpu":
            write_mjpeg_avi_encoded(encode_jpeg(clip, JpegConfig()), (W, H), path, fps=fps)
        else:
            write_mjpeg_avi(clip.cpu().numpy(), path, fps=fps)
        chunks, _, _ = read_mjpeg_avi_chunks(path)
        infos, args, scan_bytes = stage(chunks)
        say(f"{F} frames of {H} x {W} x 3 written by {name}: {sum(len(c) for c in chunks) / 1e6:.2f} MB of streams, {infos[0].segments} segment(s) a frame, "
            f"{scan_bytes / sum(i.segments for i in infos):.0f} bytes a segment on average; entropy=\"auto\" picks {D.entropy_route(infos, [len(c) for c in chunks])}")
        seg_ms, sync = routes(args, scan_bytes, (128, 256, 512))
        say(f"  ld_jpeg_decode_entropy (one lane per segment): {fmt(seg_ms)} per launch")
        for B, (ms, rmax, rmean, fallen) in sync.items():
            say(f"  ld_jpeg_decode_entropy_sync sub_bytes {B}, max_rounds 32 (all its launches): {fmt(ms)} per call; rounds max {rmax}, mean {rmean:.1f}; "
                f"{fallen} segment(s) fell back; {sum(seg_ms) / sum(ms):.2f} x the segment route")
        paths = [lambda: torch.from_numpy(read_mjpeg_avi(path)[0]).to(dev), lambda: D.decode_jpeg(read_mjpeg_avi_chunks(path)[0], dev),
                 lambda: D.decode_jpeg(read_mjpeg_avi_chunks(path)[0], dev, entropy="sync")]
        secs, got = [[], [], []], [None, None, None]
        for it in range(a.files + 1):              # read 0 warms every path up and is discarded; the order rotates with every read
            for k in [(it + d) % 3 for d in range(3)]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got[k] = paths[k]()
                torch.cuda.synchronize()
                if it:
                    secs[k].append(time.perf_counter() - t0)
        (host_s, seg_s, sync_s), (x, y, z) = secs, got
        assert torch.equal(x, y) and torch.equal(x, z)
        say(f"  end to end, AVI file -> device frames, {a.files} reads each after one discarded warm-up read, the order of the three paths rotating:")
        say(f"      host path (read_mjpeg_avi's PIL loop + .to(device)): {fmt(host_s, 's')}")
        say(f"      device path, entropy=\"segment\": {fmt(seg_s, 's')}; host / device {sum(host_s) / sum(seg_s):.2f} x")
        say(f"      device path, entropy=\"sync\" (sub_bytes 256): {fmt(sync_s, 's')}; host / device {sum(host_s) / sum(sync_s):.2f} x")
        say("")
        flush()
        del args, x, y, z
    # ---- the crossover: one frame's coefficients at restart intervals from one MCU to none ----
    frame = ref.picture("noise", H, W)
    coefs = ops.jpeg_coefs_u8(torch.from_numpy(np.stack([frame, frame])).to(dev), 95, "420")[0].cpu().numpy()
    mcus = len(coefs) // 6
    say(f"Crossover: one {H} x {W} noise frame (quality 95, 4:2:0, {mcus} MCUs) coded at restart interval ri, sixteen copies a call; sync at sub_bytes 256:")
    for ri in (1, 2, 5, 15, 45, 135, 450, 0):
        ri = min(ri, mcus - 1) if ri else 0
        jpeg = dref.encode_coefs(coefs, H, W, 95, "420", ri)
        infos, args, scan_bytes = stage([jpeg] * 16)
        seg_ms, sync = routes(args, scan_bytes, (256,))
        ms, rmax, rmean, fallen = sync[256]
        per = scan_bytes / sum(i.segments for i in infos)
        say(f"  ri {ri:4d}: {infos[0].segments:4d} segments a frame, {per:8.0f} bytes a segment = {per / 256:6.1f} subsequences; segment route "
            f"{sum(seg_ms) / len(seg_ms):7.3f} ms (spread {max(seg_ms) - min(seg_ms):.3f}), sync route {sum(ms) / len(ms):7.3f} ms (spread {max(ms) - min(ms):.3f}; "
            f"rounds max {rmax}, {fallen} fell back): segment / sync {sum(seg_ms) / sum(ms):.2f} x")
        flush()
    say("")
    say("Where the time goes inside the kernels was not profiled (no counter or trace run), and how real camera footage, rather than "
        "noise or a moving synthetic clip, converges was not measured.")
    flush()


if __name__ == "__main__":
    main()
