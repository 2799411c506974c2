"""What the decode stage (landiff_amd/decode.py: ld_jpeg_find_segments, ld_jpeg_decode_entropy, ld_jpeg_decode_rgb) costs at the sizes
the pipeline delivers, one session on one box -> profiles/jpeg_decode.txt.  For 49 frames of 480 x 720 written by encode_jpeg
(quality 95, 4:2:0, one restart interval per MCU row), the same clip retimed to 24 fps (145 frames) and 30 fps (181), and the 49
frames written by PIL (no restart markers: one lane per frame, the stated fallback):

  * each launch, warm, timed by HIP events in several windows with its spread; beside the sum the bytes that must move over the
    box's measured streaming-read bandwidth;
  * end to end, a Motion-JPEG AVI file -> frames on the device: the host path (read_mjpeg_avi's PIL loop + .to(device), what the
    parent commit does) against the device path (read_mjpeg_avi_chunks + decode_jpeg), interleaved, with the spread.

    python tools/jpeg_decode_bench.py [--launches 5] [--windows 5] [--files 5] [--small] [--out profiles/jpeg_decode.txt]
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


def stage_clip(chunks, dev):
    """What decode_jpeg hands the kernels for these streams (also tools/jpeg_sync_bench.py's staging) -> dict(infos, data, scan, ri,
    tables, tset, n_sets, rows, sub, seg, finfo, scan_bytes), the segment table already found."""
    import numpy as np
    import torch
    from landiff_amd import decode as D
    from landiff_amd import ops
    infos = [D.parse_jpeg(c) for c in chunks]
    starts = np.cumsum([0] + [len(c) for c in chunks[:-1]]).tolist()
    data = torch.frombuffer(bytearray(b"".join(chunks)), dtype=torch.uint8).to(dev)
    scan = torch.tensor([[s + i.scan_offset, len(c) - i.scan_offset] for s, i, c in zip(starts, infos, chunks)], dtype=torch.int64).to(dev)
    ri = torch.tensor([i.restart_interval for i in infos], dtype=torch.int32).to(dev)
    sets = {}
    tset_l = [sets.setdefault((i.quant, i.huffman), len(sets)) for i in infos]
    tables = torch.tensor([D.decode_tables(next(i for i, t in zip(infos, tset_l) if t == s)) for s in range(len(sets))], dtype=torch.int32).to(dev)
    tset = torch.tensor(tset_l, dtype=torch.int32).to(dev)
    rows, sub = max(i.segments for i in infos), infos[0].subsampling
    seg, finfo = ops.jpeg_find_segments(data, scan, ri, rows, infos[0].height, infos[0].width, sub)
    return dict(infos=infos, data=data, scan=scan, ri=ri, tables=tables, tset=tset, n_sets=len(sets), rows=rows, sub=sub, seg=seg, finfo=finfo,
                scan_bytes=sum(len(c) - i.scan_offset for c, i in zip(chunks, infos)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=5, help="calls between the two events of a window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per figure (their spread is reported)")
    ap.add_argument("--files", type=int, default=5, help="files read per path and clip, the two paths alternating")
    ap.add_argument("--small", action="store_true", help="quarter-size frames: a rehearsal of this script, not a measurement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "jpeg_decode.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from conform_bench import stream_read_gbs
    from retime_bench import moving_clip
    from landiff.utils import read_mjpeg_avi, read_mjpeg_avi_chunks, write_mjpeg_avi, write_mjpeg_avi_encoded
    from landiff_amd import decode as D
    from landiff_amd import ops
    from landiff_amd.encode import JpegConfig, encode_jpeg
    from landiff_amd.retime import RetimeConfig, retime_clip
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpeg_decode_bench.py measures on the GPU: no device found")
    lines = ["The decode stage (landiff_amd/decode.py): baseline JPEG streams -> uint8 frames on the GPU, equal to PIL's decode."
             + ("  SMALL shapes (a rehearsal of the script: no figure below is a measurement)" if a.small else ""),
             "tools/jpeg_decode_bench.py; all figures from one session on one box.", ""]
    say = lambda s: (print(s, flush=True), lines.append(s))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.set_num_threads(16)
    say(f"box: {socket.gethostname()}, {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; host legs with {torch.get_num_threads()} threads available")
    gbs = stream_read_gbs(torch, dev)
    say(f"streaming-read bandwidth of this box (ld_calib_stream_read, 16 B per lane over 1 GiB, bench.py's calibration): {gbs:.0f} GB/s")
    say("")
    flush()
    qd = 4 if a.small else 1
    H, W = 480 // qd, 720 // qd
    base = torch.from_numpy(moving_clip(np, 49, H, W)).to(dev)

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

    def fmt(ms, unit="ms"):
        mean = sum(ms) / len(ms)
        return (f"{mean:.3f} {unit} (mean of {len(ms)}; min {min(ms):.3f}, max {max(ms):.3f}, spread (max - min) "
                f"{max(ms) - min(ms):.3f} {unit} = {100 * (max(ms) - min(ms)) / mean:.1f} %)")

    tmp = tempfile.mkdtemp(prefix="ld_jpeg_dec_bench_")
    clips = [("encode_jpeg, 8 fps", 8, base, "gpu"), ("encode_jpeg, retimed to 24 fps", 24, retime_clip(base, RetimeConfig(out_fps=24)), "gpu"),
             ("encode_jpeg, retimed to 30 fps", 30, retime_clip(base, RetimeConfig(out_fps=30)), "gpu"),
             ("PIL (no restart markers: one lane per frame)", 8, base, "pil")]
    for name, fps, clip, writer in clips:
        F = int(clip.shape[0])
        path = os.path.join(tmp, "clip.avi")
        if writer == "gpu":
            write_mjpeg_avi_encoded(encode_jpeg(clip, JpegConfig()), (W, H), path, fps=fps)
        else:
            write_mjpeg_avi(clip.cpu().numpy(), path, fps=fps)
        chunks, _, _ = read_mjpeg_avi_chunks(path)
        st = stage_clip(chunks, dev)
        infos, data, scan, ri, tables, tset, rows, sub, seg, finfo = (st[k] for k in ("infos", "data", "scan", "ri", "tables", "tset", "rows", "sub", "seg", "finfo"))
        sets = range(st["n_sets"])
        total = sum(len(c) for c in chunks)
        say(f"{F} frames of {H} x {W} x 3 ({clip.numel() / 1e6:.0f} MB raw, {total / 1e6:.2f} MB of streams) written by {name}; "
            f"{infos[0].segments} segment(s) a frame")
        # ---- the launches, on what decode_jpeg hands them ----
        coefs, status = ops.jpeg_decode_entropy(data, seg, finfo, ri, tables, tset, H, W, sub)
        out = ops.jpeg_decode_rgb(coefs, tables, tset, H, W, sub)
        assert not bool(status.any()) and torch.equal(out.cpu(), torch.from_numpy(read_mjpeg_avi(path)[0]))
        ms_f = windows(lambda: ops.jpeg_find_segments(data, scan, ri, rows, H, W, sub))
        ms_e = windows(lambda: ops.jpeg_decode_entropy(data, seg, finfo, ri, tables, tset, H, W, sub))
        ms_r = windows(lambda: ops.jpeg_decode_rgb(coefs, tables, tset, H, W, sub, out=out))
        # streams read twice (markers, entropy), coefficients written and read, planes written and read, pixels written
        moved = 2 * total + 2 * coefs.numel() * 2 + 2 * F * ops.jpeg_dec_size(2, H, W, sub) + out.numel()
        mean = lambda ms: sum(ms) / len(ms)
        say(f"  ld_jpeg_find_segments ({len(sets)} table set(s), {rows} table rows): {fmt(ms_f)} per launch, {a.launches} launches a window")
        say(f"  ld_jpeg_decode_entropy (one lane per segment -> {coefs.numel() * 2 / 1e6:.0f} MB of coefficients): {fmt(ms_e)} per launch")
        say(f"  ld_jpeg_decode_rgb (inverse DCT into planes, then upsampling + colour: two launches): {fmt(ms_r)} per call")
        say(f"      sum of the means {mean(ms_f) + mean(ms_e) + mean(ms_r):.3f} ms; bytes that must move (streams read twice, coefficients and planes "
            f"written and read, pixels written): {moved / 1e6:.0f} MB -> bytes / bandwidth = {moved / gbs / 1e6:.3f} ms")
        # ---- end to end: an AVI file -> frames on the device ----
        host_s, dev_s = [], []
        for _ in range(a.files):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = torch.from_numpy(read_mjpeg_avi(path)[0]).to(dev)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            y = D.decode_jpeg(read_mjpeg_avi_chunks(path)[0], dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host_s.append(t1 - t0); dev_s.append(t2 - t1)
        assert torch.equal(x, y)
        say(f"  end to end, AVI file -> device frames, {a.files} reads each, alternating:")
        say(f"      host path (read_mjpeg_avi's PIL loop + .to(device)): {fmt(host_s, 's')}")
        say(f"      device path (read_mjpeg_avi_chunks + decode_jpeg: header parse, upload, four launches, the status copy): {fmt(dev_s, 's')}")
        say(f"      ratio of the means: {sum(host_s) / sum(dev_s):.2f} x")
        say("")
        flush()
        del data, coefs, out, x, y
    say("Where the time goes inside the kernels was not profiled: no counter or trace run was made.")
    flush()


if __name__ == "__main__":
    main()
