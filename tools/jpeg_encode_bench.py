"""What the encode stage (landiff_amd/encode.py: ld_jpeg_encode_u8) costs at the sizes the pipeline delivers, one session on one
box -> profiles/jpeg_encode.txt.  For 49 frames of 480 x 720 x 3 and for the same clip retimed to 24 fps (145 frames) and 30 fps (181):

  * the kernels, warm, timed by HIP events in several windows with their spread: the coefficient kernel alone (ld_jpeg_coefs_u8),
    the entropy coder's two passes alone (ld_jpeg_entropy_i16 on those coefficients) and the whole encode (ld_jpeg_encode_u8: four
    launches); beside them the bytes that must move over the box's measured streaming-read bandwidth;
  * the device-to-host copy of the streams (and of the lengths before it);
  * end to end, frames on the device -> a Motion-JPEG AVI file: the host path (.cpu() of the frames, write_mjpeg_avi's PIL loop,
    16 threads available) against the device path (encode_jpeg, write_mjpeg_avi_encoded), interleaved, with the spread;
  * the file sizes of both, and the mean squared error of both against the frames.

    python tools/jpeg_encode_bench.py [--launches 10] [--windows 5] [--files 5] [--small] [--out profiles/jpeg_encode.txt]
"""
import argparse
import io
import os
import socket
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10, help="calls between the two events of a window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per figure (their spread is reported)")
    ap.add_argument("--files", type=int, default=5, help="files written per path and clip, the two paths alternating")
    ap.add_argument("--small", action="store_true", help="quarter-size frames: a rehearsal of this script, not a measurement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "jpeg_encode.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from conform_bench import stream_read_gbs
    from retime_bench import moving_clip
    from landiff.utils import write_mjpeg_avi, write_mjpeg_avi_encoded
    from landiff_amd import ops
    from landiff_amd.encode import JpegConfig, encode_jpeg, jpeg_header
    from landiff_amd.retime import RetimeConfig, retime_clip
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpeg_encode_bench.py measures on the GPU: no device found")
    lines = ["The encode stage (landiff_amd/encode.py): baseline JPEG of uint8 frames on the GPU, quality 95, 4:2:0, one restart interval per MCU row."
             + ("  SMALL shapes (a rehearsal of the script: no figure below is a measurement)" if a.small else ""),
             "tools/jpeg_encode_bench.py; all figures from one session on one box.", ""]
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
    cfg = JpegConfig()
    header_bytes = len(jpeg_header(H, W, cfg.quality, cfg.subsampling))

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

    def pil_bytes(img):
        buf = io.BytesIO()
        Image.fromarray(img, "RGB").save(buf, format="JPEG", quality=95)
        return buf.getvalue()

    tmp = tempfile.mkdtemp(prefix="ld_jpeg_bench_")
    for fps in (8, 24, 30):
        clip = base if fps == 8 else retime_clip(base, RetimeConfig(out_fps=fps))
        F = int(clip.shape[0])
        say(f"{F} frames of {H} x {W} x 3 ({clip.numel() / 1e6:.0f} MB) at {fps} fps" + ("" if fps == 8 else " (the 49 frames through the retime stage)"))
        # ---- kernels ----
        coefs = ops.jpeg_coefs_u8(clip, cfg.quality, cfg.subsampling)
        mcux = -(-W // 16)
        rows = coefs.view(-1, mcux * 6, 64)
        ms_c = windows(lambda: ops.jpeg_coefs_u8(clip, cfg.quality, cfg.subsampling))
        ms_e = windows(lambda: ops.jpeg_entropy_i16(rows, mcux, cfg.subsampling))
        ms_t = windows(lambda: ops.jpeg_encode_u8(clip, cfg.quality, cfg.subsampling))
        jpegs = encode_jpeg(clip, cfg)
        total = sum(len(j) for j in jpegs)
        # the pixels read once, the coefficients written once and read by both entropy passes, the streams written once
        moved = clip.numel() + 3 * coefs.numel() * 2 + total
        say(f"  ld_jpeg_coefs_u8 (pixels -> {coefs.numel() * 2 / 1e6:.0f} MB of coefficients): {fmt(ms_c)} per launch, {a.launches} launches a window")
        say(f"  ld_jpeg_entropy_i16 (the counting and the writing pass, segments into slots of the bound's size): {fmt(ms_e)} per call")
        say(f"  ld_jpeg_encode_u8 (coefficients, counting pass, layout, writing pass; incl. allocating its buffers): {fmt(ms_t)} per call")
        say(f"      bytes that must move (pixels read, coefficients written once and read twice, streams written): {moved / 1e6:.0f} MB -> "
            f"bytes / bandwidth = {moved / gbs / 1e6:.3f} ms = {100 * moved / gbs / 1e6 / (sum(ms_t) / len(ms_t)):.1f} % of the call")
        say(f"      stream buffer allocated by the bound (ld_jpeg_size; never cut to fit): {ops.jpeg_size(4, F, H, W, cfg.subsampling, header_bytes) / 1e6:.0f} MB, "
            f"of which {total / 1e6:.2f} MB are written")
        # ---- device to host ----
        buf, offs, lens = ops.jpeg_encode_u8(clip, cfg.quality, cfg.subsampling)
        torch.cuda.synchronize()
        d2h_small, d2h_big, d2h_frames = [], [], []
        for _ in range(a.windows):
            t0 = time.perf_counter(); table = torch.stack([offs, lens]).cpu(); t1 = time.perf_counter()
            n = int(table[0, -1] + table[1, -1])
            host = buf[:n].cpu(); t2 = time.perf_counter()
            raw = clip.cpu(); t3 = time.perf_counter()
            d2h_small.append(1e3 * (t1 - t0)); d2h_big.append(1e3 * (t2 - t1)); d2h_frames.append(1e3 * (t3 - t2))
        say(f"  device to host: the lengths {fmt(d2h_small)}; the streams ({n / 1e6:.2f} MB) {fmt(d2h_big)}; for comparison the raw frames "
            f"({clip.numel() / 1e6:.0f} MB, pageable) {fmt(d2h_frames)}")
        del host, raw
        # ---- end to end: frames on the device -> an AVI file ----
        host_s, dev_s = [], []
        for i in range(a.files):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            write_mjpeg_avi(clip.cpu().numpy(), os.path.join(tmp, "host.avi"), fps=fps)
            t1 = time.perf_counter()
            write_mjpeg_avi_encoded(encode_jpeg(clip, cfg), (W, H), os.path.join(tmp, "dev.avi"), fps=fps)
            t2 = time.perf_counter()
            host_s.append(t1 - t0); dev_s.append(t2 - t1)
        hs, ds = os.path.getsize(os.path.join(tmp, "host.avi")), os.path.getsize(os.path.join(tmp, "dev.avi"))
        say(f"  end to end, device frames -> AVI file, {a.files} files each, alternating:")
        say(f"      host path (.cpu() + PIL loop of write_mjpeg_avi): {fmt(host_s, 's')}; file {hs / 1e6:.2f} MB")
        say(f"      device path (encode_jpeg + write_mjpeg_avi_encoded): {fmt(dev_s, 's')}; file {ds / 1e6:.2f} MB = {100 * ds / hs:.1f} % of the host path's")
        say(f"      ratio of the means: {sum(host_s) / sum(dev_s):.1f} x")
        # ---- quality against PIL at the same setting, on a few frames ----
        pick = sorted({0, F // 2, F - 1})
        frames = clip[pick].cpu().numpy()
        mse = lambda x, y: float(((x.astype(np.float64) - y.astype(np.float64)) ** 2).mean())
        dec = lambda b: np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
        row = [(k, len(jpegs[k]), len(pil_bytes(f)), mse(dec(jpegs[k]), f), mse(dec(pil_bytes(f)), f)) for k, f in zip(pick, frames)]
        say("      frame: bytes here / PIL, mse here / PIL: " + "; ".join(f"{k}: {b} / {pb}, {m:.3f} / {pm:.3f}" for k, b, pb, m, pm in row))
        say("")
        flush()
        del clip, coefs, rows, buf
    say("Where the time goes inside the kernels was not profiled: no counter or trace run was made.  What is counted above: the bytes alone "
        "would take the stated share of a call.")
    flush()


if __name__ == "__main__":
    main()
