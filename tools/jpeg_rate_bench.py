"""What rate control of the encode stage (landiff_amd/encode.py JpegRateConfig: ld_jpeg_encode_rate_u8) costs at the sizes
the pipeline delivers, one session on one box -> profiles/jpeg_rate.txt.  For 49 frames of 480 x 720 x 3 (tools/jpeg_encode_bench.py's
moving texture) and the same clip retimed to 24 fps (145 frames) and 30 fps (181), 4:2:0, ceiling 95:

  (a) off costs nothing: ld_jpeg_encode_u8 at quality 95 through this build and, with --parent_lib, through a library built from the
      parent commit, on the same buffers, the two alternating window by window, with their spreads;
  (b) the rate-controlled call in both modes at a budget of half the quality-95 size: the whole call, and per launch family -- the DCT
      (ld_jpeg_c8_u8) and the per-frame quantiser (ld_jpeg_quant_i16) timed alone, the final encode as quantiser + (a) - the coefficient
      kernel, the R trial rounds as the rest;
  (c) the same search on the host, the alternative a user has without it: .cpu() of the frames plus the same bisection over PIL's sizes.

    python tools/jpeg_rate_bench.py [--launches 5] [--windows 5] [--host_runs 1] [--parent_lib PATH] [--small] [--out profiles/jpeg_rate.txt]
"""
import argparse
import ctypes
import io
import os
import socket
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=5, help="calls between the two events of a window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per figure (their spread is reported)")
    ap.add_argument("--host_runs", type=int, default=1, help="runs of the host search per clip and mode")
    ap.add_argument("--parent_lib", default=None, help="liblandiff_hip.so built from the parent commit, for (a)")
    ap.add_argument("--small", action="store_true", help="quarter-size frames: a rehearsal of this script, not a measurement")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "jpeg_rate.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from retime_bench import moving_clip
    from landiff_amd import _lib, ops
    from landiff_amd.encode import (JpegConfig, JpegRateConfig, device_tables, encode_jpeg, jpeg_header, rate_rounds)
    from landiff_amd.retime import RetimeConfig, retime_clip
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpeg_rate_bench.py measures on the GPU: no device found")
    lines = ["Rate control of the encode stage (landiff_amd/encode.py JpegRateConfig, DESIGN 8.15): the quality searched on the GPU so that a frame "
             "or a clip fits a byte budget; 4:2:0, ceiling 95, floor 1."
             + ("  SMALL shapes (a rehearsal of the script: no figure below is a measurement)" if a.small else ""),
             "tools/jpeg_rate_bench.py; all figures from one session on one box.", ""]
    say = lambda s: (print(s, flush=True), lines.append(s))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.set_num_threads(16)
    say(f"box: {socket.gethostname()}, {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; host legs with {torch.get_num_threads()} threads available")
    say("")
    qd = 4 if a.small else 1
    H, W = 480 // qd, 720 // qd
    base = torch.from_numpy(moving_clip(np, 49, H, W)).to(dev)
    cfg = JpegConfig()
    R = rate_rounds(1, cfg.quality)
    here = _lib.load()
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        parent.ld_jpeg_encode_u8.argtypes = _lib.SIGNATURES["ld_jpeg_encode_u8"]
        parent.ld_jpeg_encode_u8.restype = ctypes.c_int
        parent.ld_version.restype = ctypes.c_int
        say(f"(a) compares this build (ABI {here.ld_version()}) with a library built from the parent commit (--parent_lib; ABI {parent.ld_version()}), both loaded in this process")
    else:
        say("(a) no --parent_lib was given: the parent commit's build is NOT measured in this file")
    say("")
    flush()

    def windows(fns):
        """Several callables, alternating window by window -> one list of per-call ms each."""
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

    mean = lambda v: sum(v) / len(v)

    def fmt(ms, unit="ms"):
        return (f"{mean(ms):.3f} {unit} (mean of {len(ms)}; min {min(ms):.3f}, max {max(ms):.3f}, spread (max - min) "
                f"{max(ms) - min(ms):.3f} {unit} = {100 * (max(ms) - min(ms)) / mean(ms):.1f} %)")

    def pil_size(img, q):
        buf = io.BytesIO()
        Image.fromarray(img, "RGB").save(buf, format="JPEG", quality=q)
        return buf.tell()

    def bisect(fits, q_min, q_max):
        lo, hi, q, n = q_min - 1, q_max + 1, q_max, 0
        while True:
            n += 1
            if fits(q):
                lo = q
            else:
                hi = q
            if hi - lo <= 1:
                return max(lo, q_min), n
            q = (lo + hi) // 2

    for fps in (8, 24, 30):
        clip = base if fps == 8 else retime_clip(base, RetimeConfig(out_fps=fps))
        F = int(clip.shape[0])
        say(f"{F} frames of {H} x {W} x 3 ({clip.numel() / 1e6:.0f} MB) at {fps} fps" + ("" if fps == 8 else " (the 49 frames through the retime stage)"))
        sizes95 = [len(j) for j in encode_jpeg(clip, cfg)]
        say(f"  at quality 95: {sum(sizes95) / 1e6:.2f} MB, {sum(sizes95) / F / 1e3:.1f} KB a frame (min {min(sizes95)}, max {max(sizes95)})")
        # ---- (a) the plain encode through both builds, on the same buffers ----
        header = torch.frombuffer(bytearray(jpeg_header(H, W, cfg.quality, cfg.subsampling)), dtype=torch.uint8).to(dev)
        cap = ops.jpeg_size(4, F, H, W, cfg.subsampling, header.numel())
        coefs = torch.empty(F, ops.jpeg_size(0, F, H, W, cfg.subsampling), 64, dtype=torch.int16, device=dev)
        seg_ws = torch.empty(2, F * ops.jpeg_size(1, F, H, W, cfg.subsampling), dtype=torch.int64, device=dev)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        table = torch.empty(2, F, dtype=torch.int64, device=dev)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def plain(lib):
            rc = lib.ld_jpeg_encode_u8(P(clip), clip.stride(0), clip.stride(1), P(device_tables(dev)), P(header), header.numel(), P(coefs), P(seg_ws),
                                       P(out), cap, P(table[0]), P(table[1]), F, H, W, 420, cfg.quality, stream())
            assert rc == 0, rc
        plain(here)
        want = table.cpu()
        want_bytes = out[:int(want[0, -1] + want[1, -1])].cpu()
        if parent is not None:
            out.zero_()
            plain(parent)
            got = table.cpu()
            assert torch.equal(got, want) and torch.equal(out[:int(got[0, -1] + got[1, -1])].cpu(), want_bytes), "the two builds write different bytes"
            ms_here, ms_parent = windows([lambda: plain(here), lambda: plain(parent)])
            say(f"  (a) ld_jpeg_encode_u8 at quality 95 on preallocated buffers (four launches), the same bytes from both builds:")
            say(f"      this build:   {fmt(ms_here)}")
            say(f"      parent build: {fmt(ms_parent)}")
            say(f"      difference of the means {mean(ms_here) - mean(ms_parent):+.4f} ms against spreads of {max(ms_here) - min(ms_here):.4f} / "
                f"{max(ms_parent) - min(ms_parent):.4f} ms")
        else:
            ms_here, = windows([lambda: plain(here)])
            say(f"  (a) ld_jpeg_encode_u8 at quality 95 on preallocated buffers (four launches), this build only: {fmt(ms_here)}")
        del out, want_bytes
        # ---- (b) the rate-controlled call ----
        ms_c, ms_c8 = windows([lambda: ops.jpeg_coefs_u8(clip, cfg.quality, cfg.subsampling), lambda: ops.jpeg_c8_u8(clip, cfg.subsampling)])
        c8 = ops.jpeg_c8_u8(clip, cfg.subsampling)
        qual = torch.full((F,), 50, dtype=torch.int32, device=dev)
        ms_q, = windows([lambda: ops.jpeg_quant_i16(c8, qual, cfg.subsampling)])
        del c8
        say(f"  (b) alone: ld_jpeg_coefs_u8 {fmt(ms_c)}; ld_jpeg_c8_u8 (the DCT, once per call) {fmt(ms_c8)}; ld_jpeg_quant_i16 (one launch) {fmt(ms_q)}")
        for mode, kw in (("frame", dict(frame_bytes=(sum(sizes95) // F) // 2)), ("clip", dict(clip_bytes=sum(sizes95) // 2))):
            rate = JpegRateConfig(**kw)
            jpegs, info = encode_jpeg(clip, cfg, rate=rate, return_rate=True)
            q = info["qualities"]
            used = [sum(1 for row in info["trials"] if row[f][0]) for f in range(F)]
            ms_r, = windows([lambda: ops.jpeg_encode_rate_u8(clip, cfg.quality, cfg.subsampling, q_min=1, **kw)])
            final = mean(ms_q) + mean(ms_here) - mean(ms_c)
            say(f"      {mode} mode, budget {rate.budget} bytes (half the quality-95 size): qualities min {min(q)} / mean {sum(q) / F:.1f} / max {max(q)}, "
                f"{sum(info['over_budget'])} frames over budget, trials a frame min {min(used)} / max {max(used)} of R = {R}; "
                f"result {sum(len(j) for j in jpegs) / 1e6:.2f} MB")
            say(f"        ld_jpeg_encode_rate_u8 (1 + 3 x {R} + 4 = {1 + 3 * R + 4} launches; incl. allocating its buffers): {fmt(ms_r)} per call "
                f"= {mean(ms_r) / mean(ms_here):.1f} x the plain encode of (a)")
            say(f"        by launch family (means): the DCT {mean(ms_c8):.3f} ms; the final encode {final:.3f} ms (quantiser + (a) - the coefficient kernel); "
                f"the {R} trial rounds {mean(ms_r) - mean(ms_c8) - final:.3f} ms by difference = {(mean(ms_r) - mean(ms_c8) - final) / R:.3f} ms a round")
            # ---- (c) the same search on the host ----
            host_s = []
            for _ in range(a.host_runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                imgs = clip.cpu().numpy()
                if mode == "frame":
                    res = [bisect(lambda t, im=im: pil_size(im, t) <= rate.budget, 1, cfg.quality) for im in imgs]
                    n_enc = sum(n for _, n in res)
                else:
                    _, n = bisect(lambda t: sum(pil_size(im, t) for im in imgs) <= rate.budget, 1, cfg.quality)
                    n_enc = n * F
                host_s.append(time.perf_counter() - t0)
            say(f"        (c) on the host: .cpu() + the same bisection over PIL's sizes ({n_enc} PIL encodes, one thread; the final streams are among them): "
                f"{fmt(host_s, 's') if len(host_s) > 1 else f'{host_s[0]:.3f} s (one run)'} = {1e3 * mean(host_s) / mean(ms_r):.0f} x the device call")
            flush()
        say("")
        flush()
        del clip, coefs
    say("Quantising inside the counting pass was not built, so there is one form of a trial in this file.  Where the time goes inside the kernels "
        "was not profiled: no counter or trace run was made.  What a budget does to a trained checkpoint's output is unmeasured.")
    flush()


if __name__ == "__main__":
    main()
