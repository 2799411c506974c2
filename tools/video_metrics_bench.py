"""What clip comparison (landiff_amd/metrics.py: ld_clip_diff_u8, ld_clip_ssim_u8) costs for a pair of 49 x 480 x 720 x 3 clips, one
session on one box -> profiles/video_metrics.txt:

  * each entry point (HIP events over repeated launches; ld_clip_diff_u8 = a clear + one kernel, ld_clip_ssim_u8 = the tile kernel +
    the sum kernel), for two random clips and for a clip against itself +-1, with and without a mask;
  * beside each: the two clips' bytes divided by the box's measured streaming-read bandwidth (bench.py's calibration:
    ld_calib_stream_read over 1 GiB), and the torch restatement of tests/metrics_ref.py on the CPU with 16 threads (int64 for the
    integer statistics, fp32 for SSIM);
  * the error table of the SSIM test: the fp32 restatement and the kernel against float64 on the cases of tests/test_gpu_metrics.py;
  * a mechanism demonstration: the tiny pipeline at random-init weights, exact against dit_cache, through LanDiffPipeline.compare.
    The figures of that leg say nothing about a trained checkpoint.

    python tools/video_metrics_bench.py [--launches 20] [--out profiles/video_metrics.txt]
    python tools/video_metrics_bench.py --kernels-only      (a few launches of each entry point and nothing else: the program a
                                                             kernel trace wraps, for the per-kernel split)
"""
import argparse
import os
import socket
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20, help="calls of an entry point between the two events")
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--small", action="store_true", help="5 frames of 120 x 180: a rehearsal of this script, not a measurement")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_metrics.txt"))
    a = ap.parse_args()
    import torch
    from conform_bench import events_ms, stream_read_gbs
    from landiff_amd import ops
    import metrics_ref as R
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU leg to fall back to"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.set_num_threads(16)
    F, H, W = (5, 120, 180) if a.small else (a.frames, 480, 720)
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8)
    near = (x.int() + torch.randint(0, 2, x.shape, generator=g).int() * 2 - 1).clamp(0, 255).to(torch.uint8)
    mask = torch.rand(F, H, W, generator=g) < 0.7
    xd, yd, nd, md = x.to(dev), y.to(dev), near.to(dev), mask.to(dev)
    legs = (("random against random", xd, yd, None), ("a clip against itself +-1", xd, nd, None), ("random against random, 70 % mask", xd, yd, md))
    if a.kernels_only:
        for _, p, q, m in legs:
            for _ in range(5):
                ops.clip_diff_u8(p, q, m)
                ops.clip_ssim_u8(p, q, m)
        torch.cuda.synchronize()
        print("kernels-only: 5 calls of each entry point per leg")
        return

    lines = [f"Clip comparison (landiff_amd/metrics.py): two uint8 clips of {F} x {H} x {W} x 3 compared on the GPU."
             + ("  SMALL shapes (a rehearsal of the script: no figure below is a measurement)" if a.small else ""),
             "tools/video_metrics_bench.py; all figures from one session on one box.", ""]
    say = lambda s: (print(s, flush=True), lines.append(s))

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    say(f"box: {socket.gethostname()}, {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; CPU legs with {torch.get_num_threads()} threads")
    gbs = stream_read_gbs(torch, dev)
    say(f"streaming-read bandwidth of this box (ld_calib_stream_read, 16 B per lane over 1 GiB, bench.py's calibration): {gbs:.0f} GB/s")
    nbytes = 2 * x.numel()
    floor_ms = nbytes / gbs / 1e6
    say(f"the two clips: {nbytes / 1e6:.0f} MB; bytes / bandwidth: {floor_ms:.3f} ms (a mask adds {mask.numel() / 1e6:.0f} MB)")
    say("")
    flush()
    times = {}
    for title, p, q, m in legs:
        d_ms = events_ms(torch, lambda: ops.clip_diff_u8(p, q, m), a.launches)
        s_ms = events_ms(torch, lambda: ops.clip_ssim_u8(p, q, m), a.launches)
        times[title] = (d_ms, s_ms)
        say(f"{title}:")
        say(f"  ld_clip_diff_u8: {d_ms:.3f} ms per call ({a.launches} calls between two events) = {nbytes / d_ms / 1e6:.0f} GB/s = "
            f"{100 * floor_ms / d_ms:.0f} % of the box's stream figure")
        say(f"  ld_clip_ssim_u8: {s_ms:.3f} ms per call = {nbytes / s_ms / 1e6:.0f} GB/s = {100 * floor_ms / s_ms:.1f} % of the box's stream figure "
            f"({s_ms / floor_ms:.0f} x bytes / bandwidth)")
        flush()
    say("")
    # ---- the CPU restatement, once each (the fp32 SSIM of a whole clip holds a few GB of intermediates)
    d_ms, s_ms = times["random against random"]
    t0 = time.perf_counter()
    want_d = R.diff_ref(x, y)
    cpu_d = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    want_s = R.ssim_ref32(x, y)
    cpu_s = (time.perf_counter() - t0) * 1e3
    say(f"torch on the CPU, {torch.get_num_threads()} threads, random against random (tests/metrics_ref.py, one run each):")
    say(f"  integer statistics in int64: {cpu_d:.0f} ms = {cpu_d / d_ms:.0f} x ld_clip_diff_u8")
    say(f"  SSIM in fp32 (the kernel's order of operations): {cpu_s:.0f} ms = {cpu_s / s_ms:.0f} x ld_clip_ssim_u8")
    got_d, got_s = ops.clip_diff_u8(xd, yd).cpu(), ops.clip_ssim_u8(xd, yd).cpu()
    say(f"  the kernels' results on that pair: integer statistics equal to int64 torch: {torch.equal(got_d, want_d)}; "
        f"largest |mean SSIM - fp32 restatement|: {float((R.mean_of(got_s) - R.mean_of(want_s)).abs().max()):.2e}")
    say("")
    flush()
    # ---- the error table of tests/test_gpu_metrics.py::test_clip_ssim_vs_float64
    import test_gpu_metrics as T
    cases, fam_err = T.build_ssim_cases()
    say("SSIM error against the float64 restatement, |mean - float64| per (frame, channel), the cases of tests/test_gpu_metrics.py")
    say("(largest over the masked and the unmasked call):")
    say(f"  {'shape':>12}  {'case':<14} {'fp32 restatement':>17} {'kernel':>11}")
    worst = {f: 0.0 for f in fam_err}
    for shape in T.SSIM_SHAPES:
        for name, fam in T.CASES.items():
            ref_e = kern_e = 0.0
            for masked in (False, True):
                p, q, mk, r64, err = cases[(shape, name, masked)]
                got = ops.clip_ssim_u8(p.to(dev), q.to(dev), None if mk is None else mk.to(dev)).cpu()
                counted = r64[..., 1] > 0
                if bool(counted.any()):
                    kern_e = max(kern_e, float((R.mean_of(got) - R.mean_of(r64))[counted].abs().max()))
                ref_e = max(ref_e, err)
            worst[fam] = max(worst[fam], kern_e)
            say(f"  {'x'.join(map(str, shape)):>12}  {name:<14} {ref_e:17.3e} {kern_e:11.3e}")
    say("  per family, largest:  " + ";  ".join(f"{f}: fp32 restatement {fam_err[f]:.1e}, kernel {worst[f]:.1e}, bound 4 x = {4 * fam_err[f]:.1e}" for f in fam_err))
    say("")
    flush()
    # ---- a mechanism demonstration
    from landiff_amd.config import PipelineConfig
    from landiff_amd.pipeline import LanDiffPipeline, synthetic_inputs
    from landiff_amd.weights import init_pipeline_state
    cfg = PipelineConfig.tiny(num_steps=6).check()
    st = init_pipeline_state(cfg, seed=1234)
    inp = synthetic_inputs(cfg, dev, n_text=6, seed=42)
    pipe = LanDiffPipeline(cfg, st, dev)
    exact = pipe(inp).clone()
    say("Mechanism demonstration -- the tiny configuration at RANDOM-INIT weights, 6 steps: these figures say nothing about a trained "
        "checkpoint or about the quality of any setting.")
    from landiff_amd.dit_cache import StepCacheConfig
    C_, S_ = True, False                                 # a step computed / skipped (its residual reused): forced plans, no threshold
    for name, dc in (("threshold 0.0 (every step computed)", 0.0), ("plan: step 4 of 6 skipped", StepCacheConfig(0.0, plan=(C_, C_, C_, C_, S_, C_))),
                     ("plan: steps 2, 4, 5 skipped", StepCacheConfig(0.0, plan=(C_, C_, S_, C_, S_, S_)))):
        other = LanDiffPipeline(cfg, st, dev, dit_cache=dc)(inp)
        m = pipe.compare(other, exact)
        say(f"  dit_cache {name}: PSNR {m.clip_psnr:.2f} dB, SSIM {m.clip_ssim:.6f}, {m.clip_differing} of {m.clip_counted} values differ, max |d| {m.clip_max_abs}")
    say(f"  LanDiffPipeline.compare on {tuple(exact.shape)}: {1e3 * pipe.timings['metrics'] / 3:.2f} ms per call, host divisions and the copy back included")
    flush()


if __name__ == "__main__":
    main()
