"""Times the frame-window attention launch (ld_attn_fwd_bf16_window) against the dense launch at the DiT's shape, and one full-size
denoiser step with the window off and on.  One box, one process: every form is warmed up, the forms are interleaved round by round
(the chip's clocks drift under its power cap: a form timed in a block of its own would be compared across that drift), device events
around every launch, medians reported next to the spread.  Writes profiles/attn_window.txt.

    python tools/attn_window_time.py [--rounds 15] [--step_rounds 5] [--no_step] [--out profiles/attn_window.txt]

Nothing here says anything about the quality of a trained checkpoint under a window: that is unmeasured.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, N, P, G = 2, 30, 17776, 226, 1350          # CFG pair, 30 heads, text 226 + 13 frames of 1350 tokens
WINDOWS = (0, 1, 2, 3, 12)


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--step_rounds", type=int, default=5)
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_window.txt"))
    a = ap.parse_args(argv)
    import torch
    from landiff_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("attn_window_time.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    last = lambda: (_lib.load().ld_attn_last_kernel() or b"").decode()
    n_tiles = -(-N // 64)
    dense_tiles = -(-N // 256) * n_tiles
    frac = {w: sum(ne for _, _, ne in ops.attn_window_check(N, P, G, w)) / dense_tiles for w in WINDOWS}

    # ---- the launch ----
    g = torch.Generator(device=dev).manual_seed(0)
    Npad = (N + 127) // 128 * 128
    q = torch.zeros(B, H, Npad, 64, device=dev, dtype=torch.bfloat16); k = torch.zeros_like(q)
    vt = torch.zeros(B, H, 64, Npad, device=dev, dtype=torch.bfloat16)
    q[:, :, :N] = torch.randn(B, H, N, 64, device=dev, generator=g).to(torch.bfloat16)
    k[:, :, :N] = torch.randn(B, H, N, 64, device=dev, generator=g).to(torch.bfloat16)
    vt[:, :, :, :N] = torch.randn(B, H, 64, N, device=dev, generator=g).to(torch.bfloat16)
    out = torch.zeros(B, N, H * 64, device=dev, dtype=torch.bfloat16)
    forms = [("dense", lambda: ops.attn_fwd(q, k, vt, out, N, N, 0.125))]
    for w in WINDOWS:
        forms.append((f"w={w}", lambda w=w: ops.attn_fwd_window(q, k, vt, out, N, 0.125, P, G, w)))
    kernels, fallbacks = {}, {}
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)
    for name, fn in forms:                          # warm-up: code objects, counter sets, clocks
        for _ in range(3):
            fn()
        kernels[name] = last()
        ops.attn_last_fallbacks(cnt)
        fallbacks[name] = int(cnt.item())
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in forms}
    for _ in range(a.rounds):
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    say(f"frame-window attention at B={B} H={H} N={N} (text {P} + 13 frames of {G}), {n_tiles} key tiles, {-(-N // 256)} query blocks per head")
    say(f"{a.rounds} interleaved rounds after 3 warm-up launches per form; device events around one launch; ms = median [min .. max]")
    say(f"{'form':6s} {'kernel':28s} {'tiles/dense':>11s} {'ms':>8s} {'[min .. max]':>20s} {'time/dense':>10s} {'time ratio / tile ratio':>24s} {'fallbacks':>9s}")
    d_med, d_min, d_max = stats(ms["dense"])
    for name, _ in forms:
        med, lo, hi = stats(ms[name])
        fr = 1.0 if name == "dense" else frac[int(name[2:])]
        say(f"{name:6s} {kernels[name]:28s} {fr:11.4f} {med:8.3f} {f'[{lo:.3f} .. {hi:.3f}]':>20s} {med / d_med:10.4f} {med / d_med / fr:24.3f} {fallbacks[name]:9d}")
    w12 = stats(ms["w=12"])[0]
    say(f"w=12 walks every tile: median {w12:.3f} ms vs dense {d_med:.3f} ms = {100 * (w12 / d_med - 1):+.2f} %; "
        f"run-to-run spread of the dense launch: [{d_min:.3f} .. {d_max:.3f}] = {100 * (d_max - d_min) / d_med:.2f} % of its median, "
        f"median absolute deviation {statistics.median(abs(x - d_med) for x in ms['dense']):.4f} ms")

    # ---- one full-size denoiser step ----
    if not a.no_step:
        del q, k, vt, out
        import time
        from landiff_amd.config import PipelineConfig
        from landiff_amd.dit import ControlDiTRunner
        from landiff_amd.weights import init_pipeline_state
        cfg = PipelineConfig.full().check()
        d = cfg.dit
        assert (d.seq_len, d.text_len, d.grid_h * d.grid_w) == (N, P, G)
        st = init_pipeline_state(cfg, seed=1234, dtype=torch.bfloat16, device=dev, parts=["dit_main", "dit_control"])
        x = torch.randn(1, d.latent_frames, d.in_channels, d.latent_h, d.latent_w, device=dev, generator=g)
        ctx = torch.randn(1, d.text_len, d.text_dim, device=dev, generator=g)
        sem = torch.randn(d.latent_frames, d.in_channels, d.latent_h, d.latent_w, device=dev, generator=g).to(torch.bfloat16)
        o = torch.empty_like(x)
        runs = []
        for w in (None, 1, 2):
            run = ControlDiTRunner(st["dit_main"], st["dit_control"], d, dev, **({} if w is None else {"attn_window": w}))
            run.set_condition(ctx, sem)
            for i in range(2):
                run.step(x, 500 - i, -0.7, 0.7, 6.0, o)
            runs.append(("off" if w is None else f"w={w}", run))
        torch.cuda.synchronize()
        sms = {name: [] for name, _ in runs}
        for r in range(a.step_rounds):
            for name, run in runs:
                t0 = time.perf_counter()
                run.step(x, 490 - r, -0.7, 0.7, 6.0, o)
                torch.cuda.synchronize()
                sms[name].append((time.perf_counter() - t0) * 1e3)
        say()
        say(f"one full-size denoiser step (control + main DiT, 45 layer calls, random weights), {a.step_rounds} interleaved rounds after 2 warm-up steps; "
            "host clock around step() + synchronise; ms = median [min .. max]")
        off = stats(sms["off"])[0]
        for name, _ in runs:
            med, lo, hi = stats(sms[name])
            say(f"window {name:4s}: {med:8.2f} [{lo:.2f} .. {hi:.2f}]   step time / window off = {med / off:.4f}")
    say()
    say("The effect of a window on a trained checkpoint's output is unmeasured.")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
