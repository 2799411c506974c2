"""Times the AR decode step of both batched engines on full-size random weights (24 layers, hidden 2048, MLP 11008), one process:
the MFMA engine (sample_many(engine="mfma"): ld_llm_decode_forward_wide + ld_llm_sample_advance_wide) at P = 1, 2, 4, 8, 12, 16 and
the GEMV engine at P = 1 (the path of sample(): ld_llm_decode_forward + ld_llm_sample_advance) and P = 4 (the _pairs entry points).
`--steps` decode steps centred on the mean KV length of a 13-frame decode after 64 text tokens (67 + 1244 / 2), device events after
a warm-up, median and min .. max of `--reps` runs.

Run:  python tools/llm_wide_time.py [--steps 300] [--reps 5] [--layers 24] [--out profiles/llm_wide_decode.txt]

It reports, it does not judge: for (mfma P = 4 vs gemv P = 4) and (mfma P = 16 vs 4 x gemv P = 4) the gap is printed next to the
run-to-run spread of both measurements; "faster" is said only where the gap exceeds the spread.
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MEAN_KV = 67 + 1244 // 2
ARMS = [("mfma", 1), ("mfma", 2), ("mfma", 4), ("mfma", 8), ("mfma", 12), ("mfma", 16), ("gemv", 1), ("gemv", 4)]


def time_steps(run, engine: str, P: int, steps: int, L0: int) -> float:
    """Seconds for `steps` decode steps of P samples starting at context length L0 (the KV rows below it hold what earlier
    timings left there: the kernels' time does not depend on the values)."""
    gens = [torch.Generator(device=run.dev).manual_seed(100 + p) for p in range(P)]
    run.out_count.zero_(); run.pos.fill_(L0 - 1); run._x_from_tail = True; run._mode = "chain"
    run.m_out_count.zero_(); run.m_pos.fill_(L0 - 1)
    run.m_attn_ws.zero_()                                          # (its counter words sit where another P's partial results were)
    wide = engine == "mfma"
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for it in range(steps):
        if P == 1 and not wide:
            run._pos_host = L0 - 1 + it
            run._decode_forward()
            run._sample_and_advance(True, 7.5, 1.0, gens[0])
        else:
            run._decode_forward_many(P, L0 - 1 + it, wide)
            run._sample_and_advance_many(gens, True, 7.5, 1.0, wide=wide)
    e1.record()
    torch.cuda.synchronize()
    run._pos_host = -1
    return e0.elapsed_time(e1) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "llm_wide_decode.txt"))
    a = ap.parse_args()
    from landiff_amd.config import LLMConfig
    from landiff_amd.llm import LLMRunner
    from landiff_amd.weights import init_state, llm_spec
    dev = torch.device("cuda:0")
    cfg = dataclasses.replace(LLMConfig(), num_layers=a.layers)
    run = LLMRunner(init_state(llm_spec(cfg), 9, dtype=torch.bfloat16, device=dev), cfg, dev, max_samples=4, wide_samples=16)
    L0 = MEAN_KV - a.steps // 2
    assert L0 > 1 and L0 + a.steps < run.Lmax and a.steps < run.Lmax
    run.forced.fill_(-1); run.allowed.zero_()                      # every position unrestricted and sampled
    g = torch.Generator(device=dev).manual_seed(1)
    for cache in run.kc_all + run.vc_all:
        for r in range(0, cache.shape[0], 2):                      # (pair by pair: a full-size cache is 11.5 GB)
            cache[r:r + 2, :L0 + a.steps + 1].copy_(torch.randn(2, L0 + a.steps + 1, *cache.shape[2:], device=dev, generator=g).to(cache.dtype))
    run.x.copy_(torch.randn(run.x.shape, device=dev, generator=g)); run.m_x.copy_(torch.randn(run.m_x.shape, device=dev, generator=g))
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: max(v) - min(v)
    times = {}
    for arm in ARMS:
        time_steps(run, *arm, 20, L0)                              # warm-up
        times[arm] = [time_steps(run, *arm, a.steps, L0) / a.steps for _ in range(a.reps)]
    t1 = med(times[("gemv", 1)])
    lines = [f"AR decode step, P samples of one prompt side by side, both engines ({cfg.num_layers} layers, hidden {cfg.hidden}, mlp {cfg.mlp}, "
             f"vocab {cfg.vocab}; KV length {L0} .. {L0 + a.steps}, {a.steps} steps per run, {a.reps} runs, device events, one process; "
             f"{torch.cuda.get_device_name(0)})",
             "gemv P = 1: ld_llm_decode_forward + ld_llm_sample_advance (the path of sample()); gemv P = 4: the _pairs entry points;",
             "mfma: ld_llm_decode_forward_wide (ld_gemv_wide, ld_llm_head_f32) + ld_llm_sample_advance_wide (sample_many(engine='mfma'))",
             "",
             "engine  P   step median us   min .. max us      step / step(gemv P=1)   tokens/s vs gemv P=1"]
    for arm in ARMS:
        t = med(times[arm])
        lines.append(f"{arm[0]:6s} {arm[1]:2d}   {t * 1e6:14.1f}   {min(times[arm]) * 1e6:.1f} .. {max(times[arm]) * 1e6:.1f}   "
                     f"{t / t1:20.3f}   {arm[1] * t1 / t:19.3f}")

    def compare(what, ta, sa, tb, sb, name_a, name_b):
        gap, sp = tb - ta, sa + sb
        verdict = (f"{name_a} is faster beyond the spread" if gap > sp else f"{name_b} is faster beyond the spread" if -gap > sp
                   else "no difference beyond the spread")
        return (f"{what}: {name_a} {ta * 1e6:.1f} us, {name_b} {tb * 1e6:.1f} us, gap {gap * 1e6:+.1f} us, run-to-run spread "
                f"(sum of both max - min) {sp * 1e6:.1f} us -> {verdict}")
    m4, g4, m16 = times[("mfma", 4)], times[("gemv", 4)], times[("mfma", 16)]
    lines += ["",
              compare("four samples per step", med(m4), spread(m4), med(g4), spread(g4), "mfma P = 4", "gemv P = 4"),
              compare("sixteen samples", med(m16), spread(m16), 4 * med(g4), 4 * spread(g4), "mfma P = 16", "4 x gemv P = 4")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
