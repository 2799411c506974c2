"""Times the AR decode step for P = 1 .. 4 samples of one prompt on full-size random weights (24 layers, hidden 2048, MLP 11008):
P = 1 through the single-pair path sample() runs (LLMRunner._decode_forward + _sample_and_advance: ld_llm_decode_forward and
ld_llm_sample_advance), P = 2, 3, 4 through the batched one sample_many() runs (_decode_forward_many + _sample_and_advance_many:
ld_llm_decode_forward_pairs and ld_llm_sample_advance_pairs).  `--steps` decode steps centred on the mean KV length of a
13-frame decode after 64 text tokens (67 + 1244 / 2), device events after a warm-up, same process, median of `--reps` runs.

Run:  python tools/llm_multi_time.py [--steps 300] [--reps 5] [--layers 24] [--out profiles/llm_multi_decode.txt]
Kernel breakdown: rocprofv3 --kernel-trace --stats -- python tools/llm_multi_time.py --reps 1 --out /dev/null   (a run of its own)

The condition it checks (exit status 1 when it does not hold): one batched decode of four samples takes less time than four
single decodes, by more than the run-to-run spread of both measurements.
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MEAN_KV = 67 + 1244 // 2


def time_steps(run, P: int, steps: int, L0: int) -> float:
    """Seconds for `steps` decode steps of P samples starting at context length L0 (the KV rows below it hold what earlier
    timings left there: the kernels' time does not depend on the values)."""
    gens = [torch.Generator(device=run.dev).manual_seed(100 + p) for p in range(P)]
    run.out_count.zero_(); run.pos.fill_(L0 - 1); run._x_from_tail = True; run._mode = "chain"
    run.m_out_count.zero_(); run.m_pos.fill_(L0 - 1)
    run.m_attn_ws.zero_()                                          # (its counter words sit where another P's partial results were)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for it in range(steps):
        if P == 1:
            run._pos_host = L0 - 1 + it
            run._decode_forward()
            run._sample_and_advance(True, 7.5, 1.0, gens[0])
        else:
            run._decode_forward_many(P, L0 - 1 + it)
            run._sample_and_advance_many(gens, True, 7.5, 1.0)
    e1.record()
    torch.cuda.synchronize()
    run._pos_host = -1
    return e0.elapsed_time(e1) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "llm_multi_decode.txt"))
    a = ap.parse_args()
    from landiff_amd.config import LLMConfig
    from landiff_amd.llm import LLMRunner
    from landiff_amd.weights import init_state, llm_spec
    dev = torch.device("cuda:0")
    cfg = dataclasses.replace(LLMConfig(), num_layers=a.layers)
    run = LLMRunner(init_state(llm_spec(cfg), 9, dtype=torch.bfloat16, device=dev), cfg, dev, max_samples=4)
    L0 = MEAN_KV - a.steps // 2
    assert L0 > 1 and L0 + a.steps < run.Lmax and a.steps < run.Lmax
    run.forced.fill_(-1); run.allowed.zero_()                      # every position unrestricted and sampled
    g = torch.Generator(device=dev).manual_seed(1)
    for cache in run.kc_all + run.vc_all:
        cache.copy_(torch.randn(cache.shape, device=dev, generator=g).to(cache.dtype))
    run.x.copy_(torch.randn(run.x.shape, device=dev, generator=g)); run.m_x.copy_(torch.randn(run.m_x.shape, device=dev, generator=g))
    med = lambda v: sorted(v)[len(v) // 2]
    times = {}
    for P in (1, 2, 3, 4):
        time_steps(run, P, 20, L0)                                 # warm-up
        times[P] = [time_steps(run, P, a.steps, L0) / a.steps for _ in range(a.reps)]
    t1, t4 = med(times[1]), med(times[4])
    spread = 4 * (max(times[1]) - min(times[1])) + (max(times[4]) - min(times[4]))
    gap = 4 * t1 - t4
    ok = gap > spread
    lines = [f"AR decode step, P samples of one prompt side by side ({cfg.num_layers} layers, hidden {cfg.hidden}, mlp {cfg.mlp}, "
             f"vocab {cfg.vocab}; KV length {L0} .. {L0 + a.steps}, {a.steps} steps per run, {a.reps} runs, device events; "
             f"{torch.cuda.get_device_name(0)})",
             "P = 1: ld_llm_decode_forward + ld_llm_sample_advance (the path of sample()); P > 1: the _pairs entry points (sample_many())",
             "",
             " P   step median us   min .. max us    step / step(P=1)   tokens/s vs P=1"]
    for P in (1, 2, 3, 4):
        t = med(times[P])
        lines.append(f" {P}   {t * 1e6:14.1f}   {min(times[P]) * 1e6:.1f} .. {max(times[P]) * 1e6:.1f}   {t / t1:16.3f}   {P * t1 / t:15.3f}")
    lines += ["",
              f"four single decodes {4 * t1 * 1e6:.1f} us per step of four tokens, one batched decode {t4 * 1e6:.1f} us: gap {gap * 1e6:.1f} us, "
              f"run-to-run spread (4 x (max - min) of P = 1, plus (max - min) of P = 4) {spread * 1e6:.1f} us -> "
              + ("batched is faster beyond the spread" if ok else "NOT faster beyond the spread")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
