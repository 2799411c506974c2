"""Times token-sequence scoring on full-size random weights (24 layers, hidden 2048, MLP 11008, 13 frames after 64 text tokens):

  * one LLMRunner.score of a whole sequence (teacher forcing in one pass: bf16 GEMM blocks over every position, final LayerNorm,
    ld_llm_head_f32, one ld_llm_token_logprobs launch), and its head and log-probability launches on their own;
  * the decode step of sample() (P = 1) and sample_many() (P = 4) with and without the per-step ld_llm_token_logprobs launch of
    return_logprobs, in the same process, set up as tools/llm_multi_time.py sets its steps up.

Device events after a warm-up, median of `--reps` runs.  With the flag off the step is launch for launch the parent commit's; its
figures there are the P = 1 / P = 4 rows of profiles/llm_multi_decode.txt, quoted in the output (labelled as quoted from an earlier run:
run-to-run drift makes them no basis for an overhead of a few microseconds; the same-process on / off difference is).

Run:  python tools/llm_score_time.py [--steps 300] [--reps 5] [--layers 24] [--out profiles/llm_score.txt]
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN_KV = 67 + 1244 // 2


def time_steps(run, P: int, steps: int, L0: int, logprobs: bool) -> float:
    """Seconds for `steps` decode steps of P samples from context length L0, with or without the log-probability launch."""
    c = run.cfg
    gens = [torch.Generator(device=run.dev).manual_seed(100 + p) for p in range(P)]
    run.out_count.zero_(); run.pos.fill_(L0 - 1); run._x_from_tail = True; run._mode = "chain"
    run.m_out_count.zero_(); run.m_pos.fill_(L0 - 1)
    run.m_attn_ws.zero_()
    lp = torch.empty(steps, P, device=run.dev, dtype=torch.float32)
    pairs = run.m_logits[:2 * P].view(P, 2 * c.vocab)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for it in range(steps):
        if P == 1:
            run._pos_host = L0 - 1 + it
            run._decode_forward()
            run._sample_and_advance(True, 7.5, 1.0, gens[0])
            if logprobs:
                run._step_logprobs(run.logits[0:1], run.logits[1:2], run.sampled.view(1), run.pos, lp[it], True, 7.5, 1.0, None, None)
        else:
            run._decode_forward_many(P, L0 - 1 + it)
            run._sample_and_advance_many(gens, True, 7.5, 1.0)
            if logprobs:
                run._step_logprobs(pairs[:, :c.vocab], pairs[:, c.vocab:], run.m_sampled[:P], run.m_pos[:P], lp[it], True, 7.5, 1.0,
                                   None, None)
    e1.record()
    torch.cuda.synchronize()
    run._pos_host = -1
    assert torch.isfinite(lp).all() or not logprobs
    return e0.elapsed_time(e1) / 1e3


def timed(fn, reps: int) -> list:
    out = []
    for _ in range(reps + 1):                                      # the first run is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / 1e3)
    return out[1:]


def parent_rows() -> dict:
    """P -> step median us of profiles/llm_multi_decode.txt (measured on the parent commit)."""
    rows = {}
    try:
        with open(os.path.join(ROOT, "profiles", "llm_multi_decode.txt")) as f:
            for line in f:
                m = re.match(r"\s*([1-4])\s+([0-9.]+)\s", line)
                if m:
                    rows[int(m.group(1))] = float(m.group(2))
    except OSError:
        pass
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "llm_score.txt"))
    a = ap.parse_args()
    from landiff_amd import ops
    from landiff_amd.config import LLMConfig
    from landiff_amd.llm import LLMRunner, forced_token_schedule
    from landiff_amd.weights import init_state, llm_spec
    dev = torch.device("cuda:0")
    cfg = dataclasses.replace(LLMConfig(), num_layers=a.layers)
    run = LLMRunner(init_state(llm_spec(cfg), 9, dtype=torch.bfloat16, device=dev), cfg, dev, max_samples=4)
    med = lambda v: sorted(v)[len(v) // 2]
    g = torch.Generator(device=dev).manual_seed(1)

    # ---- one score of a 13-frame sequence after 64 text tokens ----
    n_text, nf = 64, 13
    full_len, forced, _, n_visual = forced_token_schedule(cfg, n_text + 3, nf)
    text = torch.randn(n_text, cfg.text_dim, device=dev, generator=g)
    ids = torch.randint(0, cfg.visual_vocab, (n_visual,), device=dev, generator=g)
    t_score = timed(lambda: run.score(text, ids, num_frames=nf, guidance_scale=7.5), a.reps)
    nr = full_len - 1 - (n_text + 3)
    lnf = torch.randn(2 * nr, cfg.hidden, device=dev, generator=g)
    logits = torch.empty(2 * nr, cfg.vocab, device=dev)
    t_head = timed(lambda: ops.llm_head_f32(lnf, run.head, logits), a.reps)
    lp, tgt = torch.empty(nr, device=dev), torch.randint(0, cfg.visual_vocab, (nr,), device=dev, generator=g)
    t_lp = timed(lambda: ops.llm_token_logprobs(logits[:nr], logits[nr:], tgt, lp, True, 7.5, 1.0, pos_bias=n_text + 3, allowed=run.allowed,
                                                forced=run.forced), a.reps)
    head_flop = 2.0 * 2 * nr * cfg.vocab * cfg.hidden

    # ---- the decode step with and without the log-probability launch ----
    L0 = MEAN_KV - a.steps // 2
    assert L0 > 1 and L0 + a.steps < run.Lmax
    run.forced.fill_(-1); run.allowed.zero_()
    for cache in run.kc_all + run.vc_all:
        cache.copy_(torch.randn(cache.shape, device=dev, generator=g).to(cache.dtype))
    run.x.copy_(torch.randn(run.x.shape, device=dev, generator=g)); run.m_x.copy_(torch.randn(run.m_x.shape, device=dev, generator=g))
    steps = {}
    for P in (1, 4):
        for flag in (False, True):
            time_steps(run, P, 20, L0, flag)
            steps[(P, flag)] = [time_steps(run, P, a.steps, L0, flag) / a.steps for _ in range(a.reps)]
    parent = parent_rows()
    us = lambda v: f"{med(v) * 1e6:9.1f}   {min(v) * 1e6:.1f} .. {max(v) * 1e6:.1f}"
    lines = [f"Token-sequence scoring ({cfg.num_layers} layers, hidden {cfg.hidden}, mlp {cfg.mlp}, vocab {cfg.vocab}; {a.reps} runs after a "
             f"warm-up, device events, medians; {torch.cuda.get_device_name(0)})",
             "",
             f"LLMRunner.score, {n_visual} ids ({nf} frames after {n_text} text tokens: {full_len - 1} positions x 2 rows, {nr} x 2 head rows)",
             "                                   median ms   min .. max ms",
             f" score (whole call)               {med(t_score) * 1e3:9.2f}   {min(t_score) * 1e3:.2f} .. {max(t_score) * 1e3:.2f}",
             f" ld_llm_head_f32 [{2 * nr} x {cfg.vocab} x {cfg.hidden}]  {med(t_head) * 1e3:9.3f}   {min(t_head) * 1e3:.3f} .. {max(t_head) * 1e3:.3f}"
             f"   ({head_flop / med(t_head) / 1e12:.1f} TFLOP/s fp32)",
             f" ld_llm_token_logprobs, {nr} rows    {med(t_lp) * 1e3:9.3f}   {min(t_lp) * 1e3:.3f} .. {max(t_lp) * 1e3:.3f}",
             "",
             f"AR decode step, KV length {L0} .. {L0 + a.steps}, {a.steps} steps per run",
             " P  return_logprobs   step median us   min .. max us    parent commit, QUOTED from an earlier run (profiles/llm_multi_decode.txt)"]
    for P in (1, 4):
        for flag in (False, True):
            lines.append(f" {P}  {'on ' if flag else 'off'}              {us(steps[(P, flag)])}"
                         + (f"    {parent[P]:.1f}" if not flag and P in parent else ""))
    for P in (1, 4):
        d = med(steps[(P, True)]) - med(steps[(P, False)])
        lines.append(f" P = {P}: the launch adds {d * 1e6:.1f} us to a step ({100 * d / med(steps[(P, False)]):.2f} %)")
    lines.append(" The overhead to rely on is the same-process on / off difference above.  The parent column comes from another process on "
                 "another day: it only shows that the flag-off step is the parent's step to within box-to-box drift.")
    out = "\n".join(lines) + "\n"
    print(out, end="")
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
