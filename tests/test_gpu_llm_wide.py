"""The MFMA engine of the batched AR decode: ld_gemv_wide, ld_llm_decode_forward_wide, ld_llm_sample_advance_wide,
LLMRunner.sample_many(engine="mfma"), LanDiffPipeline.generate_samples(engine="mfma").

An MFMA sums K in another order than the register GEMV, so nothing here is bit-identical to sample(seed=...).  What is tested is
the engine's own contract:

  * accuracy by the 2x-floor rule with ld_gemv itself as the floor (float64 reference on the bf16 operands);
  * batch invariance, torch.equal: a row's bits do not depend on B, on the row's index or on the other rows -- kernel, step, decode;
  * the ids of a free-running decode equal those of sample(seed) up to the first step at which the engines' logit difference
    decides a near-tie of the draw differently, and that flip passes the inequality of tests/flip_audit.py.

Reference: Semantic1DLM.sample (landiff/llm/models/lm_model.py:417-508) over the cached blocks
(landiff/llm/modules/transformer_blocks.py:128-236), once per seed."""
import dataclasses
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS = 1e-5

# (name, K, N, form).  K 2048 / 11008 are the decoder's (one slice / six slices of K, the last one short); K 256 is shorter than a
# workgroup's slice (most waves have no step) and N 515 ends in a partial 32-row tile; K 16 is one MFMA step, N 33 one row in the
# second tile.
GEMV_CASES = [
    ("qkv_norm", 2048, 6144, "norm"),
    ("wo_resid_inplace", 2048, 2048, "resid"),
    ("gated_gelu_norm", 2048, 11008, "gated_norm"),
    ("w2_resid", 11008, 2048, "resid"),
    ("short_k_norm_resid", 256, 515, "norm_resid"),
    ("one_step", 16, 33, "plain"),
]
_OPERANDS = {}


def _operands(name, K, N, form, dev):
    """Weights, 32 distinct activation rows, the B = 32 result and the float64 reference of a case: made once, then read only."""
    if name in _OPERANDS:
        return _OPERANDS[name]
    from landiff_amd import ops
    g = torch.Generator(device=dev).manual_seed(len(name) * 1000 + K)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(BF)
    o = dict(form=form, x=rnd(32, K), w=rnd(N, K, sc=K ** -0.5))
    if "gated" in form:
        o["w2"] = rnd(N, K, sc=K ** -0.5)
    if "norm" in form:
        o["norm_w"] = 1.0 + 0.1 * torch.randn(K, device=dev, generator=g)
    if "resid" in form:
        o["resid"] = rnd(32, N)
    # float64 on the bf16 operands; the normalised activations rounded to bf16 as the kernels round them
    xn = o["x"].float()
    if "norm_w" in o:
        xn = (xn * torch.rsqrt(xn.pow(2).mean(-1, keepdim=True) + EPS) * o["norm_w"]).to(BF).float()
    ref = xn.double() @ o["w"].double().t()
    if "w2" in o:
        u = 0.7978845608028654 * (ref + 0.044715 * ref ** 3)
        ref = 0.5 * ref * (1 + torch.tanh(u)) * (xn.double() @ o["w2"].double().t())
    if "resid" in o:
        ref = ref + o["resid"].double()
    o["ref"] = ref
    o["full"] = torch.full((32, N), float("nan"), device=dev, dtype=BF)
    _run(ops.gemv_wide, o, slice(0, 32), o["full"])
    torch.cuda.synchronize()
    _OPERANDS[name] = o
    return o


def _run(fn, o, rows, out):
    """fn = ops.gemv or ops.gemv_wide on activation rows `rows`, result into out[rows] (the residual forms run in place)."""
    kw = {}
    if "w2" in o:
        kw.update(w2=o["w2"], act="gelu_tanh")
    if "norm_w" in o:
        kw.update(norm_w=o["norm_w"], norm_eps=EPS)
    dst = out[rows]
    if "resid" in o:
        dst.copy_(o["resid"][rows])
        kw.update(resid=dst)                     # out == resid, as the decode's wo / w2 projections run
    fn(o["x"][rows], o["w"], dst, **kw)


@pytest.mark.parametrize("case", GEMV_CASES, ids=[c[0] for c in GEMV_CASES])
def test_gemv_wide_accuracy_by_the_gemv_floor(cuda, case):
    """err = max|got - ref| / max|ref| of ld_gemv_wide at B = 32 against float64, at most twice the same figure of ld_gemv on the
    same rows two at a time (the shipped kernel is the yardstick: no absolute constant)."""
    from landiff_amd import ops
    name, K, N, form = case
    o = _operands(name, K, N, form, cuda)
    floor_out = torch.full((32, N), float("nan"), device=cuda, dtype=BF)
    for p in range(16):
        _run(ops.gemv, o, slice(2 * p, 2 * p + 2), floor_out)
    torch.cuda.synchronize()
    assert torch.isfinite(o["full"].float()).all() and torch.isfinite(floor_out.float()).all()
    scale = o["ref"].abs().max()
    err = ((o["full"].double() - o["ref"]).abs().max() / scale).item()
    floor = ((floor_out.double() - o["ref"]).abs().max() / scale).item()
    print(f"ld_gemv_wide {name} K={K} N={N}: err {err:.3e}, ld_gemv floor {floor:.3e}")
    assert err <= 2 * floor, (name, err, floor)


@pytest.mark.parametrize("case", GEMV_CASES, ids=[c[0] for c in GEMV_CASES])
def test_gemv_wide_batch_invariance(cuda, case):
    """A row's bits at B = 2, 8, 18 and 32 and at another row index are those of the B = 32 launch; rows beyond B of a NaN-filled
    output stay NaN; two B = 32 launches are equal."""
    from landiff_amd import ops
    name, K, N, form = case
    o = _operands(name, K, N, form, cuda)
    full = o["full"]
    again = torch.full_like(full, float("nan"))
    _run(ops.gemv_wide, o, slice(0, 32), again)
    assert torch.equal(again, full), name
    for B in (2, 8, 18):
        out = torch.full_like(full, float("nan"))
        _run(ops.gemv_wide, o, slice(0, B), out)
        assert torch.equal(out[:B], full[:B]), (name, B)
        assert torch.isnan(out[B:].float()).all(), (name, B)                   # rows of other samples untouched
    for rows in (slice(30, 32), slice(4, 12), slice(14, 32)):                  # the same rows at another index of a smaller launch
        out = torch.full_like(full, float("nan"))
        _run(ops.gemv_wide, o, rows, out)
        assert torch.equal(out[rows], full[rows]), (name, rows)
        assert torch.isnan(out[:rows.start].float()).all(), (name, rows)
    assert not torch.equal(full[0:2], full[2:4])                               # distinct rows: an index mix-up would show


def _tiny_runner(dev, wide_samples, max_samples=1):
    from landiff_amd.config import LLMConfig
    from landiff_amd.llm import LLMRunner
    from landiff_amd.weights import init_state, llm_spec
    cfg = LLMConfig.tiny()
    return cfg, LLMRunner(init_state(llm_spec(cfg), 21, dtype=BF, device=dev), cfg, dev, max_text=16, max_frames=6,
                          max_samples=max_samples, wide_samples=wide_samples)


def test_decode_forward_wide_embeds_each_samples_token_and_rows_are_independent(cuda):
    """ld_llm_decode_forward_wide, tiny configuration, P = 5: given the embedding table and token [P] against x rows filled by
    hand; two samples with equal token and cache rows get equal logits rows, distinct ones different rows."""
    from landiff_amd import ops
    cfg, run = _tiny_runner(cuda, 5)
    P, pos_value = 5, 9
    g = torch.Generator(device=cuda).manual_seed(2)
    for cache in run.kc_all + run.vc_all:
        cache.copy_(torch.randn(cache.shape, device=cuda, generator=g).to(BF))
        cache[6:8].copy_(cache[2:4])                                           # sample 3 = sample 1: same cache rows ...
    run.m_token.copy_(torch.tensor([5, 70, 33, 70, 12], device=cuda))          # ... and the same token
    run.m_pos.fill_(pos_value)
    table = ops.llm_layer_table(run.blocks, run.kc, run.vc)
    caches0 = [c.clone() for c in run.kc_all + run.vc_all]
    logits = []
    for emb in (run.emb, None):
        for c, c0 in zip(run.kc_all + run.vc_all, caches0):
            c.copy_(c0)
        run.m_attn_ws.zero_()
        run.m_x.copy_(run.emb[run.m_token].to(BF).repeat_interleave(2, 0) if emb is None else torch.full_like(run.m_x, float("nan")))
        ops.llm_decode_forward_wide(table, emb, run.m_token, run.m_pos, run.m_x, run.m_qkv, run.m_att, run.m_gate, run.m_attn_ws, run.cos,
                                    run.sin, run.ln_w, run.ln_b, run.m_lnf, run.head, run.m_logits, cfg.heads, run.Lmax, run.nsplit,
                                    cfg.rms_eps, cfg.ln_eps, pos_value=pos_value)
        logits.append(run.m_logits.clone())
    assert torch.isfinite(logits[0]).all() and torch.equal(logits[0], logits[1])
    assert torch.equal(logits[0][2:4], logits[0][6:8])
    assert not torch.equal(logits[0][0:2], logits[0][2:4]) and not torch.equal(logits[0][2:4], logits[0][8:10])


def test_sample_advance_wide_equals_single_launches(cuda):
    """ld_llm_sample_advance_wide with P = 16 against sixteen ld_llm_sample_advance launches on separate state, at an unrestricted
    position (top-k and top-p on), a restricted one and a forced one: everything torch.equal."""
    from landiff_amd import ops
    P, V, D, n_out = 16, 2055, 256, 24
    g = torch.Generator(device=cuda).manual_seed(5)
    emb = torch.randn(V, D, device=cuda, generator=g)
    forced = torch.full((64,), -1, device=cuda, dtype=torch.int32)
    allowed = torch.zeros(64, 4, device=cuda, dtype=torch.int32)
    POS = {"unrestricted": 10, "restricted": 20, "forced": 30}
    allowed[21, 0] = 3; allowed[21, 1:4] = torch.tensor([2050, 7, 2052], dtype=torch.int32)
    forced[31] = 2051
    for kind, p0 in POS.items():
        logits = torch.randn(2 * P, V, device=cuda, generator=g) * 3
        noise = torch.empty(P, V, device=cuda).exponential_(1.0, generator=g)
        top = dict(top_k=50, top_p=0.9)
        count0 = (torch.arange(P, device=cuda, dtype=torch.int32) * 3) % 7
        single = []
        for p in range(P):
            st = dict(pos=torch.full((1,), p0, device=cuda, dtype=torch.int32), token=torch.zeros(1, device=cuda, dtype=torch.int64),
                      out=torch.full((n_out,), -7, device=cuda, dtype=torch.int64), count=count0[p:p + 1].clone(),
                      sampled=torch.zeros(1, device=cuda, dtype=torch.int64), x=torch.zeros(2, D, device=cuda, dtype=BF),
                      probs=torch.zeros(1, V, device=cuda), cfg=torch.zeros(1, V, device=cuda))
            ops.llm_sample_advance(logits[2 * p:2 * p + 2], st["probs"], st["cfg"], True, 7.5, 1.0, st["pos"], allowed, noise[p:p + 1],
                                   forced, st["token"], st["out"], st["count"], st["sampled"], emb, st["x"], **top)
            single.append(st)
        pos = torch.full((P,), p0, device=cuda, dtype=torch.int32)
        token = torch.zeros(P, device=cuda, dtype=torch.int64)
        out = torch.full((P, n_out), -7, device=cuda, dtype=torch.int64)
        count, sampled = count0.clone(), torch.zeros(P, device=cuda, dtype=torch.int64)
        x = torch.zeros(2 * P, D, device=cuda, dtype=BF)
        probs, cfg = torch.zeros(P, V, device=cuda), torch.zeros(P, V, device=cuda)
        ops.llm_sample_advance_wide(logits, probs, cfg, True, 7.5, 1.0, pos, allowed, noise, forced, token, out, count, sampled, emb, x, **top)
        torch.cuda.synchronize()
        for p, st in enumerate(single):
            assert torch.equal(token[p:p + 1], st["token"]), (kind, p)
            assert torch.equal(out[p], st["out"]) and torch.equal(count[p:p + 1], st["count"]), (kind, p)
            assert torch.equal(sampled[p:p + 1], st["sampled"]) and torch.equal(pos[p:p + 1], st["pos"]), (kind, p)
            assert torch.equal(probs[p:p + 1], st["probs"]) and torch.equal(cfg[p:p + 1], st["cfg"]), (kind, p)
            assert torch.equal(x[2 * p:2 * p + 2], st["x"]), (kind, p)
        assert pos.tolist() == [p0 + 1] * P
        if kind == "forced":
            assert token.tolist() == [2051] * P and torch.equal(count, count0)
        else:
            assert torch.equal(count, count0 + 1)
        if kind == "unrestricted":
            assert len(set(token.tolist())) > 1, token.tolist()
        if kind == "restricted":
            assert set(token.tolist()) <= {2050, 7, 2052}


def _check_invariance(run, text, seeds, singles, **kw):
    """Row i of sample_many(engine="mfma") == the P = 1 call with that seed (seeds[j] for j in singles) == its row in the reversed
    seed list; the rows differ from one another."""
    many = run.sample_many(text, seeds, engine="mfma", **kw).clone()
    rev = run.sample_many(text, seeds[::-1], engine="mfma", **kw).clone()
    assert many.dtype == torch.int64 and many.shape[0] == len(seeds)
    for i in range(len(seeds)):
        assert torch.equal(many[i], rev[len(seeds) - 1 - i]), (i, seeds[i])
    for i in singles:
        one = run.sample_many(text, [seeds[i]], engine="mfma", **kw)
        assert one.shape == (1, many.shape[1]) and torch.equal(one[0], many[i]), (i, seeds[i], (one[0] != many[i]).nonzero()[:4].flatten().tolist())
    for i in range(1, len(seeds)):
        assert not torch.equal(many[0], many[i]), "the samples must differ, or the comparison shows nothing"
    return many


def test_sample_many_mfma_tiny_batch_invariance(cuda):
    """LLMConfig.tiny(), 16 seeds: guided, unguided, top-k / top-p, first_frame_tokens, a multi-segment decode with prefix_tokens;
    return_logprobs leaves the ids unchanged and is finite at the sampled positions."""
    cfg, run = _tiny_runner(cuda, 16)
    text = torch.randn(5, cfg.text_dim, generator=torch.Generator().manual_seed(3)).to(cuda)
    seeds = list(range(11, 27))
    every = range(16)
    many = _check_invariance(run, text, seeds, every, num_frames=3, guidance_scale=7.5)
    _check_invariance(run, text, seeds, (0, 7, 15), num_frames=3, guidance_scale=0.0)
    _check_invariance(run, text, seeds, (0, 7, 15), num_frames=3, guidance_scale=7.5, top_k=20, top_p=0.9)
    first = torch.arange(cfg.iframe_len, dtype=torch.int64) * 7 % cfg.visual_vocab
    ff = _check_invariance(run, text, seeds, (0, 7, 15), num_frames=3, guidance_scale=7.5, first_frame_tokens=first)
    assert torch.equal(ff[:, :cfg.iframe_len].cpu(), first[None].expand(16, -1))
    seg = torch.arange(cfg.iframe_len + 2 * cfg.pframe_len, dtype=torch.int64) * 5 % cfg.visual_vocab
    _check_invariance(run, text, seeds, (0, 7, 15), num_frames=6, guidance_scale=7.5, prefix_tokens=seg)
    ids, lp = run.sample_many(text, seeds, engine="mfma", num_frames=3, guidance_scale=7.5, return_logprobs=True)
    assert torch.equal(ids, many) and lp.shape == (16, many.shape[1]) and torch.isfinite(lp).all() and (lp <= 0).all()
    # the GEMV engine on the same runner is untouched by the wide buffers: sample_many(P = 1) is sample()
    assert torch.equal(run.sample_many(text, [11], num_frames=3)[0], run.sample(text, seed=11, num_frames=3))


_FULL = {}


def _full_width_runner(dev):
    """The configuration of test_sample_many_full_width_two_layers: hidden 2048, 16 heads, MLP 11008, vocabulary 2055, 2 layers, frame
    lengths shrunk to full_len ~284, nsplit 8; built once for the tests that need it."""
    if not _FULL:
        from landiff_amd.config import LLMConfig
        from landiff_amd.llm import LLMRunner, forced_token_schedule
        from landiff_amd.weights import init_state, llm_spec
        cfg = dataclasses.replace(LLMConfig(), num_layers=2, iframe_len=60, pframe_len=20, segment_length=8, segment_stride=8)
        full_len = forced_token_schedule(cfg, 64 + 3, 8)[0]
        assert 250 <= full_len <= 320
        run = LLMRunner(init_state(llm_spec(cfg), 9, dtype=BF, device=dev), cfg, dev, max_frames=8, wide_samples=16)
        assert run.nsplit == 8
        _FULL.update(cfg=cfg, run=run, text=torch.randn(64, cfg.text_dim, generator=torch.Generator().manual_seed(12)).to(dev))
    return _FULL["cfg"], _FULL["run"], _FULL["text"]


def test_sample_many_mfma_full_width_batch_invariance(cuda):
    """Full width, P = 16 against P = 1 for three of the seeds (one slice and six slices of K, every split count of the attention)."""
    cfg, run, text = _full_width_runner(cuda)
    seeds = list(range(42, 58))
    many = run.sample_many(text, seeds, engine="mfma", num_frames=8, guidance_scale=7.5).clone()
    for i in (0, 1, 15):
        one = run.sample_many(text, [seeds[i]], engine="mfma", num_frames=8, guidance_scale=7.5)
        assert torch.equal(one[0], many[i]), (i, (one[0] != many[i]).nonzero()[:4].flatten().tolist())
    assert not torch.equal(many[0], many[1]) and not torch.equal(many[0], many[15])


def test_mfma_two_blocks_full_width_teacher_fed_vs_oracle(cuda, oracle_bg):
    """The inputs and the oracle jobs of test_llm_two_blocks_full_width_decode_at_real_context_lengths_vs_oracle, decoded by
    sample_many(engine="mfma", teacher_fed=fed) at P = 16: every row's CFG logits equal row 0's at every step, and row 0 meets that
    test's condition at its check_it: err < max(2 * floor, 2e-2)."""
    from landiff_amd.llm import LLMRunner
    from oracle_jobs import llm_two_blocks_inputs
    cfg, sd, text, fed, S, full_len, steps, check_it = llm_two_blocks_inputs()
    run = LLMRunner({k: v.to(cuda) for k, v in sd.items()}, cfg, cuda, wide_samples=16)
    log = []
    run.sample_many(text.to(cuda), list(range(42, 58)), engine="mfma", guidance_scale=7.5, motion_score=0.1, logits_log=log,
                    teacher_fed=fed.to(cuda))
    dev = torch.stack(log, 0)                                          # [1 + steps, 16, vocab]: prefill, then one entry per decode step
    assert dev.shape[:2] == (steps + 1, 16) and steps >= 1240, (dev.shape, steps)
    for p in range(1, 16):
        assert torch.equal(dev[:, p], dev[:, 0]), (p, (dev[:, p] != dev[:, 0]).any(-1).nonzero()[:4].flatten().tolist())
    dev = dev[:, 0].cpu()
    ref32, _ = oracle_bg.result("llm_two_blocks_fp32")
    ref16, _ = oracle_bg.result("llm_two_blocks_bf16")
    rel = lambda a, b: ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()
    rows = []
    for it in check_it:
        err, floor = rel(dev[it + 1:it + 2], ref32[it]), rel(ref16[it], ref32[it])
        rows.append((S + 2 + it, err, floor))
    print("2-block full-width decode on the MFMA engine, CFG logits vs fp32 oracle (KV length: err / bf16-oracle floor): "
          + ", ".join(f"{L}: {e:.4f} / {f:.4f}" for L, e, f in rows))
    for L, err, floor in rows:
        assert err < max(2 * floor, 2e-2), (L, err, floor)


def _audit_against_gemv(run, cfg, text, seeds, num_frames, label):
    """Free-running decode of both engines per seed: step 0 (the shared prefill) is identical; the ids are equal up to the first
    differing step t, where the flip must be a near-tie by the inequality of tests/flip_audit.py; nothing after t is compared."""
    from landiff_amd.llm import forced_token_schedule
    T, scale = 1.0, 7.5
    S = text.shape[0] + 3
    full_len, forced, restricted, _ = forced_token_schedule(cfg, S, num_frames)
    positions = list(range(S + 1, full_len))                           # log entry k = the step that generates position S + 1 + k
    wide_log = []
    wide = run.sample_many(text, seeds, engine="mfma", num_frames=num_frames, guidance_scale=scale, temperature=T, logits_log=wide_log)
    wide_log = torch.stack(wide_log, 0).cpu()                          # [steps, P, V]
    report = []
    for i, s in enumerate(seeds):
        g_log = []
        ids_g = run.sample(text, seed=s, num_frames=num_frames, guidance_scale=scale, temperature=T, logits_log=g_log).cpu()
        g_log = torch.cat(g_log, 0).cpu()                              # [steps, V]
        assert g_log.shape[0] == len(positions) == wide_log.shape[0]
        ids_w = wide[i].cpu()
        assert torch.equal(wide_log[0, i], g_log[0]), (label, s)       # the shared prefill: not a vacuous comparison
        assert ids_w[0] == ids_g[0], (label, s)
        # walk the steps: k-th free position <-> k-th id
        free = [k for k, q in enumerate(positions) if q not in forced]
        assert len(free) == ids_g.numel() == ids_w.numel()
        t = next((j for j in range(len(free)) if ids_g[j] != ids_w[j]), None)
        if t is None:
            report.append(f"seed {s}: {len(free)} draws compared, 0 flips")
            continue
        assert torch.equal(ids_g[:t], ids_w[:t])
        k = free[t]
        q_pos = positions[k]
        gen = torch.Generator(device=run.dev).manual_seed(s)           # the sample's noise rows: one [vocab] Exp(1) draw per step
        noise = torch.empty(1, cfg.vocab, device=run.dev, dtype=torch.float32)
        for _ in range(k + 1):
            noise.exponential_(1.0, generator=gen)
        q = noise[0].double().cpu()
        b, a = int(ids_g[t]), int(ids_w[t])
        if q_pos in restricted:
            assert a in restricted[q_pos] and b in restricted[q_pos], (label, s, q_pos, a, b)
        lg = g_log[k].double()
        eps = float((wide_log[k, i].double() - lg).abs().max())
        margin = float((lg[b] - lg[a]) / T - (torch.log(q[b]) - torch.log(q[a])))
        bound = 2.0 * eps / T * (1 + 1e-3) + 1e-5
        report.append(f"seed {s}: {t} draws equal, first flip at draw {t} (position {q_pos}): gemv id {b}, mfma id {a}, margin {margin:.5f}, "
                      f"bound {bound:.5f} (eps {eps:.5f})")
        assert -1e-9 <= margin <= bound, (label, s, t, a, b, margin, bound)
    print(f"mfma vs gemv engine, free-running, {label}: " + "; ".join(report))


def test_mfma_ids_match_gemv_engine_up_to_audited_flips_tiny(cuda):
    cfg, run = _tiny_runner(cuda, 4)
    text = torch.randn(5, cfg.text_dim, generator=torch.Generator().manual_seed(3)).to(cuda)
    _audit_against_gemv(run, cfg, text, [11, 12, 13, 14], 6, "tiny")


def test_mfma_ids_match_gemv_engine_up_to_audited_flips_full_width(cuda):
    cfg, run, text = _full_width_runner(cuda)
    _audit_against_gemv(run, cfg, text, [42, 43, 44, 45], 8, "full width, 2 layers")


def test_generate_samples_mfma_tiny_pipeline(cuda):
    """LanDiffPipeline(wide_samples=6).generate_samples(inp, 6 seeds, engine="mfma"): six distinct uint8 videos, candidate i the
    one-seed call; keep=2 returns the two best by score in rank order and last_candidates holds all six."""
    from landiff_amd.config import PipelineConfig
    from landiff_amd.pipeline import LanDiffPipeline, rank_candidates, synthetic_inputs
    from landiff_amd.weights import init_pipeline_state
    cfg = PipelineConfig.tiny(num_steps=2).check()
    pipe = LanDiffPipeline(cfg, init_pipeline_state(cfg, seed=1234), cuda, wide_samples=6)
    inp = synthetic_inputs(cfg, cuda, n_text=6, seed=42)
    seeds = [42, 77, 78, 79, 80, 81]
    many = [v.clone() for v in pipe.generate_samples(inp, seeds, engine="mfma")]
    assert len(many) == 6 and all(v.dtype == torch.uint8 for v in many)
    for i in (0, 3, 5):
        one = pipe.generate_samples(inp, [seeds[i]], engine="mfma")
        assert len(one) == 1 and torch.equal(one[0], many[i]), i
    for i in range(6):
        for j in range(i + 1, 6):
            assert not torch.equal(many[i], many[j]), (i, j)
    best = pipe.generate_samples(inp, seeds, keep=2, engine="mfma")
    cand = pipe.last_candidates
    assert cand["seeds"] == seeds and cand["tokens"].shape[0] == 6 and len(cand["scores"]) == 6
    order = rank_candidates(cand["scores"])
    assert cand["order"] == order and len(best) == 2
    for (seed, score, frames), i in zip(best, order[:2]):
        assert seed == seeds[i] and score == cand["scores"][i] and torch.equal(frames, many[i])
    assert best[0][1] >= best[1][1]
