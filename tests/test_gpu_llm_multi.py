"""Batched AR decode: P samples of one prompt from one weight stream (ld_gemv_pairs, ld_llm_sample_advance_pairs,
ld_llm_decode_forward_pairs, LLMRunner.sample_many, LanDiffPipeline.generate_samples).

The claim under test is exactness: sample p of a batched decode is, bit for bit, what the single decode gives for its seed.  So
every comparison here is torch.equal against the single-pair path of the same build -- no tolerance anywhere:

  * ld_gemv_pairs, each pair against ld_gemv at B = 2, in every form the decode uses;
  * the key-split attention at B = 8 against four B = 2 launches, across both thresholds of the split rule;
  * ld_llm_sample_advance_pairs against single launches on separate state;
  * sample_many against sample(seed=...) on the tiny configuration and at full width, and the tiny pipeline end to end.

Reference: Semantic1DLM.sample (landiff/llm/models/lm_model.py:417-508) over the cached blocks
(landiff/llm/modules/transformer_blocks.py:128-236), once per seed."""
import dataclasses
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# (name, K, N, form).  K 2048 / 11008 are the decoder's; N 2055 is no multiple of any rows-per-batch; K 256 leaves most of a
# thread row of chunks empty (32 of 256 chunks) and N 515 ends in a partial batch of rows.
GEMV_CASES = [
    ("qkv_norm", 2048, 6144, "norm"),
    ("wo_resid_inplace", 2048, 2048, "resid"),
    ("gated_gelu_norm", 2048, 11008, "gated"),
    ("w2_resid_j6", 11008, 2048, "resid"),
    ("head_f32", 2048, 2055, "head"),
    ("short_k_norm_resid", 256, 515, "norm_resid"),
]
_GEMV_OPERANDS = {}


def _gemv_operands(name, K, N, form, dev):
    """Weights, 8 distinct activation rows and the per-pair ld_gemv reference of a case: made once, shared by P = 1..4."""
    if name in _GEMV_OPERANDS:
        return _GEMV_OPERANDS[name]
    from landiff_amd import ops
    g = torch.Generator(device=dev).manual_seed(len(name) * 1000 + K)
    rnd = lambda *s, dt=BF, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(dt)
    o = dict(form=form)
    if form == "head":
        o["x"], o["w"] = rnd(8, K, dt=torch.float32), rnd(N, K, dt=torch.float32, sc=K ** -0.5)
    else:
        o["x"], o["w"] = rnd(8, K), rnd(N, K, sc=K ** -0.5)
    if form == "gated":
        o["w2"] = rnd(N, K, sc=K ** -0.5)
    if "norm" in form or form == "gated":
        o["norm_w"] = 1.0 + 0.1 * torch.randn(K, device=dev, generator=g)
    if "resid" in form:
        o["resid"] = rnd(8, N)
    ref = torch.empty(8, N, device=dev, dtype=torch.float32 if form == "head" else BF)
    for p in range(4):
        _run_gemv(ops.gemv, o, slice(2 * p, 2 * p + 2), ref)
    o["ref"] = ref
    _GEMV_OPERANDS[name] = o
    return o


def _run_gemv(fn, o, rows, out):
    """fn = ops.gemv or ops.gemv_pairs on activation rows `rows`, result into out[rows] (the residual forms run in place)."""
    kw = {}
    if "w2" in o:
        kw.update(w2=o["w2"], act="gelu_tanh")
    if "norm_w" in o:
        kw.update(norm_w=o["norm_w"], norm_eps=1e-5)
    dst = out[rows]
    if "resid" in o:
        dst.copy_(o["resid"][rows])
        kw.update(resid=dst)                     # out == resid, as the decode's wo / w2 projections run
    fn(o["x"][rows], o["w"], dst, **kw)


@pytest.mark.parametrize("P", [1, 2, 3, 4])
@pytest.mark.parametrize("case", GEMV_CASES, ids=[c[0] for c in GEMV_CASES])
def test_gemv_pairs_equals_gemv_per_pair(cuda, case, P):
    """Rows (2p, 2p+1) of ld_gemv_pairs at B = 2P against ld_gemv at B = 2 on those rows: torch.equal."""
    from landiff_amd import ops
    name, K, N, form = case
    o = _gemv_operands(name, K, N, form, cuda)
    out = torch.full_like(o["ref"], float("nan"))
    _run_gemv(ops.gemv_pairs, o, slice(0, 2 * P), out)
    torch.cuda.synchronize()
    assert torch.isfinite(o["ref"].float()).all()
    for p in range(P):
        assert torch.equal(out[2 * p:2 * p + 2], o["ref"][2 * p:2 * p + 2]), (name, P, p)
    assert torch.isnan(out[2 * P:].float()).all()                                  # rows of other pairs untouched
    assert not torch.equal(o["ref"][0:2], o["ref"][2:4])                           # distinct pairs: an index mix-up would show


@pytest.mark.parametrize("L", [112, 113, 232, 233, 700])
def test_kv_attn_split_eight_rows_equals_four_pair_launches(cuda, L):
    """The fused RoPE / append / key-split attention launch at B = 8 against four B = 2 launches on each pair's own cache, at
    context lengths on both sides of the 1 -> 4 and 4 -> nsplit thresholds of kv_eff_splits and in the full-split regime:
    attention output, the appended K / V rows and the rest of the caches, torch.equal."""
    from landiff_amd import ops
    from oracle.llm import rope_table
    H, D, Lmax, nsplit, P = 16, 128, 768, 8, 4
    g = torch.Generator(device=cuda).manual_seed(100 + L)
    cos, sin = rope_table(D, Lmax, 10000.0)
    cos, sin = cos.to(cuda).contiguous(), sin.to(cuda).contiguous()
    kc = torch.randn(2 * P, Lmax, H, D, device=cuda, generator=g).to(BF)
    vc = torch.randn(2 * P, Lmax, H, D, device=cuda, generator=g).to(BF)
    qkv = (torch.randn(2 * P, 3 * H * D, device=cuda, generator=g) * 1.5).to(BF)
    pos = torch.full((1,), L - 1, device=cuda, dtype=torch.int32)

    def run(rows):
        B = rows.stop - rows.start
        k, v = kc[rows].clone(), vc[rows].clone()
        ws = torch.zeros(B * H * (nsplit * 130 + 1), device=cuda, dtype=torch.float32)
        out = torch.full((B, H * D), float("nan"), device=cuda, dtype=BF)
        ops.llm_kv_attn(None, k, v, pos, out, B, 1, H, Lmax, workspace=ws, nsplit=nsplit, qkv_fused=qkv[rows].contiguous(),
                        cos_t=cos, sin_t=sin)
        torch.cuda.synchronize()
        assert int(ws[B * H * nsplit * 130:].abs().sum().item()) == 0
        return out, k, v

    out8, k8, v8 = run(slice(0, 2 * P))
    assert torch.isfinite(out8.float()).all()
    for p in range(P):
        rows = slice(2 * p, 2 * p + 2)
        out2, k2, v2 = run(rows)
        assert torch.equal(out8[rows], out2), (L, p)
        assert torch.equal(k8[rows, L - 1], k2[:, L - 1]) and torch.equal(v8[rows, L - 1], v2[:, L - 1]), (L, p)
        assert not torch.equal(k2[:, L - 1], kc[rows, L - 1])                      # the append happened
        assert torch.equal(k8[rows], k2) and torch.equal(v8[rows], v2), (L, p)
    assert not torch.equal(out8[0:2], out8[2:4])


def test_sample_advance_pairs_equals_single_launches(cuda):
    """ld_llm_sample_advance_pairs with P = 3 against three ld_llm_sample_advance launches on separate state, at an unrestricted
    position (top-k and top-p on), a restricted one and a forced one: tokens, out_tokens, out_count, sampled, positions, the
    probabilities / CFG logits and the embedding rows written for the next step."""
    from landiff_amd import ops
    P, V, D, n_out = 3, 2055, 256, 16
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
        count0 = torch.tensor([0, 3, 5], device=cuda, dtype=torch.int32)
        # ---- three single launches, each on its own state ----
        single = []
        for p in range(P):
            st = dict(pos=torch.full((1,), p0, device=cuda, dtype=torch.int32), token=torch.zeros(1, device=cuda, dtype=torch.int64),
                      out=torch.full((n_out,), -7, device=cuda, dtype=torch.int64), count=count0[p:p + 1].clone(),
                      sampled=torch.zeros(1, device=cuda, dtype=torch.int64), x=torch.zeros(2, D, device=cuda, dtype=BF),
                      probs=torch.zeros(1, V, device=cuda), cfg=torch.zeros(1, V, device=cuda))
            ops.llm_sample_advance(logits[2 * p:2 * p + 2], st["probs"], st["cfg"], True, 7.5, 1.0, st["pos"], allowed, noise[p:p + 1],
                                   forced, st["token"], st["out"], st["count"], st["sampled"], emb, st["x"], **top)
            single.append(st)
        # ---- one launch of P workgroups ----
        pos = torch.full((P,), p0, device=cuda, dtype=torch.int32)
        token = torch.zeros(P, device=cuda, dtype=torch.int64)
        out = torch.full((P, n_out), -7, device=cuda, dtype=torch.int64)
        count, sampled = count0.clone(), torch.zeros(P, device=cuda, dtype=torch.int64)
        x = torch.zeros(2 * P, D, device=cuda, dtype=BF)
        probs, cfg = torch.zeros(P, V, device=cuda), torch.zeros(P, V, device=cuda)
        ops.llm_sample_advance_pairs(logits, probs, cfg, True, 7.5, 1.0, pos, allowed, noise, forced, token, out, count, sampled, emb, x, **top)
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
            assert len(set(token.tolist())) > 1, token.tolist()          # distinct logits and noise per sample
        if kind == "restricted":
            assert set(token.tolist()) <= {2050, 7, 2052}


def _tiny_runner(dev, max_samples):
    from landiff_amd.config import LLMConfig
    from landiff_amd.llm import LLMRunner
    from landiff_amd.weights import init_state, llm_spec
    cfg = LLMConfig.tiny()
    return cfg, LLMRunner(init_state(llm_spec(cfg), 21, dtype=BF, device=dev), cfg, dev, max_text=16, max_frames=6, max_samples=max_samples)


def _check_many(run, text, seeds, **kw):
    """sample_many row p == sample(seed=seeds[p]); the rows differ from each other."""
    single = [run.sample(text, seed=s, **kw).clone() for s in seeds]
    many = run.sample_many(text, seeds, **kw)
    assert many.dtype == torch.int64 and many.shape == (len(seeds), single[0].numel())
    for p, s in enumerate(seeds):
        assert torch.equal(many[p], single[p]), (p, s, (many[p] != single[p]).nonzero()[:4].flatten().tolist())
    for p in range(1, len(seeds)):
        assert not torch.equal(many[0], many[p]), "the samples must differ, or the comparison shows nothing"
    return many


def test_sample_many_tiny_equals_sample_per_seed(cuda):
    """LLMConfig.tiny(), three seeds: guided, unguided, with first_frame_tokens, a multi-segment decode with prefix_tokens and a
    runner built for more samples than asked for."""
    cfg, run = _tiny_runner(cuda, 4)
    text = torch.randn(5, cfg.text_dim, generator=torch.Generator().manual_seed(3)).to(cuda)
    seeds = [11, 12, 13]
    _check_many(run, text, seeds, num_frames=3, guidance_scale=7.5)
    _check_many(run, text, seeds, num_frames=3, guidance_scale=0.0)
    _check_many(run, text, seeds, num_frames=3, guidance_scale=7.5, top_k=20, top_p=0.9)
    first = torch.arange(cfg.iframe_len, dtype=torch.int64) * 7 % cfg.visual_vocab
    many = _check_many(run, text, seeds, num_frames=3, guidance_scale=7.5, first_frame_tokens=first)
    assert torch.equal(many[:, :cfg.iframe_len].cpu(), first[None].expand(3, -1))
    seg = torch.arange(cfg.iframe_len + 2 * cfg.pframe_len, dtype=torch.int64) * 5 % cfg.visual_vocab
    _check_many(run, text, seeds, num_frames=6, guidance_scale=7.5, prefix_tokens=seg)
    # sample() on a max_samples > 1 runner is sample() on a plain one
    _, plain = _tiny_runner(cuda, 1)
    assert torch.equal(plain.sample(text, seed=11, num_frames=3), run.sample(text, seed=11, num_frames=3))


def test_decode_forward_pairs_embeds_each_samples_token(cuda):
    """ld_llm_decode_forward_pairs given the embedding table and token [P] against the same call on x rows filled by hand."""
    from landiff_amd import ops
    cfg, run = _tiny_runner(cuda, 3)
    P, pos_value = 3, 9
    g = torch.Generator(device=cuda).manual_seed(2)
    for cache in run.kc_all + run.vc_all:
        cache.copy_(torch.randn(cache.shape, device=cuda, generator=g).to(BF))
    run.m_token.copy_(torch.tensor([5, 70, 33], device=cuda))
    run.m_pos.fill_(pos_value)
    table = ops.llm_layer_table(run.blocks, run.kc, run.vc)
    logits = []
    for emb in (run.emb, None):
        run.m_attn_ws.zero_()
        run.m_x.copy_(run.emb[run.m_token].to(BF).repeat_interleave(2, 0) if emb is None else torch.full_like(run.m_x, float("nan")))
        ops.llm_decode_forward_pairs(table, emb, run.m_token, run.m_pos, run.m_x, run.m_qkv, run.m_att, run.m_gate, run.m_attn_ws, run.cos,
                                     run.sin, run.ln_w, run.ln_b, run.m_lnf, run.head, run.m_logits, cfg.heads, run.Lmax, run.nsplit,
                                     cfg.rms_eps, cfg.ln_eps, pos_value=pos_value)
        logits.append(run.m_logits.clone())
    assert torch.isfinite(logits[0]).all() and torch.equal(logits[0], logits[1])
    assert not torch.equal(logits[0][0:2], logits[0][2:4])


def test_sample_many_full_width_two_layers(cuda):
    """Hidden 2048, 16 heads, MLP 11008, vocabulary 2055, 2 layers, frame lengths shrunk to full_len 284: the decode passes
    context lengths 113 and 233 and runs the full split count; P = 4."""
    from landiff_amd.config import LLMConfig
    from landiff_amd.llm import LLMRunner, forced_token_schedule
    from landiff_amd.weights import init_state, llm_spec
    cfg = dataclasses.replace(LLMConfig(), num_layers=2, iframe_len=60, pframe_len=20, segment_length=8, segment_stride=8)
    full_len = forced_token_schedule(cfg, 64 + 3, 8)[0]
    assert 250 <= full_len <= 320
    run = LLMRunner(init_state(llm_spec(cfg), 9, dtype=BF, device=cuda), cfg, cuda, max_frames=8, max_samples=4)
    assert run.nsplit == 8
    text = torch.randn(64, cfg.text_dim, generator=torch.Generator().manual_seed(12)).to(cuda)
    _check_many(run, text, [42, 43, 44, 45], num_frames=8, guidance_scale=7.5)


def test_generate_samples_tiny_pipeline_equals_single_calls(cuda):
    """LanDiffPipeline.generate_samples(inp, [s0, s1]) frames against the two single calls."""
    from landiff_amd.config import PipelineConfig
    from landiff_amd.pipeline import LanDiffPipeline, synthetic_inputs
    from landiff_amd.weights import init_pipeline_state
    cfg = PipelineConfig.tiny(num_steps=2).check()
    pipe = LanDiffPipeline(cfg, init_pipeline_state(cfg, seed=1234), cuda, max_samples=2)
    inp = synthetic_inputs(cfg, cuda, n_text=6, seed=42)
    seeds = [42, 77]
    single = [pipe(dataclasses.replace(inp, seed=s)).clone() for s in seeds]
    many = pipe.generate_samples(inp, seeds)
    assert len(many) == 2
    for a, b in zip(many, single):
        assert a.dtype == torch.uint8 and torch.equal(a, b)
    assert not torch.equal(many[0], many[1])
