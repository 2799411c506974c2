"""Scoring of AR token sequences: ld_llm_token_logprobs, ld_llm_head_f32, LLMRunner.score, return_logprobs of sample() /
sample_many(), and best-of-N selection in LanDiffPipeline.generate_samples(keep=k).

Reference: the distribution Semantic1DLM.sample draws from (landiff/llm/models/lm_model.py:417-454, landiff/utils.py:345-359),
restated in float64 in tests/llm_score_ref.py; for the model-level tests a teacher-forced fp32 pass through the oracle's own
blocks (oracle.llm.LLMOracle.prefix_features / block / gpt_step) followed by that restatement.

LOGPROB_BOUND: the worst absolute error of ld_llm_token_logprobs against float64 over every case of llm_score_ref.all_cases()
and the underflow rows, measured on an MI355X (ROCm 7.2), is MEASURED_WORST below; the tests assert 4 x that (the margin is for
expf / logf differences between ROCm versions).  Most of it is the fp32 rounding of the guided logits themselves (|l| up to
~150 after CFG at scale 7.5: half an ulp there is 7.6e-6) and of a result near -200."""
import dataclasses
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
MEASURED_WORST = 4.6e-5        # 4.580e-05 measured over the 58 launches; the underflow rows alone: 6.4e-06
LOGPROB_BOUND = 4 * MEASURED_WORST
assert LOGPROB_BOUND < 1e-3

_CASES = {}


def _cases():
    """The cases and their float64 results: made once, shared by every test that needs them, never modified."""
    if not _CASES:
        import llm_score_ref as R
        cases = R.all_cases() + [R.underflow_case(71), R.underflow_case(2055)]
        for c in cases:
            c["ref"], c["ref_valid"] = R.ref_logprobs(c)
        _CASES["all"] = cases
    return _CASES["all"]


def _run_case(c, dev, want_cfg=False):
    """One ld_llm_token_logprobs launch on a case, in its layout and position form -> (logprob, valid[, cfg_logits]) on the CPU."""
    from landiff_amd import ops
    n, V = c["n"], c["V"]
    if c["layout"] == "planes":                       # [2][n][ld], rows padded to ld = V + 9, NaN in the padding
        ld = V + 9
        buf = torch.full((2, n, ld), NAN, device=dev)
        buf[0, :, :V], buf[1, :, :V] = c["cond"].to(dev), c["uncond"].to(dev)
        cond, uncond = buf[0, :, :V], buf[1, :, :V]
    else:                                             # [2P][V]: rows (2p, 2p + 1) = (cond, uncond) of sample p
        buf = torch.stack([c["cond"], c["uncond"]], 1).reshape(2 * n, V).contiguous().to(dev)
        pairs = buf.view(n, 2 * V)
        cond, uncond = pairs[:, :V], pairs[:, V:]
    lp = torch.full((n,), NAN, device=dev)
    valid = torch.full((n,), -9, device=dev, dtype=torch.int32)
    kw = dict(allowed=c["allowed"].to(dev), forced=c["forced"].to(dev), top_k=c["top_k"], top_p=c["top_p"], valid=valid)
    if c["word_mode"]:                                # one position word per row, as after a sampling launch: word - 1
        kw.update(pos=(torch.tensor(c["positions"], dtype=torch.int32) + 1).to(dev), pos_stride=1 if n > 1 else 0, pos_bias=-1)
    else:
        assert c["positions"] == list(range(c["positions"][0], c["positions"][0] + n))
        kw.update(pos=None, pos_bias=c["positions"][0])
    cfg = torch.full((n, V + 3), NAN, device=dev) if want_cfg else None
    if want_cfg:
        kw.update(cfg_logits=cfg[:, :V])
    ops.llm_token_logprobs(cond, uncond if c["guided"] or c["si"] % 3 else None, c["target"].to(dev), lp, c["guided"], c["scale"],
                           c["temperature"], **kw)
    torch.cuda.synchronize()
    return (lp.cpu(), valid.cpu(), cfg.cpu()) if want_cfg else (lp.cpu(), valid.cpu())


def _check_against_ref(c, lp, valid):
    """Exact pattern of -inf / forced rows / valid; -> worst absolute error of the finite rows."""
    ref, tag = c["ref"], (c["V"], c["layout"], c["n"], c["si"])
    assert torch.equal(valid, c["ref_valid"]), (tag, valid.tolist(), c["ref_valid"].tolist())
    assert not torch.isnan(lp).any(), (tag, lp.tolist())
    assert torch.equal(torch.isinf(lp), torch.isinf(ref)), (tag, lp.tolist(), ref.tolist())
    assert (lp[torch.isinf(lp)] < 0).all()
    for r, kind in enumerate(c["kinds"]):
        if kind == "forced":
            assert lp[r].item() == 0.0 and valid[r].item() == 0, (tag, r)
        if kind == "restricted_out":
            assert lp[r].item() == -math.inf, (tag, r)
        if kind == "restricted_in":
            assert math.isfinite(lp[r].item()), (tag, r)
    fin = torch.isfinite(ref)
    return (lp[fin].double() - ref[fin]).abs().max().item() if fin.any() else 0.0


def test_token_logprobs_vs_float64(cuda):
    """Every case of llm_score_ref.all_cases(): V in {71, 2055}; [2][n][V] with padded rows at n in {1, 5, 67} and the [2P][V]
    pair layout at P = 3; guided and unguided; temperature 1.0 and 0.7; top_k in {1, 5} with a tie at the threshold; top_p in
    {0.3, 0.9}; restricted positions with 1-3 allowed ids (target inside: finite, outside: exactly -inf); forced positions
    (logprob 0, valid 0); the position as base + row and as a device word with bias -1.  Measured worst absolute error against
    float64: see MEASURED_WORST (asserted: 4 x that)."""
    worst, seen = 0.0, set()
    for c in _cases():
        lp, valid = _run_case(c, cuda)
        err = _check_against_ref(c, lp, valid)
        worst = max(worst, err)
        seen.update(c["kinds"])
        if c["top_k"] == 5 and c["layout"] == "planes" and c["n"] >= 5:
            tie_rows = [r for r, k in enumerate(c["kinds"]) if k == "free" and r % 4 == 0]
            assert tie_rows
            if c["top_p"] is None:
                assert all(math.isfinite(lp[r].item()) for r in tie_rows), (c["V"], c["si"], lp.tolist())     # the tie stayed
    print(f"\nld_llm_token_logprobs: worst |error| against float64 over {len(_cases())} launches: {worst:.3e} (bound {LOGPROB_BOUND:.3e})")
    assert seen == {"free", "restricted_in", "restricted_out", "forced"}
    assert worst <= LOGPROB_BOUND, (worst, LOGPROB_BOUND)


def test_token_logprobs_finite_where_the_probability_underflows(cuda):
    """l_t - max = -200: exp(-200) is 0 in fp32, so logf of the sampling kernel's probability is -inf; the log-domain result is
    an ordinary number and matches float64."""
    from landiff_amd import ops
    for c in _cases():
        if c["kinds"] != ["free", "free"] or c["n"] != 2 or c["top_k"] is not None or c["guided"]:
            continue
        lp, valid = _run_case(c, cuda)
        assert torch.isfinite(lp).all() and (lp < -195).all() and (lp > -215).all(), lp.tolist()
        err = (lp.double() - c["ref"]).abs().max().item()
        print(f"\nunderflow rows V={c['V']}: {lp.tolist()} float64 {c['ref'].tolist()} |error| {err:.3e}")
        assert err <= LOGPROB_BOUND, (err, LOGPROB_BOUND)
        # the shipped sampling kernel's probability of that id is exactly 0: its logarithm would be -inf
        probs = torch.full((1, c["V"]), NAN, device=cuda)
        ops.llm_logits_to_probs(torch.stack([c["cond"][0], c["uncond"][0]]).to(cuda), probs, None, False, 7.5, 1.0)
        assert probs[0, c["target"][0]].item() == 0.0


def test_token_logprobs_consistent_with_sampling_kernel(cuda):
    """Row by row against ld_llm_logits_to_probs on the same inputs: the guided logits bit-equal to its cfg_logits, and for
    targets with p >= 1e-30, exp(logprob) within the error bound of its probs[target]; a target it gives probability 0 because
    a filter removed it has logprob -inf."""
    from landiff_amd import ops
    checked = removed = 0
    for c in _cases():
        if c["n"] != 5 or c["layout"] != "planes":
            continue
        lp, valid, cfg = _run_case(c, cuda, want_cfg=True)
        al, V = c["allowed"].to(cuda), c["V"]
        for r in range(c["n"]):
            if c["kinds"][r] == "forced":
                assert torch.isnan(cfg[r]).all()                      # not a draw: nothing written
                continue
            probs, ref_cfg = torch.full((1, V), NAN, device=cuda), torch.full((1, V), NAN, device=cuda)
            pos = torch.tensor([c["positions"][r]], device=cuda, dtype=torch.int32)
            ops.llm_logits_to_probs(torch.stack([c["cond"][r], c["uncond"][r]]).to(cuda), probs, ref_cfg, c["guided"], c["scale"],
                                    c["temperature"], pos, al, top_k=c["top_k"], top_p=c["top_p"])
            assert torch.equal(cfg[r, :V], ref_cfg[0].cpu()), (V, c["si"], r)
            assert torch.isnan(cfg[r, V:]).all()
            p = probs[0, c["target"][r]].item()
            if p >= 1e-30:
                assert abs(math.exp(lp[r].item()) - p) <= LOGPROB_BOUND, (V, c["si"], r, lp[r].item(), p)
                checked += 1
            elif c["kinds"][r] != "free" or c["top_k"] is not None or c["top_p"] is not None:
                if p == 0.0 and not math.isfinite(c["ref"][r].item()):
                    assert lp[r].item() == -math.inf
                    removed += 1
    assert checked >= 20 and removed >= 5, (checked, removed)


@pytest.mark.parametrize("case", ["plain", "top_k_tie", "top_p", "restricted"])
def test_token_logprobs_support_equals_sampling_kernel(cuda, case):
    """The scorer and the sampler state one distribution (csrc/ld_llm_sample_dev.h), so their supports are the same set, id for id:
    over EVERY id of a row as the target, logprob is finite exactly where ld_llm_logits_to_probs gives a non-zero probability and
    -inf where a filter or the restriction gave 0.  V = 70 is no multiple of 64 (the last wave is partly idle in both block
    reductions); four rows of guided logits small enough that no kept probability underflows.  plain: neither filter, all 70 ids;
    top_k_tie: top-k = 5 with the 5th and 6th largest guided logits equal, 6 ids; top_p: 0.9; restricted: 3 allowed ids."""
    from landiff_amd import ops
    V, rows, scale, temperature, position = 70, 4, 7.5, 0.9, 3
    g = torch.Generator().manual_seed(70)
    cond, uncond = 0.5 * torch.randn(rows, V, generator=g), 0.5 * torch.randn(rows, V, generator=g)
    if case == "top_k_tie":
        order = (uncond + scale * (cond - uncond)).argsort(1, descending=True)
        for r in range(rows):                                             # equal operands: the guided logits tie bit for bit
            cond[r, order[r, 5]], uncond[r, order[r, 5]] = cond[r, order[r, 4]], uncond[r, order[r, 4]]
    allowed = torch.zeros(position + 2, 4, dtype=torch.int32)
    if case == "restricted":
        allowed[position + 1] = torch.tensor([3, 69, 0, 41], dtype=torch.int32)
    kw = dict(top_k=5 if case == "top_k_tie" else None, top_p=0.9 if case == "top_p" else None)
    cond, uncond, allowed = cond.to(cuda), uncond.to(cuda), allowed.to(cuda)
    pos = torch.tensor([position], device=cuda, dtype=torch.int32)
    targets = torch.arange(V, device=cuda)
    for r in range(rows):
        probs = torch.full((1, V), NAN, device=cuda)
        ops.llm_logits_to_probs(torch.stack([cond[r], uncond[r]]), probs, None, True, scale, temperature, pos, allowed, **kw)
        lp = torch.full((V,), NAN, device=cuda)
        ops.llm_token_logprobs(cond[r:r + 1].expand(V, V), uncond[r:r + 1].expand(V, V), targets, lp, True, scale, temperature,
                               pos=pos, pos_stride=0, allowed=allowed, **kw)
        kept = probs[0] > 0
        print(f"{case} row {r}: sampler support {int(kept.sum())} ids, scorer finite {int(torch.isfinite(lp).sum())}")
        assert not torch.isnan(probs).any() and not torch.isnan(lp).any()
        assert torch.equal(torch.isfinite(lp), kept), (case, r, kept.nonzero().flatten().tolist(), torch.isfinite(lp).nonzero().flatten().tolist())
        assert bool((lp[~kept] == -math.inf).all())
        n = int(kept.sum())
        assert n == {"plain": V, "top_k_tie": 6, "restricted": 3}.get(case, n) and 0 < n < (V if case == "top_p" else V + 1), (case, r, n)
        if case == "restricted":
            assert kept.nonzero().flatten().tolist() == [0, 41, 69]


# ---- ld_llm_head_f32 -------------------------------------------------------------------------------------------------
_HEAD = {}


def _head_operands(N, K, dev):
    if (N, K) not in _HEAD:
        g = torch.Generator(device=dev).manual_seed(N * 7 + K)
        a = torch.randn(257, K + 8, device=dev, generator=g)                      # strided rows: lda = K + 8
        w = torch.randn(N, K, device=dev, generator=g) * K ** -0.5
        ref = a[:, :K].double() @ w.double().t()
        mag = a[:, :K].double().abs() @ w.double().abs().t()
        _HEAD[(N, K)] = (a, w, ref, mag)
    return _HEAD[(N, K)]


@pytest.mark.parametrize("K", [256, 2048])
@pytest.mark.parametrize("N", [71, 2055])
@pytest.mark.parametrize("M", [2, 6, 134, 257])
def test_head_f32_vs_float64(cuda, M, N, K):
    """C = A . W^T in fp32 against a float64 matmul: every element within K * 2^-24 * sum|a w| (the fp32 dot-product bound for any
    summation order, the sum taken in float64); A with a row stride; rows and columns outside [M] x [N] of an over-allocated
    output stay NaN."""
    from landiff_amd import ops
    a, w, ref, mag = _head_operands(N, K, cuda)
    out = torch.full((M + 3, N + 5), NAN, device=cuda)
    ops.llm_head_f32(a[:M, :K], w, out[:M, :N])
    torch.cuda.synchronize()
    got = out[:M, :N]
    assert torch.isfinite(got).all()
    excess = ((got.double() - ref[:M]).abs() - K * 2.0 ** -24 * mag[:M]).max().item()
    rel = ((got.double() - ref[:M]).abs() / mag[:M]).max().item()
    print(f"\nhead M={M} N={N} K={K}: worst |error| / sum|a w| = {rel:.3e} (bound {K * 2.0 ** -24:.3e})")
    assert excess <= 0.0, (M, N, K, excess)
    assert torch.isnan(out[M:]).all() and torch.isnan(out[:, N:]).all()


def test_head_f32_refuses_k_not_multiple_of_4(cuda):
    from landiff_amd import _lib, ops
    a, w, out = torch.zeros(4, 12, device=cuda)[:, :10], torch.zeros(8, 10, device=cuda), torch.zeros(4, 8, device=cuda)
    with pytest.raises(_lib.LandiffHipError, match="multiples of 4"):
        ops.llm_head_f32(a, w, out)


def test_head_f32_k_tail_of_the_tile(cuda):
    """K = 40: a multiple of 4 but not of the tile's K step of 16 (the last step is half empty)."""
    from landiff_amd import ops
    g = torch.Generator(device=cuda).manual_seed(3)
    a, w = torch.randn(70, 40, device=cuda, generator=g), torch.randn(65, 40, device=cuda, generator=g)
    out = torch.full((70, 65), NAN, device=cuda)
    ops.llm_head_f32(a, w, out)
    ref, mag = a.double() @ w.double().t(), a.double().abs() @ w.double().abs().t()
    assert ((out.double() - ref).abs() <= 40 * 2.0 ** -24 * mag).all()


# ---- LLMRunner: score, return_logprobs ---------------------------------------------------------------------------------
def _tiny(dev, max_samples=1):
    from landiff_amd.config import LLMConfig
    from landiff_amd.llm import LLMRunner
    from landiff_amd.weights import init_state, llm_spec
    cfg = LLMConfig.tiny()
    sd = init_state(llm_spec(cfg), 21, dtype=BF)
    text = torch.randn(5, cfg.text_dim, generator=torch.Generator().manual_seed(3)).to(BF)
    return cfg, sd, LLMRunner(sd, cfg, dev, max_text=16, max_frames=6, max_samples=max_samples), text, 3


def _wide(dev, max_samples=1):
    """Hidden 2048, 16 heads, MLP 11008, vocabulary 2055, two layers, frame lengths shrunk (full_len 157, Lmax small)."""
    from landiff_amd.config import LLMConfig
    from landiff_amd.llm import LLMRunner
    from landiff_amd.weights import init_state, llm_spec
    cfg = dataclasses.replace(LLMConfig(), num_layers=2, iframe_len=40, pframe_len=12, segment_length=5, segment_stride=5)
    sd = init_state(llm_spec(cfg), 9, dtype=BF)
    text = torch.randn(48, cfg.text_dim, generator=torch.Generator().manual_seed(12)).to(BF)
    return cfg, sd, LLMRunner(sd, cfg, dev, max_text=48, max_frames=5, max_samples=max_samples), text, 5


_MODELS = {}


def _model(name, dev):
    """(cfg, state, runner, text, num_frames, ids, oracle log-probs fp32 / bf16): one runner and one pair of oracle passes per
    configuration for all the tests below.  The ids are a sample of the runner itself (seed 42, guided)."""
    if name not in _MODELS:
        cfg, sd, run, text, nf = (_tiny if name == "tiny" else _wide)(dev, max_samples=3)
        ids, online = run.sample(text.to(dev), seed=42, num_frames=nf, guidance_scale=7.5, return_logprobs=True)
        ids, online = ids.clone().cpu(), online.clone().cpu()
        ref32 = _oracle_logprobs(cfg, sd, text, nf, ids, torch.float32)
        ref16 = _oracle_logprobs(cfg, sd, text, nf, ids, BF)
        _MODELS[name] = dict(cfg=cfg, sd=sd, run=run, text=text.to(dev), nf=nf, ids=ids, online=online, ref32=ref32, ref16=ref16)
    return _MODELS[name]


def _oracle_logprobs(cfg, sd, text, nf, ids, dtype, scale=7.5, temperature=1.0):
    """Teacher-forced pass of the oracle's own parts in `dtype` (blocks; final LayerNorm and head in fp32 as gpt_step has them)
    over the whole sequence, then the float64 restatement at the given ids -> float64 [n_visual]."""
    from llm_score_ref import ref_logprob_row
    from oracle.common import layer_norm
    from oracle.llm import LLMOracle, forced_schedule, rope_table
    sdt = {k: (v.to(dtype) if v.dtype == BF else v) for k, v in sd.items()}
    orc = LLMOracle(sdt, cfg, dtype)
    with torch.no_grad():
        feats = orc.prefix_features(text.float(), float(nf), 0.1, True)
        S = feats.shape[1] - 1
        full_len, forced, restricted, n_visual = forced_schedule(cfg, S, nf)
        it = iter(ids.tolist())
        seq = [forced[q] if q in forced else next(it) for q in range(S + 1, full_len)]
        emb = sd["visual_embedding_model.tok_emb_code.weight"]
        x = torch.cat([feats, emb[torch.tensor(seq[:-1])].float()[None].expand(2, -1, -1)], 1).to(dtype)
        cos, sin = rope_table(cfg.head_dim, full_len, cfg.rope_theta)
        m = full_len - 1
        cache = [None] * cfg.num_layers
        # gpt_step on the same input gives the last row: the restated all-rows tail below must agree with it
        last = orc.gpt_step(x, [None] * cfg.num_layers, cos[None, :m], sin[None, :m])
        for i in range(cfg.num_layers):
            x = orc.block(i, x, cache, cos[None, :m], sin[None, :m])
        x = layer_norm(x.float(), sdt["transformer.layer_norm.weight"], sdt["transformer.layer_norm.bias"], cfg.ln_eps)
        logits = torch.nn.functional.linear(x[:, S:], sdt["transformer.head.weight"].float())        # [2, full_len - 1 - S, V]
        assert torch.allclose(logits[:, -1], last, rtol=1e-5, atol=1e-4)       # (another matmul shape: not the same bits)
    out = []
    for j, q in enumerate(range(S + 1, full_len)):
        if q in forced:
            continue
        lp, _ = ref_logprob_row(logits[0, j], logits[1, j], True, scale, temperature, restricted.get(q, []), -1, None, None, seq[j])
        out.append(lp)
    assert len(out) == n_visual
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_score_vs_oracle_pass(cuda, name):
    """LLMRunner.score of a sample's ids against the fp32 teacher-forced oracle pass, by the floor rule: the HIP
    path's error is at most 2 x the error of the same pass in torch bf16.  The online log-probabilities of the sample
    (return_logprobs) are held to the same rule; their difference from score() (prefill GEMMs against decode GEMVs) is printed.
    Measured (worst per-token |difference|): tiny: score 0.071, online 0.126, bf16 floor 0.140, score against online 0.127;
    wide: score 0.207, online 0.246, bf16 floor 0.175, score against online 0.172."""
    m = _model(name, cuda)
    run = m["run"]
    lp, total = run.score(m["text"], m["ids"], num_frames=m["nf"], guidance_scale=7.5)
    lp = lp.cpu().double()
    assert lp.shape == m["ref32"].shape and torch.isfinite(lp).all()
    assert abs(total - lp.sum().item()) < 1e-6 * max(1.0, abs(total))
    floor = (m["ref16"] - m["ref32"]).abs().max().item()
    err_score = (lp - m["ref32"]).abs().max().item()
    err_online = (m["online"].double() - m["ref32"]).abs().max().item()
    diff = (lp - m["online"].double()).abs().max().item()
    print(f"\n{name}: {lp.numel()} ids, total {total:.3f}; |score - fp32 oracle| {err_score:.4e}, |online - fp32 oracle| {err_online:.4e}, "
          f"torch bf16 floor {floor:.4e}; |score - online| {diff:.4e}")
    assert err_score <= 2 * floor, (err_score, floor)
    assert err_online <= 2 * floor, (err_online, floor)
    # ids the model did not sample score lower in total than its own sample (a sanity check of direction, not of size)
    other = (m["ids"] + 1) % m["cfg"].visual_vocab
    assert run.score(m["text"], other, num_frames=m["nf"], guidance_scale=7.5)[1] < total


def test_score_refusals(cuda):
    m = _model("tiny", cuda)
    run, text, nf, ids = m["run"], m["text"], m["nf"], m["ids"]
    long_text = torch.zeros(40, m["cfg"].text_dim, device=cuda)
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="positions"):
        run.score(long_text, ids, num_frames=6)
    with pytest.raises(ValueError, match="ids outside"):
        run.score(text, ids.clone().index_fill_(0, torch.tensor([2]), m["cfg"].visual_vocab), num_frames=nf)
    with pytest.raises(ValueError, match="ids outside"):
        run.score(text, ids.clone().index_fill_(0, torch.tensor([0]), -1), num_frames=nf)
    with pytest.raises(ValueError, match="frames hold"):
        run.score(text, ids[:-1], num_frames=nf)
    assert torch.cuda.memory_allocated() == before


def test_prefill_unchanged_by_the_refactor(cuda):
    """_prefill after its block loop moved into _prefill_blocks: logits and KV rows torch.equal to the old op sequence, restated
    here through ops."""
    from landiff_amd import ops
    m = _model("tiny", cuda)
    run, c = m["run"], m["cfg"]
    feats = run.prefix_features(m["text"], float(m["nf"]), 0.1)
    for t in run.kc + run.vc:
        t.zero_()
    run._prefill(feats.clone())                           # (the residual stream is updated in place, in the caller's tensor)
    torch.cuda.synchronize()
    got_logits, got_k, got_v = run.logits.clone(), [t.clone() for t in run.kc], [t.clone() for t in run.vc]
    for t in run.kc + run.vc:
        t.zero_()
    run.logits.fill_(NAN)
    B, mm, d = feats.shape
    M = B * mm
    x = feats.clone().reshape(M, d).contiguous()
    xn = torch.empty_like(x)
    qkv, qr, att = (torch.empty(M, n, device=cuda, dtype=BF) for n in (3 * d, d, d))
    h3, gate = torch.empty(M, c.mlp, device=cuda, dtype=BF), torch.empty(M, c.mlp, device=cuda, dtype=BF)
    run.pos0.zero_()
    for i, w in enumerate(run.blocks):
        ops.rmsnorm(x, w["n0"], xn, c.rms_eps)
        ops.gemm(xn, w["wqkv"], out=qkv)
        ops.llm_rope_append(qkv, run.cos, run.sin, run.pos0, qr, run.kc[i], run.vc[i], B, mm, c.heads, run.Lmax)
        ops.llm_kv_attn(qr, run.kc[i], run.vc[i], run.pos0, att, B, mm, c.heads, run.Lmax)
        ops.gemm(att, w["wo"], out=x, resid=x)
        ops.rmsnorm(x, w["n1"], xn, c.rms_eps)
        ops.gemm(xn, w["w3"], out=h3)
        ops.gemm(xn, w["w1"], out=gate, act="gelu_tanh", mul=h3)
        ops.gemm(gate, w["w2"], out=x, resid=x)
    ops.layernorm_bf16_to_f32(x.view(B, mm, d)[:, -1], run.ln_w, run.ln_b, run.lnf, c.ln_eps)
    ops.gemv(run.lnf, run.head, run.logits)
    torch.cuda.synchronize()
    assert torch.isfinite(got_logits).all() and torch.equal(got_logits, run.logits)
    for i in range(c.num_layers):
        assert torch.equal(got_k[i], run.kc[i]) and torch.equal(got_v[i], run.vc[i])
        assert got_k[i][:, :mm].float().abs().sum() > 0


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_return_logprobs_leaves_ids_and_matches_single(cuda, name):
    """sample_many(return_logprobs=True): ids torch.equal to the call without the flag, row p's log-probabilities torch.equal to
    sample(seed=seeds[p], return_logprobs=True); against logits_log (the guided logits of every step), a float64 log-softmax at
    the sampled ids agrees within the kernel bound."""
    from landiff_amd.llm import forced_token_schedule
    m = _model(name, cuda)
    run, text, nf, seeds = m["run"], m["text"], m["nf"], [42, 43, 44]
    kw = dict(num_frames=nf, guidance_scale=7.5)
    plain = run.sample_many(text, seeds, **kw).clone()
    log = []
    ids, lps = run.sample_many(text, seeds, return_logprobs=True, logits_log=log, **kw)
    ids, lps = ids.clone(), lps.clone()
    assert torch.equal(ids, plain)
    assert lps.dtype == torch.float32 and lps.shape == ids.shape and torch.isfinite(lps).all()
    assert torch.equal(ids[0].cpu(), m["ids"]) and torch.equal(lps[0].cpu(), m["online"])
    for p in (1, 2):
        i1, l1 = run.sample(text, seed=seeds[p], return_logprobs=True, **kw)
        assert torch.equal(i1, ids[p]) and torch.equal(l1, lps[p]), p
    assert torch.equal(run.sample(text, seed=seeds[1], **kw), ids[1])
    # float64 log-softmax of the recorded guided logits (temperature 1, no filters) at the sampled ids
    S = text.shape[0] + 3
    full_len, forced, restricted, _ = forced_token_schedule(m["cfg"], S, nf)
    steps = torch.stack(log, 0).cpu().double()                                      # [generated positions, P, V]
    assert steps.shape[0] == full_len - 1 - S
    worst, j = 0.0, 0
    for k, q in enumerate(range(S + 1, full_len)):
        if q in forced:
            continue
        l = steps[k]
        if q in restricted:
            mask = torch.full_like(l, -math.inf); mask[:, restricted[q]] = 0; l = l + mask
        ref = torch.log_softmax(l, -1).gather(1, ids[:, j].cpu()[:, None])[:, 0]
        worst = max(worst, (ref - lps[:, j].cpu().double()).abs().max().item())
        j += 1
    print(f"\n{name}: online log-probabilities against float64 log-softmax of logits_log: worst |error| {worst:.3e}")
    assert j == ids.shape[1] and worst <= LOGPROB_BOUND, (worst, LOGPROB_BOUND)


def test_return_logprobs_refusals(cuda):
    m = _model("tiny", cuda)
    run, text, nf = m["run"], m["text"], m["nf"]
    with pytest.raises(ValueError, match="return_logprobs"):
        run.sample(text, seed=42, num_frames=nf, return_logprobs=True, use_graph=True)
    with pytest.raises(ValueError, match="return_logprobs"):
        run.sample(text, seed=42, num_frames=nf, return_logprobs=True, mode="chained")
    with pytest.raises(ValueError, match="return_logprobs"):
        run.sample(text, seed=42, num_frames=nf, return_logprobs=True, teacher_fed=torch.zeros(64, dtype=torch.int64, device=cuda))
    for kw in (dict(use_graph=True), dict(mode="chained"), dict(teacher_fed=torch.zeros(64, dtype=torch.int64, device=cuda))):
        with pytest.raises(ValueError):
            run.sample_many(text, [42, 43], num_frames=nf, return_logprobs=True, **kw)


# ---- pipeline ---------------------------------------------------------------------------------------------------------------
def test_generate_samples_keep_tiny_pipeline(cuda):
    """generate_samples(keep=1) returns the candidate of highest score with the frames the keep=None call gives that seed;
    keep=len(seeds) returns all, in rank order; last_candidates holds every candidate's ids (sample_many's) and scores;
    score_tokens of a candidate is finite; score_clip without the Theia extractor fails as tokenize_frames does."""
    from landiff_amd.config import PipelineConfig
    from landiff_amd.pipeline import LanDiffPipeline, rank_candidates, synthetic_inputs
    from landiff_amd.weights import init_pipeline_state
    cfg = PipelineConfig.tiny(num_steps=2).check()
    pipe = LanDiffPipeline(cfg, init_pipeline_state(cfg, seed=1234), cuda, max_samples=3)
    inp = synthetic_inputs(cfg, cuda, n_text=6, seed=42)
    seeds = [42, 77, 5]
    every = [f.clone() for f in pipe.generate_samples(inp, seeds)]
    assert pipe.last_candidates is None                       # keep=None is the call it always was
    tokens = pipe.llm.sample_many(inp.llm_text_emb, seeds, motion_score=inp.motion_score, num_frames=cfg.llm.segment_length,
                                  guidance_scale=inp.cfg, temperature=1.0).clone()
    best = pipe.generate_samples(inp, seeds, keep=1)
    cand = pipe.last_candidates
    assert len(best) == 1 and torch.equal(cand["tokens"], tokens) and cand["seeds"] == seeds
    scores = cand["scores"]
    assert all(math.isfinite(s) for s in scores) and len(set(scores)) == 3
    top = max(range(3), key=lambda i: scores[i])
    seed, score, frames = best[0]
    assert seed == seeds[top] and score == scores[top] and torch.equal(frames, every[top])
    ranked = pipe.generate_samples(inp, seeds, keep=3)
    order = rank_candidates(scores)
    assert [s for s, _, _ in ranked] == [seeds[i] for i in order] and order[0] == top
    assert [sc for _, sc, _ in ranked] == sorted(scores, reverse=True)
    for (_, _, fr), i in zip(ranked, order):
        assert torch.equal(fr, every[i])
    lp, total = pipe.score_tokens(inp, tokens[1])
    assert math.isfinite(total) and torch.isfinite(lp).all() and lp.numel() == tokens.shape[1]
    with pytest.raises(ValueError, match="tokenize_frames needs"):
        pipe.score_clip(inp, torch.zeros(9, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="keep"):
        pipe.generate_samples(inp, seeds, keep=4)
