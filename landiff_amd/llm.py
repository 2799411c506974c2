"""Autoregressive semantic-token decode on MI355X.

Mirrors Semantic1DLM.tokenize / .sample (landiff/llm/models/lm_model.py:175-516), GPT.sample
(landiff/llm/models/transformer.py:91-119), LlamaTransformerBlock with the KV-cache path
(landiff/llm/modules/transformer_blocks.py:128-236), TextCond / MicroConditioner
(landiff/llm/modules/conditioner.py:90-170,230-323) and Rope1DPosEmb (landiff/modules/pos_emb.py:73-123).

What changes is mechanism only: weights are cast to bf16 once (the reference re-casts 2 B parameters every
forward under autocast), the KV cache is preallocated in HBM and appended in place, position / current token /
forced-token schedule live in device memory, and the per-token step is captured in a HIP graph and replayed.
torch.multinomial stays on PyTorch-ROCm so the RNG stream is the reference's (one draw per step, forced or not).
"""
from __future__ import annotations

import math

import os
import time

import torch

from . import _lib, ops
from .config import LLMConfig

BF = torch.bfloat16


def forced_token_schedule(cfg: LLMConfig, S: int, num_frames: int):
    """Position bookkeeping of lm_model.py:323-396 (END tokens enabled): returns (full_len, forced {pos: id},
    restricted {pos: [ids]}, n_visual).  S is the position of the first START_OF_IFrame."""
    I, P, seg, stride = cfg.iframe_len, cfg.pframe_len, cfg.segment_length, cfg.segment_stride
    code_len = 0
    for off in range(0, num_frames, stride):
        fl = min(off + seg, num_frames) - off
        code_len += I + (fl - 1) * P + 2 * fl
    full_len = S + code_len + 1
    block = I + (seg - 1) * P + 2 * seg
    start_i, end_i, start_p, end_p, eos_ok = set(), set(), set(), set(), set()
    for index in range(S, full_len - 1, block):          # one block per segment
        start_i.add(index)
        pos = index + 1 + I                               # END_OF_IFrame slot
        end_i.add(pos)
        pos += 1
        if index > S:
            eos_ok.add(pos)
        p_end = min(full_len - 1, pos - 1 + P * (seg - 1) + 2 * (seg - 1))
        for j in range(pos, p_end, P + 2):                # START_P, P tokens, END_P
            start_p.add(j)
            end_p.add(j + P + 1)
            if index > S:
                eos_ok.add(j + P + 2)
    forced, restricted = {}, {}
    for i in range(S + 1, full_len):
        allowed = [t for t, st in ((cfg.START_I, start_i), (cfg.START_P, start_p), (cfg.EOS, eos_ok)) if i in st]
        if allowed:
            restricted[i] = allowed
        for t, st in ((cfg.START_I, start_i), (cfg.END_I, end_i), (cfg.START_P, start_p), (cfg.END_P, end_p)):
            if i in st:
                forced[i] = t
                break
        else:
            if i == full_len - 1:
                forced[i] = cfg.EOS
    n_visual = (full_len - S - 1) - len(forced)
    return full_len, forced, restricted, n_visual


class LLMRunner:
    B = 2   # (cond, uncond)

    def __init__(self, sd: dict, cfg: LLMConfig, device, max_text: int = 512, max_frames: int = 13, max_samples: int = 1,
                 wide_samples: int = 0):
        """max_samples > 1: sample_many() decodes up to that many samples of one prompt side by side (KV cache and step buffers
        for 2 * max_samples rows; sample() keeps working on the first pair of them).  1: nothing extra is allocated.
        wide_samples (0..16, independent of max_samples): sample_many(engine="mfma") decodes up to that many samples on the MFMA
        engine (ld_gemv_wide): KV cache and step buffers for 2 * wide_samples rows, rows 0-1 being the cache sample() and the
        prefill use.  At full size (24 layers, hidden 2048, the default max_text / max_frames) a row's K and V cost ~0.36 GB:
        ~11.5 GB at wide_samples=16.  The two limits share one allocation of 2 * max(max_samples, wide_samples) rows."""
        assert 1 <= max_samples <= ops.LLM_MAX_PAIRS, f"max_samples {max_samples} outside [1, {ops.LLM_MAX_PAIRS}]"
        assert 0 <= wide_samples <= ops.LLM_MAX_WIDE, f"wide_samples {wide_samples} outside [0, {ops.LLM_MAX_WIDE}]"
        self.cfg, self.dev, self.max_samples, self.wide_samples = cfg, device, max_samples, wide_samples
        n_rows = max(max_samples, wide_samples)            # samples the m_* buffers and the KV cache hold
        multi = max_samples > 1 or wide_samples >= 1       # sample_many has buffers of its own
        c = cfg
        g = lambda k, dt=BF: sd[k].detach().to(device=device, dtype=dt).contiguous()
        self.blocks = []
        for i in range(c.num_layers):
            p = f"transformer.blocks.{i}."
            self.blocks.append(dict(n0=g(p + "norm0.weight", torch.float32), n1=g(p + "norm1.weight", torch.float32),
                                    wqkv=g(p + "wqkv.weight"), wo=g(p + "wo.weight"), w1=g(p + "mlp.w1.weight"),
                                    w3=g(p + "mlp.w3.weight"), w2=g(p + "mlp.w2.weight")))
        self.ln_w, self.ln_b = g("transformer.layer_norm.weight", torch.float32), g("transformer.layer_norm.bias", torch.float32)
        self.head = g("transformer.head.weight", torch.float32)
        self.emb = g("visual_embedding_model.tok_emb_code.weight", torch.float32)
        self.fc0 = (g("cond_model.embeddings.fc0.weight"), g("cond_model.embeddings.fc0.bias"))
        self.fc1 = (g("cond_model.embeddings.fc1.weight"), g("cond_model.embeddings.fc1.bias"))
        self.null_text = g("cond_model.null_text_embedding")
        self.micro = {k: (g(f"micro_condition.mlps.{k}.0.weight"), g(f"micro_condition.mlps.{k}.0.bias"),
                          g(f"micro_condition.mlps.{k}.2.weight"), g(f"micro_condition.mlps.{k}.2.bias"))
                      for k in ("frames", "motion_score")}
        # RoPE table (pos_emb.py:49-70)
        n_seg = -(-max_frames // c.segment_stride)
        self.Lmax = max_text + 4 + n_seg * (c.iframe_len + (c.segment_length - 1) * c.pframe_len + 2 * c.segment_length) + 2
        freqs = 1.0 / (c.rope_theta ** (torch.arange(0, c.head_dim, 2)[: c.head_dim // 2].float() / c.head_dim))
        ang = torch.outer(torch.arange(self.Lmax).float(), freqs).float()
        cis = torch.polar(torch.ones_like(ang), ang)
        self.cos, self.sin = cis.real.contiguous().to(device), cis.imag.contiguous().to(device)
        # state in HBM
        B, H, D = self.B, c.heads, c.head_dim
        if not multi:
            self.kc = [torch.zeros(B, self.Lmax, H, D, device=device, dtype=BF) for _ in range(c.num_layers)]
            self.vc = [torch.zeros(B, self.Lmax, H, D, device=device, dtype=BF) for _ in range(c.num_layers)]
        else:
            # rows (2p, 2p+1) = sample p; the first pair is the cache sample() and the prefill use (same address, same layout)
            self.kc_all = [torch.zeros(B * n_rows, self.Lmax, H, D, device=device, dtype=BF) for _ in range(c.num_layers)]
            self.vc_all = [torch.zeros(B * n_rows, self.Lmax, H, D, device=device, dtype=BF) for _ in range(c.num_layers)]
            self.kc, self.vc = [t[:B] for t in self.kc_all], [t[:B] for t in self.vc_all]
        self.pos = torch.zeros(1, device=device, dtype=torch.int32)
        self.pos0 = torch.zeros(1, device=device, dtype=torch.int32)
        self.token = torch.zeros(1, device=device, dtype=torch.int64)
        self.sampled = torch.zeros(1, 1, device=device, dtype=torch.int64)
        self.out_tokens = torch.zeros(self.Lmax, device=device, dtype=torch.int64)
        self.out_count = torch.zeros(1, device=device, dtype=torch.int32)
        self.forced = torch.full((self.Lmax + 2,), -1, device=device, dtype=torch.int32)
        self.allowed = torch.zeros(self.Lmax + 2, 4, device=device, dtype=torch.int32)
        e = lambda *s, dt=BF: torch.empty(*s, device=device, dtype=dt)
        self.x = e(B, c.hidden)
        self.xn = e(B, c.hidden)
        self.qkv = e(B, 3 * c.hidden)
        self.qr = e(B, c.hidden)
        self.att = e(B, c.hidden)
        self.gate = e(B, c.mlp)
        self.lnf = e(B, c.hidden, dt=torch.float32)
        self.logits = e(B, c.vocab, dt=torch.float32)
        self.probs = e(1, c.vocab, dt=torch.float32)
        self.cfg_logits = e(1, c.vocab, dt=torch.float32)
        self.noise = e(1, c.vocab, dt=torch.float32)       # Exp(1) draws of the step's torch.multinomial (see _sample_and_advance)
        # LD_LLM_FUSED_TAIL=0 (read once): sampling through torch.multinomial + ld_llm_decode_advance + ld_llm_embed (13 + 3 launches)
        self.fused_tail = os.environ.get("LD_LLM_FUSED_TAIL", "1") != "0"
        self._x_from_tail = False                          # the sampling launch has left the next token's embedding in self.x
        # split-K decode attention: >= one workgroup per CU, and at most 256 keys per split (ld_llm_kv_attn)
        self.nsplit = max(1, 256 // (B * H), -(-self.Lmax // 256))
        self.top_k, self.top_p = None, None
        # partial results [B*H][nsplit][130] + B*H arrival counters (zero between launches: the last split to arrive merges)
        self.attn_ws = torch.zeros(B * H * (self.nsplit * 130 + 1), device=device, dtype=torch.float32)
        if multi:
            Pm, Bm = n_rows, B * n_rows
            self.m_x, self.m_qkv, self.m_att, self.m_gate = e(Bm, c.hidden), e(Bm, 3 * c.hidden), e(Bm, c.hidden), e(Bm, c.mlp)
            self.m_lnf, self.m_logits = e(Bm, c.hidden, dt=torch.float32), e(Bm, c.vocab, dt=torch.float32)
            self.m_cfg_logits, self.m_noise = e(Pm, c.vocab, dt=torch.float32), e(Pm, c.vocab, dt=torch.float32)
            self.m_pos = torch.zeros(Pm, device=device, dtype=torch.int32)        # one word per sample (all equal; word 0 is "the" position)
            self.m_token = torch.zeros(Pm, device=device, dtype=torch.int64)
            self.m_sampled = torch.zeros(Pm, device=device, dtype=torch.int64)
            self.m_out_tokens = torch.zeros(Pm, self.Lmax, device=device, dtype=torch.int64)
            self.m_out_count = torch.zeros(Pm, device=device, dtype=torch.int32)
            # same nsplit as the two-row decode (the split rule is part of the bits), workspace for all rows
            self.m_attn_ws = torch.zeros(Bm * H * (self.nsplit * 130 + 1), device=device, dtype=torch.float32)
        self._graph = None
        self._layer_table = None
        # Three forms of a decode step's blocks, identical bits (tests/variants/variant_cases.py):
        #   "chain"    one launch per operation on the current stream (5 per block) -- what the shipped library has;
        #   "chained"  the same launches alternating between two streams with device-side dependencies (every launch requests
        #              its first weight rows while its predecessor is still running; ld_llm_decode_blocks_chained);
        #   "fused"    all blocks in one persistent launch with grid barriers (ld_llm_fused.hip).
        # The last two were measured slower and live in the VARIANTS build of the library only (landiff_amd/_lib.py:
        # VARIANTS_LIB_PATH, selected with LANDIFF_HIP_LIB): asking for them on the shipped library raises.
        # "chained" and "fused" need the GPU to themselves (their workgroups wait for other workgroups): callers that decode
        # UNDER another stream's kernels (generate_many, the streaming loop) pass mode="chain".  LD_LLM_DECODE overrides the default.
        self.decode_mode = os.environ.get("LD_LLM_DECODE", "chain")
        assert self.decode_mode in ("chain", "chained", "fused"), self.decode_mode
        self.fused_supported = (B == 2 and c.head_dim == 128 and c.hidden <= 2048 and c.mlp <= 12288 and self.nsplit >= 2
                                and -(-self.Lmax // self.nsplit) <= 256)
        self.chained_supported = (B == 2 and c.head_dim == 128 and c.hidden <= 4096 and c.mlp <= 12288 and self.nsplit >= 2
                                  and -(-self.Lmax // self.nsplit) <= 256 and 5 * c.num_layers <= 256)
        self.fused_ctl = torch.zeros(ops.LLM_FUSED_CTL_WORDS, device=device, dtype=torch.int32)
        self.chain_ctl = torch.zeros(ops.LLM_CHAIN_CTL_WORDS, device=device, dtype=torch.int32)
        self._mode = "chain"               # the form the running decode uses
        self._layer_table_dev = None
        self._side = None                  # second stream + event of the chained form
        self._chain_ev = None
        self._chain_epoch = 0
        self._pos_host = -1                # host mirror of *pos, valid only inside sample()'s loop; -1: the kernels read *pos
        self._capturing = False

    # ---- conditioning ------------------------------------------------------------------------
    def _micro_cond(self, frames: float, motion_score: float):
        c, dev = self.cfg, self.dev
        out = torch.empty(2, c.hidden, device=dev, dtype=BF)
        t = torch.empty(1, device=dev, dtype=torch.float32)
        te = torch.empty(1, c.freq_dim, device=dev, dtype=BF)
        hid = torch.empty(1, c.micro_hidden, device=dev, dtype=BF)
        for r, (key, val) in enumerate((("frames", frames), ("motion_score", motion_score))):
            w0, b0, w2, b2 = self.micro[key]
            t.fill_(float(val))
            ops.timestep_embedding(t, te)
            ops.gemv(te, w0, hid, bias=b0)
            ops.gemv(hid, w2, out[r:r + 1], bias=b2, in_act="silu")
        return out

    def prefix_features(self, text_emb: torch.Tensor, frames: float, motion_score: float):
        """[BOS][frames][motion][text x n][START_I] for (cond, uncond) -> bf16 [2, n+4, hidden]."""
        c, dev = self.cfg, self.dev
        n = text_emb.shape[0]
        t = text_emb.to(dev, BF).contiguous()
        h = ops.gemm(t, self.fc0[0], bias=self.fc0[1], act="gelu_tanh")
        cond = ops.gemm(h, self.fc1[0], bias=self.fc1[1])
        micro = self._micro_cond(frames, motion_score)
        feats = torch.empty(2, n + 4, c.hidden, device=dev, dtype=BF)
        feats[:, 0] = self.emb[c.BOS].to(BF)
        feats[:, 1:3] = micro
        feats[0, 3:3 + n] = cond
        feats[1, 3:3 + n] = self.null_text
        feats[:, 3 + n] = self.emb[c.START_I].to(BF)
        return feats

    # ---- transformer ---------------------------------------------------------------------------
    def _prefill_blocks(self, feats: torch.Tensor):
        """Every block over all m positions of feats [2, m, hidden] from position 0 (KV rows [0, m) of the first pair's cache are
        written) -> the residual stream, bf16 [2 * m, hidden]."""
        c = self.cfg
        B, m, d = feats.shape
        M = B * m
        x = feats.reshape(M, d).contiguous()
        xn = torch.empty_like(x)
        qkv = torch.empty(M, 3 * d, device=self.dev, dtype=BF)
        qr = torch.empty(M, d, device=self.dev, dtype=BF)
        att = torch.empty(M, d, device=self.dev, dtype=BF)
        h3 = torch.empty(M, c.mlp, device=self.dev, dtype=BF)
        gate = torch.empty(M, c.mlp, device=self.dev, dtype=BF)
        self.pos0.zero_()
        for i, w in enumerate(self.blocks):
            ops.rmsnorm(x, w["n0"], xn, c.rms_eps)
            ops.gemm(xn, w["wqkv"], out=qkv)
            ops.llm_rope_append(qkv, self.cos, self.sin, self.pos0, qr, self.kc[i], self.vc[i], B, m, c.heads, self.Lmax)
            ops.llm_kv_attn(qr, self.kc[i], self.vc[i], self.pos0, att, B, m, c.heads, self.Lmax)
            ops.gemm(att, w["wo"], out=x, resid=x)
            ops.rmsnorm(x, w["n1"], xn, c.rms_eps)
            ops.gemm(xn, w["w3"], out=h3)
            ops.gemm(xn, w["w1"], out=gate, act="gelu_tanh", mul=h3)
            ops.gemm(gate, w["w2"], out=x, resid=x)
        return x

    def _prefill(self, feats: torch.Tensor):
        c = self.cfg
        B, m, d = feats.shape
        x = self._prefill_blocks(feats)
        last = x.view(B, m, d)[:, -1]                       # rows (b, m-1), stride m*d
        ops.layernorm_bf16_to_f32(last, self.ln_w, self.ln_b, self.lnf, c.ln_eps)
        ops.gemv(self.lnf, self.head, self.logits)

    def _decode_forward(self):
        """One token: embedding of *token at position *pos -> logits [2, V].  All sizes are static and every per-step scalar
        lives on the device; the ~125 launches are queued by ONE native call (ld_llm_decode_forward) -- issued one by one
        from Python the step was bound by the interpreter (1.3 ms of host time per step), and replaying it as a HIP graph
        costs 1.2 ms of host time per launch of the 164-node graph."""
        c = self.cfg
        if self._layer_table is None:
            self._layer_table = ops.llm_layer_table(self.blocks, self.kc, self.vc)
        if self._mode == "chained":
            s0 = torch.cuda.current_stream(self.dev)
            if not self._x_from_tail:
                ops.llm_embed(self.emb, self.token, self.x)
            ops.llm_decode_blocks_chained(self._layer_table, self._pos_host, self.x, self.qkv, self.att, self.gate, self.attn_ws,
                                          self.cos, self.sin, c.heads, self.Lmax, self.nsplit, c.rms_eps, self.chain_ctl,
                                          self._chain_epoch, s0, self._side)
            self._chain_epoch += 1
            self._chain_ev.record(self._side)              # the step's last operation may sit on either stream: the tail follows both
            s0.wait_event(self._chain_ev)
            ops.layernorm_bf16_to_f32(self.x, self.ln_w, self.ln_b, self.lnf, c.ln_eps)
            ops.gemv(self.lnf, self.head, self.logits)
            return
        if self._mode == "fused":
            if self._layer_table_dev is None:
                self._layer_table_dev = ops.llm_layer_table_device(self._layer_table, self.dev)
            ops.llm_decode_forward_fused(self._layer_table_dev, len(self.blocks), None if self._x_from_tail else self.emb, self.token,
                                         self.pos, self.x, self.qkv, self.att, self.gate, self.attn_ws, self.cos, self.sin,
                                         self.ln_w, self.ln_b, self.lnf, self.head, self.logits, c.heads, self.Lmax, self.nsplit,
                                         c.rms_eps, c.ln_eps, self.fused_ctl)
            return
        ops.llm_decode_forward(self._layer_table, None if self._x_from_tail else self.emb, self.token, self.pos, self.x, self.qkv, self.att, self.gate,
                               self.attn_ws, self.cos, self.sin, self.ln_w, self.ln_b, self.lnf, self.head, self.logits,
                               c.heads, self.Lmax, self.nsplit, c.rms_eps, c.ln_eps,
                               pos_value=-1 if self._capturing else self._pos_host)   # (a captured graph must read *pos itself)

    def _decode_forward_per_op(self):
        """The same step issued op by op through the C-ABI (kept for tests: must equal _decode_forward bit for bit)."""
        c, B = self.cfg, self.B
        ops.llm_embed(self.emb, self.token, self.x)
        for i, w in enumerate(self.blocks):      # 6 launches per layer: RMSNorm rides in the GEMVs, RoPE/append in attention
            ops.gemv(self.x, w["wqkv"], self.qkv, norm_w=w["n0"], norm_eps=c.rms_eps)
            ops.llm_kv_attn(None, self.kc[i], self.vc[i], self.pos, self.att, B, 1, c.heads, self.Lmax,
                            workspace=self.attn_ws, nsplit=self.nsplit, qkv_fused=self.qkv, cos_t=self.cos, sin_t=self.sin)
            ops.gemv(self.att, w["wo"], self.x, resid=self.x)
            ops.gemv(self.x, w["w1"], self.gate, w2=w["w3"], act="gelu_tanh", norm_w=w["n1"], norm_eps=c.rms_eps)
            ops.gemv(self.gate, w["w2"], self.x, resid=self.x)
        ops.layernorm_bf16_to_f32(self.x, self.ln_w, self.ln_b, self.lnf, c.ln_eps)
        ops.gemv(self.lnf, self.head, self.logits)

    def _sample_and_advance(self, guided, scale, temperature, generator):
        """lm_model.py:417-508: CFG / temperature / restriction / filters -> probabilities -> one multinomial draw -> forced-token
        schedule, token record, position advance.  torch.multinomial(p, 1, generator) is argmax(p / q) with
        q = empty_like(p).exponential_(1, generator) (ATen's own formula; its other ten launches are validity checks), so the
        draw is taken inside ld_llm_sample_advance from q drawn here with the same generator: the same token from the same
        generator state (tests/test_gpu_stages.py::test_fused_sampling_equals_torch_multinomial), in 2 launches instead of 16."""
        if self._x_from_tail:
            self.noise.exponential_(1.0, generator=generator)
            ops.llm_sample_advance(self.logits, self.probs, self.cfg_logits, guided, scale, temperature, self.pos, self.allowed,
                                   self.noise, self.forced, self.token, self.out_tokens, self.out_count, self.sampled, self.emb,
                                   self.x, top_k=self.top_k, top_p=self.top_p)
            return
        ops.llm_logits_to_probs(self.logits, self.probs, self.cfg_logits, guided, scale, temperature, self.pos, self.allowed,
                                top_k=self.top_k, top_p=self.top_p)
        torch.multinomial(self.probs, num_samples=1, generator=generator, out=self.sampled)
        ops.llm_decode_advance(self.sampled, self.forced, self.pos, self.token, self.out_tokens, self.out_count)

    def _decode_forward_many(self, P: int, pos_value: int, wide: bool = False, embed: bool = False):
        """_decode_forward for P samples (rows (2p, 2p+1) of the m_* buffers): the embedding rows of their tokens, left in m_x by
        the sampling launch, at position pos_value -> logits [2P, V]; one native call, every weight matrix streamed once.
        wide: the MFMA engine (ld_llm_decode_forward_wide).  embed: m_token was written by the host (teacher feeding): the step
        embeds it from the table instead of trusting m_x."""
        c, B = self.cfg, 2 * P
        if self._layer_table is None:
            self._layer_table = ops.llm_layer_table(self.blocks, self.kc, self.vc)      # (kc[i] is the head of kc_all[i]: same address)
        ops._llm_decode_forward("ld_llm_decode_forward_wide" if wide else "ld_llm_decode_forward_pairs", self._layer_table,
                                self.emb if embed else None, self.m_token[:P], self.m_pos[:P], self.m_x[:B], self.m_qkv[:B], self.m_att[:B],
                                self.m_gate[:B], self.m_attn_ws, self.cos, self.sin, self.ln_w, self.ln_b, self.m_lnf[:B], self.head,
                                self.m_logits[:B], c.heads, self.Lmax, self.nsplit, c.rms_eps, c.ln_eps, pos_value)

    def _sample_and_advance_many(self, gens, guided, scale, temperature, top_k=None, top_p=None, logits_log=None, wide=False):
        """_sample_and_advance for len(gens) samples: generator p draws the [vocab] Exp(1) row sample() draws from it at this
        step (and nothing else), then one launch samples, records and advances every sample and embeds its next token."""
        P = len(gens)
        noise, cfg_logits = self.m_noise[:P], self.m_cfg_logits[:P]
        for p in range(P):
            noise[p].exponential_(1.0, generator=gens[p])
        ops._llm_sample_advance_many("ld_llm_sample_advance_wide" if wide else "ld_llm_sample_advance_pairs", self.m_logits[:2 * P], None,
                                     cfg_logits, guided, scale, temperature, self.m_pos[:P], self.allowed, noise, self.forced,
                                     self.m_token[:P], self.m_out_tokens[:P], self.m_out_count[:P], self.m_sampled[:P], self.emb,
                                     self.m_x[:2 * P], top_k=top_k, top_p=top_p)
        if logits_log is not None:
            logits_log.append(cfg_logits.clone())

    def _decode_plan(self, text_emb, motion_score, num_frames, first_frame_tokens, prefix_tokens):
        """What sample() / sample_many() do before the prefill: the prefix features (with the given first frame / first segment
        appended), the forced / restricted schedule uploaded to the device tables.
        -> (feats, S_last = position of the last prefilled token, full_len, forced, n_visual still to sample, n_prefix)."""
        c, dev = self.cfg, self.dev
        feats = self.prefix_features(text_emb, float(num_frames), motion_score)
        S = feats.shape[1] - 1
        full_len, forced, restricted, n_visual = forced_token_schedule(c, S, num_frames)
        if full_len > self.Lmax:
            raise ValueError(f"LLM decode of {num_frames} frames after {text_emb.shape[-2]} text tokens needs {full_len} positions; this runner "
                             f"was built for {self.Lmax} (max_text / max_frames of LLMRunner; the reference's T5 tokenizer truncates at 512)")
        S_last = S                                         # position of the last prefilled token
        if first_frame_tokens is not None:
            assert num_frames > 1 and first_frame_tokens.numel() == c.iframe_len, "first_frame_tokens: one I frame, more frames to sample"
            ids = torch.cat([first_frame_tokens.reshape(-1).to(dev, torch.int64),
                             torch.tensor([c.END_I, c.START_P], device=dev, dtype=torch.int64)])
            assert forced[S + 1 + c.iframe_len] == c.END_I and forced[S + 2 + c.iframe_len] == c.START_P
            feats = torch.cat([feats, self.emb[ids].to(BF)[None].expand(2, -1, -1)], 1)
            S_last = S + c.iframe_len + 2
            n_visual -= c.iframe_len
        n_prefix = 0
        if prefix_tokens is not None:
            assert first_frame_tokens is None, "prefix_tokens already holds the first I frame"
            block = c.iframe_len + (c.segment_length - 1) * c.pframe_len + 2 * c.segment_length
            if full_len - 1 <= S + block:
                raise ValueError("prefix_tokens: one whole segment, and at least one more segment to sample")
            tmpl = torch.tensor([forced.get(q, -1) for q in range(S + 1, S + block + 1)], dtype=torch.int64)
            slots = tmpl < 0
            vis = prefix_tokens.reshape(-1).to(dev, torch.int64)
            if vis.numel() != int(slots.sum()):
                raise ValueError(f"prefix_tokens: {vis.numel()} ids, a segment holds {int(slots.sum())}")
            ids = tmpl.to(dev)
            ids[slots.to(dev)] = vis
            feats = torch.cat([feats, self.emb[ids].to(BF)[None].expand(2, -1, -1)], 1)
            S_last = S + block
            n_prefix = vis.numel()
            n_visual -= n_prefix
        ft = torch.full((self.Lmax + 2,), -1, dtype=torch.int32)
        al = torch.zeros(self.Lmax + 2, 4, dtype=torch.int32)
        for p, t in forced.items():
            ft[p] = t
        for p, ids in restricted.items():
            al[p, 0] = len(ids)
            al[p, 1:1 + len(ids)] = torch.tensor(ids, dtype=torch.int32)
        self.forced.copy_(ft); self.allowed.copy_(al)
        return feats, S_last, full_len, forced, n_visual, n_prefix

    def _segment_notifier(self, on_segment, segment_tokens, forced, first_frame_tokens, prefix_tokens):
        """-> note(pos), called when the token of position pos has just been queued (for every sample): on_segment(s) fires after
        the last of every `segment_tokens` positions the schedule leaves free."""
        assert on_segment is None or (segment_tokens and first_frame_tokens is None and prefix_tokens is None)
        emitted = 0
        def note(pos):
            nonlocal emitted
            if on_segment is None or pos in forced:
                return
            emitted += 1
            if emitted % segment_tokens == 0:
                on_segment(emitted // segment_tokens - 1)
        return note

    def _assemble_ids(self, out, prefix_tokens, first_frame_tokens, lp_steps, S_last, full_len, forced):
        """out int64 [P, n]: the sampled ids -> the given prefix_tokens / first_frame_tokens in front of every row, clamped
        (lm_model.py:509-516); with lp_steps: (ids, logprobs [P, sampled positions])."""
        head = [t.reshape(1, -1).to(self.dev, torch.int64).expand(out.shape[0], -1) for t in (prefix_tokens, first_frame_tokens) if t is not None]
        if head:
            out = torch.cat(head + [out], 1)
        out = out.clamp(0, self.cfg.visual_vocab - 1)
        if lp_steps is None:
            return out
        return out, self._gather_logprobs(lp_steps, S_last, full_len, forced)

    # ---- decode loop -----------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, text_emb: torch.Tensor, *, motion_score: float = 0.1, num_frames: int = 13, guidance_scale: float = 7.5,
               temperature: float = 1.0, seed: int | None = None, generator=None, use_graph: bool = False,
               teacher_fed=None, logits_log=None, top_k: int | None = None, top_p: float | None = None,
               first_frame_tokens: torch.Tensor | None = None, on_segment=None, segment_tokens: int | None = None,
               mode: str | None = None, prefix_tokens: torch.Tensor | None = None, return_logprobs: bool = False):
        """Returns the clamped visual token ids, int64 [n_visual] on the device (lm_model.py:509-516).
        return_logprobs: -> (ids, logprobs): fp32 [n_visual], the log-probability of every SAMPLED id.  With first_frame_tokens /
        prefix_tokens the given ids are not draws and have none: logprobs then covers ids[-logprobs.numel():] only, it is SHORTER
        than ids under the guided, restricted, filtered distribution it
        was drawn from -- one ld_llm_token_logprobs launch per step on the step's own logits; the ids are those of the call
        without the flag.  "chain" form only: refused with use_graph, another mode or teacher_fed.
        top_k / top_p filter the unrestricted positions inside the sampling kernel (lm_model.py:441-447).
        first_frame_tokens (int64 [iframe_len], e.g. from TokenizerEncoder.encode_to_index): use_gt_first_frame of the
        reference (lm_model.py:332-352) -- the given I-frame tokens, END_OF_IFrame and the first START_OF_PFrame join the
        prefilled prefix, sampling (and the RNG stream) starts at the first P token, the result begins with the given ids.
        prefix_tokens (int64 [num_latent_tokens]: one whole segment, e.g. the .npy llm_infer saves next to a video): the same
        for the first segment of a multi-segment decode -- its ids, with the markers forced_token_schedule puts between them,
        and the next segment's START_OF_IFrame join the prefilled prefix; sampling starts at that segment's first I token.
        on_segment(s): called on the host right after the step that emits the last of every `segment_tokens` visual tokens
        has been QUEUED (tokens [s * segment_tokens, (s + 1) * segment_tokens) of self.out_tokens are then final in stream
        order) -- lets a streaming caller start on segment s while later segments are still being decoded."""
        c, dev = self.cfg, self.dev
        self.top_k, self.top_p = top_k, top_p
        # mode: the form of a decode step's blocks ("chain" / "chained" / "fused", see __init__; None: the runner's default);
        # an unsupported shape falls back to "chain"
        mode = self.decode_mode if mode is None else mode
        assert mode in ("chain", "chained", "fused"), mode
        if return_logprobs and (use_graph or mode != "chain" or teacher_fed is not None):
            raise ValueError("sample: return_logprobs needs the per-operation 'chain' form without graph capture or teacher feeding "
                             f"(use_graph={use_graph}, mode={mode!r}, teacher_fed {'given' if teacher_fed is not None else 'None'})")
        if mode != "chain" and not _lib.has_variants():
            raise _lib.LandiffHipError(f"decode mode {mode!r} needs the variants build of the library (LD_BUILD_VARIANTS=1 "
                                       f"landiff_amd/csrc/build.sh, then LANDIFF_HIP_LIB={_lib.VARIANTS_LIB_PATH}); the shipped library "
                                       "has the per-operation chain only")
        if (mode == "fused" and not self.fused_supported) or (mode == "chained" and (not self.chained_supported or use_graph)):
            mode = "chain"
        self._mode = mode
        guided = guidance_scale > 0 and guidance_scale != 1
        # unguided (ARSampleCfg's dataclass default cfg=0.0, lm_model.py:311-319): the conditional row is independent of the
        # second row, so the resident two-row buffers are kept and the sampling kernel reads row 0 only.
        feats, S_last, full_len, forced, n_visual, _ = self._decode_plan(text_emb, motion_score, num_frames, first_frame_tokens,
                                                                                prefix_tokens)
        self._x_from_tail = self.fused_tail and teacher_fed is None          # (a teacher-fed token is written by the host: re-embed it)
        self.out_count.zero_()
        if generator is None and seed:
            generator = torch.Generator(device=dev)
            generator.manual_seed(seed)                     # lm_model.py:398-402
        note_position = self._segment_notifier(on_segment, segment_tokens, forced, first_frame_tokens, prefix_tokens)
        self._prefill(feats)
        self.pos.fill_(S_last)
        self._sample_and_advance(guided, guidance_scale, temperature, generator)
        lp_steps = None
        if return_logprobs:
            lp_steps = torch.empty(full_len - (S_last + 1), 1, device=dev, dtype=torch.float32)      # one row per generated position
            self._step_logprobs(self.logits[0:1], self.logits[1:2], self.sampled.view(1), self.pos, lp_steps[0], guided,
                                guidance_scale, temperature, top_k, top_p)
        try:                               # from here on the host-side position is live: the finally below always retires it
            self._pos_host = S_last + 1
            if self._mode == "fused":
                self.fused_ctl.zero_()
            elif self._mode == "chained":
                if self._side is None:
                    self._side = torch.cuda.Stream(device=dev)
                    self._chain_ev = torch.cuda.Event()
                self.chain_ctl.zero_()
                self._chain_epoch = 0
                self._side.wait_stream(torch.cuda.current_stream(dev))      # the prefill's KV cache and the zeroed counters
            note_position(S_last + 1)
            if logits_log is not None:
                logits_log.append(self.cfg_logits.clone())
            steps = full_len - (S_last + 1) - 1
            debug = teacher_fed is not None or logits_log is not None
            graph = None
            if use_graph and not debug and steps > 4:
                graph = self._capture(guided, guidance_scale, temperature, generator)
            t_enq = time.perf_counter()
            for it in range(steps):
                if teacher_fed is not None:
                    self.token.copy_(teacher_fed[it].reshape(1))
                if graph is not None:
                    graph.replay()
                else:
                    self._decode_forward()
                    self._sample_and_advance(guided, guidance_scale, temperature, generator)
                    self._pos_host += 1
                    if lp_steps is not None:
                        self._step_logprobs(self.logits[0:1], self.logits[1:2], self.sampled.view(1), self.pos, lp_steps[it + 1],
                                            guided, guidance_scale, temperature, top_k, top_p)
                note_position(S_last + 2 + it)
                if logits_log is not None:
                    logits_log.append(self.cfg_logits.clone())
                if self._mode != "chain" and (it & 63) == 63:
                    self._raise_on_wait_timeout()          # opt-in forms only: one host sync per 64 steps instead of ~1244 steps on garbage
        finally:
            self._pos_host = -1            # any other caller of _decode_forward gets the device-side position
        self.host_enqueue_s = time.perf_counter() - t_enq      # host time to enqueue the loop (< wall time when the GPU is the bound)
        self._raise_on_wait_timeout()
        assert int(self.out_count.item()) == n_visual, (int(self.out_count.item()), n_visual)
        res = self._assemble_ids(self.out_tokens[None, :n_visual], prefix_tokens, first_frame_tokens, lp_steps, S_last, full_len, forced)
        return (res[0][0], res[1][0]) if lp_steps is not None else res[0]

    def _step_logprobs(self, cond, uncond, sampled, pos, out, guided, scale, temperature, top_k, top_p):
        """The log-probabilities of the tokens the sampling launch just drew, from the logits it read (the next forward has not
        been queued yet).  That launch has advanced the position words: bias -1 names the position it sampled at."""
        ops.llm_token_logprobs(cond, uncond, sampled, out, guided, scale, temperature, pos=pos, pos_stride=1 if pos.numel() > 1 else 0,
                               pos_bias=-1, allowed=self.allowed, forced=self.forced, top_k=top_k, top_p=top_p)

    def _gather_logprobs(self, lp_steps, S_last, full_len, forced):
        """lp_steps [generated positions, P] -> [P, sampled positions]: the rows of the positions the schedule leaves free."""
        free = torch.tensor([q not in forced for q in range(S_last + 1, full_len)], dtype=torch.bool, device=self.dev)
        return lp_steps[free].t().contiguous()

    @torch.no_grad()
    def score(self, text_emb: torch.Tensor, tokens, *, motion_score: float = 0.1, num_frames: int = 13, guidance_scale: float = 7.5,
              temperature: float = 1.0, top_k: int | None = None, top_p: float | None = None):
        """Teacher forcing in one pass: the log-probability of every id of `tokens` (int [n_visual], what sample() returns for
        this text length and num_frames) under the distribution sample() with these keywords draws that position from, given the
        ids before it -> (logprobs fp32 [n_visual] on the device, their sum as a float).  -inf where the filters remove an id.
        The ids are laid into the free slots of the forced-token schedule; one prefill-form pass (bf16 GEMMs) runs over all
        full_len - 1 positions of the (cond, uncond) pair, then the final LayerNorm, the fp32 head (ld_llm_head_f32) and ONE
        ld_llm_token_logprobs launch over the rows that predict a generated position.  Overwrites the runner's KV cache and
        schedule tables, as a sample() does.  Decode steps compute the same logits through GEMVs, which round differently: the
        online log-probabilities of sample(return_logprobs=True) agree with score() of its ids to bf16 noise, not bit for bit."""
        c, dev = self.cfg, self.dev
        S = text_emb.shape[-2] + 3                          # position of the first START_OF_IFrame (prefix_features)
        full_len, forced, _, n_visual = forced_token_schedule(c, S, num_frames)
        if full_len > self.Lmax:
            raise ValueError(f"LLM score of {num_frames} frames after {text_emb.shape[-2]} text tokens needs {full_len} positions; this runner "
                             f"was built for {self.Lmax} (max_text / max_frames of LLMRunner)")
        tok = torch.as_tensor(tokens).reshape(-1)
        if tok.is_floating_point() or tok.dtype == torch.bool:
            raise TypeError(f"score: tokens must be integer ids, got {tok.dtype}")
        if tok.numel() != n_visual:
            raise ValueError(f"score: {tok.numel()} ids, {num_frames} frames hold {n_visual}")
        if n_visual and (int(tok.min()) < 0 or int(tok.max()) >= c.visual_vocab):
            raise ValueError(f"score: ids outside [0, {c.visual_vocab}) (min {int(tok.min())}, max {int(tok.max())})")
        guided = guidance_scale > 0 and guidance_scale != 1
        feats, _, _, _, _, _ = self._decode_plan(text_emb, motion_score, num_frames, None, None)
        # ids of positions S + 1 .. full_len - 1: the schedule's forced tokens with the given ids in the free slots
        tmpl = torch.tensor([forced.get(q, -1) for q in range(S + 1, full_len)], dtype=torch.int64)
        slots = (tmpl < 0).to(dev)
        ids = tmpl.to(dev)
        ids[slots] = tok.to(dev, torch.int64)
        feats = torch.cat([feats, self.emb[ids[:-1]].to(BF)[None].expand(2, -1, -1)], 1)      # positions 0 .. full_len - 2
        m, nr = full_len - 1, full_len - 1 - S              # rows S .. m - 1 predict positions S + 1 .. full_len - 1
        xv = self._prefill_blocks(feats).view(2, m, c.hidden)
        lnf = torch.empty(2, nr, c.hidden, device=dev, dtype=torch.float32)
        for b in range(2):
            ops.layernorm_bf16_to_f32(xv[b, S:], self.ln_w, self.ln_b, lnf[b], c.ln_eps)
        logits = torch.empty(2 * nr, c.vocab, device=dev, dtype=torch.float32)
        ops.llm_head_f32(lnf.view(2 * nr, c.hidden), self.head, logits)
        lp = torch.empty(nr, device=dev, dtype=torch.float32)
        ops.llm_token_logprobs(logits[:nr], logits[nr:], ids, lp, guided, guidance_scale, temperature, pos_bias=S,
                               allowed=self.allowed, forced=self.forced, top_k=top_k, top_p=top_p)
        out = lp[slots]
        return out, float(out.double().sum().item())

    @torch.no_grad()
    def sample_many(self, text_emb: torch.Tensor, seeds, *, motion_score: float = 0.1, num_frames: int = 13, guidance_scale: float = 7.5,
                    temperature: float = 1.0, use_graph: bool = False, teacher_fed=None, logits_log=None, top_k: int | None = None,
                    top_p: float | None = None, first_frame_tokens: torch.Tensor | None = None, on_segment=None,
                    segment_tokens: int | None = None, mode: str | None = None, prefix_tokens: torch.Tensor | None = None,
                    return_logprobs: bool = False, engine: str = "gemv"):
        """len(seeds) samples of ONE prompt from one weight stream: int64 [P, n_visual], row p exactly the ids
        sample(..., seed=seeds[p]) returns.  The samples share the text, the motion score and any first_frame_tokens /
        prefix_tokens, hence the prefill (run once for the (cond, uncond) pair, its KV rows and first logits copied to the other
        pairs), the position and the forced / restricted schedule; each has its own torch.Generator seeded as sample() seeds it
        and drawing only its own noise row per step, its own token, KV rows and output row.  A step is one
        ld_llm_decode_forward_pairs (every weight matrix streamed once for all 2P rows) and one ld_llm_sample_advance_pairs.
        The per-operation "chain" form only, no graph capture, no teacher feeding.  Keywords as sample(); logits_log receives
        [P, vocab] per step; on_segment(s) fires when segment s of EVERY sample is queued (self.m_out_tokens[p]).
        return_logprobs: -> (ids, logprobs fp32 [P, sampled positions]), row p what sample(seed=seeds[p], return_logprobs=True)
        returns: one more launch per step (ld_llm_token_logprobs over the P pairs), the ids unchanged.
        engine="mfma" (opt-in; "gemv" is everything above, launch for launch): up to wide_samples (<= 16) samples per weight
        stream on the MFMA engine -- a step is one ld_llm_decode_forward_wide (block GEMVs: ld_gemv_wide; head: ld_llm_head_f32)
        and one ld_llm_sample_advance_wide.  An MFMA sums K in another order than the register GEMV, so row p is NOT bit for
        bit sample(seed=seeds[p]).  Its contract: (1) batch invariance, bit for bit -- what seed s gets depends on s and the
        prompt alone, not on P, its row or the other seeds; (2) the GEMV path's rounding points; (3) the ids equal those of
        sample(seed=s) up to the first step at which a rounding difference of the logits flips a near-tie of the draw
        (tests/flip_audit.py).  teacher_fed (this engine only): int64 [steps] (every sample) or [P, steps]: the host writes the
        fed token of each step into every sample's token word and the step re-embeds it from the table."""
        c, dev = self.cfg, self.dev
        seeds = [int(s) for s in seeds]
        P = len(seeds)
        if engine not in ("gemv", "mfma"):
            raise ValueError(f"sample_many: unknown engine {engine!r} ('gemv': register GEMV, bit-identical to sample(); 'mfma': "
                             "ld_gemv_wide, up to 16 samples)")
        wide = engine == "mfma"
        mode = "chain" if mode is None else mode
        if mode != "chain":
            raise ValueError(f"sample_many: decode mode {mode!r} is not supported (the batched decode is the per-operation 'chain' form)")
        if use_graph:
            raise ValueError("sample_many: graph capture is not supported")
        if teacher_fed is not None and not wide:
            raise ValueError("sample_many: teacher_fed is not supported (teacher forcing has one token stream)")
        if wide and not 1 <= P <= self.wide_samples:
            raise ValueError(f"sample_many(engine='mfma'): {P} seeds, this runner was built with wide_samples={self.wide_samples} "
                             f"(LLMRunner(..., wide_samples=N), N <= {ops.LLM_MAX_WIDE})")
        if not wide and not 1 <= P <= self.max_samples:
            raise ValueError(f"sample_many: {P} seeds, this runner was built with max_samples={self.max_samples} "
                             f"(LLMRunner(..., max_samples=N), N <= {ops.LLM_MAX_PAIRS})")
        if not all(seeds):
            raise ValueError("sample_many needs a non-zero seed per sample (sample() draws a zero seed from the shared default generator)")
        if return_logprobs and teacher_fed is not None:
            raise ValueError("sample_many: return_logprobs scores draws; a teacher-fed decode has none")
        fed = None
        if teacher_fed is not None:
            fed = torch.as_tensor(teacher_fed).to(dev, torch.int64)
            if fed.dim() == 1:
                fed = fed[None].expand(P, -1)
            if fed.dim() != 2 or fed.shape[0] != P:
                raise ValueError(f"sample_many: teacher_fed must be int64 [steps] or [{P}, steps], got {tuple(fed.shape)}")
            fed = fed.t().contiguous()                      # [steps, P]: one row per step
        if not wide and self.max_samples == 1:
            r = self.sample(text_emb, motion_score=motion_score, num_frames=num_frames, guidance_scale=guidance_scale,
                            temperature=temperature, seed=seeds[0], logits_log=logits_log, top_k=top_k, top_p=top_p,
                            first_frame_tokens=first_frame_tokens, on_segment=on_segment, segment_tokens=segment_tokens,
                            mode="chain", prefix_tokens=prefix_tokens, return_logprobs=return_logprobs)
            return (r[0][None], r[1][None]) if return_logprobs else r[None]
        self._mode = "chain"
        guided = guidance_scale > 0 and guidance_scale != 1
        feats, S_last, full_len, forced, n_visual, _ = self._decode_plan(text_emb, motion_score, num_frames, first_frame_tokens,
                                                                                prefix_tokens)
        gens = []
        for s in seeds:
            g = torch.Generator(device=dev)
            g.manual_seed(s)                                # lm_model.py:398-402, once per sample
            gens.append(g)
        B = 2 * P
        out_tokens, out_count = self.m_out_tokens[:P], self.m_out_count[:P]
        lp_steps = None
        if return_logprobs:
            lp_steps = torch.empty(full_len - (S_last + 1), P, device=dev, dtype=torch.float32)      # one row per generated position
            pairs = self.m_logits[:B].view(P, 2 * c.vocab)                                       # row p = (cond, uncond) of sample p
        def sample_and_advance(k=0):
            self._sample_and_advance_many(gens, guided, guidance_scale, temperature, top_k, top_p, logits_log, wide)
            if lp_steps is not None:
                self._step_logprobs(pairs[:, :c.vocab], pairs[:, c.vocab:], self.m_sampled[:P], self.m_pos[:P], lp_steps[k], guided,
                                    guidance_scale, temperature, top_k, top_p)

        note_position = self._segment_notifier(on_segment, segment_tokens, forced, first_frame_tokens, prefix_tokens)
        out_count.zero_()
        self.m_attn_ws.zero_()             # (its counter words sit where another P's partial results were)
        self._prefill(feats)
        n_pre = S_last + 1                 # prefilled positions
        for cache in self.kc_all + self.vc_all:
            for p in range(1, P):
                cache[2 * p:2 * p + 2, :n_pre].copy_(cache[:2, :n_pre])
        self.m_logits[:B].view(P, 2, c.vocab).copy_(self.logits[None].expand(P, -1, -1))
        self.m_pos.fill_(S_last)
        sample_and_advance()
        note_position(S_last + 1)
        steps = full_len - (S_last + 1) - 1
        t_enq = time.perf_counter()
        if fed is not None and fed.shape[0] < steps:
            raise ValueError(f"sample_many: teacher_fed holds {fed.shape[0]} steps, the decode runs {steps}")
        for it in range(steps):
            if fed is not None:
                self.m_token[:P].copy_(fed[it])
            self._decode_forward_many(P, S_last + 1 + it, wide, embed=fed is not None)
            sample_and_advance(it + 1)
            note_position(S_last + 2 + it)
        self.host_enqueue_s = time.perf_counter() - t_enq
        counts = out_count.tolist()
        assert counts == [n_visual] * P, (counts, n_visual)
        return self._assemble_ids(out_tokens[:, :n_visual], prefix_tokens, first_frame_tokens, lp_steps, S_last, full_len, forced)

    def _raise_on_wait_timeout(self):
        """The 'fused' and 'chained' forms spin-wait on other workgroups without a cooperative launch; a wait that gives up sets a
        device flag.  After that the barrier counters are out of step and the KV cache holds rows computed from stale inputs: the
        runner must not be used for another decode step before the next sample() (which re-zeroes the control words and prefills)."""
        if (self._mode == "fused" and int(self.fused_ctl[1].item()) != 0) or (self._mode == "chained" and int(self.chain_ctl[0].item()) != 0):
            raise RuntimeError(f"LLM decode ({self._mode}): a device-side wait timed out (the decode did not have the GPU to itself?); "
                               "the KV cache of this decode is invalid; rerun with mode='chain' / LD_LLM_DECODE=chain")

    def _capture(self, guided, scale, temperature, generator):
        """Capture one decode step (forward + sampling + advance) into a HIP graph."""
        g = torch.cuda.CUDAGraph()
        if generator is not None:
            g.register_generator_state(generator)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        self._capturing = True
        try:
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    self._decode_forward()
                    self._sample_and_advance(guided, scale, temperature, generator)
        finally:
            self._capturing = False
        torch.cuda.current_stream().wait_stream(s)
        return g
