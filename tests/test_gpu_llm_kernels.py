"""The kernels of landiff_amd/csrc/ld_llm_attn.hip, ld_llm_sample.hip and ld_llm.hip that the AR model's prefill runs, and the small
ones around every step, each against a
plain torch reference of its own -- the model-level tests reach them only through the last row's CFG logits after 2 to 24 blocks
(err < max(2 x bf16-oracle floor, 2e-2)), a bound that a missing bf16 rounding, a key too many, a position off by one for j > 0, a
wrong head stride at H != 16 or a one-pass variance all stay inside.

  * ld_llm_rope_append (m > 1, *pos != 0): bit for bit against the fp32 restatement of apply_rope (pos_emb.py:16-46);
  * ld_llm_kv_attn, the unsplit kernel (m > 1 causal, m == 1 with an explicit q): against the same-dtype-flow restatement of
    transformer_blocks.py:166-186 and against fp32 attention; causality by bit-identity; the LDS guard of the launcher;
  * ld_rmsnorm_bf16 against fp64 (transformer_blocks.py:35-40), within one bf16 rounding and >= 99 % correctly rounded;
  * ld_layernorm_bf16_to_f32, the register kernel and the three-pass kernel, against fp64 F.layer_norm;
  * ld_llm_embed bit for bit; ld_llm_logits_to_probs at a restricted position (lm_model.py:417-454).

The ld_llm*.hip files are built with -ffp-contract=off -fno-slp-vectorize, so their plain fp32 arithmetic can be restated in torch bit for bit.
Output and cache buffers start as NaN (or a known bit pattern) and bf16 tensors are compared as int16, so that a stray write shows."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

D = 128
NAN = float("nan")


def _bits(t):
    """bf16 tensor -> its int16 bit patterns on the CPU (NaN == NaN, -0 != +0)."""
    assert t.dtype == torch.bfloat16
    return t.detach().cpu().contiguous().view(torch.int16)


def _dev_pos(cuda, pos):
    return torch.tensor([pos], device=cuda, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------
# 1. ld_llm_rope_append
# ------------------------------------------------------------------------------------------------
def _rope_fp32(x, cos, sin):
    """apply_rope (pos_emb.py:16-46) on x [B, m, H, D] with per-token factors cos / sin [m, D/2]: fp32 products, one fp32
    difference / sum, ONE rounding to bf16."""
    xf = x.float().reshape(*x.shape[:-1], D // 2, 2)
    a, b = xf[..., 0], xf[..., 1]
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    return torch.stack([a * c - b * s, a * s + b * c], dim=-1).flatten(-2).to(torch.bfloat16)


@pytest.mark.parametrize("pos", [0, 37])
@pytest.mark.parametrize("B,m,H", [(1, 1, 3), (2, 5, 16), (2, 67, 3), (1, 130, 16)])
def test_rope_append_bit_exact_at_offset_positions(cuda, B, m, H, pos):
    """q_out and the K cache rows [pos, pos + m) are the rotation by the factors of position pos + j, bit for bit; the V rows are
    the input v; every other cache row keeps its initial bit pattern.  Every (batch row, token, head, q/k/v) carries its own
    offset, so that a mix-up of heads or tokens cannot cancel."""
    from landiff_amd import ops
    from oracle.llm import rope_table
    Lmax = pos + m + 3
    g = torch.Generator().manual_seed(1000 * m + 10 * H + pos)
    cos, sin = rope_table(D, Lmax, 10000.0)
    qkv = torch.randn(B, m, 3, H, D, generator=g)
    qkv += (torch.arange(H).float() * 0.25)[None, None, None, :, None] + (torch.arange(m).float() * 0.01)[None, :, None, None, None]
    qkv += (torch.arange(3).float() * 0.125)[None, None, :, None, None] + (torch.arange(B).float() * 0.5)[:, None, None, None, None]
    qkv = qkv.to(torch.bfloat16)
    # the caches start as a bit pattern that differs from slot to slot
    pat = lambda mul: ((torch.arange(B * Lmax * H * D, dtype=torch.int64) * mul) % 30011 + 1).to(torch.int16).reshape(B, Lmax, H, D)
    kc0, vc0 = pat(7), pat(13)
    kc = kc0.clone().view(torch.bfloat16).to(cuda)
    vc = vc0.clone().view(torch.bfloat16).to(cuda)
    q_out = torch.full((B, m, H, D), NAN, device=cuda, dtype=torch.bfloat16)
    ops.llm_rope_append(qkv.to(cuda), cos.to(cuda).contiguous(), sin.to(cuda).contiguous(), _dev_pos(cuda, pos), q_out, kc, vc,
                        B, m, H, Lmax)
    torch.cuda.synchronize()
    q_ref = _rope_fp32(qkv[:, :, 0], cos[pos:pos + m], sin[pos:pos + m])
    k_ref = _rope_fp32(qkv[:, :, 1], cos[pos:pos + m], sin[pos:pos + m])
    assert not torch.isnan(q_ref.float()).any()
    assert torch.equal(_bits(q_out), _bits(q_ref))
    kb, vb = _bits(kc), _bits(vc)
    assert torch.equal(kb[:, pos:pos + m], _bits(k_ref))
    assert torch.equal(vb[:, pos:pos + m], _bits(qkv[:, :, 2]))
    assert torch.equal(kb[:, :pos], kc0[:, :pos]) and torch.equal(kb[:, pos + m:], kc0[:, pos + m:])
    assert torch.equal(vb[:, :pos], vc0[:, :pos]) and torch.equal(vb[:, pos + m:], vc0[:, pos + m:])


# ------------------------------------------------------------------------------------------------
# 2. ld_llm_kv_attn, the unsplit kernel
# ------------------------------------------------------------------------------------------------
ATTN_B = 2
ATTN_CASES = [(1, 0), (1, 44), (2, 0), (17, 0), (67, 45), (300, 0), (255, 2)]
# max |got - ref| / max |fp32 ref|, as in tests/test_gpu_llm_longctx.py.  That test's 6e-3 against the same-dtype-flow restatement
# belongs to the split path, which keeps p in fp32 (it measures 4.64e-3 here at L = 45).  ld_kv_attn_kernel rounds p to bf16 as
# the restatement does: its worst measured value over ATTN_CASES x H is 1.546e-3, under a third of 6e-3, so its bound is 3 x that
# worst value.  (With the bf16 rounding of p removed from the kernel it measures up to 6.2e-3 and three cases exceed the bound.)
BOUND_SAME_FLOW_SPLIT = 6e-3
BOUND_SAME_FLOW = 3 * 1.546e-3
BOUND_FP32 = 3e-2


@functools.lru_cache(maxsize=None)
def _attn_case(H, m, pos):
    """Inputs of one attention case (CPU): q [B, m, H, D] bf16 scaled by 1.5, caches [B, Lmax, H, D] bf16 with random rows
    [0, pos + m) and NaN behind them.  Cached: the reference tests and the causality test share them; nobody writes to them."""
    L, Lmax = pos + m, pos + m + 5
    g = torch.Generator().manual_seed(7 + 1000 * m + 10 * pos + H)
    q = (torch.randn(ATTN_B, m, H, D, generator=g) * 1.5).to(torch.bfloat16)
    kc = torch.randn(ATTN_B, Lmax, H, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(ATTN_B, Lmax, H, D, generator=g).to(torch.bfloat16)
    kc[:, L:] = NAN
    vc[:, L:] = NAN
    return q, kc, vc


def _attn_refs(q, kc, vc, pos):
    """(i) the dtype flow of transformer_blocks.py:166-186 on bf16 tensors -- scores -> bf16, x 1/sqrt(128) -> bf16, causal mask,
    fp32 softmax, p -> bf16, fp32 PV, bf16 out -- and (ii) plain fp32 attention.  Query j sits at position pos + j."""
    m = q.shape[1]
    L = pos + m
    qf, K, V = q.float(), kc[:, :L].float(), vc[:, :L].float()
    s = torch.einsum("bjhd,blhd->bhjl", qf, K)
    hidden = torch.arange(L)[None, :] > (pos + torch.arange(m))[:, None]          # [m, L]: keys behind the query's position
    s16 = (s.to(torch.bfloat16).float() * (1.0 / D ** 0.5)).to(torch.bfloat16).float().masked_fill(hidden, -float("inf"))
    p16 = torch.softmax(s16, -1).to(torch.bfloat16).float()
    ref16 = torch.einsum("bhjl,blhd->bjhd", p16, V).to(torch.bfloat16).float()
    s32 = (s / D ** 0.5).masked_fill(hidden, -float("inf"))
    ref32 = torch.einsum("bhjl,blhd->bjhd", torch.softmax(s32, -1), V)
    return ref16, ref32


def _attn_errors(out, ref16, ref32):
    got = out.float().cpu().reshape(ref32.shape)
    assert torch.isfinite(got).all()
    scale = ref32.abs().max().item()
    return (got - ref16).abs().max().item() / scale, (got - ref32).abs().max().item() / scale


def _run_unsplit(cuda, q, kc, vc, pos, H):
    from landiff_amd import ops
    B, m = q.shape[:2]
    Lmax = kc.shape[1]
    out = torch.full((B, m, H * D), NAN, device=cuda, dtype=torch.bfloat16)
    ops.llm_kv_attn(q.to(cuda), kc.to(cuda), vc.to(cuda), _dev_pos(cuda, pos), out, B, m, H, Lmax)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("m,pos", ATTN_CASES)
@pytest.mark.parametrize("H", [3, 16])
def test_kv_attn_unsplit_vs_torch(cuda, H, m, pos):
    """ld_kv_attn_kernel (causal over m query rows, scores in LDS, p rounded to bf16) against the same-dtype-flow restatement (i)
    and fp32 attention (ii), error = max abs difference / max |fp32 reference|, bounds as for the split path in
    tests/test_gpu_llm_longctx.py: 6e-3 against (i), 3e-2 against (ii) -- the first tightened to 3 x the measured worst, 4.64e-3,
    because that worst is under a third of 6e-3 (BOUND_SAME_FLOW).  The rows at and behind pos + m hold NaN: a query that reads
    one key too many turns NaN.

    Measured on an MI355X, error against (i) / against (ii), x 1e-3, by (m, pos):
              (1, 0)    (1, 44)    (2, 0)     (17, 0)    (67, 45)      (300, 0)     (255, 2)
      H = 3   0 / 0     0 / 6.69   0 / 2.33   0 / 4.26   1.464 / 9.23  0.977 / 5.74  0.293 / 6.48
      H = 16  0 / 0     0 / 11.63  0 / 3.75   0 / 6.04   1.546 / 14.15 0.484 / 8.16  1.224 / 10.38
    (0: the output equals the restatement bit for bit; the rest is the fp32 summation order flipping a bf16 rounding of a score.)"""
    q, kc, vc = _attn_case(H, m, pos)
    out = _run_unsplit(cuda, q, kc, vc, pos, H)
    e16, e32 = _attn_errors(out, *_attn_refs(q, kc, vc, pos))
    print(f"ld_llm_kv_attn unsplit H={H} m={m} pos={pos}: {e16:.6f} vs the same-dtype-flow restatement, {e32:.6f} vs fp32 "
          f"(of the output range)")
    assert e16 < BOUND_SAME_FLOW, e16
    assert e32 < BOUND_FP32, e32


@pytest.mark.parametrize("H", [3, 16])
@pytest.mark.parametrize("m,pos,first", [(67, 45, True), (300, 0, False)])
def test_kv_attn_unsplit_is_causal(cuda, H, m, pos, first):
    """The cache rows (pos + j0, pos + m) replaced by other values: the output rows j <= j0 keep their bits (they never read a key
    behind their own position), every row j > j0 changes.  j0 = 0 for one case, m // 2 for the other."""
    j0 = 0 if first else m // 2
    q, kc, vc = _attn_case(H, m, pos)
    out0 = _bits(_run_unsplit(cuda, q, kc, vc, pos, H))
    g = torch.Generator().manual_seed(99)
    kc2, vc2 = kc.clone(), vc.clone()
    n = m - j0 - 1
    kc2[:, pos + j0 + 1:pos + m] = torch.randn(ATTN_B, n, H, D, generator=g).to(torch.bfloat16)
    vc2[:, pos + j0 + 1:pos + m] = torch.randn(ATTN_B, n, H, D, generator=g).to(torch.bfloat16)
    out1 = _bits(_run_unsplit(cuda, q, kc2, vc2, pos, H))
    assert torch.equal(out0[:, :j0 + 1], out1[:, :j0 + 1])
    changed = (out0[:, j0 + 1:] != out1[:, j0 + 1:]).any(dim=2).any(dim=0)          # per query row, over batch rows / heads / dims
    assert changed.all(), (j0 + 1 + torch.nonzero(~changed).flatten()).tolist()


@pytest.mark.parametrize("L", [1, 45, 300])
def test_kv_attn_single_query_through_both_paths(cuda, L):
    """One decode step (m == 1, the key already in the cache) through ld_kv_attn_kernel (nsplit = 1, explicit rotated q) and through
    the split path (nsplit = 8 with its workspace): both meet both bounds -- the unsplit kernel its tightened one, the split path
    the 6e-3 of tests/test_gpu_llm_longctx.py; they need not agree bit for bit (p is bf16 in one and fp32 in the other).
    Measured against (i) / (ii), x 1e-3: L = 1: 0 / 0 both; L = 45: unsplit 0 / 11.63, split 4.643 / 11.63; L = 300: unsplit
    0 / 20.39, split 3.945 / 18.26."""
    from landiff_amd import ops
    H, pos, nsplit = 16, L - 1, 8
    q, kc, vc = _attn_case(H, 1, pos)
    refs = _attn_refs(q, kc, vc, pos)
    Lmax = kc.shape[1]
    e16, e32 = _attn_errors(_run_unsplit(cuda, q, kc, vc, pos, H), *refs)
    ws = torch.zeros(ATTN_B * H * (nsplit * 130 + 1), device=cuda, dtype=torch.float32)
    out = torch.full((ATTN_B, 1, H * D), NAN, device=cuda, dtype=torch.bfloat16)
    ops.llm_kv_attn(q.to(cuda), kc.to(cuda), vc.to(cuda), _dev_pos(cuda, pos), out, ATTN_B, 1, H, Lmax, workspace=ws, nsplit=nsplit)
    torch.cuda.synchronize()
    s16, s32 = _attn_errors(out, *refs)
    print(f"ld_llm_kv_attn m=1 L={L}: unsplit {e16:.6f} / {e32:.6f}, split {s16:.6f} / {s32:.6f} (vs same flow / vs fp32)")
    assert e16 < BOUND_SAME_FLOW and e32 < BOUND_FP32, (e16, e32)
    assert s16 < BOUND_SAME_FLOW_SPLIT and s32 < BOUND_FP32, (s16, s32)


def test_kv_attn_unsplit_rejects_a_context_beyond_the_lds_score_buffer(cuda):
    """m = 2 with Lmax = 41 000 needs more than 160 KiB of LDS for the scores: the launcher refuses on the host with an error that
    names Lmax and launches nothing (the output is still NaN)."""
    from landiff_amd import _lib, ops
    Lmax = 41000
    q = torch.zeros(1, 2, 1, D, device=cuda, dtype=torch.bfloat16)
    kc = torch.zeros(1, Lmax, 1, D, device=cuda, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    out = torch.full((1, 2, D), NAN, device=cuda, dtype=torch.bfloat16)
    with pytest.raises(_lib.LandiffHipError, match=r"Lmax=41000"):
        ops.llm_kv_attn(q, kc, vc, _dev_pos(cuda, 0), out, 1, 2, 1, Lmax)
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()


# ------------------------------------------------------------------------------------------------
# 3. ld_rmsnorm_bf16
# ------------------------------------------------------------------------------------------------
def _rms_check(got, ref64):
    """got (bf16 values as fp64) against the fp64 reference: every element within one bf16 rounding, >= 99 % correctly rounded."""
    assert torch.isfinite(got).all()
    assert ((got - ref64).abs() <= 2.0 ** -8 * ref64.abs() * 1.001).all(), ((got - ref64).abs() / ref64.abs()).max().item()
    exact = (got == ref64.float().to(torch.bfloat16).double()).double().mean().item()
    assert exact >= 0.99, exact
    return exact


@pytest.mark.parametrize("Dm", [8, 128, 520, 2048, 4104])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 130])
def test_rmsnorm_vs_fp64(cuda, rows, Dm):
    """x * rsqrt(mean(x^2) + eps) * w (transformer_blocks.py:35-40) in fp64 on the bf16 x: every output within one bf16 rounding of
    it (half a bf16 ulp is at most 2^-8 of the value; the ~1e-6 fp32 noise can only pick the other neighbour of a near-midpoint),
    and >= 99 % of them the correctly rounded value (the fp32 noise crosses a midpoint for ~3e-4 of the elements; a second
    rounding in the flow would for far more).  A CPU fp32 restatement meets the same cap for the same data, so the cap is not
    what is measured.  Rows behind `rows` of a larger NaN-filled out stay NaN (the r >= rows guard of the 4-rows-per-block grid)."""
    from landiff_amd import ops
    eps = 1e-5
    g = torch.Generator().manual_seed(31 * rows + Dm)
    x = (torch.randn(rows, Dm, generator=g) * 2 + 0.5).to(torch.bfloat16)
    w = 1 + 0.1 * torch.randn(Dm, generator=g)
    xd = x.double()
    ref = xd * torch.rsqrt(xd.square().mean(-1, keepdim=True) + eps) * w.double()
    xf = x.float()
    cpu32 = (xf * torch.rsqrt(xf.square().mean(-1, keepdim=True) + eps) * w).to(torch.bfloat16)
    _rms_check(cpu32.double(), ref)
    big = torch.full((rows + 5, Dm), NAN, device=cuda, dtype=torch.bfloat16)
    ops.rmsnorm(x.to(cuda), w.to(cuda), big[:rows], eps)
    torch.cuda.synchronize()
    assert torch.isnan(big[rows:].float()).all()
    _rms_check(big[:rows].cpu().double(), ref)


# ------------------------------------------------------------------------------------------------
# 4. ld_layernorm_bf16_to_f32
# ------------------------------------------------------------------------------------------------
LN_EPS = 1e-5


def _ln_inputs(rows, Dm, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, Dm, generator=g) + 3).to(torch.bfloat16)      # non-zero mean: E[x^2] - mean^2 would lose its digits
    return x, torch.randn(Dm, generator=g), torch.randn(Dm, generator=g)


def _ln_ref_and_bound(x, w, b):
    """fp64 F.layer_norm on the bf16 values, and the bound: 4 x the max abs error of torch's own fp32 F.layer_norm on the CPU against
    it (the factor covers the other summation order: a 64-lane tree against torch's vectorised sum), at least 2^-20 max |ref|."""
    import torch.nn.functional as F
    Dm = x.shape[-1]
    ref = F.layer_norm(x.double(), (Dm,), w.double(), b.double(), LN_EPS)
    e_torch = (F.layer_norm(x.float(), (Dm,), w, b, LN_EPS).double() - ref).abs().max().item()
    return ref, max(4 * e_torch, 2.0 ** -20 * ref.abs().max().item()), e_torch


def _ln_run(cuda, x_dev, w, b, rows, Dm):
    """Runs the kernel on x_dev (a [rows, Dm] view, any row stride) into the first rows of a larger NaN-filled buffer; the rows
    behind stay NaN (the r >= rows guard)."""
    from landiff_amd import ops
    big = torch.full((rows + 5, Dm), NAN, device=cuda, dtype=torch.float32)
    ops.layernorm_bf16_to_f32(x_dev, w.to(cuda), b.to(cuda), big[:rows], LN_EPS)
    torch.cuda.synchronize()
    assert torch.isnan(big[rows:]).all()
    got = big[:rows].cpu().double()
    assert torch.isfinite(got).all()
    return got


@pytest.mark.parametrize("Dm", [8, 520, 2048, 4096, 2055, 4100, 4104])
@pytest.mark.parametrize("rows", [1, 2, 5])
def test_layernorm_f32out_vs_fp64(cuda, rows, Dm):
    """Both kernels behind ld_layernorm_bf16_to_f32 against fp64 F.layer_norm: D in {8, 520, 2048, 4096} takes the register kernel
    (D % 8 == 0, D <= 4096), D in {2055, 4100, 4104} the three-pass kernel (odd D; D > 4096 with D % 8 != 0 and == 0).
    Measured on an MI355X over all cases: max abs error 8.6e-8 ... 1.32e-6 against 8.6e-8 ... 1.40e-6 for torch's fp32 layer_norm
    on the CPU; the worst ratio to the bound is 0.13 (rows = 2, D = 2048: 1.32e-6 against a bound of 9.9e-6)."""
    x, w, b = _ln_inputs(rows, Dm, 17 * rows + Dm)
    ref, bound, e_torch = _ln_ref_and_bound(x, w, b)
    err = (_ln_run(cuda, x.to(cuda), w, b, rows, Dm) - ref).abs().max().item()
    print(f"ld_layernorm_bf16_to_f32 rows={rows} D={Dm}: max abs error {err:.3e} (torch fp32 on the CPU: {e_torch:.3e}, bound {bound:.3e})")
    assert err <= bound, (err, bound)


def test_layernorm_f32out_strided_rows_as_the_prefill_calls_it(cuda):
    """x = the last token's row of every batch row of a [B, m, D] buffer (row stride m * D = 7 * 2048: the register kernel)."""
    Bn, m, Dm = 2, 7, 2048
    g = torch.Generator().manual_seed(5)
    buf = (torch.randn(Bn, m, Dm, generator=g) + 3).to(torch.bfloat16)
    w, b = torch.randn(Dm, generator=g), torch.randn(Dm, generator=g)
    ref, bound, e_torch = _ln_ref_and_bound(buf[:, -1], w, b)
    x_dev = buf.to(cuda)[:, -1]
    assert x_dev.stride(0) == m * Dm and x_dev.stride(0) % 8 == 0
    err = (_ln_run(cuda, x_dev, w, b, Bn, Dm) - ref).abs().max().item()
    print(f"ld_layernorm_bf16_to_f32 strided rows (ldx {m * Dm}): max abs error {err:.3e} (torch fp32: {e_torch:.3e}, bound {bound:.3e})")
    assert err <= bound, (err, bound)


def test_layernorm_f32out_kernel_choice_by_row_stride(cuda):
    """D = 2048 out of a [rows, 2052] buffer: ldx % 8 == 4 sends a D that the register kernel takes to the three-pass kernel.  The
    same values with ldx = 2048 go to the register kernel; each meets the bound, and so does their difference."""
    rows, Dm, ld = 5, 2048, 2052
    x, w, b = _ln_inputs(rows, Dm, 23)
    ref, bound, e_torch = _ln_ref_and_bound(x, w, b)
    buf = torch.full((rows, ld), NAN, device=cuda, dtype=torch.bfloat16)
    buf[:, :Dm] = x.to(cuda)
    x_dev = buf[:, :Dm]
    assert x_dev.stride(0) == ld and ld % 8 == 4
    got_3pass = _ln_run(cuda, x_dev, w, b, rows, Dm)
    got_reg = _ln_run(cuda, x.to(cuda), w, b, rows, Dm)
    e3, er, ed = ((got_3pass - ref).abs().max().item(), (got_reg - ref).abs().max().item(), (got_3pass - got_reg).abs().max().item())
    print(f"ld_layernorm_bf16_to_f32 D=2048: ldx 2052 (three-pass) {e3:.3e}, ldx 2048 (register) {er:.3e}, between them {ed:.3e} "
          f"(torch fp32: {e_torch:.3e}, bound {bound:.3e})")
    assert e3 <= bound and er <= bound and ed <= bound, (e3, er, ed, bound)


# ------------------------------------------------------------------------------------------------
# 5. ld_llm_embed
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("token", [0, 2054])
@pytest.mark.parametrize("B,Dm", [(1, 8), (2, 2048), (4, 100)])
def test_embed_rows_bit_exact(cuda, B, Dm, token):
    """Every batch row of out is table[token] rounded to bf16, for the first and the last row of a 2055-row fp32 table; the row
    behind the B rows of a larger buffer stays NaN."""
    from landiff_amd import ops
    V = 2055
    table = torch.randn(V, Dm, generator=torch.Generator().manual_seed(Dm)) + torch.arange(V).float()[:, None] * 1e-3
    big = torch.full((B + 1, Dm), NAN, device=cuda, dtype=torch.bfloat16)
    ops.llm_embed(table.to(cuda), torch.tensor([token], device=cuda, dtype=torch.int64), big[:B])
    torch.cuda.synchronize()
    assert torch.isnan(big[B:].float()).all()
    assert torch.equal(_bits(big[:B]), _bits(table[token].to(torch.bfloat16)[None].expand(B, Dm)))


# ------------------------------------------------------------------------------------------------
# 6. ld_llm_logits_to_probs at a restricted position
# ------------------------------------------------------------------------------------------------
def test_logits_to_probs_restricted_positions(cuda):
    """lm_model.py:417-454: CFG, / temperature, then EITHER top-k -> softmax -> top-p (no candidate list, :440-447) OR the
    -inf mask outside the candidate list -> softmax (:448-452) -- the reference applies NO top-k / top-p at a restricted position,
    so the kernel is called with top_k = 5 and top_p = 0.9 throughout and must ignore them there.  The `allowed` table (6 rows,
    stride 40, row = [count, ids...]) is indexed by the position being generated, *pos + 1."""
    import torch.nn.functional as F
    from landiff_amd import ops
    V, scale, temp, stride = 2055, 7.5, 0.8, 40
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(2, V, generator=g) * 0.5
    ids = torch.cat([torch.tensor([0, V - 1]), 1 + torch.randperm(V - 2, generator=g)[:18]])
    ids = ids[torch.randperm(20, generator=g)]
    assert ids.unique().numel() == 20
    decoy = next(i for i in range(V) if i not in ids.tolist())
    allowed = torch.full((6, stride), decoy, dtype=torch.int32)       # slots behind a row's count hold an id that is NOT listed
    allowed[:, 0] = 0
    p0 = 1
    allowed[p0 + 1, 0] = 20
    allowed[p0 + 1, 1:21] = ids.to(torch.int32)
    single = 1234
    allowed[p0 + 2, 0] = 1
    allowed[p0 + 2, 1] = single
    c, u = logits[0], logits[1]
    cfg_ref = u + scale * (c - u)
    cfg_tol = 2.0 ** -22 * (u.abs() + scale * (c - u).abs())             # the fp32 roundings of the product and the sum
    tempered = (cfg_ref / temp)[None]

    def run(pos, **kw):
        probs = torch.full((1, V), NAN, device=cuda)
        cfg = torch.full((V,), NAN, device=cuda)
        ops.llm_logits_to_probs(logits.to(cuda), probs, cfg, True, scale, temp, pos=_dev_pos(cuda, pos), allowed=allowed.to(cuda), **kw)
        torch.cuda.synchronize()
        assert ((cfg.cpu() - cfg_ref).abs() <= cfg_tol).all()
        return probs.cpu()

    # ---- 20 candidates: the support is the list, whatever top_k / top_p say ----
    mask = torch.full_like(tempered, -float("inf"))
    mask[0, ids] = 0
    ref = F.softmax(tempered + mask, dim=-1)
    assert (ref[0, ids] > 0).all() and int((ref > 0).sum()) == 20
    for kw in ({}, {"top_k": 5, "top_p": 0.9}):
        out = run(p0, **kw)
        assert torch.equal(out > 0, ref > 0), (kw, torch.nonzero(out[0] > 0).flatten().tolist())
        assert (out - ref).abs().max().item() < 2e-6, kw
        assert abs(out.sum().item() - 1) < 1e-5, kw
    # ---- one candidate: probability exactly 1 ----
    out = run(p0 + 1, top_k=5, top_p=0.9)
    assert out[0, single].item() == 1.0
    assert int((out != 0).sum()) == 1
    # ---- no candidate list: top-k applies ----
    v, _ = torch.topk(tempered, 5)
    ref_k = F.softmax(tempered.masked_fill(tempered < v[:, [-1]], -float("inf")), dim=-1)
    assert int((ref_k > 0).sum()) == 5
    out = run(p0 + 2, top_k=5)
    assert torch.equal(out > 0, ref_k > 0), torch.nonzero(out[0] > 0).flatten().tolist()
    assert (out - ref_k).abs().max().item() < 2e-6 and abs(out.sum().item() - 1) < 1e-5
