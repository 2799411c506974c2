"""ld_t5_rmsnorm and ld_t5_attn on their own (until now only reached through a whole encoder against HF, at max(2 x floor, 2e-2) of the
output range), through landiff_amd.ops, against the float64 restatements of tests/kernel_ref.py -- class C: the reference rounds to
bf16 where the bf16 HF module rounds, a per-element bound is carried through the chain, and >= 99 % of the elements must be bit-equal.

The attention test uses exact-score operands: q and k sparse {-1, 0, 1} and a bias that is a multiple of 0.5, so q.k and q.k + bias are
bf16 numbers (asserted) and the only inexact steps are the fp32 softmax, the bf16 rounding of the probabilities and the fp32 p.v sum.
With random scores one flipped bf16 score of size ~4 moves a probability by ~12 %, and no tight bound would mean anything; those are
covered through the encoder tests (tests/test_t5.py).

Measured on an MI355X: ld_t5_rmsnorm equal to the chain and to HF's bf16 module in every element; ld_t5_attn worst |err| / bound 0.460,
bit-equal share >= 0.99986 over the 12 cases."""
import pytest
import torch

import kernel_ref as kr
from kernel_ref import BF

pytestmark = pytest.mark.gpu

EPS = 1e-6
TAIL = 64


@pytest.mark.parametrize("D", [64, 512, 4096])
@pytest.mark.parametrize("rows", [1, 5])
def test_t5_rmsnorm(cuda, rows, D):
    """T5LayerNorm (transformers modeling_t5.py): fp32 variance, x * rsqrt(variance + eps) rounded to bf16, weight * that rounded again.
    HF's module run in bf16 on the CPU and the kernel are both held to the float64 chain with its two rounding points, and agree with
    each other on >= 99 % of the elements.  Rows behind `rows` keep the sentinel (the r >= rows guard of the 4-rows-per-block grid)."""
    from landiff_amd import ops
    from transformers.models.t5.modeling_t5 import T5LayerNorm
    g = torch.Generator().manual_seed(7 * rows + D)
    x = (torch.randn(rows, D, generator=g) * 2 + 0.5).to(BF)
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(BF)
    ref, bound = kr.t5_rmsnorm_ref(x, w, EPS)
    hf = T5LayerNorm(D, eps=EPS).to(BF)
    with torch.no_grad():
        hf.weight.copy_(w)
        out_hf = hf(x)
    kr.check_chain(out_hf, ref, bound, f"HF T5LayerNorm in bf16 on the CPU rows={rows} D={D}")
    b = kr.sentinels((rows * D + TAIL,), BF, cuda)
    ops.t5_rmsnorm(x.to(cuda), w.to(cuda), b.view(BF)[:rows * D].view(rows, D), EPS)
    torch.cuda.synchronize()
    got = b.cpu()
    assert bool(kr.is_sentinel(got[rows * D:]).all()), "a store behind the last row"
    got = got[:rows * D].view(BF).view(rows, D)
    kr.check_chain(got, ref, bound, f"ld_t5_rmsnorm rows={rows} D={D}")
    same = (kr.bits(got) == kr.bits(out_hf)).double().mean().item()
    print(f"ld_t5_rmsnorm rows={rows} D={D}: bit-equal to HF's bf16 module on {same:.6f} of the elements")
    assert same >= kr.MIN_EQUAL


def _attn_layout(cuda, q, k, v, fused):
    """fused: q, k, v as column views of one [N, 3*H*64] buffer, out as the first H*64 columns of a sentinel buffer of the same row
    stride (landiff_amd/t5.py:123,130); else separate [N, H*64] buffers.  Returns (q, k, v, out views on the device, out bits, row stride)."""
    N, H, _ = q.shape
    inner = H * 64
    ld = 3 * inner if fused else inner
    if fused:
        qkv = torch.cat([t.reshape(N, inner) for t in (q, k, v)], dim=1).to(cuda)
        views = [qkv[:, i * inner:(i + 1) * inner] for i in range(3)]
    else:
        views = [t.reshape(N, inner).to(cuda) for t in (q, k, v)]
    ob = kr.sentinels((N + 2, ld), BF, cuda)
    return views, ob.view(BF)[:N, :inner], ob, ld


@pytest.mark.parametrize("fused", [True, False], ids=["h2_fused_ld384", "h3_separate_ld192"])
@pytest.mark.parametrize("N", [1, 5, 64, 65, 226, 512])
def test_t5_attn_exact_scores(cuda, N, fused):
    """T5Attention of the bf16 HF module: bf16 scores + bucketed relative-position bias, fp32 softmax cast to bf16, p @ v -> bf16; buckets
    from landiff_amd.t5.relative_buckets (pinned to HF on the CPU), a randomised bias table.  N covers one row, a partly filled block of
    4 query rows, exactly and just over one 64-key trip, the DiT context length and the limit.  Columns [H*64, ld) and the rows behind N
    keep the sentinel."""
    from landiff_amd import ops
    from landiff_amd.t5 import relative_buckets
    H = 2 if fused else 3
    q, k, v, table = kr.t5_exact_operands(N, H, 32, 100 * N + H)
    bucket = relative_buckets(N)
    ref, bound = kr.t5_attn_ref(q, k, v, table, bucket)                      # (asserts the exact-score premise)
    kr.check_chain(kr.t5_attn_cpu32(q, k, v, table, bucket), ref, bound, f"CPU restatement N={N} H={H}")
    (qd, kd, vd), out, ob, ld = _attn_layout(cuda, q, k, v, fused)
    assert qd.stride(0) == ld and out.stride(0) == ld
    ops.t5_attn(qd, kd, vd, out, table.to(cuda), bucket.to(cuda), H)
    torch.cuda.synchronize()
    written = torch.zeros(ob.shape, dtype=torch.bool)
    written[:N, :H * 64] = True
    kr.check_untouched(ob, written, f"ld_t5_attn N={N} H={H}")
    got = ob.cpu().view(BF)[:N, :H * 64].reshape(N, H, 64)
    kr.check_chain(got, ref, bound, f"ld_t5_attn N={N} H={H} ld={ld}")


def test_t5_attn_refuses_more_than_512_tokens(cuda):
    from landiff_amd import ops
    from landiff_amd._lib import LandiffHipError
    from landiff_amd.t5 import relative_buckets
    N, H = 513, 1
    q = torch.zeros(N, 64, dtype=BF, device=cuda)
    ob = kr.sentinels((N, 64), BF, cuda)
    with pytest.raises(LandiffHipError):
        ops.t5_attn(q, q, q, ob.view(BF), torch.zeros(32, H, dtype=BF, device=cuda), relative_buckets(N).to(cuda), H)
    torch.cuda.synchronize()
    assert bool(kr.is_sentinel(ob).all())
