"""ld_gemv on every kernel its dispatch reaches, element by element (tests/gemv_ref.py holds the reference, the case table and the
checker; tests/test_gemv_ref_host.py shows on the CPU that the checker passes a correct fp32 restatement of every case and fails
eleven kinds of wrong output).

Every case
  * asserts its route first (ld_gemv_route: kernel, J, R, U), so a retune of the dispatch fails here instead of quietly moving the
    case off the kernel it was written for;
  * hands x as a [B, K] view of a [B, K + 8] buffer whose padding holds NaN (a chunk read past K poisons the sum), the residual
    with a row stride of its own (N + 5), and out as a [B, N] view inside a [B + 2, N + 3] buffer of sentinels -- unless the case
    is "inplace": out is the residual, as the decode's wo / w2 calls run;
  * random operands: check_chain against the float64 chain rounded where the kernel rounds, with the carried per-element bound
    and >= 99 % bit-equal (fp32 weights: check_f32 against torch's fp32 on the CPU); every sentinel intact;
  * exact operands (forms without an activation or a norm): the WHOLE buffer bit for bit.

TABLE: the smallest shape at which each edge of the two kernels exists (the edge is named in the table).  COVERAGE: one tiny case
for every further instantiation -- (kernel, J, R, U, gated, norm) x B in {1, 2, 3-4} -- the default dispatch reaches.

Not covered, and why:
  * reachable only under a knob that is read once per process (the plan query shows those routes without launching them):
    LD_GEMV_R -- the register kernel with R = 8 rows per batch (B <= 2: J = 1, or J = 2 without a gate), with R = 1, and every
    (J, gated) at another R than its default (J = 1: 4; J = 2: 4, gated 2; J = 6: 2); LD_GEMV_MODE=1 -- the
    streaming kernel on the register forms' shapes (tests/test_gpu_variants.py runs tests/test_gpu_gemv.py under it);
    LD_GEMV_WGS -- another workgroup cap of the register kernel (the trips-per-workgroup count; r_grid has two at the default);
  * the variants build's dependent-launch form (ld_gemv_reg_kernel<..., CHAIN>): tests/test_gpu_variants.py;
  * reached by the default dispatch: the streaming kernel with two rows per wave (R = 2, U = 4) behind the fused norm at B <= 2 --
    it needs N >= 4096 at K > 12288, a 100 MB matrix; the norm is in the staging, which does not depend on R, the same
    instantiations run without the norm (s_r2, c_s24_b1) and the norm runs with R = 2 at B = 3 (c_s24n_b3);
  * fp32 weights with an activation, a norm or in_act: no shipped form; misaligned or out-of-range pointers.
"""
import pytest
import torch

import gemv_ref as gr
from gemv_ref import BF, CASES

pytestmark = pytest.mark.gpu

RUNS = [(c, False) for c in CASES] + [(c, True) for c in CASES if c.has_exact]


@pytest.mark.parametrize("case,exact", RUNS, ids=[f"{c.id}-{'exact' if e else 'random'}" for c, e in RUNS])
def test_gemv_route_case(cuda, case, exact):
    from landiff_amd import ops
    assert case.route() == case.plan, (case.route(), case.plan)
    o = gr.placed(case, exact, cuda)
    ref, bound, t32 = gr.reference(case, o, exact)
    kw, eps = gr.call_kwargs(case, o)
    buf, out = gr.out_buffer(case, cuda)
    assert out.stride(0) == case.N + 3 and o["x"].stride(0) == case.K + 8
    if case.has("inplace"):
        out.copy_(o["resid"])
        kw["resid"] = out
    elif kw["resid"] is not None:
        assert kw["resid"].stride(0) != out.stride(0)
    ops.gemv(o["x"], o["w"], out, norm_eps=eps, **kw)
    torch.cuda.synchronize()
    gr.check_case(case, buf, ref, bound, t32, exact, f"\n{case.id} {'exact' if exact else 'random'} [{case.edge}]")


ONE_HOT_K = (0, 7, 8, 2047, 2048, 4095, 4096, 12280, 12287)


@pytest.mark.parametrize("B,K,plan", [(2, 12288, gr.reg(6, 2)), (4, 4096, gr.reg(2, 4))], ids=["j6_b2", "j2_b4"])
def test_gemv_one_hot_sweep(cuda, B, K, plan):
    """x rows one-hot at the first and last element of a chunk, of a thread's j and of K: without an epilogue out[b] is column k_b
    of W bit for bit -- every chunk is owned once, by the right thread, for the right row."""
    from landiff_amd import ops
    N = 9
    assert gr.route(B, N, K) == plan
    g = torch.Generator().manual_seed(K)
    w = torch.randn(N, K, generator=g).to(BF).to(cuda)
    ks = [k for k in ONE_HOT_K if k < K]
    for i in range(0, len(ks), B):
        kb = (ks[i:i + B] + ks[:B])[:B]                        # B per launch (the last launch filled up from the front)
        xbuf = torch.zeros(B, K + 8, dtype=BF, device=cuda)
        xbuf[:, K:] = float("nan")
        for b, k in enumerate(kb):
            xbuf[b, k] = 1.0
        dt = BF
        buf = gr.sentinels((B + 2, N + 3), dt, cuda)
        ops.gemv(xbuf[:, :K], w, buf.view(dt)[:B, :N])
        torch.cuda.synchronize()
        want = gr.sentinels((B + 2, N + 3), dt)
        want[:B, :N] = gr.bits(w[:, kb].t().contiguous().cpu())
        gr.check_bits(buf, want, f"one-hot at k = {kb}")
