"""tests/gemv_ref.py on the CPU (no GPU): for every case of its table the plain fp32 restatement of the kernels' chain passes the
checker the GPU test uses, at least 99.5 % bit-equal -- so the checker's 99 % floor, which keeps a test from hiding a failure behind
its bound, is met by the reference alone on these very inputs -- and eleven deliberately wrong outputs fail it: a chunk of K
dropped or counted twice, rows or batch rows exchanged, a rounding point removed or added, the residual or the bias of another
row, a store into the row padding or behind the last row.  The table's route column is checked against ld_gemv_route, the
dispatch is swept for instantiations no case reaches, and every refusal is checked to happen before a launch."""
import ctypes

import pytest
import torch

import gemv_ref as gr
from gemv_ref import BF, CASES, REG, STREAM

BY_ID = {c.id: c for c in CASES}
RUNS = [(c, False) for c in CASES] + [(c, True) for c in CASES if c.has_exact]


def _run_cpu(case, exact, **wrong):
    """gemv_cpu32 on a case's operands, stored through out_buffer as the kernel stores (in place: out preset with the residual)
    -> (buffer bits, reference, bound, torch32)."""
    o = gr.placed(case, exact)
    ref, bound, t32 = gr.reference(case, o, exact)
    kw, eps = gr.call_kwargs(case, o)
    buf, out = gr.out_buffer(case)
    if case.has("inplace"):
        out.copy_(o["resid"])
        kw["resid"] = out
    got = gr.gemv_cpu32(o["x"], o["w"], eps=eps, out_f32=case.out_f32, **kw, **wrong)
    out.copy_(got)
    return buf, ref, bound, t32


def _fails(case, buf, ref, bound, t32, exact, what):
    with pytest.raises(AssertionError):
        gr.check_case(case, buf, ref, bound, t32, exact, what)


@pytest.mark.parametrize("case,exact", RUNS, ids=[f"{c.id}-{'exact' if e else 'random'}" for c, e in RUNS])
def test_cpu_fp32_restatement_passes_every_case(case, exact):
    buf, ref, bound, t32 = _run_cpu(case, exact)
    res = gr.check_case(case, buf, ref, bound, t32, exact, f"cpu fp32 {case.id}")
    if not exact and t32 is None:
        assert res[1] >= 0.995, f"{case.id}: the fp32 restatement is only {res[1]:.4f} bit-equal: change the case's seed or scale, not the cap"
        assert bool((bound > 0).all()) and bool((bound < 2.0 ** -4 * ref.abs() + 2.0 ** -6).all())        # a bound that says something


def test_reference_definition_element_by_element():
    """A few outputs of the gated + norm chain from the definition, in float64 scalars."""
    case = BY_ID["r_255"]
    o = gr.placed(case, False)
    ref, _, _ = gr.reference(case, o, False)
    x, w, w2, g = o["x"].double(), o["w"].double(), o["w2"].double(), o["norm_w"].double()
    gelu = lambda v: 0.5 * v * (1 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v ** 3)))
    for b, n in ((0, 0), (3, 6), (2, 4)):
        xn = gr.bf(x[b] * torch.rsqrt((x[b] * x[b]).mean() + 1e-5) * g)
        want = gr.bf(gr.bf(gelu(gr.bf(xn @ w[n]))) * gr.bf(xn @ w2[n]))
        assert ref[b, n] == want


# ---- wrong kernels ------------------------------------------------------------------------------------------------------------
def test_a_dropped_or_doubled_chunk_fails():
    case = BY_ID["r_w2"]                                       # K = 11008: thread t owns chunks t, t + 256, ..., j = 5 holds 96
    good = _run_cpu(case, False)
    gr.check_case(case, *good, False, "r_w2")
    k = torch.ones(case.K)
    k[-8:] = 0
    _fails(case, *_run_cpu(case, False, k_mult=k), False, "the last chunk of K dropped")
    for j in (1, 5):
        k = torch.ones(case.K)
        k[256 * j * 8: 256 * j * 8 + 8] = 2
        _fails(case, *_run_cpu(case, False, k_mult=k), False, f"chunk 256 * {j} counted twice")
    one = BY_ID["r_onechunk"]                                  # a single chunk: dropping it leaves the bias-less output zero
    _fails(one, *_run_cpu(one, False, k_mult=torch.zeros(one.K)), False, "the only chunk dropped")


def _permuted(case, exact, fn):
    buf, ref, bound, t32 = _run_cpu(case, exact)
    dt = torch.float32 if case.out_f32 else BF
    out = buf.view(dt)[:case.B, :case.N]
    out.copy_(fn(out.clone()))
    return buf, ref, bound, t32


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
def test_exchanged_rows_fail(exact):
    case = BY_ID["r_grid"]                                     # W's column 0 differs from row to row
    def swap_n(o):
        o[:, [100, 101]] = o[:, [101, 100]]
        return o
    _fails(case, *_permuted(case, exact, swap_n), exact, "rows n and n + 1 exchanged")
    _fails(case, *_permuted(case, exact, lambda o: o.flip(0)), exact, "batch rows exchanged")
    for id in ("r_j1_full", "r_f32out", "s_past_j6"):
        c = BY_ID[id]
        _fails(c, *_permuted(c, exact, lambda o: o.roll(1, 0)), exact, "batch rows rotated")


def test_the_operands_of_another_row_fail():
    for id, exact in (("r_w2", False), ("r_w2", True), ("r_j1_full", True), ("s_two_trips", False), ("r_f32out", False)):
        case = BY_ID[id]
        o = gr.placed(case, exact)
        ref, bound, t32 = gr.reference(case, o, exact)
        kw, eps = gr.call_kwargs(case, o)
        buf, out = gr.out_buffer(case)
        kw["resid"] = o["resid"][:1].expand(case.B, case.N)
        out.copy_(gr.gemv_cpu32(o["x"], o["w"], eps=eps, out_f32=case.out_f32, **kw))
        _fails(case, buf, ref, bound, t32, exact, f"{id}: the residual read from row 0 for every b")
    for id, exact in (("r_grid", False), ("r_grid", True), ("r_j2_first", False), ("s_r8_tail", False)):
        case = BY_ID[id]
        o = gr.placed(case, exact)
        ref, bound, t32 = gr.reference(case, o, exact)
        kw, eps = gr.call_kwargs(case, o)
        buf, out = gr.out_buffer(case)
        kw["bias"] = o["bias"].roll(1)
        out.copy_(gr.gemv_cpu32(o["x"], o["w"], eps=eps, out_f32=case.out_f32, **kw))
        _fails(case, buf, ref, bound, t32, exact, f"{id}: the bias of row n - 1")


def test_a_removed_or_added_rounding_point_fails():
    case = BY_ID["s_gated_loop"]                               # 2050 gated outputs: enough for the bit-equal share to speak
    gr.check_case(case, *_run_cpu(case, False), False, "s_gated_loop")
    _fails(case, *_run_cpu(case, False, drop="linear"), False, "the Linear output not rounded before act")
    _fails(case, *_run_cpu(case, False, drop="acc2"), False, "W2 x not rounded before the gate product")
    case = BY_ID["r_f32out"]
    _fails(case, *_run_cpu(case, False, drop="resid"), False, "the fp32 residual sum rounded to bf16")
    case = BY_ID["s_r2"]                                       # and the staged activations: bf16(silu(x)), not silu(x)
    o = gr.placed(case, False)
    ref, bound, t32 = gr.reference(case, o, False)
    buf, out = gr.out_buffer(case)
    out.copy_((torch.nn.functional.silu(o["x"].float()) @ o["w"].float().t() + o["bias"].float()).to(BF))
    _fails(case, buf, ref, bound, t32, False, "the activated x not rounded to bf16")


@pytest.mark.parametrize("id,exact", [("r_grid", True), ("r_grid", False), ("r_f32out", True), ("f_small", False), ("f_small", True), ("r_255", False)])
def test_a_stray_store_fails(id, exact):
    case = BY_ID[id]
    good = _run_cpu(case, exact)
    gr.check_case(case, *good, exact, id)
    for where, what in (((0, case.N), "one store into the ldo padding"), ((case.B - 1, case.N + 2), "the last padding element"),
                        ((case.B, 0), "one store into row B"), ((case.B + 1, case.N - 1), "one store into row B + 1")):
        buf, ref, bound, t32 = _run_cpu(case, exact)
        buf[where] = 0
        _fails(case, buf, ref, bound, t32, exact, what)
    buf, ref, bound, t32 = _run_cpu(case, exact)
    buf[case.B - 1, case.N - 1] = gr.sentinels((1,), torch.float32 if case.out_f32 else BF)[0]
    _fails(case, buf, ref, bound, t32, exact, "the last output left unwritten")


def test_a_chunk_read_past_k_poisons_the_sum():
    """x sits in a [B, K + 8] buffer whose padding holds NaN."""
    case = BY_ID["r_j2_first"]
    o = gr.placed(case, False)
    assert o["x"].stride(0) == case.K + 8 and bool(torch.isnan(o["x"].as_strided((case.B, 8), (case.K + 8, 1), case.K)).all())
    ref, bound, t32 = gr.reference(case, o, False)
    buf, out = gr.out_buffer(case)
    xp = o["x"].as_strided((case.B, case.K + 8), (case.K + 8, 1)).float()
    out.copy_((xp @ torch.nn.functional.pad(o["w"].float(), (0, 8)).t()).to(BF))
    _fails(case, buf, ref, bound, t32, False, "one chunk past K read")


# ---- the plan -----------------------------------------------------------------------------------------------------------------
def test_route_table():
    """ld_gemv_route answers the route column of every case, and the edges the cases sit on are where the table says."""
    for c in CASES:
        assert c.route() == c.plan, (c.id, c.route(), c.plan)
    r = lambda *a, **k: gr.route(*a, **k)
    assert r(2, 5, 2048) == (REG, 1, 4, 0) and r(2, 5, 2056) == (REG, 2, 4, 0)
    assert r(2, 5, 4096) == (REG, 2, 4, 0) and r(2, 5, 4104) == (REG, 6, 2, 0) and r(3, 5, 4104) == (STREAM, 0, 1, 4)
    assert r(2, 5, 12288) == (REG, 6, 2, 0) and r(2, 5, 12296) == (STREAM, 0, 1, 4)
    assert r(2, 5, 4096, gated=True) == (REG, 2, 2, 0) and r(2, 5, 4104, gated=True) == (STREAM, 0, 1, 4)
    assert r(2, 4095, 520, in_act=True) == (STREAM, 0, 1, 4) and r(2, 4096, 520, in_act=True) == (STREAM, 0, 2, 4)
    assert r(2, 4096, 512, in_act=True) == (STREAM, 0, 8, 1) and r(2, 4095, 512, in_act=True) == (STREAM, 0, 1, 4)
    assert r(2, 4096, 512) == (REG, 1, 4, 0) and r(2, 4096, 512, x_f32=True) == (STREAM, 0, 8, 1)
    assert r(2, 5000, 2048, x_f32=True, w_f32=True, out_f32=True) == (STREAM, 0, 1, 4)
    assert r(2, 5, 64, normed=True) == r(2, 5, 64) and r(2, 5, 64, out_f32=True) == r(2, 5, 64)          # neither moves a call
    rc = gr.route(2, 5, 64)[0]
    from landiff_amd import _lib
    assert _lib.load().ld_gemv_route(2, 5, 64, 0, 0, 0, 0, 0, 0, None, None, None) == rc                 # J, R, U may be null


def test_every_reachable_instantiation_has_a_case():
    """The dispatch swept over shapes on both sides of each threshold and every form: each (kernel, J, R, U, gated, norm, B class,
    fp32) it answers is the key of a case, or is listed in NOT_COVERED with its reason."""
    have = {c.key() for c in CASES}
    assert not (have & gr.NOT_COVERED)
    seen = set()
    for B in (1, 2, 3, 4):
        for K in (8, 512, 520, 2048, 2056, 4096, 4104, 12288, 12296, 16384):
            for N in (1, 5, 4095, 4096, 50000):
                for gated in (False, True):
                    for normed in (False, True):
                        for in_act in (False, True):
                            for x_f32, w_f32 in ((False, False), (True, False), (True, True)):
                                rc, J, R, U = gr.route(B, N, K, x_f32=x_f32, w_f32=w_f32, out_f32=w_f32, gated=gated, normed=normed, in_act=in_act)
                                if rc >= 0 and not (w_f32 and in_act):                                   # (fp32 weights with in_act: not a shipped form)
                                    seen.add((rc, J, R, U, gated, normed, min(B, 3), w_f32))
    assert seen - have == gr.NOT_COVERED, sorted(seen - have - gr.NOT_COVERED)
    assert have <= seen, sorted(have - seen)


def test_refusals_happen_before_a_launch():
    """No GPU here: a call that got as far as a launch would fail otherwise (or crash on the fake pointers)."""
    from landiff_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    f32 = ctypes.cast(p, ctypes.POINTER(ctypes.c_float))
    err = lambda: lib.ld_last_error()
    #                  x  ldx xf32 W  W2    wf32 bias  resid ldr out ldo of32 B  N  K  in_act act norm_w eps stream
    for fn, name in ((lib.ld_gemv, b"ld_gemv:"), (lib.ld_gemv_pairs, b"ld_gemv_pairs:")):
        assert fn(p, 64, 0, p, None, 0, None, None, 0, p, 64, 0, 2, 8, 64, 3, 0, f32, 1e-5, None) == -1 and b"in_act with a fused RMSNorm" in err() and name in err()
        assert fn(p, 64, 0, p, None, 0, None, None, 0, p, 64, 0, 2, 8, 12, 0, 0, None, 0.0, None) == -1 and b"multiples of 8" in err()
        assert fn(p, 64, 1, p, p, 1, None, None, 0, p, 64, 1, 2, 8, 64, 0, 0, None, 0.0, None) == -1 and b"gated form needs bf16 weights" in err()
        assert fn(p, 64, 1, p, None, 1, None, None, 0, p, 64, 0, 2, 8, 64, 0, 0, None, 0.0, None) == -1 and b"fp32 weights need fp32 in/out" in err()
        assert fn(None, 64, 0, p, None, 0, None, None, 0, p, 64, 0, 2, 8, 64, 0, 0, None, 0.0, None) == -1 and b"null" in err()
    assert lib.ld_gemv(p, 64, 0, p, None, 0, None, None, 0, p, 64, 0, 5, 8, 64, 0, 0, None, 0.0, None) == -1 and b"batch 5 not in [1,4]" in err()
    assert lib.ld_gemv_pairs(p, 64, 0, p, None, 0, None, None, 0, p, 64, 0, 5, 8, 64, 0, 0, None, 0.0, None) == -1 and b"not pairs" in err()
    assert lib.ld_gemv_wide(p, 64, 0, p, None, 0, None, None, 0, p, 64, 0, 2, 8, 64, 3, 0, None, 0.0, None) == -3 and b"no input activation" in err()
    # the route query refuses what ld_gemv refuses, with ld_gemv's message
    for kw, msg in ((dict(in_act=True, normed=True), b"ld_gemv: in_act with a fused RMSNorm"), (dict(x_f32=True, normed=True), b"ld_gemv: fused RMSNorm needs bf16"),
                    (dict(x_f32=True, w_f32=True, out_f32=True, gated=True), b"ld_gemv: gated form needs bf16 weights"),
                    (dict(x_f32=True, w_f32=True), b"ld_gemv: fp32 weights need fp32 in/out")):
        assert gr.route(2, 8, 64, **kw)[0] == -1 and msg in err(), kw
    assert gr.route(5, 8, 64)[0] == -1 and b"ld_gemv: batch 5 not in [1,4]" in err()
    assert gr.route(2, 8, 12)[0] == -1 and b"ld_gemv: K and ldx must be multiples of 8" in err()
    assert gr.route(2, 0, 64)[0] == -1 and gr.route(4, 8, 24576)[0] == -1 and b"too large for the LDS" in err()
    assert gr.route(2, 8, 64) == (REG, 1, 4, 0)


def test_ops_gemv_refuses_operands_the_kernels_would_misread():
    """ops._gemv: bias is read as bf16, resid as out's type, norm_w as K floats, w2 like w -- anything else raises before the
    library is called (CPU tensors here: a call that reached the library would raise LandiffHipError instead)."""
    from landiff_amd import ops
    B, N, K = 2, 8, 64
    x, w, out = torch.zeros(B, K, dtype=BF), torch.zeros(N, K, dtype=BF), torch.zeros(B, N, dtype=BF)
    bad = [
        (dict(bias=torch.zeros(N)), "bias must be bf16"),
        (dict(resid=torch.zeros(B, N)), "resid must have out's dtype"),
        (dict(w2=torch.zeros(N, K)), "w2 must be"),
        (dict(w2=torch.zeros(N + 1, K, dtype=BF)), "w2 must be"),
        (dict(w2=torch.zeros(K, N, dtype=BF).t()), "w2 must be"),
        (dict(norm_w=torch.zeros(K, dtype=BF)), "norm_w must be"),
        (dict(norm_w=torch.zeros(K + 8)), "norm_w must be"),
        (dict(norm_w=torch.zeros(2 * K)[::2]), "norm_w must be"),
    ]
    for fn in (ops.gemv, ops.gemv_pairs, ops.gemv_wide):
        for kw, msg in bad:
            with pytest.raises(ValueError, match=msg):
                fn(x, w, out, **kw)
    with pytest.raises(ValueError, match="resid must have out's dtype"):
        ops.gemv(x, w, torch.zeros(B, N), resid=torch.zeros(B, N, dtype=BF))
