"""ld_gemm_bf16 on every shipped route x every epilogue, element by element.

plan() (ld_gemm.hip) sends a linear GEMM to one of four routes by (M, N, K): 0 = 128x128 two-stage, 2 = 256x256 8-phase,
6 = 8-phase on the whole rounds + 256x128 half-tile tail, 7 = 8-phase on the top tile rows + 128x128 row tail (m_begin).  The DiT's
four GEMMs all run a split form (6 or 7).  Every case first asserts its route and epilogue kind through ld_gemm_route, so a retune
that moves a shape elsewhere fails here instead of losing the coverage.

Two kinds of check:
  * exact: sparse {-1, 0, 1} operands and small-integer / power-of-two epilogue operands, so every fp32 accumulation and every bf16
    rounding point is exact (the test asserts that premise); the output must equal a float64 reference bit for bit, and the output
    sits inside a buffer of NaN sentinels (extra columns, extra rows) that must come back untouched -- a skipped, half-written or
    misplaced tile, a wrong gate row or a store past M or N fails;
  * random: N(0, 1)-sized operands, a float64 reference rounded to bf16 where the kernel rounds, and a per-element bound that
    carries the error of every step (fp32 accumulation K 2^-24 sum|a||w|, one bf16 ulp per rounding, through the activation's
    slope and the later multiplies).
"""
import ctypes
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN16, NAN32 = 0x7FA5, 0x7FC0A5A5          # sentinel bit patterns (quiet NaNs) around the output
EPI_BIAS, EPI_GELU, EPI_GATE, EPI_GENERIC = 0, 1, 2, 3
M_DIT, D, ROWS, TEXT = 2 * 17776, 1920, 17776, 226


def _route(M, N, K, ldo, **epi):
    from landiff_amd import _lib, ops
    e = ops.make_epilogue(**epi)
    kind = ctypes.c_int32(-1)
    rc = _lib.load().ld_gemm_route(M, N, K, ldo, ctypes.byref(e), ctypes.byref(kind))
    return rc, kind.value


def _ulp(x):
    """bf16 unit in the last place of |x| (float64 tensor); 2^-133 (the smallest subnormal) at 0."""
    m, e = torch.frexp(x.abs())
    return torch.where(x == 0, torch.full_like(x, 2.0 ** -133), torch.ldexp(torch.ones_like(x), (e - 8).clamp(min=-133)))


def _bf(x):
    return x.to(BF).double()


ACT64 = {
    "gelu_tanh": lambda x: 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3))),
    "gelu_erf": lambda x: 0.5 * x * (1 + torch.erf(x * 0.7071067811865476)),
    "silu": lambda x: x * torch.sigmoid(x),
    "tanh": torch.tanh,
}


def _operands(M, N, K, exact, seed, dev, lda_pad=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    if exact:
        dens = (8.0 / K) ** 0.5                          # ~8 non-zero products per output: |acc| stays far below 256
        tern = lambda r, c: (torch.randint(-1, 2, (r, c), device=dev, generator=g) *
                             (torch.rand(r, c, device=dev, generator=g) < dens)).to(BF)
        abuf, w = tern(M, K + lda_pad), tern(N, K)
    else:
        abuf = torch.randn(M, K + lda_pad, device=dev, generator=g).to(BF)
        w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(BF)
    return abuf[:, :K], w, g                             # a: a row stride lda = K + lda_pad when padded


def _small(shape, g, dev, lo, hi, exact, scale=1.0):
    if exact:
        return torch.randint(lo, hi + 1, shape, device=dev, generator=g).to(BF)
    return (torch.randn(shape, device=dev, generator=g) * scale).to(BF)


def _gate_values(shape, g, dev, exact):
    if exact:
        pw = torch.tensor([0.5, 1.0, 2.0], device=dev)[torch.randint(0, 3, shape, device=dev, generator=g)]
        return (pw * (torch.randint(0, 2, shape, device=dev, generator=g) * 2 - 1)).to(BF)
    return torch.randn(shape, device=dev, generator=g).to(BF)


def _expand_gate(ada, M, N, rows, text, off_img, off_txt):
    m = torch.arange(M, device=ada.device)
    b = m // rows
    txt = ((m - b * rows) < text)[:, None]
    return torch.where(txt, ada[:, off_txt: off_txt + N][b], ada[:, off_img: off_img + N][b]).double()


def _reference(a, w, epi, exact, N):
    """float64 restatement of the epilogue (include/landiff_hip.h, ld_epilogue_t): (value, error bound) per element.  exact:
    asserts that every value the kernel rounds to bf16 is a bf16 number already (bound 0)."""
    acc = a.double() @ w.double().t()
    K = a.shape[1]
    out_f32 = epi.get("out_f32", False)
    if exact:
        err = torch.zeros_like(acc)
    else:
        err = (a.double().abs() @ w.double().abs().t()) * (K * 2.0 ** -24)
    v = acc
    if epi.get("bias") is not None:
        v = v + epi["bias"].double()

    def rnd(v, err, what):
        if exact:
            assert torch.equal(v, _bf(v)), f"premise: {what} is not exact in bf16"
            return v, err
        err = err + 2.0 ** -24 * v.abs()                 # the fp32 value being rounded
        return _bf(v), err + _ulp(v.abs() + err)

    v, err = rnd(v, err, "the Linear output")
    act = epi.get("act")
    if act:
        f = ACT64[act]
        if exact:
            raise AssertionError("activations are checked with random operands")
        fv = f(v)
        slope = torch.maximum((f(v + err) - fv).abs(), (f(v - err) - fv).abs())
        # the kernel evaluates the activation in fp32 (hardware exp2 / rcp, erff): a few fp32 ulps of the input's size
        err = slope + 2.0 ** -20 * (v.abs() + fv.abs()) + 2.0 ** -120
        v, err = rnd(fv, err, "the activation")
    if epi.get("mul") is not None:
        mv = epi["mul"].double()
        v, err = rnd(v * mv, err * mv.abs(), "x * mul")
    if epi.get("gate") is not None:
        gv = _expand_gate(epi["gate"], a.shape[0], N, epi["rows_per_batch"], epi["text_len"], epi["gate_off_img"], epi["gate_off_txt"])
        v, err = rnd(v * gv, err * gv.abs(), "x * gate")
    for name in ("resid", "add2"):
        if epi.get(name) is not None:
            v = v + epi[name].double()
            if out_f32:
                if not exact:
                    err = err + 2.0 ** -24 * v.abs()
            else:
                v, err = rnd(v, err, "x + " + name)
    if out_f32 and exact:
        assert torch.equal(v, v.float().double()), "premise: fp32 output not exact"
    return v, err


def _sentinel_buffer(M, N, ldo, dt, dev, extra_rows=3):
    """out [M, N] inside a [M + extra_rows, ldo] buffer of NaN sentinels; returns (buffer bits, out view)."""
    if dt == torch.float32:
        bits = torch.full((M + extra_rows, ldo), NAN32, device=dev, dtype=torch.int32)
    else:
        bits = torch.full((M + extra_rows, ldo), NAN16, device=dev, dtype=torch.int16)
    return bits, bits.view(dt)[:M, :N]


def _check_sentinels(bits, M, N):
    s = NAN32 if bits.dtype == torch.int32 else NAN16
    assert bool((bits[M:] == s).all()), "a store past row M"
    assert bool((bits[:M, N:] == s).all()), "a store past column N (into the ldo padding)"


# (id, route, epilogue kind, M, N, K, lda pad, ldo pad, epilogue form)
#   DiT forms: dense (gate, out != resid), h1 (gate + add2, out is resid), B = 2 x 17776 rows, text 226
#   "tail": B = 5 batches of 4130 rows: the row tail (rows >= 64 tile rows = 16384) holds the batch boundary 16520 -- inside a
#   wave tile -- and the 226 text rows behind it; "generic_gate": N % 8 != 0 on the DiT's half-tile route
EXACT_CASES = [
    ("dit_qkv_bias", 6, EPI_BIAS, M_DIT, 3 * D, D, 64, 64, "bias"),
    ("dit_dense_gate", 6, EPI_GATE, M_DIT, D, D, 64, 64, "gate"),
    ("dit_h1_gate_add2_inplace", 7, EPI_GATE, M_DIT, D, 4 * D, 0, 64, "gate_add2_inplace"),
    ("rowtail_k1920_batches_in_tail", 7, EPI_GATE, 5 * 4130, D, D, 0, 0, "gate_add2_5b"),
    ("8phase_rem0_mul", 2, EPI_GENERIC, 128 * 256, 1024, 1024, 64, 64, "mul"),
    ("8phase_rem200_f32_resid", 2, EPI_GENERIC, 89 * 256 - 40, 2048, 1024, 0, 64, "resid_f32"),
    ("dit_generic_gate_n1916", 6, EPI_GENERIC, M_DIT, D - 4, D, 0, 68, "gate"),
    ("128x128_bf16_resid", 0, EPI_GENERIC, 3000, 1000, 320, 64, 24, "resid_bf16"),
    ("128x128_bias", 0, EPI_BIAS, 4444, D, D, 0, 0, "bias"),
]


def _epilogue(form, M, N, g, dev, exact, out=None, batches=None):
    """The epilogue operands of a case form (the DiT's gate layout: ada [B, 12 N], image / text offsets as in dit.py).
    batches: (B, rows per batch, text rows) of a gate form, for callers with their own shapes (tests/test_gpu_fp8_routes.py)."""
    bias = _small((N,), g, dev, -4, 4, exact, 0.5)
    if form == "bias":
        return dict(bias=bias)
    if form == "mul":
        return dict(bias=bias, mul=_small((M, N), g, dev, -2, 2, exact))
    if form == "resid_f32":
        r = torch.randint(-8, 9, (M, N), device=dev, generator=g).float() if exact else torch.randn(M, N, device=dev, generator=g)
        return dict(bias=bias, resid=r, out_f32=True)
    if form == "resid_bf16":
        return dict(bias=bias, resid=_small((M, N), g, dev, -8, 8, exact))
    B, rows, text = batches or ((5, 4130, TEXT) if form.endswith("_5b") else (2, ROWS, TEXT))
    assert M == B * rows
    ada = _gate_values((B, 12 * N), g, dev, exact)
    e = dict(bias=bias, gate=ada, gate_bstride=12 * N, rows_per_batch=rows, text_len=text)
    if form == "gate":
        e.update(gate_off_img=2 * N, gate_off_txt=8 * N, resid=_small((M, N), g, dev, -8, 8, exact))
    else:
        e.update(gate_off_img=5 * N, gate_off_txt=11 * N, add2=_small((M, N), g, dev, -8, 8, exact))
        if form.endswith("inplace"):
            out.copy_(_small((M, N), g, dev, -8, 8, exact))
            e["resid"] = out                              # the DiT's h1: h_out += gate * y (+ control add), in place
        else:
            e["resid"] = _small((M, N), g, dev, -8, 8, exact)
    return e


@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_gemm_route_exact(cuda, case):
    """Exact operands: the whole output equals the float64 reference bit for bit; the sentinels around it are untouched."""
    from landiff_amd import ops
    name, route, kind, M, N, K, lda_pad, ldo_pad, form = case
    a, w, g = _operands(M, N, K, True, zlib.crc32(name.encode()), cuda, lda_pad)
    out_dt = torch.float32 if form == "resid_f32" else BF
    bits, out = _sentinel_buffer(M, N, N + ldo_pad, out_dt, cuda)
    epi = _epilogue(form, M, N, g, cuda, True, out=out)
    assert _route(M, N, K, out.stride(0), **epi) == (route, kind)
    assert a.stride(0) == K + lda_pad
    if epi.get("resid") is out:
        epi_ref = dict(epi, resid=out.clone())
    else:
        epi_ref = epi
    ref, _ = _reference(a, w, epi_ref, True, N)
    ops.gemm(a, w, out=out, **epi)
    torch.cuda.synchronize()
    got = out.double()
    bad = got != ref
    assert not bool(bad.any()), (f"{int(bad.sum())} of {M * N} elements differ, first at "
                                 f"{tuple(bad.nonzero()[0].tolist())}; NaN (unwritten): {int(torch.isnan(got).sum())}")
    _check_sentinels(bits, M, N)


# The smallest shape that the planner sends down the half-tile route with every edge in the tail: 65 x 8 = 520 tiles = two whole
# rounds + 8 tail tiles, among them the bottom-right corner tile -- a ragged last row (37 of 256) and a half-wide last column (120 of
# 256: its second half tile is empty).
HALF_TAIL_CORNER = (64 * 256 + 37, 7 * 256 + 120, 1024)


def run_half_tail_corner(dev):
    """Exact operands, bias + residual IN PLACE (out is resid, preset) on HALF_TAIL_CORNER, the output inside the sentinel buffer:
    bit equality with the float64 reference.  A tile computed by both launches of the split adds its product twice.  (Also run in
    a child process on the variants build: tests/test_gpu_variants.py.)"""
    from landiff_amd import ops
    M, N, K = HALF_TAIL_CORNER
    lab = _tile_launch(M, N, 6)
    assert int(lab.sum()) == 8 and int(lab[-1, -1]) == 1, "the tail is 8 tiles and holds the corner tile"
    a, w, g = _operands(M, N, K, True, zlib.crc32(b"half_tail_corner"), dev, 64)
    bits, out = _sentinel_buffer(M, N, N + 64, BF, dev)
    out.copy_(_small((M, N), g, dev, -8, 8, True))
    epi = dict(bias=_small((N,), g, dev, -4, 4, True), resid=out)
    assert _route(M, N, K, out.stride(0), **epi) == (6, EPI_GENERIC)
    ref, _ = _reference(a, w, dict(epi, resid=out.clone()), True, N)
    ops.gemm(a, w, out=out, **epi)
    torch.cuda.synchronize()
    got = out.double()
    bad = got != ref
    if bool(bad.any()):
        nbm, nbn = lab.shape
        pad = torch.zeros(nbm * 256, nbn * 256, dtype=torch.bool, device=dev)
        pad[:M, :N] = bad
        per_tile = pad.view(nbm, 256, nbn, 256).any(dim=3).any(dim=1).cpu()
        twice = got == ref + (a.double() @ w.double().t() + epi["bias"].double())      # (exact operands: bias + product, once more)
        raise AssertionError(f"{int(bad.sum())} of {M * N} elements differ in {int(per_tile[lab == 0].sum())} tiles of the whole rounds and "
                             f"{int(per_tile[lab == 1].sum())} of the 8 tail tiles, first at {tuple(bad.nonzero()[0].tolist())}; "
                             f"{int((twice & bad).sum())} of them hold the product added twice; NaN: {int(torch.isnan(got).sum())}")
    _check_sentinels(bits, M, N)


@pytest.mark.parametrize("persist", ["1", "0"], ids=["persistent", "one_workgroup_per_tile"])
def test_gemm_half_tail_corner_inplace(cuda, monkeypatch, persist):
    """HALF_TAIL_CORNER with persistent workgroups and with LD_GEMM_PERSIST=0 (the knobs are re-read per call: LD_TUNING)."""
    monkeypatch.setenv("LD_GEMM_PERSIST", persist)
    run_half_tail_corner(cuda)


# (id, route, epilogue kind, M, N, K, lda pad, act, epilogue form)
RANDOM_CASES = [
    ("dit_h4_gelu_tanh", 6, EPI_GELU, M_DIT, 4 * D, D, 64, "gelu_tanh", "bias"),
    ("dit_h1_gate_add2", 7, EPI_GATE, M_DIT, D, 4 * D, 0, None, "gate_add2"),
    ("dit_dense_gelu_tanh_mul", 6, EPI_GENERIC, M_DIT, D, D, 0, "gelu_tanh", "mul"),
    ("rowtail_gelu_erf", 7, EPI_GENERIC, 5 * 4130, D, D, 0, "gelu_erf", "bias"),
    ("8phase_rem0_silu", 2, EPI_GENERIC, 128 * 256, 1024, 1024, 0, "silu", "bias"),
    ("128x128_tanh", 0, EPI_GENERIC, 3000, 1000, 320, 64, "tanh", "bias"),
    ("8phase_rem200_f32_resid", 2, EPI_GENERIC, 89 * 256 - 40, 2048, 1024, 0, None, "resid_f32"),
]


@pytest.mark.parametrize("case", RANDOM_CASES, ids=[c[0] for c in RANDOM_CASES])
def test_gemm_route_random(cuda, case):
    """Random operands: every element within its own error bound of the float64 reference; two launches give the same bits."""
    from landiff_amd import ops
    name, route, kind, M, N, K, lda_pad, act, form = case
    a, w, g = _operands(M, N, K, False, zlib.crc32(name.encode()), cuda, lda_pad)
    epi = _epilogue(form, M, N, g, cuda, False)
    if act:
        epi["act"] = act
    out_dt = torch.float32 if epi.get("out_f32") else BF
    assert _route(M, N, K, N, **epi) == (route, kind)
    ref, err = _reference(a, w, epi, False, N)
    out = torch.empty(M, N, device=cuda, dtype=out_dt)
    ops.gemm(a, w, out=out, **epi)
    d = (out.double() - ref).abs()
    over = d > err
    # (reported, not asserted: ulps of the reference where it is not tiny -- near 0 the activation's tails and the residual's
    #  cancellation make one ulp of an earlier rounding worth many of the result's)
    big = ref.abs() >= 2.0 ** -6
    ulps = (d[big] / _ulp(ref[big])).max().item()
    print(f"\n{name}: max error {ulps:.2f} bf16 ulps of the reference (|ref| >= 2^-6), "
          f"{(d / err).max().item():.3f} of the per-element bound")
    worst = divmod((d - err).flatten().argmax().item(), N)
    assert not bool(over.any()), (f"{int(over.sum())} elements over their bound, worst at {worst}: "
                                  f"{out[worst].item()} against {ref[worst].item()} +- {err[worst].item()}")
    again = torch.empty_like(out)
    ops.gemm(a, w, out=again, **epi)
    assert torch.equal(again, out)


def _tile_launch(M, N, route):
    """Which launch of the split computes each 256x256 tile (tile rows x tile columns; 0 = the 8-phase rounds, 1 = the tail): the
    raster of ld_gemm8p_kernel / ld_gemm8p_n128_kernel (xcd_remap + group_m rows of tiles) restated."""
    nbm, nbn = (M + 255) // 256, (N + 255) // 256
    ntiles, gm = nbm * nbn, (4 if nbn <= 8 else 8)
    full = ntiles // 256
    lab = torch.zeros(nbm, nbn, dtype=torch.int64)
    if route == 7:
        lab[(full * 256) // nbn:] = 1
        return lab
    q, r = divmod(ntiles, 8)
    for v in range(full * 256, ntiles):
        x, i = v % 8, v // 8
        bid = (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + i
        group, in_group = divmod(bid, gm * nbn)
        rows_here = min(nbm - group * gm, gm)
        lab[group * gm + in_group % rows_here, in_group // rows_here] = 1
    return lab


@pytest.mark.parametrize("N,K,route", [(D, D, 6), (D, 4 * D, 7)])
def test_gemm_routes_bit_identical_to_128x128(cuda, N, K, route):
    """Row slices: a DiT-shaped GEMM (bias epilogue, random operands) against the same rows computed 256 at a time as standalone
    GEMMs on the 128x128 route -- the 8-phase rounds and each tail (half tiles / the m_begin row tail) give the same bits: every
    route accumulates the same 32-deep MFMA products in the same K order."""
    from landiff_amd import ops
    M = M_DIT
    a, w, g = _operands(M, N, K, False, 77 + K, cuda)
    bias = (torch.randn(N, device=cuda, generator=g) * 0.5).to(BF)
    assert _route(M, N, K, N, bias=bias) == (route, EPI_BIAS)
    full = ops.gemm(a, w, bias=bias)
    sl = torch.empty_like(full)
    for r0 in range(0, M, 256):
        r1 = min(r0 + 256, M)
        assert _route(r1 - r0, N, K, N, bias=bias) == (0, EPI_BIAS)
        ops.gemm(a[r0:r1], w, out=sl[r0:r1], bias=bias)
    lab = _tile_launch(M, N, route)
    assert 0 < int(lab.sum()) < lab.numel()
    nbm, nbn = lab.shape
    pad = torch.zeros(nbm * 256, nbn * 256, device=cuda, dtype=torch.float64)
    d = (full.double() - sl.double()).abs() / _ulp(sl.double())
    pad[:M, :N] = d
    per_tile = pad.view(nbm, 256, nbn, 256).amax(dim=(1, 3)).cpu()
    worst = {launch: per_tile[lab == launch].max().item() for launch in (0, 1)}
    print(f"\nroute {route}, K {K}: max ulps against the 128x128 route: 8-phase rounds {worst[0]}, tail {worst[1]}")
    assert torch.equal(full, sl), worst
