"""The fp8 and MXFP8 GEMMs on every kernel family x every epilogue specialisation, element by element.

Three families run the fp8 DiT configuration's large linears:
  row    ops.gemm_fp8                          ld_gemm_f8_kernel<E, false>   per-row / per-channel fp32 scales, applied to the accumulator
  mx2s   ops.gemm_mxfp8 under LD_GEMM_MX8P=0   ld_gemm_f8_kernel<E, true>    E8M0 block scales inside v_mfma_scale_f32_32x32x64
  mx8p   ops.gemm_mxfp8, gemm_qkv_heads_mxfp8  ld_gemm8p_mx_kernel<E>        block scales inside v_mfma_scale_f32_16x16x128, persistent walk
The launchers pick the epilogue with the bf16 GEMM's pick_epilogue, so every case first asserts its kind through ld_gemm_route: a
retune that moves a case elsewhere fails here instead of losing the coverage.

Which case runs which instantiation (exact: test_fp8_route_exact, random: test_fp8_route_random):

  epilogue     row, mx2s, mx8p
  BIAS    (0)  exact bias_ragged, scale_range; random k1920_bias
  GELU    (1)  random k1920_gelu; the bf16 leg of test_fp8_gelu_mxfp8_output (mx2s, mx8p)
  GATE    (2)  exact gate_regions, gate_add2_inplace_2rounds; random gate_regions
  GENERIC (3)  exact generic_n196, generic_f32, generic_mul; random generic_n196_resid
  GELU_MX (4)  test_fp8_gelu_mxfp8_output (mx2s, mx8p: the families that have it)
  QKV     (5)  test_fp8_qkv_heads_v_exact (mx8p: the family that has it)

Exact cases: e4m3 holds -1, 0 and 1 exactly, E8M0 block scales and power-of-two row scales are exact, so with sparse ternary
operands and small-integer / power-of-two epilogue operands every accumulation and every bf16 rounding point is exact (asserted:
the premise of _reference).  The output must equal the float64 product of the dequantised operands bit for bit, inside a buffer of
NaN sentinels that must come back untouched.  A scale byte taken from the wrong block, row, lane group or K-tile slab, a skipped
or twice-computed tile, a wrong gate row or a store past M or N fails.  Operands are drawn on the host (one stream whatever the
device), so the premise can be checked without a GPU.

Random cases: MXFP8 / e4m3 quantised N(0, 1) operands against the same float64 product, every element within its own bound
(fp32 accumulation K 2^-24 sum|a||w|, one bf16 ulp per rounding, through the activation's slope and the later multiplies).
"""
import zlib

import pytest
import torch

from test_gpu_fp8 import _mx_deq, _mx_quant_ref, _row_major, _tile_major
from test_gpu_gemm_routes import (BF, EPI_BIAS, EPI_GATE, EPI_GELU, EPI_GENERIC, NAN16, _check_sentinels, _epilogue, _expand_gate,
                                  _reference, _route, _sentinel_buffer, _small, _ulp)

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
FAMILIES = ("row", "mx2s", "mx8p")
ONE, MINUS_ONE = 0x38, 0xB8                       # e4m3 codes of 1 and -1 (0x00: 0)
FILL8 = 0xA5                                      # sentinel byte around MXFP8 outputs
TEXT = 226


def _select(monkeypatch, family):
    """The MXFP8 main loop of a family (LD_GEMM_MX8P is re-read per call under LD_TUNING=1, which conftest.py sets)."""
    if family != "row":
        monkeypatch.setenv("LD_GEMM_MX8P", "1" if family == "mx8p" else "0")


class _Operands:
    """Quantised operands of one family on the device, beside their dequantised values (float64: what the reference multiplies).
    a8 is a view of a [M, K + 64] buffer (lda = K + 64) whose padding holds the code of 1."""

    def __init__(self, family, a_codes, w_codes, sa, sw, a_deq, w_deq, dev):
        M, K = a_codes.shape
        abuf = torch.full((M, K + 64), ONE, dtype=torch.uint8)
        abuf[:, :K] = a_codes
        self.family, self.a8, self.w8 = family, abuf.to(dev)[:, :K], w_codes.contiguous().to(dev)
        # row: fp32 [rows]; MX: E8M0 bytes [rows, K / 32] -> the kernels' [K / 128][rows][4]
        self.sa, self.sw = (sa.to(dev), sw.to(dev)) if family == "row" else (_tile_major(sa).to(dev), _tile_major(sw).to(dev))
        self.a, self.w = a_deq.double().to(dev), w_deq.double().to(dev)
        assert self.a8.stride(0) == K + 64

    def run(self, out=None, **kw):
        from landiff_amd import ops
        f = ops.gemm_fp8 if self.family == "row" else ops.gemm_mxfp8
        return f(self.a8, self.sa, self.w8, self.sw, out=out, **kw)


def _ternary(rows, cols, dens, g):
    """{-1, 0, 1}, non-zero with probability dens (float32, on the host)."""
    sign = torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1
    return (sign * (torch.rand(rows, cols, generator=g) < dens)).float()


def _codes(t):
    return torch.where(t > 0, ONE, torch.where(t < 0, MINUS_ONE, 0)).to(torch.uint8)


def _block_scaled(t, e):
    """t [rows, K] times 2^(e - 127) per 32-block (e: E8M0 bytes [rows, K / 32]); float64."""
    return t.double() * torch.pow(2.0, e.double() - 127).repeat_interleave(32, dim=1)


def _exact_operands(family, M, N, K, g, dev):
    """Ternary operands at density (4 / K)^0.5 (about 4 non-zero products per output); MX: an independent E8M0 exponent in
    {126, 127, 128} per (row, 32-block); row: scales in {0.5, 1, 2}."""
    dens = (4.0 / K) ** 0.5
    ta, tw = _ternary(M, K, dens, g), _ternary(N, K, dens, g)
    if family == "row":
        sa = torch.pow(2.0, torch.randint(-1, 2, (M,), generator=g).float())
        sw = torch.pow(2.0, torch.randint(-1, 2, (N,), generator=g).float())
        return _Operands(family, _codes(ta), _codes(tw), sa, sw, ta.double() * sa.double()[:, None], tw.double() * sw.double()[:, None], dev)
    ea = torch.randint(126, 129, (M, K // 32), generator=g).to(torch.uint8)
    ew = torch.randint(126, 129, (N, K // 32), generator=g).to(torch.uint8)
    return _Operands(family, _codes(ta), _codes(tw), ea, ew, _block_scaled(ta, ea), _block_scaled(tw, ew), dev)


def _scale_range_operands(family, M, N, K, g, dev):
    """A row m is non-zero in 32-block m % 16 only (ternary, density 0.25 there), W ternary at density 0.25 everywhere, and the
    scales run over 41 binades: MX bytes 107 + (7 m + 3 b) % 41 and 107 + (5 n + 11 b) % 41, written for every block (the empty ones
    too); row scales 2^((7 m) % 41 - 20) and 2^((5 n) % 41 - 20).  Every output is a small integer times one power of two anywhere
    in 2^+-40: exact in fp32 and bf16, and wrong for any wrong block, row, byte or slab -- the 16 block positions are all 4 bytes of
    all 4 K-tiles."""
    nb = K // 32
    assert nb == 16
    m, n, b = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(nb)[None, :]
    ta = _ternary(M, K, 0.25, g) * (b == m % 16).repeat_interleave(32, dim=1)
    tw = _ternary(N, K, 0.25, g)
    if family == "row":
        sa = torch.pow(2.0, ((7 * m[:, 0]) % 41 - 20).float())
        sw = torch.pow(2.0, ((5 * n[:, 0]) % 41 - 20).float())
        return _Operands(family, _codes(ta), _codes(tw), sa, sw, ta.double() * sa.double()[:, None], tw.double() * sw.double()[:, None], dev)
    ea = (107 + (7 * m + 3 * b) % 41).to(torch.uint8)
    ew = (107 + (5 * n + 11 * b) % 41).to(torch.uint8)
    return _Operands(family, _codes(ta), _codes(tw), ea, ew, _block_scaled(ta, ea), _block_scaled(tw, ew), dev)


# (id, epilogue kind, M, N, K, ldo pad, epilogue form, (batches, rows per batch, text rows))
#   bias_ragged                ragged last tile row and column, two K-tiles
#   gate_regions               the DiT's dense form (gate offsets 2N / 8N, out != resid): batch boundaries at 1000 and 2000 inside
#                              256-row tiles, text rows, a second tile column 64 wide (three of mx8p's wave columns not live), 3 K-tiles
#   gate_add2_inplace_2rounds  the DiT's h1 form (gate offsets 5N / 11N, add2, out is resid): 65 x 4 = 260 tiles -- more than CUs, so
#                              mx8p walks a second round with the next-tile prefetch hook; one K-tile; a tile computed twice adds
#                              its product twice
#   generic_n196               N % 8 != 0: the scalar store path;  generic_f32: fp32 output, fp32 residual;  generic_mul: `mul`, a
#                              third tile column 8 wide
#   scale_range                _scale_range_operands
EXACT_CASES = [
    ("bias_ragged", EPI_BIAS, 300, 200, 256, 8, "bias", None),
    ("gate_regions", EPI_GATE, 3 * 1000, 320, 384, 64, "gate", (3, 1000, TEXT)),
    ("gate_add2_inplace_2rounds", EPI_GATE, 2 * 8320, 1024, 128, 64, "gate_add2_inplace", (2, 8320, TEXT)),
    ("generic_n196", EPI_GENERIC, 515, 196, 256, 4, "resid_bf16", None),
    ("generic_f32", EPI_GENERIC, 515, 200, 128, 8, "resid_f32", None),
    ("generic_mul", EPI_GENERIC, 260, 520, 256, 8, "mul", None),
    ("scale_range", EPI_BIAS, 512, 256, 512, 0, None, None),
]


def _to_dev(epi, dev, keep=None):
    return {k: (v.to(dev) if torch.is_tensor(v) and v is not keep else v) for k, v in epi.items()}


def build_exact(case, family, dev):
    """(operands, sentinel bits, out view, epilogue, float64 reference) of an exact case; `dev` may be the host: _reference asserts
    the premise that every value the kernel rounds is a bf16 (or fp32) number already."""
    name, kind, M, N, K, ldo_pad, form, batches = case
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{family}".encode()))
    opnd = (_scale_range_operands if name == "scale_range" else _exact_operands)(family, M, N, K, g, dev)
    out_dt = torch.float32 if form == "resid_f32" else BF
    bits, out = _sentinel_buffer(M, N, N + ldo_pad, out_dt, dev)
    epi = _to_dev(_epilogue(form, M, N, g, "cpu", True, out=out, batches=batches), dev, keep=out) if form else {}
    epi_ref = dict(epi, resid=out.clone()) if epi.get("resid") is out else epi
    ref, _ = _reference(opnd.a, opnd.w, epi_ref, True, N)
    return opnd, bits, out, epi, ref


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_fp8_route_exact(cuda, monkeypatch, case, family):
    """Exact operands: the whole output equals the float64 reference bit for bit; the sentinels around it are untouched."""
    name, kind, M, N, K, ldo_pad, form, batches = case
    _select(monkeypatch, family)
    opnd, bits, out, epi, ref = build_exact(case, family, cuda)
    rc, got_kind = _route(M, N, K, out.stride(0), **epi)
    assert rc >= 0 and got_kind == kind, (rc, got_kind)
    if name == "gate_add2_inplace_2rounds":
        assert torch.cuda.get_device_properties(cuda).multi_processor_count < 260, "the persistent walk needs a second round"
        assert epi["resid"] is out and epi["add2"] is not None
    opnd.run(out=out, **epi)
    torch.cuda.synchronize()
    got = out.double()
    bad = got != ref
    if bool(bad.any()):
        msg = (f"{int(bad.sum())} of {M * N} elements differ, first at {tuple(bad.nonzero()[0].tolist())}; "
               f"NaN (unwritten): {int(torch.isnan(got).sum())}")
        if name == "gate_add2_inplace_2rounds":     # the epilogue once more on its own result: resid + gate * y + add2
            gv = _expand_gate(epi["gate"], M, N, epi["rows_per_batch"], epi["text_len"], epi["gate_off_img"], epi["gate_off_txt"])
            twice = ref + gv * (opnd.a @ opnd.w.t() + epi["bias"].double()) + epi["add2"].double()
            msg += f"; {int((bad & (got == twice.to(BF).double())).sum())} of them hold the product added twice"
        raise AssertionError(msg)
    _check_sentinels(bits, M, N)


def test_fp8_qkv_heads_v_exact(cuda):
    """ld_gemm_qkv_heads_mxfp8 (mx8p's EPI_QKV) on exact operands: V^T[b][h][:, :N] equals the float64 a @ w_v^T + bias bit for bit,
    and of q, k and vt -- pre-filled with the sentinel -- everything at token index >= N comes back untouched.  (q and k go through
    LayerNorm: test_gpu_fp8.py checks them.)"""
    from landiff_amd import ops
    B, N, H, K, Npad = 2, 304, 3, 256, 384
    g = torch.Generator().manual_seed(zlib.crc32(b"qkv_heads_v_exact"))
    opnd = _exact_operands("mx8p", B * N, 3 * H * 64, K, g, cuda)
    bias = _small((3 * H * 64,), g, "cpu", -4, 4, True).to(cuda)
    ln = tuple((torch.randn(64, generator=g) * 0.2 + o).to(cuda, BF) for o in (1.0, 0.0, 1.0, 0.0))
    ref, _ = _reference(opnd.a, opnd.w[2 * H * 64:], dict(bias=bias[2 * H * 64:]), True, H * 64)      # [B N, H 64]: the v third
    ref = ref.view(B, N, H, 64).permute(0, 2, 3, 1)
    fill = lambda *shape: torch.full(shape, NAN16, device=cuda, dtype=torch.int16)
    qb, kb, vb = fill(B, H, Npad, 64), fill(B, H, Npad, 64), fill(B, H, 64, Npad)
    ops.gemm_qkv_heads_mxfp8(opnd.a8, opnd.sa, opnd.w8, opnd.sw, bias, qb.view(BF), kb.view(BF), vb.view(BF), B, N, H, Npad, ln, eps=1e-6)
    torch.cuda.synchronize()
    got = vb.view(BF)[..., :N].double()
    bad = got != ref
    assert not bool(bad.any()), (f"{int(bad.sum())} of {bad.numel()} elements of V^T differ, first at (b, h, d, n) = "
                                 f"{tuple(bad.nonzero()[0].tolist())}; NaN (unwritten): {int(torch.isnan(got).sum())}")
    assert bool((vb[..., N:] == NAN16).all()), "V^T written at a token index >= N"
    assert bool((qb[:, :, N:] == NAN16).all()) and bool((kb[:, :, N:] == NAN16).all()), "q / k written at a token index >= N"
    assert not bool((qb[:, :, :N] == NAN16).any()) and not bool((kb[:, :, :N] == NAN16).any()), "a q / k row left unwritten"


def _random_operands(family, M, N, K, g, dev):
    """MX: _mx_quant_ref of bf16 N(0, 1) with A's 32-blocks scaled by logspace(-2, 1), W by K^-0.5; row: e4m3 casts of N(0, 1) with
    positive random scales (outputs of order 1 in both)."""
    if family == "row":
        a8 = torch.randn(M, K, generator=g).to(F8)
        w8 = (torch.randn(N, K, generator=g) * 0.5).to(F8)
        sa = torch.rand(M, generator=g) + 0.5
        sw = (torch.rand(N, generator=g) + 0.5) * 2.0 * K ** -0.5
        return _Operands(family, a8.view(torch.uint8), w8.view(torch.uint8), sa, sw,
                         a8.float().double() * sa.double()[:, None], w8.float().double() * sw.double()[:, None], dev)
    a = (torch.randn(M, K, generator=g) * torch.logspace(-2, 1, K // 32).repeat_interleave(32)[None, :]).to(BF)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF)
    a8, ea = _mx_quant_ref(a)
    w8, ew = _mx_quant_ref(w)
    return _Operands(family, a8, w8, ea, ew, _mx_deq(a8, ea), _mx_deq(w8, ew), dev)


# (id, epilogue kind, M, N, K, epilogue form, activation, (batches, rows per batch, text rows))
RANDOM_CASES = [
    ("k1920_gelu", EPI_GELU, 700, 512, 1920, "bias", "gelu_tanh", None),                    # 15 K-tiles
    ("k1920_bias", EPI_BIAS, 700, 512, 1920, "bias", None, None),
    ("gate_regions", EPI_GATE, 3 * 1000, 320, 384, "gate", None, (3, 1000, TEXT)),
    ("generic_n196_resid", EPI_GENERIC, 515, 196, 256, "resid_bf16", None, None),
]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", RANDOM_CASES, ids=[c[0] for c in RANDOM_CASES])
def test_fp8_route_random(cuda, monkeypatch, case, family):
    """Random operands: every element within its own error bound of the float64 product of the dequantised operands.  The
    accumulation term is the derived K 2^-24 sum|a||w| of _reference (row: the two fp32 roundings of acc * (scale_a * scale_w) are
    2^-23 |acc|, far inside it at K >= 256).  The derived term held on all three families (worst element at 0.995 of its bound, a
    bf16 rounding of the Linear output that falls the other way), so no coefficient was measured for v_mfma_scale_*.  These cases do
    not see a wrong scale on a small block: the exact cases do."""
    name, kind, M, N, K, form, act, batches = case
    _select(monkeypatch, family)
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{family}".encode()))
    opnd = _random_operands(family, M, N, K, g, cuda)
    epi = _to_dev(_epilogue(form, M, N, g, "cpu", False, batches=batches), cuda)
    if act:
        epi["act"] = act
    rc, got_kind = _route(M, N, K, N, **epi)
    assert rc >= 0 and got_kind == kind, (rc, got_kind)
    ref, err = _reference(opnd.a, opnd.w, epi, False, N)
    out = opnd.run(**epi)
    d = (out.double() - ref).abs()
    over = d > err
    acc_rel = (d / (opnd.a.abs() @ opnd.w.abs().t())).max().item()       # (an upper estimate: d holds the bf16 roundings too)
    big = ref.abs() >= 2.0 ** -6
    print(f"\n{name}[{family}]: max error {(d[big] / _ulp(ref[big])).max().item():.2f} bf16 ulps of the reference (|ref| >= 2^-6), "
          f"{(d / err).max().item():.3f} of the per-element bound; max |got - ref| / sum|a||w| = {acc_rel:.3e} "
          f"(accumulation term: K 2^-24 = {K * 2.0 ** -24:.3e})")
    worst = divmod((d - err).flatten().argmax().item(), N)
    assert not bool(over.any()), (f"{int(over.sum())} elements over their bound, worst at {worst}: "
                                  f"{out[worst].item()} against {ref[worst].item()} +- {err[worst].item()}")


@pytest.mark.parametrize("family", ["mx2s", "mx8p"])
def test_fp8_gelu_mxfp8_output(cuda, monkeypatch, family):
    """The MXFP8-writing GELU epilogue (EPI_GELU_MX) on both MX loops: codes and scale bytes equal the torch restatement of the MX
    quantiser (_mx_quant_ref, not the library's) applied to the bf16 output of the same loop's bias + GELU launch, bit for bit;
    nothing of the code buffer outside [M, N] is written.  (That bf16 output is checked by test_fp8_route_random.)"""
    _select(monkeypatch, family)
    M, N, K = 700, 768, 256
    g = torch.Generator().manual_seed(zlib.crc32(f"gelu_mx/{family}".encode()))
    opnd = _random_operands(family, M, N, K, g, cuda)
    bias = torch.randn(N, generator=g).to(cuda, BF)
    rc, kind = _route(M, N, K, N, bias=bias, act="gelu_tanh")
    assert rc >= 0 and kind == EPI_GELU
    h = opnd.run(bias=bias, act="gelu_tanh")
    want_q, want_s = _mx_quant_ref(h.cpu())
    qbuf = torch.full((M + 3, N + 8), FILL8, device=cuda, dtype=torch.uint8)
    sc = torch.full((N // 128, M, 4), FILL8, device=cuda, dtype=torch.uint8)
    opnd.run(out=qbuf[:M, :N], out_scales=sc, bias=bias, act="gelu_tanh")
    torch.cuda.synchronize()
    qbuf, sc = qbuf.cpu(), _row_major(sc.cpu())
    bad_s, bad_q = sc != want_s, qbuf[:M, :N] != want_q
    assert not bool(bad_s.any()), f"{int(bad_s.sum())} of {bad_s.numel()} scale bytes differ, first at {tuple(bad_s.nonzero()[0].tolist())}"
    assert not bool(bad_q.any()), f"{int(bad_q.sum())} of {bad_q.numel()} codes differ, first at {tuple(bad_q.nonzero()[0].tolist())}"
    assert bool((qbuf[M:] == FILL8).all()) and bool((qbuf[:M, N:] == FILL8).all()), "a code stored past M or N"
