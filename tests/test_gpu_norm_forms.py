"""The forms of ld_norm_layer.hip, ld_norm_qkv.hip and ld_norm_group.hip that no direct test reached: the general LayerNorm kernel
(fp32 in / out, no weights, D above 2048, with modulation where the two-rows-per-wave kernel does not take the call), that kernel
against the two-rows-per-wave one, ld_qkv_split in its three modes, the GroupNorm statistics at 2 / 4 / 8 / 64 channels per group and both GroupNorm-apply kernels -- each against a plain
float64 reference (tests/kernel_ref.py) through landiff_amd.ops, outputs inside NaN sentinels.

The kernel choice is made through the arguments: fp32 in or out, no weights or D > 2048 reach the general LayerNorm kernel; a channel
count with 256 % (C / 8) != 0 reaches the flat GroupNorm kernel.  LD_LN_FAST=0 and LD_GN_ROWS=0 choose the same kernels for any
arguments; they are knobs like every other (re-read per call under LD_TUNING=1, conftest), and one test uses the first.

Classes (kernel_ref's docstring): B for LayerNorm without modulation, QK-LayerNorm and RoPE; C for LayerNorm + modulate and GroupNorm +
SpatialNorm + swish; A for the plain split, V in every mode and all padding.

Measured on an MI355X (worst |err| / bound, least bit-equal share): general LayerNorm bf16 out 0.500 (a half-ulp rounding), 0.9981 at
D 520 and >= 0.9993 elsewhere, fp32 out 0.115 ... 0.174 of the 4 x torch bound; LayerNorm + modulate on the general kernel and on the
two-rows-per-wave kernel: every element equal to the chain; the two kernels bit-equal (0 of 1152 / 6912 / 17280 elements differ);
QK-LayerNorm 0.500, 0.99976; RoPE 0.500, 1.0; GroupNorm apply 0.558, 0.99996 with zq, one element a whole step off without
(ratio 1.000 to three digits: the bound is one ulp plus the fp32 term), 0.99981; LD_GN_FAST_RCP=0 equal to the default in every element."""
import pytest
import torch

import kernel_ref as kr
from kernel_ref import BF

pytestmark = pytest.mark.gpu

LN_EPS = 1e-5
PAD = 8                        # extra columns of every row (ldx, ldo = D + 8: a multiple of 8 bf16 and of 4 fp32 elements)
EXTRA_ROWS = 3


def _ln_run(cuda, x, w, b, out_dtype, **mod):
    """x [rows, D] (bf16 or fp32) inside a [rows, D + PAD] buffer, out inside a sentinel [rows + EXTRA_ROWS, D + PAD] buffer; returns
    the output rows on the CPU after checking that nothing else was written."""
    from landiff_amd import ops
    rows, D = x.shape
    xbuf = torch.full((rows, D + PAD), float("nan"), dtype=x.dtype, device=cuda)
    xbuf[:, :D] = x.to(cuda)
    ob = kr.sentinels((rows + EXTRA_ROWS, D + PAD), out_dtype, cuda)
    dev = lambda t: None if t is None else t.to(cuda)
    ops.layernorm(xbuf[:, :D], dev(w), dev(b), ob.view(out_dtype)[:rows, :D], LN_EPS, **mod)
    torch.cuda.synchronize()
    written = torch.zeros(ob.shape, dtype=torch.bool)
    written[:rows, :D] = True
    kr.check_untouched(ob, written, f"ld_layernorm rows={rows} D={D}")
    return ob.cpu().view(out_dtype)[:rows, :D]


@pytest.mark.parametrize("D", [8, 64, 512, 520, 1920, 2048, 2056, 4096])
def test_layernorm_general_forms(cuda, D):
    """Class B: {x bf16, fp32} x {out bf16, fp32} x {affine, no weights} x rows {1, 5, 9} without modulation -- the general kernel --
    against float64 F.layer_norm (nn.LayerNorm of blocks.py:292-304 and dit_video_concat.py:577-586).  D covers 1, 2, 4, 5 (-> the 8-chunk
    instantiation) and 8 chunks per lane, a partly used last chunk and the D <= 4096 limit.  bf16 out: one bf16 step + 4 x torch's own
    fp32 error, >= 99 % correctly rounded; fp32 out: 4 x torch's fp32 error.  The CPU fp32 evaluation meets the same checker."""
    worst_b, worst_f, least_equal = 0.0, 0.0, 1.0
    for rows in (1, 5, 9):
        for x_f32 in (False, True):
            for affine in (True, False):
                x, w, b = kr.ln_inputs(rows, D, 131 * rows + D + x_f32, x_f32)
                if not affine:
                    w = b = None
                ref, t32 = kr.layernorm_ref(x, w, b, LN_EPS)
                noise = kr.f32_noise(ref, t32)
                what = f"rows={rows} D={D} x={'f32' if x_f32 else 'bf16'} {'affine' if affine else 'no weights'}"
                kr.check_one_rounding(t32.to(BF), ref, noise, "CPU fp32 " + what)
                r, e = kr.check_one_rounding(_ln_run(cuda, x, w, b, BF), ref, noise, "ld_layernorm bf16 out " + what)
                worst_b, least_equal = max(worst_b, r), min(least_equal, e)
                worst_f = max(worst_f, kr.check_f32(_ln_run(cuda, x, w, b, torch.float32), ref, t32, "ld_layernorm f32 out " + what))
    print(f"ld_layernorm general D={D}: bf16 out worst |err| / bound {worst_b:.3f}, least bit-equal share {least_equal:.6f}; f32 out worst |err| / bound {worst_f:.3f}")


@pytest.mark.parametrize("what", ["D_not_8k", "D_above_4096", "w_without_b"])
def test_layernorm_refusals(cuda, what):
    from landiff_amd import ops
    from landiff_amd._lib import LandiffHipError
    D = {"D_not_8k": 12, "D_above_4096": 4104}.get(what, 64)
    x = torch.ones(2, D, dtype=BF, device=cuda)
    w = torch.ones(D, dtype=BF, device=cuda)
    ob = kr.sentinels((2, D), BF, cuda)
    with pytest.raises(LandiffHipError):
        ops.layernorm(x, w, None if what == "w_without_b" else w, ob.view(BF), LN_EPS)
    torch.cuda.synchronize()
    assert bool(kr.is_sentinel(ob).all())


# rows_per_batch 5, text_len 2 over 9 rows: the text / image boundary (row 2) falls inside the first block of 4 rows (one wave each), the
# batch boundary (row 5) and batch 1's text / image boundary (row 7) inside the second; the two-rows-per-wave kernel sees row pairs
# (4, 5) and (6, 7) with different vectors and (8) alone
MOD_ROWS, MOD_RPB, MOD_TEXT = 9, 5, 2


def _mod_case(D, seed):
    x, w, b = kr.ln_inputs(MOD_ROWS, D, seed)
    g = torch.Generator().manual_seed(seed + 1)
    ada = (0.3 * torch.randn(2, 4 * D, generator=g)).to(BF)
    offs = dict(shift_img=0, scale_img=D, shift_txt=2 * D, scale_txt=3 * D)
    shift = kr.modulate_rows(ada, MOD_ROWS, MOD_RPB, MOD_TEXT, 0, 2 * D, D)
    scale = kr.modulate_rows(ada, MOD_ROWS, MOD_RPB, MOD_TEXT, D, 3 * D, D)
    return x, w, b, ada, offs, shift, scale


def _mod_run(cuda, x, w, b, ada, offs, out_dtype):
    return _ln_run(cuda, x, w, b, out_dtype, mod=ada.to(cuda), mod_bstride=ada.shape[1], rows_per_batch=MOD_RPB, text_len=MOD_TEXT, **offs)


@pytest.mark.parametrize("D,out_f32", [(2056, False), (4096, False), (1920, True)])
def test_layernorm_modulate_on_the_general_kernel(cuda, D, out_f32):
    """Class C: LayerNorm + modulate() = x * (1 + scale) + shift in bf16 ops (dit_video_concat.py:388) in the forms the two-rows-per-wave
    kernel does not take -- D above 2048, fp32 output (which stores the bf16-rounded values).  Rounding points as the kernel comment
    lists them: the LayerNorm output, 1 + scale, the product, the sum."""
    x, w, b, ada, offs, shift, scale = _mod_case(D, D)
    ref, bound = kr.ln_modulate_ref(x, w, b, LN_EPS, shift, scale)
    kr.check_chain(kr.ln_modulate_cpu32(x, w, b, LN_EPS, shift, scale), ref, bound, f"CPU fp32 LN + modulate D={D}")
    got = _mod_run(cuda, x, w, b, ada, offs, torch.float32 if out_f32 else BF)
    if out_f32:
        assert torch.equal(got, got.to(BF).float()), "the fp32 output of the modulated form holds bf16-rounded values"
    kr.check_chain(got, ref, bound, f"ld_layernorm + modulate, general kernel, D={D} {'f32' if out_f32 else 'bf16'} out")


@pytest.mark.parametrize("D", [128, 768, 1920])
def test_layernorm_mod_kernel_equals_general_kernel(cuda, monkeypatch, D):
    """The two-rows-per-wave kernel (bf16 out) against the general kernel (the same call with fp32 output, which stores the
    bf16-rounded values, and the same bf16-out call under LD_LN_FAST=0): "the same operations at the same roundings"
    (ld_norm_layer.hip) -- bit equality, over an odd row count with region and batch boundaries inside row pairs.  The
    two-rows-per-wave kernel is also held to the class-C chain on its own."""
    x, w, b, ada, offs, shift, scale = _mod_case(D, 3 * D)
    ref, bound = kr.ln_modulate_ref(x, w, b, LN_EPS, shift, scale)
    fast = _mod_run(cuda, x, w, b, ada, offs, BF)
    general = _mod_run(cuda, x, w, b, ada, offs, torch.float32)
    kr.check_chain(fast, ref, bound, f"ld_layernorm + modulate, two-rows-per-wave kernel, D={D}")
    differ = fast.float() != general
    print(f"two-rows-per-wave vs general kernel, D={D}: {int(differ.sum())} of {differ.numel()} elements differ, largest difference "
          f"{(fast.float() - general).abs().max().item():.3e}")
    kr.check_bits(fast.float(), general, f"two-rows-per-wave kernel vs general kernel, D={D}")
    monkeypatch.setenv("LD_LN_FAST", "0")
    kr.check_bits(_mod_run(cuda, x, w, b, ada, offs, BF), fast, f"general kernel, bf16 out (LD_LN_FAST=0) vs two-rows-per-wave kernel, D={D}")


# ---- head split ---------------------------------------------------------------------------------------------------------------
SPLIT_SHAPES = [(2, 70, 3, 128), (1, 64, 1, 64)]       # (B, N, H, Npad): one partly filled + one wholly padded 64-token block; exact
SPLIT_TAIL = 64


def _split_run(cuda, qkv, B, N, H, Npad, **kw):
    from landiff_amd import ops
    n = B * H * Npad * 64
    bufs = [kr.sentinels((n + SPLIT_TAIL,), BF, cuda) for _ in range(3)]
    q, k, vt = (b.view(BF)[:n] for b in bufs)
    dev = lambda t: None if t is None else tuple(u.to(cuda) for u in t)
    ops.qkv_split(qkv.to(cuda), q.view(B, H, Npad, 64), k.view(B, H, Npad, 64), vt.view(B, H, 64, Npad), B, N, H, Npad,
                  ln=dev(kw.get("ln")), rope=dev(kw.get("rope")), eps=1e-6)
    torch.cuda.synchronize()
    return [b.cpu() for b in bufs]


def _split_structure(got, want, B, N, H, Npad, what):
    """Class A parts of a normalising / rotating split: V^T whole, the zero padding rows [N, Npad) of Q and K, the tails."""
    kr.check_bits(got[2], want[2], what + ": V^T, its zero padding columns and its tail")
    for name, g, w in (("Q", got[0], want[0]), ("K", got[1], want[1])):
        kr.check_bits(g[-SPLIT_TAIL:], w[-SPLIT_TAIL:], f"{what}: behind {name}")
        kr.check_bits(g[:-SPLIT_TAIL].view(B, H, Npad, 64)[:, :, N:], w[:-SPLIT_TAIL].view(B, H, Npad, 64)[:, :, N:], f"{what}: padding rows of {name}")
    return [g[:-SPLIT_TAIL].view(BF).view(B, H, Npad, 64)[:, :, :N] for g in got[:2]]


def _split_case(B, N, H, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * N, 3 * H * 64, generator=g).to(BF)
    return g, qkv, tuple(t.contiguous() for t in kr.qkv_thirds(qkv, B, N, H))


@pytest.mark.parametrize("B,N,H,Npad", SPLIT_SHAPES)
def test_qkv_split_plain(cuda, B, N, H, Npad):
    """Class A, mode 2 (the Theia ViT's split): Q, K rows and V^T columns are the qkv thirds' bits, padding zero, tails untouched."""
    g, qkv, (q, k, v) = _split_case(B, N, H, 21)
    got = _split_run(cuda, qkv, B, N, H, Npad)
    for name, a, w in zip(("Q", "K", "V^T"), got, kr.qkv_expect_bits(q, k, v, Npad, SPLIT_TAIL)):
        kr.check_bits(a, w, f"ld_qkv_split mode 2 {name} B={B} N={N} H={H} Npad={Npad}")


@pytest.mark.parametrize("B,N,H,Npad", SPLIT_SHAPES)
def test_qkv_split_qk_layernorm(cuda, B, N, H, Npad):
    """Mode 0: query_layernorm / key_layernorm = LayerNorm(64, eps 1e-6) per head (dit_video_concat.py:649-653), class B against float64;
    V, padding and tails class A."""
    g, qkv, (q, k, v) = _split_case(B, N, H, 22)
    ln = tuple((s * torch.randn(64, generator=g) + o).to(BF) for s, o in ((0.1, 1.0), (0.1, 0.0), (0.1, 1.0), (0.1, 0.0)))
    got = _split_run(cuda, qkv, B, N, H, Npad, ln=ln)
    gq, gk = _split_structure(got, kr.qkv_expect_bits(q, k, v, Npad, SPLIT_TAIL), B, N, H, Npad, "ld_qkv_split mode 0")
    for name, t, gt, w, b in (("Q", q, gq, ln[0], ln[1]), ("K", k, gk, ln[2], ln[3])):
        ref, cpu, noise = kr.qk_layernorm_ref(t, w, b)
        kr.check_one_rounding(cpu, ref, noise, f"CPU fp32 QK-LayerNorm {name}")
        kr.check_one_rounding(gt, ref, noise, f"ld_qkv_split mode 0 {name} B={B} N={N} H={H}")


@pytest.mark.parametrize("B,N,H,Npad", SPLIT_SHAPES)
def test_qkv_split_rope(cuda, B, N, H, Npad):
    """Mode 1: interleaved-pair RoPE with an fp32 [N][32] table (tokenizer/modules/blocks.py:172-180), class B against float64; V, padding
    and tails class A."""
    g, qkv, (q, k, v) = _split_case(B, N, H, 23)
    ang = torch.rand(N, 32, generator=g) * 6.2831853
    rope = (torch.cos(ang), torch.sin(ang))
    got = _split_run(cuda, qkv, B, N, H, Npad, rope=rope)
    gq, gk = _split_structure(got, kr.qkv_expect_bits(q, k, v, Npad, SPLIT_TAIL), B, N, H, Npad, "ld_qkv_split mode 1")
    for name, t, gt in (("Q", q, gq), ("K", k, gk)):
        ref, cpu, noise = kr.rope_ref(t, *rope)
        kr.check_one_rounding(cpu, ref, noise, f"CPU fp32 RoPE {name}")
        kr.check_one_rounding(gt, ref, noise, f"ld_qkv_split mode 1 {name} B={B} N={N} H={H}")


@pytest.mark.parametrize("what", ["Npad_not_64k", "Npad_below_N", "mode0_without_weights", "mode1_without_tables"])
def test_qkv_split_refusals(cuda, what):
    from landiff_amd import ops
    from landiff_amd._lib import LandiffHipError
    N, Npad = (70, 64) if what == "Npad_below_N" else (64, 100) if what == "Npad_not_64k" else (64, 64)
    qkv = torch.ones(N, 192, dtype=BF, device=cuda)
    bufs = [kr.sentinels((128 * 64,), BF, cuda) for _ in range(3)]
    kw = dict(ln=(None,) * 4) if what == "mode0_without_weights" else dict(rope=(None, None)) if what == "mode1_without_tables" else {}
    with pytest.raises(LandiffHipError):
        ops.qkv_split(qkv, *(b.view(BF) for b in bufs), 1, N, 1, Npad, **kw)
    torch.cuda.synchronize()
    assert all(bool(kr.is_sentinel(b).all()) for b in bufs)


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------
def _gn_x(Fn, P, C, seed):
    g = torch.Generator().manual_seed(seed)
    return g, (torch.randn(Fn, P, C, generator=g) * 1.5 + 0.3).to(BF)


@pytest.mark.parametrize("Fn,P,C,G", [(1, 1, 64, 32), (2, 515, 64, 16), (1, 4100, 128, 32), (3, 77, 24, 3), (1, 300, 2048, 32)])
def test_groupnorm_stats(cuda, Fn, P, C, G):
    """float64 sums of the bf16 values per (frame group, group), relative to sum |x| and sum x^2 as test_conv_groupnorm_partials takes
    them.  2, 4, 8 and 64 channels per group; a P that ends inside a 512-row block and inside an 8-row unrolled trip; a chunk count (3)
    that does not divide 256; the widest row; F > 1.  A second call gives the same bits; nothing behind the F * G pairs is written.
    The bound is the a-priori one of recursive summation, n 2^-24 of the sum of the terms' magnitudes, with n the fp32 additions a
    thread chains before everything continues in double: ceil(min(P, 512) / (256 // (C / 8))) rows of its chunk, 8 elements each (or
    C / G of them per sub-group slot).  That is 2 ... 128 additions (1.2e-7 ... 7.6e-6) for the first four cases and 2400 (1.4e-4) for
    the 2048-wide row, where one thread walks all 300 rows of its chunk.  (A first version of this test borrowed
    test_conv_groupnorm_partials' 2e-6, which belongs to its 256-addition patches; the wide case measured 4.596e-6 on an MI355X, and a
    CPU emulation of the kernel's stated order -- fp32 per thread in row order, double above -- gives the same 4.5961e-6: the kernel
    adds what it says, in fp32.)  Measured: 0, 6.8e-8, 1.6e-7, 1.3e-8, 4.6e-6.  A dropped row or element is 1 / 300 ... 1 / 2400 of a sum."""
    from landiff_amd import ops
    _, x = _gn_x(Fn, P, C, P + C)
    want, scale = kr.gn_sums_ref(x, Fn, P, C, G)
    xd = x.to(cuda)
    outs = []
    for _ in range(2):
        buf = torch.full((Fn * G * 2 + 8,), float("nan"), dtype=torch.float64, device=cuda)
        ops.groupnorm_stats(xd, buf[:Fn * G * 2], Fn, P, C, G)
        torch.cuda.synchronize()
        assert torch.isnan(buf[Fn * G * 2:]).all()
        outs.append(buf[:Fn * G * 2].cpu().view(Fn, G, 2))
    rel = ((outs[0] - want).abs() / scale).max().item()
    cpg, rstep = C // G, 256 // (C // 8)
    adds = -(-min(P, 512) // rstep) * min(cpg, 8)
    bound = adds * 2.0 ** -24
    print(f"ld_groupnorm_stats F={Fn} P={P} C={C} G={G}: worst |err| / (sum |x|, sum x^2) {rel:.3e}, bound {bound:.3e} ({adds} chained fp32 additions)")
    assert torch.isfinite(outs[0]).all() and rel <= bound, (rel, bound)
    assert torch.equal(outs[0], outs[1])


def test_groupnorm_stats_refuses_one_channel_per_group(cuda):
    """C / G == 1 needs eight sub-group slots per thread where the kernel keeps four: refused (it used to return aliased sums)."""
    from landiff_amd import ops
    from landiff_amd._lib import LandiffHipError
    _, x = _gn_x(1, 16, 32, 1)
    stats = torch.full((32 * 2,), float("nan"), dtype=torch.float64, device=cuda)
    with pytest.raises(LandiffHipError):
        ops.groupnorm_stats(x.to(cuda), stats, 1, 16, 32, 32)
    torch.cuda.synchronize()
    assert torch.isnan(stats).all()


GN_PADS = (2, 1, 1)


def _gn_apply_run(cuda, x, sums, gamma, beta, zy, zb, Fn, T, H, W, C, G, swish):
    from landiff_amd import ops
    tp, hp, wp = GN_PADS
    shape = (Fn, T + tp, H + 2 * hp, W + 2 * wp, C)
    n = Fn * (T + tp) * (H + 2 * hp) * (W + 2 * wp) * C
    ob = kr.sentinels((n + 64,), BF, cuda)
    dev = lambda t: None if t is None else t.to(cuda)
    ops.groupnorm_apply(x.to(cuda), ob.view(BF), sums.to(cuda), gamma.to(cuda), beta.to(cuda), Fn, T, H, W, C, G, zy=dev(zy), zb=dev(zb),
                        zshape=tuple(zy.shape[:3]) if zy is not None else (1, 1, 1), tpad=tp, hpad=hp, wpad=wp, swish=swish, eps=1e-6)
    torch.cuda.synchronize()
    written = torch.zeros(n + 64, dtype=torch.bool)
    written[:n].view(shape)[:, tp:, hp:hp + H, wp:wp + W] = True
    kr.check_untouched(ob, written, "ld_groupnorm_apply: borders, halo frames and tail")
    return ob.cpu()[:n].view(BF).view(shape)[:, tp:, hp:hp + H, wp:wp + W]


@pytest.mark.parametrize("swish", [True, False], ids=["swish", "noswish"])
@pytest.mark.parametrize("W", [12, 9], ids=["w12from3", "w9from3"])
@pytest.mark.parametrize("C,G", [(24, 3), (64, 32)], ids=["flat_c24", "rows_c64"])
def test_groupnorm_apply(cuda, monkeypatch, C, G, W, swish):
    """Class C on both kernels (C 24: 3 chunks do not divide 256, the flat kernel; C 64: the rows kernel): GroupNorm in float64 -> bf16,
    SpatialNorm3D.forward's own F.interpolate(mode="nearest") calls with the first frame apart for odd T (cp_enc_dec.py:546-569), then
    norm * y + b and swish in bf16 steps.  F 2, T 3 <- 2, H 6 <- 3, W 12 <- 3 (a shift) and 9 <- 3 (the general rule); for these ratios
    torch's float-scale nearest rule equals the kernel's integer rule (asserted; tests/test_kernel_ref_host.py has where it does not).
    The statistics handed in are the float64 sums.  LD_GN_FAST_RCP=0 (the IEEE division) meets the same chain and is at most one bf16
    step from the default (v_rcp_f32)."""
    Fn, T, H = 2, 3, 6
    g, x = _gn_x(Fn * T, H * W, C, C + W)
    x = x.view(Fn * T, H, W, C)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).to(BF), (0.2 * torch.randn(C, generator=g)).to(BF)
    zy, zb = torch.randn(2, 3, 3, C, generator=g).to(BF), torch.randn(2, 3, 3, C, generator=g).to(BF)
    zyg, zbg = kr.zq_gather_torch(zy, T, H, W), kr.zq_gather_torch(zb, T, H, W)
    assert torch.equal(zyg, kr.zq_gather_int(zy, T, H, W)) and torch.equal(zbg, kr.zq_gather_int(zb, T, H, W))
    sums, _ = kr.gn_sums_ref(x, Fn, T * H * W, C, G)
    a = (Fn, T, H, W, C, G)
    ref, bound = kr.gn_apply_ref(x, sums, gamma, beta, *a, 1e-6, zy=zyg, zb=zbg, swish=swish)
    kr.check_chain(kr.gn_apply_cpu32(x, sums, gamma, beta, *a, 1e-6, zy=zyg, zb=zbg, swish=swish), ref, bound, f"CPU fp32 GN + SpatialNorm C={C} W={W} swish={swish}")
    got = _gn_apply_run(cuda, x, sums, gamma, beta, zy, zb, *a, swish)
    kr.check_chain(got, ref, bound, f"ld_groupnorm_apply C={C} G={G} W={W} swish={swish}")
    # without zq: GroupNorm (+ swish) alone (vq_gan_blocks.py:29-38)
    ref0, bound0 = kr.gn_apply_ref(x, sums, gamma, beta, *a, 1e-6, swish=swish)
    kr.check_chain(_gn_apply_run(cuda, x, sums, gamma, beta, None, None, *a, swish), ref0, bound0, f"ld_groupnorm_apply without zq C={C} W={W} swish={swish}")
    if swish:
        monkeypatch.setenv("LD_GN_FAST_RCP", "0")
        div = _gn_apply_run(cuda, x, sums, gamma, beta, zy, zb, *a, swish)
        kr.check_chain(div, ref, bound, f"ld_groupnorm_apply LD_GN_FAST_RCP=0 C={C} W={W}")
        apart = (div.double() - got.double()).abs()
        print(f"LD_GN_FAST_RCP=0 vs default C={C} W={W}: {int((apart > 0).sum())} of {apart.numel()} elements differ")
        assert bool((apart <= kr._ulp(torch.maximum(div.double().abs(), got.double().abs()))).all()), "more than one bf16 step apart"
