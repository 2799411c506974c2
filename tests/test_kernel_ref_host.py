"""tests/kernel_ref.py on the CPU: for every checker the CPU fp32 restatement of the operation passes, and deliberately wrong
outputs fail -- two patches swapped, the in-patch index transposed, the first-frame rule dropped, one border cell written, the
cond / uncond rows exchanged, one rounding point removed from a chain, 2 % of the elements one bf16 step off.  This is the evidence
that the GPU tests built on these references (test_gpu_elem_kernels.py, test_gpu_norm_forms.py, test_gpu_t5_kernels.py) would
notice a subtly wrong kernel; it costs no GPU time."""
import pytest
import torch
import torch.nn.functional as F

import kernel_ref as kr
from kernel_ref import BF


def _step_off(t, share, seed):
    """t (bf16) with `share` of its elements moved one bf16 step (the next bit pattern: one step away from zero)."""
    g = torch.Generator().manual_seed(seed)
    b = kr.bits(t.clone().contiguous())
    flat = b.view(-1)
    pick = torch.randperm(flat.numel(), generator=g)[:-(-int(share * 1000) * flat.numel() // 1000)]      # exactly that share, rounded up
    flat[pick] += 1
    return b.view(BF)


def _fails(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


# ---- class A ----------------------------------------------------------------------------------------------------------------
def test_patchify_reference_catches_swapped_patches_and_a_transposed_patch_index():
    g = torch.Generator().manual_seed(1)
    B, T, C, H, W, p = 2, 3, 4, 6, 10, 2
    x = torch.randn(B, T, C, H, W, generator=g)
    sem = torch.randn(1, T, C, H, W, generator=g).to(BF)
    want = kr.patchify_ref(x, sem, p)
    assert want.shape == (B, T * 3 * 5, C * 4)
    # the definition, element by element, for a few entries: row (t, ph, pw), column c*p*p + i*p + j
    for b, t, ph, pw, c, i, j in ((0, 0, 0, 0, 0, 0, 1), (1, 2, 2, 4, 3, 1, 0), (0, 1, 1, 3, 2, 1, 1)):
        v = (x[b, t, c, ph * p + i, pw * p + j].to(BF) + sem[0, t, c, ph * p + i, pw * p + j])
        assert want[b, (t * 3 + ph) * 5 + pw, c * 4 + i * 2 + j] == v
    kr.check_bits(want.clone(), want, "patchify")
    swapped = want.clone()
    swapped[0, 7], swapped[0, 8] = want[0, 8], want[0, 7]
    _fails(kr.check_bits, swapped, want, "two patches swapped")
    transposed = want.view(B, -1, C, p, p).transpose(3, 4).reshape(want.shape)
    _fails(kr.check_bits, transposed, want, "i*p + j <-> j*p + i")
    hw = kr.patchify_ref(x.transpose(3, 4).contiguous().view(B, T, C, H, W), sem, p)
    _fails(kr.check_bits, hw, want, "h and w exchanged")
    _fails(kr.check_bits, kr.patchify_ref(x, None, p), want, "sem dropped")
    _fails(kr.check_bits, (x + sem.float()).to(BF).view(B, T, C, 3, p, 5, p).permute(0, 1, 3, 5, 2, 4, 6).reshape(want.shape), want, "sem added in fp32")


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    """Against exact rational arithmetic on values chosen to sit on and next to fp32 rounding boundaries of the sum."""
    from fractions import Fraction
    g = torch.Generator().manual_seed(2)
    a, b, c = (torch.randn(4000, generator=g) for _ in range(3))
    a[:8] = torch.tensor([1 + 2.0 ** -12] * 8)
    b[:8] = torch.tensor([1 + 2.0 ** -12, 1 - 2.0 ** -12, 3.0, 2.0 ** -30, 1.0, -1.0, 2.0 ** 20, 2.0 ** -20])
    c[:8] = torch.tensor([2.0 ** -24, -2.0 ** -24, 2.0 ** -23, 1.0, 2.0 ** -25, 1 + 2.0 ** -23, 1.0, 2.0 ** 24])
    got = kr.fma32(a, b, c)
    for i in list(range(8)) + list(range(8, 4000, 37)):
        exact = Fraction(a[i].item()) * Fraction(b[i].item()) + Fraction(c[i].item())
        f = torch.tensor(float(exact), dtype=torch.float64)          # float(Fraction) is correctly rounded; so is fp64 -> fp32 of a value ...
        lo, hi = f.float(), f.float()
        # ... unless the double rounding matters: take the two fp32 neighbours of the exact value and pick the nearer one exactly
        cand = sorted({torch.nextafter(lo, torch.tensor(float("-inf"))).item(), lo.item(), torch.nextafter(hi, torch.tensor(float("inf"))).item()},
                      key=lambda v: (abs(Fraction(v) - exact), abs(int(torch.tensor(v, dtype=torch.float32).view(torch.int32).item()) & 1)))
        assert got[i].item() == cand[0], (i, got[i].item(), cand)
    unfused = c + a * b
    assert (got != unfused).float().mean() > 0.01                    # the two are different operations on this data


def test_unpatchify_cfg_reference_catches_exchanged_rows_and_index_errors():
    g = torch.Generator().manual_seed(3)
    T, C, H, W, p = 3, 4, 6, 10, 2
    lin = torch.randn(2, T * 3 * 5, C * 4, generator=g).to(BF)
    x = torch.randn(1, T, C, H, W, generator=g)
    want = kr.unpatchify_cfg_ref(lin, x, p, -0.7, 0.7, 6.5)
    t, c, hh, ww = 2, 3, 5, 7
    eu, ec = (lin[r, (t * 3 + hh // 2) * 5 + ww // 2, c * 4 + (hh % 2) * 2 + ww % 2].float() for r in (0, 1))
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    xs = x[0, t, c, hh, ww] * f(0.7)
    du, dc = eu * f(-0.7) + xs, ec * f(-0.7) + xs
    assert want[t, c, hh, ww] == kr.fma32(f(6.5), dc - du, du)
    kr.check_bits(want.clone(), want, "unpatchify_cfg")
    _fails(kr.check_bits, kr.unpatchify_cfg_ref(lin.flip(0), x, p, -0.7, 0.7, 6.5), want, "cond / uncond rows exchanged")
    _fails(kr.check_bits, kr.unpatchify_cfg_ref(lin.view(2, -1, C, p, p).transpose(3, 4).reshape(lin.shape), x, p, -0.7, 0.7, 6.5), want, "patch index transposed")
    _fails(kr.check_bits, kr.unpatchify_cfg_ref(lin, x, p, -0.7, 0.7, 6.5, fused_last=False), want, "unfused last step")
    # scale 1 gives the cond branch up to the rounding of (c - u) + u; the fused and unfused forms agree there (the product is exact)
    one_f, one_u = kr.unpatchify_cfg_ref(lin, x, p, -0.7, 0.7, 1.0), kr.unpatchify_cfg_ref(lin, x, p, -0.7, 0.7, 1.0, fused_last=False)
    kr.check_bits(one_f, one_u, "scale 1: fused == unfused")
    e = lin.float().view(2, T, 3, 5, C, p, p).permute(0, 1, 4, 2, 5, 3, 6).reshape(2, T, C, H, W)
    cond = e[1] * f(-0.7) + x[0] * f(0.7)
    assert ((one_f - cond).abs() <= 2.0 ** -23 * (cond.abs() + (e[0] * f(-0.7) + x[0] * f(0.7)).abs())).all()


def test_axpbypcz_reference_fused_and_unfused_forms():
    g = torch.Generator().manual_seed(4)
    x, y, z = (torch.randn(5000, generator=g) for _ in range(3))
    kr.check_bits(kr.axpbypcz_ref(x, 0.3), torch.tensor(0.3, dtype=torch.float32) * x, "x only")
    fused, eager = kr.axpbypcz_ref(x, 0.3, y, -1.7, z, 0.9), kr.axpbypcz_ref(x, 0.3, y, -1.7, z, 0.9, fused=False)
    _fails(kr.check_bits, fused, eager, "fused vs eager")
    # a rounding of each fused product, and the two partial sums may then each land one ulp apart
    v1 = x.abs() * 0.3 + y.abs() * 1.7
    lim = (y.abs() * 1.7 + z.abs() * 0.9) * 2.0 ** -24 + 2.0 ** -23 * (v1 + fused.abs())
    assert ((fused - eager).abs() <= lim).all()


def test_place_reference_catches_a_dropped_first_frame_rule_and_a_written_border():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 5, 7, 16, generator=g).to(BF)
    up = kr.place_ref(x, 1, 16, time_up=True)
    assert up.shape == (2, 5, 10, 14, 16) and kr.upsample_out_frames(3, True) == 5
    assert torch.equal(up[:, :, 3, 8], x[:, [0, 1, 1, 2, 2], 1, 4])                  # frame 0 single, the rest doubled
    no_rule = x[:, [0, 0, 1, 1, 2]].repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    want = kr.padded_expect(up, 2, 1, 1)
    kr.check_bits(kr.padded_expect(up.clone(), 2, 1, 1), want, "place mode 1")
    _fails(kr.check_bits, kr.padded_expect(no_rule, 2, 1, 1), want, "first-frame rule dropped")
    assert kr.place_ref(x, 1, 16, time_up=False).shape == (2, 3, 10, 14, 16)
    assert kr.place_ref(x[:, :2], 1, 16, time_up=True).shape == (2, 4, 10, 14, 16) and kr.place_ref(x[:, :1], 1, 16, time_up=True).shape == (2, 1, 10, 14, 16)
    border = want.clone()
    border[1, 3, 0, 5, 2] = 0
    _fails(kr.check_bits, border, want, "one border cell written")
    halo = want.clone()
    halo[0, 1, 4, 4, 0] = 0
    _fails(kr.check_bits, halo, want, "one halo-frame cell written")
    # PixelShuffle: out[2h+i][2w+j][c] = in[h][w][c*4 + i*2 + j]
    xs = torch.randn(1, 2, 3, 4, 32, generator=g).to(BF)
    ps = kr.place_ref(xs, 2, 8)
    assert ps.shape == (1, 2, 6, 8, 8) and ps[0, 1, 2 * 2 + 1, 2 * 3 + 0, 5] == xs[0, 1, 2, 3, 5 * 4 + 2]
    pad = kr.place_ref(xs[..., :3], 0, 8)
    assert torch.equal(pad[..., :3], xs[..., :3]) and not bool(pad[..., 3:].any())


def test_to_uint8_reference_on_every_finite_pattern():
    v = kr.finite_bf16_patterns()
    assert v.numel() == 65280 and torch.isfinite(v.float()).all() and kr.bits(v).unique().numel() == 65280
    u8, video = kr.to_uint8_ref(torch.cat([v, torch.tensor([float("inf"), float("-inf"), 0.0]).to(BF)]).view(-1, 3))
    assert u8[-1].tolist() == [255, 0, 127] and video[:, -1].tolist() == [1.0, 0.0, 0.5]
    assert u8.min() == 0 and u8.max() == 255 and len(u8.unique()) == 256


def test_latent_to_cl_reference_layouts():
    g = torch.Generator().manual_seed(6)
    T, C, H, W = 3, 16, 5, 7
    x = torch.randn(T, C, H, W, generator=g)
    a = kr.latent_to_cl_ref(x, T, C, H, W, 64, 1 / 1.15258426, True)
    b = kr.latent_to_cl_ref(x.permute(1, 0, 2, 3).contiguous(), T, C, H, W, 64, 1 / 1.15258426, False)
    assert torch.equal(a, b) and a.shape == (T, H, W, 64) and not bool(a[..., C:].any())
    assert a[2, 4, 6, 5] == (x[2, 5, 4, 6].to(BF) * (1 / 1.15258426))
    _fails(kr.check_bits, kr.latent_to_cl_ref(x, T, C, H, W, 64, 1 / 1.15258426, False), a, "layout flag ignored")
    _fails(kr.check_bits, (x * (1 / 1.15258426)).to(BF).permute(0, 2, 3, 1), a[..., :C], "one rounding instead of two")


# ---- class B ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 7, 64, 512, 1920])
def test_timestep_embedding_checker(dim):
    t = torch.tensor([0.0, 1.0, 17.5, 500.0, 999.0])
    ref, bound, cpu = kr.timestep_embedding_ref(t, dim)
    assert ref.shape == (5, dim) and (dim % 2 == 0 or bool((ref[:, -1] == 0).all()))
    kr.check_abs_rounding(cpu, ref, bound, f"cpu fp32, dim {dim}")
    if dim >= 64:
        _fails(kr.check_abs_rounding, _step_off(cpu, 0.02, dim), ref, bound, "2 % one step off")
        _fails(kr.check_abs_rounding, torch.cat([cpu[:, dim // 2:2 * (dim // 2)], cpu[:, :dim // 2]], dim=1), ref[:, :2 * (dim // 2)], bound[:, :2 * (dim // 2)], "sin || cos")
    if dim % 2:
        wrong = cpu.clone()
        wrong[:, -1] = 2.0 ** -20
        _fails(kr.check_abs_rounding, wrong, ref, bound, "last column of an odd dim not zero")


@pytest.mark.parametrize("D", [64, 520, 2056])
def test_layernorm_checkers(D):
    x, w, b = kr.ln_inputs(9, D, D)
    ref, t32 = kr.layernorm_ref(x, w, b, 1e-5)
    noise = kr.f32_noise(ref, t32)
    kr.check_one_rounding(t32.to(BF), ref, noise, f"cpu fp32 LayerNorm({D})")
    kr.check_f32(t32, ref, t32, f"cpu fp32 LayerNorm({D}), fp32 out")
    _fails(kr.check_one_rounding, _step_off(t32.to(BF), 0.02, D), ref, noise, "2 % one step off")
    _fails(kr.check_one_rounding, F.layer_norm(x.float(), (D,), w.float(), b.float(), 1e-3).to(BF), ref, noise, "another eps")
    _fails(kr.check_f32, F.layer_norm(x.float(), (D,), w.float(), b.float(), 1e-4), ref, t32, "fp32 out, another eps")
    _fails(kr.check_one_rounding, t32.to(BF).roll(8, dims=1), ref, noise, "chunks rotated")
    ref0, t0 = kr.layernorm_ref(x, None, None, 1e-5)
    kr.check_one_rounding(t0.to(BF), ref0, kr.f32_noise(ref0, t0), f"cpu fp32 LayerNorm({D}) without weights")


def _mod_case(rows, D, seed):
    x, w, b = kr.ln_inputs(rows, D, seed)
    g = torch.Generator().manual_seed(seed + 1)
    rpb, tl = 5, 2                                             # rows 0-1 text, 2-4 image, 5-6 text of batch 1, ...
    ada = (0.3 * torch.randn((rows + rpb - 1) // rpb, 4 * D, generator=g)).to(BF)
    shift = kr.modulate_rows(ada, rows, rpb, tl, 0, 2 * D, D)
    scale = kr.modulate_rows(ada, rows, rpb, tl, D, 3 * D, D)
    return x, w, b, ada, shift, scale


def test_ln_modulate_chain_catches_a_removed_rounding_point():
    x, w, b, ada, shift, scale = _mod_case(9, 1920, 7)
    assert torch.equal(shift[1], ada[0, 2 * 1920:3 * 1920].double()) and torch.equal(shift[2], ada[0, :1920].double())          # text / image boundary
    assert torch.equal(scale[5], ada[1, 3 * 1920:].double()) and torch.equal(scale[4], ada[0, 1920:2 * 1920].double())          # batch boundary
    ref, bound = kr.ln_modulate_ref(x, w, b, 1e-5, shift, scale)
    cpu = kr.ln_modulate_cpu32(x, w, b, 1e-5, shift, scale)
    kr.check_chain(cpu, ref, bound, "cpu fp32 LN + modulate")
    for drop in ("ln", "one_plus", "prod"):
        wrong, _ = kr.ln_modulate_ref(x, w, b, 1e-5, shift, scale, drop=drop)
        _fails(kr.check_chain, wrong.to(BF), ref, bound, f"rounding point {drop} removed")
    _fails(kr.check_chain, _step_off(cpu, 0.02, 3), ref, bound, "2 % one step off")
    wrong_rows = kr.ln_modulate_cpu32(x, w, b, 1e-5, shift.roll(1, 0), scale.roll(1, 0))
    _fails(kr.check_chain, wrong_rows, ref, bound, "region boundary one row off")


def test_qkv_split_references():
    g = torch.Generator().manual_seed(8)
    B, N, H, Npad = 2, 70, 3, 128
    qkv = torch.randn(B * N, 3 * H * 64, generator=g).to(BF)
    q, k, v = kr.qkv_thirds(qkv, B, N, H)
    assert q[1, 2, 5, 9] == qkv[N + 5, 2 * 64 + 9] and k[0, 1, 69, 63] == qkv[69, H * 64 + 64 + 63] and v[1, 0, 0, 1] == qkv[N, 2 * H * 64 + 1]
    want = kr.qkv_expect_bits(q.contiguous(), k.contiguous(), v.contiguous(), Npad, 64)
    assert all(t.numel() == B * H * Npad * 64 + 64 for t in want)
    vt = want[2][:-64].view(B, H, 64, Npad)
    assert vt[1, 2, 7, 33] == kr.bits(v.contiguous())[1, 2, 33, 7] and not bool(vt[..., N:].any()) and bool(kr.is_sentinel(want[2][-64:]).all())
    assert not bool(want[0][:-64].view(B, H, Npad, 64)[:, :, N:].any())
    unpadded = want[0].clone()
    unpadded[:-64].view(B, H, Npad, 64)[0, 0, N] = kr.NAN16
    _fails(kr.check_bits, unpadded, want[0], "a padding row left unwritten")
    # QK-LayerNorm and RoPE: the CPU restatement passes, 2 % off and a swapped pair fail
    w, b = (1 + 0.1 * torch.randn(64, generator=g)).to(BF), (0.1 * torch.randn(64, generator=g)).to(BF)
    ref, cpu, noise = kr.qk_layernorm_ref(q, w, b)
    kr.check_one_rounding(cpu, ref, noise, "cpu fp32 QK-LayerNorm")
    _fails(kr.check_one_rounding, _step_off(cpu, 0.02, 1), ref, noise, "2 % one step off")
    ang = torch.rand(N, 32, generator=g) * 6.28
    cos, sin = torch.cos(ang), torch.sin(ang)
    ref, cpu, noise = kr.rope_ref(q, cos, sin)
    assert abs(ref[0, 0, 3, 10].item() - (q[0, 0, 3, 10].double() * cos[3, 5].double() - q[0, 0, 3, 11].double() * sin[3, 5].double()).item()) < 1e-12
    kr.check_one_rounding(cpu, ref, noise, "cpu fp32 RoPE")
    _fails(kr.check_one_rounding, _step_off(cpu, 0.02, 2), ref, noise, "2 % one step off")
    _fails(kr.check_one_rounding, kr.rope_ref(q, cos, -sin)[1], ref, noise, "rotation the other way")
    half = torch.cat([q[..., :32], q[..., 32:]], -1)
    rot_half = torch.cat([half[..., :32].float() * cos - half[..., 32:].float() * sin, half[..., :32].float() * sin + half[..., 32:].float() * cos], -1).to(BF)
    _fails(kr.check_one_rounding, rot_half, ref, noise, "half-split pairs instead of interleaved ones")


@pytest.mark.parametrize("ratio", [1, 2, 4, 8, 3])
def test_nearest_index_rules_agree_for_the_pipelines_ratios(ratio):
    """torch's float-scale rule against the kernel's integer rule: every ratio the pipeline produces (1, 2, 4, 8; 3 is the GPU test's
    non-power-of-two case), every source size up to 90 -- and the odd-T time rule through SpatialNorm3D.forward's own calls."""
    for n_in in range(1, 91):
        assert torch.equal(kr.nearest_index_torch(n_in * ratio, n_in), kr.nearest_index_int(n_in * ratio, n_in)), (n_in, ratio)
    g = torch.Generator().manual_seed(ratio)
    for Tz in (1, 2, 3, 4):
        for T in ({1 + 2 * (Tz - 1), 1 + 4 * (Tz - 1), Tz} | ({2 * Tz, 4 * Tz})):
            if T < Tz:
                continue
            z = torch.randn(Tz, 2, 3, 8, generator=g).to(BF)
            assert torch.equal(kr.zq_gather_torch(z, T, 2 * ratio, 3 * ratio), kr.zq_gather_int(z, T, 2 * ratio, 3 * ratio)), (Tz, T, ratio)


def test_nearest_index_rules_differ_elsewhere():
    """Why the tests keep to those ratios: torch's float scale is not the exact integer division everywhere."""
    assert not torch.equal(kr.nearest_index_torch(82, 2), kr.nearest_index_int(82, 2))
    assert not torch.equal(kr.nearest_index_torch(123, 3), kr.nearest_index_int(123, 3))


def _gn_case(Fn, T, H, W, C, G, zs, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(Fn * T, H, W, C, generator=g) * 1.5 + 0.3).to(BF)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).to(BF), (0.2 * torch.randn(C, generator=g)).to(BF)
    zy = zb = None
    if zs:
        zy, zb = torch.randn(*zs, C, generator=g).to(BF), torch.randn(*zs, C, generator=g).to(BF)
    sums, _ = kr.gn_sums_ref(x, Fn, T * H * W, C, G)
    return x, gamma, beta, zy, zb, sums


def test_groupnorm_chain_catches_removed_roundings_and_a_dropped_first_frame_rule():
    Fn, T, H, W, C, G = 2, 3, 6, 12, 64, 32
    x, gamma, beta, zy, zb, sums = _gn_case(Fn, T, H, W, C, G, (2, 3, 3), 9)
    zyg, zbg = kr.zq_gather_torch(zy, T, H, W), kr.zq_gather_torch(zb, T, H, W)
    assert torch.equal(zyg, kr.zq_gather_int(zy, T, H, W))
    a = (Fn, T, H, W, C, G, 1e-6)
    ref, bound = kr.gn_apply_ref(x, sums, gamma, beta, *a, zy=zyg, zb=zbg)
    cpu = kr.gn_apply_cpu32(x, sums, gamma, beta, *a, zy=zyg, zb=zbg)
    kr.check_chain(cpu, ref, bound, "cpu fp32 GN + SpatialNorm + swish")
    for drop in ("gn", "prod", "sig"):
        wrong, _ = kr.gn_apply_ref(x, sums, gamma, beta, *a, zy=zyg, zb=zbg, drop=drop)
        _fails(kr.check_chain, wrong.to(BF), ref, bound, f"rounding point {drop} removed")
    _fails(kr.check_chain, _step_off(cpu, 0.02, 4), ref, bound, "2 % one step off")
    no_rule = kr.gn_apply_cpu32(x, sums, gamma, beta, *a, zy=kr.zq_gather_int(zy, T, H, W, False), zb=kr.zq_gather_int(zb, T, H, W, False))
    _fails(kr.check_chain, no_rule, ref, bound, "first-frame rule dropped")
    _fails(kr.check_chain, kr.gn_apply_cpu32(x, sums.flip(0), gamma, beta, *a, zy=zyg, zb=zbg), ref, bound, "statistics of the other frame group")
    ref_ns, bound_ns = kr.gn_apply_ref(x, sums, gamma, beta, *a, swish=False)
    kr.check_chain(kr.gn_apply_cpu32(x, sums, gamma, beta, *a, swish=False), ref_ns, bound_ns, "cpu fp32 GN alone")
    want, scale = kr.gn_sums_ref(x, Fn, T * H * W, C, G)
    assert want.shape == (Fn, G, 2) and abs(want[1, 3, 0].item() - x.double().view(Fn, -1, C)[1, :, 6:8].sum().item()) < 1e-9


@pytest.mark.parametrize("D", [64, 4096])
def test_t5_rmsnorm_chain(D):
    from transformers.models.t5.modeling_t5 import T5LayerNorm
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(5, D, generator=g) * 2).to(BF)
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(BF)
    ref, bound = kr.t5_rmsnorm_ref(x, w, 1e-6)
    hf = T5LayerNorm(D, eps=1e-6).to(BF)
    with torch.no_grad():
        hf.weight.copy_(w)
        out_hf = hf(x)
    assert out_hf.dtype == BF and torch.equal(out_hf, kr.t5_rmsnorm_cpu32(x, w, 1e-6))
    kr.check_chain(out_hf, ref, bound, f"HF T5LayerNorm({D}) in bf16 on the CPU")
    _fails(kr.check_chain, kr.t5_rmsnorm_ref(x, w, 1e-6, drop="inner")[0].to(BF), ref, bound, "inner rounding removed")
    _fails(kr.check_chain, _step_off(out_hf, 0.02, 5), ref, bound, "2 % one step off")
    xd = x.float()
    centred = (w.float() * ((xd - xd.mean(-1, keepdim=True)) * torch.rsqrt(xd.var(-1, unbiased=False, keepdim=True) + 1e-6)).to(BF)).to(BF)
    _fails(kr.check_chain, centred, ref, bound, "a LayerNorm instead of an RMS norm")


@pytest.mark.parametrize("N", [5, 65])
def test_t5_attention_chain(N):
    from landiff_amd.t5 import relative_buckets
    H = 2
    q, k, v, table = kr.t5_exact_operands(N, H, 32, N)
    bucket = relative_buckets(N)
    ref, bound = kr.t5_attn_ref(q, k, v, table, bucket)
    cpu = kr.t5_attn_cpu32(q, k, v, table, bucket)
    kr.check_chain(cpu, ref, bound, f"cpu T5 attention N={N}")
    _fails(kr.check_chain, kr.t5_attn_ref(q, k, v, table, bucket, drop="prob")[0].to(BF), ref, bound, "probabilities left unrounded")
    _fails(kr.check_chain, _step_off(cpu, 0.02, 6), ref, bound, "2 % one step off")
    _fails(kr.check_chain, kr.t5_attn_cpu32(q, k, v, table, bucket.flip(0)), ref, bound, "bias of key i seen from query j")
    _fails(kr.check_chain, kr.t5_attn_cpu32(q, k, v, table.flip(1), bucket), ref, bound, "the other head's bias column")
    scaled = kr.t5_attn_cpu32((q.float() * 0.125).to(BF), k, v, table, bucket)
    _fails(kr.check_chain, scaled, ref, bound, "scores scaled by 1/sqrt(d)")
    with pytest.raises(AssertionError, match="premise"):
        kr.t5_attn_ref((q.float() * 0.3).to(BF), k, v, table, bucket)
